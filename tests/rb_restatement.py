"""NumPy restatement of the Rao-Blackwellised filter kernel (bayesian_dlms_amd/csrc/dlm_rb.hip, dlm_rb_batch), operation for operation and in
the kernel's orders of summation, vectorised over the series of a batch.  The sums over the particles, the running sums
of the two resampling searches, the Gaussian density, Philox and the addressing of the draws are tests/pf_restatement.py's, the moments of a
log-variance row and the search tests/lw_restatement.py's, by import.

Every particle carries (m [d], C [d][d], psi [d + 1]).  C is kept here as a full matrix whose two triangles are equal bit for bit; the kernel
keeps the lower one.  The orders:

  g = G^T F:        g_a = F_0 G_0a + F_1 G_1a + ...                       (F itself without an advance)
  predict:          cg_a = C_a0 g_0 + C_a1 g_1 + ...,  f = g_0 m_0 + ...,  s = g_0 cg_0 + ..., then + (F_k F_k) (dt exp psi_k) for k = 0 ..
  R = G C G^T:      per row r:  u_b = G_r0 C_0b + G_r1 C_1b + ...,  R_rc = u_0 G_c0 + u_1 G_c1 + ... (c <= r), the diagonal + dt exp psi_r
  the Kalman update (Joseph form with the products against I - K F^T written out):
                    rf_r = R_r0 F_0 + ...,  K = rf / Q;  per row r:  k_r = rf_r / Q,  m_r += k_r e,  B_rb = R_rb - k_r rf_b,
                    bf = B_r0 F_0 + ...,  C'_rc = (B_rc - bf K_c) + (v k_r) K_c (c <= r)

The draws: Philox4x32-10 under the key DLM_KEY_RB | block (dlm_draws.h), counter (series, iteration, slot * 2048 + particle * 2): block 0 the
uniform of the second stage's resampling, block 1 the uniform of the first (auxiliary) stage's, block 2 + q the pair of the log-variances 2 q
and 2 q + 1; slot t for step t, SLOT_INIT for the initial log-variances.  There are no state draws.

`run` also returns the margins and resample_share of tests/lw_restatement.py."""
import numpy as np

from lw_restatement import ancestors, moments
from pf_restatement import GAUSSIAN, ST_NONFINITE, ST_NOT_PD, _per_series, batch_rand, log_density, normal, particle_sum, running_sums  # noqa: F401

KEY_RB = 0x52420000
BLOCK_RESAMPLE, BLOCK_FIRST, BLOCK_PARAM = 0, 1, 2
SLOT_INIT = 0x1FFFFF


def tri(d):
    """the (r, c) of the packed lower triangle by rows"""
    return [(r, c) for r in range(d) for c in range(r + 1)]


def pack(C):
    """C [N][d][d][P] -> [N][d(d+1)/2][P]"""
    return np.stack([C[:, r, c] for r, c in tri(C.shape[1])], axis=1)


def predict(m, C, psi, gf, F, adv, dte):
    """(f, s) [N][P] each: the predictive mean and the predictive variance without the observation's"""
    d = m.shape[1]
    fa = sa = None
    for a in range(d):
        cg = C[:, a, 0] * gf[0]
        for b in range(1, d):
            cg = cg + C[:, a, b] * gf[b]
        fa = gf[a] * m[:, a] if a == 0 else fa + gf[a] * m[:, a]
        sa = gf[a] * cg if a == 0 else sa + gf[a] * cg
    if adv:
        for k in range(d):
            sa = sa + (F[k] * F[k]) * (dte * np.exp(psi[:, k]))
    return fa, sa


def advance_mean(Gt, m):
    d = m.shape[1]
    out = np.empty_like(m)
    for r in range(d):
        gx = Gt[r, 0] * m[:, 0]
        for c in range(1, d):
            gx = gx + Gt[r, c] * m[:, c]
        out[:, r] = gx
    return out


def predict_cov(Gt, C, psi, dte):
    d = C.shape[1]
    R = np.empty_like(C)
    for r in range(d):
        u = [Gt[r, 0] * C[:, 0, b] for b in range(d)]
        for a in range(1, d):
            u = [u[b] + Gt[r, a] * C[:, a, b] for b in range(d)]
        for c in range(r + 1):
            acc = u[0] * Gt[c, 0]
            for b in range(1, d):
                acc = acc + u[b] * Gt[c, b]
            if c == r:
                acc = acc + dte * np.exp(psi[:, r])
            R[:, r, c] = acc
            R[:, c, r] = acc
    return R


def update(R, F, Q, v, e, m):
    """(m', C') of the Kalman update; m holds a"""
    d = m.shape[1]
    rf = []
    for r in range(d):
        acc = R[:, r, 0] * F[0]
        for c in range(1, d):
            acc = acc + R[:, r, c] * F[c]
        rf.append(acc)
    K = [rf[r] / Q for r in range(d)]
    mn, Cn = np.empty_like(m), np.empty_like(R)
    for r in range(d):
        kr = rf[r] / Q
        mn[:, r] = m[:, r] + kr * e
        row = [R[:, r, b] - kr * rf[b] for b in range(d)]
        bf = row[0] * F[0]
        for b in range(1, d):
            bf = bf + row[b] * F[b]
        vk = v * kr
        for c in range(r + 1):
            val = (row[c] - bf * K[c]) + vk * K[c]
            Cn[:, r, c] = val
            Cn[:, c, r] = val
    return mn, Cn


def run(*, F, G, g_index, dt, V, m0, C0, y, P, a, prior_w, prior_v=None, learn_v=True, n0=-1, literal=False, seed=0, series_offset=0,
        iteration=0, **unused):
    """F [d] or [T][d]; G [n_g][d][d] (row, column); g_index [T] or None; dt [T] or None; V scalar or [N] (read without learn_v); C0 [d][d] or
    [N][d][d] (the lower triangle is read); m0 [d] or [N][d]; prior_w [d][2] or [N][d][2] (mean, sd of log W_kk); prior_v [2] or [N][2]; y [N][T]
    (NaN = missing); a the shrinkage.  Returns a dict: ll [N], mean [N][T][d], cov [N][T][d][d], ess [N][T], psi_mean, psi_var [N][T][d+1],
    means [N][d][P], covs [N][d(d+1)/2][P], weights [N][P], psi [N][d+1][P], status [N], the margins and resample_share."""
    y = np.asarray(y, dtype=np.float64)
    N, T = y.shape
    G = np.asarray(G, dtype=np.float64)
    d = G.shape[1]
    F = np.asarray(F, dtype=np.float64)
    learn_v = bool(learn_v)
    assert 0.0 < a <= 1.0
    V = None if learn_v else np.broadcast_to(np.asarray(V, dtype=np.float64), (N,)).copy()
    C0, m0 = _per_series(C0, N, (d, d)), _per_series(m0, N, (d,))
    rows = d + (1 if learn_v else 0)
    pr = _per_series(prior_w, N, (d, 2))
    if learn_v:
        pr = np.concatenate([pr, _per_series(prior_v, N, (2,))[:, None, :]], axis=1)          # [N][rows][2]
    n0 = P // 5 if n0 < 0 else n0
    series = np.uint64(series_offset) + np.arange(N, dtype=np.uint64)
    rP = 1.0 / P
    shrink, keep, h = a, 1.0 - a, np.sqrt(1.0 - a * a)

    status = np.zeros(N, dtype=np.int32)
    ll = np.zeros(N)
    mean = np.full((N, T, d), np.nan)
    cov = np.full((N, T, d, d), np.nan)
    pmean = np.full((N, T, d + 1), np.nan)
    pvar = np.full((N, T, d + 1), np.nan)
    ess = np.full((N, T), np.nan)
    with np.errstate(invalid="ignore"):
        ok0 = np.all(np.isfinite(pr[:, :, 0]) & (pr[:, :, 1] >= 0.0), axis=1)
    status[~ok0] = ST_NOT_PD
    alive = ok0.copy()
    learned = pr[:, :, 1] > 0.0          # [N][rows]
    m = np.repeat(m0[:, :, None], P, axis=2)
    low = np.tril(np.ones((d, d), dtype=bool))
    C0s = np.where(low, C0, np.swapaxes(C0, 1, 2))          # the lower triangle, mirrored
    C = np.repeat(C0s[:, :, :, None], P, axis=3)
    with np.errstate(all="ignore"):
        psi = np.empty((N, rows, P))
        for r in range(rows):
            zp = normal(KEY_RB, seed, series, iteration, SLOT_INIT, P, BLOCK_PARAM, r) if learned[:, r].any() else 0.0
            psi[:, r] = np.where(learned[:, r, None], pr[:, r, 0, None] + pr[:, r, 1, None] * zp, pr[:, r, 0, None])
    wg = np.full((N, P), rP)
    hs = np.zeros((N, rows))
    ess_last = np.full(N, float(P))
    first = np.ones(N, dtype=bool)
    mg = dict(margin_search=np.inf, margin_n0=np.inf, margin_int=np.inf)
    observed_steps = resampled_steps = 0

    def outputs(t, who):
        mu = [particle_sum(wg * m[:, k]) for k in range(d)]
        for k in range(d):
            mean[who, t, k] = mu[k][who]
        for r, c in tri(d):
            s = particle_sum(wg * (C[:, r, c] + (m[:, r] - mu[r][:, None]) * (m[:, c] - mu[c][:, None])))
            cov[who, t, r, c] = s[who]
            cov[who, t, c, r] = s[who]
        for k in range(rows):
            pm, v = moments(psi[:, k], wg)
            pmean[who, t, k], pvar[who, t, k] = pm[who], v[who]

    def fail(who, qf):
        """who: the series that fail in this step; qf: their Q flags (2: not positive, 1: not finite)"""
        status[who] = np.where((qf[who] == 2.0) & first[who], ST_NOT_PD, ST_NONFINITE)

    def q_flag(Q):
        return np.where(~(Q > 0.0), 2.0, np.where(Q < np.inf, 0.0, 1.0)).max(axis=1)

    def obs_v(psi_now):
        return np.exp(psi_now[:, d]) if learn_v else V[:, None]

    def where3(who, new, old):
        return np.where(who.reshape((N,) + (1,) * (new.ndim - 1)), new, old)

    with np.errstate(all="ignore"):
        for t in range(T):
            yt = y[:, t]
            missing = np.isnan(yt)
            dte = 1.0 if dt is None else float(dt[t])
            adv = dte != 0.0
            Gt = G[0 if g_index is None else g_index[t]]
            Ft = F if F.ndim == 1 else F[t]
            mis = alive & missing
            if mis.any():
                if adv:
                    C = where3(mis, predict_cov(Gt, C, psi, dte), C)
                    m = where3(mis, advance_mean(Gt, m), m)
                outputs(t, mis)
                ess[mis, t] = ess_last[mis]
            obs = alive & ~missing
            if not obs.any():
                continue
            # -- g = G^T F, the kernel moments and the shrinkage, in place
            if adv:
                gf = []
                for c in range(d):
                    g = Ft[0] * Gt[0, c]
                    for r in range(1, d):
                        g = g + Ft[r] * Gt[r, c]
                    gf.append(g)
            else:
                gf = [Ft[c] for c in range(d)]
            for k in range(rows):
                row = psi[:, k]
                pbar, s2 = moments(row, wg)
                if literal:
                    mu0 = particle_sum(row) / float(P)
                    e = row - mu0[:, None]
                    s2 = particle_sum(e * e) / float(P - 1)
                do = obs & learned[:, k]
                psi[:, k] = np.where(do[:, None], shrink * row + keep * pbar[:, None], row)
                hs[:, k] = np.where(do, h * np.sqrt(s2), hs[:, k])
            # -- the look-ahead
            f, s = predict(m, C, psi, gf, Ft, adv, dte)
            v = obs_v(psi)
            Q = np.broadcast_to(v, s.shape) if literal else s + v
            qf = q_flag(Q)
            lam = log_density(GAUSSIAN, yt[:, None], f, Q)
            lam = np.where(obs[:, None], lam, -np.inf)
            m1 = np.fmax.reduce(np.concatenate([np.full((N, 1), -np.inf), lam], axis=1), axis=1)
            bad = obs & ((qf != 0.0) | ~np.isfinite(m1))
            fail(bad, qf)
            alive &= ~bad
            obs &= ~bad
            om = wg * np.exp(lam - m1[:, None])
            A = particle_sum(om)
            bad = obs & ~((A > 0.0) & (A < np.inf))
            fail(bad, np.zeros(N))
            alive &= ~bad
            obs &= ~bad
            if not obs.any():
                continue
            ll = np.where(obs, ll + (m1 + np.log(A)), ll)
            cum = running_sums(om)
            _, u2 = batch_rand(KEY_RB | BLOCK_FIRST, seed, series, iteration, t, P)
            target = u2 * cum[:, P - 1, None]
            anc = ancestors(cum, target, obs, mg)
            lam_anc = np.take_along_axis(lam, anc, axis=1)
            m = where3(obs, np.take_along_axis(m, anc[:, None, :], axis=2), m)
            C = where3(obs, np.take_along_axis(C, anc[:, None, None, :], axis=3), C)
            psi = where3(obs, np.take_along_axis(psi, anc[:, None, :], axis=2), psi)
            # -- propagate
            pn = psi.copy()
            for r in range(rows):
                if learned[:, r].any():
                    zp = normal(KEY_RB, seed, series, iteration, t, P, BLOCK_PARAM, r)
                    pn[:, r] = np.where(learned[:, r, None], psi[:, r] + hs[:, r, None] * zp, psi[:, r])
            f, s = predict(m, C, pn, gf, Ft, adv, dte)
            v = np.broadcast_to(obs_v(pn), s.shape)
            Q = s + v
            qf = q_flag(Q)
            l = log_density(GAUSSIAN, yt[:, None], f, Q)
            if not literal:
                l = l - lam_anc
            l = np.where(obs[:, None], l, -np.inf)
            if adv:
                R, am = predict_cov(Gt, C, pn, dte), advance_mean(Gt, m)
            else:
                R, am = C, m
            mn, Cn = update(R, Ft, Q, v, yt[:, None] - f, am)
            m2 = np.fmax.reduce(np.concatenate([np.full((N, 1), -np.inf), l], axis=1), axis=1)
            bad = obs & ((qf != 0.0) | ~np.isfinite(m2))
            fail(bad, qf)
            alive &= ~bad
            obs &= ~bad
            w = np.exp(l - m2[:, None])
            B = particle_sum(w)
            first = first & ~obs
            bad = obs & ~((B > 0.0) & (B < np.inf))
            fail(bad, np.zeros(N))
            alive &= ~bad
            obs &= ~bad
            if not obs.any():
                continue
            m, C, psi = where3(obs, mn, m), where3(obs, Cn, C), where3(obs, pn, psi)
            ll = np.where(obs, ll + (m2 + np.log(B / float(P))), ll)
            wg = np.where(obs[:, None], w / B[:, None], wg)
            sq = particle_sum(wg * wg)
            outputs(t, obs)
            e = np.floor(1.0 / sq)
            ess_last = np.where(obs, e, ess_last)
            ess[obs, t] = e[obs]
            inv = 1.0 / sq
            mg["margin_n0"] = min(mg["margin_n0"], float(np.abs(inv[obs] - n0).min()))
            rounded = obs & ~np.all(w == 1.0, axis=1)          # weights that are all exp(0): 1 / sum W^2 has no rounding to be near an integer by
            if rounded.any():
                mg["margin_int"] = min(mg["margin_int"], float(np.abs(inv[rounded] - np.round(inv[rounded])).min()))
            res = obs & (e < float(n0))
            observed_steps += int(obs.sum())
            resampled_steps += int(res.sum())
            if not res.any():
                continue
            cum = running_sums(wg)
            _, u2 = batch_rand(KEY_RB | BLOCK_RESAMPLE, seed, series, iteration, t, P)
            target = u2 * cum[:, P - 1, None]
            anc = ancestors(cum, target, res, mg)
            m = where3(res, np.take_along_axis(m, anc[:, None, :], axis=2), m)
            C = where3(res, np.take_along_axis(C, anc[:, None, None, :], axis=3), C)
            psi = where3(res, np.take_along_axis(psi, anc[:, None, :], axis=2), psi)
            wg = np.where(res[:, None], rP, wg)

    dead = status != 0
    ll[dead] = -np.inf
    means, covs, weights = m.copy(), pack(C), wg.copy()
    psi_out = np.concatenate([psi, np.full((N, d + 1 - rows, P), np.nan)], axis=1)
    for arr in (means, covs, weights, psi_out):
        arr[dead] = np.nan
    return dict(ll=ll, mean=mean, cov=cov, ess=ess, psi_mean=pmean, psi_var=pvar, means=means, covs=covs, weights=weights, psi=psi_out,
                status=status, resample_share=(resampled_steps / observed_steps if observed_steps else float("nan")), **mg)
