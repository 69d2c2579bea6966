"""NumPy restatement of the Liu-West filter kernel (bayesian_dlms_amd/csrc/dlm_lw.hip, dlm_lw_batch), operation for operation and in the
kernel's orders of summation, vectorised over the series of a batch.  The sums over the particles, the running sums of
the two resampling searches, the Cholesky factor, the densities, Philox and the addressing of the draws are tests/pf_restatement.py's, by import.

The draws: Philox4x32-10 under the key DLM_KEY_LW | block (dlm_draws.h), counter (series, iteration, slot * 2048 + particle * 2): block
q < 8 the Box-Muller pair of the state components 2 q and 2 q + 1, block 8 the uniform of the second stage's resampling, block 9 the uniform
of the first (auxiliary) stage's, block 10 + q the pair of the log-variances 2 q and 2 q + 1 (k < d: log W_kk, k = d: log V); slot t for
step t, SLOT_INIT for the initial cloud.

`run` also returns the smallest MARGINS of every data-dependent decision of the kernel on its inputs: margin_search (both searches),
margin_n0 and margin_int as tests/pf_restatement.py defines them, and the share of observed steps whose SECOND stage resampled (the first
always does)."""
import numpy as np

from pf_restatement import (BETA, GAUSSIAN, ST_NONFINITE, ST_NOT_PD, STUDENTT, _per_series, batch_rand, cholesky, log_density,  # noqa: F401
                            matvec_lower, normal, particle_sum, running_sums)

KEY_LW = 0x4C570000
BLOCK_RESAMPLE, BLOCK_FIRST, BLOCK_PARAM = 8, 9, 10
SLOT_INIT = 0x1FFFFF


def moments(row, wg):
    """(sum W row, sum W (row - mean)^2), the second in a pass of its own: [N] each"""
    mean = particle_sum(wg * row)
    e = row - mean[:, None]
    return mean, particle_sum(wg * (e * e))


def ancestors(cum, target, who, mg):
    """cum, target [N][P] -> for every series the first j with cum[j] > target (P - 1 when none is), all series at once: the running maxima
    and the targets of a series are sorted together (stable: a maximum equal to a target comes first, so it counts as not exceeding it), and
    a target's ancestor is the number of maxima before it.  Records the search margin of the series in `who`."""
    N, P = cum.shape
    top = np.maximum.accumulate(cum, axis=1)
    order = np.argsort(np.concatenate([top, target], axis=1), axis=1, kind="stable")
    is_top = order < P
    before = np.cumsum(is_top, axis=1)
    r, c = np.nonzero(~is_top)
    anc = np.empty((N, P), dtype=np.int64)
    anc[r, order[r, c] - P] = before[r, c]
    anc = np.minimum(anc, P - 1)
    at, below = np.take_along_axis(cum, anc, axis=1), np.take_along_axis(cum, np.maximum(anc - 1, 0), axis=1)
    near = np.minimum(np.abs(target - at), np.abs(target - below)) / cum[:, P - 1, None]
    if np.any(who):
        mg["margin_search"] = min(mg["margin_search"], float(near[who].min()))
    return anc


def run(*, F, G, g_index, dt, V, m0, C0, y, family, P, a, prior_w, prior_v=None, learn_v=None, n0=-1, literal=False, nu=None, seed=0,
        series_offset=0, iteration=0, **unused):
    """F [d] or [T][d]; G [n_g][d][d] (row, column); g_index [T] or None; dt [T] or None; V scalar or [N] (read without learn_v); C0 [d][d] or
    [N][d][d]; m0 [d] or [N][d]; prior_w [d][2] or [N][d][2] (mean, sd of log W_kk); prior_v [2] or [N][2]; y [N][T] (NaN = missing); nu scalar
    or [N]; a the shrinkage.  Returns a dict: ll [N], mean [N][T][d], ess [N][T], psi_mean, psi_var [N][T][d+1], cloud [N][d][P], weights
    [N][P], psi [N][d+1][P], status [N], the margins and resample_share."""
    y = np.asarray(y, dtype=np.float64)
    N, T = y.shape
    G = np.asarray(G, dtype=np.float64)
    d = G.shape[1]
    F = np.asarray(F, dtype=np.float64)
    learn_v = family in (GAUSSIAN, STUDENTT, BETA) if learn_v is None else bool(learn_v)
    assert not learn_v or family in (GAUSSIAN, STUDENTT, BETA)
    assert 0.0 < a <= 1.0
    V = None if learn_v else np.broadcast_to(np.asarray(V, dtype=np.float64), (N,)).copy()
    C0, m0 = _per_series(C0, N, (d, d)), _per_series(m0, N, (d,))
    rows = d + (1 if learn_v else 0)
    pr = _per_series(prior_w, N, (d, 2))
    if learn_v:
        pr = np.concatenate([pr, _per_series(prior_v, N, (2,))[:, None, :]], axis=1)          # [N][rows][2]
    nu = None if nu is None else np.broadcast_to(np.asarray(nu, dtype=np.float64), (N,)).copy()
    nuc = None if nu is None else nu[:, None]
    n0 = P // 5 if n0 < 0 else n0
    series = np.uint64(series_offset) + np.arange(N, dtype=np.uint64)
    rP = 1.0 / P
    shrink, keep, h = a, 1.0 - a, np.sqrt(1.0 - a * a)

    status = np.zeros(N, dtype=np.int32)
    ll = np.zeros(N)
    mean = np.full((N, T, d), np.nan)
    pmean = np.full((N, T, d + 1), np.nan)
    pvar = np.full((N, T, d + 1), np.nan)
    ess = np.full((N, T), np.nan)
    L0, ok0 = cholesky(C0)
    with np.errstate(invalid="ignore"):
        ok0 &= np.all(np.isfinite(pr[:, :, 0]) & (pr[:, :, 1] >= 0.0), axis=1)
    status[~ok0] = ST_NOT_PD
    alive = ok0.copy()
    learned = pr[:, :, 1] > 0.0          # [N][rows]
    with np.errstate(all="ignore"):
        z = np.stack([normal(KEY_LW, seed, series, iteration, SLOT_INIT, P, 0, c) for c in range(d)], axis=1)
        x = m0[:, :, None] + matvec_lower(L0, z)
        psi = np.empty((N, rows, P))
        for r in range(rows):
            zp = normal(KEY_LW, seed, series, iteration, SLOT_INIT, P, BLOCK_PARAM, r) if learned[:, r].any() else 0.0
            psi[:, r] = np.where(learned[:, r, None], pr[:, r, 0, None] + pr[:, r, 1, None] * zp, pr[:, r, 0, None])
    wg = np.full((N, P), rP)
    hs = np.zeros((N, rows))
    cloud_at_failure = {}
    ess_last = np.full(N, float(P))
    mg = dict(margin_search=np.inf, margin_n0=np.inf, margin_int=np.inf)
    observed_steps = resampled_steps = 0

    def outputs(t, who):
        for k in range(d):
            mean[who, t, k] = particle_sum(wg * x[:, k])[who]
        for k in range(rows):
            m, v = moments(psi[:, k], wg)
            pmean[who, t, k], pvar[who, t, k] = m[who], v[who]

    def fail(who):
        for n in np.nonzero(who)[0]:
            status[n] = ST_NONFINITE
            cloud_at_failure[n] = x[n].copy()

    def Gx(Gt, xs, r):
        gx = Gt[r, 0] * xs[:, 0]
        for c in range(1, d):
            gx = gx + Gt[r, c] * xs[:, c]
        return gx

    def obs_v(row):
        return np.exp(row) if learn_v else V[:, None]

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
                    xn = x.copy()
                    for r in range(d):
                        xn[:, r] = Gx(Gt, x, r) + np.sqrt(dte * np.exp(psi[:, r])) * normal(KEY_LW, seed, series, iteration, t, P, 0, r)
                    x = np.where(mis[:, None, None], xn, x)
                outputs(t, mis)
                ess[mis, t] = ess_last[mis]
            obs = alive & ~missing
            if not obs.any():
                continue
            # -- the kernel moments and the shrinkage, in place
            for k in range(rows):
                row = psi[:, k]
                pbar, s2 = moments(row, wg)
                if literal:
                    mu = particle_sum(row) / float(P)
                    e = row - mu[:, None]
                    s2 = particle_sum(e * e) / float(P - 1)
                do = obs & learned[:, k]
                psi[:, k] = np.where(do[:, None], shrink * row + keep * pbar[:, None], row)
                hs[:, k] = np.where(do, h * np.sqrt(s2), hs[:, k])
            # -- the look-ahead
            eta = None
            for r in range(d):
                gx = Gx(Gt, x, r) if adv else x[:, r]
                eta = Ft[0] * gx if r == 0 else eta + Ft[r] * gx
            lam = log_density(family, yt[:, None], eta, obs_v(psi[:, d] if learn_v else None), nuc, literal)
            lam = np.where(obs[:, None], lam, -np.inf)
            m1 = np.fmax.reduce(np.concatenate([np.full((N, 1), -np.inf), lam], axis=1), axis=1)
            bad = obs & ~np.isfinite(m1)
            om = wg * np.exp(lam - m1[:, None])
            A = particle_sum(om)
            bad |= obs & ~((A > 0.0) & (A < np.inf))
            fail(bad)
            alive &= ~bad
            obs &= ~bad
            if not obs.any():
                continue
            ll = np.where(obs, ll + (m1 + np.log(A)), ll)
            cum = running_sums(om)
            _, u2 = batch_rand(KEY_LW | BLOCK_FIRST, seed, series, iteration, t, P)
            target = u2 * cum[:, P - 1, None]
            anc = ancestors(cum, target, obs, mg)
            lam_anc = np.take_along_axis(lam, anc, axis=1)
            x = np.where(obs[:, None, None], np.take_along_axis(x, anc[:, None, :], axis=2), x)
            psi = np.where(obs[:, None, None], np.take_along_axis(psi, anc[:, None, :], axis=2), psi)
            # -- propagate
            xn = x.copy()
            pn = psi.copy()
            eta = None
            for r in range(rows):
                if learned[:, r].any():          # (a row nobody learns takes no draw: the kernel draws none, and Philox is what this file's time goes to)
                    zp = normal(KEY_LW, seed, series, iteration, t, P, BLOCK_PARAM, r)
                    pn[:, r] = np.where(learned[:, r, None], psi[:, r] + hs[:, r, None] * zp, psi[:, r])
                if r < d:
                    if adv:
                        xn[:, r] = Gx(Gt, x, r) + np.sqrt(dte * np.exp(pn[:, r])) * normal(KEY_LW, seed, series, iteration, t, P, 0, r)
                    eta = Ft[0] * xn[:, r] if r == 0 else eta + Ft[r] * xn[:, r]
            x = np.where(obs[:, None, None], xn, x)
            psi = np.where(obs[:, None, None], pn, psi)
            l = log_density(family, yt[:, None], eta, obs_v(pn[:, d] if learn_v else None), nuc, literal)
            if not literal:
                l = l - lam_anc
            l = np.where(obs[:, None], l, -np.inf)
            m2 = np.fmax.reduce(np.concatenate([np.full((N, 1), -np.inf), l], axis=1), axis=1)
            bad = obs & ~np.isfinite(m2)
            w = np.exp(l - m2[:, None])
            B = particle_sum(w)
            bad |= obs & ~((B > 0.0) & (B < np.inf))
            fail(bad)
            alive &= ~bad
            obs &= ~bad
            if not obs.any():
                continue
            ll = np.where(obs, ll + (m2 + np.log(B / float(P))), ll)
            wg = np.where(obs[:, None], w / B[:, None], wg)
            sq = particle_sum(wg * wg)
            outputs(t, obs)
            e = np.floor(1.0 / sq)
            ess_last = np.where(obs, e, ess_last)
            ess[obs, t] = e[obs]
            inv = (1.0 / sq)[obs]
            mg["margin_n0"] = min(mg["margin_n0"], float(np.abs(inv - n0).min()))
            mg["margin_int"] = min(mg["margin_int"], float(np.abs(inv - np.round(inv)).min()))
            res = obs & (e < float(n0))
            observed_steps += int(obs.sum())
            resampled_steps += int(res.sum())
            if not res.any():
                continue
            cum = running_sums(wg)
            _, u2 = batch_rand(KEY_LW | BLOCK_RESAMPLE, seed, series, iteration, t, P)
            target = u2 * cum[:, P - 1, None]
            anc = ancestors(cum, target, res, mg)
            x = np.where(res[:, None, None], np.take_along_axis(x, anc[:, None, :], axis=2), x)
            psi = np.where(res[:, None, None], np.take_along_axis(psi, anc[:, None, :], axis=2), psi)
            wg = np.where(res[:, None], rP, wg)

    dead = status != 0
    ll[dead] = -np.inf
    cloud = x.copy()
    weights = wg.copy()
    psi_out = np.concatenate([psi, np.full((N, d + 1 - rows, P), np.nan)], axis=1)
    weights[dead] = np.nan
    psi_out[dead] = np.nan
    for n in np.nonzero(dead)[0]:
        if status[n] & ST_NOT_PD:
            cloud[n] = np.nan
            mean[n] = np.nan
            pmean[n] = np.nan
            pvar[n] = np.nan
            ess[n] = np.nan
        else:
            cloud[n] = cloud_at_failure[n]
    return dict(ll=ll, mean=mean, ess=ess, psi_mean=pmean, psi_var=pvar, cloud=cloud, weights=weights, psi=psi_out, status=status,
                resample_share=(resampled_steps / observed_steps if observed_steps else float("nan")), **mg)
