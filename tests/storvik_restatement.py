"""NumPy restatement of the Storvik filter kernel (bayesian_dlms_amd/csrc/dlm_storvik.hip, dlm_storvik_batch), operation for operation and
in the kernel's orders of summation, vectorised over the series of a batch.  The sums over the particles, the running
sums of the resampling search, the Cholesky factor, the densities, Philox and the addressing of the draws are tests/pf_restatement.py's, by import.

The draws: Philox4x32-10 under the key DLM_KEY_STORVIK | attempt << 8 | block (dlm_draws.h), counter (series, iteration,
slot * 2048 + particle * 2 + which): block q < 8 the Box-Muller pair of the components 2 q and 2 q + 1, block 8 the resampling uniform,
block 9 + k the Gamma of component k (k < d: W_kk, k = d: V), whose rejection attempt j sits in the key's second byte (`which` 0 its
normal, 1 its accept uniform; attempt 255 the boost of a shape below 1); slot t for step t, SLOT_INIT for the initial cloud.

`run` also returns the smallest MARGINS of every data-dependent decision of the kernel on its inputs: margin_search, margin_n0, margin_int as
tests/pf_restatement.py defines them, margin_accept -- the smallest |log u - bound| of the Gamma's accept test, relative to the sum of the
absolute values of the terms on both sides -- and margin_v, the smallest |1 + c x| of its v <= 0 test (relative to the 1); and the share of
observed steps that resampled."""
import numpy as np

from pf_restatement import (GAUSSIAN, ST_NONFINITE, ST_NOT_PD, TWO_PI, _per_series, batch_rand, cholesky, log_density,  # noqa: F401
                            matvec_lower, normal, particle_sum, rand, running_sums)

KEY_STORVIK = 0x53740000
BLOCK_RESAMPLE, BLOCK_GAMMA, GAMMA_ATTEMPTS = 8, 9, 255
SLOT_INIT = 0x1FFFFF


def st_rand(seed, series, it, slot, particles, block, attempt=0, which=0):
    """series, particles: flat arrays of one length -> (u1 in (0, 1], u2 in [0, 1)) of that length."""
    return rand(KEY_STORVIK | (attempt << 8) | block, seed, series, it, slot, particles, which)


def _grid(series, P):
    return np.repeat(np.asarray(series, dtype=np.uint64), P), np.tile(np.arange(P, dtype=np.uint64), len(series))


def gamma(shape, seed, series, it, slot, P, comp, margins):
    """Gamma(shape[n], 1) for every particle of the series: [len(series)][P] (gamma_unit_from of dlm_draws.h with 255 attempts)."""
    ser, part = _grid(series, P)
    a = np.repeat(np.asarray(shape, dtype=np.float64), P)
    block = BLOCK_GAMMA + comp
    boost = np.ones_like(a)
    small = a < 1.0
    if small.any():
        u1, _ = st_rand(seed, ser[small], it, slot, part[small], block, GAMMA_ATTEMPTS, 0)
        boost[small] = u1 ** (1.0 / a[small])
        a[small] += 1.0
    dd = a - 1.0 / 3.0
    cc = 1.0 / np.sqrt(9.0 * dd)
    out = dd * boost
    idx = np.arange(a.size)
    for k in range(GAMMA_ATTEMPTS):
        if idx.size == 0:
            break
        u1, u2 = st_rand(seed, ser[idx], it, slot, part[idx], block, k, 0)
        x = np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI * u2)
        v = 1.0 + cc[idx] * x
        margins["margin_v"] = min(margins["margin_v"], float(np.abs(v).min()))
        pos = v > 0.0
        v = np.where(pos, v, 1.0)
        v = v * v * v
        w1, _ = st_rand(seed, ser[idx], it, slot, part[idx], block, k, 1)
        d_ = dd[idx]
        lhs, rhs = np.log(w1), 0.5 * x * x + d_ - d_ * v + d_ * np.log(v)
        scale = np.abs(lhs) + 0.5 * x * x + d_ + d_ * v + d_ * np.abs(np.log(v))
        if pos.any():
            margins["margin_accept"] = min(margins["margin_accept"], float((np.abs(lhs - rhs) / scale)[pos].min()))
        ok = pos & (lhs < rhs)
        out[idx[ok]] = d_[ok] * v[ok] * boost[idx[ok]]
        idx = idx[~ok]
    return out.reshape(len(series), P)


def run(*, F, G, g_index, dt, V, m0, C0, y, family, P, prior_w, prior_v=None, learn_v=None, n0=-1, literal=False, nu=None, seed=0,
        series_offset=0, iteration=0, **unused):
    """F [d] or [T][d]; G [n_g][d][d] (row, column); g_index [T] or None; dt [T] or None; V scalar or [N] (read without learn_v); C0 [d][d] or
    [N][d][d]; m0 [d] or [N][d]; prior_w [d][2] or [N][d][2] (shape, scale); prior_v [2] or [N][2]; y [N][T] (NaN = missing); nu scalar or [N].
    Returns a dict: ll [N], mean [N][T][d], ess [N][T], scale_mean [N][T][d+1], cloud [N][d][P], weights [N][P], scales [N][d+1][P],
    status [N], the margins and resample_share."""
    y = np.asarray(y, dtype=np.float64)
    N, T = y.shape
    G = np.asarray(G, dtype=np.float64)
    d = G.shape[1]
    F = np.asarray(F, dtype=np.float64)
    learn_v = family == GAUSSIAN if learn_v is None else bool(learn_v)
    assert not learn_v or family == GAUSSIAN
    V = None if learn_v else np.broadcast_to(np.asarray(V, dtype=np.float64), (N,)).copy()
    C0, m0 = _per_series(C0, N, (d, d)), _per_series(m0, N, (d,))
    pw = _per_series(prior_w, N, (d, 2))
    pv = _per_series(prior_v, N, (2,)) if learn_v else None
    nu = None if nu is None else np.broadcast_to(np.asarray(nu, dtype=np.float64), (N,)).copy()
    n0 = P // 5 if n0 < 0 else n0
    series = np.uint64(series_offset) + np.arange(N, dtype=np.uint64)
    rP = 1.0 / P

    status = np.zeros(N, dtype=np.int32)
    ll = np.zeros(N)
    mean = np.full((N, T, d), np.nan)
    smean = np.full((N, T, d + 1), np.nan)
    ess = np.full((N, T), np.nan)
    L0, ok0 = cholesky(C0)
    ok0 &= np.all(pw > 0.0, axis=(1, 2))
    if learn_v:
        ok0 &= np.all(pv > 0.0, axis=1)
    status[~ok0] = ST_NOT_PD
    alive = ok0.copy()
    z = np.stack([normal(KEY_STORVIK, seed, series, iteration, SLOT_INIT, P, 0, c) for c in range(d)], axis=1)
    x = m0[:, :, None] + matvec_lower(L0, z)
    bw = np.broadcast_to(pw[:, :, 1, None], (N, d, P)).copy()
    bv = np.broadcast_to(pv[:, 1, None], (N, P)).copy() if learn_v else np.zeros((N, P))
    wg = np.full((N, P), rP)
    cloud_at_failure = {}
    n_adv, n_obs = 0, np.zeros(N)
    ess_last = np.full(N, float(P))
    mg = dict(margin_search=np.inf, margin_n0=np.inf, margin_int=np.inf, margin_accept=np.inf, margin_v=np.inf)
    observed_steps = resampled_steps = 0

    def outputs(t, who):
        for k in range(d):
            mean[who, t, k] = particle_sum(wg * x[:, k])[who]
            smean[who, t, k] = particle_sum(wg * bw[:, k])[who]
        if learn_v:
            smean[who, t, d] = particle_sum(wg * bv)[who]

    with np.errstate(all="ignore"):
        for t in range(T):
            yt = y[:, t]
            missing = np.isnan(yt)
            dte = 1.0 if dt is None else float(dt[t])
            if dte != 0.0 and alive.any():
                who = np.nonzero(alive)[0]
                Gt = G[0 if g_index is None else g_index[t]]
                xo = x[who]
                for r in range(d):
                    gx = Gt[r, 0] * xo[:, 0]
                    for c in range(1, d):
                        gx = gx + Gt[r, c] * xo[:, c]
                    zr = normal(KEY_STORVIK, seed, series[who], iteration, t, P, 0, r)
                    g = gamma(pw[who, r, 0] + 0.5 * float(n_adv), seed, series[who], iteration, t, P, r, mg)
                    b = bw[who, r]
                    w = b / g
                    xn = gx + np.sqrt(dte * w) * zr
                    e = xn - gx
                    bw[who, r] = b + (0.5 * (e * e)) / dte
                    x[who, r] = xn
            if dte != 0.0:
                n_adv += 1
            mis = alive & missing
            if mis.any():
                outputs(t, mis)
                ess[mis, t] = ess_last[mis]
            obs = alive & ~missing
            if not obs.any():
                continue
            who = np.nonzero(obs)[0]
            Ft = F if F.ndim == 1 else F[t]
            eta = Ft[0] * x[who, 0]
            for k in range(1, d):
                eta = eta + Ft[k] * x[who, k]
            if learn_v:
                g = gamma(pv[who, 0] + 0.5 * n_obs[who], seed, series[who], iteration, t, P, d, mg)
                b, e = bv[who], yt[who, None] - eta
                lw = log_density(GAUSSIAN, yt[who, None], eta, b / g)
                bv[who] = b + 0.5 * (e * e)
                n_obs[who] += 1.0
            else:
                lw = log_density(family, yt[who, None], eta, V[who, None], None if nu is None else nu[who, None], literal)
            l = np.full((N, P), -np.inf)
            l[who] = lw
            m = np.fmax.reduce(np.concatenate([np.full((N, 1), -np.inf), l], axis=1), axis=1)
            fail = obs & ~np.isfinite(m)
            om = (rP if literal else wg) * np.exp(l - m[:, None])
            stot = particle_sum(om)
            fail |= obs & ~((stot > 0.0) & (stot < np.inf))
            for n in np.nonzero(fail)[0]:
                status[n] = ST_NONFINITE
                cloud_at_failure[n] = x[n].copy()
            alive &= ~fail
            obs &= ~fail
            if not obs.any():
                continue
            ll = np.where(obs, ll + (m + np.log(stot)), ll)
            w = om / stot[:, None]
            wg = np.where(obs[:, None], w, wg)
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
            total = cum[:, P - 1]
            _, u2 = batch_rand(KEY_STORVIK | BLOCK_RESAMPLE, seed, series, iteration, t, P)
            target = u2 * total[:, None]
            for n in np.nonzero(res)[0]:
                top = np.maximum.accumulate(cum[n])
                anc = np.minimum(np.searchsorted(top, target[n], side="right"), P - 1)
                near = np.minimum(np.abs(target[n] - cum[n, anc]), np.abs(target[n] - cum[n, np.maximum(anc - 1, 0)]))
                mg["margin_search"] = min(mg["margin_search"], float((near / total[n]).min()))
                x[n] = x[n][:, anc]          # the whole tuple moves: the state, the scales of W, the scale of V
                bw[n] = bw[n][:, anc]
                bv[n] = bv[n][anc]
                wg[n] = rP

    dead = status != 0
    ll[dead] = -np.inf
    cloud = x.copy()
    weights = wg.copy()
    scales = np.concatenate([bw, bv[:, None, :] if learn_v else np.full((N, 1, P), np.nan)], axis=1)
    weights[dead] = np.nan
    scales[dead] = np.nan
    for n in np.nonzero(dead)[0]:
        if status[n] & ST_NOT_PD:
            cloud[n] = np.nan
            mean[n] = np.nan
            smean[n] = np.nan
            ess[n] = np.nan
        else:
            cloud[n] = cloud_at_failure[n]
    return dict(ll=ll, mean=mean, ess=ess, scale_mean=smean, cloud=cloud, weights=weights, scales=scales, status=status,
                resample_share=(resampled_steps / observed_steps if observed_steps else float("nan")), **mg)
