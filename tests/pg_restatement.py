"""NumPy restatement of the particle-Gibbs kernel (bayesian_dlms_amd/csrc/dlm_pg.hip, dlm_pg_batch): conditional SMC with ancestor sampling,
operation for operation and in the kernel's orders of summation (pf_restatement's: `particle_sum`, `running_sums`, products with the index
ascending), vectorised over the series of a batch.

The draws: Philox4x32-10 under DLM_KEY_PG | block (dlm_draws.h), counter (series, iteration, slot * 2048 + particle * 2): block q the
Box-Muller pair of the components 2 q and 2 q + 1 of a free particle, block 8 a free particle's ancestor uniform, block 9 the reference
particle's (slot t, particle P - 1), block 10 the final index (slot SLOT_INIT, particle 0); slot t for step t, SLOT_INIT for the initial cloud.

`run` also returns margin_search: the smallest |u total - cum_j| / total over ALL its searches (the free particles', the reference's, the
final index's), which is what the exact equality of the ancestors with the kernel's rests on.

`mutant`: ONE mistake of derivation put into the arithmetic here (never into the engine), for the rehearsals of tests/test_pg_host.py:
"noise-without-dt", "ancestor-density-without-dt", "ancestor-weights-without-w", "ancestor-density-at-x"."""
import numpy as np

import pf_restatement as pr
from pf_restatement import ST_NONFINITE, ST_NOT_PD, SLOT_INIT, TWO_PI, batch_rand, cholesky, log_density, particle_sum, running_sums

KEY_PG = 0x50470000
BLOCK_RESAMPLE, BLOCK_REF, BLOCK_FINAL = 8, 9, 10
MUTANTS = ("noise-without-dt", "ancestor-density-without-dt", "ancestor-weights-without-w", "ancestor-density-at-x")


def normals(seed, series, it, slot, P, d):
    """z [N][d][P]: a pair per Philox call (pg_normals)"""
    z = np.empty((len(series), d, P))
    for q in range((d + 1) // 2):
        u1, u2 = batch_rand(KEY_PG | q, seed, series, it, slot, P)
        r, ang = np.sqrt(-2.0 * np.log(u1)), TWO_PI * u2
        z[:, 2 * q] = r * np.cos(ang)
        if 2 * q + 1 < d:
            z[:, 2 * q + 1] = r * np.sin(ang)
    return z


def search(cum, target):
    """pf_ancestor for every (series, target): cum [N][P], target [N][K] -> the first j with cum[j] > target by the kernel's bisection
    (P - 1 when none is), [N][K] int64"""
    N, P = cum.shape
    lo = np.zeros(target.shape, dtype=np.int64)
    hi = np.full(target.shape, P - 1, dtype=np.int64)
    rows = np.arange(N)[:, None]
    while np.any(lo < hi):
        mid = (lo + hi) >> 1
        go = lo < hi
        above = cum[rows, mid] > target
        hi = np.where(go & above, mid, hi)
        lo = np.where(go & ~above, mid + 1, lo)
    return lo


def _margin(cum, target, anc, total):
    rows = np.arange(cum.shape[0])[:, None]
    near = np.minimum(np.abs(target - cum[rows, anc]), np.abs(target - cum[rows, np.maximum(anc - 1, 0)]))
    return near / total[:, None]


def matvec_full(L, z):
    """L [N][d][d] (zeros above the diagonal), z [N][d][P] -> [N][d][P]: the WHOLE row, c = 0 .. d - 1 in order, as the kernel sums it"""
    out = np.empty_like(z)
    d = z.shape[1]
    for r in range(d):
        acc = L[:, r, 0, None] * z[:, 0]
        for c in range(1, d):
            acc = acc + L[:, r, c, None] * z[:, c]
        out[:, r] = acc
    return out


def run(*, F, G, g_index, dt, V, W, m0, C0, y, ref, family, P, ancestor_sampling=True, nu=None, seed=0, series_offset=0, iteration=0,
        mutant=None):
    """F [d] or [T][d]; G [n_g][d][d] (row, column); g_index [T] or None; dt [T] or None; V scalar or [N]; W, C0 [d][d] or [N][d][d]; m0 [d] or
    [N][d]; y [N][T] (NaN = missing); ref [N][T+1][d]; nu scalar or [N].  Returns a dict: ll [N], path [N][T+1][d], stats [N][d+3],
    path_index [N][T+1], clouds [N][T+1][d][P], ancestors [N][T][P], step_weights [N][T][P], status [N], margin_search."""
    y = np.asarray(y, dtype=np.float64)
    N, T = y.shape
    G = np.asarray(G, dtype=np.float64)
    d = G.shape[1]
    F = np.asarray(F, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    V = np.broadcast_to(np.asarray(V, dtype=np.float64), (N,)).copy()
    W, C0, m0 = pr._per_series(W, N, (d, d)), pr._per_series(C0, N, (d, d)), pr._per_series(m0, N, (d,))
    nu = None if nu is None else np.broadcast_to(np.asarray(nu, dtype=np.float64), (N,)).copy()
    series = np.uint64(series_offset) + np.arange(N, dtype=np.uint64)
    rP = 1.0 / P
    rows = np.arange(N)

    status = np.zeros(N, dtype=np.int32)
    ll = np.zeros(N)
    clouds = np.full((N, T + 1, d, P), np.nan)
    ancestors = np.full((N, T, P), -1, dtype=np.int64)
    step_weights = np.full((N, T, P), np.nan)
    L0, ok0 = cholesky(C0)
    Lw, okw = cholesky(W)
    status[~(ok0 & okw)] = ST_NOT_PD
    alive = ok0 & okw
    margin = np.inf

    def fail(who):
        nonlocal alive
        status[who & alive] = ST_NONFINITE
        alive = alive & ~who

    with np.errstate(all="ignore"):
        x = m0[:, :, None] + matvec_full(L0, normals(seed, series, iteration, SLOT_INIT, P, d))
        wg = np.full((N, P), rP)
        fail(~np.all(np.isfinite(ref[:, 0]), axis=1))
        x[:, :, P - 1] = ref[:, 0]
        clouds[:, 0] = x
        for t in range(T):
            yt = y[:, t]
            missing = np.isnan(yt)
            dte = 1.0 if dt is None else float(dt[t])
            Gt = G[0 if g_index is None else g_index[t]]
            # the free particles' ancestors
            cum = running_sums(wg)
            total = cum[:, P - 1]
            _, u2 = batch_rand(KEY_PG | BLOCK_RESAMPLE, seed, series, iteration, t, P)
            target = u2 * total[:, None]
            anc = search(cum, target)
            mg = _margin(cum, target, anc, total)[:, :P - 1]
            if alive.any():
                margin = min(margin, float(mg[alive].min()))
            # the reference's
            aref = np.full(N, P - 1, dtype=np.int64)
            if dte != 0.0:
                rf = ref[:, t + 1]
                fail(~np.all(np.isfinite(rf), axis=1))
                if ancestor_sampling:
                    e = np.empty((N, d, P))
                    q = np.zeros((N, P))
                    for r in range(d):
                        if mutant == "ancestor-density-at-x":
                            gx = x[:, r].copy()
                        else:
                            gx = Gt[r, 0] * x[:, 0]
                            for c in range(1, d):
                                gx = gx + Gt[r, c] * x[:, c]
                        s = rf[:, r, None] - gx
                        for c in range(r):
                            s = s - Lw[:, r, c, None] * e[:, c]
                        s = s / Lw[:, r, r, None]
                        e[:, r] = s
                        q = q + s * s
                    q = (-0.5 * q) / (1.0 if mutant == "ancestor-density-without-dt" else dte)
                    m = np.fmax.reduce(np.concatenate([np.full((N, 1), -np.inf), q], axis=1), axis=1)
                    fail(~np.isfinite(m))
                    om = (rP if mutant == "ancestor-weights-without-w" else wg) * np.exp(q - m[:, None])
                    cum2 = running_sums(om)
                    tot = cum2[:, P - 1]
                    fail(~((tot > 0.0) & (tot < np.inf)))
                    _, u = pr.rand(KEY_PG | BLOCK_REF, seed, series, iteration, t, np.full(N, P - 1, dtype=np.uint64))
                    tg = (u * tot)[:, None]
                    a2 = search(cum2, tg)
                    if alive.any():
                        margin = min(margin, float(_margin(cum2, tg, a2, tot)[alive].min()))
                    aref = a2[:, 0]
            anc[:, P - 1] = aref
            ancestors[alive, t] = anc[alive]
            x = x[rows[:, None, None], np.arange(d)[None, :, None], anc[:, None, :]]
            if dte != 0.0:
                z = normals(seed, series, iteration, t, P, d)
                lz = matvec_full(Lw, z)
                sdt = np.sqrt(1.0 if mutant == "noise-without-dt" else dte)
                xn = np.empty_like(x)
                for r in range(d):
                    gx = Gt[r, 0] * x[:, 0]
                    for c in range(1, d):
                        gx = gx + Gt[r, c] * x[:, c]
                    xn[:, r] = gx + sdt * lz[:, r]
                xn[:, :, P - 1] = ref[:, t + 1]
                x = xn
            clouds[alive, t + 1] = x[alive]
            # the weights
            obs = alive & ~missing
            wg = np.where(missing[:, None], rP, wg)
            if obs.any():
                Ft = F if F.ndim == 1 else F[t]
                eta = Ft[0] * x[:, 0]
                for k in range(1, d):
                    eta = eta + Ft[k] * x[:, k]
                l = log_density(family, yt[:, None], eta, V[:, None], None if nu is None else nu[:, None])
                m = np.fmax.reduce(np.concatenate([np.full((N, 1), -np.inf), l], axis=1), axis=1)
                fail(obs & ~np.isfinite(m))
                w = np.exp(l - m[:, None])
                stot = particle_sum(w)
                fail(obs & ~((stot > 0.0) & (stot < np.inf)))
                obs = obs & alive
                ll = np.where(obs, ll + (m + np.log(stot / float(P))), ll)
                wg = np.where(obs[:, None], w / stot[:, None], wg)
            step_weights[alive, t] = wg[alive]

        # the final index and the trace-back
        cum = running_sums(wg)
        total = cum[:, P - 1]
        _, u = pr.rand(KEY_PG | BLOCK_FINAL, seed, series, iteration, SLOT_INIT, np.zeros(N, dtype=np.uint64))
        tg = (u * total)[:, None]
        kk = search(cum, tg)
        if alive.any():
            margin = min(margin, float(_margin(cum, tg, kk, total)[alive].min()))
        k = kk[:, 0]
        path = np.full((N, T + 1, d), np.nan)
        path_index = np.full((N, T + 1), -1, dtype=np.int64)
        ss, ssy, nob = np.zeros((N, d)), np.zeros(N), np.zeros(N)
        pn = clouds[rows, T, :, k]
        path[:, T], path_index[:, T] = pn, k
        for t in range(T - 1, -1, -1):
            k = np.where(alive, ancestors[rows, t, k], 0)
            pt = clouds[rows, t, :, k]
            if family == pr.GAUSSIAN:
                seen = ~np.isnan(y[:, t])
                Ft = F if F.ndim == 1 else F[t]
                f = Ft[0] * pn[:, 0]
                for c in range(1, d):
                    f = f + Ft[c] * pn[:, c]
                ssy = np.where(seen, ssy + (y[:, t] - f) * (y[:, t] - f), ssy)
                nob = np.where(seen, nob + 1.0, nob)
            dte = 1.0 if dt is None else float(dt[t])
            if dte != 0.0:
                Gt = G[0 if g_index is None else g_index[t]]
                for r in range(d):
                    gx = Gt[r, 0] * pt[:, 0]
                    for c in range(1, d):
                        gx = gx + Gt[r, c] * pt[:, c]
                    e = pn[:, r] - gx
                    ss[:, r] = ss[:, r] + (e * e) / dte
            path[:, t], path_index[:, t] = pt, k
            pn = pt
    stats = np.concatenate([ssy[:, None], nob[:, None], ss, np.full((N, 1), float(T))], axis=1)
    dead = status != 0
    ll[dead] = -np.inf
    path[dead] = np.nan
    stats[dead] = np.nan
    path_index[dead] = -1
    return dict(ll=ll, path=path, stats=stats, path_index=path_index, clouds=clouds, ancestors=ancestors, step_weights=step_weights,
                status=status, margin_search=margin)
