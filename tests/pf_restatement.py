"""NumPy restatement of the bootstrap particle filter kernel (bayesian_dlms_amd/csrc/dlm_pf.hip, dlm_pf_batch), operation for operation and in
the kernel's orders of summation, vectorised over the series of a batch:

  particle i = 64 s + lane;  a sum over the particles: per lane over its slots s in order (from 0.0), then the xor butterfly over the lanes
  (partners 32 .. 1) -- `particle_sum`;  the running sums of the resampling search: per slot the Hillis-Steele scan over the lanes (offsets
  1 .. 32), plus the carry of the slot before -- `running_sums`;  the ancestor of particle i: the first j whose running sum exceeds
  u_i times the last one;  matrix-vector products with the index ascending, the first product starting the sum.

The draws: Philox4x32-10 under the key DLM_KEY_PF | block (dlm_draws.h), counter (series, iteration, slot * 2048 + particle * 2): block q
the Box-Muller pair of the components 2 q and 2 q + 1, block 8 the resampling uniform; slot t for step t, SLOT_INIT for the initial cloud.

`run` also returns what the tests need to know about their own inputs: the two MARGINS -- the smallest |u_i total - cum_j| / total over
all resampling searches and the smallest |1 / sum W^2 - n0| over all observed steps (a third: the smallest distance of 1 / sum W^2 from
any integer, which is what the exact equality of the ESS output rests on) -- and the share of observed steps that resampled.  The switches
q37 / q38 / q39 turn on one quirk of the reference each; the kernel's `literal` is all three."""
import numpy as np
from scipy.special import gammaln

from sampler_restatement import MASK, philox

KEY_PF = 0x50462000
BLOCK_RESAMPLE = 8
SLOT_INIT = 0x1FFFFF
GAUSSIAN, POISSON, NEGBIN, ZIP, STUDENTT, BETA = range(6)
ST_NONFINITE, ST_NOT_PD = 1, 2
TWO_PI = 6.283185307179586476925286766559


def rand(key, seed, series, it, slot, particles, which=0):
    """The two uniforms of a particle kernel (gibbs_rand of dlm_draws.h) under `key` -- the filter's key | block, for the Storvik filter
    | attempt << 8 too -- at the counter (series, iteration, slot * 2048 + particle * 2 + which).  series and particles broadcast against
    one another ([N][1] and [P]: the whole batch; two flat arrays of one length: those pairs) -> (u1 in (0, 1], u2 in [0, 1)) of that shape."""
    series, particles = np.broadcast_arrays(np.asarray(series, dtype=np.uint64), np.asarray(particles, dtype=np.uint64))
    word = (np.uint64(slot) * np.uint64(2048) + particles * np.uint64(2) + np.uint64(which)) & MASK
    z = np.zeros(series.shape, dtype=np.uint64)
    c = philox(series & MASK, series >> np.uint64(32), z + np.uint64(it & 0xFFFFFFFF), word,
               seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ key)
    f = [x.astype(np.float64) for x in c]
    u1 = (f[0] * 4294967296.0 + f[1] + 1.0) * (1.0 / 18446744073709551616.0)
    u2 = (f[2] * 4294967296.0 + f[3]) * (1.0 / 18446744073709551616.0)
    return u1, u2


def batch_rand(key, seed, series, it, slot, P):
    """`rand` for every particle of every series: series [N] -> (u1, u2), each [N][P]."""
    return rand(key, seed, np.asarray(series, dtype=np.uint64)[:, None], it, slot, np.arange(P, dtype=np.uint64))


def normal(key, seed, series, it, slot, P, base, r):
    """z_r [len(series)][P], one component of a Box-Muller pair (st_normal of dlm_storvik.hip, lw_normal of dlm_lw.hip): block
    base + r // 2 under `key`, the cosine for an even r and the sine for an odd one."""
    u1, u2 = batch_rand(key | (base + (r >> 1)), seed, series, it, slot, P)
    rad, ang = np.sqrt(-2.0 * np.log(u1)), TWO_PI * u2
    return rad * (np.sin(ang) if r & 1 else np.cos(ang))


def normals(seed, series, it, slot, P, d):
    """z [N][d][P]: the bootstrap filter's, a pair per Philox call"""
    z = np.empty((len(series), d, P))
    for q in range((d + 1) // 2):
        u1, u2 = batch_rand(KEY_PF | q, seed, series, it, slot, P)
        r, ang = np.sqrt(-2.0 * np.log(u1)), TWO_PI * u2
        z[:, 2 * q] = r * np.cos(ang)
        if 2 * q + 1 < d:
            z[:, 2 * q + 1] = r * np.sin(ang)
    return z


def particle_sum(terms):
    """terms [N][P] -> [N]: the lane-sequential sums over the slots, then the xor butterfly."""
    N, P = terms.shape
    lanes = np.zeros((N, 64))
    for s in range(P // 64):
        lanes = lanes + terms[:, 64 * s:64 * (s + 1)]
    idx = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, idx ^ m]
    return lanes[:, 0]


def running_sums(w):
    """w [N][P] -> the inclusive running sums [N][P] as the kernel forms them."""
    N, P = w.shape
    cum = np.empty_like(w)
    carry = np.zeros(N)
    for s in range(P // 64):
        v = w[:, 64 * s:64 * (s + 1)].copy()
        off = 1
        while off < 64:
            nv = v.copy()
            nv[:, off:] = v[:, off:] + v[:, :-off]
            v = nv
            off *= 2
        c = carry[:, None] + v
        cum[:, 64 * s:64 * (s + 1)] = c
        carry = c[:, 63]
    return cum


def cholesky(A):
    """A [N][d][d] -> (L [N][d][d] lower, ok [N]): the kernel's pf_chol (a series stops at its first pivot that is not positive)."""
    N, d, _ = A.shape
    L = np.zeros_like(A)
    ok = np.ones(N, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(d):
            s = A[:, j, j].copy()
            for k in range(j):
                s = s - L[:, j, k] * L[:, j, k]
            ok &= s > 0.0
            dj = np.sqrt(np.where(ok, s, 1.0))
            L[:, j, j] = dj
            for i in range(j + 1, d):
                t = A[:, i, j].copy()
                for k in range(j):
                    t = t - L[:, i, k] * L[:, j, k]
                L[:, i, j] = t / dj
    return L, ok


def matvec_lower(L, z):
    """L [N][d][d], z [N][d][P] -> [N][d][P], c = 0 .. r in order"""
    out = np.empty_like(z)
    for r in range(z.shape[1]):
        acc = L[:, r, 0, None] * z[:, 0]
        for c in range(1, r + 1):
            acc = acc + L[:, r, c, None] * z[:, c]
        out[:, r] = acc
    return out


def log_density(family, y, eta, v, nu=None, q39=False, terms=False):
    """log p(y | eta, v) as the kernel computes it (pf_obs + pf_logdens): y, v, nu broadcast against eta.  terms=True: also the sum of the
    absolute values of the terms the density is made of (what its rounding error scales with)."""
    y, eta, v = np.broadcast_arrays(np.asarray(y, dtype=np.float64), np.asarray(eta, dtype=np.float64), np.asarray(v, dtype=np.float64))
    with np.errstate(all="ignore"):
        if family == GAUSSIAN:
            e = y - eta
            parts = [-(0.5 * np.log(TWO_PI * v)), -((0.5 * (e * e)) / v)]
            val = parts[0] + parts[1]
        elif family == POISSON:
            k = np.trunc(y)
            parts = [k * eta, -np.exp(eta), -gammaln(k + 1.0)]
            val = (parts[0] + parts[1]) + parts[2]
        elif family == NEGBIN:
            size, mu = np.exp(v), np.exp(eta)
            parts = [gammaln(size + y), -gammaln(y + 1.0), -gammaln(size), size * np.log(size / (mu + size)), y * np.log(mu / (mu + size))]
            val = (((parts[0] + parts[1]) + parts[2]) + parts[3]) + parts[4]
        elif family == ZIP:
            ev = np.exp(v)
            p = ev / (1.0 + ev)
            zero = np.log(p + (1.0 - p) * np.exp(-np.exp(eta)))
            pz = [y * eta, -np.log(1.0 + ev), -np.exp(eta), -gammaln(y + 1.0)]
            nonzero = ((pz[0] + pz[1]) + pz[2]) + pz[3]
            is0 = np.abs(y) < 1e-5
            val = np.where(is0, zero, nonzero)
            parts = [np.where(is0, zero, sum(np.abs(q) for q in pz))]
        elif family == STUDENTT:
            nu = np.asarray(nu, dtype=np.float64)
            sc = np.sqrt(v)
            e = y - eta
            parts = [gammaln((nu + 1.0) * 0.5), -(0.5 * np.log(np.pi * nu * sc if q39 else np.pi * nu * sc * sc)), -gammaln(nu * 0.5),
                     -(((nu + 1.0) * 0.5) * np.log1p((e * e) / (nu * sc * sc)))]
            val = ((parts[0] + parts[1]) + parts[2]) + parts[3]
        else:
            mean = np.where(eta < -5.0, 0.0, np.where(eta > 5.0, 1.0, 1.0 / (1.0 + np.exp(-eta))))
            aa = (mean * (1.0 - mean)) / v
            al, be = mean * (aa - 1.0), (1.0 - mean) * (aa - 1.0)
            good = (al > 0.0) & (be > 0.0)
            als, bes = np.where(good, al, 1.0), np.where(good, be, 1.0)
            parts = [(als - 1.0) * np.log(y), (bes - 1.0) * np.log(1.0 - y), -gammaln(als), -gammaln(bes), gammaln(als + bes)]
            val = (parts[0] + parts[1]) - ((-parts[2] + -parts[3]) - parts[4])
            val = np.where(good, val, -np.inf)
    if terms:
        return val, sum(np.abs(q) for q in parts)
    return val


def _per_series(a, N, shape):
    a = np.asarray(a, dtype=np.float64)
    return np.broadcast_to(a, (N,) + shape).copy() if a.shape == shape else a.reshape((N,) + shape).copy()


def run(*, F, G, g_index, dt, V, W, m0, C0, y, family, P, n0=-1, literal=False, q37=None, q38=None, q39=None, nu=None, seed=0,
        series_offset=0, iteration=0):
    """F [d] or [T][d]; G [n_g][d][d] (row, column); g_index [T] or None; dt [T] or None; V scalar or [N]; W, C0 [d][d] or [N][d][d]; m0 [d] or
    [N][d]; y [N][T] (NaN = missing); nu scalar or [N].  Returns a dict: ll [N], mean [N][T][d], ess [N][T], cloud [N][d][P], weights [N][P],
    status [N], margin_search, margin_n0, margin_int, resample_share."""
    q37 = literal if q37 is None else q37
    q38 = literal if q38 is None else q38
    q39 = literal if q39 is None else q39
    y = np.asarray(y, dtype=np.float64)
    N, T = y.shape
    G = np.asarray(G, dtype=np.float64)
    n_g, d = G.shape[0], G.shape[1]
    F = np.asarray(F, dtype=np.float64)
    V = np.broadcast_to(np.asarray(V, dtype=np.float64), (N,)).copy()
    W, C0, m0 = _per_series(W, N, (d, d)), _per_series(C0, N, (d, d)), _per_series(m0, N, (d,))
    nu = None if nu is None else np.broadcast_to(np.asarray(nu, dtype=np.float64), (N,)).copy()
    n0 = P // 5 if n0 < 0 else n0
    series = np.uint64(series_offset) + np.arange(N, dtype=np.uint64)
    rP = 1.0 / P

    status = np.zeros(N, dtype=np.int32)
    ll = np.zeros(N)
    mean = np.full((N, T, d), np.nan)
    ess = np.full((N, T), np.nan)
    L0, ok0 = cholesky(C0)
    Lw, okw = cholesky(W)
    status[~(ok0 & okw)] = ST_NOT_PD
    alive = ok0 & okw
    x = m0[:, :, None] + matvec_lower(L0, normals(seed, series, iteration, SLOT_INIT, P, d))
    wg = np.full((N, P), rP)
    cloud_at_failure = {}
    dt_held = np.zeros(N)
    ess_last = np.full(N, float(P))
    margin_search = margin_n0 = margin_int = np.inf
    observed_steps = resampled_steps = 0

    def means(t, who):
        for k in range(d):
            mean[who, t, k] = particle_sum(wg * x[:, k])[who]

    with np.errstate(all="ignore"):
        for t in range(T):
            yt = y[:, t]
            missing = np.isnan(yt)
            dte = (1.0 if dt is None else dt[t]) + dt_held
            dt_held = np.where(missing & bool(q38) & (n_g == 1), dte, 0.0)
            adv = alive & (dte != 0.0)
            if adv.any():
                Gt = G[0 if g_index is None else g_index[t]]
                z = normals(seed, series, iteration, t, P, d)
                lz = matvec_lower(Lw, z)
                xn = np.empty_like(x)
                for r in range(d):
                    gx = Gt[r, 0] * x[:, 0]
                    for c in range(1, d):
                        gx = gx + Gt[r, c] * x[:, c]
                    xn[:, r] = gx + np.sqrt(dte)[:, None] * lz[:, r]
                x = np.where(adv[:, None, None], xn, x)
            mis = alive & missing
            if mis.any():
                means(t, mis)
                ess[mis, t] = ess_last[mis]
            obs = alive & ~missing
            if not obs.any():
                continue
            Ft = F if F.ndim == 1 else F[t]
            eta = Ft[0] * x[:, 0]
            for k in range(1, d):
                eta = eta + Ft[k] * x[:, k]
            l = log_density(family, yt[:, None], eta, V[:, None], None if nu is None else nu[:, None], q39)
            m = np.fmax.reduce(np.concatenate([np.full((N, 1), -np.inf), l], axis=1), axis=1)
            fail = obs & ~np.isfinite(m)
            om = (rP if q37 else wg) * np.exp(l - m[:, None])
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
            means(t, obs)
            e = np.floor(1.0 / sq)
            ess_last = np.where(obs, e, ess_last)
            ess[obs, t] = e[obs]
            inv = (1.0 / sq)[obs]
            margin_n0 = min(margin_n0, np.abs(inv - n0).min())
            margin_int = min(margin_int, np.abs(inv - np.round(inv)).min())
            res = obs & (e < float(n0))
            observed_steps += int(obs.sum())
            resampled_steps += int(res.sum())
            if not res.any():
                continue
            cum = running_sums(wg)
            total = cum[:, P - 1]
            _, u2 = batch_rand(KEY_PF | BLOCK_RESAMPLE, seed, series, iteration, t, P)
            target = u2 * total[:, None]
            for n in np.nonzero(res)[0]:
                top = np.maximum.accumulate(cum[n])          # the first j with cum[j] > target = the first j whose running maximum is
                anc = np.minimum(np.searchsorted(top, target[n], side="right"), P - 1)
                near = np.minimum(np.abs(target[n] - cum[n, anc]), np.abs(target[n] - cum[n, np.maximum(anc - 1, 0)]))
                margin_search = min(margin_search, (near / total[n]).min())
                x[n] = x[n][:, anc]
                wg[n] = rP

    ll[status != 0] = -np.inf
    dead = status != 0
    cloud = x.copy()
    weights = wg.copy()
    weights[dead] = np.nan
    for n in np.nonzero(dead)[0]:
        if status[n] & ST_NOT_PD:
            cloud[n] = np.nan
            mean[n] = np.nan
            ess[n] = np.nan
        else:
            cloud[n] = cloud_at_failure[n]
    return dict(ll=ll, mean=mean, ess=ess, cloud=cloud, weights=weights, status=status, margin_search=margin_search, margin_n0=margin_n0,
                margin_int=margin_int, resample_share=(resampled_steps / observed_steps if observed_steps else float("nan")))


def kalman(F, G, g_index, dt, V, W, m0, C0, y):
    """The Kalman filter of one Gaussian series on the particle filter's conventions (dt == 0: no advance): the filtered means [T][d] and
    the prediction-error log-likelihood, sum over the observed t of log N(y_t; F_t^T a_t, F_t^T R_t F_t + V)."""
    F, G = np.asarray(F, dtype=np.float64), np.asarray(G, dtype=np.float64)
    m, C = np.asarray(m0, dtype=np.float64).copy(), np.asarray(C0, dtype=np.float64).copy()
    T = len(y)
    ms, ll = np.empty((T, m.size)), 0.0
    for t in range(T):
        step = 1.0 if dt is None else dt[t]
        if step != 0.0:
            Gt = G[0 if g_index is None else g_index[t]]
            m, C = Gt @ m, Gt @ C @ Gt.T + W * step
        if not np.isnan(y[t]):
            Ft = F if F.ndim == 1 else F[t]
            f, q = Ft @ m, Ft @ C @ Ft + V
            e = y[t] - f
            ll += -0.5 * np.log(2.0 * np.pi * q) - 0.5 * e * e / q
            K = C @ Ft / q
            m, C = m + K * e, C - np.outer(K, K) * q
        ms[t] = m
    return ms, ll
