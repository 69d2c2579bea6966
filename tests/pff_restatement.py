"""NumPy restatement of the observation draws of the forecast kernel (bayesian_dlms_amd/csrc/dlm_obs_draws.h, dlm_pf_forecast.hip), operation
for operation, on top of tests/pf_restatement.py (Philox, the state step, the fixed orders of summation).

A SITE is where a draw takes its uniforms from: (seed, series, iteration, slot, particle), series and particles flat arrays of one length M
(M draws side by side).  Every sampler returns (draws [M], margins [M]): a draw's MARGIN is the smallest relative gap of any compare or accept
decision that was evaluated for it -- |a - b| / max(|a|, |b|) of a comparison a < b, the distance to the nearest integer over the magnitude
for a floor.  The device's exp / log / pow / lgamma may differ from libm's by ulps; a draw whose margin stands clear of that (1e-9, seven
orders of magnitude above double rounding) has to be EQUAL on the device.

The blocks (dlm_draws.h): BLOCK_OBS the observation's first pair (u1, u2) -- the Box-Muller cosine of the Gaussian and Student-t families, u1
the zero-inflation uniform, u2 the inversion uniform of a rate below PTRS_FROM; BLOCK_POISSON + j attempt j of Hoermann's PTRS; BLOCK_GAMMA_A /
BLOCK_GAMMA_B + j attempt j of the first / second Gamma (which 0 the normal's pair, which 1 the accept uniform), j = GAMMA_ATTEMPTS the boost."""
from dataclasses import dataclass

import numpy as np
from scipy.special import gammaln

import pf_restatement as pr

BLOCK_RESAMPLE0, BLOCK_OBS, BLOCK_POISSON = 9, 10, 11
POISSON_ATTEMPTS = GAMMA_ATTEMPTS = 32
BLOCK_GAMMA_A = BLOCK_POISSON + POISSON_ATTEMPTS
BLOCK_GAMMA_B = BLOCK_GAMMA_A + GAMMA_ATTEMPTS + 1
PTRS_FROM, RATE_MAX, INVERSION_STEPS = 10.0, 1e15, 128
TINY = np.finfo(np.float64).tiny


@dataclass
class Site:
    seed: int
    series: np.ndarray      # [M] uint64
    iteration: int
    slot: int
    particles: np.ndarray   # [M] uint64

    def take(self, idx):
        return Site(self.seed, self.series[idx], self.iteration, self.slot, self.particles[idx])

    def rand(self, block, which=0):
        return pr.rand(pr.KEY_PF | block, self.seed, self.series, self.iteration, self.slot, self.particles, which)


def batch_site(seed, series, iteration, slot, P):
    """Every particle of every series: M = len(series) P, series-major."""
    series = np.asarray(series, dtype=np.uint64)
    return Site(seed, np.repeat(series, P), iteration, slot, np.tile(np.arange(P, dtype=np.uint64), len(series)))


def gap(a, b):
    """The relative gap of a comparison of a with b."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    return np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), TINY)


def gamma_draw(a, base, site):
    """Gamma(a, 1) [M]: gamma_unit_from of dlm_draws.h with GAMMA_ATTEMPTS attempts in the blocks base + j."""
    a = np.array(a, dtype=np.float64)
    M = a.size
    margin = gap(a, 1.0)
    boost = np.ones(M)
    small = a < 1.0
    if small.any():
        idx = np.nonzero(small)[0]
        u1, _ = site.take(idx).rand(base + GAMMA_ATTEMPTS)
        boost[idx] = np.power(u1, 1.0 / a[idx])
        a[idx] = a[idx] + 1.0
    dd = a - 1.0 / 3.0
    cc = 1.0 / np.sqrt(9.0 * dd)
    out = dd * boost
    active = np.ones(M, dtype=bool)
    with np.errstate(all="ignore"):
        for k in range(GAMMA_ATTEMPTS):
            idx = np.nonzero(active)[0]
            if idx.size == 0:
                break
            s = site.take(idx)
            u1, u2 = s.rand(base + k, 0)
            x = np.sqrt(-2.0 * np.log(u1)) * np.cos(pr.TWO_PI * u2)
            v = 1.0 + cc[idx] * x
            margin[idx] = np.minimum(margin[idx], gap(1.0, -(cc[idx] * x)))
            pos = v > 0.0
            v3 = v * v * v
            w1, _ = s.rand(base + k, 1)
            lhs = np.log(w1)
            d = dd[idx]
            rhs = ((0.5 * x * x + d) - d * v3) + d * np.log(np.where(pos, v3, 1.0))
            margin[idx] = np.where(pos, np.minimum(margin[idx], gap(lhs, rhs)), margin[idx])
            acc = pos & (lhs < rhs)
            take = idx[acc]
            out[take] = (d[acc] * v3[acc]) * boost[take]
            active[take] = False
    return out, margin


def poisson_draw(lam, site):
    """Poisson(lam) [M], NaN for a rate outside [0, RATE_MAX]: pf_poisson_draw."""
    lam = np.asarray(lam, dtype=np.float64)
    M = lam.size
    out = np.full(M, np.nan)
    margin = np.full(M, np.inf)
    with np.errstate(all="ignore"):
        valid = (lam >= 0.0) & (lam <= RATE_MAX)
        margin[valid] = np.minimum(gap(lam[valid], PTRS_FROM), gap(lam[valid], RATE_MAX))
        # -- sequential inversion of one uniform
        idx = np.nonzero(valid & (lam < PTRS_FROM))[0]
        if idx.size:
            l = lam[idx]
            _, u = site.take(idx).rand(BLOCK_OBS)
            p = np.exp(-l)
            cdf = p.copy()
            k = np.zeros(idx.size)
            mg = np.full(idx.size, np.inf)
            active = np.ones(idx.size, dtype=bool)
            for j in range(1, INVERSION_STEPS + 1):
                mg = np.where(active, np.minimum(mg, gap(u, cdf)), mg)
                active &= ~(u < cdf)
                if not active.any():
                    break
                p = np.where(active, (p * l) / float(j), p)
                nxt = cdf + p
                stall = active & (nxt == cdf)
                mg = np.where(stall, 0.0, mg)          # (the far tail, u within an ulp of 1: excused)
                active &= ~stall
                cdf = np.where(active, nxt, cdf)
                k = np.where(active, float(j), k)
            out[idx] = k
            margin[idx] = np.minimum(margin[idx], mg)
        # -- PTRS
        idx = np.nonzero(valid & ~(lam < PTRS_FROM))[0]
        if idx.size:
            out[idx] = np.floor(lam[idx])
            active = np.ones(idx.size, dtype=bool)
            for j in range(POISSON_ATTEMPTS):
                sub = np.nonzero(active)[0]
                if sub.size == 0:
                    break
                g = idx[sub]
                l = lam[g]
                slam, loglam = np.sqrt(l), np.log(l)
                b = 0.931 + 2.53 * slam
                a = -0.059 + 0.02483 * b
                invalpha = 1.1239 + 1.1328 / (b - 3.4)
                vr = 0.9277 - 3.6224 / (b - 2.0)
                V, u2 = site.take(g).rand(BLOCK_POISSON + j)
                U = u2 - 0.5
                us = 0.5 - np.abs(U)
                arg = (((2.0 * a) / us + b) * U + l) + 0.43
                k = np.floor(arg)
                mg = np.minimum(np.abs(arg - np.round(arg)) / np.maximum(np.abs(arg), 1.0), gap(us, 0.07))
                wide = us >= 0.07
                mg = np.where(wide, np.minimum(mg, gap(V, vr)), mg)
                quick = wide & (V <= vr)
                rest = ~quick
                neg = k < 0.0                                   # (k is an integer: the floor's margin covers it)
                small = us < 0.013
                mg = np.where(rest & ~neg, np.minimum(mg, gap(us, 0.013)), mg)
                mg = np.where(rest & ~neg & small, np.minimum(mg, gap(V, us)), mg)
                skip = rest & (neg | (small & (V > us)))
                test = rest & ~skip
                ks = np.where(test, k, 1.0)
                lhs = (np.log(V) + np.log(invalpha)) - np.log(a / (us * us) + b)
                rhs = (ks * loglam - l) - gammaln(ks + 1.0)
                mg = np.where(test, np.minimum(mg, gap(lhs, rhs)), mg)
                acc = quick | (test & (lhs <= rhs))
                margin[g] = np.minimum(margin[g], mg)
                out[g[acc]] = k[acc]
                active[sub[acc]] = False
    return out, margin


def normal_draw(site):
    u1, u2 = site.rand(BLOCK_OBS)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(pr.TWO_PI * u2)


def obs_draw(family, eta, v, nu, site):
    """One draw of y | eta, v per site (pf_obs_draw): eta [M]; v, nu scalars or [M] -> (draws [M], margins [M])."""
    eta = np.asarray(eta, dtype=np.float64)
    M = eta.size
    v = np.broadcast_to(np.asarray(v, dtype=np.float64), (M,))
    inf = np.full(M, np.inf)
    with np.errstate(all="ignore"):
        if family == pr.GAUSSIAN:
            return eta + np.sqrt(v) * normal_draw(site), inf
        if family == pr.POISSON:
            return poisson_draw(np.exp(eta), site)
        if family == pr.NEGBIN:
            size, mu = np.exp(v), np.exp(eta)
            ok = (size > 0.0) & (size < np.inf)
            g, mg = gamma_draw(np.where(ok, size, 1.0), BLOCK_GAMMA_A, site)
            k, mk = poisson_draw((g * mu) / size, site)
            return np.where(ok, k, np.nan), np.minimum(mg, mk)
        if family == pr.ZIP:
            ev = np.exp(v)
            p0 = ev / (1.0 + ev)
            lam = np.exp(eta)
            ok = lam <= RATE_MAX
            u1, _ = site.rand(BLOCK_OBS)
            zero = u1 < p0
            k, mk = poisson_draw(np.where(ok, lam, 0.0), site)
            margin = np.minimum(gap(lam, RATE_MAX), gap(u1, p0))
            return np.where(ok, np.where(zero, 0.0, k), np.nan), np.where(zero, margin, np.minimum(margin, mk))
        if family == pr.STUDENTT:
            nu = np.broadcast_to(np.asarray(nu, dtype=np.float64), (M,))
            z = normal_draw(site)
            g, _ = gamma_draw(nu * 0.5, BLOCK_GAMMA_A, site)
            w = ((nu * v) * 0.5) / g
            return eta + np.sqrt(w) * z, inf
        mean = np.where(eta < -5.0, 0.0, np.where(eta > 5.0, 1.0, 1.0 / (1.0 + np.exp(-eta))))
        aa = (mean * (1.0 - mean)) / v
        al, be = mean * (aa - 1.0), (1.0 - mean) * (aa - 1.0)
        ok = (al > 0.0) & (be > 0.0) & (al < np.inf) & (be < np.inf)
        ga, _ = gamma_draw(np.where(ok, al, 1.0), BLOCK_GAMMA_A, site)
        gb, _ = gamma_draw(np.where(ok, be, 1.0), BLOCK_GAMMA_B, site)
        return np.where(ok, ga / (ga + gb), np.nan), inf


def forecast_mean(draws):
    """draws [N][P] -> [N]: the kernel's fmean, the fixed-order sum of pf_restatement.particle_sum times 1 / P."""
    return pr.particle_sum(draws) * (1.0 / draws.shape[1])


def simulate(*, F, G, g_index, dt, V, W, m0, C0, family, P, H, N, nu=None, seed=0, series_offset=0, iteration=0, slot_offset=0):
    """The forecast kernel with cloud0 = NULL and every y missing (nothing is weighted or resampled): the initial cloud as
    pf_restatement.run draws it, H steps from the slots slot_offset + h, one draw per particle and step.  F [d] or [H][d]; G [n_g][d][d];
    V, nu scalars or [N]; W, C0 [d][d]; m0 [d].  Returns {"draws" [N][H][P], "margin" [N][H][P], "fmean" [N][H], "eta" [N][H][P]}."""
    G = np.asarray(G, dtype=np.float64)
    d = G.shape[1]
    F = np.asarray(F, dtype=np.float64)
    series = np.uint64(series_offset) + np.arange(N, dtype=np.uint64)
    V = np.broadcast_to(np.asarray(V, dtype=np.float64), (N,))
    nu = None if nu is None else np.broadcast_to(np.asarray(nu, dtype=np.float64), (N,))
    L0, ok0 = pr.cholesky(np.broadcast_to(np.asarray(C0, dtype=np.float64), (N, d, d)).copy())
    Lw, okw = pr.cholesky(np.broadcast_to(np.asarray(W, dtype=np.float64), (N, d, d)).copy())
    assert ok0.all() and okw.all()
    x = np.broadcast_to(np.asarray(m0, dtype=np.float64), (N, d))[:, :, None] + pr.matvec_lower(L0, pr.normals(seed, series, iteration, pr.SLOT_INIT, P, d))
    draws, margin, etas = np.empty((N, H, P)), np.empty((N, H, P)), np.empty((N, H, P))
    for h in range(H):
        step = 1.0 if dt is None else dt[h]
        if step != 0.0:
            Gt = G[0 if g_index is None else g_index[h]]
            lz = pr.matvec_lower(Lw, pr.normals(seed, series, iteration, slot_offset + h, P, d))
            xn = np.empty_like(x)
            for r in range(d):
                gx = Gt[r, 0] * x[:, 0]
                for c in range(1, d):
                    gx = gx + Gt[r, c] * x[:, c]
                xn[:, r] = gx + np.sqrt(step) * lz[:, r]
            x = xn
        Fh = F if F.ndim == 1 else F[h]
        eta = Fh[0] * x[:, 0]
        for k in range(1, d):
            eta = eta + Fh[k] * x[:, k]
        site = batch_site(seed, series, iteration, slot_offset + h, P)
        y, mg = obs_draw(family, eta.reshape(-1), np.repeat(V, P), None if nu is None else np.repeat(nu, P), site)
        draws[:, h], margin[:, h], etas[:, h] = y.reshape(N, P), mg.reshape(N, P), eta
    fmean = np.stack([forecast_mean(draws[:, h]) for h in range(H)], axis=1)
    return dict(draws=draws, margin=margin, fmean=fmean, eta=etas)
