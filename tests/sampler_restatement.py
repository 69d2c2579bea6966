"""NumPy restatements of the Gibbs parameter steps, operation for operation and in the kernels' summation order: what the GPU tests
hold the kernels to draw for draw, and what the host tests check against the models.  First bayesian_dlms_amd/csrc/dlm_draws.h --
Philox4x32-10, gibbs_rand, gamma_unit, draw_normal, draw_log_uniform, the Beta proposal, the slot table -- and the lane-sequential sums
with their xor butterfly (wave_sum); then one series of each kernel: `step` (k_studentt_step, with its Poisson sampler), `params_step`
(k_sv_params) and `ou_params_step` (k_sv_ou_params), each with the helpers that make its prior."""
import math

import numpy as np

from bayesian_dlms_amd import _lib

MASK = np.uint64(0xFFFFFFFF)
KEY_GIBBS, KEY_STUDENTT, KEY_SV, KEY_SVOU = 0x47494242, 0x53545544, 0x5354564F, 0x53564F55
# the scalar slots: from SLOT_TOP downward, per sampler
SLOT_TOP = 0x1FFFFF
ST_SLOT_PROP_GAMMA, ST_SLOT_POISSON, ST_SLOT_ACCEPT, ST_SLOT_SCALE = (SLOT_TOP - k for k in range(4))
SV_SLOT_PHI, SV_SLOT_MU, SV_SLOT_SIGMA, SV_SLOT_PROP_A, SV_SLOT_PROP_B, SV_SLOT_ACCEPT = (SLOT_TOP - k for k in range(6))
(SVOU_SLOT_PROP_A, SVOU_SLOT_PROP_B, SVOU_SLOT_ACC_PHI, SVOU_SLOT_Z_SIGMA, SVOU_SLOT_ACC_SIGMA, SVOU_SLOT_Z_MU,
 SVOU_SLOT_ACC_MU) = (SLOT_TOP - k for k in range(7))
OU_FIELDS = ("literal", "phi_a", "phi_b", "mu_mean", "mu_sd", "sigma_shape", "sigma_scale", "prop_lambda", "prop_tau", "delta_sigma", "delta_mu")


def philox(c0, c1, c2, c3, k0, k1):
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0 = (k0 + np.uint64(0x9E3779B9)) & MASK
        k1 = (k1 + np.uint64(0xBB67AE85)) & MASK
    return c0, c1, c2, c3


def gibbs_rand(seed, series, it, comp, attempt, which, key):
    comp = np.asarray(comp, dtype=np.uint64)
    word = (comp * np.uint64(2048) + np.uint64(attempt) * np.uint64(2) + np.uint64(which)) & MASK
    z = np.zeros_like(comp)
    c = philox(z + np.uint64(series & 0xFFFFFFFF), z + np.uint64(series >> 32), z + np.uint64(it & 0xFFFFFFFF), word,
               seed & 0xFFFFFFFF, (seed >> 32) ^ key)
    f = [x.astype(np.float64) for x in c]
    u1 = (f[0] * 4294967296.0 + f[1] + 1.0) * (1.0 / 18446744073709551616.0)
    u2 = (f[2] * 4294967296.0 + f[3]) * (1.0 / 18446744073709551616.0)
    return u1, u2


def gamma_unit(a, seed, series, it, comp, key):
    """Vectorised over (a, comp) for one series."""
    a = np.array(a, dtype=np.float64, ndmin=1).copy()
    comp = np.broadcast_to(np.asarray(comp, dtype=np.uint64), a.shape).copy()
    boost = np.ones_like(a)
    small = a < 1.0
    if small.any():
        u1, _ = gibbs_rand(seed, series, it, comp[small], 1023, 0, key)
        boost[small] = u1 ** (1.0 / a[small])
        a[small] += 1.0
    dd = a - 1.0 / 3.0
    cc = 1.0 / np.sqrt(9.0 * dd)
    out = dd * boost
    todo = np.ones(a.shape, bool)
    for k in range(1023):
        idx = np.nonzero(todo)[0]
        if idx.size == 0:
            break
        u1, u2 = gibbs_rand(seed, series, it, comp[idx], k, 0, key)
        x = np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586476925286766559 * u2)
        v = 1.0 + cc[idx] * x
        pos = v > 0.0
        v = np.where(pos, v, 1.0)
        v = v * v * v
        w1, _ = gibbs_rand(seed, series, it, comp[idx], k, 1, key)
        ddi = dd[idx]
        ok = pos & (np.log(w1) < 0.5 * x * x + ddi - ddi * v + ddi * np.log(v))
        out[idx[ok]] = ddi[ok] * v[ok] * boost[idx[ok]]
        todo[idx[ok]] = False
    return out


def normal(key, seed, series, it, slot, attempt=0):
    """draw_normal: the Box-Muller cosine of attempt `attempt` of a scalar slot."""
    u1, u2 = gibbs_rand(seed, series, it, [slot], attempt, 0, key)
    return math.sqrt(-2.0 * math.log(u1[0])) * math.cos(6.283185307179586476925286766559 * u2[0])


def log_uniform(key, seed, series, it, slot):
    """draw_log_uniform: log u of a scalar slot's (0, 1] uniform."""
    u1, _ = gibbs_rand(seed, series, it, [slot], 0, 0, key)
    return math.log(u1[0])


def beta_proposal(phi0, lam, tau, key, seed, series, it, slot_a, slot_b):
    """BetaProposal: phi' ~ Beta(lam phi0 + tau, lam (1 - phi0) + tau) as ga / (ga + gb).  -> (phi', lq): lq() = (log q(phi' | phi0),
    log q(phi0 | phi')), for a phi' inside (0, 1)."""
    A0, B0 = lam * phi0 + tau, lam * (1.0 - phi0) + tau
    ga = gamma_unit(A0, seed, series, it, slot_a, key)[0]
    gb = gamma_unit(B0, seed, series, it, slot_b, key)[0]
    phip = ga / (ga + gb)

    def lq():
        lg, log = math.lgamma, math.log
        A1, B1 = lam * phip + tau, lam * (1.0 - phip) + tau
        lq_fwd = lg(A0 + B0) - lg(A0) - lg(B0) + (A0 - 1.0) * log(phip) + (B0 - 1.0) * log(1.0 - phip)
        lq_back = lg(A1 + B1) - lg(A1) - lg(B1) + (A1 - 1.0) * log(phi0) + (B1 - 1.0) * log(1.0 - phi0)
        return lq_fwd, lq_back
    return phip, lq


def ptrs_loggam(x):
    if x == 1.0 or x == 2.0:
        return 0.0
    n = int(7.0 - x) if x < 7.0 else 0
    x0 = x + n
    x2 = (1.0 / x0) * (1.0 / x0)
    c = [8.333333333333333e-02, -2.777777777777778e-03, 7.936507936507937e-04, -5.952380952380952e-04, 8.417508417508418e-04,
         -1.917526917526918e-03, 6.410256410256410e-03, -2.955065359477124e-02, 1.796443723688307e-01, -1.39243221690590e+00]
    gl0 = c[9]
    for k in range(8, -1, -1):
        gl0 *= x2
        gl0 += c[k]
    gl = gl0 / x0 + 0.5 * 1.8378770664093453e+00 + (x0 - 0.5) * math.log(x0) - x0
    for _ in range(n):
        gl -= math.log(x0 - 1.0)
        x0 -= 1.0
    return gl


def poisson(lam, seed, series, it):
    if not lam > 0.0:
        return 0.0
    if lam < 10.0:
        _, u2 = gibbs_rand(seed, series, it, [ST_SLOT_POISSON], 0, 0, KEY_STUDENTT)
        u = u2[0]
        p = math.exp(-lam); cdf = p; k = 0.0
        while u > cdf and k < 200.0:
            k += 1.0; p *= lam / k; cdf += p
        return k
    slam, loglam = math.sqrt(lam), math.log(lam)
    b = 0.931 + 2.53 * slam
    a = -0.059 + 0.02483 * b
    invalpha = 1.1239 + 1.1328 / (b - 3.4)
    vr = 0.9277 - 3.6224 / (b - 2.0)
    for att in range(1023):
        u1, u2 = gibbs_rand(seed, series, it, [ST_SLOT_POISSON], att, 0, KEY_STUDENTT)
        U, V = u2[0] - 0.5, u1[0]
        us = 0.5 - abs(U)
        if not us > 0.0:
            continue
        k = math.floor((2.0 * a / us + b) * U + lam + 0.43)
        if us >= 0.07 and V <= vr:
            return float(k)
        if k < 0.0 or (us < 0.013 and V > us):
            continue
        if math.log(V) + math.log(invalpha) - math.log(a / (us * us) + b) <= -lam + k * loglam - ptrs_loggam(k + 1.0):
            return float(k)
    return math.floor(lam)


def wave_sum(terms):
    """terms [T] in t order (0 where a lane adds nothing): the lane-sequential sums, then the xor butterfly."""
    T = terms.size
    rows = -(-T // 64)
    pad = np.zeros(rows * 64)
    pad[:T] = terms
    lanes = np.zeros(64)
    for r in range(rows):
        lanes = lanes + pad[r * 64:(r + 1) * 64]
    idx = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[idx ^ m]
    return lanes[0]


def dot_rows(F, x):
    """sum_i F[.., i] x[.., i] in i order (the kernel's loop)."""
    f = np.zeros(x.shape[0])
    for i in range(x.shape[1]):
        f = f + F[:, i] * x[:, i]
    return f


def step(F, y, theta, stats, prior, s, nu, *, seed, series, it, literal):
    """One series.  F [T][d] (time-varying) or [d]; y [T]; theta [T+1][d]; stats [d + 3].  Returns (v [T], s', nu', W diag [d],
    accepted, loglik)."""
    lam_prior, r, aw, bw = prior
    T, d = y.size, theta.shape[1]
    Ft = np.broadcast_to(np.asarray(F, dtype=np.float64).reshape(-1, d), (T, d))
    L = d + 3
    wsh = aw + 0.5 * stats[L - 1]
    wd = np.array([(bw + 0.5 * stats[2 + i]) / gamma_unit(wsh, seed, series, it, 1 + i, KEY_GIBBS)[0] for i in range(d)])
    dnu = float(nu)
    q = dnu / (r + dnu)
    g = gamma_unit(r, seed, series, it, ST_SLOT_PROP_GAMMA, KEY_STUDENTT)[0]
    nup = poisson(g * (q / (1.0 - q)), seed, series, it) + 1.0
    prop_ok = 1.0 <= nup < 1.0e9
    sc = math.sqrt(s)
    den0 = dnu * sc * sc if literal else dnu * s
    den1 = nup * sc * sc if literal else nup * s
    f1 = dot_rows(Ft, theta[1:])
    e1 = y - f1
    e = y - dot_rows(Ft, theta[:-1]) if literal else e1
    obs = ~np.isnan(y)
    with np.errstate(invalid="ignore"):
        A0 = wave_sum(np.where(obs, np.log1p(e1 * e1 / den0), 0.0))
        A1 = wave_sum(np.where(obs, np.log1p(e1 * e1 / den1), 0.0))
    nobs = float(obs.sum())
    off = 0.0 if literal else 1.0
    k1, k2 = dnu - off, nup - off
    lg = math.lgamma
    c0 = sc if literal else s
    PI = 3.141592653589793
    ll0 = nobs * (lg((dnu + 1.0) * 0.5) - 0.5 * math.log(PI * dnu * c0) - lg(dnu * 0.5)) - (dnu + 1.0) * 0.5 * A0
    ll_out, acc = ll0, 0
    if prop_ok:
        ll1 = nobs * (lg((nup + 1.0) * 0.5) - 0.5 * math.log(PI * nup * c0) - lg(nup * 0.5)) - (nup + 1.0) * 0.5 * A1
        lm0 = ll0 + (dnu * math.log(lam_prior) - lam_prior - lg(dnu + 1.0))
        lm1 = ll1 + (nup * math.log(lam_prior) - lam_prior - lg(nup + 1.0))
        q1, q2 = nup / (r + nup), dnu / (r + dnu)
        pp1 = lg(r + k1) - lg(k1 + 1.0) - lg(r) + r * math.log(1.0 - q1) + k1 * math.log(q1)
        pp2 = lg(r + k2) - lg(k2 + 1.0) - lg(r) + r * math.log(1.0 - q2) + k2 * math.log(q2)
        lacc = lm1 + pp1 - lm0 - pp2
        if log_uniform(KEY_STUDENTT, seed, series, it, ST_SLOT_ACCEPT) < lacc:
            acc, ll_out = 1, ll1
    nu_v = float(nup) if (acc and not literal) else dnu
    eobs = ~np.isnan(e)
    shape = np.where(eobs | literal, (nu_v + 1.0) * 0.5, nu_v * 0.5)
    beta = nu_v * s * 0.5 + np.where(eobs, np.nan_to_num(e) * np.nan_to_num(e) * 0.5, 0.0)
    v = beta / gamma_unit(shape, seed, series, it, np.arange(T), KEY_STUDENTT)
    R = wave_sum(1.0 / v)
    snew = gamma_unit(T * nu_v * 0.5 + 1.0, seed, series, it, ST_SLOT_SCALE, KEY_STUDENTT)[0] / (nu_v * 0.5 * R)
    return v, snew, int(nup) if acc else int(nu), wd, acc, ll_out


# ---- k_sv_params ----------------------------------------------------------------------------------------------------------------
def params_step(al, sv, pr, *, seed, series, it):
    """One series of k_sv_params.  al [T+1]; sv = (phi, mu, sigma); pr: the ten fields of dlm_sv_prior as a dict.
    -> (phi, mu, sigma, accepted, status, attempts)."""
    T = al.size - 1
    lit, beta = bool(pr["literal"]), bool(pr["phi_update"])
    phi0, mu0, sig0 = (float(x) for x in sv)
    if not (math.isfinite(phi0) and math.isfinite(mu0) and sig0 > 0.0 and sig0 < math.inf) or (beta and not 0.0 < phi0 < 1.0):
        return math.nan, math.nan, math.nan, 0, _lib.ST_NONFINITE, 0
    s2 = sig0 * sig0
    a0, a1, aT = al[0], al[1], al[T]
    prev, cur = al[1:T], al[2:T + 1]             # the pairs t = 2..T
    st, acc, attempts, phi = 0, 0, 0, phi0
    if not beta:
        p, c = prev - mu0, cur - mu0
        d0, d1, dT = a0 - mu0, a1 - mu0, aT - mu0
        S = wave_sum(p * p) + (dT * dT if lit else d0 * d0)
        S2 = wave_sum(p * c) + (0.0 if lit else d0 * d1)
        psi2 = pr["phi_b"] * pr["phi_b"]
        prec = 1.0 / psi2 + S if lit else 1.0 / psi2 + S / s2
        mean = (pr["phi_a"] / psi2 + S2) / prec if lit else (pr["phi_a"] / psi2 + S2 / s2) / prec
        sd = math.sqrt(1.0 / prec)
        if lit:
            phi, attempts = mean + sd * normal(KEY_SV, seed, series, it, SV_SLOT_PHI, 0), 1
        else:
            ok = False
            for k in range(1023):
                cand = mean + sd * normal(KEY_SV, seed, series, it, SV_SLOT_PHI, k)
                attempts += 1
                if abs(cand) < 1.0:
                    phi, ok = cand, True
                    break
            if not ok:
                st |= _lib.ST_NOT_PD
    else:
        phip, lq = beta_proposal(phi0, pr["prop_lambda"], pr["prop_tau"], KEY_SV, seed, series, it, SV_SLOT_PROP_A, SV_SLOT_PROP_B)
        p, c = prev - mu0, cur - mu0
        r0, r1 = c - phi0 * p, c - phip * p
        d0, d1 = a0 - mu0, a1 - mu0
        f0, f1 = d1 - phi0 * d0, d1 - phip * d0
        Q0 = wave_sum(r0 * r0) + (0.0 if lit else f0 * f0)
        Q1 = wave_sum(r1 * r1) + (0.0 if lit else f1 * f1)
        if 0.0 < phip < 1.0:
            log = math.log
            pa, pb = pr["phi_a"], pr["phi_b"]
            o0, o1 = 1.0 - phi0 * phi0, 1.0 - phip * phip
            lt0 = (pa - 1.0) * log(phi0) + (pb - 1.0) * log(1.0 - phi0) + 0.5 * log(o0) - 0.5 * d0 * d0 * o0 / s2 - 0.5 * Q0 / s2
            lt1 = (pa - 1.0) * log(phip) + (pb - 1.0) * log(1.0 - phip) + 0.5 * log(o1) - 0.5 * d0 * d0 * o1 / s2 - 0.5 * Q1 / s2
            lq_fwd, lq_back = lq()
            lacc = lt1 - lt0 + lq_back - lq_fwd
            if log_uniform(KEY_SV, seed, series, it, SV_SLOT_ACCEPT) < lacc:
                acc, phi = 1, phip
    M = wave_sum(cur - phi * prev) + (0.0 if lit else a1 - phi * a0)
    pm2, omp, Td = pr["mu_sd"] * pr["mu_sd"], 1.0 - phi, float(T)
    mprec = 1.0 / pm2 + (Td - 1.0) * omp * omp if lit else 1.0 / pm2 + Td * omp * omp / s2
    mmean = (pr["mu_mean"] / pm2 + omp * M) / mprec if lit else (pr["mu_mean"] / pm2 + omp / s2 * M) / mprec
    mu = mmean + math.sqrt(1.0 / mprec) * normal(KEY_SV, seed, series, it, SV_SLOT_MU, 0)
    r = (cur - mu) - phi * (prev - mu)
    fr = (a1 - mu) - phi * (a0 - mu)
    Q = wave_sum(r * r) + (0.0 if lit else fr * fr)
    shape = pr["sigma_shape"] + ((Td + 1.0) * 0.5 if lit else Td * 0.5)
    scale = pr["sigma_scale"] + 0.5 * Q
    sig = math.sqrt(scale / gamma_unit(shape, seed, series, it, SV_SLOT_SIGMA, KEY_SV)[0])
    return phi, mu, sig, acc, st, attempts


def sv_prior(phi_update, literal, phi_a, phi_b, mu=(1.0, 2.0), sigma=(3.0, 0.5), prop=(100.0, 0.05)):
    return dict(phi_update=phi_update, literal=literal, phi_a=phi_a, phi_b=phi_b, mu_mean=mu[0], mu_sd=mu[1], sigma_shape=sigma[0],
                sigma_scale=sigma[1], prop_lambda=prop[0], prop_tau=prop[1])


def sv_prior_tuple(pr):
    return tuple(pr[k] for k, _ in _lib.SvPrior._fields_)


# ---- k_sv_ou_params -------------------------------------------------------------------------------------------------------------
def ou_prior(literal=0, phi=(5.0, 2.0), mu=(1.0, 2.0), sigma=(3.0, 0.5), prop=(10.0, 0.05), delta=(0.3, 0.3)):
    return dict(literal=literal, phi_a=phi[0], phi_b=phi[1], mu_mean=mu[0], mu_sd=mu[1], sigma_shape=sigma[0], sigma_scale=sigma[1],
                prop_lambda=prop[0], prop_tau=prop[1], delta_sigma=delta[0], delta_mu=delta[1])


def ou_prior_tuple(pr):
    return tuple(pr[k] for k in OU_FIELDS)


def ou_sums(al, times, mu0, phi):
    """(L, A, B, C, n) of one row at the rate phi: the terms of t = 2..T in t order (0 where dt = 0), summed as the wave sums them."""
    T = al.size - 1
    dt = times[1:] - times[:-1]                  # dt_t = times[t-1] - times[t-2], t = 2..T
    pos = dt > 0.0
    d = np.where(pos, dt, 1.0)
    p, c = al[1:T] - mu0, al[2:T + 1] - mu0
    with np.errstate(all="ignore"):
        e = np.exp(-phi * d)
        g = -np.expm1(-2.0 * phi * d)
        ig = 1.0 / g
        r, w = c - e * p, 1.0 - e
        terms = (np.log(g), r * r * ig, r * w * ig, w * w * ig)
        return tuple(wave_sum(np.where(pos, x, 0.0)) for x in terms) + (float(pos.sum()),)


def ou_params_step(times, al, sv, pr, *, seed, series, it):
    """One series of k_sv_ou_params.  al [T+1]; sv = (phi, mu, sigma); pr: the eleven fields of dlm_sv_ou_prior as a dict.
    -> (phi, mu, sigma, accepted (phi, sigma, mu), status, margins (phi, sigma, mu), moves): margin = |log u - Delta| of a decision
    that was made (inf where none was); moves = ((phi', Delta), (sigma', Delta), (mu', Delta)), what each move proposed and its log
    acceptance ratio (tests/test_stochvol_ou_host.py holds them against the model's log density written out term by term)."""
    nan3, inf3 = (math.nan,) * 3, [math.inf] * 3
    lit = bool(pr["literal"])
    phi0, mu0, sig0 = (float(x) for x in sv)
    dt = times[1:] - times[:-1]
    bad = not (0.0 < phi0 < 1.0) or not math.isfinite(mu0) or not (0.0 < sig0 < math.inf)
    bad = bad or not bool(((dt >= 0.0) & (dt < math.inf)).all())
    if bad:
        return nan3 + ((0, 0, 0), _lib.ST_NONFINITE, inf3, None)
    phip, lq = beta_proposal(phi0, pr["prop_lambda"], pr["prop_tau"], KEY_SVOU, seed, series, it, SVOU_SLOT_PROP_A, SVOU_SLOT_PROP_B)
    L0, SA0, SB0, SC0, nd = ou_sums(al, times, mu0, phi0)
    if not all(math.isfinite(x) for x in (L0, SA0, SB0, SC0)):
        return nan3 + ((0, 0, 0), _lib.ST_NONFINITE, inf3, None)
    margins, moves = list(inf3), [(phip, math.nan), None, None]
    log = math.log
    acc_phi = acc_sig = acc_mu = 0
    phi, SA, SB, SC = phi0, SA0, SB0, SC0
    if 0.0 < phip < 1.0:
        L1, SA1, SB1, SC1, _ = ou_sums(al, times, mu0, phip)
        pa, pb, s2 = pr["phi_a"], pr["phi_b"], sig0 * sig0
        lt0 = (pa - 1.0) * log(phi0) + (pb - 1.0) * log(1.0 - phi0) + 0.5 * nd * log(2.0 * phi0) - 0.5 * L0 - phi0 * SA0 / s2
        lt1 = (pa - 1.0) * log(phip) + (pb - 1.0) * log(1.0 - phip) + 0.5 * nd * log(2.0 * phip) - 0.5 * L1 - phip * SA1 / s2
        lq_fwd, lq_back = lq()
        lacc = lt1 - lt0 if lit else lt1 - lt0 + lq_back - lq_fwd
        lu = log_uniform(KEY_SVOU, seed, series, it, SVOU_SLOT_ACC_PHI)
        moves[0] = (phip, lacc)
        if not math.isnan(lacc):
            margins[0] = abs(lu - lacc)
        if lu < lacc:
            acc_phi, phi, SA, SB, SC = 1, phip, SA1, SB1, SC1
    d0 = al[0] - mu0
    sig = sig0
    sigp = sig0 * math.exp(pr["delta_sigma"] * normal(KEY_SVOU, seed, series, it, SVOU_SLOT_Z_SIGMA))
    moves[1] = (sigp, math.nan)
    if 0.0 < sigp < math.inf:
        sh, sc = pr["sigma_shape"], pr["sigma_scale"]
        ls0, ls1 = log(sig0), log(sigp)
        lt0 = -(sh + 1.0) * ls0 - sc / sig0 - nd * ls0 - phi * SA / (sig0 * sig0)
        lt1 = -(sh + 1.0) * ls1 - sc / sigp - nd * ls1 - phi * SA / (sigp * sigp)
        if not lit:
            lt0 = lt0 - ls0 - d0 * d0 / (2.0 * sig0 * sig0)
            lt1 = lt1 - ls1 - d0 * d0 / (2.0 * sigp * sigp)
        lacc = lt1 - lt0 if lit else lt1 - lt0 + log(sigp / sig0)
        lu = log_uniform(KEY_SVOU, seed, series, it, SVOU_SLOT_ACC_SIGMA)
        margins[1], moves[1] = abs(lu - lacc), (sigp, lacc)
        if lu < lacc:
            acc_sig, sig = 1, sigp
    mu = mu0
    mup = mu0 + pr["delta_mu"] * normal(KEY_SVOU, seed, series, it, SVOU_SLOT_Z_MU)
    dl, s2, ps2 = mup - mu0, sig * sig, pr["mu_sd"] * pr["mu_sd"]
    Q1 = SA - 2.0 * dl * SB + dl * dl * SC
    m0, m1 = mu0 - pr["mu_mean"], mup - pr["mu_mean"]
    lt0 = -(m0 * m0) / (2.0 * ps2) - phi * SA / s2
    lt1 = -(m1 * m1) / (2.0 * ps2) - phi * Q1 / s2
    if not lit:
        d1 = al[0] - mup
        lt0 = lt0 - d0 * d0 / (2.0 * s2)
        lt1 = lt1 - d1 * d1 / (2.0 * s2)
    lu = log_uniform(KEY_SVOU, seed, series, it, SVOU_SLOT_ACC_MU)
    margins[2], moves[2] = abs(lu - (lt1 - lt0)), (mup, lt1 - lt0)
    if lu < lt1 - lt0:
        acc_mu, mu = 1, mup
    return phi, mu, sig, (acc_phi, acc_sig, acc_mu), 0, margins, moves


def ou_grid(T, seed):
    """An irregular grid: gaps from [0.1, 3]; from T = 8 on one repeated time (a dt = 0 inside the row) and one long gap."""
    gaps = np.random.default_rng(seed).uniform(0.1, 3.0, T - 1)
    if T >= 8:
        gaps[T // 2] = 0.0
        gaps[T // 3] = 40.0
    return np.concatenate([[0.5], 0.5 + np.cumsum(gaps)])


def ou_paths(times, sv, rng):
    """alpha [N][T+1] from the model at the parameters sv [N][3]: alpha_0 ~ N(mu, sigma^2), alpha_1 = alpha_0, then the OU transitions."""
    N, T = sv.shape[0], times.size
    phi, mu, sig = sv.T
    alpha = np.empty((N, T + 1))
    alpha[:, 0] = mu + sig * rng.standard_normal(N)
    alpha[:, 1] = alpha[:, 0]
    for t in range(2, T + 1):
        dt = times[t - 1] - times[t - 2]
        if dt == 0.0:
            alpha[:, t] = alpha[:, t - 1]
            continue
        sd = sig * np.sqrt(-np.expm1(-2.0 * phi * dt) / (2.0 * phi))
        alpha[:, t] = mu + np.exp(-phi * dt) * (alpha[:, t - 1] - mu) + sd * rng.standard_normal(N)
    return alpha


def ou_params_inputs(N, T, seed):
    rng = np.random.default_rng(seed)
    times = ou_grid(T, seed)
    sv = np.stack([rng.uniform(0.1, 0.9, N), rng.uniform(-1.0, 2.0, N), rng.uniform(0.1, 0.5, N)], axis=1)
    return times, ou_paths(times, sv, rng), sv
