"""The six kernels of the factor stochastic-volatility family (bayesian_dlms_amd/csrc/dlm_fsv.hip, dlm_dlmfsv.hip, dlm_fsv_solve.h) in
closed form and 50 significant digits (Python's decimal module, as tests/joint_posterior.py does it), with the error bound every
result is held to (tests/test_fsv_dense_reference_host.py: the NumPy restatements; tests/test_fsv_dense_reference_gpu.py: the device).

Nothing here follows a kernel's order of operations: dense matrices, exact sums, ONE textbook Cholesky factorisation P = L L^T, the
explicit inverses L^-1 and P^-1 = L^-T L^-1.  Inputs are the doubles the engine receives, converted exactly (Decimal(float) is exact);
exp is decimal's.  The normals z and the unit Gamma g are the Philox restatement's doubles (fsv_restatement.normals / gamma_units,
dlmfsv_restatement.normals, which tests/test_factorsv_host.py pins), taken as exact: the device's own copies differ from them by the
last bits of log, cos and sqrt, which the bounds carry as a term of their own.  Every result is returned as a double `hi` and the
remainder `lo` = exact - hi, so that `error(got, hi, lo)` is the distance to the 50-digit value, not to its rounding.  The arithmetic is
the standard library's; NumPy, which every test here has, carries the arrays and takes the two 2-norms of a system (of P and of the
50-digit P^-1, each rounded to doubles first: a norm does not notice that rounding).

  factors     every time with all p components finite:  P = beta^T D beta + diag(exp(-alpha_{.,t+1})) (+ I without alpha), D = diag(1/v),
              f = P^-1 beta^T D y_t + L^-T z;  literal: P^-1 beta^T D y_t + P^-1 z
  loadings    over the counted times S = sum f f^T, c_i = sum f y_i, ssy = sum_t sum_i (y_ti - beta_i f_t)^2 at the old beta, exactly;
              sigma^2 = scale' / g,  shape' = shape + n p / 2, scale' = scale + ssy / 2   (literal, Q28: shape + n / 2, scale + ssy / (2 p));
              row i >= 1, q = min(i, k):  P = S_q / sigma^2 + I / s^2,  r = (c_i - [i < k] S_{0:q,i}) / sigma^2 + m / s^2, the draw as above
              (literal, Q29-Q30 and Q27: P = S_q / sigma^2 + I s^2, r = c_i / sigma^2, the draw P^-1 (r + z))
  impute      every partially missing time: f given the observed components (the sums over the observed i alone), then
              r_ti = beta_i f + sqrt(v_i) z_i for the missing i
  variance    V_t = beta diag(exp alpha_{.,t+1}) beta^T + diag(v)
  center      r = y - F_t^T theta_{t+1}
  innovations w_t = theta_{t+1} - G theta_t

THE BOUNDS.  u = 2^-53, gamma_n = n u / (1 - n u).  A first-order bound counts once (the reference is exact) and is doubled for the
neglected higher-order terms, the convention of tests/test_dlmfsv_gpu.py.  Nothing in a bound is computed from the output under test.

center, innovations:  d products, d - 1 additions and one subtraction on terms whose magnitudes sum to m = |y_i| + sum_j |F_ji theta_j|:
    |r - r*| <= 2 (d + 2) u m.
variance:  exp, two products and k additions (the diagonal's included) on a term, k + 4 roundings, each taken at 1 ulp = 2 u as
    tests/test_dlmfsv_gpu.py takes them:  |V - V*| <= 4 (k + 4) u m,  m = sum_l |beta_il beta_jl| e_l + v_i [i == j]
    (that file's 8 (k + 4) u is this bound on either side of an inexact reference).

The solves (factors, impute, the loading rows), for one k x k system x = P^-1 r + L^-T z, all norms 2-norms unless marked F(robenius):
  formation   the computed P and r are P + E_P, r + e_r with, entry by entry,
              factors, impute:  |E_P| <= gamma_{p+2} |beta|^T D |beta| + diag(u P_jj + 3 u exp(-alpha_j)),   |e_r| <= gamma_{p+2} |beta|^T D |y|
              (1 / v, two products and p - 1 additions; on the diagonal the addition of exp(-alpha) and the 1 ulp = 2 u of exp)
              loading rows:  see `loadings`: the sums' gamma_{Tp+2} on their absolute sums and the relative error of sigma^2.
  solve       Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 10.3: the computed factor is exact for P + dP1,
              |dP1| <= gamma_{k+1} |L||L^T|;  Thm 10.4: the two substitutions included, (P + dP) x = r with |dP| <= gamma_{3k+1} |L||L^T|;
              || |L||L^T| || <= k ||P|| (eq. 10.7) and || |L||L^T| ||_F <= ||L||_F^2 = trace P <= k ||P||.  So with E = ||E_P||_F + k gamma_{3k+1} ||P||
              B_mean = ||P^-1|| (||e_r|| + E ||P^-1 r||)                  (backward error times cond_2(P) = ||P|| ||P^-1||, relative to ||P^-1 r||)
  L^-T z      the first-order change of the Cholesky factor under P + X is dL = L phi(L^-1 X L^-T), phi = the strict lower triangle plus
              half the diagonal, ||phi(Y)||_F <= ||Y||_F / sqrt 2 for symmetric Y; the change of L^-T z is then -L^-T phi^T z:
              B_L   = ||P^-1||^(3/2) (||E_P||_F + k gamma_{k+1} ||P||) ||z|| / sqrt 2
              the back substitution solves (L + dL2)^T x = fl(L^-1 r + z), |dL2| <= gamma_k |L| (Higham Thm 8.5), ||dL2|| <= gamma_k sqrt(k ||P||):
              B_sub = gamma_k sqrt(k cond_2(P)) ||L^-T z||,      B_add = ||P^-1||^(1/2) u (sqrt(r^T P^-1 r) + ||z||)
  normals     z = sqrt(-2 ln u1) cos(2 pi u2): the device and the restatement form the same argument fl(2 pi u2) (one IEEE product of the
              same doubles), so the rounding of 2 pi u2 cancels between them; they differ by the two logs (1 ulp each, halved by the
              square root), the two correctly rounded square roots, the two cosines (2 ulp on the device, 1 ulp in the C library) and the
              two products: (2 + 2 + 2 + 6 + 2) u = 14 u, taken as C_Z = 16, in units of the radius rho = sqrt(-2 ln u1) >= |z|.  No document
              on this machine states the accuracy of the device's log and cos; 1 ulp and 2 ulp are the figures of the accuracy tables of the
              HIP programming guide (device math functions, double precision) and of the OpenCL specification's full profile.
              B_z   = ||P^-1||^(1/2) C_Z u ||rho||
  default     ||x - x*||_inf <= ||x - x*|| <= 2 (B_mean + B_L + B_sub + B_add + B_z)
  literal     x = P^-1 (r + z):  2 ||P^-1|| (||e_r|| + u || |r| + |z| || + C_Z u ||rho|| + E ||P^-1 (r + z)||)
impute adds for a missing component i:  ||beta_i|| times the bound of f (Cauchy-Schwarz), gamma_{k+2} (sum_j |beta_ij f_j| + sqrt(v_i) |z_i|)
for the k products, the additions and the correctly rounded sqrt(v_i), and sqrt(v_i) C_Z u rho_i; the sum doubled as above.
sigma^2 and the loading sums: `loadings`."""
import functools
import math
import os
import sys
from decimal import Decimal, getcontext

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dlmfsv_restatement as dr  # noqa: E402
import fsv_restatement as fr  # noqa: E402
from sampler_restatement import gibbs_rand  # noqa: E402

PREC = 50
U = 2.0 ** -53
C_Z = 16.0
RHO_MAX = math.sqrt(-2.0 * math.log(2.0 ** -64))          # the largest radius a (0, 1] uniform of 64 bits gives
_ZERO, _ONE = Decimal(0), Decimal(1)


def gam(n):
    return n * U / (1.0 - n * U)


def _dec(x):
    return Decimal(float(x))


def _vec(a):
    return [Decimal(float(x)) for x in a]


def _rows(a):
    return [[Decimal(float(x)) for x in row] for row in a]


def _split(x):
    """A Decimal as (hi, lo): hi the nearest double, lo = x - hi."""
    hi = float(x)
    return hi, float(x - Decimal(hi))


def error(got, hi, lo):
    """|got - (hi + lo)|: got - hi is exact for a got near hi."""
    return np.abs((np.asarray(got, dtype=np.float64) - hi) - lo)


def radii(key, seed, series, it, comp, attempt):
    """sqrt(-2 ln u1) of the draw_normal that fr.normals / dr.normals give for the same arguments (a double: within 1 ulp, which a bound
    does not notice)."""
    series, comp, attempt = np.broadcast_arrays(np.asarray(series, np.int64), np.asarray(comp, np.int64), np.asarray(attempt, np.int64))
    u1, _ = gibbs_rand(seed, series, it, comp, attempt, 0, key)
    return np.sqrt(-2.0 * np.log(u1))


def _cholesky(P):
    k = len(P)
    L = [[_ZERO] * k for _ in range(k)]
    for j in range(k):
        s = P[j][j] - sum((v * v for v in L[j][:j]), _ZERO)
        if not s > 0:
            raise ArithmeticError("the dense reference met a matrix that is not positive definite in 50 digits")
        L[j][j] = s.sqrt()
        for i in range(j + 1, k):
            L[i][j] = (P[i][j] - sum((a * b for a, b in zip(L[i][:j], L[j][:j])), _ZERO)) / L[j][j]
    return L


def _lower_inverse(L):
    k = len(L)
    M = [[_ZERO] * k for _ in range(k)]
    for j in range(k):
        M[j][j] = _ONE / L[j][j]
        for i in range(j + 1, k):
            M[i][j] = -sum((L[i][m] * M[m][j] for m in range(j, i)), _ZERO) / L[i][i]
    return M


def _norm2(v):
    return math.sqrt(sum(float(x) ** 2 for x in v))


def solve(P, r, z, rho, EP, er):
    """One system in 50 digits.  P [k][k], r [k] Decimals; z [k] the normals (doubles, exact), rho [k] their radii; EP [k][k], er [k] the
    entrywise formation bounds (floats).  -> dict: x, x_lit (lists of Decimals), bound, bound_lit, cond, norm, norm_inv, xinf, xinf_lit."""
    k = len(r)
    zd = _vec(z)
    L = _cholesky(P)
    M = _lower_inverse(L)                                                            # L^-1
    Pinv = [[sum((M[m][a] * M[m][b] for m in range(max(a, b), k)), _ZERO) for b in range(k)] for a in range(k)]
    mean = [sum((Pinv[a][b] * r[b] for b in range(k)), _ZERO) for a in range(k)]
    xz = [sum((M[m][a] * zd[m] for m in range(a, k)), _ZERO) for a in range(k)]         # L^-T z
    x = [a + b for a, b in zip(mean, xz)]
    x_lit = [sum((Pinv[a][b] * (r[b] + zd[b]) for b in range(k)), _ZERO) for a in range(k)]
    # the 2-norms of P and of the 50-digit P^-1, each rounded to doubles first (a norm is insensitive to that rounding)
    nP = float(np.linalg.norm(np.array([[float(v) for v in row] for row in P]), 2))
    nI = float(np.linalg.norm(np.array([[float(v) for v in row] for row in Pinv]), 2))
    EF = math.sqrt(sum(float(e) ** 2 for row in EP for e in row))
    ern, zn, rhon = _norm2(er), _norm2(z), _norm2(rho)
    E = EF + k * gam(3 * k + 1) * nP
    w = math.sqrt(max(float(sum((a * b for a, b in zip(r, mean)), _ZERO)), 0.0))
    b_mean = nI * (ern + E * _norm2(mean))
    b_l = nI ** 1.5 * (EF + k * gam(k + 1) * nP) * zn / math.sqrt(2.0)
    b_sub = gam(k) * math.sqrt(k * nP * nI) * _norm2(xz)
    b_add = math.sqrt(nI) * U * (w + zn)
    b_z = math.sqrt(nI) * C_Z * U * rhon
    rz = _norm2([abs(float(a)) + abs(float(b)) for a, b in zip(r, z)])
    b_lit = nI * (ern + U * rz + C_Z * U * rhon + E * _norm2(x_lit))
    return {"x": x, "x_lit": x_lit, "bound": 2.0 * (b_mean + b_l + b_sub + b_add + b_z), "bound_lit": 2.0 * b_lit, "cond": nP * nI,
            "norm": nP, "norm_inv": nI, "xinf": max(abs(float(v)) for v in x), "xinf_lit": max(abs(float(v)) for v in x_lit)}


def _panel_terms(beta, v):
    """Of one panel: beta and 1 / v as Decimals."""
    b = _rows(beta)
    iv = [_ONE / x for x in _vec(v)]
    return b, iv


def _new(shape, fill=np.nan):
    return np.full(shape, fill, dtype=np.float64)


def factors(y, beta, v, alpha, *, seed, series_offset, it):
    """y [N][T][p], beta [N][p][k], v [N][p], alpha [N][k][T+1] or None.  -> dict of arrays: f, f_lo, f_lit, f_lit_lo [N][k][T] (NaN where
    a component of y_t is not finite); bound, bound_lit, cond, norm, norm_inv, xinf, xinf_lit [N][T] (NaN likewise); mag_P [N] and mag_r
    [N][T]: the largest entries of |beta|^T D |beta| and of |beta|^T D |y_t|; rho [N][T][k]: the radius of every normal."""
    getcontext().prec = PREC
    N, T, p = y.shape
    k = beta.shape[2]
    series = (series_offset + np.arange(N))[:, None, None]
    comp, att = np.arange(T)[None, :, None], np.arange(k)[None, None, :]
    z = fr.normals(seed, series, it, comp, att)
    rho = radii(fr.KEY_FSV, seed, series, it, comp, att)
    out = {key: _new((N, k, T)) for key in ("f", "f_lo", "f_lit", "f_lit_lo")}
    out.update({key: _new((N, T)) for key in ("bound", "bound_lit", "cond", "norm", "norm_inv", "xinf", "xinf_lit", "mag_r")})
    out["mag_P"], out["rho"] = _new((N,)), rho
    g2 = gam(p + 2)
    for n in range(N):
        b, iv = _panel_terms(beta[n], v[n])
        A = [[sum((b[i][a] * iv[i] * b[i][c] for i in range(p)), _ZERO) for c in range(k)] for a in range(k)]
        Aabs = [[float(sum((abs(b[i][a] * b[i][c]) * iv[i] for i in range(p)), _ZERO)) for c in range(k)] for a in range(k)]
        out["mag_P"][n] = max(max(row) for row in Aabs)
        for t in range(T):
            if not np.isfinite(y[n, t]).all():
                continue
            yt = _vec(y[n, t])
            d = [_ONE] * k if alpha is None else [(-_dec(alpha[n, j, t + 1])).exp() for j in range(k)]
            P = [[A[a][c] + (d[a] if a == c else _ZERO) for c in range(k)] for a in range(k)]
            r = [sum((b[i][a] * iv[i] * yt[i] for i in range(p)), _ZERO) for a in range(k)]
            rabs = [float(sum((abs(b[i][a] * yt[i]) * iv[i] for i in range(p)), _ZERO)) for a in range(k)]
            EP = [[g2 * Aabs[a][c] + ((U * float(P[a][a]) + 3.0 * U * float(d[a])) if a == c else 0.0) for c in range(k)] for a in range(k)]
            s = solve(P, r, z[n, t], rho[n, t], EP, [g2 * m for m in rabs])
            for j in range(k):
                out["f"][n, j, t], out["f_lo"][n, j, t] = _split(s["x"][j])
                out["f_lit"][n, j, t], out["f_lit_lo"][n, j, t] = _split(s["x_lit"][j])
            for key in ("bound", "bound_lit", "cond", "norm", "norm_inv", "xinf", "xinf_lit"):
                out[key][n, t] = s[key]
            out["mag_r"][n, t] = max(rabs)
    return out


def impute(r, beta, v, alpha, *, seed, series_offset, it):
    """r [N][T][p] (not finite = missing), beta, v, alpha as above.  -> dict: r, r_lo [N][T][p]: the input where nothing is drawn (lo = 0),
    the 50-digit draw at the missing components of a partially missing time; bound [N][T][p] (0 where copied); part [N][T] bool; cond,
    bound_f, xinf [N][T] of the factor system of a partially missing time (xinf: the largest of |f*| and the drawn |r*|)."""
    getcontext().prec = PREC
    N, T, p = r.shape
    k = beta.shape[2]
    series = (series_offset + np.arange(N))[:, None, None]
    comp = np.arange(T)[None, :, None]
    z = dr.normals(seed, series, it, comp, np.arange(k)[None, None, :])
    rho = radii(dr.KEY_DLMFSV, seed, series, it, comp, np.arange(k)[None, None, :])
    zi = dr.normals(seed, series, it, comp, 8 + np.arange(p)[None, None, :])
    rhoi = radii(dr.KEY_DLMFSV, seed, series, it, comp, 8 + np.arange(p)[None, None, :])
    obs = np.isfinite(r)
    part = obs.any(axis=2) & ~obs.all(axis=2)
    out = {"r": np.array(r, dtype=np.float64), "r_lo": np.zeros((N, T, p)), "bound": np.zeros((N, T, p)), "part": part}
    out.update({key: _new((N, T)) for key in ("cond", "bound_f", "xinf")})
    g2 = gam(p + 2)
    for n in range(N):
        b, iv = _panel_terms(beta[n], v[n])
        sd = [x.sqrt() for x in _vec(v[n])]
        for t in np.nonzero(part[n])[0]:
            o = [i for i in range(p) if obs[n, t, i]]
            yt = {i: _dec(r[n, t, i]) for i in o}
            d = [(-_dec(alpha[n, j, t + 1])).exp() for j in range(k)]
            P = [[sum((b[i][a] * iv[i] * b[i][c] for i in o), _ZERO) + (d[a] if a == c else _ZERO) for c in range(k)] for a in range(k)]
            Aabs = [[float(sum((abs(b[i][a] * b[i][c]) * iv[i] for i in o), _ZERO)) for c in range(k)] for a in range(k)]
            c = [sum((b[i][a] * iv[i] * yt[i] for i in o), _ZERO) for a in range(k)]
            cabs = [float(sum((abs(b[i][a] * yt[i]) * iv[i] for i in o), _ZERO)) for a in range(k)]
            EP = [[g2 * Aabs[a][q] + ((U * float(P[a][a]) + 3.0 * U * float(d[a])) if a == q else 0.0) for q in range(k)] for a in range(k)]
            s = solve(P, c, z[n, t], rho[n, t], EP, [g2 * m for m in cabs])
            xinf = s["xinf"]
            for i in range(p):
                if obs[n, t, i]:
                    continue
                zz = _dec(zi[n, t, i])
                val = sum((b[i][j] * s["x"][j] for j in range(k)), _ZERO) + sd[i] * zz
                mag = float(sum((abs(b[i][j] * s["x"][j]) for j in range(k)), _ZERO) + sd[i] * abs(zz))
                out["r"][n, t, i], out["r_lo"][n, t, i] = _split(val)
                out["bound"][n, t, i] = 2.0 * (_norm2(b[i]) * 0.5 * s["bound"] + gam(k + 2) * mag + float(sd[i]) * C_Z * U * rhoi[n, t, i])
                xinf = max(xinf, abs(float(val)))
            out["cond"][n, t], out["bound_f"][n, t], out["xinf"][n, t] = s["cond"], s["bound"], xinf
    return out


def loadings(y, f, beta, prior, *, seed, series_offset, it):
    """y [N][T][p], f [N][k][T], beta [N][p][k] (the old loadings), prior: the dict of fsv_restatement.fsv_prior.  A time is counted when
    y_t and f_t are finite.  -> dict: beta, beta_lo [N][p][k] (the fixed entries too), v, v_lo [N] (sigma^2), bound_v [N], bound [N][p]
    (of row i's draw; 0 for row 0), cond, xinf [N][p] (NaN for row 0), empty [N] bool (no counted time: nothing else is filled in),
    S_abs, c_abs, ssy_abs [N]: the largest absolute sums.

    The bounds.  The device's sums are of n <= T terms (S, c) and of n p terms (ssy), in its own order; any order of summation is within
    gamma_{m-1} of the sum of the absolute terms, the products add one rounding: gamma_{Tp+2} on the absolute sums
    S_abs = sum |f_a f_b|, c_abs = sum |f_a y_i|, ssy_abs = sum (|y_ti| + sum_j |beta_ij f_jt|)^2 covers each (the residual's own k + 1
    roundings enter ssy twice, 2 (k + 1) u ssy_abs at first order: inside the final doubling whenever T p >= 2 k - 1, which every case of
    the table satisfies).  sigma^2 = scale' / g: relative error
        e_s = gamma_{Tp+2} (ssy_abs / 2) / scale' + 2 u + e_g        (the addition into scale' and the division)
    (literal: ssy_abs / (2 p)), e_g the relative difference of the device's unit Gamma from the restatement's: g = dd w^3, w = 1 + cc x,
    x a normal of radius at most RHO_MAX: e_g = 3 cc C_Z u RHO_MAX / w + 8 u with w = (g / dd)^(1/3) (shape' >= 1 here: no boost).
    |sigma^2 - sigma^2*| <= 2 e_s sigma^2*.  The loading rows inherit e_s:
        |E_P|_ab <= (gamma_{Tp+2} S_abs_ab + (e_s + u) |S_ab|) / sigma^2 + [a == b] (u P_aa + 2 u / s^2)        (literal: 2 u s^2)
        |e_r|_a  <= (gamma_{Tp+2} (c_abs_ia + S_abs_ai) + (e_s + 2 u) (|c_ia| + |S_ai|)) / sigma^2 + u |r_a| + 3 u |m| / s^2
    and the solve adds what the module docstring derives."""
    getcontext().prec = PREC
    N, T, p = y.shape
    k = beta.shape[2]
    lit = bool(prior["literal"])
    counted = np.isfinite(y).all(axis=2) & np.isfinite(f).all(axis=1)
    nobs = counted.sum(axis=1)
    series = series_offset + np.arange(N)
    out = {"beta": _new((N, p, k)), "beta_lo": np.zeros((N, p, k)), "v": _new((N,)), "v_lo": np.zeros(N), "bound_v": _new((N,)),
           "bound": np.zeros((N, p)), "cond": _new((N, p)), "xinf": _new((N, p)), "empty": nobs == 0,
           "S_abs": _new((N,)), "c_abs": _new((N,)), "ssy_abs": _new((N,))}
    gs = gam(T * p + 2)
    sd2 = _dec(prior["beta_sd"]) * _dec(prior["beta_sd"])
    pdiag = sd2 if lit else _ONE / sd2
    pmean = _ZERO if lit else _dec(prior["beta_mean"]) / sd2
    live = np.nonzero(nobs > 0)[0]
    shape = prior["sigma_shape"] + (0.5 * nobs if lit else 0.5 * (nobs * float(p)))
    g = np.full(N, np.nan)
    if live.size:
        g[live] = fr.gamma_units(shape[live], seed, series[live], it, fr.FSV_SLOT_SIGMA, fr.KEY_FSV)
    for n in live:
        b = _rows(beta[n])
        times = np.nonzero(counted[n])[0]
        ft = [_vec(f[n, :, t]) for t in times]
        yt = [_vec(y[n, t]) for t in times]
        S = [[sum((x[a] * x[c] for x in ft), _ZERO) for c in range(k)] for a in range(k)]
        Sabs = [[sum((abs(x[a] * x[c]) for x in ft), _ZERO) for c in range(k)] for a in range(k)]
        c = [[sum((x[a] * w[i] for x, w in zip(ft, yt)), _ZERO) for a in range(k)] for i in range(p)]
        cabs = [[sum((abs(x[a] * w[i]) for x, w in zip(ft, yt)), _ZERO) for a in range(k)] for i in range(p)]
        ssy = sum(((w[i] - sum((b[i][j] * x[j] for j in range(k)), _ZERO)) ** 2 for x, w in zip(ft, yt) for i in range(p)), _ZERO)
        ssy_abs = sum(((abs(w[i]) + sum((abs(b[i][j] * x[j]) for j in range(k)), _ZERO)) ** 2 for x, w in zip(ft, yt) for i in range(p)), _ZERO)
        half = _ONE / (2 * p) if lit else _ONE / 2
        scale = _dec(prior["sigma_scale"]) + ssy * half
        s2 = scale / _dec(g[n])
        assert shape[n] >= 1.0
        dd = shape[n] - 1.0 / 3.0
        cc = 1.0 / math.sqrt(9.0 * dd)
        e_g = 3.0 * cc * C_Z * U * RHO_MAX / (g[n] / dd) ** (1.0 / 3.0) + 8.0 * U
        e_s = gs * float(ssy_abs * half / scale) + 2.0 * U + e_g
        out["v"][n], out["v_lo"][n] = _split(s2)
        out["bound_v"][n] = 2.0 * e_s * float(s2)
        out["S_abs"][n], out["c_abs"][n], out["ssy_abs"][n] = float(max(max(row) for row in Sabs)), float(max(max(row) for row in cabs)), float(ssy_abs)
        s2f = float(s2)
        for i in range(p):
            for j in range(k):
                out["beta"][n, i, j] = 1.0 if j == i else 0.0
            q = min(i, k)
            if q == 0:
                continue
            P = [[S[a][e] / s2 + (pdiag if a == e else _ZERO) for e in range(q)] for a in range(q)]
            own = [c[i][a] - (S[a][i] if (i < k and not lit) else _ZERO) for a in range(q)]
            own_abs = [cabs[i][a] + (Sabs[a][i] if (i < k and not lit) else _ZERO) for a in range(q)]
            own_mag = [abs(c[i][a]) + (abs(S[a][i]) if (i < k and not lit) else _ZERO) for a in range(q)]
            r = [o / s2 + pmean for o in own]
            EP = [[(gs * float(Sabs[a][e]) + (e_s + U) * abs(float(S[a][e]))) / s2f + ((U * float(P[a][a]) + 2.0 * U * float(pdiag)) if a == e else 0.0)
                   for e in range(q)] for a in range(q)]
            er = [(gs * float(own_abs[a]) + (e_s + 2.0 * U) * float(own_mag[a])) / s2f + U * abs(float(r[a])) + 3.0 * U * abs(float(pmean)) for a in range(q)]
            att = np.arange(q)
            z = fr.normals(seed, series[n], it, fr.FSV_SLOT_ROW0 - i, att)
            rho = radii(fr.KEY_FSV, seed, series[n], it, fr.FSV_SLOT_ROW0 - i, att)
            s = solve(P, r, z, rho, EP, er)
            x = s["x_lit"] if lit else s["x"]
            for j in range(q):
                out["beta"][n, i, j], out["beta_lo"][n, i, j] = _split(x[j])
            out["bound"][n, i] = s["bound_lit"] if lit else s["bound"]
            out["cond"][n, i], out["xinf"][n, i] = s["cond"], s["xinf_lit"] if lit else s["xinf"]
    return out


def variance(beta, v, alpha):
    """beta [N][p][k], v [N][p], alpha [N][k][T+1].  -> dict: V, V_lo, bound [N][T][p][p]."""
    getcontext().prec = PREC
    N, p, k = beta.shape
    T = alpha.shape[2] - 1
    out = {key: _new((N, T, p, p)) for key in ("V", "V_lo", "bound")}
    c = 4.0 * (k + 4) * U
    for n in range(N):
        b, vd = _rows(beta[n]), _vec(v[n])
        bb = [[[b[i][l] * b[j][l] for l in range(k)] for j in range(i + 1)] for i in range(p)]
        for t in range(T):
            e = [_dec(alpha[n, l, t + 1]).exp() for l in range(k)]
            for i in range(p):
                for j in range(i + 1):
                    val = sum((x * w for x, w in zip(bb[i][j], e)), _ZERO)
                    mag = sum((abs(x) * w for x, w in zip(bb[i][j], e)), _ZERO)
                    if i == j:
                        val, mag = val + vd[i], mag + vd[i]
                    hi, lo = _split(val)
                    out["V"][n, t, i, j] = out["V"][n, t, j, i] = hi
                    out["V_lo"][n, t, i, j] = out["V_lo"][n, t, j, i] = lo
                    out["bound"][n, t, i, j] = out["bound"][n, t, j, i] = c * float(mag)
    return out


def _affine(x, coef, prev):
    """x [N][T][m] minus sum_j coef[t][j][i] prev[n][t][j]: (hi, lo, bound) [N][T][m]; coef [T][d][m] (or [d][m]), prev [N][T][d]."""
    getcontext().prec = PREC
    N, T, m = x.shape
    d = prev.shape[2]
    hi, lo, bound = _new((N, T, m)), _new((N, T, m)), _new((N, T, m))
    c = 2.0 * (d + 2) * U
    table = coef.ndim == 3
    C = None if table else [list(col) for col in zip(*_rows(coef))]                 # [m][d]
    for t in range(T):
        Ct = [list(col) for col in zip(*_rows(coef[t]))] if table else C
        for n in range(N):
            th = _vec(prev[n, t])
            for i in range(m):
                if x[n, t, i] != x[n, t, i]:
                    continue
                terms = [a * w for a, w in zip(Ct[i], th)]
                xv = _dec(x[n, t, i])
                hi[n, t, i], lo[n, t, i] = _split(xv - sum(terms, _ZERO))
                bound[n, t, i] = c * float(abs(xv) + sum((abs(w) for w in terms), _ZERO))
    return hi, lo, bound


def center(y, theta, F):
    """y [N][T][p] (a NaN stays NaN), theta [N][T+1][d], F [T][d][p] or [d][p].  -> dict: r, r_lo, bound [N][T][p]."""
    hi, lo, bound = _affine(y, np.asarray(F), theta[:, 1:])
    return {"r": hi, "r_lo": lo, "bound": bound}


def innovations(theta, G):
    """theta [N][T+1][d], G [d][d] (w_t = theta_{t+1} - G theta_t).  -> dict: w, w_lo, bound [N][T][d]."""
    hi, lo, bound = _affine(theta[:, 1:], np.asarray(G).T, theta[:, :-1])
    return {"w": hi, "w_lo": lo, "bound": bound}


# ---- the case table and its inputs (shared by the host and the GPU test) ----------------------------------------------------------------
SEED, OFFSET, ITER = 0x1234_5678_9ABC, 7, 3          # tests/test_factorsv_gpu.py's
REL_MAX = 1e-6                                        # no asserted bound of a draw may exceed this, relative to ||x*||_inf of its system
_T4 = (2, 255, 256, 257)
# (T, p, k).  factors, impute: one lane per time, 256 times per block
SOLVE_CASES = [(_T4[(k - 1) % 4], k, k) for k in range(1, 9)] + [(5, 64, 1), (6, 9, 4), (6, 14, 5), (6, 20, 6), (6, 27, 7), (6, 35, 8), (6, 64, 8)]
# loadings: a row per lane, S on the lanes < k (k + 1) / 2, time t on wave t mod 4.  (T, p, k, N): N = 3 has a panel without a counted time
_NS = [(k * (k + 1) // 2 - 1 + e, k) for k in range(4, 9) for e in (0, 1)]
LOADINGS_CASES = ([(3, k, k, 3 if k == 4 else 2) for k in range(1, 9)] + [(5 + i % 5, p, k, 2) for i, (p, k) in enumerate(_NS)] + [(2, 64, 8, 2)])
# variance: chunks of 64 times; p^2 against 256.  (3, 3, 3) is not a layout edge: it launches k = 3
VARIANCE_CASES = ([(T, p, min(p, 4 + (3 * a + b) % 4)) for a, p in enumerate((1, 2, 11, 15, 16, 17)) for b, T in enumerate((63, 64, 65))]
                  + [(3, 64, 8), (129, 5, 5), (3, 3, 3)])
CENTER_CASES = [(33, 64, 64, False), (2049, 1, 1, False), (410, 5, 7, True)]          # (T, p, d, a table of F_t)
INNOVATION_CASES = [(33, 64), (2049, 1), (158, 13)]                                    # (T, d)
# The wide ranges: alpha uniform on [-a, a], v log-uniform on 10^[lo, hi], the free loadings uniform on [-b, b].  Chosen per kernel so that
# every bound stays below REL_MAX (the factor systems then reach condition numbers of 1e5 to 1e6); the well-conditioned set is that of
# tests/test_factorsv_gpu.py.
WELL = dict(alpha=1.0, v=(math.log10(0.3), math.log10(1.5)), beta=0.8)
WIDE = {"factors": dict(alpha=8.0, v=(-3.0, 2.0), beta=3.0), "impute": dict(alpha=4.0, v=(-2.0, 2.0), beta=3.0),
        "loadings": dict(alpha=3.0, v=(-0.5, 1.5), beta=2.0)}
WIDE_PRIOR = dict(beta=(0.3, 3.0), sigma=(4.0, 1.5))


def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _model(rng, N, T, p, k, rg):
    beta = np.zeros((N, p, k))
    fm = fr.free_mask(p, k)
    beta[:, fm] = rng.uniform(-rg["beta"], rg["beta"], (N, int(fm.sum())))
    beta[:, np.arange(k), np.arange(k)] = 1.0
    v = 10.0 ** rng.uniform(rg["v"][0], rg["v"][1], (N, p))
    alpha = rng.uniform(-rg["alpha"], rg["alpha"], (N, k, T + 1))
    f = rng.standard_normal((N, k, T)) * np.exp(0.5 * alpha[:, :, 1:])
    y = np.einsum("nij,njt->nti", beta, f) + np.sqrt(v)[:, None, :] * rng.standard_normal((N, T, p))
    return beta, v, alpha, f, y


@functools.lru_cache(maxsize=None)
def solve_inputs(kind, case, wide):
    """{"y", "beta", "v", "alpha"} of a factors or an impute case (N = 2), read-only.  From T = 8 on one wholly missing time per panel; for
    impute every component is missing with probability 0.15 besides (p = 1 has no partially missing time: the call copies)."""
    T, p, k = case
    N = 2
    rng = np.random.default_rng([T, p, k, int(wide), kind == "impute"])
    beta, v, alpha, _, y = _model(rng, N, T, p, k, WIDE[kind] if wide else WELL)
    if kind == "impute":
        y[rng.random((N, T, p)) < 0.15] = np.nan
    if T >= 8:
        y[np.arange(N), rng.integers(0, T, N), :] = np.nan
    return _freeze({"y": y, "beta": beta, "v": v, "alpha": alpha})


def loadings_missing(index, n, T):
    """The wholly missing time of panel n of loadings case `index` (None below T = 8): the cases with T >= 8 put one on every wave."""
    return None if T < 8 else (2 * index + n) % 4 + 4 * (index % 2)


@functools.lru_cache(maxsize=None)
def loadings_inputs(index, wide):
    """{"y", "f", "beta", "prior"} of loadings case `index`, read-only: sigma^2 one value per panel, f NaN at the missing time, the last
    panel of N = 3 without a counted time."""
    T, p, k, N = LOADINGS_CASES[index]
    rng = np.random.default_rng([index, T, p, k, int(wide)])
    rg = dict(WIDE["loadings"] if wide else WELL)
    beta, v, alpha, f, y = _model(rng, N, T, p, k, rg)
    s2 = v[:, :1]
    y = np.einsum("nij,njt->nti", beta, f) + np.sqrt(s2)[:, None, :] * rng.standard_normal((N, T, p))
    for n in range(N):
        t = loadings_missing(index, n, T)
        if t is not None:
            y[n, t] = np.nan
            f[n, :, t] = np.nan
    if N == 3:
        y[2] = np.nan
        f[2] = np.nan
    prior = fr.fsv_prior(0, **WIDE_PRIOR) if wide else fr.fsv_prior(0)
    return _freeze({"y": y, "f": f, "beta": beta, "v": np.broadcast_to(s2, (N, p)).copy(), "prior": prior})


@functools.lru_cache(maxsize=None)
def variance_inputs(case):
    T, p, k = case
    rng = np.random.default_rng([T, p, k, 5])
    beta, v, alpha, _, _ = _model(rng, 2, T, p, k, dict(alpha=4.0, v=(-2.0, 2.0), beta=3.0))
    return _freeze({"beta": beta, "v": v, "alpha": alpha})


@functools.lru_cache(maxsize=None)
def center_inputs(case):
    T, p, d, table = case
    rng = np.random.default_rng([T, p, d, 6])
    y = rng.standard_normal((2, T, p)) * 3.0
    y[rng.random((2, T, p)) < 0.1] = np.nan
    return _freeze({"y": y, "theta": rng.standard_normal((2, T + 1, d)) * 10.0 ** rng.uniform(-2, 2, (2, T + 1, d)),
                    "F": rng.standard_normal((T, d, p) if table else (d, p))})


@functools.lru_cache(maxsize=None)
def innovation_inputs(case):
    T, d = case
    rng = np.random.default_rng([T, d, 7])
    return _freeze({"theta": rng.standard_normal((2, T + 1, d)) * 10.0 ** rng.uniform(-2, 2, (2, T + 1, d)), "G": rng.standard_normal((d, d))})


KW = dict(seed=SEED, series_offset=OFFSET, it=ITER)


def ratio_factors(ref, got, literal):
    """(the largest error / bound, the largest bound / ||x*||_inf) of factors `got` [N][k][T]; the NaN patterns must agree."""
    hi, lo = (ref["f_lit"], ref["f_lit_lo"]) if literal else (ref["f"], ref["f_lo"])
    bound, xinf = (ref["bound_lit"], ref["xinf_lit"]) if literal else (ref["bound"], ref["xinf"])
    got = np.asarray(got)
    assert np.array_equal(np.isnan(got), np.isnan(hi))
    m = ~np.isnan(bound)
    if not m.any():
        return 0.0, 0.0
    err = np.max(error(got, hi, lo), axis=1)
    return float((err[m] / bound[m]).max()), float((bound[m] / xinf[m]).max())


def ratio_impute(ref, got):
    got = np.asarray(got)
    assert np.array_equal(np.isnan(got), np.isnan(ref["r"]))
    drawn = ref["bound"] > 0.0
    same = ~drawn & ~np.isnan(ref["r"])
    assert np.array_equal(got[same], ref["r"][same])                                   # what is not drawn is copied bit for bit
    if not drawn.any():
        return 0.0, 0.0
    err = error(got, ref["r"], ref["r_lo"])
    rel = (ref["bound"].max(axis=2) / ref["xinf"])[ref["part"]]
    return float((err[drawn] / ref["bound"][drawn]).max()), float(rel.max())


def ratio_loadings(ref, beta, v):
    """(error / bound of the rows, of sigma^2, the largest bound / ||x*||_inf) over the panels with a counted time."""
    beta, v = np.asarray(beta), np.asarray(v)
    live = ~ref["empty"]
    assert (v[live] == v[live][:, :1]).all()
    k = beta.shape[2]
    fixed = ~fr.free_mask(beta.shape[1], k)
    assert np.array_equal(beta[live][:, fixed], ref["beta"][live][:, fixed])           # the unit diagonal and the zeros above it
    err = error(beta, ref["beta"], ref["beta_lo"]).max(axis=2)[live][:, 1:]
    rb = float((err / ref["bound"][live][:, 1:]).max()) if err.size else 0.0
    rv = float((error(v[:, 0], ref["v"], ref["v_lo"])[live] / ref["bound_v"][live]).max())
    rel = float((ref["bound"][live][:, 1:] / ref["xinf"][live][:, 1:]).max()) if err.size else 0.0
    return rb, rv, rel


# ---- the references of the table, computed once per process -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def factors_ref(case, wide, with_alpha):
    x = solve_inputs("factors", case, wide)
    return factors(x["y"], x["beta"], x["v"], x["alpha"] if with_alpha else None, **KW)


@functools.lru_cache(maxsize=None)
def impute_ref(case, wide):
    x = solve_inputs("impute", case, wide)
    return impute(x["y"], x["beta"], x["v"], x["alpha"], **KW)


@functools.lru_cache(maxsize=None)
def loadings_ref(index, wide, literal):
    x = loadings_inputs(index, wide)
    return loadings(x["y"], x["f"], x["beta"], dict(x["prior"], literal=literal), **KW)


def not_pd_inputs():
    """k = p = 2, beta_10 = 1e8, v = 1 and alpha_{1,t+1} = 700 at time "t" = 2 of panel 0 (T = 5), beside clean times and a clean panel: the
    second pivot of P_t, 1 + e^-700 - 1e16 / (1 + 1e16 + e^-alpha_0), rounds to zero in doubles.  "clean": the same with alpha = 0 there."""
    rng = np.random.default_rng(41)
    N, T = 2, 5
    beta = np.zeros((N, 2, 2))
    beta[:, 0, 0] = beta[:, 1, 1] = 1.0
    beta[0, 1, 0], beta[1, 1, 0] = 1e8, 0.5
    clean = rng.uniform(-1.0, 1.0, (N, 2, T + 1))
    alpha = clean.copy()
    alpha[0, 1, 3] = 700.0
    y = rng.standard_normal((N, T, 2))
    part = y.copy()
    part[0, 2, 0] = np.nan          # observed at that time: the component with the loading 1e8
    part[1, 1, 1] = np.nan
    return {"y": y, "part": part, "beta": beta, "v": np.ones((N, 2)), "alpha": alpha, "clean": clean, "t": 2}


# ---- the perturbed inputs that the bounds must catch ------------------------------------------------------------------------------------------
def zero_last_free(beta):
    """beta with the last row's last free entry zeroed."""
    b = beta.copy()
    p, k = b.shape[1:]
    b[:, p - 1, min(p - 1, k) - 1] = 0.0
    return b


def through_float32(a):
    return a.astype(np.float32).astype(np.float64)


def extremes(conds):
    """The keys of the smallest and the largest value of `conds`."""
    order = sorted(conds, key=conds.get)
    return order[0], order[-1]
