"""NumPy restatement of the two kernels of bayesian_dlms_amd/csrc/dlm_fsv_forecast.hip and of the composition the three forecast drivers
make of them (bayesian_dlms_amd/_dlmfsv.py: forecast).  The Philox counters and the normal are
tests/sampler_restatement.py's, the variance stream is tests/dlmfsv_restatement.py's.

  sv_paths          k_sv_paths, operation for operation: the GPU test holds the kernel to it draw for draw
  mixture_summary   k_mixture_moments and k_mixture_quantiles: the same sums (in NumPy's order -- the GPU test holds both to mpmath within the
                    summation bound, not to each other bit for bit) and the same stopping rule (the root of the mixture's CDF bracketed to
                    adjacent doubles)
  compose           the drivers: the training filter per draw, the paths from alpha_T, the stream, the Kalman forecast, one summary per panel

`mutant` injects ONE mistake; the host tests prove that each check rejects each of them:
  "step"      alpha_h = phi alpha_{h-1} + sigma z in place of mu + phi (alpha_{h-1} - mu) + sigma z
  "variance"  sigma_eta^2 where the standard deviation belongs
  "start"     a stationary start in place of alpha0
  "cov"       the covariance without the Cov(f) term (the average of the Q_c alone)
  "average"   the quantiles of the ONE Gaussian with the mixture's mean and variance in place of the mixture's"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sampler_restatement import gibbs_rand  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402

KEY_SVPATH = 0x53500000
SLOT_START = 0
TWO_PI = 6.283185307179586476925286766559
MUTANTS = ("step", "variance", "start", "cov", "average")
MAX_EVALS = 3500


# ---- k_sv_paths ------------------------------------------------------------------------------------------------------------------------
def path_normals(seed, series, it, slots, R, j):
    """draw_normal on DLM_KEY_SVPATH + j for the slots [S] and the paths 0 .. R - 1 of one series -> [R][S]."""
    slots = np.asarray(slots, dtype=np.int64).reshape(1, -1)
    r = np.arange(R, dtype=np.int64).reshape(-1, 1)
    u1, u2 = gibbs_rand(seed, int(series), it, np.broadcast_to(slots, (R, slots.shape[1])), np.broadcast_to(r, (R, slots.shape[1])), 0, KEY_SVPATH + j)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI * u2)


def sv_paths(sv, alpha0, H, R, *, seed=0, series_offset=0, iteration=0, mutant=None):
    """sv [N][k][3], alpha0 [N][k] or None -> (alpha [N][R][k][H+1], status [N])."""
    sv = np.asarray(sv, dtype=np.float64)
    N, k = sv.shape[:2]
    alpha = np.full((N, R, k, H + 1), np.nan)
    status = np.zeros(N, np.int32)
    if mutant == "start":
        alpha0 = None
    for n in range(N):
        a0 = None if alpha0 is None else np.asarray(alpha0, dtype=np.float64)[n]
        if not np.isfinite(sv[n]).all() or (a0 is not None and not np.isfinite(a0).all()):
            status[n] = _lib.ST_NONFINITE
            continue
        if not ((np.abs(sv[n, :, 0]) < 1.0).all() and (sv[n, :, 2] > 0.0).all()):
            status[n] = _lib.ST_NOT_PD
            continue
        for j in range(k):
            phi, mu, sg = sv[n, j]
            if mutant == "variance":
                sg = sg * sg
            z = path_normals(seed, series_offset + n, iteration, np.arange(H + 1), R, j)          # slot 0: the start; slot h: step h
            a = np.full(R, a0[j]) if a0 is not None else mu + sg / math.sqrt(1.0 - phi * phi) * z[:, SLOT_START]
            alpha[n, :, j, 0] = a
            for h in range(1, H + 1):
                a = (phi * a + sg * z[:, h]) if mutant == "step" else (mu + phi * (a - mu) + sg * z[:, h])
                alpha[n, :, j, h] = a
    return alpha, status


# ---- k_mixture_moments, k_mixture_quantiles ----------------------------------------------------------------------------------------------
def _erfc(x):
    from scipy.special import erfc
    return erfc(x)


def mixture_cdf(x, f, s):
    """F(x) and the density's sum as the kernel forms them: f, s = sqrt(2 Q_ii) [C]."""
    z = (x - f) / s
    ec = 0.5 * _erfc(np.abs(z))
    return float(np.sum(np.where(z > 0.0, 1.0 - ec, ec)) / f.size), float(np.sum(np.exp(-z * z) / s) / f.size * 0.56418958354775628695)


def mixture_quantile(f, q, prob):
    """The stopping rule of k_mixture_quantiles on the components (f [C], variances q [C]): the bracket, the overshot Newton step, the
    midpoint where it leaves the bracket or two evaluations in a row did not halve it; an exact hit or hi next to lo ends it."""
    from scipy.special import ndtri
    f, q = np.asarray(f, dtype=np.float64), np.asarray(q, dtype=np.float64)
    s = np.sqrt(2.0 * q)
    pad = (abs(float(ndtri(prob))) + 1.0) * float(s.max())
    lo, hi = float(f.min()) - pad, float(f.max()) + pad
    x, res, slow = lo + 0.5 * (hi - lo), hi, 0
    for _ in range(MAX_EVALS):
        F, D = mixture_cdf(x, f, s)
        if F == prob:
            return x
        width = hi - lo
        if F < prob:
            lo = x
        else:
            hi = x
        res = hi
        if not np.nextafter(lo, np.inf) < hi:
            break
        slow = 0 if hi - lo <= 0.5 * width else slow + 1
        with np.errstate(all="ignore"):
            step = np.float64(F - prob) / np.float64(D)
            xn = float(x - (step + 1e-3 * step))
        if slow >= 2 or not lo < xn < hi:
            xn, slow = lo + 0.5 * (hi - lo), 0
        if not lo < xn < hi:
            xn = float(np.nextafter(lo, np.inf))
        x = xn
    return res


def mixture_summary(f, Q, probs=(), *, mutant=None):
    """f [N][C][H][p] or None (zero means), Q [N][C][H][p][p] -> (mean [N][H][p], cov [N][H][p][p], quant [N][H][p][nq], status [N])."""
    Q = np.asarray(Q, dtype=np.float64)
    N, C, H, p = Q.shape[:4]
    f = np.zeros((N, C, H, p)) if f is None else np.asarray(f, dtype=np.float64)
    probs = [float(x) for x in probs]
    with np.errstate(all="ignore"):
        mean = f.sum(axis=1) / C
        second = Q if mutant == "cov" else Q + f[..., :, None] * f[..., None, :]
        cov = second.sum(axis=1) / C - (0.0 if mutant == "cov" else mean[..., :, None] * mean[..., None, :])
        iu = np.triu_indices(p, 1)
        cov[..., iu[1], iu[0]] = cov[..., iu[0], iu[1]]                                  # the kernel reads (lo, hi) for both halves
    quant = np.full((N, H, p, len(probs)), np.nan)
    status = np.zeros(N, np.int32)
    diag = np.diagonal(Q, axis1=3, axis2=4)                                              # [N][C][H][p]
    for n in range(N):
        for h in range(H):
            for i in range(p):
                qi, fi = diag[n, :, h, i], f[n, :, h, i]
                bad = (0 if ((qi > 0.0) & (qi < np.inf)).all() else _lib.ST_NOT_PD) | (0 if np.isfinite(fi).all() else _lib.ST_NONFINITE)
                if bad:
                    status[n] |= bad
                    mean[n, h, i] = np.nan
                    cov[n, h, i, :] = np.nan
                    cov[n, h, :, i] = np.nan
                    continue
                for iq, prob in enumerate(probs):
                    if mutant == "average":
                        from scipy.special import ndtri
                        quant[n, h, i, iq] = mean[n, h, i] + math.sqrt(cov[n, h, i, i]) * float(ndtri(prob))
                    else:
                        quant[n, h, i, iq] = mixture_quantile(fi, qi, prob)
    return mean, cov, quant, status


# ---- the drivers' composition ---------------------------------------------------------------------------------------------------------
def variance(beta, v, alpha):
    """k_dlmfsv_variance (tests/dlmfsv_restatement.py has it with its error bound): beta [R][q][k], v [R][q], alpha [R][k][H+1] -> [R][H][q][q]."""
    R, q, k = beta.shape
    H = alpha.shape[2] - 1
    e = np.exp(alpha[:, :, 1:])
    V = np.zeros((R, H, q, q))
    for l in range(k):
        V = V + (beta[:, :, None, l] * beta[:, None, :, l])[:, None] * e[:, l, :, None, None]
    idx = np.arange(q)
    V[:, :, idx, idx] = V[:, :, idx, idx] + v[:, None, :]
    return V


def model_tables(mat):
    """(F [T][d][p], G [d][d]) of a materialised model with one G."""
    d, p, T = mat.d, mat.p, mat.T
    F = np.stack([mat.F[t * mat.f_stride:t * mat.f_stride + d * p].reshape(p, d).T for t in range(T)])
    return F, mat.G.reshape(mat.n_g, d, d)[0].T


def kalman(F, G, m, Cm, V, W, y=None):
    """The Kalman filter of one row: F [T][d][p], V [T][p][p], W [T][d][d], y [T][p] or None (a pure forecast) -> (f [T][p], Q [T][p][p],
    m_T, C_T)."""
    T = F.shape[0]
    fs, Qs = [], []
    for t in range(T):
        a = G @ m
        Rm = G @ Cm @ G.T + W[t]
        ft = F[t].T @ a
        Qt = F[t].T @ Rm @ F[t] + V[t]
        fs.append(ft); Qs.append(0.5 * (Qt + Qt.T))
        if y is None:
            m, Cm = a, Rm
        else:
            K = np.linalg.solve(Qt, F[t].T @ Rm).T
            m = a + K @ (y[t] - ft)
            Cm = Rm - K @ Qt @ K.T
            Cm = 0.5 * (Cm + Cm.T)
    return np.array(fs), np.array(Qs), m, Cm


def compose(kind, draws, H, R, *, train=None, fore=None, ys=None, m0=None, C0=None, probs=(0.25, 0.75), seed=0, series_offset=0, mutant=None):
    """The drivers, restated.  kind: "fsv", "obs" (DlmFsv: the stream is V_t) or "sys" (DlmFsvSystem: W_t).  draws: {"beta" [M][N][q][k],
    "v" [M][N][q], "sv" [M][N][k][3], "alpha" [M][N][k][T+1], "static" [M][N][s] (the diagonal of W or V)}.  train / fore: (F, G) of the
    training period and of the horizon (model_tables).  Draw m is the Philox iteration.  -> mixture_summary's four over the M R components."""
    beta, v, sv, alpha = (np.asarray(draws[key], dtype=np.float64) for key in ("beta", "v", "sv", "alpha"))
    M, N, q, k = beta.shape
    fs = None if kind == "fsv" else np.zeros((N, M * R, H, fore[0].shape[2]))
    Qs = []
    for n in range(N):
        comps = []
        for m in range(M):
            paths, _ = sv_paths(sv[m, n:n + 1], alpha[m, n:n + 1, :, -1], H, R, seed=seed, series_offset=series_offset + n, iteration=m, mutant=mutant)
            S = variance(np.broadcast_to(beta[m, n], (R, q, k)), np.broadcast_to(v[m, n], (R, q)), paths[0])      # [R][H][q][q]
            if kind == "fsv":
                comps.append(S)
                continue
            static = np.diag(np.asarray(draws["static"], dtype=np.float64)[m, n])
            T = ys.shape[1]
            St = variance(beta[m, n][None], v[m, n][None], alpha[m, n][None])[0]                                   # the training stream [T][q][q]
            rep = lambda A, L: np.broadcast_to(A, (L,) + A.shape)
            Vt, Wt = (St, rep(static, T)) if kind == "obs" else (rep(static, T), St)
            _, _, mT, CT = kalman(train[0], train[1], m0, C0, Vt, Wt, ys[n])
            out = []
            for r in range(R):
                Vh, Wh = (S[r], rep(static, H)) if kind == "obs" else (rep(static, H), S[r])
                fr_, Qr, _, _ = kalman(fore[0], fore[1], mT, CT, Vh, Wh)
                fs[n, m * R + r] = fr_
                out.append(Qr)
            comps.append(np.array(out))
        Qs.append(np.concatenate(comps))
    return mixture_summary(fs, np.array(Qs), probs, mutant=mutant)


# ---- small cases both test files use ---------------------------------------------------------------------------------------------------
def toy_model(p, d):
    """A time-invariant DLM with a dense d x p observation matrix (p may exceed d) and a stable G."""
    from bayesian_dlms_amd.dlm import Dlm
    F = np.cos(0.7 * np.arange(d)[:, None] + 1.3 * np.arange(p)[None, :]) + (np.arange(d)[:, None] == np.arange(p)[None, :] % d)
    G = 0.9 * np.eye(d) + 0.1 * np.eye(d, k=1)
    return Dlm(lambda t: F.copy(), lambda dt: G.copy())


def toy_draws(kind, p, d, k, *, N=2, M=3, T=6, seed=1, beta0=False):
    """(mod, ys [N][T][p], draws, {"m0", "C0"}) for kind "obs" / "sys" (mod None and ys None for "fsv"): M kept draws of N panels; the
    static variance's diagonal is draws["static"]."""
    rng = np.random.default_rng(seed)
    q = d if kind == "sys" else p
    draws = {"beta": np.zeros((M, N, q, k)) if beta0 else 0.7 * rng.normal(size=(M, N, q, k)), "v": rng.uniform(0.5, 1.5, (M, N, q)),
             "sv": np.stack([rng.uniform(-0.9, 0.9, (M, N, k)), 0.5 * rng.normal(size=(M, N, k)), rng.uniform(0.1, 0.4, (M, N, k))], axis=3),
             "alpha": 0.5 * rng.normal(size=(M, N, k, T + 1))}
    if kind == "fsv":
        return None, None, draws, {}
    draws["static"] = rng.uniform(0.5, 1.5, (M, N, p if kind == "sys" else d))
    return toy_model(p, d), rng.normal(size=(N, T, p)), draws, {"m0": 0.1 * np.arange(d, dtype=np.float64), "C0": 2.0 * np.eye(d) + 0.3}
