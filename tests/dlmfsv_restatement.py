"""NumPy restatement of the three kernels of bayesian_dlms_amd/csrc/dlm_dlmfsv.hip, operation for operation and in the kernels' summation
order, vectorised over the panels -- `center` (k_dlmfsv_center), `impute` (k_dlmfsv_impute) and `variance` (k_dlmfsv_variance) -- and the exact-invariance setup of the
DLM with factor stochastic-volatility noise that tests/test_dlmfsv_host.py and tests/test_dlmfsv_gpu.py share.

`sweep_host` is one iteration of bayesian_dlms_amd/dlmfsv.py on the CPU, in the default order or in the reference's (literal_order):
  1 center, impute   2 fsv_restatement.factors   3 the mixture weights of tests/test_stochvol_gpu.py, the oracle's AR(1) filter and backward
  sampler, the conjugate draws of k_sv_params (sampler_restatement.params_step's sums, vectorised)   4 fsv_restatement.loadings
  5 variance   6 the oracle's filter and backward sampler with the V_t stream (as tests/gibbs_invariance.py uses them)   7 W | theta.
`exact_start` draws (W, beta, sigma^2, sv, alpha, theta, f, y) from the model's joint law; `figures` / `failed` hold the collapsed state
(theta, alpha, sv, beta, sigma^2, W) at a sweep boundary against closed-form laws (f is auxiliary there: the next sweep redraws it first).

`mutant` injects ONE mistake into center or variance:  "pair_theta_t" centre on theta_t, not theta_{t+1};  "alpha_t" V_t from alpha_t;
"no_diag_v" V_t without diag(v);  "half_exp" exp(alpha / 2) for exp(alpha);  "f_transposed" F read row-major (F_ji at j p + i).

The toy (`toy`): one time point, alpha ~ N(0, 1), f ~ N(0, e^alpha), theta ~ N(0, 1), y = theta + f + N(0, 1/4); alpha | f by inversion on
a grid.  The default order (f | theta, alpha, y; alpha | f; theta | y, alpha with f integrated out) leaves the joint law invariant, the
reference's (alpha | f; f | theta, alpha, y; theta | y, alpha) does not.

Run as a script the module prints the rehearsal table and the toy of profiles/r16_notes.md:  python tests/dlmfsv_restatement.py [N]."""
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fsv_restatement as fr  # noqa: E402
import oracle  # noqa: E402
from sampler_restatement import gibbs_rand  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, materialise  # noqa: E402

KEY_DLMFSV = 0x444C4653
TWO_PI = fr.TWO_PI
MUTANTS = ("pair_theta_t", "alpha_t", "no_diag_v", "half_exp", "f_transposed")


# ---- the two kernels ----------------------------------------------------------------------------------------------------------------
def f_tables(mat):
    """F [T][d][p] of a materialised model."""
    d, p, T = mat.d, mat.p, mat.T
    return np.stack([mat.F[t * mat.f_stride:t * mat.f_stride + d * p].reshape(p, d).T for t in range(T)])


def center(y, theta, F, *, mutant=None):
    """k_dlmfsv_center.  y [N][T][p], theta [N][T+1][d], F [T][d][p] (or [d][p]).  -> (r [N][T][p], status [N], the magnitude
    |y_ti| + sum_j |F_ji theta_j| of every element, for the error bound)."""
    N, T, p = y.shape
    d = theta.shape[2]
    F = np.broadcast_to(F, (T, d, p))
    if mutant == "f_transposed":
        F = np.stack([np.ascontiguousarray(Ft.T).reshape(d, p) for Ft in F])      # the column-major buffer read as row-major d x p
    th = theta[:, :-1] if mutant == "pair_theta_t" else theta[:, 1:]
    with np.errstate(all="ignore"):
        s = np.zeros((N, T, p))
        mag = np.zeros((N, T, p))
        for j in range(d):
            term = F[None, :, j, :] * th[:, :, j, None]
            s = s + term
            mag = mag + np.abs(term)
        r = y - s
    status = np.where(np.isfinite(theta[:, 1:]).all(axis=(1, 2)), 0, _lib.ST_NONFINITE).astype(np.int32)
    return r, status, mag + np.abs(np.nan_to_num(y))


def variance(beta, v, alpha, *, mutant=None):
    """k_dlmfsv_variance.  beta [N][p][k], v [N][p], alpha [N][k][T+1].  -> (V [N][T][p][p], status [N], the magnitude
    sum_l |beta_il beta_jl| e_l + v_i [i == j] of every entry)."""
    N, p, k = beta.shape
    T = alpha.shape[2] - 1
    with np.errstate(all="ignore"):
        x = alpha[:, :, :-1] if mutant == "alpha_t" else alpha[:, :, 1:]
        e = np.exp(0.5 * x) if mutant == "half_exp" else np.exp(x)                   # [N][k][T]
        V = np.zeros((N, T, p, p))
        mag = np.zeros((N, T, p, p))
        for l in range(k):
            b = beta[:, :, None, l] * beta[:, None, :, l]                            # [N][p][p]
            term = b[:, None] * e[:, l, :, None, None]
            V = V + term
            mag = mag + np.abs(term)
        if mutant != "no_diag_v":
            idx = np.arange(p)
            V[:, :, idx, idx] = V[:, :, idx, idx] + v[:, None, :]
            mag[:, :, idx, idx] = mag[:, :, idx, idx] + np.abs(v[:, None, :])
    xa = alpha[:, :, 1:]
    bad = ~np.isfinite(beta).all(axis=(1, 2)) | ~((v > 0.0) & (v < np.inf)).all(axis=1) | ~np.isfinite(xa).all(axis=(1, 2))
    with np.errstate(all="ignore"):
        bad |= ~(np.exp(xa) < np.inf).all(axis=(1, 2))
    return V, np.where(bad, _lib.ST_NONFINITE, 0).astype(np.int32), mag


def normals(seed, series, it, comp, attempt):
    """draw_normal on DLM_KEY_DLMFSV for arrays (series, comp, attempt) of one shape."""
    series, comp, attempt = np.broadcast_arrays(np.asarray(series, np.int64), np.asarray(comp, np.int64), np.asarray(attempt, np.int64))
    u1, u2 = gibbs_rand(seed, series, it, comp, attempt, 0, KEY_DLMFSV)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI * u2)


def impute(r, beta, v, alpha, *, seed, series_offset, it):
    """k_dlmfsv_impute.  r [N][T][p] (NaN = missing), beta [N][p][k], v [N][p], alpha [N][k][T+1].  A time with some but not all components
    missing gets them drawn: f_t | (the observed components, alpha_{t+1}, beta, v), then r_ti = beta_i f_t + sqrt(v_i) z for the missing i.
    Every other entry is r's.  -> (r_out, status [N], the largest condition number of a P_t)."""
    N, T, p = r.shape
    k = beta.shape[2]
    obs = np.isfinite(r)
    part = obs.any(axis=2) & ~obs.all(axis=2)
    with np.errstate(all="ignore"):
        iv = 1.0 / v
        A = np.zeros((N, T, k, k))
        rr = np.zeros((N, T, k))
        for i in range(p):
            o = obs[:, :, i]
            w = r[:, :, i] * iv[:, None, i]
            for a in range(k):
                rr[:, :, a] = np.where(o, rr[:, :, a] + beta[:, None, i, a] * w, rr[:, :, a])
                for c in range(a + 1):
                    A[:, :, a, c] = np.where(o, A[:, :, a, c] + (beta[:, None, i, a] * iv[:, None, i]) * beta[:, None, i, c], A[:, :, a, c])
        x = np.transpose(alpha[:, :, 1:], (0, 2, 1))
        dd = np.exp(-x)
        abad = (~np.isfinite(x) | ~(dd < np.inf)).any(axis=2) & part
        P = A.copy()
        for j in range(k):
            P[:, :, j, j] = A[:, :, j, j] + dd[:, :, j]
        series = (series_offset + np.arange(N))[:, None, None]
        z = normals(seed, series, it, np.arange(T)[None, :, None], np.arange(k)[None, None, :])
        f, ok = fr.solve_draw(P, rr, z, False)
        zi = normals(seed, series, it, np.arange(T)[None, :, None], 8 + np.arange(p)[None, None, :])          # attempt 8 + i: after the k <= 8 of f
        m = np.zeros((N, T, p))
        for j in range(k):
            m = m + beta[:, None, :, j] * f[:, :, None, j]
        drawn = m + np.sqrt(v)[:, None, :] * zi
    bad = ~np.isfinite(beta).all(axis=(1, 2)) | ~((v > 0.0) & (v < np.inf)).all(axis=1)
    fill = part & ~abad & ok & ~bad[:, None]
    out = np.where(fill[:, :, None] & ~obs, drawn, r)
    status = np.zeros(N, np.int32)
    status[abad.any(axis=1)] |= _lib.ST_NONFINITE
    status[(part & ~abad & ~ok).any(axis=1)] |= _lib.ST_NOT_PD
    status[bad] = _lib.ST_NONFINITE
    return out, status, fr._cond(P[fill])


# ---- the exact-invariance setup -----------------------------------------------------------------------------------------------------
SEED = 20261                 # fixed before any run
INV_N, INV_P, INV_K, INV_T = 16384, 3, 2, 6
INV_MISSING_TIME, INV_MISSING_COMPONENT = 0.1, 0.1
INV_FSV_PRIOR = fr.fsv_prior()                              # beta ~ N(0.3, 0.7^2), sigma^2 ~ InverseGamma(4, 1.5)
INV_PRIOR_W = (4.0, 1.5)                                    # W_ii ~ InverseGamma(4, 1.5)
# Gaussian(mean, sd) of phi (on (-1, 1)) and of mu, InverseGamma of sigma_eta^2.  phi stays five prior standard deviations below 1: a chain
# drawn at phi = 1 - 4e-6 has a stationary standard deviation of 150 and exp(alpha) of 1e57, which is the joint law's but no test of arithmetic
INV_SV_PRIOR = dict(phi=(0.5, 0.1), mu=(0.0, 0.5), sigma=(4.0, 0.5))
INV_M0, INV_C0 = np.array([0.5, -0.2, 0.3, 0.1]), np.diag([4.0, 1.0, 4.0, 4.0])
SE_BOUND, P_MARGINAL = fr.SE_BOUND, fr.P_MARGINAL           # tests/gibbs_invariance.py
CHECKS = ("W KS", "sigma KS", "beta mean", "beta variance", "transition mean", "transition variance", "residual mean", "residual variance",
          "innovation mean", "innovation variance")


def inv_model():
    """polynomial(2) |*| polynomial(1) |*| polynomial(1): d = 4, p = 3, so a transposed F is another matrix."""
    return Dlm.polynomial(2) * Dlm.polynomial(1) * Dlm.polynomial(1)


def inv_mat(T=INV_T):
    return materialise(inv_model(), np.arange(1, T + 1, dtype=np.float64))


def exact_start(N=INV_N, seed=SEED):
    """{"W" [N][d], "beta", "v", "sv" [N][k][3], "alpha", "theta" [N][T+1][d], "f" [N][k][T], "y" [N][T][p]} from the model's joint law;
    then whole times are masked with probability 0.1 and single components with probability 0.1 (the masks do not depend on the values)."""
    rng = np.random.default_rng([seed, 0x444C4D])
    p, k, T = INV_P, INV_K, INV_T
    mat = inv_mat()
    d = mat.d
    F = f_tables(mat)
    G = mat.G.reshape(d, d).T
    W = INV_PRIOR_W[1] / rng.gamma(INV_PRIOR_W[0], 1.0, (N, d))
    phi = INV_SV_PRIOR["phi"][0] + INV_SV_PRIOR["phi"][1] * rng.standard_normal((N, k))
    while (np.abs(phi) >= 1.0).any():
        again = np.abs(phi) >= 1.0
        phi[again] = INV_SV_PRIOR["phi"][0] + INV_SV_PRIOR["phi"][1] * rng.standard_normal(int(again.sum()))
    mu = INV_SV_PRIOR["mu"][0] + INV_SV_PRIOR["mu"][1] * rng.standard_normal((N, k))
    sig = np.sqrt(INV_SV_PRIOR["sigma"][1] / rng.gamma(INV_SV_PRIOR["sigma"][0], 1.0, (N, k)))
    alpha = np.empty((N, k, T + 1))
    alpha[:, :, 0] = mu + sig / np.sqrt(1.0 - phi * phi) * rng.standard_normal((N, k))
    for t in range(T):
        alpha[:, :, t + 1] = mu + phi * (alpha[:, :, t] - mu) + sig * rng.standard_normal((N, k))
    fm = fr.free_mask(p, k)
    beta = np.zeros((N, p, k))
    beta[:, fm] = INV_FSV_PRIOR["beta_mean"] + INV_FSV_PRIOR["beta_sd"] * rng.standard_normal((N, int(fm.sum())))
    beta[:, np.arange(k), np.arange(k)] = 1.0
    s2 = INV_FSV_PRIOR["sigma_scale"] / rng.gamma(INV_FSV_PRIOR["sigma_shape"], 1.0, N)
    f = rng.standard_normal((N, k, T)) * np.exp(0.5 * alpha[:, :, 1:])
    theta = np.empty((N, T + 1, d))
    theta[:, 0] = INV_M0 + rng.standard_normal((N, d)) @ np.linalg.cholesky(INV_C0).T
    y = np.empty((N, T, p))
    for t in range(T):
        theta[:, t + 1] = theta[:, t] @ G.T + np.sqrt(W) * rng.standard_normal((N, d))
        y[:, t] = theta[:, t + 1] @ F[t] + np.einsum("nij,nj->ni", beta, f[:, :, t]) + np.sqrt(s2)[:, None] * rng.standard_normal((N, p))
    y[rng.random((N, T)) < INV_MISSING_TIME] = np.nan
    y[rng.random((N, T, p)) < INV_MISSING_COMPONENT] = np.nan
    return {"W": W, "beta": beta, "v": np.broadcast_to(s2[:, None], (N, p)).copy(), "sv": np.stack([phi, mu, sig], axis=2), "alpha": alpha,
            "theta": theta, "f": f, "y": y}


def _volatility_host(f, alpha, sv, rng):
    """Step 3 on the CPU for the chains f [M][T], alpha [M][T+1], sv [M][3]: the mixture indicators given alpha (the weights of
    tests/test_stochvol_gpu.py), the oracle's AR(1) FFBS, then phi, mu, sigma_eta by k_sv_params' default conjugate draws."""
    from test_stochvol_gpu import MEANS, VARS, mixture_weights
    M, T = f.shape
    ly, obs, degenerate, pc = mixture_weights(f, alpha)
    assert not degenerate.any()
    us = rng.random((M, T)) * pc[..., 6]
    kt = (us[..., None] >= pc[..., :6]).sum(axis=-1)
    ystar, vm = np.where(obs, ly - MEANS[kt], np.nan), VARS[kt]
    z = rng.standard_normal((M, T + 1))
    new = np.empty_like(alpha)
    for m in range(M):
        flt = oracle.ar1_filter(ystar[m], vm[m], sv[m, 0], sv[m, 1], sv[m, 2])
        new[m] = oracle.ar1_backward_sample(flt, sv[m, 0], z[m])
    pr = INV_SV_PRIOR
    mu0, s2 = sv[:, 1], sv[:, 2] ** 2
    prev, cur = new[:, :-1] - mu0[:, None], new[:, 1:] - mu0[:, None]
    psi2 = pr["phi"][1] ** 2
    prec = 1.0 / psi2 + (prev * prev).sum(axis=1) / s2
    mean = (pr["phi"][0] / psi2 + (prev * cur).sum(axis=1) / s2) / prec
    phi = mean + rng.standard_normal(M) / np.sqrt(prec)
    while (np.abs(phi) >= 1.0).any():
        again = np.abs(phi) >= 1.0
        phi[again] = mean[again] + rng.standard_normal(int(again.sum())) / np.sqrt(prec[again])
    pm2, omp = pr["mu"][1] ** 2, 1.0 - phi
    mprec = 1.0 / pm2 + T * omp * omp / s2
    mmean = (pr["mu"][0] / pm2 + omp / s2 * (new[:, 1:] - phi[:, None] * new[:, :-1]).sum(axis=1)) / mprec
    mu = mmean + rng.standard_normal(M) / np.sqrt(mprec)
    res = (new[:, 1:] - mu[:, None]) - phi[:, None] * (new[:, :-1] - mu[:, None])
    sig = np.sqrt((pr["sigma"][1] + 0.5 * (res * res).sum(axis=1)) / rng.gamma(pr["sigma"][0] + 0.5 * T, 1.0, M))
    return new, np.stack([phi, mu, sig], axis=1)


def sweep_host(state, it, *, literal_order=False, mutant=None, seed=SEED, impute_partial=True):
    """One iteration on the CPU from `state` (not written to): the new state.  impute_partial=False: the reference's treatment of a
    partially missing time."""
    rng = np.random.default_rng([seed, 7, it])
    mat = inv_mat(state["y"].shape[1])
    d, p, T = mat.d, mat.p, mat.T
    F = f_tables(mat)
    G = mat.G.reshape(d, d).T
    y, N = state["y"], state["y"].shape[0]
    k = state["beta"].shape[2]
    r, st, _ = center(y, state["theta"], F, mutant=mutant)
    assert not st.any()
    if impute_partial:
        r, st, _ = impute(r, state["beta"], state["v"], state["alpha"], seed=seed, series_offset=0, it=it)
        assert not st.any()
    alpha, sv, f = state["alpha"], state["sv"], state["f"]
    draw_f = lambda al: fr.factors(r, state["beta"], state["v"], al, seed=seed, series_offset=0, it=it)
    if not literal_order:
        f, st, _ = draw_f(alpha)
    a2, s2 = _volatility_host(f.reshape(N * k, T), alpha.reshape(N * k, T + 1), sv.reshape(N * k, 3), rng)
    alpha, sv = a2.reshape(N, k, T + 1), s2.reshape(N, k, 3)
    if literal_order:
        f, st, _ = draw_f(alpha)
    beta, v, st2, _ = fr.loadings(r, f, state["beta"], state["v"], INV_FSV_PRIOR, seed=seed, series_offset=0, it=it)
    # a panel without a wholly observed time keeps its beta and sigma^2 (flagged by the loadings call): the identity leaves any law invariant
    empty = ~np.isfinite(y).all(axis=2).any(axis=1)
    assert not st.any() and not st2[~empty].any(), (st.max(), st2.max())
    V, st, _ = variance(beta, v, alpha, mutant=mutant)
    assert not st.any()
    om = oracle.Model(mat.d, mat.p, mat.T, mat.F, mat.G, mat.g_index, mat.dt, mat.f_stride)
    z = rng.standard_normal((N, T + 1, d))
    theta = np.empty((N, T + 1, d))
    for n in range(N):
        Wn = np.diag(state["W"][n])
        flt = oracle.kf_filter(om, V[n], Wn, INV_M0, INV_C0, y[n])
        b = oracle.backward_sample(om, Wn, flt, z[n], factor="chol")
        assert flt["rc"] == 0 and b["rc"] == 0, (n, flt["rc"], b["rc"])
        theta[n] = b["theta"]
    diff = theta[:, 1:] - theta[:, :-1] @ G.T
    W = (INV_PRIOR_W[1] + 0.5 * (diff * diff).sum(axis=1)) / rng.gamma(INV_PRIOR_W[0] + 0.5 * T, 1.0, (N, d))
    return {"W": W, "beta": beta, "v": v, "sv": sv, "alpha": alpha, "theta": theta, "f": f, "y": y}


def run_host(start, sweeps, **kw):
    state = start
    for it in range(sweeps):
        state = sweep_host(state, it, **kw)
    return state


def _se(x, obs=None):
    """Largest |mean| and |var - 1| over the columns of x [N][..] in standard errors, each column at its count (obs [N][..])."""
    obs = np.ones(x.shape, bool) if obs is None else obs
    return fr._se(np.where(obs, x, 0.0), obs)


def figures(state, start=None):
    """The figures of the checks on the collapsed state (theta, alpha, sv, beta, sigma^2, W) with its y."""
    from scipy import stats as ss
    y, theta, alpha, sv, beta, v, W = (state[q] for q in ("y", "theta", "alpha", "sv", "beta", "v", "W"))
    N, T, p = y.shape
    k, d = beta.shape[2], theta.shape[2]
    mat = inv_mat(T)
    F = f_tables(mat)
    G = mat.G.reshape(d, d).T
    out = {"N": N}
    out["W KS"] = min(float(ss.kstest(W[:, i], ss.invgamma(INV_PRIOR_W[0], scale=INV_PRIOR_W[1]).cdf).pvalue) for i in range(d))
    out["sigma KS"] = float(ss.kstest(1.0 / v[:, 0], ss.gamma(INV_FSV_PRIOR["sigma_shape"], scale=1.0 / INV_FSV_PRIOR["sigma_scale"]).cdf).pvalue)
    zb = (beta[:, fr.free_mask(p, k)] - INV_FSV_PRIOR["beta_mean"]) / INV_FSV_PRIOR["beta_sd"]
    out["beta mean"], out["beta variance"] = _se(zb)
    out["transition mean"], out["transition variance"] = _se((theta[:, 1:] - theta[:, :-1] @ G.T) / np.sqrt(W)[:, None, :])
    # L_t^-1 (y_t - F_t^T theta_{t+1}) over the observed components, L_t the Cholesky factor of that block of V_t: with f integrated out
    # the residual of an observed block is N(0, V_t[obs, obs]); component c of the whitened vector is kept in column (t, c-th observed)
    Vt = variance(beta, v, alpha)[0]
    res = y - np.einsum("tdj,ntd->ntj", F, theta[:, 1:])
    obs = np.isfinite(y)
    white, wobs = np.zeros((N, T, p)), np.zeros((N, T, p), bool)
    for pattern in range(1, 1 << p):
        sel = np.array([bool(pattern >> i & 1) for i in range(p)])
        rows = (obs == sel).all(axis=2)
        if not rows.any():
            continue
        L = np.linalg.cholesky(Vt[rows][:, sel][:, :, sel])
        w = np.linalg.solve(L, res[rows][:, sel][:, :, None])[:, :, 0]
        q = int(sel.sum())
        tmp = np.zeros((int(rows.sum()), p)); tmp[:, :q] = w
        white[rows] = tmp
        tm = np.zeros((int(rows.sum()), p), bool); tm[:, :q] = True
        wobs[rows] = tm
    out["residual mean"], out["residual variance"] = _se(white, wobs)
    phi, mu, sig = (sv[:, :, i, None] for i in range(3))
    inn = ((alpha[:, :, 1:] - mu) - phi * (alpha[:, :, :-1] - mu)) / sig
    out["innovation mean"], out["innovation variance"] = _se(inn)
    if start is not None:
        out["moved theta"] = float(np.abs(theta - start["theta"]).mean())
        out["moved W"] = float(np.mean(np.abs(W - start["W"]) / start["W"]))
    return out


def failed(fig):
    """The names of the checks `fig` fails, in the order of CHECKS."""
    level = {"W KS": P_MARGINAL / 4, "sigma KS": P_MARGINAL}
    return [c for c in CHECKS if (not fig[c] >= level[c] if c in level else not fig[c] <= SE_BOUND)]


def describe(fig):
    return (f"N {fig['N']}  KS p: W {fig['W KS']:.3g} sigma^2 {fig['sigma KS']:.3g}   (mean, var) in standard errors: beta {fig['beta mean']:.2f} "
            f"{fig['beta variance']:.2f}  transitions {fig['transition mean']:.2f} {fig['transition variance']:.2f}  residuals "
            f"{fig['residual mean']:.2f} {fig['residual variance']:.2f}  innovations {fig['innovation mean']:.2f} {fig['innovation variance']:.2f}")


# ---- the toy ------------------------------------------------------------------------------------------------------------------------------
TOY_N, TOY_SEED, TOY_V = 200000, 20262, 0.25
_GRID = np.linspace(-5.5, 5.5, 111)


def _toy_alpha_given_f(f, rng):
    """alpha | f by inversion of the piecewise-linear cdf on _GRID: log density -alpha^2 / 2 - alpha / 2 - f^2 e^-alpha / 2."""
    out = np.empty_like(f)
    for lo in range(0, f.size, 25000):
        ff = f[lo:lo + 25000, None]
        lp = -0.5 * _GRID * _GRID - 0.5 * _GRID - 0.5 * ff * ff * np.exp(-_GRID)
        dens = np.exp(lp - lp.max(axis=1, keepdims=True))
        cdf = np.concatenate([np.zeros((ff.shape[0], 1)), np.cumsum(0.5 * (dens[:, 1:] + dens[:, :-1]), axis=1)], axis=1)
        u = rng.random(ff.shape[0]) * cdf[:, -1]
        j = np.clip((cdf <= u[:, None]).sum(axis=1) - 1, 0, _GRID.size - 2)
        rows = np.arange(ff.shape[0])
        c0, c1 = cdf[rows, j], cdf[rows, j + 1]
        out[lo:lo + 25000] = _GRID[j] + (u - c0) / (c1 - c0) * (_GRID[1] - _GRID[0])
    return out


def toy(sweeps, literal_order, N=TOY_N, seed=TOY_SEED):
    """{"mean", "var"}: the mean and the variance of alpha after the sweeps, in standard errors from N(0, 1)'s."""
    rng = np.random.default_rng([seed, int(literal_order)])
    alpha = rng.standard_normal(N)
    f = np.exp(0.5 * alpha) * rng.standard_normal(N)
    theta = rng.standard_normal(N)
    y = theta + f + math.sqrt(TOY_V) * rng.standard_normal(N)

    def draw_f():
        prec = 1.0 / TOY_V + np.exp(-alpha)
        return (y - theta) / TOY_V / prec + rng.standard_normal(N) / np.sqrt(prec)
    for _ in range(sweeps):
        if literal_order:
            alpha = _toy_alpha_given_f(f, rng)
            f = draw_f()
        else:
            f = draw_f()
            alpha = _toy_alpha_given_f(f, rng)
        s2 = np.exp(alpha) + TOY_V
        prec = 1.0 + 1.0 / s2
        theta = y / s2 / prec + rng.standard_normal(N) / np.sqrt(prec)
    return {"mean": float(alpha.mean() * math.sqrt(N)), "var": float((alpha.var() - 1.0) / math.sqrt(2.0 / N))}


def rehearse(N=INV_N, out=sys.stdout):
    start = exact_start(N)
    for sweeps in (1, 3):
        t0 = time.time()
        fig = figures(run_host(start, sweeps), start)
        print(f"default order, {sweeps} sweep(s): {describe(fig)}   fails: {failed(fig)}   [{time.time() - t0:.0f} s]", file=out, flush=True)
    fig = figures(run_host(start, 3, impute_partial=False), start)
    print(f"partially missing times as the reference treats them (Q34), 3 sweeps: {describe(fig)}   fails: {failed(fig)}", file=out, flush=True)
    fig = figures(run_host(start, 3, literal_order=True), start)
    print(f"reference order, 3 sweeps: {describe(fig)}   fails: {failed(fig)}", file=out, flush=True)
    for m in MUTANTS:
        fig = figures(run_host(start, 1, mutant=m), start)
        print(f"{m:13s} 1 sweep: {describe(fig)}   fails: {failed(fig)}", file=out, flush=True)
    for lit in (False, True):
        for sweeps in (3, 10):
            print(f"toy, {'reference' if lit else 'default'} order, {sweeps} sweeps, {TOY_N} replicates: alpha (mean, var) {toy(sweeps, lit)} standard errors",
                  file=out, flush=True)


if __name__ == "__main__":
    rehearse(*[int(a) for a in sys.argv[1:]])
