"""NumPy restatement of k_dlmfsvsys_innovations (bayesian_dlms_amd/csrc/dlm_dlmfsv.hip), operation for operation and in the kernel's
summation order, vectorised over the panels -- `innovations` -- and the exact-invariance setup of the DLM with factor stochastic-volatility
SYSTEM noise that tests/test_dlmfsvsys_host.py and tests/test_dlmfsvsys_gpu.py share.

`sweep_host` is one iteration of bayesian_dlms_amd/dlmfsvsys.py on the CPU, in the default order or in the reference's (literal_order):
  1 innovations   2 fsv_restatement.factors on w   3 dlmfsv_restatement's volatility step (mixture weights, the oracle's AR(1) filter and
  backward sampler, k_sv_params' conjugate draws)   4 fsv_restatement.loadings on (w, f)   5 dlmfsv_restatement.variance with p := d
  6 the oracle's filter and backward sampler with the W_t stream (as tests/dlmfsv_restatement.py uses them with V_t)   7 V | theta, y.
`exact_start` draws (V, beta, sigma^2, sv, alpha, f, theta, y) from the model's joint law; `figures` / `failed` hold the collapsed state
(theta, alpha, sv, beta, sigma^2, V) at a sweep boundary against closed-form laws (f is auxiliary there: the next sweep redraws it first).

`mutant` injects ONE mistake:  "g_transposed" w_t = theta_{t+1} - G^T theta_t;  "pair_theta_t" the innovations shifted by one time
against alpha (w[t] := theta_t - G theta_{t-1} for t >= 1);  "alpha_t" W_t from alpha_t;  "no_diag_v" W_t without diag(v);  "w_as_v" the V
draw fed W_out (the transitions' sums of squares for the observations').

The toy (`toy`): one time point, alpha ~ N(0, 1), f ~ N(0, e^alpha), theta = f + N(0, 1/4), y = theta + N(0, 1); alpha | f by inversion on a
grid.  The default order (f | theta, alpha; alpha | f; theta | y, alpha with f integrated out) leaves the joint law invariant, the
reference's (alpha | f; f | theta, alpha; theta | y, alpha) does not.

Run as a script the module prints the rehearsal table and the toy of profiles/r17_notes.md:  python tests/dlmfsvsys_restatement.py [N]."""
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dlmfsv_restatement as dr  # noqa: E402
import fsv_restatement as fr  # noqa: E402
import oracle  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, materialise  # noqa: E402

MUTANTS = ("g_transposed", "pair_theta_t", "alpha_t", "no_diag_v", "w_as_v")


# ---- the kernel -------------------------------------------------------------------------------------------------------------------------
def innovations(theta, G, *, mutant=None):
    """k_dlmfsvsys_innovations.  theta [N][T+1][d], G [d][d].  -> (w [N][T][d], status [N], the magnitude |theta_{t+1,i}| +
    sum_j |G_ij theta_tj| of every element, for the error bound)."""
    N, T1, d = theta.shape
    G = np.asarray(G, dtype=np.float64)
    if mutant == "g_transposed":
        G = G.T
    with np.errstate(all="ignore"):
        s = np.zeros((N, T1 - 1, d))
        mag = np.zeros((N, T1 - 1, d))
        for j in range(d):
            term = G[None, None, :, j] * theta[:, :-1, j, None]
            s = s + term
            mag = mag + np.abs(term)
        w = theta[:, 1:] - s
        mag = mag + np.abs(theta[:, 1:])
    if mutant == "pair_theta_t":
        w = np.concatenate([w[:, :1], w[:, :-1]], axis=1)
    status = np.where(np.isfinite(theta).all(axis=(1, 2)), 0, _lib.ST_NONFINITE).astype(np.int32)
    return w, status, mag


# ---- the exact-invariance setup -----------------------------------------------------------------------------------------------------
SEED = 20263                 # fixed before any run
INV_N, INV_D, INV_K, INV_P, INV_T = 16384, 3, 2, 2, 6
INV_MISSING_TIME, INV_MISSING_COMPONENT = 0.1, 0.1
INV_FSV_PRIOR = fr.fsv_prior()                              # beta ~ N(0.3, 0.7^2), sigma^2 ~ InverseGamma(4, 1.5)
INV_PRIOR_V = (4.0, 1.5)                                    # V_ii ~ InverseGamma(4, 1.5)
INV_SV_PRIOR = dr.INV_SV_PRIOR                              # dlmfsv_restatement's, for its reason (phi five prior sds below 1)
INV_M0, INV_C0 = np.array([0.5, -0.2, 0.3]), np.diag([4.0, 1.0, 4.0])
SE_BOUND, P_MARGINAL = fr.SE_BOUND, fr.P_MARGINAL           # tests/gibbs_invariance.py
CHECKS = ("V KS", "sigma KS", "beta mean", "beta variance", "transition mean", "transition variance", "residual mean", "residual variance",
          "innovation mean", "innovation variance")


def inv_model():
    """polynomial(2) |*| polynomial(1): d = 3, p = 2, G = [[1, 1, 0], [0, 1, 0], [0, 0, 1]] -- not symmetric, so a transposed G is
    another matrix, and p != d, so a transposed F is too."""
    return Dlm.polynomial(2) * Dlm.polynomial(1)


def inv_mat(T=INV_T):
    return materialise(inv_model(), np.arange(1, T + 1, dtype=np.float64))


def exact_start(N=INV_N, seed=SEED):
    """{"V" [N][p], "beta" [N][d][k], "v" [N][d], "sv" [N][k][3], "alpha", "theta" [N][T+1][d], "f" [N][k][T], "y" [N][T][p]} from the
    model's joint law; then whole times are masked with probability 0.1 and single components with probability 0.1 (the masks do not
    depend on the values)."""
    rng = np.random.default_rng([seed, 0x444C53])
    d, k, p, T = INV_D, INV_K, INV_P, INV_T
    mat = inv_mat()
    assert (mat.d, mat.p) == (d, p)
    F = dr.f_tables(mat)
    G = mat.G.reshape(d, d).T
    V = INV_PRIOR_V[1] / rng.gamma(INV_PRIOR_V[0], 1.0, (N, p))
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
    fm = fr.free_mask(d, k)
    beta = np.zeros((N, d, k))
    beta[:, fm] = INV_FSV_PRIOR["beta_mean"] + INV_FSV_PRIOR["beta_sd"] * rng.standard_normal((N, int(fm.sum())))
    beta[:, np.arange(k), np.arange(k)] = 1.0
    s2 = INV_FSV_PRIOR["sigma_scale"] / rng.gamma(INV_FSV_PRIOR["sigma_shape"], 1.0, N)
    f = rng.standard_normal((N, k, T)) * np.exp(0.5 * alpha[:, :, 1:])
    theta = np.empty((N, T + 1, d))
    theta[:, 0] = INV_M0 + rng.standard_normal((N, d)) @ np.linalg.cholesky(INV_C0).T
    y = np.empty((N, T, p))
    for t in range(T):
        theta[:, t + 1] = theta[:, t] @ G.T + np.einsum("nij,nj->ni", beta, f[:, :, t]) + np.sqrt(s2)[:, None] * rng.standard_normal((N, d))
        y[:, t] = theta[:, t + 1] @ F[t] + np.sqrt(V) * rng.standard_normal((N, p))
    y[rng.random((N, T)) < INV_MISSING_TIME] = np.nan
    y[rng.random((N, T, p)) < INV_MISSING_COMPONENT] = np.nan
    return {"V": V, "beta": beta, "v": np.broadcast_to(s2[:, None], (N, d)).copy(), "sv": np.stack([phi, mu, sig], axis=2), "alpha": alpha,
            "theta": theta, "f": f, "y": y}


def sweep_host(state, it, *, literal_order=False, mutant=None, seed=SEED):
    """One iteration on the CPU from `state` (not written to): the new state."""
    rng = np.random.default_rng([seed, 7, it])
    mat = inv_mat(state["y"].shape[1])
    d, p, T = mat.d, mat.p, mat.T
    F = dr.f_tables(mat)
    G = mat.G.reshape(d, d).T
    y, N = state["y"], state["y"].shape[0]
    k = state["beta"].shape[2]
    w, st, _ = innovations(state["theta"], G, mutant=mutant)
    assert not st.any()
    alpha, sv, f = state["alpha"], state["sv"], state["f"]
    draw_f = lambda al: fr.factors(w, state["beta"], state["v"], al, seed=seed, series_offset=0, it=it)
    if not literal_order:
        f, st, _ = draw_f(alpha)
    a2, s2 = dr._volatility_host(f.reshape(N * k, T), alpha.reshape(N * k, T + 1), sv.reshape(N * k, 3), rng)
    alpha, sv = a2.reshape(N, k, T + 1), s2.reshape(N, k, 3)
    if literal_order:
        f, st, _ = draw_f(alpha)
    beta, v, st2, _ = fr.loadings(w, f, state["beta"], state["v"], INV_FSV_PRIOR, seed=seed, series_offset=0, it=it)
    assert not st.any() and not st2.any(), (st.max(), st2.max())
    vm = mutant if mutant in ("alpha_t", "no_diag_v") else None
    W, st, _ = dr.variance(beta, v, alpha, mutant=vm)                            # [N][T][d][d]
    assert not st.any()
    om = oracle.Model(mat.d, mat.p, mat.T, mat.F, mat.G, mat.g_index, mat.dt, mat.f_stride)
    z = rng.standard_normal((N, T + 1, d))
    theta = np.empty((N, T + 1, d))
    for n in range(N):
        flt = oracle.kf_filter(om, np.diag(state["V"][n]), W[n], INV_M0, INV_C0, y[n])
        b = oracle.backward_sample(om, W[n], flt, z[n], factor="chol")
        assert flt["rc"] == 0 and b["rc"] == 0, (n, flt["rc"], b["rc"])
        theta[n] = b["theta"]
    if mutant == "w_as_v":
        diff = (theta[:, 1:] - theta[:, :-1] @ G.T)[:, :, :p]
        ss, cnt = (diff * diff).sum(axis=1), np.full((N, p), float(T))
    else:
        res = y - np.einsum("tdj,ntd->ntj", F, theta[:, 1:])
        obs = np.isfinite(y)
        ss, cnt = np.where(obs, res * res, 0.0).sum(axis=1), obs.sum(axis=1).astype(np.float64)
    V = (INV_PRIOR_V[1] + 0.5 * ss) / rng.gamma(INV_PRIOR_V[0] + 0.5 * cnt, 1.0)
    return {"V": V, "beta": beta, "v": v, "sv": sv, "alpha": alpha, "theta": theta, "f": f, "y": y}


def run_host(start, sweeps, **kw):
    state = start
    for it in range(sweeps):
        state = sweep_host(state, it, **kw)
    return state


def figures(state, start=None):
    """The figures of the checks on the collapsed state (theta, alpha, sv, beta, sigma^2, V) with its y."""
    from scipy import stats as ss
    y, theta, alpha, sv, beta, v, V = (state[q] for q in ("y", "theta", "alpha", "sv", "beta", "v", "V"))
    N, T, p = y.shape
    k, d = beta.shape[2], theta.shape[2]
    mat = inv_mat(T)
    F = dr.f_tables(mat)
    G = mat.G.reshape(d, d).T
    out = {"N": N}
    out["V KS"] = min(float(ss.kstest(V[:, i], ss.invgamma(INV_PRIOR_V[0], scale=INV_PRIOR_V[1]).cdf).pvalue) for i in range(p))
    out["sigma KS"] = float(ss.kstest(1.0 / v[:, 0], ss.gamma(INV_FSV_PRIOR["sigma_shape"], scale=1.0 / INV_FSV_PRIOR["sigma_scale"]).cdf).pvalue)
    zb = (beta[:, fr.free_mask(d, k)] - INV_FSV_PRIOR["beta_mean"]) / INV_FSV_PRIOR["beta_sd"]
    out["beta mean"], out["beta variance"] = dr._se(zb)
    # L_t^-1 (theta_{t+1} - G theta_t), L_t the Cholesky factor of W_t: with f integrated out the innovation is N(0, W_t)
    Wt = dr.variance(beta, v, alpha)[0]
    w = theta[:, 1:] - theta[:, :-1] @ G.T
    out["transition mean"], out["transition variance"] = dr._se(np.linalg.solve(np.linalg.cholesky(Wt), w[..., None])[..., 0])
    res = (y - np.einsum("tdj,ntd->ntj", F, theta[:, 1:])) / np.sqrt(V)[:, None, :]
    out["residual mean"], out["residual variance"] = dr._se(np.nan_to_num(res), np.isfinite(y))
    phi, mu, sig = (sv[:, :, i, None] for i in range(3))
    inn = ((alpha[:, :, 1:] - mu) - phi * (alpha[:, :, :-1] - mu)) / sig
    out["innovation mean"], out["innovation variance"] = dr._se(inn)
    if start is not None:
        out["moved theta"] = float(np.abs(theta - start["theta"]).mean())
        out["moved V"] = float(np.mean(np.abs(V - start["V"]) / start["V"]))
    return out


def failed(fig):
    """The names of the checks `fig` fails, in the order of CHECKS: a KS p-value not above 1e-3, any other figure beyond five standard errors."""
    return [c for c in CHECKS if (not fig[c] > P_MARGINAL if c.endswith("KS") else not fig[c] <= SE_BOUND)]


def describe(fig):
    return (f"N {fig['N']}  KS p: V {fig['V KS']:.3g} sigma^2 {fig['sigma KS']:.3g}   (mean, var) in standard errors: beta {fig['beta mean']:.2f} "
            f"{fig['beta variance']:.2f}  transitions {fig['transition mean']:.2f} {fig['transition variance']:.2f}  residuals "
            f"{fig['residual mean']:.2f} {fig['residual variance']:.2f}  innovations {fig['innovation mean']:.2f} {fig['innovation variance']:.2f}")


# ---- the toy ------------------------------------------------------------------------------------------------------------------------------
TOY_N, TOY_SEED, TOY_V = 200000, 20264, 0.25


def toy(sweeps, literal_order, N=TOY_N, seed=TOY_SEED):
    """{"mean", "var"}: the mean and the variance of alpha after the sweeps, in standard errors from N(0, 1)'s."""
    rng = np.random.default_rng([seed, int(literal_order)])
    alpha = rng.standard_normal(N)
    f = np.exp(0.5 * alpha) * rng.standard_normal(N)
    theta = f + math.sqrt(TOY_V) * rng.standard_normal(N)
    y = theta + rng.standard_normal(N)

    def draw_f():
        prec = 1.0 / TOY_V + np.exp(-alpha)
        return theta / TOY_V / prec + rng.standard_normal(N) / np.sqrt(prec)
    for _ in range(sweeps):
        if literal_order:
            alpha = dr._toy_alpha_given_f(f, rng)
            f = draw_f()
        else:
            f = draw_f()
            alpha = dr._toy_alpha_given_f(f, rng)
        prec = 1.0 + 1.0 / (np.exp(alpha) + TOY_V)
        theta = y / prec + rng.standard_normal(N) / np.sqrt(prec)
    return {"mean": float(alpha.mean() * math.sqrt(N)), "var": float((alpha.var() - 1.0) / math.sqrt(2.0 / N))}


def rehearse(N=INV_N, out=sys.stdout):
    start = exact_start(N)
    state = start
    for sweeps in (1, 2, 3):
        t0 = time.time()
        state = sweep_host(state, sweeps - 1)
        fig = figures(state, start)
        print(f"default order, {sweeps} sweep(s): {describe(fig)}   fails: {failed(fig)}   [{time.time() - t0:.0f} s]", file=out, flush=True)
    for sweeps in (1, 3):
        fig = figures(run_host(start, sweeps, literal_order=True), start)
        print(f"reference order, {sweeps} sweep(s): {describe(fig)}   fails: {failed(fig)}", file=out, flush=True)
    for m in MUTANTS:
        fig = figures(run_host(start, 1, mutant=m), start)
        print(f"{m:13s} 1 sweep: {describe(fig)}   fails: {failed(fig)}", file=out, flush=True)
    for lit in (False, True):
        for sweeps in (3, 10):
            print(f"toy, {'reference' if lit else 'default'} order, {sweeps} sweeps, {TOY_N} replicates: alpha (mean, var) {toy(sweeps, lit)} standard errors",
                  file=out, flush=True)


if __name__ == "__main__":
    rehearse(*[int(a) for a in sys.argv[1:]])
