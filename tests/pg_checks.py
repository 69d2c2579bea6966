"""What a particle-Gibbs run is held to, in one place: tests/test_pg_host.py applies it to the restatement (tests/pg_restatement.py),
tests/test_pg_gpu.py to the kernel, at the same N, K, P and seeds.  Every bound is stated here with where it comes from; none was taken
from what the code under test gives.

  invariance   reference paths drawn from the exact smoothing law (tests/pg_grid_reference.py), K sweeps: per record the sample mean within
               SIGMAS sqrt(var / n), the sample variance within SIGMAS sqrt((mu_4 - var^2) / n) (the EXACT fourth moment), per step the mean of
               x_t x_{t+1} within SIGMAS sqrt(Var(x_t x_{t+1}) / n); n the series of the quarter that shares a parameter set.
  ancestor law per step with dt_t != 0, from the trace: p_j ~ W_{t-1,j} N(ref_{t+1}; G_t x_t,j, W dt_t) by scipy.stats; the averages over the
               series of log p_a - sum p log p and of x_t,a - sum p_j x_t,j lie within SIGMAS standard errors of 0, the standard error from
               the EXACT conditional variances under p (the draw is independent of everything else given the cloud and the weights).
  renewal      the share of series whose path still starts in the reference particle (path_index[0] == P - 1).
  trace        exact equalities between path, path_index, clouds, ancestors and ref; stats against NumPy sums to 1e-12 relative.
  gaussian     d = 2 and d = 3 against the Kalman smoother (the oracle's): means, variances and every lag-one cross-covariance, the
               standard errors those of a Gaussian law (which it is): sqrt(S_ii / n), S_ii sqrt(2 / n), sqrt((S_ii S'_jj + C_ij^2) / n).
  joint        (W, x, y) -- and V, Gaussian family -- from the model's joint law, K iterations of ParticleGibbs.sample, then the checks of
               tests/gibbs_invariance.py."""
import functools
import math

import numpy as np
from scipy import stats

import pf_cases as pc
import pf_grid_reference as gr
import pf_restatement as pr
import pg_grid_reference as gs

N, K, P, SIGMAS, SEED = 4096, 3, 64, 5.0, 2028
INVARIANCE_NAMES = list(gr.NAMES)
ANCESTOR_NAMES = ["irregular-studentt", "irregular-gaussian"]
# The share of series with path_index[0] == P - 1 after ONE sweep from the exact start, measured on the RESTATEMENT by
# tests/test_pg_host.py (which asserts these very figures) at N, P and invariance_args' seeds: (ancestor sampling, plain conditional SMC).
RESTATEMENT_KEPT = {
    "irregular-gaussian": (0.0623, 0.3611), "irregular-poisson": (0.1968, 0.4136), "irregular-negbin": (0.1934, 0.4224),
    "irregular-zip": (0.4182, 0.5540), "irregular-studentt": (0.1741, 0.5654), "irregular-beta": (0.0510, 0.3306),
    "per-series-poisson": (0.2595, 0.4507), "per-series-studentt": (0.0923, 0.4902), "first-missing-poisson": (0.0857, 0.3037),
}


def invariance_args(name, **over):
    """pg_restatement.run's arguments (and through pg_cases.engine_run the engine's) for a case of the grid smoother: N series, series n
    under parameter set n mod SETS with an exact draw of ITS smoothing law as the reference path"""
    kw = dict(gr.inputs(name, N), family=gr.by_name(name)["family"], P=P, ancestor_sampling=True, seed=SEED, series_offset=0, iteration=0,
              ref=gs.reference_paths(name, N))
    kw.update(over)
    return kw


def moment_z(name, path):
    """the largest |sample - exact| / standard error over the records (means, variances) and the steps (cross-moments), over the quarters"""
    worst = {"mean": 0.0, "var": 0.0, "cross": 0.0}
    for q, sl in enumerate(gr.quarters(name, path.shape[0])):
        x = np.asarray(path)[sl, :, 0]
        n, ex = x.shape[0], gs.smoothing(name, q)
        z = {"mean": np.abs(x.mean(axis=0) - ex["mean"]) / np.sqrt(ex["var"] / n),
             "var": np.abs(x.var(axis=0, ddof=1) - ex["var"]) / np.sqrt((ex["mu4"] - ex["var"] ** 2) / n),
             "cross": np.abs((x[:, :-1] * x[:, 1:]).mean(axis=0) - ex["cross"]) / np.sqrt(ex["cross_var"] / n)}
        for k in worst:
            worst[k] = max(worst[k], float(z[k].max()))
    return worst


def hold_invariance(name, path, label=""):
    z = moment_z(name, path)
    print(f"{name} {label}: worst over t, in standard errors: means {z['mean']:.2f}, variances {z['var']:.2f}, lag-one cross-moments {z['cross']:.2f}")
    assert z["mean"] <= SIGMAS and z["var"] <= SIGMAS and z["cross"] <= SIGMAS, z
    return z


def ancestor_z(kw, out):
    """per statistic the largest |average over the series| / standard error over the steps with dt_t != 0: ("log p_a", "x_a")"""
    clouds, anc, sw, ref = out["clouds"][:, :, 0, :], out["ancestors"], out["step_weights"], np.asarray(kw["ref"])[:, :, 0]
    n, Pn = clouds.shape[0], clouds.shape[2]
    W = np.broadcast_to(np.asarray(kw["W"], dtype=np.float64).reshape(-1), (n,))
    worst = [0.0, 0.0]
    for t in range(gs.T):
        a = anc[:, t, Pn - 1]
        if gs.DT[t] == 0.0:
            assert np.all(a == Pn - 1), t
            continue
        wprev = np.full((n, Pn), 1.0 / Pn) if t == 0 else sw[:, t - 1]
        lp = np.log(wprev) + stats.norm.logpdf(ref[:, t + 1, None], gs.G_T[t] * clouds[:, t], np.sqrt(W * gs.DT[t])[:, None])
        lp = lp - lp.max(axis=1, keepdims=True)
        p = np.exp(lp); p = p / p.sum(axis=1, keepdims=True)
        lp = np.log(p)
        rows = np.arange(n)
        for k, f in enumerate((np.where(p > 0.0, lp, 0.0), clouds[:, t])):
            e1 = (p * f).sum(axis=1)
            var = (p * f * f).sum(axis=1) - e1 * e1
            z = abs(float((f[rows, a] - e1).mean())) / math.sqrt(float(var.mean()) / n)
            worst[k] = max(worst[k], z)
        assert np.all(p[rows, a] > 0.0), t
    return worst


def hold_ancestor_law(kw, out, label=""):
    assert np.all(out["status"] == 0)
    z = ancestor_z(kw, out)
    print(f"ancestor law {label}: worst over t, in standard errors: log p_a {z[0]:.2f}, x_a {z[1]:.2f}")
    assert z[0] <= SIGMAS and z[1] <= SIGMAS, z
    return z


def kept_share(path_index, Pn):
    return float((np.asarray(path_index)[:, 0] == Pn - 1).mean())


def hold_renewal(name, on, off, measured=None):
    """on / off: the kept share with and without ancestor sampling; measured: RESTATEMENT_KEPT's entry (the host test passes none: it is
    what measures it, and holds its figure to the table)"""
    want = RESTATEMENT_KEPT[name][0] if measured is None else measured
    se = math.sqrt(max(want * (1.0 - want), 1.0 / N) / N)
    print(f"{name}: share of paths that still start in the reference particle: {on:.4f} with ancestor sampling (the restatement: {want:.4f}, "
          f"{abs(on - want) / se:.2f} binomial se), {off:.4f} without")
    assert on < 0.5, on
    assert abs(on - want) <= SIGMAS * se, (on, want, se)
    assert off > on, (on, off)


def hold_trace(kw, out):
    """checks 4: exact equalities of the trace-back and the conditioning, the statistics to 1e-12 relative"""
    import pg_cases as gc
    assert np.all(out["status"] == 0)
    path, k, clouds, anc, ref = out["path"], out["path_index"], out["clouds"], out["ancestors"], np.asarray(kw["ref"])
    n, T1, d = path.shape
    Pn = clouds.shape[3]
    rows = np.arange(n)
    dt = np.ones(T1 - 1) if kw["dt"] is None else np.asarray(kw["dt"])
    assert np.all((k >= 0) & (k < Pn)) and np.all((anc >= 0) & (anc < Pn))
    for t in range(T1):
        np.testing.assert_array_equal(path[:, t], clouds[rows, t, :, k[:, t]], err_msg=f"path[{t}]")
        if t == 0 or dt[t - 1] != 0.0:
            np.testing.assert_array_equal(clouds[:, t, :, Pn - 1], ref[:, t], err_msg=f"the reference particle at {t}")
        else:          # no advance: ref_t is not read, the reference particle stays where it was
            np.testing.assert_array_equal(clouds[:, t, :, Pn - 1], clouds[:, t - 1, :, Pn - 1], err_msg=f"the reference particle at {t}")
        if t:
            np.testing.assert_array_equal(k[:, t - 1], anc[rows, t - 1, k[:, t]], err_msg=f"path_index[{t - 1}]")
            if dt[t - 1] == 0.0:
                np.testing.assert_array_equal(path[:, t], path[:, t - 1], err_msg=f"dt = 0 at step {t - 1}")
                assert np.all(anc[:, t - 1, Pn - 1] == Pn - 1)
            if not kw["ancestor_sampling"]:
                assert np.all(anc[:, t - 1, Pn - 1] == Pn - 1)
    want = gc.path_stats(kw, path)
    np.testing.assert_allclose(out["stats"], want, rtol=1e-12, atol=0.0)
    w = out["step_weights"]
    assert np.all(w >= 0.0) and np.allclose(w.sum(axis=2), 1.0, rtol=0.0, atol=1e-12)
    missing = np.isnan(np.asarray(kw["y"]))
    assert np.all(w[missing] == 1.0 / Pn)


# ---- 5: Gaussian, d = 2 and d = 3 ------------------------------------------------------------------------------------------------------------
GAUSSIAN_NAMES = ["trend", "level-seasonal"]
GAUSSIAN_T = 10


@functools.lru_cache(maxsize=None)
def gaussian_case(which):
    """One series of a Gaussian DLM on an irregular grid with one missing y, replicated N times: the model's tables, the arrays the engine
    and the restatement take, and the Kalman smoother's moments (the oracle's filter and smoother; the lag-one cross-covariance
    Cov(x_t, x_{t+1} | y) = C_t G_t^T R_{t+1}^-1 S_{t+1})."""
    import oracle
    from bayesian_dlms_amd.dlm import Dlm, DlmParameters, materialise
    rng = np.random.default_rng([SEED, 5, len(which)])
    mod = Dlm.polynomial(2) if which == "trend" else Dlm.polynomial(1) + Dlm.seasonal(12, 1)
    times = np.cumsum(np.tile([1.0, 0.5, 2.0, 1.0, 1.5], GAUSSIAN_T // 5))
    mat = materialise(mod, times)
    d, T = mat.d, mat.T
    W = np.diag([0.3, 0.05] if d == 2 else [0.3, 0.1, 0.1])
    V, m0, C0 = 0.5, np.zeros(d), np.eye(d)
    om = oracle.Model(mat.d, mat.p, mat.T, mat.F, mat.G, mat.g_index, mat.dt, mat.f_stride)
    dt = np.ones(T) if mat.dt is None else np.asarray(mat.dt)
    gi = np.zeros(T, dtype=int) if mat.g_index is None else np.asarray(mat.g_index)
    G = np.stack([oracle.from_cm(mat.G[g * d * d:(g + 1) * d * d], d, d) for g in range(mat.n_g)])
    F = np.stack([oracle.from_cm(mat.F[t * mat.f_stride:t * mat.f_stride + d], d, 1)[:, 0] for t in range(T)])
    x = m0 + np.linalg.cholesky(C0) @ rng.standard_normal(d)
    y = np.empty(T)
    for t in range(T):
        x = G[gi[t]] @ x + np.sqrt(dt[t]) * (np.sqrt(np.diag(W)) * rng.standard_normal(d))
        y[t] = F[t] @ x + math.sqrt(V) * rng.standard_normal()
    y[4] = np.nan
    f = oracle.kf_filter(om, np.array([[V]]), W, m0, C0, y)
    s = oracle.smoother(om, f)
    assert f["rc"] == 0 and s["rc"] == 0
    sm = s["s"]
    S = np.stack([oracle.from_cm(s["S"][t], d, d) for t in range(T + 1)])
    C = np.stack([oracle.from_cm(f["C"][t], d, d) for t in range(T + 1)])
    R = np.stack([oracle.from_cm(f["R"][t], d, d) for t in range(T + 1)])
    cross = np.stack([C[t] @ G[gi[t]].T @ np.linalg.solve(R[t + 1], S[t + 1]) for t in range(T)])          # [T][i of x_t][j of x_{t+1}]
    kw = dict(F=F, G=G, g_index=None if mat.g_index is None else gi.astype(np.int32), dt=dt, V=V, W=W, m0=m0, C0=C0, y=np.tile(y, (N, 1)), nu=None,
              family=pr.GAUSSIAN, P=P, ancestor_sampling=True, seed=SEED + 5, series_offset=0, iteration=0)
    return dict(mat=mat, params=DlmParameters(np.array([[V]]), W, m0, C0), y3=np.tile(y, (N, 1))[:, :, None], kw=kw, mean=sm, cov=S, cross=cross)


def gaussian_z(which, path):
    c = gaussian_case(which)
    x = np.asarray(path)
    n = x.shape[0]
    var = np.diagonal(c["cov"], axis1=1, axis2=2)
    xc = x - x.mean(axis=0)
    z_mean = np.abs(x.mean(axis=0) - c["mean"]) / np.sqrt(var / n)
    z_var = np.abs(x.var(axis=0, ddof=1) - var) / (var * math.sqrt(2.0 / n))
    sc = np.einsum("nti,ntj->tij", xc[:, :-1], xc[:, 1:]) / (n - 1)
    se = np.sqrt((var[:-1, :, None] * var[1:, None, :] + c["cross"] ** 2) / n)
    return float(z_mean.max()), float(z_var.max()), float((np.abs(sc - c["cross"]) / se).max())


def hold_gaussian(which, path, label=""):
    z = gaussian_z(which, path)
    print(f"gaussian {which} {label}: worst over t and the components, in standard errors: means {z[0]:.2f}, variances {z[1]:.2f}, "
          f"lag-one cross-covariances {z[2]:.2f}")
    assert max(z) <= SIGMAS, z
    return z


# ---- 7: the sampler's joint law --------------------------------------------------------------------------------------------------------------
JOINT_NAMES = ["poisson-level", "gaussian-trend"]


@functools.lru_cache(maxsize=None)
def joint_case(which):
    """A tests/gibbs_invariance.py Case (its priors, its irregular grid): Poisson d = 1 with no missing value, Gaussian d = 2 with two"""
    import gibbs_invariance as gi
    from bayesian_dlms_amd.dlm import Dlm
    from bayesian_dlms_amd.gibbs import InverseGamma
    pv, pw = InverseGamma(4.0, 6.0), InverseGamma(4.0, 1.5)
    times = np.cumsum([1.0, 2.0, 0.5, 1.0, 3.0, 1.0, 0.25, 2.0])
    if which == "poisson-level":
        return gi.Case("pg-poisson-level", Dlm.polynomial(1), times, [], pv, InverseGamma(6.0, 0.5), [0.5], [[0.25]], {}, N=N, K=K)
    return gi.Case("pg-gaussian-trend", Dlm.polynomial(2), times, [(2, 0), (5, 0)], pv, pw, [0.5, -0.2], np.diag([4.0, 1.0]), {}, N=N, K=K)


def joint_start(which):
    """the exact start of gibbs_invariance (V, W, theta, y from the joint law); the Poisson case keeps theta and W and draws y afresh as
    Poisson(exp(F_t^T theta_{t+1})) (V is not a parameter of that family)"""
    import gibbs_invariance as gi
    case = joint_case(which)
    start = gi.exact_start(case, N, SEED)
    if which == "poisson-level":
        rng = np.random.default_rng([SEED, 7])
        eta = np.einsum("tdj,ntd->ntj", case.F, start["theta"][:, 1:])
        start = dict(start, y=rng.poisson(np.exp(eta)).astype(np.float64), V=np.ones_like(start["V"]))
    return case, start


def run_joint_engine(which, eng):
    """K iterations of ParticleGibbs.sample from the exact start -> (case, start, V [N][1], W [N][d], theta [N][T+1][d])"""
    from bayesian_dlms_amd.dglm import BatchedParameters, Dglm, ParticleGibbs
    case, start = joint_start(which)
    d = case.mat.d
    mod = Dglm.poisson(case.mod) if which == "poisson-level" else Dglm.gaussian(case.mod)
    Wm = np.zeros((N, d, d)); Wm[:, np.arange(d), np.arange(d)] = start["W"]
    init = BatchedParameters(start["V"].reshape(N, 1, 1), Wm, np.tile(case.m0, (N, 1)), np.tile(case.c0, (N, 1, 1)))
    pgs = ParticleGibbs(P, ancestor_sampling=True)
    for st in pgs.sample(mod, (case.times, start["y"][:, :, 0]), case.prior_w, init, eng, K, prior_v=None if which == "poisson-level" else case.prior_v,
                         seed=SEED, init_path=start["theta"]):
        assert st.status == 0
    return case, start, st.v.cpu().numpy().reshape(N, 1), st.w.cpu().numpy(), st.path.cpu().numpy()


def hold_joint(which, result):
    import gibbs_invariance as gi
    case, start, V, W, theta = result
    if which != "poisson-level":
        return gi.checks(case, V, W, theta, start["y"], start)
    # the Poisson family: W against its prior, the whitened transitions, the new-draw floor on W (V is no parameter here)
    assert np.isfinite(W).all() and np.isfinite(theta).all() and np.array_equal(V, start["V"])
    pvals = [float(stats.kstest(W[:, i], stats.invgamma(case.prior_w.shape, scale=case.prior_w.scale).cdf).pvalue) for i in range(case.mat.d)]
    diff = theta[:, 1:] - np.einsum("tde,nte->ntd", case.G, theta[:, :-1])
    trans = gi._deviation(diff / np.sqrt(W[:, None, :] * case.dt[None, :, None]), N)
    moved = float(np.mean(np.abs(W - start["W"]) / start["W"]))
    print(f"{case.name}: N {N}  min p W {min(pvals):.3g}   whitened transitions (mean, var) in standard errors: {trans[0]:.2f} {trans[1]:.2f}   "
          f"mean |W_new - W_start| / W_start {moved:.3f}")
    assert min(pvals) >= gi.P_MARGINAL / case.mat.d, pvals
    assert max(trans) <= gi.SE_BOUND, trans
    assert moved > gi.NEW_DRAW_FLOOR, moved
