"""Exact-invariance tests of the Gibbs samplers' parameter half (tests/test_gibbs_invariance_host.py, _gpu.py).

Draw (parameters, states, y) from the model's own joint law and run K sweeps of a sampler.  Every sweep is a composition of draws from
full conditionals of that joint law, so if each conditional is right the triple still has exactly the joint law afterwards: the
parameters follow their priors, the whitened transitions and observation residuals are independent N(0, 1).  A batch of N series is N
independent replicates, so the laws can be tested in one call.  Nothing here is shared with the kernels or with the oracle's
restatement of their statistics: the start is host NumPy, the checks are closed-form laws.

The model, stated once.  V_jj ~ InverseGamma(prior_v), W_ii ~ InverseGamma(prior_w) or W ~ InverseWishart(prior_w);
x_0 ~ N(m0, C0), x_t = G_t x_{t-1} + w_t, w_t ~ N(0, W dt_t), y_t = F_t^T x_t + v_t, v_t ~ N(0, V); theta[t] = x_t (T + 1 records), so
y[t] (0-based) belongs to theta[t + 1].  The conjugate draws, from include/dlm_engine.h (dlm_ffbs_batch, dlm_dinvgamma_step_batch):
  ssy_j = sum over the observed y_tj of (y_t - F_t^T theta_{t+1})_j^2,   n_j = the number of observed y_tj,
  ss_i  = sum_t (theta_{t+1} - G_t theta_t)_i^2 / dt_t   over all T transitions,   outer = sum_t diff_t diff_t^T / dt_t,
  V_jj ~ InverseGamma(a_v + n_j / 2, b_v + ssy_j / 2),  W_ii ~ InverseGamma(a_w + T / 2, b_w + ss_i / 2),  W ~ InverseWishart(nu + T, Psi + outer).

`sweep_host` is one sweep on the CPU: the oracle's filter and backward sampler per series, the statistics and draws above in NumPy.
Its `mutant` argument injects one mistake into those statistics or draws (never into the engine): the rehearsal that shows each of
them fail is what gives the passing tests their meaning.  Run as a script the module prints the rehearsal table of
profiles/r13_notes.md:  python tests/gibbs_invariance.py [N] [K].

The Student-t sampler (section `Student-t` below) has a flat prior on its scale s, so s is held fixed: with the same scale_in in
every call the steps form a partially collapsed Gibbs sampler of p(theta, W, nu, v | y, s)."""
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _dir in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _dir not in sys.path:
        sys.path.insert(0, _dir)

import oracle  # noqa: E402
from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters, materialise  # noqa: E402
from bayesian_dlms_amd.gibbs import InverseGamma, InverseWishart  # noqa: E402

SEED = 20261                                   # fixed before any run; every start and every sweep derives from it
MUTANTS = ("pair_theta_t", "missing_counted", "ss_without_dt", "shape_T_minus_1", "first_transition_dropped")
MUTANT_CHECK = {"pair_theta_t": "marginal V", "missing_counted": "marginal V", "ss_without_dt": "marginal W",
                "shape_T_minus_1": "marginal W", "first_transition_dropped": "marginal W"}
P_MARGINAL = 1e-3          # family-wise: each of the m marginals of a case at p >= P_MARGINAL / m
SE_BOUND = 5.0             # whitened means within 5 / sqrt(N), variances within 5 sqrt(2 / N) (tests/test_stochvol_gpu.py)
# Mean |V_new - V_start| / V_start after the sweeps.  Two independent draws of InverseGamma(4, .) differ by ~0.6 in this measure; the
# oracle sampler gave 0.46 .. 0.55 over the cases after one sweep and 0.54 .. 0.68 after three (profiles/r13_notes.md); a sampler
# that returns its input gives 0.
NEW_DRAW_FLOOR = 0.15
# Student-t: the same floor for mean |W_new - W_start| / W_start (the NumPy step gave 0.42 .. 0.43 after one sweep, 0.65 .. 0.69 after
# three) and for the median of |v_new - v_start| / v_start (0.63 .. 0.73 after one sweep and after three: v_t is redrawn whole in every
# sweep; the median, since the ratio of two heavy-tailed draws has no useful mean); nu must have changed in at least 0.15 of the chains
# (0.38 .. 0.39 after one sweep, 0.64 .. 0.67 after three; a Metropolis move that never accepts gives 0).
ST_NU_MOVED_FLOOR = 0.15
IW_REFERENCE_DRAWS = 1 << 16


class CheckFailed(AssertionError):
    """An invariance check that failed; `check` names it ("marginal V", "marginal W", "whitened transition", "whitened residual",
    "pairing control", "new draw")."""

    def __init__(self, check, detail):
        super().__init__(f"{check}: {detail}")
        self.check = check


def model_tables(mat):
    """(dt [T], G [T][d][d], F [T][d][p]) of a materialised model, one entry per step."""
    d, p, T = mat.d, mat.p, mat.T
    dt = np.ones(T) if mat.dt is None else np.asarray(mat.dt, dtype=np.float64)
    gi = np.zeros(T, dtype=int) if mat.g_index is None else np.asarray(mat.g_index)
    G = np.stack([oracle.from_cm(mat.G[g * d * d:(g + 1) * d * d], d, d) for g in gi])
    F = np.stack([oracle.from_cm(mat.F[t * mat.f_stride:t * mat.f_stride + d * p], d, p) for t in range(T)])
    return dt, G, F


class Case:
    """One model with its priors, its fixed NaN mask (`missing`: (t, j) pairs) and the routes it must reach: a dict label -> (flags,
    the Engine.last_variant of dlm_ffbs_batch for per-series parameters, read off sampler_common in dlm_engine.hip).  N, K: the batch
    and the sweeps of the GPU tests, chosen by the rehearsal."""

    def __init__(self, name, mod, times, missing, prior_v, prior_w, m0, c0, routes, N=8192, K=3, host_N=1024):
        self.name, self.mod, self.times, self.missing = name, mod, np.asarray(times, dtype=np.float64), tuple(missing)
        self.prior_v, self.prior_w, self.routes, self.N, self.K, self.host_N = prior_v, prior_w, routes, N, K, host_N
        self.mat = materialise(mod, self.times)
        d, p, T = self.mat.d, self.mat.p, self.mat.T
        self.m0 = np.asarray(m0, dtype=np.float64).reshape(d)
        self.c0 = np.asarray(c0, dtype=np.float64).reshape(d, d)
        self.wishart = isinstance(prior_w, InverseWishart)
        self.dt, self.G, self.F = model_tables(self.mat)
        self.obs = np.ones((T, p), dtype=bool)
        for t, j in self.missing:
            self.obs[t, j] = False
        self._iw_ref = None

    @property
    def n_marginals(self):
        return self.mat.p + self.mat.d + (2 if self.wishart else 0)

    def params_list(self, V, W):
        """N per-series DlmParameters from V [N][p] (diagonals) and W [N][d] (diagonals) or [N][d][d]."""
        return [DlmParameters(np.diag(v), w if self.wishart else np.diag(w), self.m0, self.c0) for v, w in zip(V, W)]

    def iw_reference(self):
        """2^16 host draws of the Inverse-Wishart prior: (diag [M][d], trace [M], log det [M]); made once, never written to."""
        if self._iw_ref is None:
            rng = np.random.default_rng([SEED, 0x4957])
            draws = np.stack([self.prior_w.draw(rng) for _ in range(IW_REFERENCE_DRAWS)])
            ref = wishart_summaries(draws)
            for a in ref:
                a.setflags(write=False)
            self._iw_ref = ref
        return self._iw_ref


def wishart_summaries(W):
    return np.diagonal(W, axis1=1, axis2=2).copy(), np.trace(W, axis1=1, axis2=2), np.linalg.slogdet(W)[1]


def _c2_model():
    return Dlm.polynomial(1) + Dlm.seasonal(24, 6)


def _blocks(n):
    mod = Dlm.polynomial(2)
    for _ in range(n - 1):
        mod = mod * Dlm.polynomial(2)
    return mod


def _build_cases():
    S, FW, NW, O = _lib.OPT_FFBS_SIMSMOOTH, _lib.OPT_FORCE_WAVE, _lib.OPT_NO_WAVE, _lib.OPT_STATS_OUTER
    pv, pw = InverseGamma(4.0, 6.0), InverseGamma(4.0, 1.5)
    rng = np.random.default_rng(1301)
    m13 = rng.standard_normal(13)
    cases = [
        # the grid of the NumPy rehearsal that motivated these tests
        Case("level", Dlm.polynomial(1), np.cumsum([1.0, 2.0, 0.5, 1.0, 3.0, 1.0, 0.25, 2.0]), [(2, 0), (5, 0)], pv, pw, [0.5], [[4.0]],
             {"sampler": (0, "lane-sampler"), "simsmooth": (S, "lane-simsmooth")}),
        # d <= 15 with p = 2: the per-wave kernels' small shapes (no lanes: those are p = 1); n_j differs between the components
        Case("trend2x2", Dlm.polynomial(2) * Dlm.polynomial(2), np.cumsum([1.0, 2.0, 0.5, 1.0, 1.5, 1.0]), [(2, 1), (4, 0), (4, 1)], pv, pw,
             [0.5, -0.2, 0.3, 0.1], np.diag([4.0, 1.0, 4.0, 1.0]), {"sampler": (0, "sparse16-sampler"), "simsmooth": (S, "wave-simsmooth")}),
        Case("c2", _c2_model(), np.cumsum([1.0, 2.0, 0.5, 1.0, 3.0, 1.0]), [(3, 0)], pv, pw, m13, 4.0 * np.eye(13),
             {"sampler": (0, "sparse16-sampler"), "simsmooth": (S, "sparse16-simsmooth")}),
        Case("blocks20", _blocks(10), np.arange(1.0, 5.0), [(1, 4)], pv, pw, 0.1 * rng.standard_normal(20), np.diag(np.linspace(0.5, 2.0, 20)),
             {"wave": (FW, "wave-sampler"), "wave-simsmooth": (FW | S, "wave-simsmooth"), "generic": (NW, "generic")}, N=2048, host_N=512),
        Case("wishart2", Dlm.polynomial(1) * Dlm.polynomial(1), np.cumsum([1.0, 2.0, 0.5, 1.0, 3.0, 1.0]), [], pv, InverseWishart(6.0, np.eye(2)),
             [0.5, -0.5], 4.0 * np.eye(2), {"sampler": (O, "sparse16-sampler")}, host_N=512),
        Case("wishart13", _c2_model(), np.arange(1.0, 5.0), [], pv, InverseWishart(17.0, 0.3 * np.eye(13)), m13, 4.0 * np.eye(13),
             {"sampler": (O, "sparse16-sampler")}, host_N=256),
    ]
    return {c.name: c for c in cases}


CASES = _build_cases()
DIAGONAL_CASES = [n for n, c in CASES.items() if not c.wishart]


def _simulate(case, rng, N, W_chol, v_sd):
    """theta [N][T+1][d], y [N][T][p] (no mask yet) with state noise W_chol [N][d][d] (lower factors) and observation standard
    deviations v_sd [N][T][p]."""
    d, p, T = case.mat.d, case.mat.p, case.mat.T
    theta = np.empty((N, T + 1, d))
    theta[:, 0] = case.m0 + rng.standard_normal((N, d)) @ np.linalg.cholesky(case.c0).T
    y = np.empty((N, T, p))
    for t in range(T):
        w = np.einsum("nij,nj->ni", W_chol, rng.standard_normal((N, d))) * math.sqrt(case.dt[t])
        theta[:, t + 1] = theta[:, t] @ case.G[t].T + w
        y[:, t] = theta[:, t + 1] @ case.F[t] + v_sd[:, t] * rng.standard_normal((N, p))
    return theta, y


def exact_start(case, N, seed=SEED):
    """{"V" [N][p], "W" [N][d] or [N][d][d], "theta" [N][T+1][d], "y" [N][T][p]} drawn from the joint law of the case; the case's mask
    is set afterwards (it does not depend on the values, so the law of the observed part is untouched)."""
    rng = np.random.default_rng([seed, sum(case.name.encode())])
    d, p, T = case.mat.d, case.mat.p, case.mat.T
    V = case.prior_v.draw(rng, size=(N, p))
    if case.wishart:
        W = np.stack([case.prior_w.draw(rng) for _ in range(N)])
        Lw = np.linalg.cholesky(W)
    else:
        W = case.prior_w.draw(rng, size=(N, d))
        Lw = np.sqrt(W)[:, :, None] * np.eye(d)
    theta, y = _simulate(case, rng, N, Lw, np.broadcast_to(np.sqrt(V)[:, None, :], (N, T, p)))
    y[:, ~case.obs] = np.nan
    return {"V": V, "W": W, "theta": theta, "y": y}


# ---- the statistics and the conjugate draws, from the formulas of include/dlm_engine.h --------------------------------------------
def statistics(case, theta, y, mutant=None):
    """(ssy [N][p], n [N][p], ss [N][d], outer [N][d][d], transitions) of a state draw."""
    T = case.mat.T
    state = theta[:, :-1] if mutant == "pair_theta_t" else theta[:, 1:]
    resid = y - np.einsum("tdj,ntd->ntj", case.F, state)
    obs = ~np.isnan(y)
    ssy = np.where(obs, np.nan_to_num(resid) ** 2, 0.0).sum(axis=1)
    n = np.full(ssy.shape, float(T)) if mutant == "missing_counted" else obs.sum(axis=1).astype(np.float64)
    diff = theta[:, 1:] - np.einsum("tde,nte->ntd", case.G, theta[:, :-1])
    weight = np.ones(T) if mutant == "ss_without_dt" else 1.0 / case.dt
    if mutant == "first_transition_dropped":
        weight = weight.copy(); weight[0] = 0.0
    ss = np.einsum("ntd,t->nd", diff * diff, weight)
    outer = np.einsum("nti,ntj,t->nij", diff, diff, weight)
    return ssy, n, ss, outer, float(T)


def conjugate_draws(case, stats, rng, mutant=None):
    ssy, n, ss, outer, T = stats
    V = 1.0 / rng.gamma(case.prior_v.shape + 0.5 * n, 1.0 / (case.prior_v.scale + 0.5 * ssy))
    if case.wishart:
        W = np.stack([InverseWishart(case.prior_w.nu + T, case.prior_w.psi + o).draw(rng) for o in outer])
    else:
        count = T - 1.0 if mutant == "shape_T_minus_1" else T
        W = 1.0 / rng.gamma(case.prior_w.shape + 0.5 * count, 1.0 / (case.prior_w.scale + 0.5 * ss))
    return V, W


def sweep_host(case, state, mutant=None, rng=None):
    """One sweep on the CPU: theta | (V, W, y) by the oracle's filter and backward sampler (one call per series, every return code
    checked), then (V, W) | (theta, y) in NumPy.  Returns the new state; `state` is not written to."""
    rng = np.random.default_rng([SEED, 1]) if rng is None else rng
    mat = case.mat
    d, T = mat.d, mat.T
    om = oracle.Model(mat.d, mat.p, mat.T, mat.F, mat.G, mat.g_index, mat.dt, mat.f_stride)
    y, N = state["y"], state["y"].shape[0]
    theta = np.empty((N, T + 1, d))
    z = rng.standard_normal((N, T + 1, d))
    for k, par in enumerate(case.params_list(state["V"], state["W"])):
        f = oracle.kf_filter(om, par.v, par.w, par.m0, par.c0, y[k])
        b = oracle.backward_sample(om, par.w, f, z[k], factor="chol")
        assert f["rc"] == 0 and b["rc"] == 0, (case.name, k, f["rc"], b["rc"])
        theta[k] = b["theta"]
    V, W = conjugate_draws(case, statistics(case, theta, y, mutant), rng, mutant)
    return {"V": V, "W": W, "theta": theta, "y": y}


# ---- the checks ----------------------------------------------------------------------------------------------------------------------
def _whitened(case, V, W, theta, y):
    """(transitions [N][T][d], residuals against theta[t+1] [N][T][p], residuals against theta[t])."""
    w_diag = np.diagonal(W, axis1=1, axis2=2) if case.wishart else W
    diff = theta[:, 1:] - np.einsum("tde,nte->ntd", case.G, theta[:, :-1])
    trans = diff / np.sqrt(w_diag[:, None, :] * case.dt[None, :, None])
    sd = np.sqrt(V)[:, None, :]
    right = (y - np.einsum("tdj,ntd->ntj", case.F, theta[:, 1:])) / sd
    wrong = (y - np.einsum("tdj,ntd->ntj", case.F, theta[:, :-1])) / sd
    return trans, right, wrong


def _deviation(x, N):
    """Largest |mean| and |var - 1| over the columns of x [N][..], in standard errors."""
    return float(np.abs(x.mean(axis=0)).max() * math.sqrt(N)), float(np.abs(x.var(axis=0) - 1.0).max() / math.sqrt(2.0 / N))


def measure(case, V, W, theta, y, start=None):
    """The figures behind `checks`: p-values of the marginals, whitened deviations in standard errors, the move from `start`."""
    from scipy import stats as ss
    N = V.shape[0]
    pv = {}
    for j in range(case.mat.p):
        pv[f"V{j}"] = float(ss.kstest(V[:, j], ss.invgamma(case.prior_v.shape, scale=case.prior_v.scale).cdf).pvalue)
    if case.wishart:
        # W ~ InverseWishart(nu, Psi) of dimension d has W_ii ~ InverseGamma((nu - d + 1) / 2, Psi_ii / 2); the two-sample test against host
        # draws of the same InverseWishart.draw needs no such argument and also covers the trace and the determinant
        ref_diag, ref_tr, ref_ld = case.iw_reference()
        diag, tr, ld = wishart_summaries(W)
        for i in range(case.mat.d):
            pv[f"W{i}"] = float(ss.ks_2samp(diag[:, i], ref_diag[:, i]).pvalue)
        pv["trW"] = float(ss.ks_2samp(tr, ref_tr).pvalue)
        pv["logdetW"] = float(ss.ks_2samp(ld, ref_ld).pvalue)
    else:
        for i in range(case.mat.d):
            pv[f"W{i}"] = float(ss.kstest(W[:, i], ss.invgamma(case.prior_w.shape, scale=case.prior_w.scale).cdf).pvalue)
    trans, right, wrong = _whitened(case, V, W, theta, y)
    out = {"N": N, "p": pv, "p_min_V": min(v for k, v in pv.items() if k[0] == "V"),
           "p_min_W": min(v for k, v in pv.items() if k[0] != "V"),
           "trans": _deviation(trans, N), "resid": _deviation(right[:, case.obs], N), "control": _deviation(wrong[:, case.obs], N)}
    out["p_min"] = min(out["p_min_V"], out["p_min_W"])
    out["dev_max"] = max(out["trans"] + out["resid"])
    out["moved"] = None if start is None else float(np.mean(np.abs(V - start["V"]) / start["V"]))
    return out


def checks(case, V, W, theta, y, start=None):
    """The assertions shared by the host and GPU tests; V [N][p] and W [N][d] diagonals (W [N][d][d] for a Wishart case), theta the
    final state draw, `start` the exact start (for the new-draw check).  Raises CheckFailed naming the first check that fails, in the
    order marginal V, marginal W, whitened transition, whitened residual, pairing control, new draw; returns the figures."""
    assert np.isfinite(V).all() and np.isfinite(W).all() and np.isfinite(theta).all(), "a chain left the finite numbers"
    m = measure(case, V, W, theta, y, start)
    print(f"{case.name}: N {m['N']}  min p  V {m['p_min_V']:.3g}  W {m['p_min_W']:.3g}   whitened (mean, var) in standard errors: transitions "
          f"{m['trans'][0]:.2f} {m['trans'][1]:.2f}  residuals {m['resid'][0]:.2f} {m['resid'][1]:.2f}  against theta[t] {m['control'][0]:.1f} "
          f"{m['control'][1]:.1f}   moved {m['moved']}")
    level = P_MARGINAL / case.n_marginals
    for name, key in (("marginal V", "p_min_V"), ("marginal W", "p_min_W")):
        if not m[key] >= level:
            raise CheckFailed(name, f"{case.name}: p {m[key]:.3g} < {level:.3g}; " + ", ".join(f"{k} {v:.3g}" for k, v in m["p"].items()))
    for name, key in (("whitened transition", "trans"), ("whitened residual", "resid")):
        if not max(m[key]) <= SE_BOUND:
            raise CheckFailed(name, f"{case.name}: mean {m[key][0]:.2f}, variance {m[key][1]:.2f} standard errors")
    if not max(m["control"]) > SE_BOUND:
        raise CheckFailed("pairing control", f"{case.name}: y_t - F^T theta_t also looks white ({m['control']}): the check has no power here")
    if start is not None and not m["moved"] > NEW_DRAW_FLOOR:
        raise CheckFailed("new draw", f"{case.name}: mean |V_new - V_start| / V_start = {m['moved']:.3g}")
    return m


def run_host(case, N, K, mutant=None, seed=SEED):
    """K host sweeps from the exact start: (start, final state)."""
    start = exact_start(case, N, seed)
    rng = np.random.default_rng([seed, 2, sum(case.name.encode())])
    state = start
    for _ in range(K):
        state = sweep_host(case, state, mutant, rng)
    return start, state


# ---- Student-t ------------------------------------------------------------------------------------------------------------------------
ST_MUTANTS = ("pair_theta_t", "hastings_without_proposal", "missing_observed_shape")
# (the first check that fails, in st_checks' order, on the c2 case: residuals against theta_t are too wide, which first drags nu down)
ST_MUTANT_CHECK = {"pair_theta_t": "nu", "hastings_without_proposal": "nu", "missing_observed_shape": "v"}


class StCase:
    """A Student-t case: univariate model, W_ii ~ InverseGamma(prior_w), nu ~ Poisson(rate) on nu >= 1, the scale s fixed; 10 % of
    y masked by a mask fixed per case.  prior = the (rate, proposal size, shape, scale) tuple of Engine.studentt_step."""

    def __init__(self, name, mod, T, prior, scale, m0, c0, routes, N=8192, K=3, host_N=512):
        self.name, self.mod, self.prior, self.scale, self.routes, self.N, self.K, self.host_N = name, mod, prior, float(scale), routes, N, K, host_N
        self.times = np.arange(1, T + 1, dtype=np.float64)
        self.mat = materialise(mod, self.times)
        self.m0 = np.asarray(m0, dtype=np.float64).reshape(self.mat.d)
        self.c0 = np.asarray(c0, dtype=np.float64).reshape(self.mat.d, self.mat.d)
        self.dt, self.G, self.F = model_tables(self.mat)
        self.prior_w = InverseGamma(prior[2], prior[3])
        rng = np.random.default_rng([SEED, 3, sum(name.encode())])
        self.obs = np.ones((T, 1), dtype=bool)
        self.obs[rng.choice(T, size=max(1, round(0.1 * T)), replace=False), 0] = False

    def nu_pmf(self, kmax):
        """Poisson(rate) conditioned on nu >= 1, on 1 .. kmax."""
        lam = self.prior[0]
        k = np.arange(1, kmax + 1)
        pm = np.exp(k * math.log(lam) - lam - np.array([math.lgamma(v + 1.0) for v in k]))
        return pm / (1.0 - math.exp(-lam))


def _st_cases():
    T = 10
    rng = np.random.default_rng(1302)
    x = 1.0 + 0.5 * rng.standard_normal(T)
    c2 = _c2_model()
    tv = Dlm(lambda t: c2.f(t) * x[int(t) - 1], c2.g)          # a time-varying F (as _inputs(..., tv_f=True) of tests/test_studentt_gpu.py has at d = 1)
    prior = (3.0, 1.0, 4.0, 1.5)
    S = _lib.OPT_FFBS_SIMSMOOTH
    cases = [StCase("level", Dlm.polynomial(1), T, prior, 1.5, [0.5], [[4.0]], {"sampler": (0, "lane-sampler"), "simsmooth": (S, "sparse16-simsmooth")}),
             StCase("c2", tv, T, prior, 1.5, rng.standard_normal(13), 4.0 * np.eye(13), {"sampler": (0, "sparse16-sampler")}, host_N=256)]
    return {c.name: c for c in cases}


ST_CASES = _st_cases()


def st_exact_start(case, N, seed=SEED):
    """{"nu" [N] int32, "W" [N][d], "v" [N][T], "theta" [N][T+1][d], "y" [N][T]} from the joint law given s."""
    rng = np.random.default_rng([seed, 4, sum(case.name.encode())])
    d, T = case.mat.d, case.mat.T
    nu = rng.poisson(case.prior[0], N)
    while (nu == 0).any():                       # rejection: Poisson(rate) conditioned on nu >= 1
        again = nu == 0
        nu[again] = rng.poisson(case.prior[0], int(again.sum()))
    W = case.prior_w.draw(rng, size=(N, d))
    v = (0.5 * nu[:, None] * case.scale) / rng.gamma(0.5 * nu[:, None], 1.0, size=(N, T))
    theta, y = _simulate(case, rng, N, np.sqrt(W)[:, :, None] * np.eye(d), np.sqrt(v)[:, :, None])
    y = y[:, :, 0]
    y[:, ~case.obs[:, 0]] = np.nan
    return {"nu": nu.astype(np.int32), "W": W, "v": v, "theta": theta, "y": y}


def st_measure(case, nu, W, v, theta, y, start=None):
    from scipy import stats as ss
    N = nu.shape[0]
    kmax = 1
    pmf = case.nu_pmf(60)
    while pmf[kmax:].sum() * N >= 20.0 and pmf[kmax - 1] * N >= 20.0:       # pool the tail so that every expected count is >= 20
        kmax += 1
    expected = np.concatenate([pmf[:kmax - 1], [1.0 - pmf[:kmax - 1].sum()]]) * N
    counts = np.bincount(np.minimum(nu, kmax), minlength=kmax + 1)[1:]
    out = {"N": N, "p_nu": float(ss.chisquare(counts, expected).pvalue)}
    iw = ss.invgamma(case.prior_w.shape, scale=case.prior_w.scale).cdf
    out["p_W"] = min(float(ss.kstest(W[:, i], iw).pvalue) for i in range(case.mat.d))
    u = ss.invgamma.cdf(v, 0.5 * nu[:, None], scale=0.5 * nu[:, None] * case.scale)
    out["p_v"] = float(ss.kstest(u.reshape(-1), "uniform").pvalue)
    out["p_v_missing"] = float(ss.kstest(u[:, ~case.obs[:, 0]].reshape(-1), "uniform").pvalue)
    f1 = np.einsum("td,ntd->nt", case.F[:, :, 0], theta[:, 1:])
    f0 = np.einsum("td,ntd->nt", case.F[:, :, 0], theta[:, :-1])
    o = case.obs[:, 0]
    out["resid"] = _deviation(((y - f1) / np.sqrt(v))[:, o], N)
    out["control"] = _deviation(((y - f0) / np.sqrt(v))[:, o], N)
    diff = theta[:, 1:] - np.einsum("tde,nte->ntd", case.G, theta[:, :-1])
    out["trans"] = _deviation(diff / np.sqrt(W[:, None, :] * case.dt[None, :, None]), N)
    out["p_min"] = min(out["p_nu"], out["p_W"], out["p_v"], out["p_v_missing"])
    out["moved"] = None if start is None else (float(np.mean(np.abs(W - start["W"]) / start["W"])), float(np.mean(nu != start["nu"])),
                                                  float(np.median(np.abs(v - start["v"]) / start["v"])))
    out["dev_max"] = max(out["trans"] + out["resid"])
    return out


def st_checks(case, nu, W, v, theta, y, start=None):
    """nu by chi-square against the truncated Poisson, W_ii by KS against its prior, u_t = cdf of InverseGamma(nu / 2, nu s / 2) at v_t
    (at the final nu) against the uniform -- all t, and the missing t alone --, the whitened residuals and transitions.  The order of the
    assertions: nu, W, v, whitened transition, whitened residual, pairing control."""
    assert np.isfinite(W).all() and np.isfinite(v).all() and np.isfinite(theta).all() and (nu >= 1).all()
    m = st_measure(case, nu, W, v, theta, y, start)
    print(f"student-t {case.name}: N {m['N']}  p  nu {m['p_nu']:.3g}  W {m['p_W']:.3g}  v {m['p_v']:.3g}  v at the missing t {m['p_v_missing']:.3g}   whitened "
          f"(mean, var) in standard errors: transitions {m['trans'][0]:.2f} {m['trans'][1]:.2f}  residuals {m['resid'][0]:.2f} {m['resid'][1]:.2f}  "
          f"against theta[t] {m['control'][0]:.1f} {m['control'][1]:.1f}")
    level = P_MARGINAL / (case.mat.d + 3)
    for name, p in (("nu", m["p_nu"]), ("W", m["p_W"]), ("v", min(m["p_v"], m["p_v_missing"]))):
        if not p >= level:
            raise CheckFailed(name, f"student-t {case.name}: p {p:.3g} < {level:.3g}")
    for name, key in (("whitened transition", "trans"), ("whitened residual", "resid")):
        if not max(m[key]) <= SE_BOUND:
            raise CheckFailed(name, f"student-t {case.name}: mean {m[key][0]:.2f}, variance {m[key][1]:.2f} standard errors")
    if not max(m["control"]) > SE_BOUND:
        raise CheckFailed("pairing control", f"student-t {case.name}: y_t - F_t^T theta_t also looks white ({m['control']})")
    if start is not None:
        print(f"student-t {case.name}: moved: mean |W_new - W_start| / W_start {m['moved'][0]:.3f}, share of chains with a new nu {m['moved'][1]:.3f}, "
              f"median |v_new - v_start| / v_start {m['moved'][2]:.3f}")
        if not (m["moved"][0] > NEW_DRAW_FLOOR and m["moved"][1] > ST_NU_MOVED_FLOOR and m["moved"][2] > NEW_DRAW_FLOOR):
            raise CheckFailed("new draw", f"student-t {case.name}: W moved by {m['moved'][0]:.3g}, nu changed in {m['moved'][1]:.3g} of the chains, "
                                          f"v moved by {m['moved'][2]:.3g}")
    return m


def st_sweep_host(case, state, it, mutant=None, seed=SEED, rng=None):
    """One sweep on the CPU: theta | (v, W, y) by the oracle with the V_t stream v, then the NumPy `step` of tests/sampler_restatement.py
    (imported: the restatement the kernel is pinned to draw for draw) with scale_in = s; its scale_out is ignored.  The mutants wrap it."""
    import sampler_restatement as st
    rng = np.random.default_rng([seed, 5, it]) if rng is None else rng
    mat = case.mat
    d, T = mat.d, mat.T
    om = oracle.Model(mat.d, mat.p, mat.T, mat.F, mat.G, mat.g_index, mat.dt, mat.f_stride)
    y, N, s = state["y"], state["y"].shape[0], case.scale
    Fm = case.F[:, :, 0]
    out = {"nu": np.empty(N, np.int32), "W": np.empty((N, d)), "v": np.empty((N, T)), "theta": np.empty((N, T + 1, d)), "y": y}
    z = rng.standard_normal((N, T + 1, d))
    for k in range(N):
        Wk = np.diag(state["W"][k])
        f = oracle.kf_filter(om, state["v"][k].reshape(T, 1, 1), Wk, case.m0, case.c0, y[k])
        b = oracle.backward_sample(om, Wk, f, z[k], factor="chol")
        assert f["rc"] == 0 and b["rc"] == 0, (case.name, k, f["rc"], b["rc"])
        theta = b["theta"]
        diff = theta[1:] - np.einsum("tde,te->td", case.G, theta[:-1])
        stats = np.concatenate([[0.0, 0.0], (diff * diff / case.dt[:, None]).sum(axis=0), [float(T)]])      # [ssy | n | ss | T]: the step reads ss and T
        nu0 = int(state["nu"][k])
        paired = np.concatenate([theta[:1], theta[:-1]]) if mutant == "pair_theta_t" else theta     # record t + 1 holds theta[t]: y_t meets theta_t
        v, _, nu1, wd, acc, _ = st.step(Fm, y[k], paired, stats, case.prior, s, nu0, seed=seed, series=k, it=it, literal=False)
        if mutant == "hastings_without_proposal":
            nu1 = _nu_move_without_proposal(st, case, y[k], theta, nu0, seed, k, it)
        if mutant in ("hastings_without_proposal", "missing_observed_shape"):
            e = y[k] - np.einsum("td,td->t", Fm, theta[1:])
            o = ~np.isnan(e)
            shape = np.where(o | (mutant == "missing_observed_shape"), 0.5 * (nu1 + 1.0), 0.5 * nu1)
            beta = 0.5 * nu1 * s + np.where(o, 0.5 * np.nan_to_num(e) ** 2, 0.0)
            v = beta / st.gamma_unit(shape, seed, k, it, np.arange(T), st.KEY_STUDENTT)
        out["nu"][k], out["W"][k], out["v"][k], out["theta"][k] = nu1, wd, v, theta
    return out


def _nu_move_without_proposal(st, case, y, theta, nu0, seed, series, it):
    """The Metropolis-Hastings move of nu as `step` makes it (the same proposal, from the same draws, and the same uniform) but accepted
    on the ratio of the targets alone."""
    from scipy import stats as ss
    lam, r = case.prior[0], case.prior[1]
    g = st.gamma_unit(r, seed, series, it, st.ST_SLOT_PROP_GAMMA, st.KEY_STUDENTT)[0]
    nup = st.poisson(g * (nu0 / r), seed, series, it) + 1.0
    e = y - np.einsum("td,td->t", case.F[:, :, 0], theta[1:])
    e = e[~np.isnan(e)]
    target = lambda nu: ss.t.logpdf(e, nu, scale=math.sqrt(case.scale)).sum() + nu * math.log(lam) - math.lgamma(nu + 1.0)
    u = st.gibbs_rand(seed, series, it, [st.ST_SLOT_ACCEPT], 0, 0, st.KEY_STUDENTT)[0][0]
    return int(nup) if math.log(u) < target(nup) - target(float(nu0)) else nu0


def st_run_host(case, N, K, mutant=None, seed=SEED):
    state = st_exact_start(case, N, seed)
    for it in range(K):
        state = st_sweep_host(case, state, it, mutant, seed)
    return state


# ---- the rehearsal table ----------------------------------------------------------------------------------------------------------------
def rehearse(N=None, K=None, out=sys.stdout):
    """Every case through the oracle sampler, `level` and `c2` through every mutant, at the GPU tests' N and K (or the ones given)."""
    for case in CASES.values():
        n, k = N or case.N, K or case.K
        t0 = time.time()
        start, fin = run_host(case, n, k)
        m = measure(case, fin["V"], fin["W"], fin["theta"], fin["y"], start)
        print(f"{case.name:10s} N {n} K {k}  correct: min p {m['p_min']:.3g} (V {m['p_min_V']:.3g}, W {m['p_min_W']:.3g})  whitened max {m['dev_max']:.2f} se  "
              f"control {max(m['control']):.1f} se  moved {m['moved']:.3f}  [{time.time() - t0:.1f} s]", file=out, flush=True)
        if case.name in ("level", "c2"):
            for mut in MUTANTS:
                start, fin = run_host(case, n, k, mut)
                m = measure(case, fin["V"], fin["W"], fin["theta"], fin["y"], start)
                key = "p_min_V" if MUTANT_CHECK[mut] == "marginal V" else "p_min_W"
                print(f"{'':10s} {mut:26s} {MUTANT_CHECK[mut]}: p {m[key]:.3g}", file=out, flush=True)


def st_rehearse(N=None, K=None, out=sys.stdout):
    for case in ST_CASES.values():
        n, k = N or case.N, K or case.K
        for mut in (None,) + ST_MUTANTS:
            t0 = time.time()
            fin = st_run_host(case, n, k, mut)
            m = st_measure(case, fin["nu"], fin["W"], fin["v"], fin["theta"], fin["y"])
            print(f"student-t {case.name:6s} N {n} K {k} {str(mut):26s} p: nu {m['p_nu']:.3g}  W {m['p_W']:.3g}  v {m['p_v']:.3g}  v missing {m['p_v_missing']:.3g}  "
                  f"residuals {m['resid'][0]:.2f} {m['resid'][1]:.2f} se  transitions {max(m['trans']):.2f} se  control {max(m['control']):.1f} se  [{time.time() - t0:.1f} s]",
                  file=out, flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    run = rehearse
    if args[:1] == ["studentt"]:
        run, args = st_rehearse, args[1:]
    run(*[int(a) for a in args])
