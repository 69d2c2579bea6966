"""The inputs of the Storvik filter tests, made from seeds: the table of shapes the kernel is held to on the GPU (tests/test_storvik_gpu.py)
and that tests/test_storvik_host.py checks on the restatement alone, and the two models of the evidence checks with their grid integrals.
Every entry of the table is the smallest shape at which its part of the kernel can go wrong:

  P   64 one slot of particles, 128 a carry between two slots, 192 an odd slot count, 1024 the edge of the particle field;
  d   1, 2, 3 and the limit 16, with a dense G; the two largest holdings the kernel keeps in LDS (d = 16 with P = 512, d = 8 with P = 1024);
  T   1, 2, 12 and 24;  a missing value first, in the middle and last;  an irregular grid with three distinct G and a dt = 0 inside;
  N   1, 2, 5, 67;  shared and per-series m0, C0 and priors;  n0 = -1, P (always resample), 0 (never);  a prior shape of 0.6 on W (the boost of
      the Gamma below 1);  learn_v = 0 for each of the six families;  literal = 1.

`reference(name)` runs the restatement once per process and keeps the result."""
import functools

import numpy as np
from scipy.special import gammaln

import pf_cases as pc
import pf_restatement as pr
import storvik_restatement as sr


def case(name, d, P, T, N, family=pr.GAUSSIAN, learn_v=True, n0=-1, literal=False, missing=(), irregular=False, per_series=False, seed=1,
         v_scale=1.0, w_shape=4.0):
    return dict(name=name, d=d, P=P, T=T, N=N, family=family, learn_v=learn_v, n0=n0, literal=literal, missing=tuple(missing),
                irregular=irregular, per_series=per_series, seed=seed, v_scale=v_scale, w_shape=w_shape)


TABLE = [
    case("p64-d1", 1, 64, 24, 5),
    case("p128-d2-missing-per-series", 2, 128, 24, 5, missing=(0, 11, 23), per_series=True),
    case("p192-d3-irregular", 3, 192, 24, 5, irregular=True),
    case("p1024-d2", 2, 1024, 12, 1),
    case("d16-p64", 16, 64, 12, 1),
    case("d16-p512-t2", 16, 512, 2, 2),
    case("d8-p1024-t2", 8, 1024, 2, 2),
    case("t1", 2, 128, 1, 5),
    case("n67-per-series", 1, 64, 12, 67, per_series=True),
    case("always", 2, 128, 12, 5, n0=128),
    case("never", 2, 128, 12, 5, n0=0, v_scale=40.0),   # (a wide likelihood: without resampling a narrow one leaves ONE particle)
    case("w-shape-0.6", 2, 128, 12, 5, w_shape=0.6),
    case("literal-gaussian", 2, 128, 12, 5, literal=True),
] + [case("learnv0-" + pc.FAMILY_NAMES[f], 2, 128, 12, 5, family=f, learn_v=False) for f in range(6)]
FORCED = {"always": 1.0, "never": 0.0}   # n0 = P and n0 = 0 leave the resampling test one branch
DEVICE_RUNS = ("p128-d2-missing-per-series", "p192-d3-irregular", "d8-p1024-t2")


def by_name(name):
    return next(c for c in TABLE if c["name"] == name)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The arrays of a table entry: what the restatement takes, and through `engine_run` the engine.  The data are simulated from the model
    at the variances the priors are centred on (prior mean = scale / (shape - 1) for the shape 4 of the table; the shape 0.6 keeps the scale)."""
    c = by_name(name)

    def priors(d, Wd, V, N, scale):
        prior_w = np.stack([np.full(d, c["w_shape"]), 3.0 * Wd], axis=1)          # [d][2] = (shape, scale)
        prior_v = np.array([4.0, 3.0 * V])
        if scale is not None:
            prior_w = prior_w[None] * np.stack([np.ones(N), scale], axis=1)[:, None, :] + np.stack([0.25 * np.arange(N), np.zeros(N)], axis=1)[:, None, :]
            prior_v = prior_v[None] * np.stack([np.ones(N), scale[::-1]], axis=1) + np.stack([0.5 * (np.arange(N) % 3), np.zeros(N)], axis=1)
        return prior_w, prior_v if c["learn_v"] else None

    return pc.learner_inputs(c, 3000, priors)


def run_args(name, **over):
    c, a = by_name(name), inputs(name)
    kw = dict(a, family=c["family"], learn_v=c["learn_v"], P=c["P"], n0=c["n0"], literal=c["literal"], seed=40 + c["seed"], series_offset=3,
              iteration=5)
    kw.update(over)
    return kw


@functools.lru_cache(maxsize=None)
def reference(name):
    return sr.run(**run_args(name))


def engine_run(eng, kw, device=False):
    """Engine.storvik_filter on the arguments `sr.run` takes -> NumPy arrays."""
    return pc.engine_run(eng, kw, "storvik_filter", device)


# ---- the models of the evidence checks: Gaussian, T = 24, dt_0 = 0, y_7 missing, P = 128, n0 = -1, 4096 replicates that differ in the series
# index.  "level": G = F = 1, m0 = 0, C0 = 1, V ~ IG(4, 3) and W ~ IG(4, 0.9) both learned, data simulated at V = 1, W = 0.3.  "dense": d = 2 with
# a dense non-symmetric G, V = 1 known (learn_v = 0), W_1 ~ IG(4, 0.9), W_2 ~ IG(4, 0.45), data simulated at W = diag(0.3, 0.15).
# The exact evidence log Z = log of the integral of (Kalman likelihood) x (priors) over the two unknown log-variances, by the rectangle rule on
# a grid of GRID^2 points over [LOG_LO, LOG_HI]^2: the integrand is smooth and falls below 1e-30 of its peak at the edges (asserted), where
# the rectangle rule converges faster than any power of the spacing; halving the spacing changes log Z by less than 1e-9 (asserted in the
# host test), against standard errors of the estimates of about 1e-2.
REPLICATES, EVIDENCE_T, EVIDENCE_P = 4096, 24, 128
LOG_LO, LOG_HI, GRID = -7.0, 7.0, 281
SIGMAS = 4.0          # the evidence checks: within 4 of the estimate's own standard errors
# The posterior means at T of the "level" model, v_mean and w_mean averaged over the replicates against the grid's E[V | y], E[W | y]: ratio
# estimators with a bias of order 1 / P.  Bound: 2 % relative at P = 1024, with as many replicates as keep the host test under a minute.
# Measured on the restatement (96 replicates): v_mean 0.88118 against 0.88722 (-0.68 %), w_mean 0.41126 against 0.41317 (-0.46 %); with
# literal = True v_mean is 4.34862, 4.90 times the grid's.
MEANS_P, MEANS_REPLICATES, MEANS_RTOL = 1024, 96, 0.02


@functools.lru_cache(maxsize=None)
def evidence_inputs(which):
    rng = np.random.default_rng(177 if which == "level" else 178)
    T = EVIDENCE_T
    if which == "level":
        d, G, F, Wd = 1, np.eye(1), np.array([1.0]), np.array([0.3])
        prior_w, prior_v, learn_v = np.array([[4.0, 0.9]]), np.array([4.0, 3.0]), True
    else:
        d = 2
        G = np.array([[0.9, 0.25], [-0.2, 0.85]])
        F, Wd = np.array([1.0, 0.5]), np.array([0.3, 0.15])
        prior_w, prior_v, learn_v = np.array([[4.0, 0.9], [4.0, 0.45]]), None, False
    m0, C0 = np.zeros(d), np.eye(d)
    dt = np.array([0.0] + [1.0] * (T - 1))
    x = np.linalg.cholesky(C0) @ rng.standard_normal(d)
    y = np.empty(T)
    for t in range(T):
        if dt[t] != 0.0:
            x = G @ x + np.sqrt(Wd) * rng.standard_normal(d)
        y[t] = F @ x + rng.standard_normal()
    y[7] = np.nan
    return dict(F=F, G=G[None], g_index=None, dt=dt, V=1.0, W=np.diag(Wd), m0=m0, C0=C0, y=y, nu=None, prior_w=prior_w, prior_v=prior_v,
                learn_v=learn_v)


def evidence_args(which, replicates=REPLICATES, **over):
    a = dict(evidence_inputs(which))
    a["y"] = np.tile(a["y"], (replicates, 1))
    kw = dict(a, family=pr.GAUSSIAN, P=EVIDENCE_P, n0=-1, literal=False, seed=11, series_offset=0, iteration=0)
    kw.update(over)
    return kw


def kalman_loglik_grid(a, V, Wd):
    """The Kalman log-likelihood of the model's one series on the filter's conventions (dt == 0: no advance; a missing y: no update),
    vectorised: V [...] and Wd [...][d] broadcast against one another."""
    F, G, y, dt = a["F"], a["G"][0], a["y"], a["dt"]
    d = F.size
    shape = np.broadcast(V, Wd[..., 0]).shape
    m = np.broadcast_to(a["m0"], shape + (d,)).copy()
    C = np.broadcast_to(a["C0"], shape + (d, d)).copy()
    Wm = Wd[..., :, None] * np.eye(d)
    ll = np.zeros(shape)
    for t in range(len(y)):
        if dt[t] != 0.0:
            m = m @ G.T
            C = G @ C @ G.T + Wm * dt[t]
        if not np.isnan(y[t]):
            f = m @ F
            CF = C @ F
            q = CF @ F + V
            e = y[t] - f
            ll = ll - 0.5 * np.log(2.0 * np.pi * q) - 0.5 * e * e / q
            K = CF / q[..., None]
            m = m + K * e[..., None]
            C = C - K[..., :, None] * K[..., None, :] * q[..., None, None]
    return ll


def log_inverse_gamma(v, shape, scale):
    return shape * np.log(scale) - gammaln(shape) - (shape + 1.0) * np.log(v) - scale / v


@functools.lru_cache(maxsize=None)
def exact(which, grid=GRID):
    """(log Z, the posterior means of the two unknown variances at T, the integrand's largest value on the edge of the grid relative to its
    peak): for "level" the unknowns are (V, W), for "dense" (W_1, W_2)."""
    a = evidence_inputs(which)
    u = np.linspace(LOG_LO, LOG_HI, grid)
    h = u[1] - u[0]
    A, B = np.meshgrid(np.exp(u), np.exp(u), indexing="ij")
    if which == "level":
        ll = kalman_loglik_grid(a, A, B[..., None])
        lp = log_inverse_gamma(A, *a["prior_v"]) + log_inverse_gamma(B, *a["prior_w"][0])
    else:
        ll = kalman_loglik_grid(a, np.float64(a["V"]), np.stack([A, B], axis=-1))
        lp = log_inverse_gamma(A, *a["prior_w"][0]) + log_inverse_gamma(B, *a["prior_w"][1])
    lt = ll + lp + np.log(A) + np.log(B)          # the Jacobian of the log scale
    peak = lt.max()
    wt = np.exp(lt - peak)
    edge = max(wt[0].max(), wt[-1].max(), wt[:, 0].max(), wt[:, -1].max())
    tot = wt.sum()
    return float(peak + np.log(tot) + 2.0 * np.log(h)), (float((wt * A).sum() / tot), float((wt * B).sum() / tot)), float(edge)


def unbiasedness(ll_hat, log_z):
    """(mean of exp(ll_hat - log Z), its standard error from the sample, the largest ratio)"""
    r = np.exp(np.asarray(ll_hat) - log_z)
    return float(r.mean()), float(r.std(ddof=1) / np.sqrt(r.size)), float(r.max())


def final_variance_means(out, a):
    """(v_mean, w_mean [d]) at the last step from a run's scale_mean [N][T][d+1], averaged over the series: scale_mean / (shape - 1) with the
    shapes the time grid and the missing pattern fix."""
    y, dt = np.atleast_2d(a["y"]), a["dt"]
    d = out["scale_mean"].shape[2] - 1
    shape_w = a["prior_w"][:, 0] + 0.5 * float(np.count_nonzero(dt))
    shape_v = a["prior_v"][0] + 0.5 * float(np.count_nonzero(~np.isnan(y[0]))) if a["prior_v"] is not None else np.nan
    last = out["scale_mean"][:, -1]
    return float((last[:, d] / (shape_v - 1.0)).mean()), (last[:, :d] / (shape_w - 1.0)).mean(axis=0)
