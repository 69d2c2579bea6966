"""The exact SMOOTHING law of the d = 1, T = 12 cases of tests/pf_grid_reference.py (imported unchanged: the cases, their data, the
scipy.stats densities), for the particle-Gibbs tests (tests/test_pg_host.py, test_pg_gpu.py).

A conditional-SMC sweep leaves p(x_{0:T} | y) invariant.  Here that law is carried on the uniform grid of the state the grid filter uses,
with nothing taken from the kernel or its restatement.  The path has T + 1 records (dlm_ffbs_batch's convention): record 0 is the state
before the first step, y_t belongs to record t + 1, step t takes record t to record t + 1 through

  K_t(x, x') = N(x'; g_t x, W dt_t)    (dt_t = 0: x' = x, the step does not advance)       g_t(x') = p(y_t | F_t x', V)   (1 for a missing y_t).

  forward   alpha_0 = N(m0, C0),  alpha_{t+1}(x') ~ g_t(x') h sum_i K_t(x_i, x') alpha_t(x_i)           (the grid filter's recursion)
  backward  beta_T = 1,           beta_t(x) = h sum_j K_t(x, x_j) g_t(x_j) beta_{t+1}(x_j)              (dt_t = 0: beta_t = g_t beta_{t+1})
  record t:  p_t(x) ~ alpha_t(x) beta_t(x);   records (t, t + 1):  p(x, x') ~ alpha_t(x) K_t(x, x') g_t(x') beta_{t+1}(x')

`smoothing` returns per record the mean, the variance and the fourth central moment (the standard error of a sample variance is
sqrt((mu_4 - var^2) / N), not the Gaussian var sqrt(2 / N)), and per step the raw cross-moment E x_t x_{t+1} with the variance of the
product.  `sample_paths` draws exact paths backwards: x_T ~ alpha_T, x_t | x_{t+1} ~ alpha_t(x) K_t(x, x_{t+1}), a grid point each, then
every DISTINCT state (a dt_t = 0 step repeats one) is spread uniformly over its cell of width h (which adds h^2 / 12 to the variances: 0.1 %
of the smallest of them, a twentieth of the standard error of 4096 draws).  `spacing_error` is what halving h moves, in posterior
standard deviations: tests/test_pg_host.py asserts that it is below 1e-6."""
import functools

import numpy as np
from scipy import stats

import pf_grid_reference as gr
from pf_grid_reference import DT, F_T, G_INDEX, G_VALUES, NAMES, T  # noqa: F401

G_T = G_VALUES[G_INDEX]


def _grid(s, M):
    m, s2 = float(s["m0"]), float(s["C0"])
    lo, hi = m - gr.SPAN * np.sqrt(s2), m + gr.SPAN * np.sqrt(s2)
    for t in range(T):
        if DT[t] != 0.0:
            m, s2 = G_T[t] * m, G_T[t] * G_T[t] * s2 + s["W"] * DT[t]
            lo, hi = min(lo, m - gr.SPAN * np.sqrt(s2)), max(hi, m + gr.SPAN * np.sqrt(s2))
    return np.linspace(lo, hi, M)


def _kernel(x, t, W):
    """K[i][j] = N(x_j; g_t x_i, W dt_t)"""
    s = np.sqrt(W * DT[t])
    e = (x[None, :] - G_T[t] * x[:, None]) / s
    return np.exp(-0.5 * e * e) / (s * np.sqrt(2.0 * np.pi))


def _obs(family, s, t, x):
    """g_t on the grid, scaled by its maximum (1 for a missing y_t)"""
    if np.isnan(s["y"][t]):
        return np.ones_like(x)
    l = gr.obs_logpdf(family, s["y"][t], F_T[t] * x, s["V"], s["nu"])
    return np.exp(l - l.max())


@functools.lru_cache(maxsize=None)
def _law(name, q, M):
    """(x [M], alpha [T+1][M], beta [T+1][M], g [T][M]) of parameter set q, each row scaled to its own convenience"""
    fam, s = gr.by_name(name)["family"], gr.parameter_sets(name)[q]
    x = _grid(s, M)
    h = x[1] - x[0]
    alpha = np.empty((T + 1, M)); beta = np.empty((T + 1, M)); g = np.empty((T, M))
    alpha[0] = stats.norm.pdf(x, float(s["m0"]), np.sqrt(float(s["C0"])))
    for t in range(T):
        g[t] = _obs(fam, s, t, x)
        a = alpha[t] if DT[t] == 0.0 else h * (alpha[t] @ _kernel(x, t, s["W"]))
        a = a * g[t]
        alpha[t + 1] = a / (h * a.sum())
    beta[T] = 1.0
    for t in range(T - 1, -1, -1):
        b = g[t] * beta[t + 1]
        b = b if DT[t] == 0.0 else h * (_kernel(x, t, s["W"]) @ b)
        beta[t] = b / b.max()
    return x, alpha, beta, g


@functools.lru_cache(maxsize=None)
def smoothing(name, q=0, M=gr.M_STATE):
    """dict: mean, var, mu4 [T+1] of the records; cross, cross_var [T] of the products x_t x_{t+1}; filt_mean [T] (the grid filter's means,
    for the comparison with pf_grid_reference.exact)"""
    x, alpha, beta, g = _law(name, q, M)
    s = gr.parameter_sets(name)[q]
    p = alpha * beta
    p = p / p.sum(axis=1, keepdims=True)
    mean = p @ x
    c = x[None, :] - mean[:, None]
    out = dict(mean=mean, var=(p * c ** 2).sum(axis=1), mu4=(p * c ** 4).sum(axis=1), cross=np.empty(T), cross_var=np.empty(T),
               filt_mean=(alpha[1:] @ x) / alpha[1:].sum(axis=1))
    for t in range(T):
        if DT[t] == 0.0:          # the two records are one state
            e1, e2 = (p[t] * x ** 2).sum(), (p[t] * x ** 4).sum()
        else:
            J = alpha[t][:, None] * _kernel(x, t, s["W"]) * (g[t] * beta[t + 1])[None, :]
            J = J / J.sum()
            xx = x[:, None] * x[None, :]
            e1, e2 = (J * xx).sum(), (J * xx ** 2).sum()
        out["cross"][t], out["cross_var"][t] = e1, e2 - e1 * e1
    return out


def spacing_error(name, q=0):
    """the largest change of a mean, a standard deviation, a fourth root of mu4 and a cross-moment when the grid spacing is halved, in
    posterior standard deviations (the cross-moments: in products of the two)"""
    a, b = smoothing(name, q, gr.M_STATE), smoothing(name, q, 2 * gr.M_STATE - 1)
    sd = np.sqrt(b["var"])
    return float(max((np.abs(a["mean"] - b["mean"]) / sd).max(), (np.abs(np.sqrt(a["var"]) - sd) / sd).max(),
                     (np.abs(a["mu4"] ** 0.25 - b["mu4"] ** 0.25) / sd).max(), (np.abs(a["cross"] - b["cross"]) / (sd[:-1] * sd[1:])).max(),
                     (np.abs(np.sqrt(a["cross_var"]) - np.sqrt(b["cross_var"])) / (sd[:-1] * sd[1:])).max()))


def sample_paths(name, q, count, rng, M=gr.M_STATE):
    """`count` exact draws of x_{0:T} | y under parameter set q -> [count][T+1]"""
    x, alpha, beta, g = _law(name, q, M)
    s = gr.parameter_sets(name)[q]
    h = x[1] - x[0]

    def draw(pm):          # pm [count][M] unnormalised -> a grid index per row
        cdf = np.cumsum(pm, axis=1)
        u = rng.uniform(size=(count, 1)) * cdf[:, -1:]
        return np.minimum((cdf <= u).sum(axis=1), M - 1)
    idx = np.empty((count, T + 1), dtype=np.int64)
    idx[:, T] = draw(np.broadcast_to(alpha[T], (count, M)))
    for t in range(T - 1, -1, -1):
        if DT[t] == 0.0:
            idx[:, t] = idx[:, t + 1]
        else:
            idx[:, t] = draw(alpha[t][None, :] * _kernel(x, t, s["W"])[:, idx[:, t + 1]].T)
    path = np.empty((count, T + 1))
    for t in range(T, -1, -1):
        repeat = t < T and DT[t] == 0.0
        path[:, t] = path[:, t + 1] if repeat else x[idx[:, t]] + h * (rng.uniform(size=count) - 0.5)
    return path


@functools.lru_cache(maxsize=None)
def reference_paths(name, replicates, seed=28):
    """[replicates][T+1][1]: exact paths for the batch of gr.inputs(name, replicates) -- series n carries parameter set n mod SETS and is
    drawn from THAT set's law"""
    sets = gr.parameter_sets(name)
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    out = np.empty((replicates, T + 1, 1))
    for q, sl in enumerate(gr.quarters(name, replicates)):
        count = len(range(*sl.indices(replicates)))
        out[sl, :, 0] = sample_paths(name, q, count, rng)
    out.setflags(write=False)
    return out
