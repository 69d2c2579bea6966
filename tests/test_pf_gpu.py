"""dlm_pf_batch on the GPU (ParticleFilter.step / likelihood) and the particle-marginal Metropolis driver.

The kernel is held to its NumPy restatement (tests/pf_restatement.py) on the table of tests/pf_cases.py at the project's draw-for-draw
tolerance (the constants of tests/test_factorsv_gpu.py): the arithmetic is restated operation for operation and in the kernel's orders of
summation (the build contracts no a * b + c), so what remains is the last bits of log, exp, cos, sin and lgamma.  The ESS must be EQUAL,
and so must, in effect, the ancestors: a resampling that picked another particle anywhere leaves a final cloud that differs in the first
digit.  tests/test_pf_host.py shows that no comparison of the kernel's is within 1e-11 of flipping on these inputs.  Then: the batch does not
depend on how it is split, the estimate is unbiased and the means are the Kalman filter's on the device too, the bad series, and the driver.
What kernel and restatement could share -- every family, an irregular grid, g_index, F_t, per-series parameters: tests/test_pf_exact_gpu.py.

The largest relative difference seen on an MI355X is in profiles/r19_notes.md."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pf_cases as pc  # noqa: E402
import pf_restatement as pr  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dglm import INIT_ITERATION, BatchedParameters, Dglm, Metropolis, ParticleFilter  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters  # noqa: E402
from bayesian_dlms_amd.engine import Engine, EngineError  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-11, 1e-12
SIGMAS = 5.0
KEYS = ("ll", "mean", "ess", "cloud", "weights")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _rel(a, b):
    ok = np.isfinite(b)
    return float((np.abs(a[ok] - b[ok]) / (np.abs(b[ok]) + ATOL / RTOL)).max()) if ok.any() else 0.0


# ---- kernel against restatement ---------------------------------------------------------------------------------------------------------
# every entry through host arrays (the engine stages them), three of them through device arrays as well
RUNS = [(c["name"], False) for c in pc.TABLE] + [(n, True) for n in ("p128-d2-missing-per-series", "p192-d3-irregular", "d16-p1024-t2")]


@pytest.mark.parametrize("name,device", RUNS, ids=[n + ("-device" if dev else "") for n, dev in RUNS])
def test_kernel_matches_restatement(eng, name, device):
    ref = pc.reference(name)
    out = pc.engine_run(eng, pc.run_args(name), device=device)
    assert eng.last_variant == "pf-wave"
    np.testing.assert_array_equal(out["status"], ref["status"])
    np.testing.assert_array_equal(out["ess"], ref["ess"])
    print(f"{name}: largest relative difference " + ", ".join(f"{k} {_rel(out[k], ref[k]):.2e}" for k in KEYS))
    for k in KEYS:
        np.testing.assert_allclose(out[k], ref[k], rtol=RTOL, atol=ATOL, err_msg=k)


# ---- the batch does not depend on how it is split ---------------------------------------------------------------------------------------
def _slice(kw, lo, hi):
    """Series lo .. hi - 1 of a batch with per-series parameters, as a batch of its own."""
    cut = dict(kw, y=kw["y"][lo:hi], series_offset=kw["series_offset"] + lo)
    for k in ("V", "W", "m0", "C0"):
        cut[k] = kw[k][lo:hi]
    return cut


def test_halves_with_series_offset_equal_the_whole_batch(eng):
    kw = pc.run_args("n67-per-series")
    whole = pc.engine_run(eng, kw)
    again = pc.engine_run(eng, kw)
    lo, hi = pc.engine_run(eng, _slice(kw, 0, 34)), pc.engine_run(eng, _slice(kw, 34, 67), device=True)
    for k in KEYS + ("status",):
        np.testing.assert_array_equal(whole[k], again[k], err_msg=k)          # the same iteration: the same bits
        np.testing.assert_array_equal(whole[k], np.concatenate([lo[k], hi[k]]), err_msg=k)
    other = pc.engine_run(eng, dict(kw, iteration=kw["iteration"] + 1))
    assert np.all(other["ll"] != whole["ll"])          # another iteration: other draws for every series


# ---- unbiased on the device, means, P = 64 against P = 1024 ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["level", "dense"])
def test_likelihood_estimate_is_unbiased_and_means_are_the_kalman_filter_s(eng, which):
    _, ll = pc.exact(which)
    out = pc.engine_run(eng, pc.unbiased_args(which), device=True)
    m, se = pc.unbiasedness(out["ll"], ll)
    print(f"{which}: mean exp(ll_hat - ll) = {m:.5f} +- {se:.5f}")
    assert np.all(out["status"] == 0) and abs(m - 1.0) <= SIGMAS * se
    ms, ll = pc.exact(which, True)
    out = pc.engine_run(eng, pc.unbiased_args(which, True), device=True)
    z = pc.mean_z(out["mean"], ms)
    m, se = pc.unbiasedness(out["ll"], ll)
    print(f"{which}, diffuse: largest |mean - Kalman| = {z.max():.2f} standard errors; mean exp(ll_hat - ll) = {m:.5f} +- {se:.5f}")
    assert np.all(z <= SIGMAS) and abs(m - 1.0) <= SIGMAS * se


@pytest.mark.parametrize("family", [pr.POISSON, pr.STUDENTT], ids=["poisson", "studentt"])
def test_estimate_does_not_depend_on_the_number_of_particles(eng, family):
    """E exp(ll_hat) is the likelihood for every P: the means at P = 64 and P = 1024 agree within 5 combined standard errors."""
    name = "family-" + pc.FAMILY_NAMES[family]
    kw = pc.run_args(name)
    kw = dict(kw, y=np.tile(kw["y"][:1], (pc.REPLICATES, 1)), nu=None if kw["nu"] is None else 6.0, series_offset=0)
    ll = {P: pc.engine_run(eng, dict(kw, P=P), device=True)["ll"] for P in (64, 1024)}
    c = ll[1024].mean()
    (m1, s1), (m2, s2) = (pc.unbiasedness(ll[P], c) for P in (64, 1024))
    print(f"{name}: mean exp(ll_hat - c) = {m1:.5f} +- {s1:.5f} at P = 64, {m2:.5f} +- {s2:.5f} at P = 1024")
    assert abs(m1 - m2) <= SIGMAS * np.hypot(s1, s2)


# ---- status -------------------------------------------------------------------------------------------------------------------------------
def test_a_beta_series_with_y_outside_the_unit_interval_fails_alone(eng):
    kw = pc.run_args("family-beta")
    y = kw["y"].copy(); y[2, 5] = 1.5
    bad, good = pc.engine_run(eng, dict(kw, y=y)), pc.engine_run(eng, kw)
    assert bad["status"].tolist() == [0, 0, _lib.ST_NONFINITE, 0, 0] and bad["ll"][2] == -np.inf
    assert np.all(np.isfinite(bad["mean"][2, :5])) and np.all(np.isnan(bad["mean"][2, 5:])) and np.all(np.isnan(bad["ess"][2, 5:]))
    for k in KEYS:
        np.testing.assert_array_equal(np.delete(bad[k], 2, axis=0), np.delete(good[k], 2, axis=0), err_msg=k)
    ref = pr.run(**dict(kw, y=y))
    for k in KEYS:
        np.testing.assert_allclose(bad[k], ref[k], rtol=RTOL, atol=ATOL, err_msg=k)


def test_an_indefinite_w_or_c0_is_not_pd(eng):
    kw = pc.run_args("p128-d2-missing-per-series")
    W = kw["W"].copy(); W[1] = np.array([[1.0, 2.0], [2.0, 1.0]])
    C0 = kw["C0"].copy(); C0[3] = -C0[3]
    out = pc.engine_run(eng, dict(kw, W=W, C0=C0))
    assert out["status"].tolist() == [0, _lib.ST_NOT_PD, 0, _lib.ST_NOT_PD, 0]
    assert np.all(out["ll"][[1, 3]] == -np.inf) and np.all(np.isnan(out["cloud"][[1, 3]])) and np.all(np.isnan(out["mean"][[1, 3]]))
    ref = pc.reference("p128-d2-missing-per-series")
    for k in KEYS:
        np.testing.assert_array_equal(out[k][[0, 2, 4]], pc.engine_run(eng, kw)[k][[0, 2, 4]], err_msg=k)
        np.testing.assert_allclose(out[k][[0, 2, 4]], ref[k][[0, 2, 4]], rtol=RTOL, atol=ATOL, err_msg=k)


def test_engine_refuses_what_it_does_not_cover(eng):
    kw = pc.run_args("p64-d1")
    mat, par = pc.materialised(kw), pc.packed_params(kw, 5)
    for P in (96, 2048):
        with pytest.raises(EngineError, match="multiple of 64"):
            eng.particle_filter(mat, par, kw["y"], family=0, n_particles=P)
    with pytest.raises(EngineError, match="obs_param"):
        eng.particle_filter(mat, par, kw["y"], family=_lib.OBS_STUDENTT, n_particles=64)
    # straight at the C ABI: DLM_ERR_UNSUPPORTED with a message, no launch
    import ctypes
    from bayesian_dlms_amd.engine import _Host
    y = np.ascontiguousarray(kw["y"])
    md, pd, op, keep = eng.prepare(mat, par, 5, _Host())
    ll = np.empty(5)
    for P, d in ((96, 1), (2048, 1), (64, 17)):
        md.d = d
        desc = _lib.PfDesc(0, P, -1, 0)
        rc = eng.lib.dlm_pf_batch(eng.h, md, pd, ctypes.byref(desc), None, _Host.ptr(y), 0, op, _Host.ptr(ll), None, None, None, None, None)
        assert rc == -3 and len(eng.lib.dlm_last_error(eng.h)) > 20          # DLM_ERR_UNSUPPORTED, and it says why


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
def _level_problem(T=12, seed=4):
    rng = np.random.default_rng(seed)
    x = np.cumsum(np.sqrt(0.3) * rng.standard_normal(T))
    return np.arange(1.0, T + 1), x + rng.standard_normal(T)


def test_metropolis_dglm_equals_its_calls_composed_by_hand(eng):
    times, y = _level_problem()
    mod = Dglm.poisson(Dlm.polynomial(1))
    y = np.round(np.exp(0.5 * y))
    N, n, seed = 7, 128, 99
    init = DlmParameters(np.eye(1), 0.2 * np.eye(1), np.array([0.3]), 0.5 * np.eye(1))
    proposal = Metropolis.symmetric_proposal(0.5)
    prior = lambda p: -0.5 * np.log(p.w[:, 0, 0]) ** 2 - 0.5 * p.m0[:, 0] ** 2
    states = list(Metropolis.dglm(mod, (times, y), proposal, prior, init, n, eng, 3, seed, n_chains=N))
    # by hand
    rng = np.random.default_rng(seed)
    cur, ll, acc = BatchedParameters.of(init, N), np.full(N, -1e99), np.zeros(N, dtype=np.int64)
    for k in range(3):
        prop = proposal(cur, rng)
        pll = ParticleFilter.likelihood(mod, (times, y), n, prop, eng, seed=seed, iteration=k) + prior(prop)
        take = np.log(rng.uniform(size=N)) < pll - ll
        cur, ll, acc = cur.where(take, prop), np.where(take, pll, ll), acc + take
        for a, b in ((states[k].parameters.v, cur.v), (states[k].parameters.w, cur.w), (states[k].parameters.m0, cur.m0),
                     (states[k].parameters.c0, cur.c0), (states[k].ll, ll), (states[k].accepted, acc)):
            np.testing.assert_array_equal(a, b)
    assert np.all(states[0].accepted == 1) and 0 < states[2].accepted.sum() < 3 * N          # the first proposal is always taken; later ones are not


def _kalman_loglik_level(y, W, V=1.0, m0=0.0, C0=1.0):
    """Local level, the particle filter's grid (no advance before the first observation), vectorised over W."""
    m, C, ll = np.full_like(W, m0), np.full_like(W, C0), np.zeros_like(W)
    for t, yt in enumerate(y):
        if t:
            C = C + W
        q = C + V
        e = yt - m
        ll = ll - 0.5 * np.log(2.0 * np.pi * q) - 0.5 * e * e / q
        m, C = m + C / q * e, C - C * C / q
    return ll


def test_pmmh_leaves_the_exact_posterior_invariant(eng):
    """Gaussian local level, T = 12, P = 64, 4096 chains; only log W moves, under a Gaussian prior.  The chains start from draws of the exact
    posterior (a grid over log W with the Kalman likelihood); particle-marginal Metropolis is exact for ANY P, so after 40 iterations the mean
    and the variance of log W across the chains are the posterior's within 5 standard errors (the variance's from the fourth moment)."""
    times, y = _level_problem()
    N, P, iters, mu0, s0, step = 4096, 64, 40, np.log(0.3), 0.8, 0.6
    grid = np.linspace(mu0 - 8 * s0, mu0 + 8 * s0, 8001)
    logp = _kalman_loglik_level(y, np.exp(grid)) - 0.5 * ((grid - mu0) / s0) ** 2
    pdf = np.exp(logp - logp.max()); pdf /= pdf.sum()
    pm = float((pdf * grid).sum()); pv = float((pdf * (grid - pm) ** 2).sum())
    rng = np.random.default_rng(12)
    h = grid[1] - grid[0]
    start = rng.choice(grid, size=N, p=pdf) + h * (rng.uniform(size=N) - 0.5)
    init = BatchedParameters(np.ones((N, 1, 1)), np.exp(start)[:, None, None], np.zeros((N, 1)), np.ones((N, 1, 1)))

    def proposal(p, r):
        return BatchedParameters(p.v, p.w * np.exp(step * r.standard_normal(p.w.shape)), p.m0, p.c0)
    prior = lambda p: -0.5 * ((np.log(p.w[:, 0, 0]) - mu0) / s0) ** 2
    mod = Dglm.gaussian(Dlm.polynomial(1))
    for st in Metropolis.dglm(mod, (times, y), proposal, prior, init, P, eng, iters, seed=31, evaluate_init=True):
        pass
    lw = np.log(st.parameters.w[:, 0, 0])
    rate = st.accepted.mean() / iters
    m, v = lw.mean(), lw.var(ddof=1)
    se_m = np.sqrt(v / N)
    se_v = np.sqrt((((lw - m) ** 4).mean() - v * v) / N)
    print(f"log W after {iters} iterations: mean {m:.4f} (posterior {pm:.4f}, se {se_m:.4f}), variance {v:.4f} (posterior {pv:.4f}, se {se_v:.4f}), "
          f"acceptance {rate:.2f}")
    assert 0.1 < rate < 0.9 and np.all(st.accepted > 0)
    assert abs(m - pm) <= SIGMAS * se_m and abs(v - pv) <= SIGMAS * se_v
    assert INIT_ITERATION == 0xFFFFFFFF
