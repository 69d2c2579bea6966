"""dlm_pf_resampled on the GPU: the bootstrap particle filter with its resampling scheme chosen.

The kernel is held to its NumPy restatement (tests/pf_resample_restatement.py) on the table of tests/pf_resample_cases.py under every
scheme at the draw-for-draw tolerance of tests/test_pf_gpu.py: ESS and status EQUAL, and so in effect the ancestors -- another particle
picked anywhere leaves a cloud that differs in the first digit.  tests/test_pf_resample_host.py shows that no search, no ESS test and no
Metropolis decision on these inputs is within 1e-11 of flipping.  Then: multinomial through the new export is dlm_pf_batch bit for bit;
the offspring counts of systematic and stratified resampling, recovered from the kernel's own outputs, obey their bounds; the likelihood
estimate stays unbiased for the exact grid likelihood under both; the batch does not depend on how it is split; particle-marginal Metropolis
leaves the exact posterior invariant under systematic resampling; and the engine refuses what the header says it refuses."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pf_cases as pc  # noqa: E402
import pf_grid_reference as gr  # noqa: E402
import pf_resample_cases as rc  # noqa: E402
import pf_resample_restatement as rr  # noqa: E402
import test_pf_gpu as base  # noqa: E402  (the PMMH problem and its exact posterior)

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dglm import BatchedParameters, Dglm, Metropolis, Resampling  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm  # noqa: E402
from bayesian_dlms_amd.engine import Engine, EngineError, _Host  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-11, 1e-12
SIGMAS = 5.0
KEYS = ("ll", "mean", "ess", "cloud", "weights")
ERR_ARG = -1


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _rel(a, b):
    ok = np.isfinite(b)
    return float((np.abs(a[ok] - b[ok]) / (np.abs(b[ok]) + ATOL / RTOL)).max()) if ok.any() else 0.0


# ---- 7: kernel against restatement ----------------------------------------------------------------------------------------------------------
RUNS = [r + (False,) for r in rc.RUNS] + [r + (True,) for r in rc.DEVICE_RUNS]


@pytest.mark.parametrize("name,scheme,b,device", RUNS, ids=[rc.run_id(*r[:3]) + ("-device" if r[3] else "") for r in RUNS])
def test_kernel_matches_restatement(eng, name, scheme, b, device):
    ref = rc.reference(name, scheme, b)
    out = rc.engine_run(eng, rc.run_args(name, scheme, b), device=device)
    assert eng.last_variant == "pf-wave"
    print(f"{rc.run_id(name, scheme, b)}: largest relative difference " + ", ".join(f"{k} {_rel(out[k], ref[k]):.2e}" for k in KEYS))
    np.testing.assert_array_equal(out["status"], ref["status"])
    np.testing.assert_array_equal(out["ess"], ref["ess"])
    for k in KEYS:
        np.testing.assert_allclose(out[k], ref[k], rtol=RTOL, atol=ATOL, err_msg=k)


# ---- 8, 13: the C ABI itself ----------------------------------------------------------------------------------------------------------------
def _abi_call(eng, kw, resample):
    """One call straight at the C ABI on host arrays: dlm_pf_batch (resample None) or dlm_pf_resampled with the dlm_resample_desc
    `resample` (a _lib.ResampleDesc, or "null") -> (the return code, the outputs)."""
    y = np.ascontiguousarray(kw["y"])
    N, T = y.shape
    mat = pc.materialised(kw)
    d, P = mat.d, kw["P"]
    md, pd, op, keep = eng.prepare(mat, pc.packed_params(kw, N), N, _Host(), 0, kw["seed"], kw["series_offset"])
    out = dict(ll=np.full(N, np.nan), mean=np.full((N, T, d), np.nan), ess=np.full((N, T), np.nan), cloud=np.full((N, d, P), np.nan),
               weights=np.full((N, P), np.nan), status=np.full(N, -7, dtype=np.int32))
    desc = _lib.PfDesc(kw["family"], P, kw["n0"], 1 if kw["literal"] else 0)
    tail = (None, _Host.ptr(y), kw["iteration"], op) + tuple(_Host.ptr(a) for a in out.values())
    if resample is None:
        code = eng.lib.dlm_pf_batch(eng.h, md, pd, ctypes.byref(desc), *tail)
    else:
        code = eng.lib.dlm_pf_resampled(eng.h, md, pd, ctypes.byref(desc), None if resample == "null" else ctypes.byref(resample), *tail)
    return code, out


def test_multinomial_through_the_new_export_is_dlm_pf_batch_bit_for_bit(eng):
    kw = pc.run_args("p192-d3-irregular")
    code_old, old = _abi_call(eng, kw, None)
    code_new, new = _abi_call(eng, kw, _lib.ResampleDesc(_lib.RESAMPLE_MULTINOMIAL, 0))
    assert code_old == 0 and code_new == 0 and np.all(np.isfinite(old["ll"])) and np.all(old["status"] == 0)
    for k in KEYS + ("status",):
        np.testing.assert_array_equal(new[k], old[k], err_msg=k)
    via = pc.engine_run(eng, kw)          # the binding, which takes the multinomial scheme to dlm_pf_batch
    for k in KEYS + ("status",):
        np.testing.assert_array_equal(via[k], old[k], err_msg=k)
    other = _abi_call(eng, kw, _lib.ResampleDesc(_lib.RESAMPLE_SYSTEMATIC, 0))[1]
    assert np.all(other["ll"] != old["ll"])          # (the descriptor is read: another scheme, another estimate)


def test_engine_refuses_a_bad_resampling_descriptor(eng):
    kw = pc.run_args("p64-d1")
    good = _abi_call(eng, kw, _lib.ResampleDesc(_lib.RESAMPLE_SYSTEMATIC, 0))
    assert good[0] == 0
    bad = ["null", _lib.ResampleDesc(4, 0), _lib.ResampleDesc(-1, 0), _lib.ResampleDesc(_lib.RESAMPLE_METROPOLIS, 0),
           _lib.ResampleDesc(_lib.RESAMPLE_METROPOLIS, 65), _lib.ResampleDesc(_lib.RESAMPLE_METROPOLIS, -1),
           _lib.ResampleDesc(_lib.RESAMPLE_MULTINOMIAL, 10), _lib.ResampleDesc(_lib.RESAMPLE_STRATIFIED, 1),
           _lib.ResampleDesc(_lib.RESAMPLE_SYSTEMATIC, 64)]
    for desc in bad:
        code, out = _abi_call(eng, kw, desc)
        assert code == ERR_ARG and len(eng.lib.dlm_last_error(eng.h)) > 10, (desc if desc == "null" else (desc.scheme, desc.mh_steps))
        assert np.all(np.isnan(out["ll"])) and np.all(out["status"] == -7)          # nothing was launched, nothing written
    again = _abi_call(eng, kw, _lib.ResampleDesc(_lib.RESAMPLE_SYSTEMATIC, 0))          # the batch after the refusals runs clean
    assert again[0] == 0 and np.all(again[1]["status"] == 0)
    for k in KEYS:
        np.testing.assert_array_equal(again[1][k], good[1][k], err_msg=k)
    code, _ = _abi_call(eng, kw, _lib.ResampleDesc(_lib.RESAMPLE_METROPOLIS, 64))
    assert code == 0
    mat, par = pc.materialised(kw), pc.packed_params(kw, 5)
    for over in (dict(resample=4), dict(resample=_lib.RESAMPLE_METROPOLIS), dict(resample=_lib.RESAMPLE_METROPOLIS, mh_steps=65), dict(mh_steps=3)):
        with pytest.raises(EngineError, match="RESAMPLE_|mh_steps"):
            eng.particle_filter(mat, par, kw["y"], family=0, n_particles=64, **over)


# ---- 9: offspring counts from the kernel's own outputs --------------------------------------------------------------------------------------
def _one_step(P, N=67):
    """d = 1, T = 1: the initial cloud is weighed once (dt_0 = 0) and, with n0 = P + 1, resampled once"""
    rng = np.random.default_rng(300 + P)
    return dict(F=np.array([1.0]), G=np.array([[[0.9]]]), g_index=None, dt=np.array([0.0]), V=0.15, W=np.array([[0.15]]), m0=np.array([0.2]),
                C0=np.array([[0.6]]), y=0.2 + 0.9 * rng.standard_normal((N, 1)), nu=None, family=0, P=P, literal=False, seed=61, series_offset=9,
                iteration=2)


@pytest.mark.parametrize("scheme", [rr.SYSTEMATIC, rr.STRATIFIED], ids=["systematic", "stratified"])
@pytest.mark.parametrize("P", [64, 128])
def test_offspring_counts_of_the_kernel(eng, P, scheme):
    kw = _one_step(P)
    before = rc.engine_run(eng, dict(kw, n0=0, resample=scheme, mh_steps=0))          # never resamples: the cloud and its weights
    after = rc.engine_run(eng, dict(kw, n0=P + 1, resample=scheme, mh_steps=0))
    assert np.all(before["status"] == 0) and np.all(after["status"] == 0)
    np.testing.assert_array_equal(after["ll"], before["ll"])
    np.testing.assert_array_equal(after["weights"], np.full((67, P), 1.0 / P))
    xb, xa, w = before["cloud"][:, 0], after["cloud"][:, 0], before["weights"]
    order = np.argsort(xb, axis=1)
    srt = np.take_along_axis(xb, order, axis=1)
    assert np.all(np.diff(srt, axis=1) > 0.0)          # the values before are distinct: a value names its particle
    pos = np.stack([np.searchsorted(srt[n], xa[n]) for n in range(67)])
    assert np.all(pos < P) and np.all(np.take_along_axis(srt, np.minimum(pos, P - 1), axis=1) == xa)          # every particle after IS one from before
    anc = np.take_along_axis(order, pos, axis=1)
    assert (P * w).max() > 3.0 and ((P * w) < 0.5).mean() > 0.1          # uneven weights: the bounds say something
    rc.hold_offspring(scheme, anc, w)
    multinomial = rc.engine_run(eng, dict(kw, n0=P + 1, resample=rr.MULTINOMIAL, mh_steps=0))["cloud"][:, 0]
    assert np.any(np.diff(np.take_along_axis(order, np.stack([np.searchsorted(srt[n], multinomial[n]) for n in range(67)]), axis=1), axis=1) < 0)


# ---- 10: unbiased for the exact grid likelihood on the device -------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [rr.STRATIFIED, rr.SYSTEMATIC], ids=["stratified", "systematic"])
@pytest.mark.parametrize("name", gr.NAMES)
def test_likelihood_estimate_stays_unbiased_on_the_device(eng, name, scheme):
    out = rc.engine_run(eng, dict(gr.args_of("pf", name), resample=scheme, mh_steps=0), device=True)
    gr.hold_likelihood("pf", name, out)


# ---- 11: the batch does not depend on how it is split ---------------------------------------------------------------------------------------
def _slice(kw, lo, hi):
    """Series lo .. hi - 1 of a batch with per-series parameters, as a batch of its own."""
    cut = dict(kw, y=kw["y"][lo:hi], series_offset=kw["series_offset"] + lo)
    for k in ("V", "W", "m0", "C0"):
        cut[k] = kw[k][lo:hi]
    return cut


@pytest.mark.parametrize("scheme,b", [(rr.SYSTEMATIC, 0), (rr.METROPOLIS, 10)], ids=["systematic", "metropolis10"])
def test_parts_with_series_offset_equal_the_whole_batch(eng, scheme, b):
    kw = dict(pc.run_args("n67-per-series"), resample=scheme, mh_steps=b)
    whole = rc.engine_run(eng, kw)
    lo, hi = rc.engine_run(eng, _slice(kw, 0, 20)), rc.engine_run(eng, _slice(kw, 20, 67), device=True)
    assert np.all(whole["status"] == 0) and (whole["ess"] < 64 // 5).any()          # it did resample
    for k in KEYS + ("status",):
        np.testing.assert_array_equal(whole[k], np.concatenate([lo[k], hi[k]]), err_msg=k)


# ---- 12: particle-marginal Metropolis under systematic resampling ---------------------------------------------------------------------------
def test_pmmh_leaves_the_exact_posterior_invariant_under_systematic_resampling(eng):
    """tests/test_pf_gpu.py's check, its sizes and its bound: Gaussian local level, T = 12, P = 64, 4096 chains started from draws of the
    exact posterior of log W; after 40 iterations its mean and variance across the chains are the posterior's within 5 standard errors."""
    times, y = base._level_problem()
    N, P, iters, mu0, s0, step = 4096, 64, 40, np.log(0.3), 0.8, 0.6
    grid = np.linspace(mu0 - 8 * s0, mu0 + 8 * s0, 8001)
    logp = base._kalman_loglik_level(y, np.exp(grid)) - 0.5 * ((grid - mu0) / s0) ** 2
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
    for st in Metropolis.dglm(mod, (times, y), proposal, prior, init, P, eng, iters, seed=31, evaluate_init=True, resample=Resampling.systematic):
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
    with pytest.raises(EngineError, match="wrong posterior"):
        Metropolis.dglm(mod, (times, y), proposal, prior, init, P, eng, iters, seed=31, resample=Resampling.metropolis(10))
