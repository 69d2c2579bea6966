"""dlm_storvik_batch on the GPU (StorvikFilter.step / filterTs with online learning of the variances).

The kernel is held to its NumPy restatement (tests/storvik_restatement.py) on the table of tests/storvik_cases.py at the tolerance of
tests/test_pf_gpu.py: the arithmetic is restated operation for operation and in the kernel's orders of summation, so what remains is the last
bits of log, exp, cos, sin, pow and lgamma.  The ESS must be EQUAL, and so must, in effect, the ancestors and every accept decision of the
Gammas: one that went the other way leaves a final cloud that differs in the first digit.  tests/test_storvik_host.py shows that no comparison
of the kernel's is within 1e-11 of flipping on these inputs.  Then: the batch does not depend on how it is split, the evidence estimate is
unbiased on the device too, the bad series, the refusals, and the Python driver.

The largest relative difference seen on an MI355X is in profiles/r20_notes.md."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pf_cases as pc  # noqa: E402
import storvik_cases as sc  # noqa: E402
import storvik_restatement as sr  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dglm import Dglm, StorvikFilter  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters  # noqa: E402
from bayesian_dlms_amd.engine import Engine, EngineError  # noqa: E402
from bayesian_dlms_amd.gibbs import InverseGamma  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-11, 1e-12
KEYS = ("ll", "mean", "ess", "scale_mean", "cloud", "weights", "scales")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _rel(a, b):
    ok = np.isfinite(b)
    return float((np.abs(a[ok] - b[ok]) / (np.abs(b[ok]) + ATOL / RTOL)).max()) if ok.any() else 0.0


# ---- kernel against restatement ---------------------------------------------------------------------------------------------------------
RUNS = [(c["name"], False) for c in sc.TABLE] + [(n, True) for n in sc.DEVICE_RUNS]


@pytest.mark.parametrize("name,device", RUNS, ids=[n + ("-device" if dev else "") for n, dev in RUNS])
def test_kernel_matches_restatement(eng, name, device):
    ref = sc.reference(name)
    out = sc.engine_run(eng, sc.run_args(name), device=device)
    assert eng.last_variant == "storvik-wave"
    np.testing.assert_array_equal(out["status"], ref["status"])
    np.testing.assert_array_equal(out["ess"], ref["ess"])
    print(f"{name}: largest relative difference " + ", ".join(f"{k} {_rel(out[k], ref[k]):.2e}" for k in KEYS))
    for k in KEYS:
        np.testing.assert_allclose(out[k], ref[k], rtol=RTOL, atol=ATOL, err_msg=k)


# ---- the batch does not depend on how it is split ---------------------------------------------------------------------------------------
def _slice(kw, lo, hi):
    """Series lo .. hi - 1 of a batch with per-series m0, C0 and priors, as a batch of its own."""
    cut = dict(kw, y=kw["y"][lo:hi], series_offset=kw["series_offset"] + lo)
    for k in ("m0", "C0", "prior_w", "prior_v"):
        cut[k] = kw[k][lo:hi]
    return cut


def test_halves_with_series_offset_equal_the_whole_batch(eng):
    kw = sc.run_args("n67-per-series")
    whole = sc.engine_run(eng, kw)
    again = sc.engine_run(eng, kw)
    lo, hi = sc.engine_run(eng, _slice(kw, 0, 34)), sc.engine_run(eng, _slice(kw, 34, 67), device=True)
    for k in KEYS + ("status",):
        np.testing.assert_array_equal(whole[k], again[k], err_msg=k)          # the same iteration: the same bits
        np.testing.assert_array_equal(whole[k], np.concatenate([lo[k], hi[k]]), err_msg=k)
    other = sc.engine_run(eng, dict(kw, iteration=kw["iteration"] + 1))
    assert np.all(other["ll"] != whole["ll"])          # another iteration: other draws for every series


# ---- the evidence on the device ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["level", "dense"])
def test_evidence_estimate_is_unbiased_and_literal_is_not(eng, which):
    log_z, _, _ = sc.exact(which)
    out = sc.engine_run(eng, sc.evidence_args(which), device=True)
    m, se, top = sc.unbiasedness(out["ll"], log_z)
    print(f"{which}: mean exp(ll - log Z) = {m:.5f} +- {se:.5f} (largest ratio {top:.1f})")
    assert np.all(out["status"] == 0) and abs(m - 1.0) <= sc.SIGMAS * se
    lit = sc.engine_run(eng, sc.evidence_args(which, literal=True), device=True)
    m, se, top = sc.unbiasedness(lit["ll"], log_z)
    print(f"{which}, literal: mean exp(ll - log Z) = {m:.5f} +- {se:.5f}")
    assert abs(m - 1.0) > sc.SIGMAS * se


# ---- status -------------------------------------------------------------------------------------------------------------------------------
def test_a_failing_series_fails_alone(eng):
    kw = sc.run_args("p128-d2-missing-per-series")
    C0 = kw["C0"].copy(); C0[3] = -C0[3]
    pw = kw["prior_w"].copy(); pw[1, 1, 1] = 0.0          # a prior scale of 0
    good = sc.engine_run(eng, kw)
    out = sc.engine_run(eng, dict(kw, C0=C0, prior_w=pw))
    assert out["status"].tolist() == [0, _lib.ST_NOT_PD, 0, _lib.ST_NOT_PD, 0]
    assert np.all(out["ll"][[1, 3]] == -np.inf)
    for k in ("mean", "ess", "scale_mean", "cloud", "weights", "scales"):
        assert np.all(np.isnan(out[k][[1, 3]])), k
    for k in KEYS:
        np.testing.assert_array_equal(out[k][[0, 2, 4]], good[k][[0, 2, 4]], err_msg=k)
    pv = kw["prior_v"].copy(); pv[0, 0] = np.nan          # a prior shape that is NaN
    out = sc.engine_run(eng, dict(kw, prior_v=pv))
    assert out["status"].tolist() == [_lib.ST_NOT_PD, 0, 0, 0, 0] and out["ll"][0] == -np.inf
    for k in KEYS:
        np.testing.assert_array_equal(out[k][1:], good[k][1:], err_msg=k)


def test_a_beta_series_with_y_outside_the_unit_interval_fails_alone(eng):
    kw = sc.run_args("learnv0-beta")
    y = kw["y"].copy(); y[2, 5] = 1.5
    bad, good = sc.engine_run(eng, dict(kw, y=y)), sc.engine_run(eng, kw)
    assert bad["status"].tolist() == [0, 0, _lib.ST_NONFINITE, 0, 0] and bad["ll"][2] == -np.inf
    assert np.all(np.isfinite(bad["mean"][2, :5])) and np.all(np.isnan(bad["mean"][2, 5:])) and np.all(np.isnan(bad["scale_mean"][2, 5:]))
    for k in KEYS:
        np.testing.assert_array_equal(np.delete(bad[k], 2, axis=0), np.delete(good[k], 2, axis=0), err_msg=k)
    ref = sr.run(**dict(kw, y=y))
    for k in KEYS:
        np.testing.assert_allclose(bad[k], ref[k], rtol=RTOL, atol=ATOL, err_msg=k)


def test_engine_refuses_what_it_does_not_cover(eng):
    from bayesian_dlms_amd.engine import _Host
    kw = sc.run_args("p64-d1")
    mat, par = pc.materialised(kw), pc.packed_params(kw, 5)
    with pytest.raises(EngineError, match="Gaussian"):
        eng.storvik_filter(mat, par, kw["y"], kw["prior_w"], family=_lib.OBS_POISSON, n_particles=64, prior_v=kw["prior_v"], learn_v=True)
    # straight at the C ABI: the code and a message, no launch
    y = np.ascontiguousarray(kw["y"])
    md, pd, op, keep = eng.prepare(mat, par, 5, _Host())
    ll = np.empty(5)
    pw16, pv = np.tile([4.0, 1.0], (16, 1)), np.array([4.0, 1.0])

    def call(desc):
        return eng.lib.dlm_storvik_batch(eng.h, md, pd, ctypes.byref(desc), _Host.ptr(pv), 0, _Host.ptr(pw16), 0, None, _Host.ptr(y), 0, op,
                                         _Host.ptr(ll), None, None, None, None, None, None, None)
    assert call(_lib.StorvikDesc(_lib.OBS_POISSON, 64, -1, 0, 1)) == -1 and b"Gaussian" in eng.lib.dlm_last_error(eng.h)          # DLM_ERR_ARG
    md.d = 16
    assert call(_lib.StorvikDesc(0, 1024, -1, 0, 1)) == -3 and b"LDS" in eng.lib.dlm_last_error(eng.h)          # DLM_ERR_UNSUPPORTED: d = 16, P = 1024
    md.d, md.p = 1, 2
    assert call(_lib.StorvikDesc(0, 64, -1, 0, 1)) == -3 and b"p = 1" in eng.lib.dlm_last_error(eng.h)
    md.p = 1
    for P in (96, 2048):
        assert call(_lib.StorvikDesc(0, P, -1, 0, 1)) == -3
    assert call(_lib.StorvikDesc(0, 64, -1, 0, 1)) == 0 and np.all(np.isfinite(ll))          # and the same call inside the limits runs


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
def test_storvik_filter_equals_the_raw_engine_call(eng):
    rng = np.random.default_rng(8)
    T, N, n = 14, 3, 128
    times = np.concatenate([[1.0, 2.0, 4.0], np.arange(5.0, T + 2.0)])          # one step of 2
    y = np.cumsum(np.sqrt(0.3) * rng.standard_normal((N, T)), axis=1) + rng.standard_normal((N, T))
    y[1, 4] = np.nan
    mod = Dglm.gaussian(Dlm.polynomial(2))
    p = DlmParameters(np.eye(1), np.eye(2), np.array([0.1, 0.0]), np.eye(2))
    prior_v, prior_w = InverseGamma(0.4, 2.0), [InverseGamma(4.0, 0.9), InverseGamma(0.9, 0.1)]
    out = StorvikFilter(n, 40).filter(mod, (times, y), p, prior_v, prior_w, eng, seed=5, iteration=2, series_offset=9)
    from bayesian_dlms_amd.dglm import materialise_pf
    pw = np.array([[4.0, 0.9], [0.9, 0.1]])
    raw = eng.storvik_filter(materialise_pf(mod, times), p, y, pw, family=_lib.OBS_GAUSSIAN, n_particles=n, prior_v=np.array([0.4, 2.0]),
                             learn_v=True, n0=40, iteration=2, seed=5, series_offset=9)
    for k in KEYS + ("status",):
        np.testing.assert_array_equal(out[k], np.asarray(raw[k]), err_msg=k)
    assert eng.last_variant == "storvik-wave" and np.all(out["status"] == 0)
    # the shapes: + 0.5 per advance (dt_0 = 0: none) and per observation; the means are scale_mean / (shape - 1), NaN up to shape 1
    adv = np.arange(T)
    np.testing.assert_array_equal(out["shape_w"], np.broadcast_to(pw[None, None, :, 0] + 0.5 * adv[None, :, None], (N, T, 2)))
    seen = np.cumsum(~np.isnan(y), axis=1)
    np.testing.assert_array_equal(out["shape_v"], 0.4 + 0.5 * seen)
    with np.errstate(invalid="ignore", divide="ignore"):
        wm = np.where(out["shape_w"] > 1.0, out["scale_mean"][:, :, :2] / (out["shape_w"] - 1.0), np.nan)
        vm = np.where(out["shape_v"] > 1.0, out["scale_mean"][:, :, 2] / (out["shape_v"] - 1.0), np.nan)
    np.testing.assert_array_equal(out["w_mean"], wm)
    np.testing.assert_array_equal(out["v_mean"], vm)
    assert np.all(np.isnan(out["w_mean"][:, 0, 1])) and np.all(np.isfinite(out["w_mean"][:, 1:, 1])) and np.all(np.isfinite(out["w_mean"][:, :, 0]))
    assert np.all(np.isnan(out["v_mean"][:, 0])) and np.all(np.isfinite(out["v_mean"][:, 1:]))
    # a family other than the Gaussian learns W alone
    cnt = StorvikFilter(n).filter(Dglm.poisson(Dlm.polynomial(2)), (times, np.round(np.exp(0.3 * y))), p, None, prior_w[0], eng, seed=5)
    assert np.all(cnt["status"] == 0) and np.all(np.isnan(cnt["v_mean"])) and np.all(np.isnan(cnt["scales"][:, 2])) and np.all(np.isfinite(cnt["ll"]))
