"""The Rao-Blackwellised filter without a GPU: the restatement the kernel is held to (tests/rb_restatement.py) against what it must compute --
with known variances the Kalman filter itself (likelihood, filtered means and covariances, ESS = P; and NOT so under `literal`); with a static
parameter cloud the evidence with the variances integrated over their log-normal priors (lw_cases.exact), at a standard error well below the
Liu-West restatement's on the same inputs; with a < 1 the posterior means of the log-variances against the same grid -- and the inputs of the
GPU tests (tests/rb_cases.py) against what makes them worth running: no comparison of the kernel's within a rounding error of flipping, and
both branches of the second stage's resampling test taken.  Then the code objects, the build and the argument checks.

Bounds.  Known variances: rtol 1e-10 (two orders of summation of the same recursion).  Unbiasedness: SIGMAS = 4 standard errors of the
estimate, from its own sample of 4096 replicates.  Margins: those of tests/test_lw_host.py (1e-11 for the two searches and n0, 1e-9 for the
distance of 1 / sum W^2 from an integer, over the steps whose weights are not all exp(0)).  Learning: the larger of 3 standard errors of the
replicate mean and twice the deviation measured on the restatement (tests/rb_cases.py has the figures)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lw_cases as lc  # noqa: E402
import lw_restatement as lr  # noqa: E402
import rb_cases as rc  # noqa: E402
import rb_restatement as rr  # noqa: E402
import storvik_cases as sc  # noqa: E402
from code_object import kernel_resources  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dglm import Dglm, RaoBlackwellFilter  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters  # noqa: E402
from bayesian_dlms_amd.engine import EngineError  # noqa: E402
from bayesian_dlms_amd.stochvol import Gaussian  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN, MARGIN_INT = 1e-11, 1e-9


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in rc.TABLE])
def test_table_entry_has_margins(name):
    r = rc.reference(name)
    print(f"{name}: share {r['resample_share']:.2f}, margins search {r['margin_search']:.2e}, n0 {r['margin_n0']:.2e}, integer {r['margin_int']:.2e}")
    assert np.all(r["status"] == 0) and np.all(np.isfinite(r["ll"]))
    if name in rc.FORCED:          # n0 = P + 1, n0 = 0: one branch by construction
        assert r["resample_share"] == rc.FORCED[name]
    assert r["margin_search"] >= MARGIN and r["margin_n0"] >= MARGIN          # (an entry that fails: change its seed, not the bound)
    assert r["margin_int"] >= MARGIN_INT
    if name in rc.EXACT_ESS:          # variances that do not move: the second stage's log-weights are 0 exactly
        assert np.all(r["ess"] == rc.by_name(name)["P"]) and r["margin_int"] == np.inf


def test_table_reaches_the_second_stage_s_resampling():
    shares = {c["name"]: rc.reference(c["name"])["resample_share"] for c in rc.TABLE}
    print("share of observed steps whose second stage resamples: " + ", ".join(f"{k} {v:.2f}" for k, v in shares.items()))
    inside = [k for k, v in shares.items() if rc.SHARE_LO <= v <= rc.SHARE_HI]
    assert len(inside) >= rc.SHARE_ENTRIES and all(k.startswith("share-") for k in inside)
    assert shares["always"] == 1.0 and shares["never"] == 0.0
    # the default n0 never resamples where the variances do not move
    assert shares["a1-static"] == 0.0 and shares["known-kalman"] == 0.0


def test_table_covers_the_shapes():
    t = rc.TABLE
    assert {(c["d"], c["P"]) for c in t} >= {(1, 64), (2, 128), (3, 128), (16, 64)}
    assert all(6 <= c["T"] <= 24 for c in t) and all(2 <= c["N"] <= 5 or c["N"] == 67 for c in t) and any(c["N"] == 67 and c["per_series"] for c in t)
    assert {c["N"] for c in t} >= {2, 5, 67}
    assert {c["learn_v"] for c in t} == {False, True} and {c["literal"] for c in t} == {False, True} and {c["n0"] for c in t} >= {-1, 0, 129}
    assert {c["a"] for c in t} >= {1.0, 0.95, 0.7} and any(c["sd0"] and c["sd0"] != "all" for c in t) and any(c["sd0"] == "all" for c in t)
    assert any(set(c["missing"]) >= {0, c["T"] - 1} and len(c["missing"]) >= 3 for c in t)
    irr = rc.inputs("p128-d3-irregular")
    assert irr["G"].shape[0] == 3 and (irr["dt"][1:] == 0.0).sum() == 1 and irr["dt"][0] == 0.0 and irr["g_index"] is not None
    per = rc.inputs("n67-per-series")
    assert per["prior_w"].shape == (67, 1, 2) and per["prior_v"].shape == (67, 2) and per["C0"].shape == (67, 1, 1) and per["m0"].shape == (67, 1)
    assert len(rc.DEVICE_RUNS) == 3


def test_lds_admits_the_required_shapes():
    """(d(d+1)/2 + 2 d + 3.5) P + 64 d(d+1)/2 + 3 d + 1 doubles inside 160 KB"""
    lds, have = _lib.rb_lds_bytes, _lib.RB_LDS_BYTES
    for d, P in ((1, 1024), (2, 1024), (3, 1024), (4, 512), (8, 256), (13, 64), (16, 64)):
        assert lds(d, P) <= have, (d, P)
    assert lds(3, 1024) == 130128 and lds(16, 64) == 157832          # the two largest holdings, as the header states them
    assert lds(4, 1024) > have and lds(16, 128) > have
    tri = lambda d: d * (d + 1) // 2
    assert all(lds(d, P) == ((tri(d) + 2 * d + 3) * P + 64 * tri(d) + 3 * d + 1) * 8 + 4 * P for d in (1, 5, 16) for P in (64, 1024))
    src = open(os.path.join(ROOT, "bayesian_dlms_amd", "csrc", "dlm_rb.hip")).read()
    assert "((tri + 2 * (size_t)d + 3) * P + tri * 64 + 3 * (size_t)d + 1) * sizeof(double) + (size_t)P * sizeof(int)" in src


def test_restatement_reports_both_status_bits():
    kw = rc.run_args("p128-d2-missing-per-series")
    good = rc.reference("p128-d2-missing-per-series")
    keys = ("ll", "mean", "cov", "ess", "psi_mean", "psi_var", "means", "covs", "weights", "psi")
    # a prior sd that is negative, a prior mean that is NaN: no step is made
    pw = kw["prior_w"].copy(); pw[1, 1, 1] = -0.25
    pv = kw["prior_v"].copy(); pv[3, 0] = np.nan
    r = rr.run(**dict(kw, prior_w=pw, prior_v=pv))
    assert r["status"].tolist() == [0, rr.ST_NOT_PD, 0, rr.ST_NOT_PD, 0] and np.all(r["ll"][[1, 3]] == -np.inf)
    for k in keys[1:]:
        assert np.all(np.isnan(r[k][[1, 3]])), k
    for k in keys:
        np.testing.assert_array_equal(r[k][[0, 2, 4]], good[k][[0, 2, 4]], err_msg=k)
    # a C0 whose Q is not positive at the first observed step (t = 1: y_0 is missing): the missing step's outputs stand
    C0 = kw["C0"].copy(); C0[2] = -40.0 * C0[2]
    r = rr.run(**dict(kw, C0=C0))
    assert r["status"].tolist() == [0, 0, rr.ST_NOT_PD, 0, 0] and r["ll"][2] == -np.inf
    assert np.all(np.isfinite(r["mean"][2, 0])) and np.all(np.isnan(r["mean"][2, 1:])) and np.all(np.isnan(r["means"][2]))
    # a log-variance whose exp overflows: Q is not finite
    pw = kw["prior_w"].copy(); pw[4, 0, 0] = 800.0
    r = rr.run(**dict(kw, prior_w=pw))
    assert r["status"].tolist() == [0, 0, 0, 0, rr.ST_NONFINITE] and r["ll"][4] == -np.inf and np.all(np.isnan(r["cov"][4, 1:]))
    for k in keys:
        np.testing.assert_array_equal(r[k][:4], good[k][:4], err_msg=k)


def test_a_known_row_stays_where_it_is():
    r, kw = rc.reference("sd0-one-row"), rc.run_args("sd0-one-row")
    assert np.all(r["psi"][:, 1] == kw["prior_w"][1, 0]) and np.all(r["psi"][:, 0].std(axis=1) > 0.0)
    np.testing.assert_allclose(r["psi_var"][:, :, 1], 0.0, atol=1e-28)


# ---- check 1: known variances are the Kalman filter -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", rc.KNOWN_MODELS)
@pytest.mark.parametrize("a", [1.0, 0.9])
def test_known_variances_are_the_kalman_filter(which, a):
    ms, Cs, ll = rc.known_exact(which)
    for seed, P in ((11, 64), (12, 128)):
        r = rr.run(**rc.known_args(which, a=a, P=P, seed=seed))
        assert np.all(r["status"] == 0) and np.all(r["ess"] == P)
        np.testing.assert_allclose(r["ll"], ll, rtol=rc.KNOWN_RTOL)
        for n in range(r["ll"].size):
            np.testing.assert_allclose(r["mean"][n], ms, rtol=rc.KNOWN_RTOL, atol=1e-14)
            np.testing.assert_allclose(r["cov"][n], Cs, rtol=rc.KNOWN_RTOL, atol=1e-14)
    if which == "irregular":          # the oracle's filter shares nothing with the restatement
        om, oC = rc.oracle_filter(which)
        np.testing.assert_allclose(r["mean"][0], om, rtol=rc.KNOWN_RTOL, atol=1e-14)
        np.testing.assert_allclose(r["cov"][0], oC, rtol=rc.KNOWN_RTOL, atol=1e-14)
    # `literal` looks ahead with the observation variance alone and does not divide by it: not the Kalman likelihood
    lit = rr.run(**rc.known_args(which, a=a, literal=True))
    print(f"{which}, a = {a}, literal: ll - Kalman = {lit['ll'][0] - ll:+.4f}, largest |mean - Kalman| = {np.abs(lit['mean'][0] - ms).max():.3e}")
    assert abs(lit["ll"][0] - ll) > 1e-3 * abs(ll)


# ---- checks 2 and 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(run, fn, *args, **over):
        key = (run.__module__, args, tuple(sorted(over.items())))
        if key not in cache:
            cache[key] = run(**fn(*args, **over))
        return cache[key]
    return get


@pytest.mark.parametrize("which", ["level", "dense"])
def test_static_cloud_the_evidence_estimate_is_unbiased_and_tighter_than_liu_west(runs, which):
    log_z, _, _ = lc.exact(which, lc.STATIC_SD, lc.STATIC_T)
    r = runs(rr.run, rc.learn_args, which, lc.STATIC_SD, lc.STATIC_T, lc.REPLICATES)
    m, se, top = sc.unbiasedness(r["ll"], log_z)
    share = top / np.exp(r["ll"] - log_z).sum()
    lw = runs(lr.run, lc.learn_args, which, lc.STATIC_SD, lc.STATIC_T, lc.REPLICATES)
    _, se_lw, _ = sc.unbiasedness(lw["ll"], log_z)
    print(f"{which}, a = 1, sd {lc.STATIC_SD}, T {lc.STATIC_T}: mean exp(ll - log Z) = {m:.5f} +- {se:.5f}, largest ratio {share:.5f} of the sum; "
          f"Liu-West's standard error {se_lw:.5f}, {se_lw / se:.2f} times this one")
    assert np.all(r["status"] == 0) and np.all(r["ess"] == lc.learn_args(which, lc.STATIC_SD, lc.STATIC_T, 1)["P"])
    assert abs(m - 1.0) <= rc.SIGMAS * se
    assert share < rc.TOP_SHARE
    assert se <= se_lw / rc.SE_FACTOR


@pytest.mark.parametrize("which", ["level", "dense"])
def test_learning_the_posterior_means_of_the_log_variances(runs, which):
    _, grid, _ = lc.exact(which, lc.LEARN_SD, lc.LEARN_T)
    over = dict(a=lc.LEARN_A, P=lc.LEARN_P)
    fm = lc.final_log_means(runs(rr.run, rc.learn_args, which, lc.LEARN_SD, lc.LEARN_T, lc.LEARN_REPLICATES, **over), which)
    mean, se = fm.mean(axis=0), fm.std(axis=0, ddof=1) / np.sqrt(fm.shape[0])
    dev, bound = np.abs(mean - np.asarray(grid)), rc.learn_bound(which, se)
    print(f"{which}, a = {lc.LEARN_A}, P = {lc.LEARN_P}, {lc.LEARN_REPLICATES} replicates: means {mean} against the grid's {grid}: deviation {dev}, "
          f"standard errors {se}, bound {bound}")
    assert np.all(dev <= bound)
    # what this test measures is what rb_cases.LEARN_MEASURED records (the bound of the device test)
    np.testing.assert_allclose(dev, rc.LEARN_MEASURED[which], atol=5e-5)
    lit = lc.final_log_means(runs(rr.run, rc.learn_args, which, lc.LEARN_SD, lc.LEARN_T, lc.LEARN_REPLICATES, literal=True, **over), which)
    print(f"literal (reported, not asserted): deviation {np.abs(lit.mean(axis=0) - np.asarray(grid))}")


# ---- the code objects -----------------------------------------------------------------------------------------------------------------
def test_kernel_has_no_scratch_and_no_spills():
    """dlm_rb.o: every instantiation of k_rb keeps everything in registers"""
    counts = []
    for d in range(1, 17):
        scratch, spills, vgprs = kernel_resources("dlm_rb.o", f"k_rbILi{d}E")
        counts.append(vgprs)
        assert (scratch, spills) == (0, 0), (d, scratch, spills)
    print("k_rb registers (VGPRs + AGPRs), d = 1 .. 16:", counts)
    assert all(c <= 512 for c in counts) and all(c <= 256 for c in counts[:8])          # __launch_bounds__(64, 2) up to d = 8


# ---- build and API --------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_call_with_the_header_s_signature():
    lib = _lib.load()
    assert hasattr(lib, "dlm_rb_batch")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dlm_engine.h")).read(), flags=re.S)
    decl = re.search(r"int dlm_rb_batch\(([^;]*)\);", hdr).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    name, res, args = next(s for s in _lib.SYMBOLS if s[0] == "dlm_rb_batch")
    assert res is ctypes.c_int and len(args) == len(params) == 22
    for p, a in zip(params, args):
        if "uint64_t" in p and "*" not in p:
            assert a is ctypes.c_uint64, p
        elif "int64_t" in p and "*" not in p:
            assert a is ctypes.c_int64, p
        else:
            assert "*" in p and a in (ctypes.c_void_p, _lib._MP, _lib._PP, _lib._OP, ctypes.POINTER(_lib.RbDesc)), p
    fields = re.search(r"typedef struct \{([^}]*)\} dlm_rb_desc;", hdr).group(1)
    assert re.findall(r"(?:int32_t|double) (\w+);", fields) == [f for f, _ in _lib.RbDesc._fields_]
    assert [t for _, t in _lib.RbDesc._fields_] == [ctypes.c_int32] * 4 + [ctypes.c_double] and ctypes.sizeof(_lib.RbDesc) == 24
    src = open(os.path.join(ROOT, "bayesian_dlms_amd", "csrc", "dlm_draws.h")).read()
    assert f"DLM_KEY_RB = 0x{rr.KEY_RB:08X}u" in src
    assert (f"DLM_RB_BLOCK_RESAMPLE = {rr.BLOCK_RESAMPLE}u, DLM_RB_BLOCK_FIRST = {rr.BLOCK_FIRST}u, DLM_RB_BLOCK_PARAM = {rr.BLOCK_PARAM}u") in src
    assert "DLM_RB_SLOT_INIT = DLM_SLOT_TOP" in src and rr.SLOT_INIT == 0x1FFFFF
    # every stream's key is its own, and no other shares the upper half of the key word with this one
    keys = [int(k, 16) for k in re.findall(r"constexpr unsigned DLM_KEY_\w+ = (0x[0-9A-Fa-f]{8})u", src)]
    assert len(keys) >= 10 and len(set(keys)) == len(keys) and sum((k >> 16) == (rr.KEY_RB >> 16) for k in keys) == 1
    # the glue declares it
    assert "dlm_rb_batch(" in open(os.path.join(ROOT, "integration", "jni", "dlm_jni.cpp")).read()
    assert "@native def rbFilter(" in open(os.path.join(ROOT, "integration", "scala", "Batched.scala")).read()
    # both libraries are linked from the new translation unit
    from bayesian_dlms_amd import build
    assert "dlm_rb.hip" in build.SOURCES and "dlm_rb.hip" not in build.DRAIN_SOURCES


def test_a_null_engine_or_descriptor_is_an_argument_error():
    lib = _lib.load()
    assert lib.dlm_rb_batch(None, None, None, None, None, 0, None, 0, None, 0, None, *([None] * 11)) == -1


def _series(T=6, p=1):
    return np.arange(1.0, T + 1), np.zeros((T, p))[None] if p > 1 else np.zeros(T)


@pytest.mark.parametrize("n", [96, 2048, 0, 32])
def test_python_layer_refuses_particle_counts(n):
    with pytest.raises(EngineError, match="multiple of 64 between 64 and 1024"):
        RaoBlackwellFilter(n, 0.95)


@pytest.mark.parametrize("a", [0.0, -0.5, 1.0001, float("nan")])
def test_python_layer_refuses_a_shrinkage_outside_the_unit_interval(a):
    with pytest.raises(ValueError, match="0 < a <= 1"):
        RaoBlackwellFilter(128, a)


def test_python_layer_refuses_what_the_engine_does_not_cover():
    from bayesian_dlms_amd.engine import Engine
    par = lambda d, p: DlmParameters(np.eye(p), np.eye(d), np.zeros(d), np.eye(d))
    g = Gaussian(0.0, 0.5)
    with pytest.raises(EngineError, match="d <= 16, got d = 17"):
        RaoBlackwellFilter(64, 0.95).filter(Dlm.polynomial(17), _series(), par(17, 1), g, g, None)
    two = Dlm.polynomial(1) * Dlm.polynomial(1)
    with pytest.raises(EngineError, match=r"univariate observation \(p = 1"):
        RaoBlackwellFilter(128, 0.95).filter(Dglm.gaussian(two), _series(p=2), par(2, 2), g, g, None)
    with pytest.raises(EngineError, match="one Gaussian or d = 2 of them"):
        RaoBlackwellFilter(128, 0.95).filter(Dlm.polynomial(2), _series(), par(2, 1), g, [g, g, g], None)
    with pytest.raises(EngineError, match="takes a Gaussian DLM"):
        RaoBlackwellFilter(128, 0.95).filter(Dglm.poisson(Dlm.polynomial(1)), _series(), par(1, 1), g, g, None)
    with pytest.raises(EngineError, match="takes a Gaussian DLM"):
        RaoBlackwellFilter(128, 0.95).filter(Dglm.student_t(5.0, Dlm.polynomial(1)), _series(), par(1, 1), g, g, None)
    # (d, P) beyond the LDS: every particle carries a covariance
    with pytest.raises(EngineError, match="covariance in LDS: d = 4 with 1024 particles"):
        RaoBlackwellFilter(1024, 0.95).filter(Dlm.polynomial(4), _series(), par(4, 1), g, g, None)
    with pytest.raises(EngineError, match="covariance in LDS: d = 16 with 128 particles"):
        RaoBlackwellFilter(128, 0.95).filter(Dglm.gaussian(Dlm.polynomial(16)), _series(), par(16, 1), g, g, None)
    # the checks of Engine.rb_filter that come before anything touches the device
    eng = Engine.__new__(Engine)
    from bayesian_dlms_amd.dglm import materialise_pf
    mat = materialise_pf(Dlm.polynomial(1), np.arange(1.0, 7.0))
    y = np.zeros((1, 6))
    with pytest.raises(EngineError, match="learn_v needs prior_v"):
        Engine.rb_filter(eng, mat, par(1, 1), y, [[0.0, 1.0]], n_particles=64, a=0.9)
    with pytest.raises(EngineError, match=r"prior_w must be \[d\]\[2\]"):
        Engine.rb_filter(eng, mat, par(1, 1), y, [0.0, 1.0, 2.0], n_particles=64, a=0.9, learn_v=False)
    with pytest.raises(EngineError, match="0 < a <= 1"):
        Engine.rb_filter(eng, mat, par(1, 1), y, [[0.0, 1.0]], n_particles=64, a=0.0, learn_v=False)
    mat9 = materialise_pf(Dlm.polynomial(9), np.arange(1.0, 7.0))
    with pytest.raises(EngineError, match="covariance in LDS"):
        Engine.rb_filter(eng, mat9, par(9, 1), y, np.zeros((9, 2)), n_particles=320, a=0.9, learn_v=False)
