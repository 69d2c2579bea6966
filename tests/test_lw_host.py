"""The Liu-West filter without a GPU: the restatement the kernel is held to (tests/lw_restatement.py) against what it must compute -- with
known parameters the Kalman likelihood (unbiased; and NOT unbiased under `literal`, which drops the division by the first-stage density);
with a static parameter cloud the evidence with the variances integrated over their log-normal priors (a grid integral of the Kalman
likelihood); with a < 1 the posterior means of the log-variances against the same grid -- and the inputs of the GPU tests
(tests/lw_cases.py) against what makes them worth running: no comparison of the kernel's within a rounding error of flipping, and both
branches of the second stage's resampling test taken over the table.  Then the code objects, the build and the argument checks.

Bounds.  Unbiasedness: SIGMAS = 4 standard errors of the estimate, from its own sample of 4096 replicates.  Margins: those of
tests/test_pf_host.py (1e-11 for the two searches and n0, 1e-9 for the distance of 1 / sum W^2 from an integer).  Learning: the larger of 3
standard errors of the replicate mean and twice the deviation measured on the restatement (tests/lw_cases.py has the figures)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lw_cases as lc  # noqa: E402
import lw_restatement as lr  # noqa: E402
import pf_cases as pc  # noqa: E402
import storvik_cases as sc  # noqa: E402
from code_object import kernel_resources  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dglm import AuxFilter, Dglm, LiuAndWestFilter  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters  # noqa: E402
from bayesian_dlms_amd.engine import EngineError  # noqa: E402
from bayesian_dlms_amd.stochvol import Gaussian  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN, MARGIN_INT = 1e-11, 1e-9


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in lc.TABLE])
def test_table_entry_has_margins(name):
    r = lc.reference(name)
    print(f"{name}: share {r['resample_share']:.2f}, margins search {r['margin_search']:.2e}, n0 {r['margin_n0']:.2e}, integer {r['margin_int']:.2e}")
    assert np.all(r["status"] == 0) and np.all(np.isfinite(r["ll"]))
    if name in lc.FORCED:          # n0 = P + 1, n0 = 0: one branch by construction
        assert r["resample_share"] == lc.FORCED[name]
    assert r["margin_search"] >= MARGIN and r["margin_n0"] >= MARGIN          # (an entry that fails: change its seed, not the bound)
    assert r["margin_int"] >= MARGIN_INT


def test_table_takes_both_branches_of_the_second_stage():
    shares = {c["name"]: lc.reference(c["name"])["resample_share"] for c in lc.TABLE if c["name"] not in lc.FORCED}
    steps = {c["name"]: c["N"] * (c["T"] - len(c["missing"])) for c in lc.TABLE}
    total = sum(shares[k] * steps[k] for k in shares) / sum(steps[k] for k in shares)
    print(f"share of steps whose second stage resamples, over the table without the two forcing entries: {total:.1%}; "
          f"per entry {min(shares.values()):.0%} .. {max(shares.values()):.0%}; entries with both branches: "
          f"{sum(0.0 < s < 1.0 for s in shares.values())} of {len(shares)}")
    assert 0.0 < total < 1.0


def test_table_covers_the_shapes():
    t = lc.TABLE
    assert {(c["d"], c["P"]) for c in t} >= {(1, 64), (2, 128), (3, 128), (16, 64)}
    assert all(6 <= c["T"] <= 24 for c in t) and all(2 <= c["N"] <= 5 or c["N"] == 67 for c in t) and any(c["N"] == 67 and c["per_series"] for c in t)
    assert {c["family"] for c in t if not c["learn_v"]} == set(range(6)) and {c["family"] for c in t if c["learn_v"]} == set(lc.SCALE_FAMILIES)
    assert {c["literal"] for c in t} == {False, True} and {c["n0"] for c in t} >= {-1, 0, 129}
    assert 1.0 in {c["a"] for c in t} and min(c["a"] for c in t) <= 0.7 and any(c["sd0"] for c in t)
    assert any(set(c["missing"]) >= {0, c["T"] - 1} and len(c["missing"]) >= 3 for c in t)
    irr = lc.inputs("p128-d3-irregular")
    assert irr["G"].shape[0] == 3 and (irr["dt"][1:] == 0.0).sum() == 1 and irr["g_index"] is not None and len(set(irr["dt"])) == 4
    per = lc.inputs("n67-per-series")
    assert per["prior_w"].shape == (67, 1, 2) and per["prior_v"].shape == (67, 2) and per["C0"].shape == (67, 1, 1) and per["m0"].shape == (67, 1)
    assert len(lc.DEVICE_RUNS) == 3
    # the two largest holdings fit the 160 KB of a workgroup, the next ones do not: (2 d + 3.5) P + d^2 + d + 1 doubles
    lds = lambda d, P: ((2 * d + 3) * P + d * d + d + 1) * 8 + 4 * P
    assert lds(16, 512) <= 160 * 1024 and lds(8, 1024) <= 160 * 1024 and lds(16, 576) > 160 * 1024 and lds(9, 1024) > 160 * 1024


def test_restatement_reports_failures():
    kw = lc.run_args("learnv0-beta")
    y = kw["y"].copy(); y[1, 5] = 1.5
    r = lr.run(**dict(kw, y=y))
    assert r["status"].tolist() == [0, lr.ST_NONFINITE, 0] and r["ll"][1] == -np.inf
    assert np.all(np.isfinite(r["psi_mean"][1, :5, :2])) and np.all(np.isnan(r["psi_mean"][1, 5:])) and np.all(np.isnan(r["psi"][1]))
    good = lc.reference("learnv0-beta")
    for k in ("ll", "mean", "ess", "psi_mean", "psi_var", "cloud", "weights", "psi"):
        np.testing.assert_array_equal(np.delete(r[k], 1, axis=0), np.delete(good[k], 1, axis=0))
    for bad in (-0.1, np.nan):
        pw = kw["prior_w"].copy(); pw[1, 1] = bad
        r = lr.run(**dict(kw, prior_w=pw))
        assert np.all(r["status"] == lr.ST_NOT_PD) and np.all(r["ll"] == -np.inf)
    pw = kw["prior_w"].copy(); pw[0, 0] = np.inf
    assert np.all(lr.run(**dict(kw, prior_w=pw))["status"] == lr.ST_NOT_PD)


def test_a_known_row_stays_where_it_is():
    r, kw = lc.reference("sd0-one-row"), lc.run_args("sd0-one-row")
    assert np.all(r["psi"][:, 1] == kw["prior_w"][1, 0]) and np.all(r["psi"][:, 0].std(axis=1) > 0.0)
    np.testing.assert_allclose(r["psi_var"][:, :, 1], 0.0, atol=1e-28)


# ---- check 1: known parameters ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(fn, *args, **over):
        key = (fn.__name__, args, tuple(sorted(over.items())))
        if key not in cache:
            cache[key] = lr.run(**fn(*args, **over))
        return cache[key]
    return get


@pytest.mark.parametrize("which", ["level", "dense"])
@pytest.mark.parametrize("diffuse", [False, True], ids=["v1", "v500"])
def test_known_parameters_the_likelihood_estimate_is_unbiased_and_literal_is_not(runs, which, diffuse):
    ll = lc.known_exact(which, diffuse)
    r = runs(lc.known_args, which, diffuse)
    m, se = pc.unbiasedness(r["ll"], ll)
    print(f"{which}, V = {500 if diffuse else 1}: mean exp(ll - log L) = {m:.5f} +- {se:.5f}")
    assert np.all(r["status"] == 0) and abs(m - 1.0) <= lc.SIGMAS * se
    lit = runs(lc.known_args, which, diffuse, literal=True)          # Q51: the division by lambda left out
    ml, sel = pc.unbiasedness(lit["ll"], ll)
    print(f"{which}, V = {500 if diffuse else 1}, literal: mean exp(ll - log L) = {ml:.3e} +- {sel:.3e}")
    assert abs(ml - 1.0) > lc.SIGMAS * sel


# ---- check 2: a static parameter cloud ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["level", "dense"])
def test_grid_integral_has_converged(which):
    for sd, T in ((lc.STATIC_SD, lc.STATIC_T), (lc.LEARN_SD, lc.LEARN_T)):
        log_z, means, edge = lc.exact(which, sd, T)
        fine, fine_means, _ = lc.exact(which, sd, T, 2 * sc.GRID - 1)
        print(f"{which}, sd {sd}, T {T}: log Z = {log_z:.10f} (half the spacing: {fine - log_z:+.1e}), posterior means of the logs {means}, edge {edge:.1e}")
        assert abs(fine - log_z) < 1e-9 and edge < 1e-20
        np.testing.assert_allclose(means, fine_means, rtol=1e-9)


@pytest.mark.parametrize("which", ["level", "dense"])
def test_static_cloud_the_evidence_estimate_is_unbiased(runs, which):
    log_z, _, _ = lc.exact(which, lc.STATIC_SD, lc.STATIC_T)
    r = runs(lc.learn_args, which, lc.STATIC_SD, lc.STATIC_T, lc.REPLICATES)
    m, se, top = sc.unbiasedness(r["ll"], log_z)
    print(f"{which}, a = 1, sd {lc.STATIC_SD}, T {lc.STATIC_T}: mean exp(ll - log Z) = {m:.5f} +- {se:.5f} (largest ratio {top:.1f})")
    assert np.all(r["status"] == 0) and se <= lc.STATIC_SE_MAX and abs(m - 1.0) <= lc.SIGMAS * se


# ---- check 3: learning ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["level", "dense"])
def test_learning_the_posterior_means_of_the_log_variances(runs, which):
    _, grid, _ = lc.exact(which, lc.LEARN_SD, lc.LEARN_T)
    over = dict(a=lc.LEARN_A, P=lc.LEARN_P)
    fm = lc.final_log_means(runs(lc.learn_args, which, lc.LEARN_SD, lc.LEARN_T, lc.LEARN_REPLICATES, **over), which)
    mean, se = fm.mean(axis=0), fm.std(axis=0, ddof=1) / np.sqrt(fm.shape[0])
    dev, bound = np.abs(mean - np.asarray(grid)), lc.learn_bound(which, se)
    print(f"{which}, a = {lc.LEARN_A}, P = {lc.LEARN_P}, {lc.LEARN_REPLICATES} replicates: means {mean} against the grid's {grid}: deviation {dev}, "
          f"standard errors {se}, bound {bound}")
    assert np.all(dev <= bound)
    # what this test measures is what lw_cases.LEARN_MEASURED records (the bound of the device test)
    np.testing.assert_allclose(dev, lc.LEARN_MEASURED[which], atol=5e-5)
    lit = lc.final_log_means(runs(lc.learn_args, which, lc.LEARN_SD, lc.LEARN_T, lc.LEARN_REPLICATES, literal=True, **over), which)
    print(f"literal (reported, not asserted): deviation {np.abs(lit.mean(axis=0) - np.asarray(grid))}")


# ---- the code objects -----------------------------------------------------------------------------------------------------------------
# VGPRs of k_pf and k_storvik at d = 1 .. 16 before dlm_lw.hip existed (profiles/r20_notes.md): the new kernel and its key change neither
PF_VGPRS = [156, 157, 153, 159, 171, 176, 190, 193, 204, 212, 222, 230, 240, 247, 259, 270]
STORVIK_VGPRS = [200, 209, 207, 211, 213, 217, 222, 227, 232, 237, 242, 247, 255, 262, 264, 266]
# and of k_lw as it was written.  Its normals, searches, gathers, normalisation and resampling are dlm_pf_common.h's now and keep
# these; its initial cloud, its results tail and the order of LwArgs' fields stay its own because each moves a count (profiles/r23_notes.md)
LW_VGPRS = [200, 205, 208, 205, 209, 212, 217, 220, 224, 229, 233, 237, 241, 245, 249, 253]


def test_kernels_have_no_scratch_and_no_spills():
    """dlm_lw.o: every instantiation of k_lw keeps everything in registers; k_pf and k_storvik as before."""
    counts = []
    for d in range(1, 17):
        scratch, spills, vgprs = kernel_resources("dlm_lw.o", f"k_lwILi{d}E")
        counts.append(vgprs)
        assert (scratch, spills) == (0, 0), (d, scratch, spills)
    print("k_lw registers (VGPRs + AGPRs), d = 1 .. 16:", counts)
    assert counts == LW_VGPRS
    for obj, kern, before in (("dlm_pf.o", "k_pf", PF_VGPRS), ("dlm_storvik.o", "k_storvik", STORVIK_VGPRS)):
        res = [kernel_resources(obj, f"{kern}ILi{d}E") for d in range(1, 17)]
        print(f"{kern} registers (VGPRs + AGPRs), d = 1 .. 16:", [r[2] for r in res])
        assert all(r[:2] == (0, 0) for r in res)
        assert [r[2] for r in res] == before, kern


# ---- build and API --------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_call_with_the_header_s_signature():
    lib = _lib.load()
    assert hasattr(lib, "dlm_lw_batch")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dlm_engine.h")).read(), flags=re.S)
    decl = re.search(r"int dlm_lw_batch\(([^;]*)\);", hdr).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    name, res, args = next(s for s in _lib.SYMBOLS if s[0] == "dlm_lw_batch")
    assert res is ctypes.c_int and len(args) == len(params) == 21
    for p, a in zip(params, args):
        if "uint64_t" in p and "*" not in p:
            assert a is ctypes.c_uint64, p
        elif "int64_t" in p and "*" not in p:
            assert a is ctypes.c_int64, p
        else:
            assert "*" in p and a in (ctypes.c_void_p, _lib._MP, _lib._PP, _lib._OP, ctypes.POINTER(_lib.LwDesc)), p
    fields = re.search(r"typedef struct \{([^}]*)\} dlm_lw_desc;", hdr).group(1)
    assert re.findall(r"(?:int32_t|double) (\w+);", fields) == [f for f, _ in _lib.LwDesc._fields_]
    assert [t for _, t in _lib.LwDesc._fields_] == [ctypes.c_int32] * 5 + [ctypes.c_double] and ctypes.sizeof(_lib.LwDesc) == 32
    src = open(os.path.join(ROOT, "bayesian_dlms_amd", "csrc", "dlm_draws.h")).read()
    assert f"DLM_KEY_LW = 0x{lr.KEY_LW:08X}u" in src
    assert (f"DLM_LW_BLOCK_RESAMPLE = {lr.BLOCK_RESAMPLE}u, DLM_LW_BLOCK_FIRST = {lr.BLOCK_FIRST}u, DLM_LW_BLOCK_PARAM = {lr.BLOCK_PARAM}u") in src
    assert "DLM_LW_SLOT_INIT = DLM_SLOT_TOP" in src and lr.SLOT_INIT == 0x1FFFFF
    # no other stream's key shares the upper half of the key word with it
    keys = [int(k, 16) for k in re.findall(r"constexpr unsigned DLM_KEY_\w+ = (0x[0-9A-Fa-f]{8})u", src)]
    assert len(keys) >= 9 and sum((k >> 16) == (lr.KEY_LW >> 16) for k in keys) == 1
    # the glue declares it
    assert "dlm_lw_batch(" in open(os.path.join(ROOT, "integration", "jni", "dlm_jni.cpp")).read()
    assert "@native def lwFilter(" in open(os.path.join(ROOT, "integration", "scala", "Batched.scala")).read()


def test_a_null_engine_or_descriptor_is_an_argument_error():
    lib = _lib.load()
    assert lib.dlm_lw_batch(None, None, None, None, None, 0, None, 0, None, None, 0, None, *([None] * 9)) == -1


def _series(T=6, p=1):
    return np.arange(1.0, T + 1), np.zeros((T, p))[None] if p > 1 else np.zeros(T)


@pytest.mark.parametrize("n", [96, 2048, 0, 32])
def test_python_layer_refuses_particle_counts(n):
    with pytest.raises(EngineError, match="multiple of 64 between 64 and 1024"):
        LiuAndWestFilter(n, 0.95)
    with pytest.raises(EngineError, match="multiple of 64 between 64 and 1024"):
        AuxFilter(n)


@pytest.mark.parametrize("a", [0.0, -0.5, 1.0001, float("nan")])
def test_python_layer_refuses_a_shrinkage_outside_the_unit_interval(a):
    with pytest.raises(ValueError, match="0 < a <= 1"):
        LiuAndWestFilter(128, a)


def test_python_layer_refuses_what_the_engine_does_not_cover():
    from bayesian_dlms_amd.engine import Engine
    par = lambda d, p: DlmParameters(np.eye(p), np.eye(d), np.zeros(d), np.eye(d))
    g = Gaussian(0.0, 0.5)
    with pytest.raises(EngineError, match="d <= 16, got d = 17"):
        LiuAndWestFilter(128, 0.95).filter(Dglm.gaussian(Dlm.polynomial(17)), _series(), par(17, 1), g, g, None)
    two = Dlm.polynomial(1) * Dlm.polynomial(1)
    with pytest.raises(EngineError, match=r"univariate observation \(p = 1"):
        LiuAndWestFilter(128, 0.95).filter(Dglm.gaussian(two), _series(p=2), par(2, 2), g, g, None)
    with pytest.raises(EngineError, match="one Gaussian or d = 2 of them"):
        LiuAndWestFilter(128, 0.95).filter(Dglm.gaussian(Dlm.polynomial(2)), _series(), par(2, 1), g, [g, g, g], None)
    full = DlmParameters(np.eye(1), np.array([[1.0, 0.2], [0.2, 1.0]]), np.zeros(2), np.eye(2))
    with pytest.raises(ValueError, match="diagonal W"):
        AuxFilter(128).filter(Dglm.gaussian(Dlm.polynomial(2)), _series(), full, None)
    # the checks of Engine.lw_filter that come before anything touches the device
    eng = Engine.__new__(Engine)
    from bayesian_dlms_amd.dglm import materialise_pf
    mat = materialise_pf(Dglm.poisson(Dlm.polynomial(1)), np.arange(1.0, 7.0))
    y = np.zeros((1, 6))
    for fam in (_lib.OBS_POISSON, _lib.OBS_NEGBIN, _lib.OBS_ZIP):
        with pytest.raises(EngineError, match="learn_v needs OBS_GAUSSIAN, OBS_STUDENTT or OBS_BETA"):
            Engine.lw_filter(eng, mat, par(1, 1), y, [[0.0, 1.0]], family=fam, n_particles=64, a=0.9, prior_v=[0.0, 1.0], learn_v=True)
    with pytest.raises(EngineError, match="learn_v needs prior_v"):
        Engine.lw_filter(eng, mat, par(1, 1), y, [[0.0, 1.0]], family=_lib.OBS_BETA, n_particles=64, a=0.9)
    with pytest.raises(EngineError, match=r"prior_w must be \[d\]\[2\]"):
        Engine.lw_filter(eng, mat, par(1, 1), y, [0.0, 1.0, 2.0], family=_lib.OBS_POISSON, n_particles=64, a=0.9)
    with pytest.raises(EngineError, match="0 < a <= 1"):
        Engine.lw_filter(eng, mat, par(1, 1), y, [[0.0, 1.0]], family=_lib.OBS_POISSON, n_particles=64, a=0.0)
