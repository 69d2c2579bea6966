"""The Storvik filter without a GPU: the restatement the kernel is held to (tests/storvik_restatement.py) against what it must compute --
the evidence p(y_1:T) with the variances integrated over their priors, which a grid integral of the Kalman likelihood gives (unbiased; and
NOT unbiased under `literal`), and the posterior means of the variances against the same grid -- and the inputs of the GPU tests
(tests/storvik_cases.py) against what makes them worth running: both branches of the resampling test taken, and no comparison of the
kernel's within a rounding error of flipping.  Then the code objects, the build and the argument checks.

Bounds.  Evidence: 4 standard errors of the estimate, from its own sample of 4096 replicates.  Margins: those of tests/test_pf_host.py for the
quantities the two filters share (1e-11 for the search and n0, 1e-9 for the distance of 1 / sum W^2 from an integer), and the same relative
1e-11 for the Gamma's accept test and its v <= 0 test.  Posterior means: 2 % relative at P = 1024 (tests/storvik_cases.py)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import storvik_cases as sc  # noqa: E402
import storvik_restatement as sr  # noqa: E402
from code_object import kernel_resources  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dglm import Dglm, StorvikFilter  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters  # noqa: E402
from bayesian_dlms_amd.engine import EngineError  # noqa: E402
from bayesian_dlms_amd.gibbs import InverseGamma  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN, MARGIN_INT = 1e-11, 1e-9


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in sc.TABLE])
def test_table_entry_takes_both_branches_with_margins(name):
    r = sc.reference(name)
    print(f"{name}: share {r['resample_share']:.2f}, margins search {r['margin_search']:.2e}, n0 {r['margin_n0']:.2e}, integer {r['margin_int']:.2e}, "
          f"accept {r['margin_accept']:.2e}, v {r['margin_v']:.2e}")
    assert np.all(r["status"] == 0) and np.all(np.isfinite(r["ll"]))
    if name in sc.FORCED:          # n0 = P, n0 = 0: one branch by construction
        assert r["resample_share"] == sc.FORCED[name]
    else:
        assert 0.0 < r["resample_share"] < 1.0
    assert r["margin_search"] >= MARGIN and r["margin_n0"] >= MARGIN          # (an entry that fails: change its seed, not the bound)
    assert r["margin_int"] >= MARGIN_INT
    assert r["margin_accept"] >= MARGIN and r["margin_v"] >= MARGIN


def test_table_covers_the_shapes():
    t = sc.TABLE
    assert {(c["d"], c["P"]) for c in t} >= {(1, 64), (2, 128), (3, 192), (2, 1024), (16, 64), (16, 512), (8, 1024)}
    assert {c["T"] for c in t} >= {1, 2, 12, 24} and {c["N"] for c in t} >= {1, 5, 67}
    assert {c["family"] for c in t if not c["learn_v"]} == set(range(6)) and {c["literal"] for c in t} == {False, True}
    assert {c["n0"] for c in t} >= {-1, 0, 128} and any(c["per_series"] for c in t) and any(c["w_shape"] < 1.0 for c in t)
    assert any(set(c["missing"]) >= {0, c["T"] - 1} and len(c["missing"]) >= 3 for c in t)
    irr = sc.inputs("p192-d3-irregular")
    assert irr["G"].shape[0] == 3 and (irr["dt"][1:] == 0.0).sum() == 1 and np.all(irr["G"] != 0.0)
    per = sc.inputs("p128-d2-missing-per-series")
    assert per["prior_w"].shape == (5, 2, 2) and per["prior_v"].shape == (5, 2) and per["C0"].shape == (5, 2, 2) and per["m0"].shape == (5, 2)
    # the two largest holdings fit the 160 KB of a workgroup, the next ones do not: (2 d + 3.5) P + d^2 doubles
    lds = lambda d, P: ((2 * d + 3) * P + d * d) * 8 + 4 * P
    assert lds(16, 512) <= 160 * 1024 and lds(8, 1024) <= 160 * 1024 and lds(16, 576) > 160 * 1024 and lds(9, 1024) > 160 * 1024


def test_restatement_reports_failures():
    kw = sc.run_args("learnv0-beta")
    y = kw["y"].copy(); y[2, 5] = 1.5
    r = sr.run(**dict(kw, y=y))
    assert r["status"].tolist() == [0, 0, sr.ST_NONFINITE, 0, 0] and r["ll"][2] == -np.inf
    assert np.all(np.isfinite(r["scale_mean"][2, :5, :2])) and np.all(np.isnan(r["scale_mean"][2, 5:])) and np.all(np.isnan(r["scales"][2]))
    good = sc.reference("learnv0-beta")
    for k in ("ll", "mean", "ess", "scale_mean", "cloud", "weights", "scales"):
        np.testing.assert_array_equal(np.delete(r[k], 2, axis=0), np.delete(good[k], 2, axis=0))
    pw = kw["prior_w"].copy(); pw[1, 1] = 0.0
    r = sr.run(**dict(kw, prior_w=pw))
    assert np.all(r["status"] == sr.ST_NOT_PD) and np.all(r["ll"] == -np.inf)


def test_gamma_of_the_restatement_has_the_gamma_s_moments():
    """Shapes 0.6 (the boost), 1 and 7.5: mean and variance of 64 x 1024 draws within 5 standard errors of the shape."""
    mg = dict(margin_accept=np.inf, margin_v=np.inf)
    for shape in (0.6, 1.0, 7.5):
        g = sr.gamma(np.full(64, shape), 3, np.arange(64, dtype=np.uint64), 1, 2, 1024, 1, mg).ravel()
        n = g.size
        assert np.all(g > 0.0)
        assert abs(g.mean() - shape) <= 5.0 * np.sqrt(shape / n)
        m4 = ((g - g.mean()) ** 4).mean()
        assert abs(g.var() - shape) <= 5.0 * np.sqrt((m4 - shape * shape) / n)


# ---- the evidence ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(which, **over):
        key = (which, tuple(sorted(over.items())))
        if key not in cache:
            cache[key] = sr.run(**sc.evidence_args(which, **over))
        return cache[key]
    return get


@pytest.mark.parametrize("which", ["level", "dense"])
def test_grid_integral_has_converged(which):
    log_z, means, edge = sc.exact(which)
    fine, fine_means, _ = sc.exact(which, 2 * sc.GRID - 1)
    print(f"{which}: log Z = {log_z:.10f} (half the spacing: {fine - log_z:+.1e}), posterior means {means}, edge {edge:.1e}")
    assert abs(fine - log_z) < 1e-9 and edge < 1e-30
    np.testing.assert_allclose(means, fine_means, rtol=1e-9)


@pytest.mark.parametrize("which", ["level", "dense"])
def test_evidence_estimate_is_unbiased(runs, which):
    log_z, _, _ = sc.exact(which)
    r = runs(which)
    m, se, top = sc.unbiasedness(r["ll"], log_z)
    print(f"{which}: mean exp(ll - log Z) = {m:.5f} +- {se:.5f} (largest ratio {top:.1f}), share of steps resampled {r['resample_share']:.2f}")
    assert np.all(r["status"] == 0) and abs(m - 1.0) <= sc.SIGMAS * se
    assert 0.05 < r["resample_share"] < 0.95          # the estimate went through both branches


@pytest.mark.parametrize("which", ["level", "dense"])
def test_the_same_check_fails_under_literal(runs, which):
    """Q43: the weights of a step that did not resample are forgotten."""
    log_z, _, _ = sc.exact(which)
    m, se, _ = sc.unbiasedness(runs(which, literal=True)["ll"], log_z)
    print(f"{which}, literal: mean exp(ll - log Z) = {m:.5f} +- {se:.5f}")
    assert abs(m - 1.0) > sc.SIGMAS * se


def test_posterior_means_of_the_variances_at_the_last_step(runs):
    _, (ev, ew), _ = sc.exact("level")
    a = sc.evidence_inputs("level")
    r = runs("level", replicates=sc.MEANS_REPLICATES, P=sc.MEANS_P)
    vm, wm = sc.final_variance_means(r, a)
    print(f"P = {sc.MEANS_P}, {sc.MEANS_REPLICATES} replicates: v_mean {vm:.5f} against {ev:.5f} ({vm / ev - 1.0:+.2%}), "
          f"w_mean {wm[0]:.5f} against {ew:.5f} ({wm[0] / ew - 1.0:+.2%})")
    assert abs(vm / ev - 1.0) <= sc.MEANS_RTOL and abs(wm[0] / ew - 1.0) <= sc.MEANS_RTOL
    # the check is sharp: the literal filter is off by a multiple in V
    lit = runs("level", replicates=sc.MEANS_REPLICATES, P=sc.MEANS_P, literal=True)
    vl, _ = sc.final_variance_means(lit, a)
    print(f"literal: v_mean {vl:.5f} ({vl / ev:.2f} x)")
    assert abs(vl / ev - 1.0) > 10 * sc.MEANS_RTOL


# ---- the code objects -----------------------------------------------------------------------------------------------------------------
def test_kernels_have_no_scratch_and_no_spills():
    """dlm_storvik.o: every instantiation of k_storvik keeps everything in registers.  dlm_pf.o after the helpers moved to dlm_pf_common.h:
    as before, no scratch and no spills (its register counts, unchanged by the move, are in profiles/r20_notes.md)."""
    counts = []
    for d in range(1, 17):
        scratch, spills, vgprs = kernel_resources("dlm_storvik.o", f"k_storvikILi{d}E")
        counts.append(vgprs)
        assert (scratch, spills) == (0, 0), (d, scratch, spills)
    print("k_storvik registers (VGPRs + AGPRs), d = 1 .. 16:", counts)
    pf = [kernel_resources("dlm_pf.o", f"k_pfILi{d}E") for d in range(1, 17)]
    print("k_pf registers (VGPRs + AGPRs), d = 1 .. 16:", [r[2] for r in pf])
    assert all(r[:2] == (0, 0) for r in pf)


# ---- build and API --------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_call_with_the_header_s_signature():
    lib = _lib.load()
    assert hasattr(lib, "dlm_storvik_batch")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dlm_engine.h")).read(), flags=re.S)
    decl = re.search(r"int dlm_storvik_batch\(([^;]*)\);", hdr).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    name, res, args = next(s for s in _lib.SYMBOLS if s[0] == "dlm_storvik_batch")
    assert res is ctypes.c_int and len(args) == len(params) == 20
    for p, a in zip(params, args):
        if "uint64_t" in p and "*" not in p:
            assert a is ctypes.c_uint64, p
        elif "int64_t" in p and "*" not in p:
            assert a is ctypes.c_int64, p
        else:
            assert "*" in p and a in (ctypes.c_void_p, _lib._MP, _lib._PP, _lib._OP, ctypes.POINTER(_lib.StorvikDesc)), p
    fields = re.search(r"typedef struct \{([^}]*)\} dlm_storvik_desc;", hdr).group(1)
    assert re.findall(r"int32_t (\w+);", fields) == [f for f, _ in _lib.StorvikDesc._fields_]
    src = open(os.path.join(ROOT, "bayesian_dlms_amd", "csrc", "dlm_draws.h")).read()
    assert f"DLM_KEY_STORVIK = 0x{sr.KEY_STORVIK:08X}u" in src
    assert (f"DLM_STORVIK_BLOCK_RESAMPLE = {sr.BLOCK_RESAMPLE}u, DLM_STORVIK_BLOCK_GAMMA = {sr.BLOCK_GAMMA}u, "
            f"DLM_STORVIK_GAMMA_ATTEMPTS = {sr.GAMMA_ATTEMPTS}u") in src
    assert "DLM_STORVIK_SLOT_INIT = DLM_SLOT_TOP" in src and sr.SLOT_INIT == 0x1FFFFF
    # no other stream's key shares the upper half of the key word with it: the two low bytes are the attempt and the block
    keys = [int(k, 16) for k in re.findall(r"constexpr unsigned DLM_KEY_\w+ = (0x[0-9A-Fa-f]{8})u", src)]
    assert len(keys) >= 8 and sum((k >> 16) == (sr.KEY_STORVIK >> 16) for k in keys) == 1


def test_a_null_engine_or_descriptor_is_an_argument_error():
    lib = _lib.load()
    assert lib.dlm_storvik_batch(None, None, None, None, None, 0, None, 0, None, None, 0, None, None, None, None, None, None, None, None, None) == -1


def _series(T=6, p=1):
    return np.arange(1.0, T + 1), np.zeros((T, p))[None] if p > 1 else np.zeros(T)


@pytest.mark.parametrize("n", [96, 2048, 0, 32])
def test_python_layer_refuses_particle_counts(n):
    with pytest.raises(EngineError, match="multiple of 64 between 64 and 1024"):
        StorvikFilter(n)


def test_python_layer_refuses_what_the_engine_does_not_cover():
    from bayesian_dlms_amd.engine import Engine
    par = lambda d, p: DlmParameters(np.eye(p), np.eye(d), np.zeros(d), np.eye(d))
    ig = InverseGamma(4.0, 1.0)
    with pytest.raises(EngineError, match="d <= 16, got d = 17"):
        StorvikFilter(128).filter(Dglm.gaussian(Dlm.polynomial(17)), _series(), par(17, 1), ig, ig, None)
    two = Dlm.polynomial(1) * Dlm.polynomial(1)
    with pytest.raises(EngineError, match=r"univariate observation \(p = 1"):
        StorvikFilter(128).filter(Dglm.gaussian(two), _series(p=2), par(2, 2), ig, ig, None)
    with pytest.raises(EngineError, match="one InverseGamma or d = 2 of them"):
        StorvikFilter(128).filter(Dglm.gaussian(Dlm.polynomial(2)), _series(), par(2, 1), ig, [ig, ig, ig], None)
    # the checks of Engine.storvik_filter that come before anything touches the device
    eng = Engine.__new__(Engine)
    from bayesian_dlms_amd.dglm import materialise_pf
    mat = materialise_pf(Dglm.poisson(Dlm.polynomial(1)), np.arange(1.0, 7.0))
    y = np.zeros((1, 6))
    with pytest.raises(EngineError, match="learn_v needs OBS_GAUSSIAN"):
        Engine.storvik_filter(eng, mat, par(1, 1), y, [[4.0, 1.0]], family=_lib.OBS_POISSON, n_particles=64, prior_v=[4.0, 1.0], learn_v=True)
    with pytest.raises(EngineError, match="learn_v needs prior_v"):
        Engine.storvik_filter(eng, mat, par(1, 1), y, [[4.0, 1.0]], family=_lib.OBS_GAUSSIAN, n_particles=64)
    with pytest.raises(EngineError, match=r"prior_w must be \[d\]\[2\]"):
        Engine.storvik_filter(eng, mat, par(1, 1), y, [4.0, 1.0, 2.0], family=_lib.OBS_POISSON, n_particles=64)
