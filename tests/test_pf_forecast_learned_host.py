"""The forecast from a learning filter's cloud without a GPU: the restatement (tests/pffl_restatement.py) against the exact laws the GPU tests
hold the kernel to, at the GPU tests' sizes, and two deliberately wrong restatements against the same checks -- the thresholds are honest in
both directions --; the discrete draws of the device comparison within the cap of excused draws on the restatement alone; the new key's
block table against dlm_draws.h; the prototypes against the header; the refusals of the Python layers, raised before any engine call; the
`forecast` wrappers' time0 and slot_offset; the keep-alive under DLM_OPT_ASYNC; and what the code objects say about the new kernels.

Bounds.  Laws: Kolmogorov-Smirnov p-values above 1e-4 (tests/test_pf_forecast_host.py's); fixed seeds, so the tests are deterministic."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pf_restatement as pr  # noqa: E402
import pffl_cases as lc  # noqa: E402
import pffl_restatement as lr  # noqa: E402
from code_object import kernel_resources  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dglm import AuxFilter, Dglm, LiuAndWestFilter, RaoBlackwellFilter, StorvikFilter  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters  # noqa: E402
from bayesian_dlms_amd.engine import Engine, EngineError, check_pf_forecast_learned_lds  # noqa: E402
from bayesian_dlms_amd.gibbs import InverseGamma  # noqa: E402
from bayesian_dlms_amd.stochvol import Gaussian  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the laws, on the restatement and on two wrong ones --------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2])
def test_restatement_has_the_conditional_law_with_log_variances(d):
    kw, cloud, psi_w, psi_v = lc.logvar_law(d)
    ref = lc.restated(kw, cloud, psi_w, psi_v, kind=lr.FC_LOGVAR)
    pvals = lc.logvar_pvalues(d, ref["draws"])
    print(f"d = {d}: p-values at h = 1 and h = H: {pvals}")
    assert not ref["status"].any() and min(pvals) > lc.P_VALUE


def test_restatement_has_the_law_of_scales_drawn_once():
    kw, cloud, bw, bv, shapes = lc.ig_law()
    ref = lc.restated(kw, cloud, bw, bv, kind=lr.FC_IG_SCALE, shapes=shapes)
    pvals = lc.ig_pvalues(ref["cloud"], ref["draws"])
    print(f"p-values of the state's and the observation's Student-t: {pvals}")
    assert not ref["status"].any() and min(pvals) > lc.P_VALUE
    # the Gammas are the ones the restatement hands out, and the variances the scales over them
    series = np.uint64(kw["series_offset"]) + np.arange(lc.IG_N, dtype=np.uint64)
    g = lr.fcl_gamma(np.full(lc.IG_N, lc.IG_SHAPE), kw["seed"], series, kw["iteration"], 0, lc.IG_P, 0)
    np.testing.assert_array_equal(ref["var_w"][:, 0], bw[:, 0] / g)
    from scipy import stats
    assert stats.kstest(g.reshape(-1), stats.gamma(lc.IG_SHAPE).cdf).pvalue > lc.P_VALUE


def test_wrong_restatements_fail_the_same_checks():
    """The checks have teeth at these sizes: a sampler that redraws its variances at every step, and one that leaves the square root out."""
    kw, cloud, bw, bv, shapes = lc.ig_law()
    for mutant in lr.MUTANTS:
        ref = lc.restated(kw, cloud, bw, bv, kind=lr.FC_IG_SCALE, shapes=shapes, mutant=mutant)
        pvals = lc.ig_pvalues(ref["cloud"], ref["draws"])
        print(f"{mutant}: p-values {pvals}")
        assert pvals[0] < lc.P_VALUE, mutant
    kw, cloud, psi_w, psi_v = lc.logvar_law(2)
    ref = lc.restated(kw, cloud, psi_w, psi_v, kind=lr.FC_LOGVAR, mutant="no-sqrt")
    pvals = lc.logvar_pvalues(2, ref["draws"])
    print(f"no-sqrt, log-variances, d = 2: p-values {pvals}")
    assert pvals[1] < lc.P_VALUE


# ---- 2. the inputs of the device comparison ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family_name,kind", lc.DRAW_CASES)
def test_cases_of_the_device_comparison_stay_within_the_cap(family_name, kind):
    """On the restatement alone: every series runs, the rows differ by particle, the entry resampling took some particle twice, and of the
    discrete draws at most 1 in 10^4 would have to be excused."""
    kw, cloud, weights, pw, pv, shapes = lc.draws_case(family_name, kind)
    ref = lc.draws_reference(family_name, kind)
    assert not ref["status"].any() and np.all(np.isfinite(ref["draws"]))
    assert np.ptp(ref["var_w"], axis=2).min() > 0.0
    assert any(len(np.unique(ref["cloud_entry"][n, 0])) < cloud.shape[2] for n in range(cloud.shape[0]))
    if kw["family"] in lc.DISCRETE:
        share = float((ref["margin"] <= lc.MARGIN).mean())
        assert share <= lc.EXCUSED_SHARE, share
    if kind == "ig":
        assert np.all(ref["var_w"] != pw[:, :, :1]) and (pv is None or np.ptp(ref["var_v"], axis=1).min() > 0.0)


def test_restatement_stops_a_poisoned_series_alone():
    kw, cloud, weights, pw, pv, shapes = lc.draws_case("gaussian", "ig")
    good = lc.draws_reference("gaussian", "ig")
    bad_pw, bad_w, bad_sh = pw.copy(), weights.copy(), shapes.copy()
    bad_pw[0, 1, 5] = np.nan
    bad_w[1, 7] = -0.5
    bad_sh[2, 0] = 0.0
    bad = lc.restated(kw, cloud, bad_pw, pv, kind=lr.FC_IG_SCALE, shapes=bad_sh, weights=bad_w, slot_offset=4)
    assert bad["status"].tolist() == [pr.ST_NOT_PD, pr.ST_NONFINITE, pr.ST_NOT_PD] and not good["status"].any()


# ---- 3. the streams -----------------------------------------------------------------------------------------------------------------------------
def test_block_tables_match_the_header():
    src = open(os.path.join(ROOT, "bayesian_dlms_amd", "csrc", "dlm_draws.h")).read()
    assert f"DLM_KEY_FCL = 0x{lr.KEY_FCL:08X}u" in src
    assert f"DLM_FCL_BLOCK_GAMMA = {lr.FCL_BLOCK_GAMMA}u, DLM_FCL_GAMMA_ATTEMPTS = {lr.FCL_GAMMA_ATTEMPTS}u" in src
    assert f"DLM_RB_BLOCK_STATE = {lr.RB_BLOCK_STATE}u" in src and f"DLM_KEY_RB = 0x{lr.KEY_RB:08X}u" in src
    assert src.count("DLM_FCL_") >= 6 and src.count("DLM_RB_BLOCK_STATE") >= 4          # the table, the constants and their static_asserts
    keys = dict(re.findall(r"constexpr unsigned (DLM_KEY_\w+) = (0x[0-9A-Fa-f]+)u", src))
    assert len(set(keys.values())) == len(keys) and "DLM_KEY_FCL" in keys
    # the state draw's blocks stand clear of the Rao-Blackwellised filter's own (resample, first stage, the pairs of d + 1 log-variances)
    assert lr.RB_BLOCK_STATE >= 2 + (_lib.PF_MAX_D + 2) // 2
    kern = open(os.path.join(ROOT, "bayesian_dlms_amd", "csrc", "dlm_pf_forecast_learned.hip")).read()
    assert "while (true)" not in kern and "for (;;)" not in kern
    assert (_lib.FC_VAR, _lib.FC_LOGVAR, _lib.FC_IG_SCALE) == (lr.FC_VAR, lr.FC_LOGVAR, lr.FC_IG_SCALE)
    hdr = open(os.path.join(ROOT, "include", "dlm_engine.h")).read()
    assert "enum { DLM_FC_VAR = 0, DLM_FC_LOGVAR = 1, DLM_FC_IG_SCALE = 2 };" in hdr


# ---- 4. the binding -----------------------------------------------------------------------------------------------------------------------------
def _prototype(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dlm_engine.h")).read(), flags=re.S)
    decl = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
    return hdr, [" ".join(p.split()) for p in decl.split(",")]


def test_library_exports_both_calls_with_the_header_s_signatures():
    lib = _lib.load()
    for name, count in (("dlm_pf_forecast_learned", 22), ("dlm_rb_state_draw", 11)):
        assert hasattr(lib, name)
        hdr, params = _prototype(name)
        _, res, args = next(s for s in _lib.SYMBOLS if s[0] == name)
        assert res is ctypes.c_int and len(args) == len(params) == count
        for p, a in zip(params, args):
            if "uint64_t" in p and "*" not in p:
                assert a is ctypes.c_uint64, p
            elif "int64_t" in p and "*" not in p:
                assert a is ctypes.c_int64, p
            elif "int32_t" in p and "*" not in p:
                assert a is ctypes.c_int32, p
            elif "int32_t* ranks" in p:
                assert a is _lib._ip, p
            else:
                assert "*" in p and a in (ctypes.c_void_p, _lib._MP, _lib._PP, _lib._OP, ctypes.POINTER(_lib.PfForecastLearnedDesc)), p
    fields = re.search(r"typedef struct \{([^}]*)\} dlm_pf_forecast_learned_desc;", hdr).group(1)
    assert re.findall(r"int(?:32|64)_t (\w+);", fields) == [f for f, _ in _lib.PfForecastLearnedDesc._fields_]
    assert dict(_lib.PfForecastLearnedDesc._fields_)["slot_offset"] is ctypes.c_int64
    for d, P in ((1, 64), (8, 1024), (16, 512), (16, 1024)):
        assert _lib.pf_forecast_learned_lds_bytes(d, P) == (2 * d + 3) * P * 8 + 4 * P
    src = open(os.path.join(ROOT, "bayesian_dlms_amd", "csrc", "dlm_pf_forecast_learned.hip")).read()
    assert "return (size_t)(2 * d + 3) * P * sizeof(double) + (size_t)P * sizeof(int);" in src


def test_async_calls_keep_every_array_they_passed_until_sync():
    import test_engine_calls_host as calls
    f32 = lambda *shape: np.random.default_rng(sum(shape)).uniform(0.5, 1.5, shape).astype(np.float32)
    d, N, P = calls.d, calls.N, calls.P
    run = lambda e, f: e.pf_forecast_learned(calls.MAT_PF, calls.PAR, f32(N, d, P), f32(N, d, P), f32(N, P), family=_lib.OBS_STUDENTT,
                                             var_kind=_lib.FC_IG_SCALE, shapes=f32(N, d + 1), weights=f32(N, P), ranks=(1, P // 2, P - 1),
                                             obs_param=5.0, slot_offset=7, want_draws=True, flags=f)
    draw = lambda e, f: e.rb_state_draw(f32(N, d, P), f32(N, d * (d + 1) // 2, P), slot=9, flags=f)
    for fn, symbol, least in ((run, "dlm_pf_forecast_learned", 14), (draw, "dlm_rb_state_draw", 4)):
        eng = calls._engine()
        result = fn(eng, calls.ASYNC)
        kept, own = calls._addresses(eng._keep), calls._addresses(result)
        (_, args, addresses), = [c for c in eng.lib.calls if c[0] == symbol]
        assert len(addresses) >= least and addresses - own <= kept and addresses <= kept, symbol
        eng.sync()
        assert eng._keep == []
        eng = calls._engine()
        out = fn(eng, 0)
        assert eng._keep == []
    assert list(out) == ["cloud", "status"]
    eng = calls._engine()
    out = run(eng, 0)
    assert list(out) == ["fmean", "fquant", "draws", "mean", "cloud", "var_w", "var_v", "status"]
    (_, args, _), = eng.lib.calls
    assert list(args[5]) == [1, P // 2, P - 1] and (args[3].n_ranks, args[3].slot_offset, args[3].n_particles, args[3].var_kind) == (3, 7, P, 2)
    assert args[11] == d + 1          # shapes per series: their stride


# ---- 5. refusals, raised before any engine call ---------------------------------------------------------------------------------------------------
class _NoEngine:
    def __getattr__(self, name):
        raise AssertionError(f"the engine was reached ({name}) before the refusal")


def _stub_engine():
    eng = Engine.__new__(Engine)
    eng.lib, eng.h, eng.device, eng._keep = _NoEngine(), None, 0, []
    return eng


PAR = DlmParameters(np.eye(1), np.eye(1), np.zeros(1), np.eye(1))
MOD = Dglm.poisson(Dlm.polynomial(1))
TIMES = np.arange(1.0, 5.0)


@pytest.mark.parametrize("n", [96, 2048, 32])
def test_refuses_particle_counts(n):
    with pytest.raises(EngineError, match="multiple of 64 between 64 and 1024"):
        Dglm.forecast_learned(MOD, np.zeros((1, 1, n)), np.ones((1, 1, n)), None, TIMES, PAR, _NoEngine(), var_kind=_lib.FC_VAR)
    with pytest.raises(EngineError, match="multiple of 64 between 64 and 1024"):
        _stub_engine().rb_state_draw(np.zeros((1, 1, n)), np.ones((1, 1, n)), slot=0)


def test_refuses_what_does_not_fit_the_lds():
    for d, P in ((16, 512), (8, 1024), (1, 1024)):
        check_pf_forecast_learned_lds(d, P)
    for d, P in ((16, 1024), (16, 640), (9, 1024)):
        with pytest.raises(EngineError, match="LDS"):
            check_pf_forecast_learned_lds(d, P)
    mod = Dglm.gaussian(Dlm.polynomial(16))
    with pytest.raises(EngineError, match="LDS"):
        Dglm.forecast_learned(mod, np.zeros((1, 16, 1024)), np.ones((1, 16, 1024)), None, TIMES, DlmParameters(np.eye(1), np.eye(16), np.zeros(16), np.eye(16)),
                              _NoEngine(), var_kind=_lib.FC_VAR)


def test_refuses_rows_ranks_and_slots():
    from bayesian_dlms_amd.dglm import materialise_forecast
    mat = materialise_forecast(MOD, TIMES, 0.0)
    cloud, rows = np.zeros((2, 1, 64)), np.ones((2, 1, 64))
    kw = dict(family=_lib.OBS_POISSON, var_kind=_lib.FC_VAR)
    call = lambda *a, **k: _stub_engine().pf_forecast_learned(mat, PAR, *a, **dict(kw, **k))
    with pytest.raises(EngineError, match="var_w"):
        call(cloud, None)
    with pytest.raises(EngineError, match="at most 8 ranks"):
        call(cloud, rows, ranks=range(9))
    with pytest.raises(EngineError, match="0 <= rank < n_particles = 64"):
        call(cloud, rows, ranks=(0, 64))
    with pytest.raises(EngineError, match="FC_IG_SCALE needs shapes"):
        call(cloud, rows, var_kind=_lib.FC_IG_SCALE)
    with pytest.raises(EngineError, match="var_kind"):
        call(cloud, rows, var_kind=3)
    for family in (_lib.OBS_NEGBIN, _lib.OBS_ZIP):
        for kind in (_lib.FC_LOGVAR, _lib.FC_IG_SCALE):
            with pytest.raises(EngineError, match="no variance"):
                call(cloud, rows, rows[:, 0], family=family, var_kind=kind, shapes=np.ones(2))
    with pytest.raises(EngineError, match="obs_param"):
        call(cloud, rows, family=_lib.OBS_STUDENTT)
    with pytest.raises(EngineError, match="slot_offset"):
        call(cloud, rows, slot_offset=_lib.PF_MAX_T - 3)
    with pytest.raises(EngineError, match="slot_offset"):
        call(cloud, rows, slot_offset=-1)
    with pytest.raises(EngineError, match="shape"):
        call(cloud, np.ones((2, 2, 64)))
    with pytest.raises(EngineError, match="shape"):
        call(cloud, rows, weights=np.ones((2, 32)))
    with pytest.raises(EngineError, match="shapes must be"):
        call(cloud, rows, var_kind=_lib.FC_IG_SCALE, shapes=np.ones(3))
    with pytest.raises(ValueError, match="outside"):
        Dglm.forecast_learned(MOD, cloud, rows, None, TIMES, PAR, _NoEngine(), var_kind=_lib.FC_VAR, prob=0.001)
    with pytest.raises(ValueError, match="summary"):
        Dglm.forecast_learned(MOD, cloud, rows, None, TIMES, PAR, _NoEngine(), var_kind=_lib.FC_VAR, summary="mode")
    with pytest.raises(EngineError, match="covs must be"):
        _stub_engine().rb_state_draw(np.zeros((1, 2, 64)), np.ones((1, 2, 64)), slot=0)
    with pytest.raises(EngineError, match="slot must"):
        _stub_engine().rb_state_draw(np.zeros((1, 2, 64)), np.ones((1, 3, 64)), slot=1 << 21)


# ---- 6. the wrappers: filter first, then forecast from the last training time and the next Philox slot ------------------------------------------------
class _Recorder:
    """Stands where the engine would: the filters return arrays of the right shapes, the two new calls record what they were given."""

    def __init__(self, N, d, P):
        self.N, self.d, self.P, self.seen = N, d, P, {}

    def _filter(self, T, **extra):
        N, d, P = self.N, self.d, self.P
        out = dict(ll=np.zeros(N), mean=np.zeros((N, T, d)), ess=np.ones((N, T)), cloud=np.zeros((N, d, P)), weights=np.full((N, P), 1.0 / P),
                   status=np.zeros(N, np.int32))
        out.update(extra)
        return out

    def storvik_filter(self, mat, p, y, pw, **kw):
        N, d, P, T = self.N, self.d, self.P, mat.T
        return self._filter(T, scale_mean=np.ones((N, T, d + 1)), scales=np.full((N, d + 1, P), 2.0))

    def lw_filter(self, mat, p, y, pw, **kw):
        N, d, P, T = self.N, self.d, self.P, mat.T
        return self._filter(T, psi_mean=np.zeros((N, T, d + 1)), psi_var=np.zeros((N, T, d + 1)), psi=np.full((N, d + 1, P), -1.0))

    def rb_filter(self, mat, p, y, pw, **kw):
        N, d, P, T = self.N, self.d, self.P, mat.T
        out = self.lw_filter(mat, p, y, pw)
        del out["cloud"]
        return dict(out, cov=np.zeros((N, T, d, d)), means=np.zeros((N, d, P)), covs=np.ones((N, d * (d + 1) // 2, P)))

    def rb_state_draw(self, means, covs, **kw):
        self.seen["draw"] = kw
        return dict(cloud=np.full(means.shape, 3.0), status=np.zeros(self.N, np.int32))

    def pf_forecast_learned(self, mat, params, cloud, var_w, var_v, **kw):
        self.seen["forecast"] = dict(kw, mat=mat, cloud=cloud, var_w=var_w, var_v=var_v)
        N, d, P, H = self.N, self.d, self.P, mat.T
        return dict(fmean=np.zeros((N, H)), fquant=np.zeros((N, H, len(kw["ranks"]))), draws=None, mean=np.zeros((N, H, d)), cloud=np.zeros((N, d, P)),
                    var_w=np.ones((N, d, P)), var_v=np.ones((N, P)), status=np.zeros(N, np.int32))


def test_forecast_wrappers_pass_time0_and_slot_offset():
    N, d, P, T = 2, 2, 64, 7
    mod = Dglm.gaussian(Dlm.polynomial(d))
    p = DlmParameters(np.eye(1), np.diag([0.3, 0.2]), np.zeros(d), np.eye(d))
    train = (np.arange(1.0, T + 1), np.zeros((N, T)))
    test_times = np.array([9.5, 10.5, 12.0])
    runs = {
        "storvik": lambda e: StorvikFilter(P).forecast(mod, train, test_times, p, InverseGamma(3.0, 2.0), InverseGamma(3.0, 1.0), e, seed=4, iteration=2, series_offset=6),
        "lw": lambda e: LiuAndWestFilter(P, 0.95).forecast(mod, train, test_times, p, Gaussian(0.0, 1.0), Gaussian(-1.0, 1.0), e, seed=4, iteration=2, series_offset=6),
        "aux": lambda e: AuxFilter(P).forecast(mod, train, test_times, p, e, seed=4, iteration=2, series_offset=6),
        "rb": lambda e: RaoBlackwellFilter(P, 0.95).forecast(mod, train, test_times, p, Gaussian(0.0, 1.0), Gaussian(-1.0, 1.0), e, seed=4, iteration=2, series_offset=6,
                                                             summary="median"),
    }
    for name, run in runs.items():
        rec = _Recorder(N, d, P)
        out = run(rec)
        seen = rec.seen["forecast"]
        np.testing.assert_array_equal(seen["mat"].dt, [2.5, 1.0, 1.5])          # time0 = the last training time, 7
        assert seen["slot_offset"] == T and (seen["seed"], seen["iteration"], seen["series_offset"]) == (4, 2, 6), name
        assert seen["weights"].shape == (N, P) and seen["var_w"].shape == (N, d, P), name
        assert "filter" in out and "ll" not in out and out["var_w"].shape == (N, d, P) and out["var_v"].shape == (N, P), name
        assert len(seen["ranks"]) == (3 if name == "rb" else 2) and ("median" if name == "rb" else "mean") in out, name
        if name == "storvik":
            assert seen["var_kind"] == _lib.FC_IG_SCALE and seen["var_v"].shape == (N, P)
            np.testing.assert_array_equal(seen["shapes"], np.tile([3.0 + 0.5 * (T - 1), 3.0 + 0.5 * (T - 1), 3.0 + 0.5 * T], (N, 1)))
        else:
            assert seen["var_kind"] == _lib.FC_LOGVAR and seen["shapes"] is None, name
            assert (seen["var_v"] is None) == (name == "aux"), name
        if name == "rb":
            assert rec.seen["draw"] == dict(slot=T, iteration=2, seed=4, series_offset=6)
            assert np.all(seen["cloud"] == 3.0) and np.all(out["cloud0"] == 3.0)
    for cls in (StorvikFilter, LiuAndWestFilter, AuxFilter, RaoBlackwellFilter):
        assert "filter" in cls.forecast.__doc__
    assert "run the filter over them first" in Dglm.forecast_learned.__doc__ and "run the filter over them first" in Engine.pf_forecast_learned.__doc__


# ---- 7. the code objects ----------------------------------------------------------------------------------------------------------------------------
def test_new_kernels_spill_no_vgprs_and_the_state_draw_has_no_scratch():
    """All 16 instantiations of both kernels: no scratch, no spilled VGPRs.  The forecast kernel takes the Gamma and Poisson draws INLINED
    (pf_obs_draw<true>): called, their frames are 16 bytes of private segment at every d.  What the build produces at d > 8:
    the same, within the 512 registers of one wave per SIMD."""
    counts = []
    for d in range(1, 17):
        scratch, spills, vgprs = kernel_resources("dlm_pf_forecast_learned.o", f"k_pf_forecast_learnedILi{d}E")
        counts.append(vgprs)
        assert (scratch, spills) == (0, 0) and vgprs <= (256 if d <= 8 else 512), (d, scratch, spills, vgprs)
        assert kernel_resources("dlm_pf_forecast_learned.o", f"k_rb_state_drawILi{d}E")[:2] == (0, 0), d
    print("k_pf_forecast_learned registers (VGPRs + AGPRs), d = 1 .. 16:", counts)
    print("k_rb_state_draw registers, d = 1 .. 16:", [kernel_resources("dlm_pf_forecast_learned.o", f"k_rb_state_drawILi{d}E")[2] for d in range(1, 17)])
    src = open(os.path.join(ROOT, "bayesian_dlms_amd", "csrc", "dlm_pf_forecast_learned.hip")).read()
    assert "pf_obs_draw<true>(" in src and "__noinline__ double" not in src


def test_forecast_kernel_has_no_scratch_up_to_d_8():
    """No scratch and no spilled VGPRs at d <= 8, within the 256 registers of two waves per SIMD: 165, 167, 169, 171, 175, 183, 194, 198."""
    for d in range(1, 9):
        scratch, spills, vgprs = kernel_resources("dlm_pf_forecast_learned.o", f"k_pf_forecast_learnedILi{d}E")
        assert (scratch, spills) == (0, 0) and vgprs <= 256, (d, scratch, spills, vgprs)
