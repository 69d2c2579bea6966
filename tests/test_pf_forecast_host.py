"""The particle forecast without a GPU: the restated observation samplers (tests/pff_restatement.py) against the laws they must have, the
interval rule of Dglm.meanAndIntervals / medianAndIntervals, the inputs of the GPU tests (tests/pff_cases.py) against what makes them worth
running, and the refusals of the Python layers, which are raised before any engine call.

Bounds.  Laws: 65 536 draws from fixed seeds, chi-square against the exact pmf (bins merged to an expected count of at least 20) for the
counts, Kolmogorov-Smirnov against the exact cdf for the others, every p-value above 1e-4 -- a fixed-seed test is deterministic, and a
wrong sampler (a rate off by 1 %, a normal approximation, a threshold on the wrong side) has a p-value below 1e-30 at this size.  Excused
draws: at most 1 in 10^4 of a case may have a restated margin of 1e-9 or less (the expected share is far smaller)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pf_restatement as pr  # noqa: E402
import pff_cases as fc  # noqa: E402
import pff_restatement as fr  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dglm import Dglm, ParticleFilter, materialise_forecast, materialise_pf  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters  # noqa: E402
from bayesian_dlms_amd.engine import Engine, EngineError, check_pf_ranks  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the laws of the restated samplers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.POINT_NAMES)
def test_restated_sampler_has_the_right_law(name):
    p = fc.point_by_name(name)
    draws, margins = fc.restated_draws(p)
    pv = fc.law_pvalue(p, draws)
    excused = float((margins <= fc.MARGIN).mean())
    print(f"{name}: p-value {pv:.4f}, excused share {excused:.2e}")
    assert draws.shape == (fc.LAW_DRAWS,) and pv > fc.P_VALUE
    assert excused <= fc.EXCUSED_SHARE


def test_a_wrong_sampler_fails_the_same_check():
    """The check has teeth: the right draws at a rate 2 % off, and a rounded normal approximation in place of the exact Poisson draw."""
    p = fc.point_by_name("poisson-37.5")
    draws, _ = fc.restated_draws(p)
    assert fc.law_pvalue(dict(p, eta=p["eta"] + 0.02), draws) < 1e-12
    z = fr.normal_draw(fr.batch_site(3, np.arange(64), 0, 0, 1024))
    assert fc.law_pvalue(fc.point_by_name("poisson-4"), np.maximum(np.round(4.0 + 2.0 * z), 0.0)) < 1e-12


def test_sampler_edges():
    site = fr.batch_site(1, np.arange(1), 0, 0, 64)
    zero, _ = fr.poisson_draw(np.zeros(64), site)
    assert np.all(zero == 0.0)                                  # lambda = 0 gives 0
    for lam in (np.inf, np.nan, -1.0, 2e15):
        assert np.all(np.isnan(fr.poisson_draw(np.full(64, lam), site)[0]))
    bad, _ = fr.obs_draw(pr.BETA, np.zeros(64), 0.3, None, site)       # variance above mean (1 - mean): alpha <= 0 (Q41)
    assert np.all(np.isnan(bad))
    y, _ = fr.obs_draw(pr.ZIP, np.full(64, 800.0), -1.0, None, site)   # exp(eta) overflows: the rate is refused, zero-inflated or not
    assert np.all(np.isnan(y))


def test_degenerate_cases_of_the_device_comparison_stay_within_the_cap():
    """The inputs of the GPU comparison, on the restatement alone: eta is eta* to rounding, and no discrete draw has to be excused (at most
    1 in 10^4 of the 4096 draws of a case may be: none)."""
    for p in fc.LAW_POINTS:
        ref = fc.degenerate_reference(p["name"], 4, 256, 4)
        assert np.all(np.abs(ref["eta"] - p["eta"]) <= 1e-13) and np.all(np.isfinite(ref["draws"]))
        if p["family"] in fc.DISCRETE:
            share = float((ref["margin"] <= fc.MARGIN).mean())
            assert share <= fc.EXCUSED_SHARE, (p["name"], share)


def test_block_table_matches_the_header():
    src = open(os.path.join(ROOT, "bayesian_dlms_amd", "csrc", "dlm_draws.h")).read()
    assert f"DLM_PF_BLOCK_RESAMPLE0 = {fr.BLOCK_RESAMPLE0}u, DLM_PF_BLOCK_OBS = {fr.BLOCK_OBS}u" in src
    assert f"DLM_PF_POISSON_ATTEMPTS = {fr.POISSON_ATTEMPTS}u, DLM_PF_GAMMA_ATTEMPTS = {fr.GAMMA_ATTEMPTS}u" in src
    assert f"DLM_PF_BLOCK_POISSON = {fr.BLOCK_POISSON}u" in src
    assert (fr.BLOCK_GAMMA_A, fr.BLOCK_GAMMA_B) == (43, 76) and fr.BLOCK_GAMMA_B + fr.GAMMA_ATTEMPTS < 256
    obs = open(os.path.join(ROOT, "bayesian_dlms_amd", "csrc", "dlm_obs_draws.h")).read()
    assert f"PF_POISSON_PTRS_FROM = {fr.PTRS_FROM}" in obs and f"PF_POISSON_INVERSION_STEPS = {fr.INVERSION_STEPS}" in obs
    assert "while (true)" not in obs and "for (;;)" not in obs


# ---- 2. the interval rule ---------------------------------------------------------------------------------------------------------------------
def test_intervals_reproduce_the_reference_rule_on_a_hand_worked_case():
    """n = 8, prob = 0.75: index = floor(6.0) = 6; sorted = [1, 1, 2, 3, 4, 5, 6, 9]: upper = sorted[6] = 6, lower = sorted[8 - 6] = 2,
    median = sorted[4] = 4, mean = 31 / 8.  Two columns: the second is the first reversed and negated."""
    x = np.array([3.0, 1.0, 4.0, 1.0, 5.0, 9.0, 2.0, 6.0])
    samples = np.stack([x, -x[::-1]], axis=1)
    mean, lower, upper = Dglm.mean_and_intervals(0.75)(samples)
    np.testing.assert_array_equal(mean, [3.875, -3.875])
    np.testing.assert_array_equal(lower, [2.0, -5.0])
    np.testing.assert_array_equal(upper, [6.0, -1.0])
    median, lower2, upper2 = Dglm.median_and_intervals(0.75)(samples)
    np.testing.assert_array_equal(median, [4.0, -3.0])
    np.testing.assert_array_equal(lower2, lower)
    np.testing.assert_array_equal(upper2, upper)
    assert Dglm.interval_ranks(8, 0.75) == (2, 4, 6)


@pytest.mark.parametrize("n,prob", [(8, 0.1), (8, 1.0), (8, 0.0), (8, 1.5), (8, -0.2), (8, float("nan")), (1024, 0.0005)])
def test_intervals_refuse_a_prob_whose_indices_fall_outside_the_sample(n, prob):
    with pytest.raises(ValueError, match="outside"):
        Dglm.interval_ranks(n, prob)
    with pytest.raises(ValueError, match="outside"):
        Dglm.mean_and_intervals(prob)(np.zeros((n, 2)))
    with pytest.raises(ValueError, match="outside"):
        Dglm.median_and_intervals(prob)(np.zeros((n, 2)))


@pytest.mark.parametrize("n,prob", [(64, 0.75), (192, 0.9), (1024, 0.975), (320, 0.5), (64, 0.02)])
def test_ranks_are_the_indices_the_host_functions_use(n, prob):
    lo, med, up = Dglm.interval_ranks(n, prob)
    assert (up, lo, med) == (int(np.floor(n * prob)), n - int(np.floor(n * prob)), n // 2)
    x = np.random.default_rng(n).permutation(n).astype(np.float64)          # sorted: 0 .. n - 1, so a statistic IS its rank
    _, lower, upper = Dglm.mean_and_intervals(prob)(x)
    median, _, _ = Dglm.median_and_intervals(prob)(x)
    assert (lower[0], median[0], upper[0]) == (lo, med, up)


# ---- 3. refusals, raised before any engine call ------------------------------------------------------------------------------------------------
PAR = DlmParameters(np.eye(1), np.eye(1), np.zeros(1), np.eye(1))
MOD = Dglm.poisson(Dlm.polynomial(1))
YS = (np.arange(1.0, 5.0), np.full(4, np.nan))


class _NoEngine:
    """Stands where the engine would: any call fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the engine was reached ({name}) before the refusal")


def _stub_engine():
    eng = Engine.__new__(Engine)
    eng.lib, eng.h, eng.device, eng._keep = _NoEngine(), None, 0, []
    return eng


@pytest.mark.parametrize("n", [96, 2048, 32])
def test_forecast_refuses_particle_counts(n):
    with pytest.raises(EngineError, match="multiple of 64 between 64 and 1024"):
        Dglm.forecast_particles(MOD, np.zeros((1, 1, n)), PAR, YS, _NoEngine())
    with pytest.raises(EngineError, match="multiple of 64 between 64 and 1024"):
        _stub_engine().pf_forecast(materialise_pf(MOD, YS[0]), PAR, np.full((1, 4), np.nan), family=_lib.OBS_POISSON, n_particles=n)


def test_forecast_refuses_ranks_and_weights_without_a_cloud():
    mat, y = materialise_pf(MOD, YS[0]), np.full((1, 4), np.nan)
    kw = dict(family=_lib.OBS_POISSON, n_particles=64)
    with pytest.raises(EngineError, match="at most 8 ranks"):
        _stub_engine().pf_forecast(mat, PAR, y, ranks=range(9), **kw)
    with pytest.raises(EngineError, match="0 <= rank < n_particles = 64"):
        _stub_engine().pf_forecast(mat, PAR, y, ranks=(0, 64), **kw)
    with pytest.raises(EngineError, match="0 <= rank < n_particles = 64"):
        _stub_engine().pf_forecast(mat, PAR, y, ranks=(-1,), **kw)
    with pytest.raises(EngineError, match="weights need the cloud"):
        _stub_engine().pf_forecast(mat, PAR, y, weights=np.full((1, 64), 1 / 64), **kw)
    with pytest.raises(EngineError, match="weights need the cloud"):
        Dglm.forecast_particles(MOD, None, PAR, YS, _NoEngine(), weights=np.full((1, 64), 1 / 64), n_particles=64)
    with pytest.raises(EngineError, match="slot_offset"):
        _stub_engine().pf_forecast(mat, PAR, y, slot_offset=_lib.PF_MAX_T - 3, **kw)
    with pytest.raises(ValueError, match="outside"):
        Dglm.forecast_particles(MOD, np.zeros((1, 1, 64)), PAR, YS, _NoEngine(), prob=0.001)
    with pytest.raises(ValueError, match="summary"):
        Dglm.forecast_particles(MOD, np.zeros((1, 1, 64)), PAR, YS, _NoEngine(), summary="mode")
    assert check_pf_ranks((0, 63), 64) == [0, 63]


# ---- the binding: the symbol, its prototype, the one call path ------------------------------------------------------------------------------------
def test_library_exports_the_call_with_the_header_s_signature():
    lib = _lib.load()
    assert hasattr(lib, "dlm_pf_forecast_particles")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dlm_engine.h")).read(), flags=re.S)
    decl = re.search(r"int dlm_pf_forecast_particles\(([^;]*)\);", hdr).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    name, res, args = next(s for s in _lib.SYMBOLS if s[0] == "dlm_pf_forecast_particles")
    assert res is ctypes.c_int and len(args) == len(params) == 19
    for p, a in zip(params, args):
        if "uint64_t" in p and "*" not in p:
            assert a is ctypes.c_uint64, p
        elif "int32_t* ranks" in p:
            assert a is _lib._ip, p
        else:
            assert "*" in p and a in (ctypes.c_void_p, _lib._MP, _lib._PP, _lib._OP, ctypes.POINTER(_lib.PfForecastDesc)), p
    fields = re.search(r"typedef struct \{([^}]*)\} dlm_pf_forecast_desc;", hdr).group(1)
    assert re.findall(r"int(?:32|64)_t (\w+);", fields) == [f for f, _ in _lib.PfForecastDesc._fields_]
    assert re.search(r"int64_t\s+slot_offset;", fields) and dict(_lib.PfForecastDesc._fields_)["slot_offset"] is ctypes.c_int64


def test_async_forecast_keeps_every_array_it_passed_until_sync():
    """Engine.pf_forecast goes through Engine._call: under DLM_OPT_ASYNC every array whose address crossed is held until sync(), the float64
    copies `put` made of float32 inputs included; without the flag nothing is held.  (What tests/test_engine_calls_host.py asserts of the
    *_batch entry points, by its own recording stub.)"""
    import test_engine_calls_host as calls
    f32 = lambda *shape: np.random.default_rng(sum(shape)).uniform(0.5, 1.5, shape).astype(np.float32)
    d, T, N, P = calls.d, calls.T, calls.N, calls.P
    run = lambda e, f: e.pf_forecast(calls.MAT_PF, calls.PAR, calls.Y1, cloud=f32(N, d, P), weights=f32(N, P), ranks=(1, P // 2, P - 1),
                                     want_draws=True, flags=f, **calls.pf)
    eng = calls._engine()
    result = run(eng, calls.ASYNC)
    kept, own = calls._addresses(eng._keep), calls._addresses(result)
    (symbol, args, addresses), = [c for c in eng.lib.calls if c[0] == "dlm_pf_forecast_particles"]
    assert len(addresses) >= 10 and addresses - own <= kept and addresses <= kept
    assert list(args[5]) == [1, P // 2, P - 1] and (args[3].n_ranks, args[3].slot_offset, args[3].n_particles) == (3, 0, P)
    eng.sync()
    assert eng._keep == []
    eng = calls._engine()
    out = run(eng, 0)
    assert eng._keep == [] and list(out) == ["fmean", "fquant", "draws", "ll", "mean", "cloud", "weights", "status"]


# ---- the forecast grid ---------------------------------------------------------------------------------------------------------------------------
def test_forecast_grid_starts_at_the_cloud_s_time():
    mod = Dlm(lambda t: np.array([[1.0], [0.0]]), lambda step: np.array([[1.0, step], [0.0, 1.0]]))          # a G that depends on the step
    times = np.array([5.0, 6.0, 6.0, 8.5])
    ref = materialise_forecast(mod, times)                 # the reference's scan: the first step has dt = 0 (Q71)
    np.testing.assert_array_equal(ref.dt, [0.0, 1.0, 0.0, 2.5])
    mat = materialise_forecast(mod, times, time0=3.0)
    np.testing.assert_array_equal(mat.dt, [2.0, 1.0, 0.0, 2.5])
    assert mat.n_g == 3 and mat.g_index.tolist() == [1, 0, 0, 2]
    for k, step in enumerate((1.0, 2.0, 2.5)):
        np.testing.assert_array_equal(mat.G[4 * k:4 * k + 4].reshape(2, 2).T, mod.g(step))
    with pytest.raises(ValueError, match="must not"):
        materialise_forecast(mod, times, time0=5.5)
    assert ParticleFilter(64).forecast.__doc__ and Dglm.forecast_particles.__doc__
