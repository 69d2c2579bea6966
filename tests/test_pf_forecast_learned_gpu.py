"""dlm_pf_forecast_learned and dlm_rb_state_draw on the device (bayesian_dlms_amd/csrc/dlm_pf_forecast_learned.hip).

Bounds.  RTOL, ATOL = 1e-11, 1e-12 (tests/test_pf_gpu.py's) where the device's exp / log / cos / sqrt stand between the kernel and its NumPy
restatement; exact equality where they do not (the anchor: the same kernel code on both sides) and for the discrete draws whose restated
margin exceeds 1e-9, at most 1 in 10^4 excused (tests/test_pf_forecast_gpu.py's rule); law tests at p > 1e-4 and 4.5 standard errors."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pf_cases as pc  # noqa: E402
import pf_restatement as pr  # noqa: E402
import pff_cases as fc  # noqa: E402
import pffl_cases as lc  # noqa: E402
import pffl_restatement as lr  # noqa: E402

from bayesian_dlms_amd import _lib, api  # noqa: E402
from bayesian_dlms_amd.dglm import AuxFilter, Dglm, LiuAndWestFilter, RaoBlackwellFilter, StorvikFilter  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters  # noqa: E402
from bayesian_dlms_amd.engine import Engine, EngineError, _Host  # noqa: E402
from bayesian_dlms_amd.gibbs import InverseGamma  # noqa: E402
from bayesian_dlms_amd.stochvol import Gaussian  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-11, 1e-12
SIGMAS = 4.5
KEYS = ("fmean", "fquant", "draws", "mean", "cloud", "var_w", "var_v", "status")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


# ---- 1. the anchor: equal variances are the existing kernel, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", lc.ANCHOR_NAMES)
def test_equal_variances_reproduce_the_particle_forecast_bit_for_bit(eng, name, weighted):
    kw, cloud, weights, pw, pv = lc.anchor(name)
    P = kw["P"]
    w = weights if weighted else None
    ranks = (0, P // 4, P // 2, P - 1)
    old = fc.forecast_run(eng, kw, cloud=cloud, weights=w, slot_offset=9, ranks=ranks, want_draws=True)
    new = lc.learned_run(eng, kw, cloud, pw, pv, kind=_lib.FC_VAR, weights=w, slot_offset=9, ranks=ranks)
    shared = lc.learned_run(eng, kw, cloud, pw, None, kind=_lib.FC_VAR, weights=w, slot_offset=9, ranks=ranks)          # every particle takes params->V
    assert not old["status"].any() and not new["status"].any() and kw["dt"][0] == 0.0 and len(set(kw["dt"])) >= 3          # (a dt = 0 first step, an irregular grid)
    for k in ("fmean", "fquant", "draws", "mean", "cloud"):
        np.testing.assert_array_equal(new[k], old[k], err_msg=k)
        np.testing.assert_array_equal(shared[k], old[k], err_msg=k)
    np.testing.assert_array_equal(new["var_v"], pv)
    np.testing.assert_array_equal(new["var_w"], pw)


# ---- 2. every D launched once ------------------------------------------------------------------------------------------------------------------------
def _compare(out, ref, family=pr.GAUSSIAN, what=""):
    np.testing.assert_array_equal(out["status"], ref["status"], err_msg=what)
    for k in ("var_w", "var_v", "cloud", "mean"):
        np.testing.assert_allclose(out[k], ref[k], rtol=RTOL, atol=ATOL, err_msg=f"{what} {k}")
    if family in lc.DISCRETE:
        held = ref["margin"] > lc.MARGIN
        differ = int((out["draws"] != ref["draws"]).sum())
        print(f"{what}: {differ} of {held.size} draws differ, {int((~held).sum())} excused")
        assert 1.0 - held.mean() <= lc.EXCUSED_SHARE
        np.testing.assert_array_equal(out["draws"][held], ref["draws"][held])
    else:
        rel = np.abs(out["draws"] - ref["draws"]) / (np.abs(ref["draws"]) + ATOL / RTOL)
        print(f"{what}: largest relative difference of a draw {rel.max():.2e}")
        np.testing.assert_allclose(out["draws"], ref["draws"], rtol=RTOL, atol=ATOL, err_msg=what)
        np.testing.assert_allclose(out["fmean"], ref["fmean"], rtol=RTOL, atol=ATOL, err_msg=what)
    # the summaries are those of the kernel's own draws, bit for bit
    np.testing.assert_array_equal(out["fmean"], np.stack([lr.fr.forecast_mean(out["draws"][:, h]) for h in range(out["draws"].shape[1])], axis=1))


@pytest.mark.parametrize("d", range(1, 17))
def test_every_state_dimension_matches_the_restatement(eng, d):
    kw, cloud, weights, psi_w, psi_v = lc.dims_case(d)
    P = kw["P"]
    out = lc.learned_run(eng, kw, cloud, psi_w, psi_v, kind=_lib.FC_LOGVAR, weights=weights, slot_offset=2, ranks=(0, P - 1))
    ref = lc.restated(kw, cloud, psi_w, psi_v, kind=lr.FC_LOGVAR, weights=weights, slot_offset=2)
    _compare(out, ref, what=f"d = {d}")
    np.testing.assert_array_equal(out["fquant"], np.sort(out["draws"], axis=2)[:, :, [0, P - 1]])
    assert eng.last_variant == "pf-forecast-learned-wave"


def test_lds_boundary_runs_and_beyond_is_unsupported(eng):
    kw, cloud, weights, psi_w, psi_v = lc.dims_case(16, P=512, N=1)
    out = lc.learned_run(eng, kw, cloud, psi_w, psi_v, kind=_lib.FC_LOGVAR, weights=weights, ranks=(0, 256, 511))
    ref = lc.restated(kw, cloud, psi_w, psi_v, kind=lr.FC_LOGVAR, weights=weights)
    _compare(out, ref, what="d = 16, P = 512")
    np.testing.assert_array_equal(out["fquant"], np.sort(out["draws"], axis=2)[:, :, [0, 256, 511]])
    # d = 16, P = 1024: refused by the engine itself, before any launch
    N, d, P, H = 1, 16, 1024, 2
    md, pd, op, keep = eng.prepare(pc.materialised(kw), pc.packed_params(kw, N), N, _Host())
    big, fmean = np.zeros((N, d, P)), np.full((N, H), -7.0)
    desc = _lib.PfForecastLearnedDesc(0, P, _lib.FC_VAR, 0, 0)
    ptr = _Host.ptr
    rc = eng.lib.dlm_pf_forecast_learned(eng.h, md, pd, ctypes.byref(desc), None, None, ptr(big), None, ptr(big + 1.0), None, None, 0, 0, op,
                                         ptr(fmean), None, None, None, None, None, None, None)
    assert rc == -3 and b"LDS" in eng.lib.dlm_last_error(eng.h) and np.all(fmean == -7.0)
    with pytest.raises(EngineError, match="LDS"):
        eng.pf_forecast_learned(pc.materialised(kw), pc.packed_params(kw, N), big, big + 1.0, None, family=0, var_kind=_lib.FC_VAR)


# ---- 3. the draws against the restatement, all three kinds of rows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("family_name,kind", lc.DRAW_CASES)
def test_kernel_draws_match_the_restatement(eng, family_name, kind):
    kw, cloud, weights, pw, pv, shapes = lc.draws_case(family_name, kind)
    ref = lc.draws_reference(family_name, kind)
    out = lc.learned_run(eng, kw, cloud, pw, pv, kind=lc.KINDS[kind], shapes=shapes, weights=weights, slot_offset=4, ranks=(0, 64, 127))
    _compare(out, ref, family=kw["family"], what=f"{family_name} {kind}")
    np.testing.assert_array_equal(out["fquant"], np.sort(out["draws"], axis=2)[:, :, [0, 64, 127]])
    if pv is None:
        assert np.all(out["var_v"] == kw["V"])


# ---- 4. the exact conditional law with log-variances -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2])
def test_device_draws_have_the_conditional_law_with_log_variances(eng, d):
    kw, cloud, psi_w, psi_v = lc.logvar_law(d)
    out = lc.learned_run(eng, kw, cloud, psi_w, psi_v, kind=_lib.FC_LOGVAR, device=True)
    pvals = lc.logvar_pvalues(d, out["draws"])
    print(f"d = {d}: p-values at h = 1 and h = H: {pvals}")
    assert not out["status"].any() and min(pvals) > lc.P_VALUE


# ---- 5. the exact law with InverseGamma scales, drawn once -----------------------------------------------------------------------------------------------------
def test_device_draws_have_the_law_of_scales_drawn_once(eng):
    kw, cloud, bw, bv, shapes = lc.ig_law()
    out = lc.learned_run(eng, kw, cloud, bw, bv, kind=_lib.FC_IG_SCALE, shapes=shapes, device=True)
    pvals = lc.ig_pvalues(out["cloud"], out["draws"])
    print(f"p-values of the state's and the observation's Student-t: {pvals}")
    assert not out["status"].any() and min(pvals) > lc.P_VALUE


# ---- 6. the Rao-Blackwellised filter end to end, and its state draw ---------------------------------------------------------------------------------------------
def _kalman_posterior(F, G, V, W, m0, C0, y):
    """The Kalman filter with the initial state AT the first observation -> (m_T, C_T)."""
    m, C = m0.copy(), C0.copy()
    for t, yt in enumerate(y):
        if t > 0:
            m, C = G @ m, G @ C @ G.T + W
        q = F @ C @ F + V
        k = C @ F / q
        m, C = m + k * (yt - F @ m), C - np.outer(k, k) * q
    return m, C


def test_rao_blackwell_forecast_is_the_kalman_forecast(eng):
    d, T, H, P, N = 2, 20, 5, 256, 16
    mod = Dlm.polynomial(d)
    W, V = np.diag([0.3, 0.05]), 0.8
    p = DlmParameters(np.array([[V]]), W, np.zeros(d), np.eye(d))
    rng = np.random.default_rng(66)
    x, y = np.linalg.cholesky(p.c0) @ rng.standard_normal(d), np.empty(T)
    F, G = mod.f(1.0)[:, 0], mod.g(1.0)
    for t in range(T):
        if t > 0:
            x = G @ x + np.sqrt(np.diag(W)) * rng.standard_normal(d)
        y[t] = F @ x + np.sqrt(V) * rng.standard_normal()
    times = np.arange(1.0, T + 1)
    known = [Gaussian(float(np.log(w)), 0.0) for w in np.diag(W)]
    out = RaoBlackwellFilter(P, 0.95).forecast(mod, (times, np.tile(y, (N, 1))), times[-1] + np.arange(1.0, H + 1), p, Gaussian(float(np.log(V)), 0.0),
                                               known, eng, seed=3, series_offset=1, return_draws=True)
    assert not out["status"].any() and not out["filter"]["status"].any() and out["draws"].shape == (N, H, P)
    mT, CT = _kalman_posterior(F, G, V, W, p.m0, p.c0, y)
    np.testing.assert_allclose(out["filter"]["mean"][0, -1], mT, rtol=1e-9)
    _, f, Q = api.forecast(mod, mT[None], CT[None], float(times[-1]), p, eng, H + 1)
    pooled = np.transpose(out["draws"], (1, 0, 2)).reshape(H, N * P)
    n = N * P
    for h in range(H):
        fh, Qh = f[0, h + 1, 0], Q[0, h + 1, 0, 0]
        z_mean = abs(pooled[h].mean() - fh) / np.sqrt(Qh / n)
        z_var = abs(pooled[h].var(ddof=1) - Qh) / (Qh * np.sqrt(2.0 / (n - 1)))
        print(f"step {h + 1}: f = {fh:.4f}, Q = {Qh:.4f}; the pooled draws' mean and variance are {z_mean:.2f} and {z_var:.2f} standard errors away")
        assert z_mean <= SIGMAS and z_var <= SIGMAS
    # the state draw itself: the filter's moments are every particle's, so the drawn states have them
    x0 = np.transpose(out["cloud0"], (1, 0, 2)).reshape(d, n)
    assert np.all(np.abs(x0.mean(axis=1) - mT) / np.sqrt(np.diag(CT) / n) <= SIGMAS)


@pytest.mark.parametrize("d", range(1, 17))
def test_state_draw_matches_the_restatement(eng, d):
    means, covs = lc.state_draw_case(d)
    ref, status = lr.state_draw(means, covs, slot=11, seed=8, series_offset=4, iteration=3)
    out = eng.rb_state_draw(means, covs, slot=11, seed=8, series_offset=4, iteration=3)
    assert not status.any() and not np.asarray(out["status"]).any() and eng.last_variant == "rb-state-draw"
    np.testing.assert_allclose(out["cloud"], ref, rtol=RTOL, atol=ATOL)


def test_state_draw_fails_a_series_with_a_bad_covariance_alone(eng):
    import torch
    means, covs = lc.state_draw_case(3, P=128, N=4)
    good = eng.rb_state_draw(means, covs, slot=0, seed=1)
    bad_covs = covs.copy()
    bad_covs[1, 2, 77] = -1.0          # C[1][1] of one particle
    bad_covs[3, 0, 5] = np.nan
    bad = eng.rb_state_draw(torch.as_tensor(means, device="cuda"), torch.as_tensor(bad_covs, device="cuda"), slot=0, seed=1)
    bad = {k: v.cpu().numpy() for k, v in bad.items()}
    assert bad["status"].tolist() == [0, _lib.ST_NOT_PD, 0, _lib.ST_NOT_PD]
    assert np.all(np.isnan(bad["cloud"][[1, 3]]))
    np.testing.assert_array_equal(bad["cloud"][[0, 2]], np.asarray(good["cloud"])[[0, 2]])
    # halves of the batch
    hi = eng.rb_state_draw(means[2:], covs[2:], slot=0, seed=1, series_offset=2)
    np.testing.assert_array_equal(np.asarray(hi["cloud"]), np.asarray(good["cloud"])[2:])


# ---- 7. the Liu-West and Storvik filters end to end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", [pr.GAUSSIAN, pr.STUDENTT, pr.BETA])
def test_liu_west_forecast_with_known_variances_is_the_particle_forecast(eng, family):
    base = Dlm.polynomial(1)
    mod = {pr.GAUSSIAN: Dglm.gaussian(base), pr.STUDENTT: Dglm.student_t(5.0, base), pr.BETA: Dglm.beta(base)}[family]
    V, W = pc.FAMILY_V[family], 0.02
    p = DlmParameters(np.array([[V]]), np.array([[W]]), np.zeros(1), np.array([[0.3]]))
    N, T, H, P = 4, 12, 4, 128
    rng = np.random.default_rng(70 + family)
    ys = np.array([mod.simulate_regular(p, T, rng=rng)[1] for _ in range(N)])
    train, test_times = (np.arange(1.0, T + 1), ys), T + np.array([0.5, 1.5, 1.5, 4.0])
    kw = dict(seed=6, iteration=1, series_offset=2)
    out = LiuAndWestFilter(P, 0.97).forecast(mod, train, test_times, p, Gaussian(float(np.log(V)), 0.0), Gaussian(float(np.log(W)), 0.0), eng,
                                             prob=0.9, return_draws=True, **kw)
    filt = out["filter"]
    assert not out["status"].any()
    np.testing.assert_allclose(filt["psi"][:, 0], np.log(W), rtol=1e-13)
    np.testing.assert_allclose(filt["psi"][:, 1], np.log(V), rtol=1e-13)
    pe = DlmParameters(np.array([[np.exp(filt["psi"][0, 1, 0])]]), np.array([[np.exp(filt["psi"][0, 0, 0])]]), p.m0, p.c0)
    hand = Dglm.forecast_particles(mod, filt["cloud"], pe, (test_times, np.full((N, H), np.nan)), eng, weights=filt["weights"], time0=float(T),
                                   slot_offset=T, prob=0.9, return_draws=True, **kw)
    for k in ("draws", "mean", "lower", "upper", "state_mean", "cloud"):
        np.testing.assert_allclose(out[k], hand[k], rtol=RTOL, atol=ATOL, err_msg=k)
    np.testing.assert_array_equal(out["time"], test_times)
    # the auxiliary filter forecasts through the same call: p's own variances, V shared
    aux = AuxFilter(P).forecast(mod, train, test_times, p, eng, prob=0.9, **kw)
    assert not aux["status"].any() and np.all(aux["var_v"] == V) and np.all(aux["lower"] <= aux["upper"])


@pytest.mark.parametrize("summary", ["mean", "median"])
def test_storvik_forecast_end_to_end(eng, summary):
    mod = Dglm.gaussian(Dlm.polynomial(2))
    p = DlmParameters(np.array([[0.5]]), np.diag([0.1, 0.01]), np.zeros(2), np.eye(2))
    N, T, H, P = 6, 30, 8, 256
    rng = np.random.default_rng(81)
    ys = np.array([mod.simulate_regular(p, T, rng=rng)[1] for _ in range(N)])
    out = StorvikFilter(P).forecast(mod, (np.arange(1.0, T + 1), ys), T + np.arange(1.0, H + 1), p, InverseGamma(3.0, 1.0), InverseGamma(3.0, 0.2), eng,
                                    seed=2, summary=summary, prob=0.9, return_draws=True)
    assert not out["status"].any() and not out["filter"]["status"].any()
    assert out[summary].shape == out["lower"].shape == out["upper"].shape == (N, H) and out["state_mean"].shape == (N, H, 2)
    assert out["draws"].shape == (N, H, P) and out["var_w"].shape == (N, 2, P) and out["var_v"].shape == (N, P) and out["cloud"].shape == (N, 2, P)
    assert all(np.all(np.isfinite(out[k])) for k in (summary, "lower", "upper", "state_mean", "draws", "var_w", "var_v", "cloud"))
    assert np.all(out["lower"] <= out[summary]) and np.all(out[summary] <= out["upper"]) and np.all(out["lower"] < out["upper"])
    assert np.all(out["var_w"] > 0.0) and np.all(out["var_v"] > 0.0) and np.ptp(out["var_v"], axis=1).min() > 0.0
    fn = Dglm.mean_and_intervals if summary == "mean" else Dglm.median_and_intervals
    centre, lower, upper = fn(0.9)(out["draws"][0].T)
    np.testing.assert_array_equal(lower, out["lower"][0])
    np.testing.assert_array_equal(upper, out["upper"][0])


# ---- 8. plumbing -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_halves_and_device_arrays_give_the_bits_of_the_whole(eng):
    kw, cloud, weights, pw, pv, shapes = lc.draws_case("studentt", "ig")          # N = 3, per-series nu and shapes
    run = lambda lo, hi, **k: lc.learned_run(eng, lc.series(kw, lo, hi), cloud[lo:hi], pw[lo:hi], pv[lo:hi], kind=_lib.FC_IG_SCALE, shapes=shapes[lo:hi],
                                             weights=weights[lo:hi], slot_offset=4, ranks=(0, 64, 127), **k)
    whole, lo, hi, dev = run(0, 3), run(0, 1), run(1, 3, device=True), run(0, 3, device=True)
    for k in KEYS:
        np.testing.assert_array_equal(whole[k], np.concatenate([lo[k], hi[k]]), err_msg=k)
        np.testing.assert_array_equal(whole[k], dev[k], err_msg=k)
    none = lc.learned_run(eng, kw, cloud, pw, pv, kind=_lib.FC_IG_SCALE, shapes=shapes, weights=weights, slot_offset=4, want_draws=False)
    assert none["draws"] is None and none["fquant"] is None
    np.testing.assert_array_equal(none["fmean"], whole["fmean"])


def test_poisoned_series_fail_alone(eng):
    kw, cloud, weights, pw, pv, shapes = lc.draws_case("gaussian", "ig")
    cloud, weights, pw, pv, shapes = (np.concatenate([a, a[:2]]) for a in (cloud, weights, pw, pv, shapes))          # N = 5
    kw = dict(kw, y=np.full((5, kw["y"].shape[1]), np.nan))
    run = lambda pw, weights, shapes: lc.learned_run(eng, kw, cloud, pw, pv, kind=_lib.FC_IG_SCALE, shapes=shapes, weights=weights, slot_offset=4, ranks=(0, 127))
    good = run(pw, weights, shapes)
    assert not good["status"].any()
    bad_pw, bad_w, bad_sh = pw.copy(), weights.copy(), shapes.copy()
    bad_pw[0, 1, 5] = np.nan          # a NaN variance
    bad_w[1, 7] = -0.5                # a negative weight
    bad_sh[3, 0] = 0.0                # a zero shape
    bad = run(bad_pw, bad_w, bad_sh)
    assert bad["status"].tolist() == [_lib.ST_NOT_PD, _lib.ST_NONFINITE, 0, _lib.ST_NOT_PD, 0]
    for n in (0, 1, 3):
        for k in ("fmean", "fquant", "draws", "mean", "var_w", "var_v"):
            assert np.all(np.isnan(bad[k][n])), (n, k)
    assert np.all(np.isnan(bad["cloud"][[0, 3]])) and np.all(np.isfinite(bad["cloud"][1]))
    for k in KEYS:
        np.testing.assert_array_equal(bad[k][[2, 4]], good[k][[2, 4]], err_msg=k)
    # a zero variance: a known, noiseless component of the state under FC_VAR, refused for the observation scale
    vw = np.abs(pw); vw[2, 0] = 0.0
    zero = lc.learned_run(eng, kw, cloud, vw, np.abs(pv), kind=_lib.FC_VAR, ranks=(0,))
    assert not zero["status"].any() and np.all(zero["var_w"][2, 0] == 0.0)
    zv = np.abs(pv); zv[4, 3] = 0.0
    assert lc.learned_run(eng, kw, cloud, vw, zv, kind=_lib.FC_VAR, ranks=(0,))["status"].tolist() == [0, 0, 0, 0, _lib.ST_NOT_PD]
    # a draw that is not finite stops the series at that step: a Beta variance above mean (1 - mean)
    kb, cb, wb, pwb, pvb, _ = lc.draws_case("beta", "var")
    pvb = pvb.copy(); pvb[1, 9] = 0.3
    late = lc.learned_run(eng, kb, cb, pwb, pvb, kind=_lib.FC_VAR, ranks=(0,))
    assert late["status"].tolist() == [0, _lib.ST_NONFINITE, 0] and np.all(np.isnan(late["fmean"][1])) and np.all(np.isfinite(late["var_v"][1]))


def test_argument_errors_return_their_codes_without_launching(eng):
    kw, cloud, weights, pw, pv, shapes = lc.draws_case("gaussian", "ig")
    N, d, P = cloud.shape
    H = kw["y"].shape[1]
    mat, par = pc.materialised(kw), pc.packed_params(kw, N)
    md, pd, op, keep = eng.prepare(mat, par, N, _Host())
    fmean, fquant = np.full((N, H), -7.0), np.full((N, H, 8), -7.0)
    ptr = _Host.ptr
    cloud, pw, pv, weights, shapes = (np.ascontiguousarray(a) for a in (cloud, pw, pv, weights, shapes))
    tv = _lib.ParamsDesc(pd.V, pd.v_stride, pd.W, pd.w_stride, pd.m0, pd.m0_stride, pd.C0, pd.c0_stride, 1, 0)          # a time-varying V

    def call(family=0, P=P, kind=_lib.FC_IG_SCALE, ranks=(0,), slot=0, c0=cloud, w=pw, v=pv, sh=shapes, stride=d + 1, fm=fmean, fq=fquant, n_ranks=None,
             params=pd):
        desc = _lib.PfForecastLearnedDesc(family, P, kind, len(ranks) if n_ranks is None else n_ranks, slot)
        rk = (ctypes.c_int32 * max(1, len(ranks)))(*ranks)
        return eng.lib.dlm_pf_forecast_learned(eng.h, md, params, ctypes.byref(desc), None, rk, ptr(c0), ptr(weights), ptr(w), ptr(v), ptr(sh), stride, 0, op,
                                               ptr(fm), ptr(fq), None, None, None, None, None, None)
    ARG, UNSUPPORTED = -1, -3
    assert call() == 0 and np.all(fmean != -7.0)          # (the call itself is sound)
    fmean[:] = -7.0
    for what, rc in ((dict(c0=None), ARG), (dict(w=None), ARG), (dict(sh=None), ARG), (dict(family=pr.NEGBIN, kind=_lib.FC_LOGVAR), ARG),
                     (dict(family=pr.ZIP, kind=_lib.FC_IG_SCALE), ARG), (dict(family=pr.ZIP, kind=_lib.FC_LOGVAR), ARG), (dict(n_ranks=9), ARG),
                     (dict(n_ranks=-1), ARG), (dict(ranks=(P,)), ARG), (dict(ranks=(0, -1)), ARG), (dict(fq=None), ARG), (dict(fm=None), ARG),
                     (dict(slot=-1), ARG), (dict(params=tv, v=None), ARG), (dict(kind=3), ARG), (dict(family=6), ARG), (dict(stride=d), ARG),
                     (dict(family=pr.STUDENTT), ARG), (dict(slot=_lib.PF_MAX_T - H + 1), UNSUPPORTED), (dict(P=96), UNSUPPORTED), (dict(P=2048), UNSUPPORTED)):
        assert call(**what) == rc, what
        assert len(eng.lib.dlm_last_error(eng.h)) >= 10          # and it says why
    assert np.all(fmean == -7.0)          # nothing ran
    assert call(family=pr.NEGBIN, kind=_lib.FC_VAR, slot=_lib.PF_MAX_T - H) == 0          # (the count families take pv as their v under FC_VAR)
    # the state draw's
    means, covs = lc.state_draw_case(2)
    out = np.full(means.shape, -7.0)
    draw = lambda d=2, N=3, P=64, m=means, c=covs, slot=0, o=out: eng.lib.dlm_rb_state_draw(eng.h, d, N, P, ptr(m), ptr(c), slot, 0, op, ptr(o), None)
    for what, rc in ((dict(m=None), ARG), (dict(c=None), ARG), (dict(o=None), ARG), (dict(slot=-1), ARG), (dict(slot=1 << 21), ARG), (dict(N=0), ARG),
                     (dict(d=17), UNSUPPORTED), (dict(P=96), UNSUPPORTED), (dict(P=2048), UNSUPPORTED)):
        assert draw(**what) == rc, what
    assert np.all(out == -7.0) and draw(slot=(1 << 21) - 1) == 0 and np.all(out != -7.0)


def test_async_call_is_complete_after_sync(eng):
    """DLM_OPT_ASYNC on device arrays: the call returns before the kernel has finished, the arrays it was given are held until sync(), and
    the results after sync() are the synchronous call's."""
    kw, cloud, weights, pw, pv, shapes = lc.draws_case("gaussian", "logvar")
    ref = lc.learned_run(eng, kw, cloud, pw, pv, kind=_lib.FC_LOGVAR, weights=weights, ranks=(0, 127), device=True)
    import torch
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    out = eng.pf_forecast_learned(pc.materialised(kw), pc.packed_params(kw, 3), dev(cloud), dev(pw), dev(pv), family=kw["family"], var_kind=_lib.FC_LOGVAR,
                                  weights=dev(weights), ranks=(0, 127), iteration=kw["iteration"], seed=kw["seed"], series_offset=kw["series_offset"],
                                  want_draws=True, flags=_lib.OPT_ASYNC)
    assert eng._keep
    eng.sync()
    assert eng._keep == []
    for k in KEYS:
        np.testing.assert_array_equal(out[k].cpu().numpy(), ref[k], err_msg=k)
