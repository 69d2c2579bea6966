"""dlm_lw_batch on the GPU (LiuAndWestFilter.step, and with a = 1 and known variances AuxFilter.step).

The kernel is held to its NumPy restatement (tests/lw_restatement.py) on the table of tests/lw_cases.py at the tolerance of
tests/test_pf_gpu.py: the arithmetic is restated operation for operation and in the kernel's orders of summation, so what remains is the last
bits of log, exp, cos, sin and lgamma.  The ESS must be EQUAL, and so must, in effect, the ancestors of both stages: one that went the other
way leaves a final cloud that differs in the first digit.  tests/test_lw_host.py shows that no comparison of the kernel's is within 1e-11 of
flipping on these inputs.  Then: the batch does not depend on how it is split; the three statistical checks of the host test on the
engine's output; the bad series; the refusals; the Python drivers.

The largest relative difference seen on an MI355X is in profiles/r21_notes.md."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lw_cases as lc  # noqa: E402
import lw_restatement as lr  # noqa: E402
import pf_cases as pc  # noqa: E402
import storvik_cases as sc  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dglm import AuxFilter, Dglm, LiuAndWestFilter, ParticleFilter, materialise_pf  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters  # noqa: E402
from bayesian_dlms_amd.engine import Engine, EngineError  # noqa: E402
from bayesian_dlms_amd.stochvol import Gaussian  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-11, 1e-12
KEYS = ("ll", "mean", "ess", "psi_mean", "psi_var", "cloud", "weights", "psi")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _rel(a, b):
    ok = np.isfinite(b)
    return float((np.abs(a[ok] - b[ok]) / (np.abs(b[ok]) + ATOL / RTOL)).max()) if ok.any() else 0.0


# ---- kernel against restatement ---------------------------------------------------------------------------------------------------------
RUNS = [(c["name"], False) for c in lc.TABLE] + [(n, True) for n in lc.DEVICE_RUNS]


@pytest.mark.parametrize("name,device", RUNS, ids=[n + ("-device" if dev else "") for n, dev in RUNS])
def test_kernel_matches_restatement(eng, name, device):
    ref = lc.reference(name)
    out = lc.engine_run(eng, lc.run_args(name), device=device)
    assert eng.last_variant == "lw-wave"
    print(f"{name}: largest relative difference " + ", ".join(f"{k} {_rel(out[k], ref[k]):.2e}" for k in KEYS))
    np.testing.assert_array_equal(out["status"], ref["status"])
    np.testing.assert_array_equal(out["ess"], ref["ess"])
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
    kw = lc.run_args("n67-per-series")
    whole = lc.engine_run(eng, kw)
    again = lc.engine_run(eng, kw)
    lo, hi = lc.engine_run(eng, _slice(kw, 0, 34)), lc.engine_run(eng, _slice(kw, 34, 67), device=True)
    for k in KEYS + ("status",):
        np.testing.assert_array_equal(whole[k], again[k], err_msg=k)          # the same iteration: the same bits
        np.testing.assert_array_equal(whole[k], np.concatenate([lo[k], hi[k]]), err_msg=k)
    other = lc.engine_run(eng, dict(kw, iteration=kw["iteration"] + 1))
    assert np.all(other["ll"] != whole["ll"])          # another iteration: other draws for every series


# ---- the three statistical checks on the engine's output -------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["level", "dense"])
@pytest.mark.parametrize("diffuse", [False, True], ids=["v1", "v500"])
def test_known_parameters_the_likelihood_estimate_is_unbiased_and_literal_is_not(eng, which, diffuse):
    ll = lc.known_exact(which, diffuse)
    out = lc.engine_run(eng, lc.known_args(which, diffuse), device=True)
    m, se = pc.unbiasedness(out["ll"], ll)
    print(f"{which}, V = {500 if diffuse else 1}: mean exp(ll - log L) = {m:.5f} +- {se:.5f}")
    assert np.all(out["status"] == 0) and abs(m - 1.0) <= lc.SIGMAS * se
    lit = lc.engine_run(eng, lc.known_args(which, diffuse, literal=True), device=True)
    ml, sel = pc.unbiasedness(lit["ll"], ll)
    print(f"{which}, V = {500 if diffuse else 1}, literal: mean exp(ll - log L) = {ml:.3e} +- {sel:.3e}")
    assert abs(ml - 1.0) > lc.SIGMAS * sel


@pytest.mark.parametrize("which", ["level", "dense"])
def test_static_cloud_the_evidence_estimate_is_unbiased(eng, which):
    log_z, _, _ = lc.exact(which, lc.STATIC_SD, lc.STATIC_T)
    out = lc.engine_run(eng, lc.learn_args(which, lc.STATIC_SD, lc.STATIC_T, lc.REPLICATES), device=True)
    m, se, top = sc.unbiasedness(out["ll"], log_z)
    print(f"{which}, a = 1, sd {lc.STATIC_SD}, T {lc.STATIC_T}: mean exp(ll - log Z) = {m:.5f} +- {se:.5f} (largest ratio {top:.1f})")
    assert np.all(out["status"] == 0) and se <= lc.STATIC_SE_MAX and abs(m - 1.0) <= lc.SIGMAS * se


@pytest.mark.parametrize("which", ["level", "dense"])
def test_learning_the_posterior_means_of_the_log_variances(eng, which):
    _, grid, _ = lc.exact(which, lc.LEARN_SD, lc.LEARN_T)
    kw = lc.learn_args(which, lc.LEARN_SD, lc.LEARN_T, lc.LEARN_REPLICATES, a=lc.LEARN_A, P=lc.LEARN_P)
    fm = lc.final_log_means(lc.engine_run(eng, kw, device=True), which)
    mean, se = fm.mean(axis=0), fm.std(axis=0, ddof=1) / np.sqrt(fm.shape[0])
    dev, bound = np.abs(mean - np.asarray(grid)), lc.learn_bound(which, se)
    print(f"{which}, a = {lc.LEARN_A}: means {mean} against the grid's {grid}: deviation {dev}, standard errors {se}, bound {bound}")
    assert np.all(dev <= bound)
    lit = lc.final_log_means(lc.engine_run(eng, dict(kw, literal=True), device=True), which)
    print(f"literal (reported, not asserted): deviation {np.abs(lit.mean(axis=0) - np.asarray(grid))}")


# ---- status -------------------------------------------------------------------------------------------------------------------------------
def test_a_failing_series_fails_alone(eng):
    kw = lc.run_args("p128-d2-missing-per-series")
    C0 = kw["C0"].copy(); C0[3] = -C0[3]
    pw = kw["prior_w"].copy(); pw[1, 1, 1] = -0.25          # a negative prior sd
    good = lc.engine_run(eng, kw)
    out = lc.engine_run(eng, dict(kw, C0=C0, prior_w=pw))
    assert out["status"].tolist() == [0, _lib.ST_NOT_PD, 0, _lib.ST_NOT_PD, 0]
    assert np.all(out["ll"][[1, 3]] == -np.inf)
    for k in ("mean", "ess", "psi_mean", "psi_var", "cloud", "weights", "psi"):
        assert np.all(np.isnan(out[k][[1, 3]])), k
    for k in KEYS:
        np.testing.assert_array_equal(out[k][[0, 2, 4]], good[k][[0, 2, 4]], err_msg=k)
    pv = kw["prior_v"].copy(); pv[0, 0] = np.nan          # a prior mean that is NaN
    out = lc.engine_run(eng, dict(kw, prior_v=pv))
    assert out["status"].tolist() == [_lib.ST_NOT_PD, 0, 0, 0, 0] and out["ll"][0] == -np.inf
    for k in KEYS:
        np.testing.assert_array_equal(out[k][1:], good[k][1:], err_msg=k)


def test_a_beta_series_with_y_outside_the_unit_interval_fails_alone(eng):
    kw = lc.run_args("learnv0-beta")
    y = kw["y"].copy(); y[1, 5] = 1.5
    bad, good = lc.engine_run(eng, dict(kw, y=y)), lc.engine_run(eng, kw)
    assert bad["status"].tolist() == [0, _lib.ST_NONFINITE, 0] and bad["ll"][1] == -np.inf
    assert np.all(np.isfinite(bad["mean"][1, :5])) and np.all(np.isnan(bad["mean"][1, 5:])) and np.all(np.isnan(bad["psi_mean"][1, 5:]))
    for k in KEYS:
        np.testing.assert_array_equal(np.delete(bad[k], 1, axis=0), np.delete(good[k], 1, axis=0), err_msg=k)
    ref = lr.run(**dict(kw, y=y))
    for k in KEYS:
        np.testing.assert_allclose(bad[k], ref[k], rtol=RTOL, atol=ATOL, err_msg=k)


def test_engine_refuses_what_it_does_not_cover(eng):
    from bayesian_dlms_amd.engine import _Host
    kw = lc.run_args("p64-d1")
    mat, par = pc.materialised(kw), pc.packed_params(kw, 5)
    with pytest.raises(EngineError, match="positive scale"):
        eng.lw_filter(mat, par, kw["y"], kw["prior_w"], family=_lib.OBS_POISSON, n_particles=64, a=0.9, prior_v=kw["prior_v"], learn_v=True)
    # straight at the C ABI: the code and a message, no launch
    y = np.ascontiguousarray(kw["y"])
    md, pd, op, keep = eng.prepare(mat, par, 5, _Host())
    ll = np.empty(5)
    pw16, pv = np.tile([0.0, 0.5], (16, 1)), np.array([0.0, 0.5])

    def call(desc):
        return eng.lib.dlm_lw_batch(eng.h, md, pd, ctypes.byref(desc), _Host.ptr(pv), 0, _Host.ptr(pw16), 0, None, _Host.ptr(y), 0, op,
                                    _Host.ptr(ll), None, None, None, None, None, None, None, None)
    err = lambda: eng.lib.dlm_last_error(eng.h)
    for fam in (_lib.OBS_POISSON, _lib.OBS_NEGBIN, _lib.OBS_ZIP):
        assert call(_lib.LwDesc(fam, 64, -1, 0, 1, 0.9)) == -1 and b"positive scale" in err()          # DLM_ERR_ARG
    for a in (0.0, -0.1, 1.5, float("nan")):
        assert call(_lib.LwDesc(0, 64, -1, 0, 1, a)) == -1 and b"0 < a <= 1" in err()
    assert call(_lib.LwDesc(6, 64, -1, 0, 0, 0.9)) == -1 and call(_lib.LwDesc(0, 64, -1, 2, 1, 0.9)) == -1 and call(_lib.LwDesc(0, 64, -1, 0, 2, 0.9)) == -1
    md.d = 16
    assert call(_lib.LwDesc(0, 1024, -1, 0, 1, 0.9)) == -3 and b"LDS" in err()          # DLM_ERR_UNSUPPORTED: d = 16, P = 1024
    md.d = 9
    assert call(_lib.LwDesc(0, 1024, -1, 0, 1, 0.9)) == -3 and b"LDS" in err()
    md.d, md.p = 1, 2
    assert call(_lib.LwDesc(0, 64, -1, 0, 1, 0.9)) == -3 and b"p = 1" in err()
    md.p = 1
    for P in (96, 2048):
        assert call(_lib.LwDesc(0, P, -1, 0, 1, 0.9)) == -3
    assert call(_lib.LwDesc(0, 64, -1, 0, 1, 1.0)) == 0 and np.all(np.isfinite(ll))          # and the same call inside the limits runs


def test_the_largest_holdings_run(eng):
    """d = 8 with P = 1024 and d = 16 with P = 512: the two largest shapes lw_lds_bytes grants inside 160 KB."""
    for d, P in ((8, 1024), (16, 512)):
        rng = np.random.default_rng(d)
        G0, Wfull, F = pc.dense_model(d, rng)
        T, N = 3, 2
        kw = dict(F=F, G=G0[None], g_index=None, dt=np.array([0.0, 1.0, 1.0]), V=0.05, W=np.diag(np.diag(Wfull)), m0=np.zeros(d), C0=np.eye(d),
                  y=0.3 * rng.standard_normal((N, T)), nu=None, prior_w=np.stack([np.log(np.diag(Wfull)), np.full(d, 0.5)], axis=1),
                  prior_v=np.array([np.log(0.05), 0.5]), family=0, learn_v=True, P=P, a=0.95, n0=-1, literal=False, seed=3, series_offset=0,
                  iteration=0)
        out, ref = lc.engine_run(eng, kw), lr.run(**kw)
        np.testing.assert_array_equal(out["ess"], ref["ess"])
        for k in KEYS:
            np.testing.assert_allclose(out[k], ref[k], rtol=RTOL, atol=ATOL, err_msg=f"d = {d}, P = {P}: {k}")


# ---- the drivers --------------------------------------------------------------------------------------------------------------------------
def test_liu_west_and_aux_filters_equal_the_raw_engine_call(eng):
    rng = np.random.default_rng(8)
    T, N, n = 14, 3, 128
    times = np.concatenate([[1.0, 2.0, 4.0], np.arange(5.0, T + 2.0)])          # one step of 2
    y = np.cumsum(np.sqrt(0.3) * rng.standard_normal((N, T)), axis=1) + rng.standard_normal((N, T))
    y[1, 4] = np.nan
    mod = Dglm.student_t(5.0, Dlm.polynomial(2))
    p = DlmParameters(np.eye(1), np.diag([0.3, 0.05]), np.array([0.1, 0.0]), np.eye(2))
    prior_v, prior_w = Gaussian(0.1, 0.4), [Gaussian(-1.0, 0.5), Gaussian(-3.0, 0.0)]
    out = LiuAndWestFilter(n, 0.97, 40).filter(mod, (times, y), p, prior_v, prior_w, eng, seed=5, iteration=2, series_offset=9)
    mat = materialise_pf(mod, times)
    raw = eng.lw_filter(mat, p, y, np.array([[-1.0, 0.5], [-3.0, 0.0]]), family=_lib.OBS_STUDENTT, n_particles=n, a=0.97,
                        prior_v=np.array([0.1, 0.4]), learn_v=True, n0=40, obs_param=5.0, iteration=2, seed=5, series_offset=9)
    for k in KEYS + ("status",):
        np.testing.assert_array_equal(out[k], np.asarray(raw[k]), err_msg=k)
    assert eng.last_variant == "lw-wave" and np.all(out["status"] == 0)
    moments = np.exp(out["psi_mean"] + out["psi_var"] / 2.0)
    np.testing.assert_array_equal(out["w_mean"], moments[:, :, :2])
    np.testing.assert_array_equal(out["v_mean"], moments[:, :, 2])
    assert np.all(out["psi"][:, 1] == -3.0) and np.all(np.isfinite(out["v_mean"]))
    # a family whose v is no scale learns W alone
    cnt = LiuAndWestFilter(n, 0.97).filter(Dglm.poisson(Dlm.polynomial(2)), (times, np.round(np.exp(0.3 * y))), p, None, prior_w[0], eng, seed=5)
    assert np.all(cnt["status"] == 0) and np.all(np.isnan(cnt["v_mean"])) and np.all(np.isnan(cnt["psi"][:, 2])) and np.all(np.isfinite(cnt["ll"]))
    # AuxFilter: a = 1, sd = 0, means log diag(W), V from p
    gm = Dglm.gaussian(Dlm.polynomial(2))
    aux = AuxFilter(n, 40).filter(gm, (times, y), p, eng, seed=5, iteration=2, series_offset=9)
    raw = eng.lw_filter(mat, p, y, np.array([[np.log(0.3), 0.0], [np.log(0.05), 0.0]]), family=_lib.OBS_GAUSSIAN, n_particles=n, a=1.0,
                        learn_v=False, n0=40, iteration=2, seed=5, series_offset=9)
    for k in KEYS + ("status",):
        np.testing.assert_array_equal(aux[k], np.asarray(raw[k]), err_msg=k)
    np.testing.assert_array_equal(AuxFilter(n, 40).likelihood(gm, (times, y), p, eng, seed=5, iteration=2, series_offset=9), aux["ll"])


def test_aux_likelihood_can_stand_in_for_the_particle_filter_s(eng):
    """Both estimates of the Kalman likelihood of pf_cases' dense model (with the diagonal of its W) are within SIGMAS standard errors."""
    a = lc.known_inputs("dense", False)
    exact = lc.known_exact("dense", False)
    mod = Dglm.gaussian(Dlm(lambda t: a["F"][:, None], lambda s: a["G"][0]))
    p = DlmParameters(np.array([[a["V"]]]), a["W"], a["m0"], a["C0"])
    times = np.arange(1.0, a["y"].shape[1] + 1.0)
    for name, ll in (("AuxFilter", AuxFilter(128).likelihood(mod, (times, a["y"]), p, eng, seed=4)),
                     ("ParticleFilter", ParticleFilter.likelihood(mod, (times, a["y"]), 128, p, eng, seed=4))):
        m, se = pc.unbiasedness(ll, exact)
        print(f"{name}: mean exp(ll - log L) = {m:.5f} +- {se:.5f}")
        assert ll.shape == (lc.REPLICATES,) and abs(m - 1.0) <= lc.SIGMAS * se
