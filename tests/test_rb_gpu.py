"""dlm_rb_batch on the GPU (RaoBlackwellFilter.scala: the Liu-West filter with the state integrated out).

The kernel is held to its NumPy restatement (tests/rb_restatement.py) on the table of tests/rb_cases.py at the tolerance of
tests/test_lw_gpu.py: the arithmetic is restated operation for operation and in the kernel's orders of summation, so what remains is the last
bits of log, exp, cos and sin.  The ESS must be EQUAL, and so must, in effect, the ancestors of both stages.  tests/test_rb_host.py shows that
no comparison of the kernel's is within 1e-11 of flipping on these inputs.  Then: the two largest holdings; the batch does not depend on how it
is split; the three statistical checks of the host test on the engine's output, the first against Engine.loglik and Engine.filter on the
device; the bad series; every argument code; the Python driver."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lw_cases as lc  # noqa: E402
import pf_cases as pc  # noqa: E402
import rb_cases as rc  # noqa: E402
import rb_restatement as rr  # noqa: E402
import storvik_cases as sc  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dglm import Dglm, RaoBlackwellFilter, materialise_pf  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters  # noqa: E402
from bayesian_dlms_amd.engine import Engine, EngineError  # noqa: E402
from bayesian_dlms_amd.stochvol import Gaussian  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-11, 1e-12
KEYS = ("ll", "mean", "cov", "ess", "psi_mean", "psi_var", "means", "covs", "weights", "psi")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _rel(a, b):
    ok = np.isfinite(b)
    return float((np.abs(a[ok] - b[ok]) / (np.abs(b[ok]) + ATOL / RTOL)).max()) if ok.any() else 0.0


def _compare(out, ref, what):
    np.testing.assert_array_equal(out["status"], ref["status"], err_msg=what)
    np.testing.assert_array_equal(out["ess"], ref["ess"], err_msg=what)
    for k in KEYS:
        np.testing.assert_allclose(out[k], ref[k], rtol=RTOL, atol=ATOL, err_msg=f"{what}: {k}")


# ---- kernel against restatement ---------------------------------------------------------------------------------------------------------
RUNS = [(c["name"], False) for c in rc.TABLE] + [(n, True) for n in rc.DEVICE_RUNS]


@pytest.mark.parametrize("name,device", RUNS, ids=[n + ("-device" if dev else "") for n, dev in RUNS])
def test_kernel_matches_restatement(eng, name, device):
    ref = rc.reference(name)
    out = rc.engine_run(eng, rc.run_args(name), device=device)
    assert eng.last_variant == "rb-wave"
    print(f"{name}: largest relative difference " + ", ".join(f"{k} {_rel(out[k], ref[k]):.2e}" for k in KEYS))
    _compare(out, ref, name)
    np.testing.assert_array_equal(out["cov"], np.swapaxes(out["cov"], 2, 3))          # symmetric bit for bit


def test_the_largest_holdings_run(eng):
    """d = 16 with P = 64 and d = 3 with P = 1024: the largest P at d = 16 and the largest d at P = 1024 that rb_lds_bytes grants inside 160 KB."""
    for d, P in ((16, 64), (3, 1024)):
        rng = np.random.default_rng(d)
        G0, Wfull, F = pc.dense_model(d, rng)
        T, N = 2, 2
        kw = dict(F=F, G=G0[None], g_index=None, dt=np.array([0.0, 1.0]), V=0.05, W=np.diag(np.diag(Wfull)), m0=np.zeros(d), C0=np.eye(d),
                  y=0.3 * rng.standard_normal((N, T)), prior_w=np.stack([np.log(np.diag(Wfull)), np.full(d, 0.5)], axis=1),
                  prior_v=np.array([np.log(0.05), 0.5]), learn_v=True, P=P, a=0.95, n0=P + 1, literal=False, seed=3, series_offset=0, iteration=0)
        _compare(rc.engine_run(eng, kw), rr.run(**kw), f"d = {d}, P = {P}")


# ---- the batch does not depend on how it is split ---------------------------------------------------------------------------------------
def _slice(kw, lo, hi):
    """Series lo .. hi - 1 of a batch with per-series m0, C0 and priors, as a batch of its own."""
    cut = dict(kw, y=kw["y"][lo:hi], series_offset=kw["series_offset"] + lo, V=kw["V"][lo:hi])
    for k in ("m0", "C0", "prior_w", "prior_v"):
        cut[k] = kw[k][lo:hi]
    return cut


def test_halves_with_series_offset_equal_the_whole_batch(eng):
    kw = rc.run_args("n67-per-series")
    whole = rc.engine_run(eng, kw)
    again = rc.engine_run(eng, kw)
    lo, hi = rc.engine_run(eng, _slice(kw, 0, 34)), rc.engine_run(eng, _slice(kw, 34, 67), device=True)
    for k in KEYS + ("status",):
        np.testing.assert_array_equal(whole[k], again[k], err_msg=k)          # the same iteration: the same bits
        np.testing.assert_array_equal(whole[k], np.concatenate([lo[k], hi[k]]), err_msg=k)
    other = rc.engine_run(eng, dict(kw, iteration=kw["iteration"] + 1))
    assert np.all(other["ll"] != whole["ll"])          # another iteration: other draws for every series


# ---- check 1 on the engine's output, against the engine's own Kalman filter on the device ---------------------------------------------------
@pytest.mark.parametrize("which", rc.KNOWN_MODELS)
@pytest.mark.parametrize("a", [1.0, 0.9])
def test_known_variances_are_the_kalman_filter(eng, which, a):
    import torch
    ms, Cs, ll = rc.known_exact(which)
    kw0 = rc.known_args(which)
    mat, par = pc.materialised(kw0), pc.packed_params(kw0, 1)
    d, T = mat.d, mat.T
    y1 = torch.as_tensor(kw0["y"][:1].reshape(1, T, 1), device="cuda")
    dev_ll = eng.loglik(mat, par, y1)["loglik"].cpu().numpy()[0]
    filt = eng.filter(mat, par, y1)["filt"].cpu().numpy()[0]          # [T+1][d + d*d], record 0 the initial state
    dev_m, dev_C = filt[1:, :d], filt[1:, d:].reshape(T, d, d)
    np.testing.assert_allclose(dev_ll, ll, rtol=rc.KNOWN_RTOL)
    for seed, P in ((11, 64), (12, 128)):
        out = rc.engine_run(eng, rc.known_args(which, a=a, P=P, seed=seed), device=True)
        assert np.all(out["status"] == 0) and np.all(out["ess"] == P)
        np.testing.assert_allclose(out["ll"], dev_ll, rtol=rc.KNOWN_RTOL)
        for n in range(out["ll"].size):
            np.testing.assert_allclose(out["mean"][n], dev_m, rtol=rc.KNOWN_RTOL, atol=1e-14)
            np.testing.assert_allclose(out["cov"][n], dev_C, rtol=rc.KNOWN_RTOL, atol=1e-14)
            np.testing.assert_allclose(out["mean"][n], ms, rtol=rc.KNOWN_RTOL, atol=1e-14)
            np.testing.assert_allclose(out["cov"][n], Cs, rtol=rc.KNOWN_RTOL, atol=1e-14)
    lit = rc.engine_run(eng, rc.known_args(which, a=a, literal=True), device=True)
    print(f"{which}, a = {a}, literal: ll - Kalman = {lit['ll'][0] - ll:+.4f}")
    assert abs(lit["ll"][0] - ll) > 1e-3 * abs(ll)


# ---- checks 2 and 3 on the engine's output ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["level", "dense"])
def test_static_cloud_the_evidence_estimate_is_unbiased_and_tighter_than_liu_west(eng, which):
    log_z, _, _ = lc.exact(which, lc.STATIC_SD, lc.STATIC_T)
    out = rc.engine_run(eng, rc.learn_args(which, lc.STATIC_SD, lc.STATIC_T, lc.REPLICATES), device=True)
    m, se, top = sc.unbiasedness(out["ll"], log_z)
    share = top / np.exp(out["ll"] - log_z).sum()
    lw = lc.engine_run(eng, lc.learn_args(which, lc.STATIC_SD, lc.STATIC_T, lc.REPLICATES), device=True)
    _, se_lw, _ = sc.unbiasedness(lw["ll"], log_z)
    print(f"{which}, a = 1, sd {lc.STATIC_SD}, T {lc.STATIC_T}: mean exp(ll - log Z) = {m:.5f} +- {se:.5f}, largest ratio {share:.5f} of the sum; "
          f"Liu-West's standard error {se_lw:.5f}, {se_lw / se:.2f} times this one")
    assert np.all(out["status"] == 0) and abs(m - 1.0) <= rc.SIGMAS * se
    assert share < rc.TOP_SHARE
    assert se <= se_lw / rc.SE_FACTOR


@pytest.mark.parametrize("which", ["level", "dense"])
def test_learning_the_posterior_means_of_the_log_variances(eng, which):
    _, grid, _ = lc.exact(which, lc.LEARN_SD, lc.LEARN_T)
    kw = rc.learn_args(which, lc.LEARN_SD, lc.LEARN_T, lc.LEARN_REPLICATES, a=lc.LEARN_A, P=lc.LEARN_P)
    fm = lc.final_log_means(rc.engine_run(eng, kw, device=True), which)
    mean, se = fm.mean(axis=0), fm.std(axis=0, ddof=1) / np.sqrt(fm.shape[0])
    dev, bound = np.abs(mean - np.asarray(grid)), rc.learn_bound(which, se)
    print(f"{which}, a = {lc.LEARN_A}: means {mean} against the grid's {grid}: deviation {dev}, standard errors {se}, bound {bound}")
    assert np.all(dev <= bound)
    lit = lc.final_log_means(rc.engine_run(eng, dict(kw, literal=True), device=True), which)
    print(f"literal (reported, not asserted): deviation {np.abs(lit.mean(axis=0) - np.asarray(grid))}")


# ---- status -------------------------------------------------------------------------------------------------------------------------------
def test_failing_series_fail_alone_with_both_status_bits(eng):
    kw = rc.run_args("p128-d2-missing-per-series")
    pw = kw["prior_w"].copy(); pw[1, 1, 1] = -0.25          # a negative prior sd: DLM_ST_NOT_PD before any step
    pw[4, 0, 0] = 800.0                                     # exp overflows: a Q that is not finite, DLM_ST_NONFINITE
    C0 = kw["C0"].copy(); C0[2] = -40.0 * C0[2]             # a Q that is not positive where C0 is first used: DLM_ST_NOT_PD at t = 1
    bad_kw = dict(kw, prior_w=pw, C0=C0)
    good, out, ref = rc.engine_run(eng, kw), rc.engine_run(eng, bad_kw), rr.run(**bad_kw)
    assert out["status"].tolist() == [0, _lib.ST_NOT_PD, _lib.ST_NOT_PD, 0, _lib.ST_NONFINITE]
    assert np.all(out["ll"][[1, 2, 4]] == -np.inf)
    for k in KEYS[1:]:
        assert np.all(np.isnan(out[k][1])), k
    assert np.all(np.isfinite(out["mean"][2, 0])) and np.all(np.isnan(out["mean"][2, 1:])) and np.all(np.isnan(out["cov"][4, 1:]))
    for k in ("means", "covs", "weights", "psi"):
        assert np.all(np.isnan(out[k][[1, 2, 4]])), k
    for k in KEYS:
        np.testing.assert_array_equal(out[k][[0, 3]], good[k][[0, 3]], err_msg=k)          # the neighbours: bit for bit a clean run's
    _compare(out, ref, "bad series")


def test_engine_refuses_what_it_does_not_cover(eng):
    from bayesian_dlms_amd.engine import _Host
    kw = rc.run_args("p64-d1")
    mat, par = pc.materialised(kw), pc.packed_params(kw, 5)
    # straight at the C ABI: the code and a message, no launch
    y = np.ascontiguousarray(kw["y"])
    md, pd, op, keep = eng.prepare(mat, par, 5, _Host())
    ll = np.empty(5)
    pw16, pv = np.tile([0.0, 0.5], (16, 1)), np.array([0.0, 0.5])

    def call(desc, pv=pv, pw=pw16, yy=y, out=ll, pv_stride=0, pw_stride=0):
        p = lambda a: None if a is None else _Host.ptr(a)
        return eng.lib.dlm_rb_batch(eng.h, md, pd, ctypes.byref(desc), p(pv), pv_stride, p(pw), pw_stride, p(yy), 0, op, p(out), *([None] * 10))
    err = lambda: eng.lib.dlm_last_error(eng.h)
    for a in (0.0, -0.1, 1.5, float("nan")):
        assert call(_lib.RbDesc(64, -1, 0, 1, a)) == -1 and b"0 < a <= 1" in err()          # DLM_ERR_ARG
    assert call(_lib.RbDesc(64, -1, 2, 1, 0.9)) == -1 and b"literal" in err()
    assert call(_lib.RbDesc(64, -1, 0, 2, 0.9)) == -1 and b"learn_v" in err()
    assert call(_lib.RbDesc(64, -1, 0, 1, 0.9), pv=None) == -1 and b"prior_v" in err()
    assert call(_lib.RbDesc(64, -1, 0, 1, 0.9), pw=None) == -1 and b"prior_w" in err()
    assert call(_lib.RbDesc(64, -1, 0, 1, 0.9), pv_stride=1) == -1 and call(_lib.RbDesc(64, -1, 0, 1, 0.9), pw_stride=1) == -1
    assert call(_lib.RbDesc(64, -1, 0, 1, 0.9), yy=None) == -1 and call(_lib.RbDesc(64, -1, 0, 1, 0.9), out=None) == -1
    assert eng.lib.dlm_rb_batch(eng.h, md, pd, None, None, 0, None, 0, None, 0, op, *([None] * 11)) == -1
    for d, P in ((16, 128), (13, 128), (9, 320), (4, 1024)):          # DLM_ERR_UNSUPPORTED: beyond the LDS
        md.d = d
        assert call(_lib.RbDesc(P, -1, 0, 1, 0.9)) == -3 and b"LDS" in err(), (d, P)
    md.d, md.p = 1, 2
    assert call(_lib.RbDesc(64, -1, 0, 1, 0.9)) == -3 and b"p = 1" in err()
    md.p = 1
    for P in (96, 2048, 0):
        assert call(_lib.RbDesc(P, -1, 0, 1, 0.9)) == -3
    assert call(_lib.RbDesc(64, -1, 0, 1, 1.0)) == 0 and np.all(np.isfinite(ll))          # and the same call inside the limits runs
    # the Python layer says the same before anything is staged
    with pytest.raises(EngineError, match="covariance in LDS"):
        eng.rb_filter(pc.materialised(rc.run_args("d16-p64")), pc.packed_params(rc.run_args("d16-p64"), 2), rc.run_args("d16-p64")["y"],
                      rc.run_args("d16-p64")["prior_w"], n_particles=128, a=0.9, prior_v=[0.0, 0.5])


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
def test_rao_blackwell_filter_equals_the_raw_engine_call(eng):
    rng = np.random.default_rng(8)
    T, N, n = 14, 3, 128
    times = np.concatenate([[1.0, 2.0, 4.0], np.arange(5.0, T + 2.0)])          # one step of 2
    y = np.cumsum(np.sqrt(0.3) * rng.standard_normal((N, T)), axis=1) + rng.standard_normal((N, T))
    y[1, 4] = np.nan
    dlm = Dlm.polynomial(2)
    p = DlmParameters(np.eye(1), np.diag([0.3, 0.05]), np.array([0.1, 0.0]), np.eye(2))
    prior_v, prior_w = Gaussian(0.1, 0.4), [Gaussian(-1.0, 0.5), Gaussian(-3.0, 0.0)]
    out = RaoBlackwellFilter(n, 0.97, 126).filter(dlm, (times, y), p, prior_v, prior_w, eng, seed=5, iteration=2, series_offset=9)
    mat = materialise_pf(dlm, times)
    raw = eng.rb_filter(mat, p, y, np.array([[-1.0, 0.5], [-3.0, 0.0]]), n_particles=n, a=0.97, prior_v=np.array([0.1, 0.4]), learn_v=True,
                        n0=126, iteration=2, seed=5, series_offset=9)
    for k in KEYS + ("status",):
        np.testing.assert_array_equal(out[k], np.asarray(raw[k]), err_msg=k)
    assert eng.last_variant == "rb-wave" and np.all(out["status"] == 0)
    moments = np.exp(out["psi_mean"] + out["psi_var"] / 2.0)
    np.testing.assert_array_equal(out["w_mean"], moments[:, :, :2])
    np.testing.assert_array_equal(out["v_mean"], moments[:, :, 2])
    assert np.all(out["psi"][:, 1] == -3.0) and np.all(np.isfinite(out["v_mean"]))
    # a Gaussian Dglm is the same model; V known: p.v is read, the entries of V are NaN
    same = RaoBlackwellFilter(n, 0.97, 126).filter(Dglm.gaussian(dlm), (times, y), p, prior_v, prior_w, eng, seed=5, iteration=2, series_offset=9)
    for k in KEYS + ("status",):
        np.testing.assert_array_equal(same[k], out[k], err_msg=k)
    known = RaoBlackwellFilter(n, 0.97).filter(dlm, (times, y), p, None, prior_w, eng, learn_v=False, seed=5)
    assert np.all(known["status"] == 0) and np.all(np.isnan(known["v_mean"])) and np.all(np.isnan(known["psi"][:, 2])) and np.all(np.isfinite(known["ll"]))
