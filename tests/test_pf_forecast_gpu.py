"""dlm_pf_forecast_particles on the device (bayesian_dlms_amd/csrc/dlm_pf_forecast.hip, dlm_obs_draws.h).

  the filter inside the forecast IS dlm_pf_batch: a filter over 12 steps against a filter over the first 5 and a forecast over the other 7
    from its cloud -- per-step means and the final cloud bit for bit, ll within H_total 2^-52 max|partial sum| (the split changes only the
    order of H_total additions); and the forecast from its own initial cloud against the whole filter, ll included, bit for bit;
  the order statistics are those of the draws (np.sort), the mean is the restatement's fixed-order sum of them, bit for bit, and neither
    depends on whether the draws are written;
  the draws against the restatement: continuous families within the RTOL / ATOL of tests/test_pf_gpu.py, discrete ones EQUAL wherever the
    restated margin exceeds 1e-9, at most 1 draw in 10^4 excused;  the laws of the device's own draws (chi-square / KS, p > 1e-4);
  the exact predictive of a d = 1 model on pf_grid_reference's grid: means within 4.5 standard errors (from the 64 replicas), the exact
    predictive cdf at the replica-averaged median within 4.5 binomial standard errors of 0.5;
  plumbing: split batches, device arrays, poisoned series, the argument errors;  ParticleFilter.forecast end to end."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pf_cases as pc  # noqa: E402
import pf_restatement as pr  # noqa: E402
import pff_cases as fc  # noqa: E402
import pff_restatement as fr  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dglm import Dglm, ParticleFilter  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters  # noqa: E402
from bayesian_dlms_amd.engine import Engine, _Host  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-11, 1e-12          # tests/test_pf_gpu.py's
SIGMAS = 4.5
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


# ---- 4. the filter inside the forecast --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.SPLIT_NAMES)
def test_filter_then_forecast_is_the_filter(eng, name):
    kw = fc.case_args(name)
    T1, H = fc.T1, fc.H_TOTAL
    whole = pc.engine_run(eng, kw)
    first = pc.engine_run(eng, fc.steps(kw, 0, T1))
    rest = fc.forecast_run(eng, fc.steps(kw, T1, H), cloud=first["cloud"], slot_offset=T1)
    assert eng.last_variant == "pf-forecast-wave"
    assert not whole["status"].any() and not first["status"].any() and not rest["status"].any()
    np.testing.assert_array_equal(first["mean"], whole["mean"][:, :T1])
    np.testing.assert_array_equal(rest["mean"], whole["mean"][:, T1:])
    np.testing.assert_array_equal(rest["cloud"], whole["cloud"])
    np.testing.assert_array_equal(rest["weights"], whole["weights"])
    # ll: the same H_total terms, added in another order.  ll_first and ll are partial sums of the whole run and ll_forecast is one of the
    # forecast's, so the largest of the three is at most the max |partial sum| the bound speaks of
    scale = np.maximum(np.abs(whole["ll"]), np.maximum(np.abs(first["ll"]), np.abs(rest["ll"])))
    err = np.abs((first["ll"] + rest["ll"]) - whole["ll"])
    print(f"{name}: |ll_first + ll_forecast - ll| <= {err.max():.2e}, bound {(H * EPS * scale).min():.2e}")
    assert np.all(err <= H * EPS * scale)
    # from its own initial cloud the forecast is the filter, ll included
    own = fc.forecast_run(eng, kw)
    for k in ("ll", "mean", "cloud", "weights", "status"):
        np.testing.assert_array_equal(own[k], whole[k], err_msg=k)
    assert np.all(np.isfinite(own["fmean"]))


def test_weighted_entry_cloud_is_resampled_once(eng):
    """A filter that never resamples (n0 = 0) hands over a weighted cloud.  The forecast resamples it once at entry: the running sums in
    the kernel's order, the uniforms of block 9 of the first forecast slot, the search -- restated here with pf_restatement's functions; from
    the cloud so resampled, unweighted, the forecast has the same bits."""
    kw = fc.steps(fc.case_args("split-gaussian"), 0, fc.T1)
    first = pc.engine_run(eng, dict(kw, n0=0))
    assert np.ptp(first["weights"], axis=1).min() > 0.0
    rest = fc.steps(fc.case_args("split-gaussian"), fc.T1, fc.H_TOTAL)
    N, P = rest["y"].shape[0], rest["P"]
    a = fc.forecast_run(eng, rest, cloud=first["cloud"], weights=first["weights"], slot_offset=fc.T1, ranks=(0, P - 1), want_draws=True)
    cum = pr.running_sums(first["weights"])
    series = np.uint64(rest["series_offset"]) + np.arange(N, dtype=np.uint64)
    _, u2 = pr.batch_rand(pr.KEY_PF | fr.BLOCK_RESAMPLE0, rest["seed"], series, rest["iteration"], fc.T1, P)
    picked = np.empty_like(first["cloud"])
    for n in range(N):
        anc = np.minimum(np.searchsorted(np.maximum.accumulate(cum[n]), u2[n] * cum[n, P - 1], side="right"), P - 1)
        picked[n] = first["cloud"][n][:, anc]
    assert any(len(np.unique(picked[n, 0])) < P for n in range(N))          # (a resampling: some particle was taken twice)
    b = fc.forecast_run(eng, rest, cloud=picked, slot_offset=fc.T1, ranks=(0, P - 1), want_draws=True)
    assert not a["status"].any() and not b["status"].any()
    for k in ("fmean", "fquant", "draws", "ll", "mean", "cloud", "weights"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # weights that are negative, or sum to nothing, stop their series alone
    bad = first["weights"].copy(); bad[1, 3] = -0.25; bad[2] = 0.0
    c = fc.forecast_run(eng, rest, cloud=first["cloud"], weights=bad, slot_offset=fc.T1, ranks=(0,))
    assert c["status"].tolist() == [0, _lib.ST_NONFINITE, _lib.ST_NONFINITE] and np.all(np.isnan(c["fmean"][1:])) and np.all(np.isnan(c["fquant"][1:]))
    np.testing.assert_array_equal(c["fmean"][0], a["fmean"][0])


# ---- 5. order statistics and mean ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.ORDER_NAMES)
def test_order_statistics_and_mean_are_those_of_the_draws(eng, name):
    kw = fc.case_args(name, "ORDER")
    P = kw["P"]
    ranks = fc.order_ranks(P)
    out = fc.forecast_run(eng, kw, ranks=ranks, want_draws=True)
    assert not out["status"].any() and out["draws"].shape == kw["y"].shape + (P,)
    srt = np.sort(out["draws"], axis=2)
    np.testing.assert_array_equal(out["fquant"], srt[:, :, list(ranks)])
    if kw["family"] == pr.POISSON:
        assert max(len(np.unique(row)) for row in out["draws"].reshape(-1, P)) < P          # ties in every row
    for h in range(kw["y"].shape[1]):
        np.testing.assert_array_equal(out["fmean"][:, h], fr.forecast_mean(out["draws"][:, h]))
    bare = fc.forecast_run(eng, kw, ranks=ranks)
    assert bare["draws"] is None
    for k in ("fmean", "fquant", "ll", "mean", "cloud"):
        np.testing.assert_array_equal(bare[k], out[k], err_msg=k)
    none = fc.forecast_run(eng, kw)          # no ranks: no sort, the same mean
    assert none["fquant"] is None
    np.testing.assert_array_equal(none["fmean"], out["fmean"])


# ---- 6. the draws against the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.POINT_NAMES)
def test_kernel_draws_match_the_restatement(eng, name):
    p = fc.point_by_name(name)
    N, P, H = 4, 256, 4
    ref = fc.degenerate_reference(name, N, P, H)
    out = fc.forecast_run(eng, fc.degenerate_args(p, N, P, H), want_draws=True)
    assert not out["status"].any()
    if p["family"] in fc.DISCRETE:
        held = ref["margin"] > fc.MARGIN
        excused = 1.0 - held.mean()
        differ = int((out["draws"] != ref["draws"]).sum())
        print(f"{name}: {differ} of {held.size} draws differ, {int((~held).sum())} excused")
        assert excused <= fc.EXCUSED_SHARE
        np.testing.assert_array_equal(out["draws"][held], ref["draws"][held])
    else:
        rel = np.abs(out["draws"] - ref["draws"]) / (np.abs(ref["draws"]) + ATOL / RTOL)
        print(f"{name}: largest relative difference {rel.max():.2e}")
        np.testing.assert_allclose(out["draws"], ref["draws"], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(out["fmean"], ref["fmean"], rtol=RTOL, atol=ATOL)


# ---- 7. the laws on the device -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.DEVICE_LAW_NAMES)
def test_device_draws_have_the_right_law(eng, name):
    p = fc.point_by_name(name)
    out = fc.forecast_run(eng, fc.degenerate_args(p, 16, 1024, 4), want_draws=True, device=True)
    assert not out["status"].any()
    pv = fc.law_pvalue(p, out["draws"])
    print(f"{name}: p-value {pv:.4f} over {out['draws'].size} draws")
    assert out["draws"].size == fc.LAW_DRAWS and pv > fc.P_VALUE


# ---- 8. the exact predictive ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(fc.PRED_FAMILIES))
def test_forecast_matches_the_exact_predictive(eng, which):
    """64 replicas of one series (they differ in the series index of their Philox streams), P = 1024, steps 0 .. 2 observed and 3 .. 5 not.
    Mean: the replica average of fmean[h] within 4.5 of ITS standard errors of the grid's predictive mean.  Median: the exact predictive cdf F
    at the replica average q of the median order statistic within tol = 4.5 sqrt(0.25 / (64 * 1024)) of 0.5.  For the counts F is a step
    function and q lies between two of its steps unless every replica agrees: there 0.5 has to lie in the jump that q straddles,
    F(ceil(q) - 1) - tol <= 0.5 <= F(floor(q)) + tol fails for a legitimate q, F(floor(q) - 1) - tol < 0.5 <= F(ceil(q)) + tol is the
    statement that the medians sit on the exact median or on its neighbour."""
    kw = fc.predictive_args(which)
    means, cdf = fc.predictive_exact(which)
    P, N = fc.PRED_P, fc.PRED_N
    out = fc.forecast_run(eng, kw, ranks=(P // 2,), device=True)
    assert not out["status"].any()
    avg, se = out["fmean"].mean(axis=0), out["fmean"].std(axis=0, ddof=1) / np.sqrt(N)
    z = np.abs(avg - means) / se
    print(f"{which}: |mean - exact| in standard errors {np.round(z, 2).tolist()}")
    assert np.all(z <= SIGMAS)
    q = out["fquant"][:, :, 0].mean(axis=0)
    tol = SIGMAS * np.sqrt(0.25 / (N * P))
    for h in range(fc.PRED_H):
        if kw["family"] == pr.POISSON:
            below, above = float(cdf(h, np.floor(q[h]) - 1.0)[0]), float(cdf(h, np.ceil(q[h]))[0])
            print(f"{which} step {h}: averaged median {q[h]:.3f}, F just below {below:.4f}, F at it {above:.4f}")
            assert below - tol < 0.5 <= above + tol
        else:
            at = float(cdf(h, q[h])[0])
            print(f"{which} step {h}: F(averaged median) - 0.5 = {at - 0.5:+.5f}, tol {tol:.5f}")
            assert abs(at - 0.5) <= tol


# ---- 9. plumbing -------------------------------------------------------------------------------------------------------------------------------------
KEYS = ("fmean", "fquant", "draws", "ll", "mean", "cloud", "weights", "status")


def test_halves_and_device_arrays_give_the_bits_of_the_whole(eng):
    kw = fc.case_args("split-poisson-missing")
    kw = dict(kw, y=np.tile(kw["y"], (3, 1)))          # N = 9
    ranks = (0, 96, 191)
    whole = fc.forecast_run(eng, kw, ranks=ranks, want_draws=True)
    lo, hi = fc.forecast_run(eng, fc.series(kw, 0, 4), ranks=ranks, want_draws=True), fc.forecast_run(eng, fc.series(kw, 4, 9), ranks=ranks, want_draws=True, device=True)
    dev = fc.forecast_run(eng, kw, ranks=ranks, want_draws=True, device=True)
    for k in KEYS:
        np.testing.assert_array_equal(whole[k], np.concatenate([lo[k], hi[k]]), err_msg=k)
        np.testing.assert_array_equal(whole[k], dev[k], err_msg=k)
    # a continuation from a cloud, on device arrays
    first = pc.engine_run(eng, fc.steps(kw, 0, fc.T1))
    rest = fc.steps(kw, fc.T1, fc.H_TOTAL)
    a = fc.forecast_run(eng, rest, cloud=first["cloud"], weights=first["weights"], slot_offset=fc.T1, ranks=ranks)
    b = fc.forecast_run(eng, rest, cloud=first["cloud"], weights=first["weights"], slot_offset=fc.T1, ranks=ranks, device=True)
    for k in ("fmean", "fquant", "ll", "mean", "cloud"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_poisoned_series_fail_alone(eng):
    kw = fc.case_args("split-beta")          # d = 1, P = 64, N = 3 -> 5 series with per-series V and W
    N = 5
    y = np.tile(kw["y"][:1], (N, 1))
    W = np.tile(kw["W"][None], (N, 1, 1)); V = np.full(N, kw["V"])
    good = fc.forecast_run(eng, dict(kw, y=y, W=W, V=V), ranks=(0, 32, 63), want_draws=True)
    assert not good["status"].any()
    Wb, Vb = W.copy(), V.copy()
    Wb[2] = -1.0          # not positive definite
    Vb[3] = 0.3           # above mean (1 - mean) <= 0.25: alpha <= 0 for every particle (Q41)
    bad = fc.forecast_run(eng, dict(kw, y=y, W=Wb, V=Vb), ranks=(0, 32, 63), want_draws=True)
    assert bad["status"].tolist() == [0, 0, _lib.ST_NOT_PD, _lib.ST_NONFINITE, 0]
    for n in (2, 3):
        assert bad["ll"][n] == -np.inf
        for k in ("fmean", "fquant", "draws", "mean", "weights"):
            assert np.all(np.isnan(bad[k][n])), (n, k)
    assert np.all(np.isnan(bad["cloud"][2])) and np.all(np.isfinite(bad["cloud"][3]))
    for k in KEYS:
        np.testing.assert_array_equal(np.delete(bad[k], (2, 3), axis=0), np.delete(good[k], (2, 3), axis=0), err_msg=k)
    # a variance that fails LATER: a Beta draw needs alpha > 0 at every particle, and series 1 (V = 0.2: |eta| < 0.96 or so) loses that once
    # its cloud, tight at first, has spread; the restatement says at which step
    late_kw = dict(kw, y=np.full_like(y, np.nan), W=W * 2.0, V=np.where(np.arange(N) == 1, 0.2, V), C0=kw["C0"] * 1e-4)
    sim = fr.simulate(**{k: late_kw[k] for k in ("F", "G", "g_index", "dt", "m0", "C0", "family", "P", "seed", "iteration")}, V=0.2, W=kw["W"] * 2.0,
                      H=y.shape[1], N=1, series_offset=kw["series_offset"] + 1)
    t = int(np.isnan(sim["draws"][0]).any(axis=1).argmax())
    assert 1 <= t < y.shape[1]
    late = fc.forecast_run(eng, late_kw, ranks=(0,), want_draws=True)
    assert late["status"].tolist() == [0, _lib.ST_NONFINITE, 0, 0, 0]
    assert np.all(np.isfinite(late["fmean"][1, :t])) and np.all(np.isnan(late["fmean"][1, t:])) and np.all(np.isnan(late["draws"][1, t:]))
    assert np.all(np.isfinite(late["mean"][1, :t])) and np.all(np.isnan(late["mean"][1, t:])) and np.all(np.isnan(late["fquant"][1, t:]))


def test_argument_errors_return_their_codes_without_launching(eng):
    kw = fc.case_args("split-poisson")
    N, H, P = kw["y"].shape[0], kw["y"].shape[1], kw["P"]
    mat, par = pc.materialised(kw), pc.packed_params(kw, N)
    y = np.ascontiguousarray(kw["y"])
    md, pd, op, keep = eng.prepare(mat, par, N, _Host())
    fmean, fquant, ll = np.full((N, H), -7.0), np.full((N, H, 8), -7.0), np.full(N, -7.0)
    cloud0, w0 = np.zeros((N, mat.d, P)), np.full((N, P), 1.0 / P)
    ptr = _Host.ptr

    def call(family=1, P=P, literal=0, ranks=(0,), slot=0, cloud=None, weights=None, fm=fmean, fq=fquant, n_ranks=None):
        desc = _lib.PfForecastDesc(family, P, literal, len(ranks) if n_ranks is None else n_ranks, slot)
        rk = (ctypes.c_int32 * max(1, len(ranks)))(*ranks)
        return eng.lib.dlm_pf_forecast_particles(eng.h, md, pd, ctypes.byref(desc), None, rk, ptr(cloud), ptr(weights), ptr(y), 0, op,
                                                 ptr(fm), ptr(fq), None, ptr(ll), None, None, None, None)
    ARG, UNSUPPORTED = -1, -3
    assert call() == 0 and np.all(fmean != -7.0)          # (the call itself is sound)
    fmean[:], ll[:] = -7.0, -7.0
    for what, rc in ((dict(n_ranks=9), ARG), (dict(n_ranks=-1), ARG), (dict(ranks=(P,)), ARG), (dict(ranks=(0, -1)), ARG), (dict(family=6), ARG),
                     (dict(family=-1), ARG), (dict(literal=2), ARG), (dict(weights=w0), ARG), (dict(fm=None), ARG), (dict(fq=None), ARG),
                     (dict(slot=-1), ARG), (dict(slot=_lib.PF_MAX_T - H + 1), UNSUPPORTED), (dict(P=96), UNSUPPORTED), (dict(P=2048), UNSUPPORTED)):
        assert call(**what) == rc, what
        assert len(eng.lib.dlm_last_error(eng.h)) >= 10          # and it says why
    assert np.all(fmean == -7.0) and np.all(ll == -7.0)          # nothing ran
    assert call(slot=_lib.PF_MAX_T - H, cloud=cloud0, weights=w0) == 0


# ---- 10. end to end -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("summary", ["mean", "median"])
def test_particle_filter_forecast_end_to_end(eng, summary):
    mod = Dglm.poisson(Dlm.polynomial(1))
    p = DlmParameters(np.array([[1.0]]), np.array([[0.01]]), np.array([1.5]), np.array([[0.5]]))
    N, n_train, n_test = 8, 40, 10
    rng = np.random.default_rng(12)
    times, ys = None, []
    for _ in range(N):
        times, y, _ = mod.simulate_regular(p, n_train + n_test, rng=rng)
        ys.append(y)
    ys = np.array(ys)
    train, test = (times[:n_train], ys[:, :n_train]), (times[n_train:], np.full((N, n_test), np.nan))
    pf = ParticleFilter(256)
    kw = dict(seed=5, iteration=2, series_offset=9)
    out = pf.forecast(mod, train, test, p, eng, prob=0.9, summary=summary, return_draws=True, **kw)
    assert not out["status"].any() and out["draws"].shape == (N, n_test, 256)
    assert np.all(out["lower"] <= out[summary]) and np.all(out[summary] <= out["upper"]) and np.all(out["lower"] < out["upper"])
    np.testing.assert_array_equal(out["time"], times[n_train:])
    # composed by hand
    filt = pf.filter(mod, train, p, eng, **kw)
    hand = Dglm.forecast_particles(mod, filt["cloud"], p, test, eng, weights=filt["weights"], time0=times[n_train - 1], slot_offset=n_train,
                                   prob=0.9, summary=summary, return_draws=True, **kw)
    for k in ("time", summary, "lower", "upper", "state_mean", "ll", "cloud", "status", "draws"):
        np.testing.assert_array_equal(out[k], hand[k], err_msg=k)
    # the summaries are the host functions' of the draws
    fn = Dglm.mean_and_intervals if summary == "mean" else Dglm.median_and_intervals
    for n in (0, N - 1):
        centre, lower, upper = fn(0.9)(out["draws"][n].T)
        np.testing.assert_array_equal(lower, out["lower"][n])
        np.testing.assert_array_equal(upper, out["upper"][n])
        if summary == "median":
            np.testing.assert_array_equal(centre, out["median"][n])
        else:
            np.testing.assert_allclose(centre, out["mean"][n], rtol=1e-13)          # (the host adds the draws in order, the kernel in its own)
    # the data lie inside the 80 % band about as often as they should: not a test of the filter, a guard against a band of the wrong scale
    inside = ((ys[:, n_train:] >= out["lower"]) & (ys[:, n_train:] <= out["upper"])).mean()
    print(f"{summary}: {inside:.2f} of the held-out counts inside the band")
    assert 0.5 <= inside <= 1.0
