"""Every state dimension D = 1 .. 16 of the six particle kernels (k_pf, k_storvik, k_lw, k_rb, k_pg, k_pf_forecast) on the GPU: 96 code objects,
each launched here at least once, on tests/pf_dims_cases.model(d) -- a dense non-symmetric G, three of them through g_index, dt = 0 first and
inside the series, a time-varying F_t, one missing value, T = 8.

A    one launch per (kernel, d) against the kernel's restatement, held as that kernel's own test_kernel_matches_restatement holds it: status
     and ESS (k_pg: ancestors and path indices) EQUAL, everything else at rtol 1e-11 / atol 1e-12.  tests/test_pf_dims_host.py shows that no
     comparison of these inputs is within 1e-11 of flipping.
B    against the Kalman filter, which restates nothing of the kernels:
B.1  k_rb with known variances IS the Kalman filter of every series (rtol 1e-10, atol 1e-14: a factor of 10 and more above the float64
     recursion's own rounding, measured against long double in the host file), ESS = P;
B.2  k_pf and the auxiliary k_lw on 1024 replicas of one series: mean exp(ll_hat - ll_Kalman) within 5 of its standard errors of 1 with no ratio
     above 2 % of the sum; in the diffuse setting the replica-averaged filtering means within 5 standard errors of the Kalman means at every
     (t, k), which are at least 20 standard errors from the unweighted cloud's somewhere;
B.3  k_pf_forecast (a) from its own cloud IS k_pf with n0 = P + 1, bit for bit; (b) with every y missing its 16 384 draws of a step have the
     mean and the variance of N(F_t^T a_t, F_t^T R_t F_t + V) within 5 standard errors, and fmean is the fixed-order mean of the draws;
B.4  k_pg at d = 5, 9, 16: tests/pg_checks.py's Gaussian check (K = 3 sweeps of N = 4096 paths from an exact start, P = 64; means, variances and
     lag-one cross-covariances within 5 standard errors of the Kalman smoother's).

The host file rehearses B on the restatements and shows which bound each of seven misreadings of the model misses.  The figures seen on an
MI355X are in profiles/r30_notes.md."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pf_cases as pc  # noqa: E402
import pf_dims_cases as dc  # noqa: E402
import pff_cases as fc  # noqa: E402
import pff_restatement as fr  # noqa: E402
import pg_cases as gc  # noqa: E402
import pg_checks as ck  # noqa: E402
import rb_cases as rc  # noqa: E402

from bayesian_dlms_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-11, 1e-12


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _rel(a, b):
    ok = np.isfinite(b)
    return float((np.abs(a[ok] - b[ok]) / (np.abs(b[ok]) + ATOL / RTOL)).max()) if ok.any() else 0.0


# ---- A: every instantiation against its restatement ------------------------------------------------------------------------------------------
AD = [(k, d) for k in dc.KERNELS for d in dc.DIMS]


@pytest.mark.parametrize("kernel,d", AD, ids=[f"{k}-d{d}" for k, d in AD])
def test_kernel_matches_restatement_at_every_d(eng, kernel, d):
    ref = dc.a_reference(kernel, d)
    out = dc.a_engine(eng, kernel, d)
    assert eng.last_variant == dc.VARIANT[kernel]
    assert np.all(ref["status"] == 0)
    for k in dc.EQUAL[kernel]:
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    print(f"A {kernel} d = {d}: largest relative difference " + ", ".join(f"{k} {_rel(out[k], ref[k]):.2e}" for k in dc.CLOSE[kernel]))
    for k in dc.CLOSE[kernel]:
        np.testing.assert_allclose(out[k], ref[k], rtol=RTOL, atol=ATOL, err_msg=k)
    if kernel == "rb":
        np.testing.assert_array_equal(out["cov"], np.swapaxes(out["cov"], 2, 3))          # symmetric bit for bit
    if kernel == "pff":          # the mean and the order statistics are those of the draws the kernel itself wrote
        P = dc.a_args(kernel, d)["P"]
        np.testing.assert_array_equal(out["fquant"], np.sort(out["draws"], axis=2)[:, :, list(dc.RANKS(P))])
        for t in range(dc.T):
            np.testing.assert_array_equal(out["fmean"][:, t], fr.forecast_mean(out["draws"][:, t]))


# ---- B.1: k_rb with known variances is the Kalman filter ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", dc.DIMS)
def test_rb_with_known_variances_is_the_kalman_filter_of_every_series(eng, d):
    kw = dc.b1_args(d)
    out = rc.engine_run(eng, kw)
    assert eng.last_variant == "rb-wave"
    assert np.all(out["status"] == 0) and np.all(out["ess"] == kw["P"])
    worst = 0.0
    for n in range(dc.N_A):
        ms, Cs, ll = rc.kalman_moments(dc.series_of(kw, n))
        worst = max(worst, _kal(out["ll"][n], ll), _kal(out["mean"][n], ms), _kal(out["cov"][n], Cs))
        np.testing.assert_allclose(out["ll"][n], ll, rtol=rc.KNOWN_RTOL, atol=1e-14)
        np.testing.assert_allclose(out["mean"][n], ms, rtol=rc.KNOWN_RTOL, atol=1e-14)
        np.testing.assert_allclose(out["cov"][n], Cs, rtol=rc.KNOWN_RTOL, atol=1e-14)
    print(f"B.1 d = {d}: largest |k_rb - Kalman| as a share of the bound {worst:.2e}")


def _kal(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    return float((np.abs(got - ref) / (rc.KNOWN_RTOL * np.abs(ref) + 1e-14)).max())


# ---- B.2: k_pf and the auxiliary k_lw ---------------------------------------------------------------------------------------------------------
B2 = [(k, d) for k in ("pf", "lw") for d in dc.DIMS]


def _b2_run(eng, kernel, kw):
    out = pc.engine_run(eng, kw, "particle_filter" if kernel == "pf" else "lw_filter", device=True)
    assert eng.last_variant == dc.VARIANT[kernel]
    assert np.all(out["status"] == 0)
    return out


@pytest.mark.parametrize("kernel,d", B2, ids=[f"{k}-d{d}" for k, d in B2])
def test_likelihood_estimate_and_filtering_means_against_the_kalman_filter(eng, kernel, d):
    _, ll = dc.b2_exact(kernel, d, False)
    out = _b2_run(eng, kernel, dc.b2_args(kernel, d, False))
    m, se, top = dc.likelihood_figures(out["ll"], ll)
    print(f"B.2 {kernel} d = {d}: mean exp(ll_hat - ll) = {m:.4f} +- {se:.4f} ({(m - 1.0) / se:+.2f} se), top share {top:.4f}")
    assert dc.likelihood_misses(out["ll"], ll) == []
    out = _b2_run(eng, kernel, dc.b2_args(kernel, d, True))
    z, sep = dc.means_figures(kernel, d, True, out["mean"])
    print(f"B.2 {kernel} d = {d}, diffuse: largest |mean - Kalman| = {z:.2f} se; Kalman - unweighted cloud up to {sep:.1f} se")
    assert dc.means_misses(kernel, d, True, out["mean"]) == []


# ---- B.3: k_pf_forecast ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", dc.DIMS)
def test_forecast_from_its_own_cloud_is_the_filter_bit_for_bit(eng, d):
    kw = dc.b2_args("pf", d, False)
    kw = dict(kw, n0=kw["P"] + 1)
    whole = pc.engine_run(eng, kw, device=True)
    assert eng.last_variant == "pf-wave"
    own = fc.forecast_run(eng, kw, device=True)
    assert eng.last_variant == "pf-forecast-wave"
    assert not whole["status"].any()
    for k in ("ll", "mean", "cloud", "weights", "status"):
        np.testing.assert_array_equal(own[k], whole[k], err_msg=k)
    assert np.all(np.isfinite(own["fmean"]))


@pytest.mark.parametrize("d", dc.DIMS)
def test_pure_forecast_draws_follow_the_kalman_prediction_law(eng, d):
    out = fc.forecast_run(eng, dc.b3_args(d), want_draws=True, device=True)
    assert eng.last_variant == "pf-forecast-wave"
    assert not out["status"].any() and out["draws"].shape == (dc.PURE_N, dc.T, dc.PURE_P)
    zm, zv = dc.draws_figures(d, out["draws"])
    print(f"B.3b d = {d}: largest z over t: mean {zm.max():.2f}, variance {zv.max():.2f}")
    assert dc.draws_misses(d, out["draws"]) == []
    for t in range(dc.T):
        np.testing.assert_array_equal(out["fmean"][:, t], fr.forecast_mean(out["draws"][:, t]))


# ---- B.4: k_pg against the Kalman smoother ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", dc.PG_DIMS)
def test_gaussian_paths_keep_the_kalman_smoother_s_moments_on_the_dense_model(eng, d):
    c = dc.pg_case(d)
    path = c["start"]
    assert max(dc.smoother_z(d, path)) <= ck.SIGMAS          # the start IS a sample of the law: the yardstick sees it as one
    for k in range(ck.K):
        out = gc.engine_run(eng, dict(c["kw"], ref=path, iteration=k), device=True, traces=False)
        assert eng.last_variant == "pg-wave"
        assert np.all(out["status"] == 0)
        path = out["path"]
    assert not np.array_equal(path, c["start"])
    z = dc.smoother_z(d, path)
    print(f"B.4 d = {d} after {ck.K} sweeps, worst in standard errors: means {z[0]:.2f}, variances {z[1]:.2f}, lag-one cross-covariances {z[2]:.2f}")
    assert max(z) <= ck.SIGMAS, z
