"""Every state dimension of the particle kernels, without a GPU: what tests/test_pf_dims_gpu.py asks of the kernels is asked here of their
restatements first, and the inputs of tests/pf_dims_cases.py are shown to be worth running.

A   for every (kernel, d): the restatement runs clean and none of its data-dependent comparisons is within 1e-11 of flipping (the margins of
    tests/test_pf_host.py, test_storvik_host.py, test_lw_host.py, test_rb_host.py; 1e-8 for k_pg as tests/test_pg_host.py); over the sweep of d
    both branches of the resampling test are taken.  (k_rb's look-ahead leaves the second stage's weights nearly even: tests/rb_cases.py says
    why n0 = -1 never resamples there, and reaches that branch with entries of its own.  Its share is printed, and asserted to be 0.)
B.1 k_rb's restatement with known variances against the Kalman filter at every d, and the float64 Kalman recursion against the same recursion
    in np.longdouble: the test's bound (rtol 1e-10, atol 1e-14) has to stand a factor of 10 above the recursion's own rounding.
B.2 the likelihood estimate and the filtering means of k_pf's restatement at all sixteen d; the auxiliary k_lw's at d = 2, 5, 9, 16 only (all
    sixteen take it another minute and a half, and this file beyond three; they were run once, and hold: profiles/r30_notes.md).
B.3 (b) the pure forecast's draws against the Kalman prediction law at every d.
B.4 `smoother` against the joint Gaussian law written out densely; the exact start passes the check it is the start of.
Then the mutants: each misreading of tests/pf_dims_cases.MUTANTS, put into the restatement's inputs at d = 2, 5, 9, 16, has to miss a bound of
B.3 (b) or B.2 (k_pf); which one is printed.  The figures are in profiles/r30_notes.md."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lw_restatement as lr  # noqa: E402
import pf_dims_cases as dc  # noqa: E402
import pf_restatement as pr  # noqa: E402
import pff_restatement as fr  # noqa: E402
import rb_cases as rc  # noqa: E402
import rb_restatement as rr  # noqa: E402

MARGIN, MARGIN_INT, MARGIN_PG = 1e-11, 1e-9, 1e-8
REHEARSED = (2, 5, 9, 16)
AD = [(k, d) for k in dc.KERNELS for d in dc.DIMS]


def test_model_is_the_one_the_tests_speak_of():
    for d in dc.DIMS:
        m = dc.model(d)
        assert m["G"].shape == (3, d, d) and m["F"].shape == (dc.T, d) and sorted(set(m["g_index"].tolist())) == [0, 1, 2]
        assert m["dt"][0] == 0.0 and m["dt"][dc.T // 2] == 0.0 and np.count_nonzero(m["dt"] == 0.0) == 2
        assert np.all(m["G"] != 0.0) and np.all(m["W"] != 0.0) and np.all(np.ptp(m["F"], axis=0) > 0.0)
        if d > 1:
            assert not np.allclose(m["G"][0], m["G"][0].T) and not np.allclose(m["G"][0], m["G"][1])
        for k in dc.KERNELS:
            a = dc.a_args(k, d)
            assert np.isnan(a["y"]).sum(axis=0).tolist() == [dc.N_A * (t == dc.MISSING) for t in range(dc.T)]
            assert a["V"].shape == (dc.N_A,) and a["W"].shape == a["C0"].shape == (dc.N_A, d, d) and a["m0"].shape == (dc.N_A, d)
            assert a["P"] == (64 if k == "rb" and d >= 13 else 128)
            diagonal = np.all(a["W"][:, ~np.eye(d, dtype=bool)] == 0.0)
            assert diagonal == (k in ("storvik", "lw", "rb") or d == 1)


# ---- A ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,d", AD, ids=[f"{k}-d{d}" for k, d in AD])
def test_part_a_entry_runs_with_margins(kernel, d):
    r = dc.a_reference(kernel, d)
    assert np.all(r["status"] == 0) and np.all(np.isfinite(r["ll"]))
    figures = {k: r[k] for k in ("resample_share", "margin_search", "margin_n0", "margin_int", "margin_accept", "margin_v") if k in r}
    print(f"{kernel} d = {d}: " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    assert r["margin_search"] >= (MARGIN_PG if kernel == "pg" else MARGIN)          # (an entry that fails: another seed in SEED_OF, not another bound)
    if kernel != "pg":
        assert r["margin_n0"] >= MARGIN and r["margin_int"] >= MARGIN_INT
    if kernel == "storvik":
        assert r["margin_accept"] >= MARGIN and r["margin_v"] >= MARGIN
    if kernel == "pff":
        assert r["resample_share"] == 1.0 and np.all(np.isfinite(r["draws"]))


@pytest.mark.parametrize("kernel", ["pf", "storvik", "lw", "rb"])
def test_part_a_takes_both_branches_of_the_resampling_test_in_the_sweep(kernel):
    share = np.array([dc.a_reference(kernel, d)["resample_share"] for d in dc.DIMS])
    print(f"{kernel}: share of observed steps that resampled, d = 1 .. 16: " + " ".join(f"{s:.2f}" for s in share))
    if kernel == "rb":          # the look-ahead evens the second stage's weights: floor(P / 5) is never reached (tests/rb_cases.py)
        assert np.all(share == 0.0)
    else:
        assert np.all(share > 0.0) and np.all(share < 1.0)


# ---- B.1 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", dc.DIMS)
def test_rb_restatement_with_known_variances_is_the_kalman_filter(d):
    kw = dc.b1_args(d)
    r = rr.run(**kw)
    assert np.all(r["status"] == 0) and np.all(r["ess"][~np.isnan(kw["y"])] == kw["P"])
    worst = 0.0
    for n in range(dc.N_A):
        a = dc.series_of(kw, n)
        ms, Cs, ll = rc.kalman_moments(a)
        np.testing.assert_allclose(r["ll"][n], ll, rtol=rc.KNOWN_RTOL, atol=1e-14)
        np.testing.assert_allclose(r["mean"][n], ms, rtol=rc.KNOWN_RTOL, atol=1e-14)
        np.testing.assert_allclose(r["cov"][n], Cs, rtol=rc.KNOWN_RTOL, atol=1e-14)
        # the recursion's own rounding, as a share of the bound
        lm, lC, lll = dc.kalman_moments_long(a)
        for got, ref in ((ms, lm), (Cs, lC), (np.float64(ll), lll)):
            ref = np.asarray(ref)
            worst = max(worst, float((np.abs(got - ref) / (rc.KNOWN_RTOL * np.abs(ref) + 1e-14)).max()))
    print(f"d = {d}: float64 Kalman recursion against long double: {worst:.2e} of the bound")
    assert worst <= 0.1


# ---- B.2 -------------------------------------------------------------------------------------------------------------------------------------
B2 = [("pf", d) for d in dc.DIMS] + [("lw", d) for d in REHEARSED]


def _run(kernel, kw):
    return (pr.run if kernel == "pf" else lr.run)(**kw)


@pytest.mark.parametrize("kernel,d", B2, ids=[f"{k}-d{d}" for k, d in B2])
def test_likelihood_estimate_and_filtering_means_against_the_kalman_filter(kernel, d):
    _, ll = dc.b2_exact(kernel, d, False)
    r = _run(kernel, dc.b2_args(kernel, d, False))
    m, se, top = dc.likelihood_figures(r["ll"], ll)
    print(f"{kernel} d = {d}: mean exp(ll_hat - ll) = {m:.4f} +- {se:.4f} ({(m - 1.0) / se:+.2f} se), top share {top:.4f}, "
          f"share of steps resampled {r['resample_share']:.2f}")
    assert np.all(r["status"] == 0)
    assert dc.likelihood_misses(r["ll"], ll) == []
    r = _run(kernel, dc.b2_args(kernel, d, True))
    z, sep = dc.means_figures(kernel, d, True, r["mean"])
    print(f"{kernel} d = {d}, diffuse: largest |mean - Kalman| = {z:.2f} se; Kalman - unweighted cloud up to {sep:.1f} se")
    assert np.all(r["status"] == 0)
    assert dc.means_misses(kernel, d, True, r["mean"]) == []


# ---- B.3 (b) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", dc.DIMS)
def test_pure_forecast_draws_follow_the_kalman_prediction_law(d):
    sim = fr.simulate(**dc.simulate_args(dc.b3_args(d)))
    zm, zv = dc.draws_figures(d, sim["draws"])
    print(f"d = {d}: largest z over t: mean {zm.max():.2f}, variance {zv.max():.2f}")
    assert sim["draws"].shape == (dc.PURE_N, dc.T, dc.PURE_P) and dc.draws_misses(d, sim["draws"]) == []


# ---- the mutants -----------------------------------------------------------------------------------------------------------------------------
MD = [(m, d) for m in dc.MUTANTS for d in REHEARSED]


@pytest.mark.parametrize("mutant,d", MD, ids=[f"{m}-d{d}" for m, d in MD])
def test_a_misread_model_misses_a_bound(mutant, d):
    """The restatement under one misreading, the Kalman reference under the true inputs: first the pure forecast (B.3 b), then, if that holds,
    k_pf's likelihood estimate and filtering means (B.2)."""
    misses = ["B.3b " + s for s in dc.draws_misses(d, fr.simulate(**dc.simulate_args(dc.b3_args(d, mutant)))["draws"])]
    if not misses:
        _, ll = dc.b2_exact("pf", d, False)
        misses += ["B.2 likelihood " + s for s in dc.likelihood_misses(pr.run(**dc.b2_args("pf", d, False, mutant=mutant))["ll"], ll)]
    if not misses:
        misses += ["B.2 means " + s for s in dc.means_misses("pf", d, True, pr.run(**dc.b2_args("pf", d, True, mutant=mutant))["mean"])]
    print(f"{mutant} at d = {d} misses: " + ("; ".join(misses) if misses else "NOTHING"))
    assert misses


# ---- B.4 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", dc.PG_DIMS)
def test_smoother_is_the_dense_joint_law_s_and_the_exact_start_is_a_sample_of_it(d):
    """The oracle's smoother multiplies by G_t where dt_t = 0 (the reference's G(0) is the identity; a table entry behind g_index is not), so
    the yardstick here is the joint Gaussian law of (x_0 .. x_T, y) written out densely and conditioned on the observed y."""
    import pg_checks as ck
    c = dc.pg_case(d)
    kw = c["kw"]
    T1 = dc.T + 1
    mu, Sig = np.zeros((T1, d)), np.zeros((T1, T1, d, d))
    mu[0], Sig[0, 0] = kw["m0"], kw["C0"]
    for t in range(dc.T):
        A = kw["G"][kw["g_index"][t]] if kw["dt"][t] != 0.0 else np.eye(d)
        mu[t + 1] = A @ mu[t]
        for s in range(t + 1):
            Sig[s, t + 1] = Sig[s, t] @ A.T
            Sig[t + 1, s] = Sig[s, t + 1].T
        Sig[t + 1, t + 1] = A @ Sig[t, t] @ A.T + kw["W"] * kw["dt"][t]
    big = Sig.transpose(0, 2, 1, 3).reshape(T1 * d, T1 * d)
    seen = [t for t in range(dc.T) if not np.isnan(kw["y"][0, t])]
    H = np.zeros((len(seen), T1 * d))
    for i, t in enumerate(seen):
        H[i, (t + 1) * d:(t + 2) * d] = kw["F"][t]
    Kg = np.linalg.solve(H @ big @ H.T + kw["V"] * np.eye(len(seen)), H @ big).T
    post_mean = (mu.reshape(-1) + Kg @ (kw["y"][0, seen] - H @ mu.reshape(-1))).reshape(T1, d)
    post = (big - Kg @ H @ big).reshape(T1, d, T1, d)
    scale = np.abs(c["cov"]).max()
    np.testing.assert_allclose(c["mean"], post_mean, rtol=0, atol=1e-10)
    for t in range(T1):
        np.testing.assert_allclose(c["cov"][t], post[t, :, t, :], rtol=0, atol=1e-10 * scale)
        if t < dc.T:
            np.testing.assert_allclose(c["cross"][t], post[t, :, t + 1, :], rtol=0, atol=1e-10 * scale)
    z = dc.smoother_z(d, c["start"])
    print(f"d = {d}: the exact start, worst in standard errors: means {z[0]:.2f}, variances {z[1]:.2f}, lag-one cross-covariances {z[2]:.2f}")
    assert max(z) <= ck.SIGMAS
