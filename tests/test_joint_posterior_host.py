"""The oracle's construction of every sampler's draw against the dense joint posterior (tests/joint_posterior.py).

Each construction is affine in its normals, theta = s + L z; s and L L^T must be the mean and the FULL covariance of the stacked path
given y, which joint_posterior.dense_posterior obtains in 50 digits without any recursion.  The bound 1e-10 only has to separate
rounding (<= 1.3e-14 for every construction on these cases, profiles/r10_notes.md) from a mistake of derivation (>= 1e-3).  Two pins keep the
sensitivity of the method on record: the literal SvdSampler and polynomial(2) at a repeated time."""
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import joint_posterior as jp  # noqa: E402

BOUND = 1e-10


def _check(case, draw, label):
    mean, cov, _ = case.reference()
    s, L = jp.affine_map(draw, case.n_normals)
    e_mean, e_cov = jp.measure(s, L, mean, cov)
    print(f"{case.name:40s} {label:12s} e_mean {e_mean:.2e}  e_cov {e_cov:.2e}")
    assert e_mean <= BOUND and e_cov <= BOUND, (case.name, label, e_mean, e_cov)


@pytest.mark.parametrize("case", jp.CASES, ids=jp.CASE_IDS)
def test_oracle_draw_is_the_joint_posterior(case):
    if case.kind == "ffbs":
        _check(case, case.oracle_draw("chol"), "chol")
        _check(case, case.oracle_draw("eig"), "eig")
    else:
        _check(case, case.oracle_draw(), case.kind)


@pytest.mark.parametrize("case", jp.DLM_MODELS, ids=lambda c: c.name)
def test_oracle_smoother_filter_and_loglik_are_the_dense_ones(case):
    """s_t and the diagonal blocks S_t of the smoother, (m_T, C_T) of the filter, oracle.loglik."""
    mat, p, y = case.mat, case.p, case.y
    d, T = mat.d, mat.T
    mean, cov, ll = case.reference()
    om = jp.omodel(mat)
    f = oracle.kf_filter(om, p.v, p.w, p.m0, p.c0, y)
    sm = oracle.smoother(om, f)
    scale_m, scale_c = max(1.0, np.abs(mean).max()), np.abs(cov).max()
    e_s = np.abs(sm["s"].reshape(-1) - mean).max() / scale_m
    e_S = max(np.abs(oracle.from_cm(sm["S"][t], d, d) - cov[t * d:(t + 1) * d, t * d:(t + 1) * d]).max() for t in range(T + 1)) / scale_c
    e_m = np.abs(f["m"][T] - mean[T * d:]).max() / scale_m
    e_C = np.abs(oracle.from_cm(f["C"][T], d, d) - cov[T * d:, T * d:]).max() / scale_c
    e_ll = abs(oracle.loglik(om, f, y) - ll) / max(1.0, abs(ll))
    print(f"{case.name:40s} s {e_s:.2e} S {e_S:.2e} m_T {e_m:.2e} C_T {e_C:.2e} loglik {e_ll:.2e}")
    assert max(e_s, e_S, e_m, e_C, e_ll) <= BOUND


def test_pin_literal_svd_sampler_is_another_distribution():
    """SvdSampler as written does not draw from the posterior: the method sees it."""
    case = next(c for c in jp.CASES if c.name == "svd_c2_T4")
    mat, p = case.mat, case.p
    om = jp.omodel(mat)
    sf = oracle.svd_filter(om, p.v, p.w, p.m0, p.c0, case.y)
    draw = lambda z: np.stack([oracle.svd_backward_sample(om, p.w, sf, zn, literal_q9=True)["theta"].reshape(-1) for zn in z])
    e_mean, e_cov = jp.measure(*jp.affine_map(draw, case.n_normals), *case.reference()[:2])
    print(f"svd_c2_T4 literal Q9: e_mean {e_mean:.3g}  e_cov {e_cov:.3g}")
    assert e_cov > 1e-2


def test_pin_repeated_time_with_g0_not_identity():
    """polynomial(2) on times 1, 2, 2, 4.5, 5, 9: the forward pass does not advance at dt = 0, so the filter and the
    log-likelihood are those of the dense model; the backward passes apply g(0) != I there, so the smoothed and sampled records
    before the repeated time are not."""
    case = jp.poly2_repeated_time()
    mat, p, y = case.mat, case.p, case.y
    d, T = mat.d, mat.T
    mean, cov, ll = case.reference()
    om = jp.omodel(mat)
    f = oracle.kf_filter(om, p.v, p.w, p.m0, p.c0, y)
    assert abs(oracle.loglik(om, f, y) - ll) <= BOUND * max(1.0, abs(ll))
    assert np.abs(f["m"][T] - mean[T * d:]).max() <= BOUND * max(1.0, np.abs(mean).max())
    assert np.abs(oracle.from_cm(f["C"][T], d, d) - cov[T * d:, T * d:]).max() <= BOUND * np.abs(cov).max()
    sm = oracle.smoother(om, f)
    before = slice(0, 3 * d)      # records 0 .. 2: the backward step from record 3 (dt = 0) and everything behind it
    e_s = np.abs(sm["s"].reshape(-1) - mean)[before].max() / max(1.0, np.abs(mean).max())
    s, L = jp.affine_map(case.oracle_draw("chol"), case.n_normals)
    e_mean = np.abs(s - mean)[before].max() / max(1.0, np.abs(mean).max())
    e_cov = np.abs(L @ L.T - cov)[before, before].max() / np.abs(cov).max()
    after = slice(3 * d, None)    # from the repeated time on everything is the posterior
    e_after = max(np.abs(s - mean)[after].max() / max(1.0, np.abs(mean).max()), np.abs(L @ L.T - cov)[after, after].max() / np.abs(cov).max())
    print(f"poly2 repeated time: smoother e_s {e_s:.3g}  sampler e_mean {e_mean:.3g} e_cov {e_cov:.3g}  after the repeat {e_after:.2e}")
    assert e_s > 1e-3 and e_mean > 1e-3 and e_cov > 1e-3
    assert e_after <= BOUND


def test_affine_map_and_measure_on_a_known_map():
    rng = np.random.default_rng(0)
    A, b = rng.standard_normal((5, 3)), rng.standard_normal(5)
    s, L = jp.affine_map(lambda z: z @ A.T + b, 3)
    np.testing.assert_array_equal(s, b)
    np.testing.assert_allclose(L, A, rtol=0, atol=1e-15)
    e_mean, e_cov = jp.measure(s, L, b, A @ A.T)
    assert e_mean == 0.0 and e_cov <= 1e-15
    assert jp.measure(s + 1.0, L, b, A @ A.T)[0] == pytest.approx(1.0 / max(1.0, np.abs(b).max()))
