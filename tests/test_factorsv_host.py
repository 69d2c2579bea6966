"""The factor stochastic-volatility sampler on the CPU: the NumPy restatement of its two kernels (tests/fsv_restatement.py) against the
model -- the default arithmetic leaves the joint law invariant, each of the reference's four quirks and the
literal mode as a whole do not -- and what bayesian_dlms_amd/factorsv.py does without a device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fsv_restatement as fr  # noqa: E402
import sampler_restatement as sr  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.factorsv import FactorSv, FsvParameters  # noqa: E402
from bayesian_dlms_amd.gibbs import InverseGamma  # noqa: E402
from bayesian_dlms_amd.stochvol import Gaussian, SvParameters  # noqa: E402


@pytest.fixture(scope="module")
def start():
    s = fr.exact_start()
    for a in s.values():
        a.setflags(write=False)
    return s


def test_the_default_arithmetic_leaves_the_joint_law_invariant(start):
    fig = fr.figures(start, *fr.step_host(start))
    print(fr.describe(fig))
    assert fr.failed(fig) == [], fr.describe(fig)


@pytest.mark.parametrize("which", fr.MUTANTS + ("literal",))
def test_each_quirk_alone_and_the_literal_mode_fail_their_check(start, which):
    kw = {"literal": True} if which == "literal" else {"mutant": which}
    fig = fr.figures(start, *fr.step_host(start, **kw))
    print(which, fr.describe(fig), fr.failed(fig))
    assert fr.MUTANT_CHECK[which] in fr.failed(fig), (which, fr.describe(fig))


def test_the_rehearsal_table_of_the_quirks(start):
    """What each quirk breaks, as the NumPy prototype that motivated the corrected defaults found it (profiles/r15_notes.md)."""
    figs = {m: fr.figures(start, *fr.step_host(start, mutant=m)) for m in fr.MUTANTS}
    assert figs["Q27"]["factor variance"] > 10.0 and figs["Q27"]["beta variance"] > fr.SE_BOUND and figs["Q27"]["sigma KS"] < 1e-6
    assert figs["Q28"]["sigma KS"] < 1e-6 and figs["Q28"]["residual variance"] > fr.SE_BOUND
    assert figs["Q29"]["beta mean"] > fr.SE_BOUND and figs["Q29"]["beta variance"] > 30.0
    assert figs["Q30"]["beta variance"] > 20.0 and figs["Q30"]["residual variance"] > 20.0
    # a quirk of the loadings leaves the factor draw alone, and Q28 leaves beta's law alone
    for m in ("Q28", "Q29", "Q30"):
        assert figs[m]["factor variance"] <= fr.SE_BOUND and figs[m]["factor mean"] <= fr.SE_BOUND
    assert figs["Q28"]["beta variance"] <= fr.SE_BOUND


def test_the_batched_gamma_is_the_restatement_s_gamma():
    shape = np.array([0.4, 1.0, 3.7, 17.5, 250.0])
    series = np.array([0, 5, 77, 1 << 33, 12])
    got = fr.gamma_units(shape, 9, series, 3, fr.FSV_SLOT_SIGMA, fr.KEY_FSV)
    want = [sr.gamma_unit(a, 9, int(s), 3, fr.FSV_SLOT_SIGMA, fr.KEY_FSV)[0] for a, s in zip(shape, series)]
    assert np.array_equal(got, np.array(want))


def test_the_vectorised_normals_are_draw_normal():
    series, comp, att = np.array([3, 1 << 35]), np.array([0, fr.FSV_SLOT_ROW0 - 7]), np.array([0, 5])
    got = fr.normals(11, series, (1 << 64) - 1, comp, att)
    want = [sr.normal(fr.KEY_FSV, 11, int(s), (1 << 64) - 1, int(c), int(a)) for s, c, a in zip(series, comp, att)]
    assert np.array_equal(got, np.array(want))


def test_solve_draw_against_dense_linear_algebra():
    rng = np.random.default_rng(4)
    for q in (1, 2, 5, 8):
        A = rng.standard_normal((7, q, q + 2))
        P = A @ np.swapaxes(A, 1, 2) + 0.5 * np.eye(q)
        r, z = rng.standard_normal((7, q)), rng.standard_normal((7, q))
        L = np.linalg.cholesky(P)
        x, ok = fr.solve_draw(P, r, z, False)
        want = np.linalg.solve(P, r[..., None])[..., 0] + np.linalg.solve(np.swapaxes(L, 1, 2), z[..., None])[..., 0]
        assert ok.all() and np.allclose(x, want, rtol=1e-10, atol=1e-12)
        x, ok = fr.solve_draw(P, r, z, True)
        assert ok.all() and np.allclose(x, np.linalg.solve(P, (r + z)[..., None])[..., 0], rtol=1e-10, atol=1e-12)
    bad = np.array([[[1.0, 0.0], [2.0, 1.0]]])          # the lower triangle of [[1, 2], [2, 1]]: not positive definite
    assert not fr.solve_draw(bad, np.ones((1, 2)), np.zeros((1, 2)), False)[1].any()


def test_partially_missing_times_empty_panels_and_bad_rows_in_the_restatement():
    rng = np.random.default_rng(5)
    N, T, p, k = 4, 9, 4, 2
    beta = np.broadcast_to(FactorSv.build_beta(p, k, 0.4), (N, p, k)).copy()
    v = np.full((N, p), 0.5)
    y = rng.standard_normal((N, T, p))
    y[0, 2, 1] = np.nan                          # partially missing: wholly missing
    y[1] = np.nan                                # a panel without an observed time
    v[2, 3] = 0.0                                # a bad row
    f, st, _ = fr.factors(y, beta, v, None, seed=1, series_offset=0, it=0)
    assert np.isnan(f[0, :, 2]).all() and np.isfinite(np.delete(f[0], 2, axis=1)).all()
    assert np.isnan(f[1]).all() and st[1] == 0
    assert np.isnan(f[2]).all() and st[2] == _lib.ST_NONFINITE and st[3] == 0 and np.isfinite(f[3]).all()
    b, vo, st, _ = fr.loadings(y, f, beta, v, fr.fsv_prior(), seed=1, series_offset=0, it=0)
    assert st[1] == _lib.ST_NONFINITE and np.array_equal(b[1], beta[1]) and np.array_equal(vo[1], v[1])
    assert st[2] == _lib.ST_NONFINITE and np.array_equal(b[2], beta[2])          # every f of panel 2 is NaN: no counted time
    assert st[0] == 0 and st[3] == 0 and np.isfinite(b[[0, 3]]).all() and (vo[[0, 3]] > 0.0).all()
    assert np.array_equal(b[0][np.triu_indices(p, 0, k)], FactorSv.make_beta(p, k)[np.triu_indices(p, 0, k)])


# ---- factorsv.py without a device ----------------------------------------------------------------------------------------------------
def _params(p=5, k=2, v=0.5):
    return FsvParameters(v, FactorSv.build_beta(p, k, 0.3), [SvParameters(0.8, 0.0, 0.3)] * k)


def test_make_beta_and_build_beta():
    assert np.array_equal(FactorSv.make_beta(3, 2), [[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]])
    draws = iter(range(2, 100))
    b = FactorSv.build_beta(4, 3, lambda: next(draws))
    assert np.array_equal(b, [[1.0, 0.0, 0.0], [2.0, 1.0, 0.0], [3.0, 4.0, 1.0], [5.0, 6.0, 7.0]])
    for p, k in ((2, 3), (65, 2), (9, 9), (3, 0)):
        with pytest.raises(ValueError):
            FactorSv.build_beta(p, k, 0.0)


def test_fsv_parameters_shapes_and_validation():
    par = _params()
    assert (par.p, par.k) == (5, 2) and par.v.shape == (5,) and par.sv().shape == (2, 3)
    assert all(isinstance(q, SvParameters) for q in par.factor_params)
    assert np.array_equal(FsvParameters(np.diag([1.0, 2.0, 3.0]), FactorSv.make_beta(3, 1), [(0.5, 0.0, 0.1)]).v, [1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        FsvParameters(0.5, FactorSv.make_beta(5, 2), [SvParameters(0.8, 0.0, 0.3)])          # one triple for two factors
    with pytest.raises(ValueError):
        FsvParameters(-1.0, FactorSv.make_beta(5, 2), [SvParameters(0.8, 0.0, 0.3)] * 2)
    with pytest.raises(ValueError):
        FsvParameters(1.0, FactorSv.make_beta(5, 2), [SvParameters(1.2, 0.0, 0.3)] * 2)      # not stationary
    with pytest.raises(ValueError):
        FsvParameters(1.0, np.ones((3, 9)), [SvParameters(0.8, 0.0, 0.3)] * 9)


def test_simulate_shapes_and_moments():
    par = _params()
    y, f, alpha = FactorSv.simulate(par, 7, 2000, seed=3)
    assert y.shape == (2000, 7, 5) and f.shape == (2000, 2, 7) and alpha.shape == (2000, 2, 8)
    assert np.array_equal(FactorSv.simulate(par, 7, 2000, seed=3)[0], y)
    white = f / np.exp(0.5 * alpha[:, :, 1:])
    assert abs(white.mean()) < 0.05 and abs(white.var() - 1.0) < 0.05
    res = y - np.einsum("ij,njt->nti", par.beta, f)
    assert abs(res.var() - 0.5) < 0.02


def test_sample_ar_validates_before_it_touches_a_device():
    par = _params()
    g, ig = Gaussian(0.0, 1.0), InverseGamma(3.0, 1.0)
    ys = np.zeros((2, 6, 5))
    with pytest.raises(TypeError):
        FactorSv.sample_ar((0.0, 1.0), ig, g, g, ig, ys, par, None, n_iter=1)
    with pytest.raises(TypeError):
        FactorSv.sample_ar(g, ig, g, g, ig, ys, (0.5, par.beta), None, n_iter=1)
    with pytest.raises(ValueError):
        FactorSv.sample_ar(g, ig, g, g, ig, np.zeros((2, 6, 4)), par, None, n_iter=1)          # p of ys and of beta differ
    with pytest.raises(ValueError):
        FactorSv.sample_ar(g, ig, g, g, ig, np.zeros((2, 1, 5)), par, None, n_iter=1)          # T < 2
    with pytest.raises(ValueError):
        FactorSv.sample_ar(g, ig, g, g, ig, np.zeros((6, 5)), par, None, n_iter=1)


def test_the_bindings_carry_the_prior_struct_and_both_exports():
    assert [n for n, _ in _lib.FsvPrior._fields_] == ["literal", "beta_mean", "beta_sd", "sigma_shape", "sigma_scale"]
    assert fr.fsv_prior_tuple(fr.fsv_prior(1)) == (1, 0.3, 0.7, 4.0, 1.5)
    names = {n for n, _, _ in _lib.SYMBOLS}
    assert {"dlm_fsv_factors_batch", "dlm_fsv_loadings_batch"} <= names
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bayesian_dlms_amd", "csrc", "dlm_draws.h")).read()
    assert f"DLM_KEY_FSV = 0x{fr.KEY_FSV:08X}u" in src and "DLM_FSV_SLOT_ROW0 = DLM_SLOT_TOP - 1" in src
