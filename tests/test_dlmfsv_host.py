"""The DLM with factor stochastic-volatility noise on the CPU: the NumPy restatement of its two kernels (tests/dlmfsv_restatement.py)
against plain linear algebra and against the model -- the exact-invariance check of one iteration, what each injected mistake breaks, the
toy that separates the default order of the steps from the reference's -- and what bayesian_dlms_amd/dlmfsv.py does
without a device.

What the invariance check measures at the size the tests run at (16 384 panels, p = 3, k = 2, T = 6, d = 4; whole times missing with
probability 0.1 and single components with probability 0.1; profiles/r16_notes.md has the table): every figure within 3.3 standard
errors after 1, 3 and 6 sweeps (residual variance 2.27, 2.38, 1.67).  That holds because the partially missing times are completed
before the factor calls (`impute`): with the reference's treatment -- such a time wholly missing for the factor
calls, partially observed for the state draw -- the residual variance stands at 6.08 standard errors after 3 sweeps, which
test_the_reference_treatment_of_partially_missing_times_fails holds it to."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dlmfsv_restatement as dr  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters  # noqa: E402
from bayesian_dlms_amd.dlmfsv import DlmFsv, DlmFsvParameters  # noqa: E402
from bayesian_dlms_amd.factorsv import FactorSv, FsvParameters  # noqa: E402
from bayesian_dlms_amd.gibbs import InverseGamma  # noqa: E402
from bayesian_dlms_amd.stochvol import Gaussian, SvParameters  # noqa: E402
from code_object import kernel_resources  # noqa: E402

# the check each mistake is named for at this size (one sweep).  half_exp and alpha_t fail none and are left out, not tuned in: their
# largest figure is the residual variance, 3.2 and 4.4 standard errors against 2.3 without them -- under these priors alpha stays near 0 and
# moves little from one time to the next, so exp(alpha / 2), exp(alpha_t) and exp(alpha_{t+1}) are too close for one sweep at this size
MUTANT_CHECK = {"pair_theta_t": "sigma KS", "no_diag_v": "W KS", "f_transposed": "beta mean"}


@pytest.fixture(scope="module")
def start():
    s = dr.exact_start()
    for a in s.values():
        a.setflags(write=False)
    return s


# ---- the restatements' identities ------------------------------------------------------------------------------------------------------
def _small(N=3, T=7, p=4, k=2, d=5, seed=1):
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((N, T, p))
    y[rng.random((N, T, p)) < 0.2] = np.nan
    beta = rng.standard_normal((N, p, k))
    return (y, rng.standard_normal((N, T + 1, d)), rng.standard_normal((T, d, p)), beta, rng.uniform(0.2, 2.0, (N, p)),
            rng.standard_normal((N, k, T + 1)))


def test_center_keeps_nan_and_is_y_minus_f_theta():
    y, theta, F, *_ = _small()
    r, st, mag = dr.center(y, theta, F)
    assert np.array_equal(np.isnan(r), np.isnan(y)) and not st.any()
    want = y - np.einsum("tdj,ntd->ntj", F, theta[:, 1:])
    m = ~np.isnan(y)
    assert np.allclose(r[m], want[m], rtol=0.0, atol=1e-14 * mag.max())
    assert not np.allclose(r[m], (y - np.einsum("tdj,ntd->ntj", F, theta[:, :-1]))[m])          # theta[t+1], not theta[t]
    r1, _, _ = dr.center(y, theta, F[0])                                                         # one matrix: broadcast over the times
    assert np.array_equal(r1[:, 0], r[:, 0], equal_nan=True)
    bad = theta.copy()
    bad[1, 3, 2] = np.inf
    bad[2, 0, 0] = np.nan                                                                        # theta_0 belongs to no observation
    assert dr.center(y, bad, F)[1].tolist() == [0, _lib.ST_NONFINITE, 0]


def test_variance_is_symmetric_bit_for_bit_and_the_dense_form():
    *_, beta, v, alpha = _small()
    V, st, mag = dr.variance(beta, v, alpha)
    assert np.array_equal(V, np.swapaxes(V, 2, 3)) and not st.any()
    want = np.einsum("nil,nlt,njl->ntij", beta, np.exp(alpha[:, :, 1:]), beta) + np.einsum("ni,ij->nij", v, np.eye(4))[:, None]
    assert np.allclose(V, want, rtol=1e-14, atol=1e-14 * mag.max())
    assert (np.linalg.eigvalsh(V) > 0.0).all()
    for mutant in ("alpha_t", "no_diag_v", "half_exp"):
        assert not np.allclose(dr.variance(beta, v, alpha, mutant=mutant)[0], want)
    for field, idx, value in (("beta", (1, 1, 1), np.nan), ("v", (1, 2), 0.0), ("v", (1, 2), -1.0), ("alpha", (1, 1, 2), np.inf), ("alpha", (1, 1, 2), 800.0)):
        arrs = {"beta": beta.copy(), "v": v.copy(), "alpha": alpha.copy()}
        arrs[field][idx] = value
        assert dr.variance(arrs["beta"], arrs["v"], arrs["alpha"])[1].tolist() == [0, _lib.ST_NONFINITE, 0], (field, value)


def test_a_transposed_f_is_another_matrix_in_the_invariance_model():
    mat = dr.inv_mat()
    assert (mat.d, mat.p) == (4, 3) and mat.f_stride == 0
    F = dr.f_tables(mat)
    assert np.array_equal(F[0], [[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    theta = np.arange(1.0, 4.0 * 3 + 1).reshape(1, 3, 4)
    r, _, _ = dr.center(np.zeros((1, 2, 3)), theta, F[:2])
    rt, _, _ = dr.center(np.zeros((1, 2, 3)), theta, F[:2], mutant="f_transposed")
    assert np.array_equal(r[0, 0], [-5.0, -7.0, -8.0]) and not np.array_equal(r, rt)


# ---- exact invariance --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def swept(start):
    """The states after 1 and 3 sweeps of the default order (the third sweep continues the first: one chain)."""
    out, state = {}, start
    for it in range(3):
        state = dr.sweep_host(state, it)
        out[it + 1] = state
    return out


@pytest.mark.parametrize("sweeps", [1, 3])
def test_the_default_order_leaves_the_joint_law_invariant(start, swept, sweeps):
    fig = dr.figures(swept[sweeps], start)
    print(f"{sweeps} sweep(s): {dr.describe(fig)}  moved: theta {fig['moved theta']:.3f} W {fig['moved W']:.3f}")
    assert dr.failed(fig) == [], dr.describe(fig)
    assert fig["moved theta"] > 0.05 and fig["moved W"] > 0.15


def test_the_reference_treatment_of_partially_missing_times_fails(start):
    """Q34: without the completion of the partially missing times the same three sweeps leave the joint law (residual variance 6.08
    standard errors; 4.02 after one sweep, which still passes)."""
    state = start
    for it in range(3):
        state = dr.sweep_host(state, it, impute_partial=False)
    fig = dr.figures(state, start)
    print(dr.describe(fig))
    assert "residual variance" in dr.failed(fig), dr.describe(fig)


def test_impute_completes_the_partially_missing_times_alone():
    y, theta, F, beta, v, alpha = _small(N=4, T=9, p=4, k=2)
    beta[:, 0, 0], beta[:, 0, 1], beta[:, 1, 1] = 1.0, 0.0, 1.0
    r = dr.center(y, theta, F)[0]
    r[0, 1] = np.nan                                         # a wholly missing time
    r[0, 2] = np.arange(4.0)                                 # a complete one
    r[0, 3, :] = [np.nan, 0.5, np.nan, np.inf]               # inf counts as missing
    out, st, _ = dr.impute(r, beta, v, alpha, seed=3, series_offset=5, it=2)
    obs = np.isfinite(r)
    part = obs.any(axis=2) & ~obs.all(axis=2)
    assert not st.any() and part.any()
    assert np.array_equal(out[obs], r[obs]) and np.isnan(out[0, 1]).all()
    assert np.isfinite(out[part]).all() and np.array_equal(np.isnan(out[~part]), np.isnan(r[~part]))
    again, _, _ = dr.impute(r, beta, v, alpha, seed=3, series_offset=5, it=2)
    other, _, _ = dr.impute(r, beta, v, alpha, seed=3, series_offset=5, it=3)
    assert np.array_equal(again, out, equal_nan=True) and not np.array_equal(other[part], out[part])
    half, _, _ = dr.impute(r[2:], beta[2:], v[2:], alpha[2:], seed=3, series_offset=7, it=2)
    assert np.array_equal(half, out[2:], equal_nan=True)
    # the draw's law: with many replicates of one partially missing time the completed components have the model's conditional moments
    M = 40000
    b1, v1, a1 = np.broadcast_to(beta[:1], (M, 4, 2)), np.broadcast_to(v[:1], (M, 4)), np.broadcast_to(alpha[:1, :, :2], (M, 2, 2))
    r1 = np.tile(np.array([[[0.7, np.nan, -0.4, np.nan]]]), (M, 1, 1))
    got = dr.impute(r1, b1, v1, a1, seed=1, series_offset=0, it=0)[0][:, 0]
    V = dr.variance(beta[:1], v[:1], alpha[:1, :, :2])[0][0, 0]
    o, m = [0, 2], [1, 3]
    K = V[np.ix_(m, o)] @ np.linalg.inv(V[np.ix_(o, o)])
    mean, cov = K @ np.array([0.7, -0.4]), V[np.ix_(m, m)] - K @ V[np.ix_(o, m)]
    assert np.abs(got[:, m].mean(axis=0) - mean).max() < 5.0 * np.sqrt(cov.diagonal().max() / M)
    assert np.abs(np.cov(got[:, m].T) - cov).max() < 0.05 * cov.diagonal().max()
    bad = v.copy()
    bad[1, 0] = 0.0
    al = alpha.copy()
    al[2, 0, 1 + int(np.nonzero(part[2])[0][0])] = np.nan
    out2, st2, _ = dr.impute(r, beta, bad, al, seed=3, series_offset=5, it=2)
    assert st2.tolist() == [0, _lib.ST_NONFINITE, _lib.ST_NONFINITE, 0] and np.array_equal(out2[1], r[1], equal_nan=True)
    assert np.array_equal(out2[[0, 3]], out[[0, 3]], equal_nan=True)


def test_whole_missing_times_alone_leave_the_joint_law_invariant(monkeypatch):
    """The same model, sweeps and bounds with whole times missing (probability 0.1) and no single component: nothing to complete."""
    monkeypatch.setattr(dr, "INV_MISSING_COMPONENT", 0.0)
    start = dr.exact_start()
    assert np.array_equal(np.isnan(start["y"]).any(axis=2), np.isnan(start["y"]).all(axis=2)) and np.isnan(start["y"]).any()
    state = start
    for it in range(3):
        state = dr.sweep_host(state, it)
        if it in (0, 2):
            fig = dr.figures(state, start)
            print(f"{it + 1} sweep(s): {dr.describe(fig)}")
            assert dr.failed(fig) == [], dr.describe(fig)


@pytest.mark.parametrize("mutant", sorted(MUTANT_CHECK))
def test_each_mistake_alone_fails_its_check(start, mutant):
    fig = dr.figures(dr.sweep_host(start, 0, mutant=mutant), start)
    print(mutant, dr.describe(fig), dr.failed(fig))
    assert MUTANT_CHECK[mutant] in dr.failed(fig), (mutant, dr.describe(fig))


def test_the_toy_separates_the_two_orders():
    """Default order: every figure within 5 standard errors; the reference's order leaves the mean of alpha by more than 4 after 10 sweeps
    (-7.3 at this seed; -4.1 after 3)."""
    for sweeps in (3, 10):
        fig = dr.toy(sweeps, False)
        print(f"default order, {sweeps} sweeps: {fig}")
        assert abs(fig["mean"]) <= 5.0 and abs(fig["var"]) <= 5.0
    fig = dr.toy(10, True)
    print(f"reference order, 10 sweeps: {fig}")
    assert abs(fig["mean"]) > 4.0


# ---- dlmfsv.py without a device -----------------------------------------------------------------------------------------------------------
def _params(p=3, k=2, d=4):
    fsv = FsvParameters(0.5, FactorSv.build_beta(p, k, 0.3), [SvParameters(0.8, 0.0, 0.3)] * k)
    return DlmFsvParameters(DlmParameters(np.eye(p), 0.1 * np.eye(d), np.zeros(d), np.eye(d)), fsv)


PRIORS = (Gaussian(0.0, 1.0), InverseGamma(3.0, 0.3), Gaussian(0.8, 0.1), Gaussian(0.0, 1.0), InverseGamma(3.0, 1.0), InverseGamma(3.0, 0.5))


def test_parameters_are_validated():
    par = _params()
    assert par.fsv.p == 3 and par.dlm.w.shape == (4, 4)
    with pytest.raises(TypeError):
        DlmFsvParameters(par.dlm, (0.5, par.fsv.beta))
    with pytest.raises(TypeError):
        DlmFsvParameters(None, par.fsv)
    w = 0.1 * np.eye(4)
    w[0, 1] = 0.01
    with pytest.raises(ValueError):          # W must be diagonal
        DlmFsvParameters(DlmParameters(np.eye(3), w, np.zeros(4), np.eye(4)), par.fsv)
    with pytest.raises(ValueError):
        DlmFsvParameters(DlmParameters(np.eye(3), np.diag([0.1, 0.0, 0.1, 0.1]), np.zeros(4), np.eye(4)), par.fsv)


def test_sample_validates_before_it_touches_a_device():
    par, mod = _params(), dr.inv_model()
    ys = np.zeros((2, 6, 3))
    run = lambda *a, **kw: DlmFsv.sample(*a, None, n_iter=1, **kw)
    with pytest.raises(TypeError):
        run((0.0, 1.0), *PRIORS[1:], ys, mod, par)
    with pytest.raises(TypeError):
        run(*PRIORS[:5], Gaussian(0.0, 1.0), ys, mod, par)          # prior_w must be an InverseGamma
    with pytest.raises(TypeError):
        run(*PRIORS, ys, mod, par.fsv)
    with pytest.raises(ValueError):
        run(*PRIORS, np.zeros((2, 6, 4)), mod, par)                 # p of ys and of the model differ
    with pytest.raises(ValueError):
        run(*PRIORS, np.zeros((6, 3)), mod, par)
    with pytest.raises(ValueError):
        run(*PRIORS, np.zeros((2, 1, 3)), mod, par)                 # T < 2
    with pytest.raises(ValueError):
        run(*PRIORS, ys, Dlm.polynomial(1) * Dlm.polynomial(1) * Dlm.polynomial(1), par)          # d = 3 against a 4 x 4 W
    with pytest.raises(ValueError, match="regular unit time grid"):
        run(*PRIORS, ys, mod, par, times=[1.0, 2.0, 3.0, 4.0, 5.0, 7.0])
    with pytest.raises(ValueError, match="regular unit time grid"):
        run(*PRIORS, ys, mod, par, times=0.5 * np.arange(6))
    with pytest.raises(ValueError, match="regular unit time grid"):
        run(*PRIORS, ys, mod, par, times=np.arange(5.0))


def test_simulate_shapes_and_moments():
    par, mod = _params(), dr.inv_model()
    y, theta, f, alpha = DlmFsv.simulate(mod, par, 7, 4000, seed=3)
    assert y.shape == (4000, 7, 3) and theta.shape == (4000, 8, 4) and f.shape == (4000, 2, 7) and alpha.shape == (4000, 2, 8)
    assert np.array_equal(DlmFsv.simulate(mod, par, 7, 4000, seed=3)[0], y)
    G = np.eye(4) + np.eye(4, k=1) * np.array([1.0, 0.0, 0.0, 0.0])[:, None]
    trans = (theta[:, 1:] - theta[:, :-1] @ G.T) / np.sqrt(0.1)
    assert abs(trans.mean()) < 0.02 and abs(trans.var() - 1.0) < 0.02
    res = y - theta[:, 1:][:, :, [0, 2, 3]] - np.einsum("ij,njt->nti", par.fsv.beta, f)
    assert abs(res.var() - 0.5) < 0.02


def test_the_state_draw_never_shares_its_normals_with_a_volatility_draw():
    from bayesian_dlms_amd.stochvol import StochasticVolatility
    a = {DlmFsv._seed_theta(s, k) for s in (0, 1, 21) for k in range(50)}
    b = {StochasticVolatility._seed_ffbs(s, k) for s in (0, 1, 21) for k in range(50)}
    assert len(a) == 150 and not (a & b)


def test_the_bindings_carry_both_exports():
    names = {n for n, _, _ in _lib.SYMBOLS}
    assert {"dlm_dlmfsv_center_batch", "dlm_dlmfsv_impute_batch", "dlm_dlmfsv_variance_batch"} <= names
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in ("dlm_dlmfsv_center_batch", "dlm_dlmfsv_impute_batch", "dlm_dlmfsv_variance_batch"))
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bayesian_dlms_amd", "csrc", "dlm_draws.h")).read()
    assert f"DLM_KEY_DLMFSV = 0x{dr.KEY_DLMFSV:08X}u" in src


def test_the_kernels_have_no_scratch_and_no_spills():
    assert kernel_resources("dlm_dlmfsv.o", "k_dlmfsv_center")[:2] == (0, 0)
    for k in range(1, 9):
        assert kernel_resources("dlm_dlmfsv.o", f"k_dlmfsv_varianceILi{k}E")[:2] == (0, 0), k
        assert kernel_resources("dlm_dlmfsv.o", f"k_dlmfsv_imputeILi{k}E")[:2] == (0, 0), k
