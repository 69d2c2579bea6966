"""dlm_fsv_factors_batch / dlm_fsv_loadings_batch on the GPU (FactorSv.sampleFactors, sampleSigmaUni, sampleBeta) and the
FactorSv.sample_ar driver.

The kernels are held draw for draw to their NumPy restatement (tests/fsv_restatement.py) at the project's draw-for-draw tolerance
(tests/test_stochvol_gpu.py): the arithmetic is restated operation for operation (the build contracts no a * b + c), so what remains
is the last bits of log, cos and exp, carried through systems whose condition number the inputs keep below 1e3 (asserted).  Then the
exact-invariance check on the device, the bad rows, the argument errors, the sharding and the driver.
Beyond condition numbers of 1e3 and at k = 4..7, which no shape here reaches, tests/test_fsv_dense_reference_gpu.py holds both kernels to a
50-digit dense reference within bounds derived from the arithmetic.

The largest relative difference seen on an MI355X is in profiles/r15_notes.md."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fsv_dense_reference as dense  # noqa: E402
import fsv_restatement as fr  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.engine import Engine, EngineError  # noqa: E402
from bayesian_dlms_amd.factorsv import INIT_ITERATION, FactorSv, FsvParameters  # noqa: E402
from bayesian_dlms_amd.gibbs import InverseGamma  # noqa: E402
from bayesian_dlms_amd.stochvol import MASK64, Gaussian, SvParameters  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-11, 1e-12
COND_MAX = 1e3
SHAPES = [(1, 2, 1, 1), (3, 64, 5, 2), (2, 257, 9, 3), (2, 70, 64, 8)]          # (N, T, p, k)
LOADINGS_SHAPES = SHAPES + [(2, 1000, 5, 2)]
SEED, OFFSET, ITER = 0x1234_5678_9ABC, 7, 3


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _dev(a):
    import torch
    return torch.as_tensor(np.array(a), device="cuda:0")          # (a copy: the shared inputs are read-only)


@functools.lru_cache(maxsize=None)
def inputs(N, T, p, k):
    """y, beta, v, alpha of a batch, read-only.  From T = 8 on: one wholly missing time per panel, one partially missing one in panel 0;
    from N = 3 on the last panel has no observed time at all."""
    rng = np.random.default_rng([N, T, p, k])
    beta = np.zeros((N, p, k))
    beta[:, fr.free_mask(p, k)] = rng.uniform(-0.8, 0.8, (N, int(fr.free_mask(p, k).sum())))
    beta[:, np.arange(k), np.arange(k)] = 1.0
    v = rng.uniform(0.3, 1.5, (N, p))
    alpha = rng.uniform(-1.0, 1.0, (N, k, T + 1))
    f = rng.standard_normal((N, k, T)) * np.exp(0.5 * alpha[:, :, 1:])
    y = np.einsum("nij,njt->nti", beta, f) + np.sqrt(v)[:, None, :] * rng.standard_normal((N, T, p))
    if T >= 8:
        y[np.arange(N), rng.integers(0, T, N), :] = np.nan
        y[0, 5, p - 1] = np.nan
    if N >= 3:
        y[N - 1] = np.nan
    out = {"y": y, "beta": beta, "v": v, "alpha": alpha}
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(N, T, p, k, literal):
    """The restatement's results for a batch, computed once: the factors with and without alpha, the loadings from those factors."""
    d = inputs(N, T, p, k)
    kw = dict(seed=SEED, series_offset=OFFSET, it=ITER)
    f, fst, c1 = fr.factors(d["y"], d["beta"], d["v"], d["alpha"], literal=literal, **kw)
    f0, f0st, c0 = fr.factors(d["y"], d["beta"], d["v"], None, literal=literal, **kw)
    b, v, lst, c2 = fr.loadings(d["y"], f, d["beta"], d["v"], fr.fsv_prior(1 if literal else 0), **kw)
    print(f"restatement {(N, T, p, k)} literal {literal}: largest condition number  P_t {max(c0, c1):.3g}  row precision {c2:.3g}")
    assert max(c0, c1, c2) < COND_MAX
    return {"f": f, "f_status": fst, "f0": f0, "f0_status": f0st, "beta": b, "v": v, "l_status": lst}


def _close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    m = ~np.isnan(want)
    rel = float((np.abs(got[m] - want[m]) / np.maximum(np.abs(want[m]), 1e-300)).max()) if m.any() else 0.0
    print(f"{what}: largest relative difference {rel:.3g}")
    np.testing.assert_allclose(got[m], want[m], rtol=RTOL, atol=ATOL, err_msg=what)
    return rel


@pytest.mark.parametrize("literal", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_factors_draw_for_draw(eng, shape, literal):
    d, ref = inputs(*shape), reference(*shape, literal)
    kw = dict(iteration=ITER, seed=SEED, series_offset=OFFSET, literal=literal)
    out = eng.fsv_factors(_dev(d["y"]), _dev(d["beta"]), _dev(d["v"]), _dev(d["alpha"]), **kw)
    assert eng.last_variant == "fsv-factors"
    _close(out["f"].cpu().numpy(), ref["f"], f"factors {shape} literal {literal}")
    assert np.array_equal(out["status"].cpu().numpy(), ref["f_status"])
    init = eng.fsv_factors(d["y"], d["beta"], d["v"], None, **kw)                 # host arrays, alpha = None: initialiseFactors
    _close(init["f"], ref["f0"], f"factors without alpha {shape} literal {literal}")
    assert np.array_equal(init["status"], ref["f0_status"])
    # another iteration and another offset are other draws
    other = eng.fsv_factors(d["y"], d["beta"], d["v"], d["alpha"], iteration=ITER + 1, seed=SEED, series_offset=OFFSET, literal=literal)["f"]
    moved = eng.fsv_factors(d["y"], d["beta"], d["v"], d["alpha"], iteration=ITER, seed=SEED, series_offset=OFFSET + 1, literal=literal)["f"]
    obs = ~np.isnan(ref["f"])
    assert (other[obs] != ref["f"][obs]).all() and (moved[obs] != ref["f"][obs]).all()


@pytest.mark.parametrize("literal", [False, True])
@pytest.mark.parametrize("shape", LOADINGS_SHAPES)
def test_loadings_draw_for_draw(eng, shape, literal):
    N, T, p, k = shape
    d, ref = inputs(*shape), reference(*shape, literal)
    pr = fr.fsv_prior_tuple(fr.fsv_prior(1 if literal else 0))
    kw = dict(iteration=ITER, seed=SEED, series_offset=OFFSET)
    beta, v = _dev(d["beta"]), _dev(d["v"])
    out = eng.fsv_loadings(_dev(d["y"]), _dev(ref["f"]), beta, pr, v=v, out={"beta": beta, "v": v}, **kw)          # in place
    assert eng.last_variant == "fsv-loadings"
    assert out["beta"].data_ptr() == beta.data_ptr() and out["v"].data_ptr() == v.data_ptr()
    _close(beta.cpu().numpy(), ref["beta"], f"loadings beta {shape} literal {literal}")
    _close(v.cpu().numpy(), ref["v"], f"loadings sigma^2 {shape} literal {literal}")
    st = out["status"].cpu().numpy()
    assert np.array_equal(st, ref["l_status"])
    host = eng.fsv_loadings(d["y"], ref["f"], d["beta"], pr, v=d["v"], **kw)          # host arrays, fresh outputs: the same bits
    assert np.array_equal(host["beta"], beta.cpu().numpy(), equal_nan=True) and np.array_equal(host["v"], v.cpu().numpy(), equal_nan=True)
    got = host["beta"]
    assert np.array_equal(got[:, np.arange(k), np.arange(k)], np.ones((N, k))) and (got[:, ~fr.free_mask(p, k) & ~np.eye(p, k, dtype=bool)] == 0.0).all()
    if N >= 3:          # the panel without an observed time keeps its inputs; without v there is nothing to keep for v_out
        assert st[N - 1] == _lib.ST_NONFINITE and not st[:N - 1].any()
        assert np.array_equal(got[N - 1], d["beta"][N - 1]) and np.array_equal(host["v"][N - 1], d["v"][N - 1])
        assert np.isnan(eng.fsv_loadings(d["y"], ref["f"], d["beta"], pr, **kw)["v"][N - 1]).all()


def test_exact_invariance_on_the_device(eng):
    start = fr.exact_start()
    y = _dev(start["y"])
    f = eng.fsv_factors(y, _dev(start["beta"]), _dev(start["v"]), _dev(start["alpha"]), iteration=0, seed=fr.SEED)
    ld = eng.fsv_loadings(y, f["f"], _dev(start["beta"]), fr.fsv_prior_tuple(fr.INV_PRIOR), iteration=0, seed=fr.SEED, v=_dev(start["v"]))
    assert not f["status"].any().item() and not ld["status"].any().item()
    fig = fr.figures(start, f["f"].cpu().numpy(), ld["beta"].cpu().numpy(), ld["v"].cpu().numpy())
    print(fr.describe(fig))
    assert fig["beta mean"] <= fr.SE_BOUND and fig["beta variance"] <= fr.SE_BOUND
    assert fig["sigma KS"] > fr.P_MARGINAL
    assert fig["factor mean"] <= fr.SE_BOUND and fig["factor variance"] <= fr.SE_BOUND
    assert fig["residual mean"] <= fr.SE_BOUND and fig["residual variance"] <= fr.SE_BOUND
    assert fig["moved beta"] > fr.NEW_DRAW_FLOOR and fig["moved f"] > fr.NEW_DRAW_FLOOR
    assert fr.failed(fig) == []


def test_the_literal_mode_on_the_device_fails_the_invariance_check(eng):
    start = fr.exact_start()
    y = _dev(start["y"])
    f = eng.fsv_factors(y, _dev(start["beta"]), _dev(start["v"]), _dev(start["alpha"]), iteration=0, seed=fr.SEED, literal=True)
    ld = eng.fsv_loadings(y, f["f"], _dev(start["beta"]), fr.fsv_prior_tuple(dict(fr.INV_PRIOR, literal=1)), iteration=0, seed=fr.SEED)
    fig = fr.figures(start, f["f"].cpu().numpy(), ld["beta"].cpu().numpy(), ld["v"].cpu().numpy())
    print(fr.describe(fig), fr.failed(fig))
    assert {"beta variance", "sigma KS", "factor variance"} <= set(fr.failed(fig))


def test_bad_rows_get_their_status_and_leave_their_neighbours_alone(eng):
    shape = (3, 64, 5, 2)
    d = inputs(*shape)
    N = 6
    y, beta, v, alpha = (np.concatenate([d[key], d[key]]) for key in ("y", "beta", "v", "alpha"))
    y[2] = d["y"][0]          # (panel 2 of the inputs has no observed time: give it some)
    y[5] = d["y"][1]
    kw = dict(iteration=ITER, seed=SEED, series_offset=OFFSET)
    clean = eng.fsv_factors(y, beta, v, alpha, **kw)
    assert not clean["status"].any()
    bb, bv, ba = beta.copy(), v.copy(), alpha.copy()
    bb[1, 3, 1] = np.inf
    bv[3, 2] = 0.0
    bv[4, 0] = -1.0
    ba[5, 1, 8] = np.nan          # alpha of time 7
    out = eng.fsv_factors(y, bb, bv, ba, **kw)
    assert out["status"].tolist() == [0, _lib.ST_NONFINITE, 0, _lib.ST_NONFINITE, _lib.ST_NONFINITE, _lib.ST_NONFINITE]
    for n in (1, 3, 4):
        assert np.isnan(out["f"][n]).all()
    for n in (0, 2):
        assert np.array_equal(out["f"][n], clean["f"][n], equal_nan=True)
    assert np.isnan(out["f"][5, :, 7]).all() and np.array_equal(np.delete(out["f"][5], 7, axis=1), np.delete(clean["f"][5], 7, axis=1), equal_nan=True)
    pr = fr.fsv_prior_tuple(fr.fsv_prior())
    lclean = eng.fsv_loadings(y, clean["f"], beta, pr, v=v, **kw)
    assert not lclean["status"].any()
    lb = beta.copy()
    lb[1, 2, 0] = np.nan          # ssy of panel 1 is not finite
    ff = clean["f"].copy()
    ff[4] = np.nan                # no counted time in panel 4
    lout = eng.fsv_loadings(y, ff, lb, pr, v=v, **kw)
    assert lout["status"].tolist() == [0, _lib.ST_NONFINITE, 0, 0, _lib.ST_NONFINITE, 0]
    assert np.isnan(lout["beta"][1]).all() and np.isnan(lout["v"][1]).all()
    assert np.array_equal(lout["beta"][4], beta[4]) and np.array_equal(lout["v"][4], v[4])
    for n in (0, 2, 3, 5):
        assert np.array_equal(lout["beta"][n], lclean["beta"][n]) and np.array_equal(lout["v"][n], lclean["v"][n])


def test_a_pivot_that_rounds_to_zero_gets_not_pd_at_its_time_alone(eng):
    """k = p = 2, beta_10 = 1e8, v = 1, alpha_{1,t+1} = 700 at one time of panel 0: the second pivot of P_t rounds to zero (in 50 digits the
    matrix is positive definite: tests/test_fsv_dense_reference_host.py)."""
    x = dense.not_pd_inputs()
    kw = dict(iteration=ITER, seed=SEED, series_offset=OFFSET)
    t = x["t"]
    clean = eng.fsv_factors(x["y"], x["beta"], x["v"], x["clean"], **kw)
    assert not clean["status"].any() and np.isfinite(clean["f"]).all()
    out = eng.fsv_factors(_dev(x["y"]), _dev(x["beta"]), _dev(x["v"]), _dev(x["alpha"]), **kw)
    f, st = out["f"].cpu().numpy(), out["status"].cpu().numpy()
    assert st.tolist() == [_lib.ST_NOT_PD, 0]
    assert np.isnan(f[0, :, t]).all()
    assert np.array_equal(np.delete(f[0], t, axis=1), np.delete(clean["f"][0], t, axis=1)) and np.array_equal(f[1], clean["f"][1])
    want, wst, _ = fr.factors(x["y"], x["beta"], x["v"], x["alpha"], seed=SEED, series_offset=OFFSET, it=ITER)
    assert wst.tolist() == st.tolist() and np.array_equal(np.isnan(want), np.isnan(f))


def test_loadings_with_a_first_pivot_that_underflows_get_not_pd(eng):
    """The status is reachable in the loadings step: literal mode (P = S_q / sigma^2 + I s^2, Q29) with a prior standard deviation whose
    square underflows and ONE counted time whose first factor's square underflows too give P_00 = 0 for every row.  (With a tiny but
    representable s^2 and an ordinary f_t the rank-one S makes the second pivot rounding noise around zero; its sign then depends on the last
    bits of sigma^2, whose Gamma draw the device and the restatement do not share to the bit, so that variant is not asserted.)"""
    N, T, p, k = 2, 4, 4, 3
    rng = np.random.default_rng(43)
    f, y = rng.standard_normal((N, k, T)), rng.standard_normal((N, T, p))
    beta = np.zeros((N, p, k))
    beta[:, fr.free_mask(p, k)] = rng.uniform(-0.8, 0.8, (N, int(fr.free_mask(p, k).sum())))
    beta[:, np.arange(k), np.arange(k)] = 1.0
    prior = fr.fsv_prior(1, beta=(0.3, 1e-170))
    pr = fr.fsv_prior_tuple(prior)
    kw = dict(iteration=ITER, seed=SEED, series_offset=OFFSET)
    clean = eng.fsv_loadings(y, f, beta, pr, **kw)
    assert not clean["status"].any() and np.isfinite(clean["beta"]).all()
    yb, fb = y.copy(), f.copy()
    yb[0, 1:] = np.nan
    fb[0, 0, 0] = 1e-170
    out = eng.fsv_loadings(_dev(yb), _dev(fb), _dev(beta), pr, **kw)
    b, v, st = out["beta"].cpu().numpy(), out["v"].cpu().numpy(), out["status"].cpu().numpy()
    assert st.tolist() == [_lib.ST_NOT_PD, 0]
    assert np.array_equal(np.isnan(b[0]), fr.free_mask(p, k)) and np.isfinite(v).all()
    assert np.array_equal(b[1], clean["beta"][1]) and np.array_equal(v[1], clean["v"][1])
    wb, wv, wst, _ = fr.loadings(yb, fb, beta, None, prior, seed=SEED, series_offset=OFFSET, it=ITER)
    assert wst.tolist() == st.tolist() and np.array_equal(np.isnan(wb), np.isnan(b))
    np.testing.assert_allclose(v, wv, rtol=RTOL)


def test_argument_errors(eng):
    d = inputs(3, 64, 5, 2)
    y, beta, v, alpha = d["y"], d["beta"], d["v"], d["alpha"]
    f = np.zeros((3, 2, 64))
    ok = (0, 0.3, 0.7, 4.0, 1.5)
    for prior in ((2, 0.3, 0.7, 4.0, 1.5), (0, 0.3, 0.0, 4.0, 1.5), (0, 0.3, -1.0, 4.0, 1.5), (0, np.inf, 0.7, 4.0, 1.5),
                  (0, 0.3, 0.7, 0.0, 1.5), (0, 0.3, 0.7, 4.0, 0.0), (0, 0.3, 0.7, 4.0, np.nan)):
        with pytest.raises(EngineError):
            eng.fsv_loadings(y, f, beta, prior, iteration=0)
    for p, k in ((10, 9), (65, 2), (2, 3)):          # k above 8, p above 64, p below k
        yy, bb, vv = np.zeros((1, 4, p)), np.zeros((1, p, k)), np.ones((1, p))
        with pytest.raises(EngineError):
            eng.fsv_factors(yy, bb, vv, None, iteration=0)
        with pytest.raises(EngineError):
            eng.fsv_loadings(yy, np.zeros((1, k, 4)), bb, ok, iteration=0)
    with pytest.raises(EngineError):          # T < 2
        eng.fsv_factors(y[:, :1], beta, v, None, iteration=0)
    with pytest.raises(EngineError):
        eng.fsv_loadings(y[:, :1], f[:, :, :1], beta, ok, iteration=0)
    big = 0x1FFFBF + 1          # DLM_FSV_MAX_T + 1
    with pytest.raises(EngineError):
        eng.fsv_factors(np.zeros((1, big, 1)), np.ones((1, 1, 1)), np.ones((1, 1)), None, iteration=0)
    with pytest.raises(EngineError):          # shapes that do not belong together
        eng.fsv_factors(y, beta, v[:, :4], alpha, iteration=0)
    with pytest.raises(EngineError):
        eng.fsv_factors(y, beta, v, alpha[:, :, :-1], iteration=0)
    with pytest.raises(EngineError):
        eng.fsv_loadings(y, f[:, :, :-1], beta, ok, iteration=0)
    with pytest.raises(EngineError):          # literal outside {0, 1} at the C interface
        eng._check(eng.lib.dlm_fsv_factors_batch(eng.h, 3, 64, 5, 2, y.ctypes.data, beta.ctypes.data, v.ctypes.data, None, 2, 0,
                                                 _lib.Options(0, _lib.DLM_MEM_HOST, 0, 0), f.ctypes.data, None))


def test_two_halves_with_a_series_offset_are_the_whole_batch(eng):
    d = inputs(2, 257, 9, 3)
    y, beta, v, alpha = (np.concatenate([d[key]] * 3) for key in ("y", "beta", "v", "alpha"))          # six panels
    kw = dict(iteration=ITER, seed=SEED)
    pr = fr.fsv_prior_tuple(fr.fsv_prior())
    whole = eng.fsv_factors(y, beta, v, alpha, series_offset=OFFSET, **kw)
    lwhole = eng.fsv_loadings(y, whole["f"], beta, pr, v=v, series_offset=OFFSET, **kw)
    for lo, hi in ((0, 3), (3, 6)):
        part = eng.fsv_factors(y[lo:hi], beta[lo:hi], v[lo:hi], alpha[lo:hi], series_offset=OFFSET + lo, **kw)
        assert np.array_equal(part["f"], whole["f"][lo:hi], equal_nan=True)
        lpart = eng.fsv_loadings(y[lo:hi], part["f"], beta[lo:hi], pr, v=v[lo:hi], series_offset=OFFSET + lo, **kw)
        assert np.array_equal(lpart["beta"], lwhole["beta"][lo:hi]) and np.array_equal(lpart["v"], lwhole["v"][lo:hi])
    assert not np.array_equal(whole["f"][0], whole["f"][2], equal_nan=True)          # the same panel at another offset: other draws


def _by_hand(eng, ys, par, priors, n_iter, seed, so, literal):
    """The driver's five calls composed by hand: the factor chains are the series (so + n) k + j of the volatility calls."""
    prior_beta, prior_sigma_eta, prior_mu, prior_phi, prior_sigma = priors
    N, T, p = ys.shape
    k = par.k
    lit = 1 if literal else 0
    y = _dev(ys)
    beta, v = _dev(np.broadcast_to(par.beta, (N, p, k))), _dev(np.broadcast_to(par.v, (N, p)))
    sv = _dev(np.broadcast_to(par.sv(), (N, k, 3))).reshape(N * k, 3)
    svp = _lib.SvPrior(0, lit, prior_phi.mean, prior_phi.sd, prior_mu.mean, prior_mu.sd, prior_sigma_eta.shape, prior_sigma_eta.scale, 100.0, 0.05)
    fp = _lib.FsvPrior(lit, prior_beta.mean, prior_beta.sd, prior_sigma.shape, prior_sigma.scale)
    ffbs_seed = lambda c: (seed * 1000003 + c) & MASK64
    f = eng.fsv_factors(y, beta, v, None, iteration=INIT_ITERATION, seed=seed, series_offset=so, literal=literal)["f"]
    mix = eng.sv_mixture(f.reshape(N * k, T), None, iteration=0, seed=seed, series_offset=so * k)
    alpha = eng.ar1_ffbs(mix["ystar"], mix["v"], sv, seed=ffbs_seed(0), series_offset=so * k, want_filt=False)["theta"]
    states = []
    for it in range(n_iter):
        mix = eng.sv_mixture(f.reshape(N * k, T), alpha, iteration=it, seed=seed, series_offset=so * k)
        if it == 0:          # chain (n, j) = (1, 1) alone, at its own series index: the same indicators' ystar
            one = eng.sv_mixture(f[1, 1].reshape(1, T), alpha[k + 1].reshape(1, T + 1), iteration=0, seed=seed, series_offset=(so + 1) * k + 1)
            assert np.array_equal(one["ystar"].cpu().numpy()[0], mix["ystar"].cpu().numpy()[k + 1], equal_nan=True)
        alpha = eng.ar1_ffbs(mix["ystar"], mix["v"], sv, seed=ffbs_seed(it + 1), series_offset=so * k, want_filt=False)["theta"]
        sv = eng.sv_params(alpha, sv, svp, iteration=it, seed=seed, series_offset=so * k)["sv"]
        f = eng.fsv_factors(y, beta, v, alpha.reshape(N, k, T + 1), iteration=it, seed=seed, series_offset=so, literal=literal)["f"]
        ld = eng.fsv_loadings(y, f, beta, fp, iteration=it, seed=seed, series_offset=so, v=v)
        beta, v = ld["beta"], ld["v"]
        states.append(tuple(a.cpu().numpy().copy() for a in (beta, v, sv.reshape(N, k, 3), f, alpha.reshape(N, k, T + 1))))
    return states


@pytest.mark.parametrize("literal", [False, True])
def test_the_driver_is_the_five_calls_composed_by_hand(eng, literal):
    par = FsvParameters(0.5, FactorSv.build_beta(6, 2, 0.2), [SvParameters(0.8, 0.0, 0.3), SvParameters(0.6, -0.5, 0.4)])
    ys, _, _ = FactorSv.simulate(par, 40, 3, seed=11)
    ys[0, 4] = np.nan
    ys[2, 9, 1] = np.nan
    priors = (Gaussian(0.0, 1.0), InverseGamma(3.0, 0.3), Gaussian(0.0, 1.0), Gaussian(0.8, 0.1), InverseGamma(3.0, 1.0))
    want = _by_hand(eng, ys, par, priors, 3, 21, 5, literal)
    got = list(FactorSv.sample_ar(*priors, ys, par, eng, n_iter=3, seed=21, series_offset=5, literal=literal))
    assert len(got) == 3
    for s, (beta, v, sv, f, alpha) in zip(got, want):
        assert all(np.array_equal(s.params[key], a, equal_nan=True) for key, a in (("beta", beta), ("v", v), ("sv", sv)))
        assert np.array_equal(s.factors, f, equal_nan=True) and np.array_equal(s.volatility, alpha, equal_nan=True)
        assert s.status.shape == (3,) and (literal or not s.status.any())
    assert np.isnan(got[-1].factors[0, :, 4]).all() and np.isnan(got[-1].factors[2, :, 9]).all()
    light = list(FactorSv.sample_ar(*priors, ys, par, eng, n_iter=1, seed=21, series_offset=5, literal=literal, keep_factors=False))[0]
    assert light.factors is None and light.volatility is None and np.array_equal(light.params["beta"], want[0][0])


def test_a_run_on_simulated_data_prints_what_it_recovers(eng):
    truth = FsvParameters(0.25, FactorSv.build_beta(6, 2, 0.6), [SvParameters(0.8, 0.0, 0.3)] * 2)
    ys, _, _ = FactorSv.simulate(truth, 200, 32, seed=2)
    init = FsvParameters(1.0, FactorSv.make_beta(6, 2), [SvParameters(0.8, 0.0, 0.3)] * 2)
    priors = (Gaussian(0.0, 1.0), InverseGamma(3.0, 0.3), Gaussian(0.0, 1.0), Gaussian(0.8, 0.1), InverseGamma(3.0, 1.0))
    kept = [s for i, s in enumerate(FactorSv.sample_ar(*priors, ys, init, eng, n_iter=60, seed=4, keep_factors=False)) if i >= 30]
    beta = np.mean([s.params["beta"] for s in kept], axis=(0, 1))
    s2 = float(np.mean([s.params["v"] for s in kept]))
    print(f"simulated with the free loadings 0.6 and sigma^2 0.25; mean over 32 panels and the iterations 30..59:\nbeta\n{np.round(beta, 3)}\nsigma^2 {s2:.3f}")
    assert np.isfinite(beta).all() and np.isfinite(s2)          # (printed only: no assertion on what was recovered)
