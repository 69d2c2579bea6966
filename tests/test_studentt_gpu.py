"""dlm_studentt_step_batch on the GPU (StudentT.step, StudentTGibbs.scala:182-212) and the StudentT.sample driver.

The NumPy restatement of one step (`step` of tests/sampler_restatement.py) follows bayesian_dlms_amd/csrc/dlm_studentt.hip operation
for operation: the Philox stream, the Marsaglia-Tsang Gamma of gamma_unit, the Poisson sampler (inversion / PTRS), the lane-sequential
sums with their xor butterfly, and both modes.  The tests
compare the kernel with it draw for draw, then check the distributions, the nu chain's target, shard invariance and the driver."""
import math

import numpy as np
import pytest

from bayesian_dlms_amd import _lib
from bayesian_dlms_amd.dlm import Dlm, DlmParameters, materialise
from bayesian_dlms_amd.engine import Engine, EngineError
from bayesian_dlms_amd.gibbs import InverseGamma
from bayesian_dlms_amd.studentt import NegativeBinomialProposal, Poisson, StudentT
from sampler_restatement import step

PRIOR = (3.0, 1.0, 3.0, 3.0)     # Poisson(3) prior of nu, proposal size 1, InverseGamma(3, 3) prior of W: the example's


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _c3():
    return Dlm.polynomial(1) + Dlm.seasonal(24, 6)


def _inputs(d, N, T, seed, tv_f=False):
    rng = np.random.default_rng(seed)
    if d == 13:
        mat = materialise(_c3(), np.arange(1, T + 1, dtype=np.float64))
    elif tv_f:
        x = rng.standard_normal(T)
        mat = materialise(Dlm(lambda t: np.array([[x[int(t) - 1]]]), lambda dt: np.eye(1)), np.arange(1, T + 1, dtype=np.float64))
    else:
        mat = materialise(Dlm.polynomial(1), np.arange(1, T + 1, dtype=np.float64))
    theta = rng.standard_normal((N, T + 1, d))
    y = rng.standard_normal((N, T)) * 2.0 + (np.einsum("td,ntd->nt", np.asarray(mat.F).reshape(-1, d) if mat.f_stride else
                                                       np.broadcast_to(np.asarray(mat.F).reshape(1, d), (T, d)), theta[:, 1:]))
    y[rng.random((N, T)) < 0.1] = np.nan
    stats = np.concatenate([rng.random((N, 1)) * 50, np.full((N, 1), T * 0.9), rng.random((N, d)) * 20, np.full((N, 1), float(T))], axis=1)
    scale = rng.random(N) * 3 + 0.5
    nu = rng.integers(1, 9, N).astype(np.int32)
    return mat, y, theta, stats, scale, nu


@pytest.mark.gpu
@pytest.mark.parametrize("d,literal,tv_f", [(1, False, False), (1, True, False), (1, False, True), (13, False, False), (13, True, False)])
def test_draw_for_draw_against_the_numpy_restatement(eng, d, literal, tv_f):
    N, T, seed, it, off = 257, 150, 77, 5, 1000
    mat, y, theta, stats, scale, nu = _inputs(d, N, T, 11 + d, tv_f)
    acc0 = np.arange(N, dtype=np.int32)
    out = eng.studentt_step(mat, y, theta, stats, PRIOR, scale, nu, iteration=it, accepted=acc0.copy(), seed=seed,
                            series_offset=off, literal=literal)
    assert eng.last_variant == "studentt-step"
    assert (out["status"] == 0).all()
    Fm = np.asarray(mat.F).reshape(-1, d)
    for n in (0, 100, 256):
        v, s2, nu2, wd, acc, ll = step(Fm if mat.f_stride else Fm[0], y[n], theta[n], stats[n], PRIOR, scale[n], nu[n],
                                       seed=seed, series=off + n, it=it, literal=literal)
        np.testing.assert_allclose(out["v"][n], v, rtol=1e-12)
        np.testing.assert_allclose(out["scale"][n], s2, rtol=1e-12)
        np.testing.assert_allclose(out["loglik"][n], ll, rtol=1e-12)
        assert out["nu"][n] == nu2 and out["accepted"][n] == acc0[n] + acc
        np.testing.assert_allclose(np.diag(out["W"][n].reshape(d, d)), wd, rtol=1e-12)
    # W_out is dlm_dinvgamma_step_batch's W_out, bit for bit
    _, Wd = eng.dinvgamma_step(d, 1, stats, (1.0, 1.0), (PRIOR[2], PRIOR[3]), iteration=it, seed=seed, series_offset=off)
    assert np.array_equal(out["W"], Wd)
    assert 0 < (out["accepted"] - acc0).sum() < N


@pytest.mark.gpu
def test_q11_pairing_of_the_residuals(eng):
    N, T, k = 4, 40, 17
    mat = materialise(Dlm.polynomial(1), np.arange(1, T + 1, dtype=np.float64))
    theta = np.zeros((N, T + 1, 1)); theta[:, k + 1, 0] = 1e3       # the state at time k (record k + 1)
    y = np.zeros((N, T)); stats = np.ones((N, 4)); scale = np.ones(N); nu = np.full(N, 4, np.int32)
    cor = eng.studentt_step(mat, y, theta, stats, PRIOR, scale, nu, iteration=0, seed=3)["v"]
    lit = eng.studentt_step(mat, y, theta, stats, PRIOR, scale, nu, iteration=0, seed=3, literal=True)["v"]
    assert (cor[:, k] > 1e4).all() and (np.delete(cor, k, axis=1) < 1e3).all()
    assert (lit[:, k + 1] > 1e4).all() and (lit[:, k] < 1e3).all() and (np.delete(lit, k + 1, axis=1) < 1e3).all()


@pytest.mark.gpu
@pytest.mark.parametrize("literal", [False, True])
def test_variance_and_scale_draws_follow_their_conditionals(eng, literal):
    from scipy import stats as ss
    N, T = 4096, 60
    mat, y, theta, stats, scale, nu = _inputs(1, N, T, 5)
    nu[:] = 4
    out = eng.studentt_step(mat, y, theta, stats, PRIOR, scale, nu, iteration=2, seed=21, literal=literal)
    nu_v = (out["nu"] if not literal else nu).astype(np.float64)
    pair = theta[:, :-1, 0] if literal else theta[:, 1:, 0]
    e = y - pair
    obs = ~np.isnan(y)
    beta = nu_v[:, None] * scale[:, None] * 0.5 + np.where(obs, np.nan_to_num(e) ** 2 * 0.5, 0.0)
    alpha = np.where(obs | literal, (nu_v[:, None] + 1) * 0.5, nu_v[:, None] * 0.5)
    u = ss.gamma.cdf(beta / out["v"], alpha)
    assert ss.kstest(u[obs], "uniform").pvalue > 1e-3
    assert ss.kstest(u[~obs], "uniform").pvalue > 1e-3
    g = out["scale"] * nu_v / 2 * (1.0 / out["v"]).sum(axis=1)
    assert ss.kstest(ss.gamma.cdf(g, T * nu_v / 2 + 1), "uniform").pvalue > 1e-3


def _mh_stationary(literal, lam, r, K=400):
    from math import exp, lgamma, log
    lp = lambda k: k * log(lam) - lam - lgamma(k + 1)
    def lnb(frm, k):
        q = frm / (r + frm)
        return lgamma(r + k) - lgamma(k + 1) - lgamma(r) + r * log(1 - q) + k * log(q)
    off = 0 if literal else 1
    M = np.zeros((K, K))
    for a in range(1, K + 1):
        for b in range(1, K + 1):
            acc = lp(b) + lnb(b, a - off) - lp(a) - lnb(a, b - off)
            M[a - 1, b - 1] += exp(lnb(a, b - 1)) * min(1.0, exp(min(acc, 0.0)))
        M[a - 1, a - 1] += 1.0 - M[a - 1].sum()
    w, V = np.linalg.eig(M.T)
    pi = np.real(V[:, np.argmin(np.abs(w - 1))])
    return pi / pi.sum()


@pytest.mark.gpu
def test_nu_chain_targets_the_prior_without_data(eng):
    """All-missing y (ll = 0): the corrected chain's nu is Poisson(3) on nu >= 1; the literal one the stationary law of its own MH kernel."""
    import torch
    from scipy import stats as ss
    N, T, steps = 8192, 8, 300
    mat = materialise(Dlm.polynomial(1), np.arange(1, T + 1, dtype=np.float64))
    dev = torch.device("cuda", 0)
    y = torch.full((N, T), float("nan"), dtype=torch.float64, device=dev)
    theta = torch.zeros((N, T + 1, 1), dtype=torch.float64, device=dev)
    st = torch.ones((N, 4), dtype=torch.float64, device=dev)
    sc = torch.ones(N, dtype=torch.float64, device=dev)
    lam, r = PRIOR[0], PRIOR[1]
    ks = np.arange(1, 401)
    pois = np.exp(ks * np.log(lam) - lam - np.array([math.lgamma(k + 1) for k in ks])); pois /= pois.sum()
    lit_pi = _mh_stationary(True, lam, r)
    tv = 0.5 * np.abs(lit_pi - pois).sum()
    assert tv > 0.05, tv                  # the two targets differ by far more than the sampling noise of 8192 chains (~0.01)
    def binned(p):
        return np.concatenate([p[:7], [p[7:].sum()]])
    for literal, target in ((False, pois), (True, lit_pi)):
        nu = torch.as_tensor(np.random.default_rng(1).poisson(lam, N).clip(1).astype(np.int32), device=dev)
        for it in range(steps):
            nu = eng.studentt_step(mat, y, theta, st, PRIOR, sc, nu, iteration=it, seed=8, literal=literal)["nu"]
        h = np.bincount(np.minimum(nu.cpu().numpy(), 8), minlength=9)[1:]
        assert ss.chisquare(h, binned(target) * N).pvalue > 1e-3, (literal, h, binned(target) * N)
        if literal:     # and the literal histogram is not Poisson's
            assert ss.chisquare(h, binned(pois) * N).pvalue < 1e-6


@pytest.mark.gpu
def test_shard_and_memory_mode_invariance(eng):
    import torch
    N, T = 257, 120
    mat, y, theta, stats, scale, nu = _inputs(13, N, T, 3)
    full = eng.studentt_step(mat, y, theta, stats, PRIOR, scale, nu, iteration=4, seed=5, series_offset=10)
    h = 100
    a = eng.studentt_step(mat, y[:h], theta[:h], stats[:h], PRIOR, scale[:h], nu[:h], iteration=4, seed=5, series_offset=10)
    b = eng.studentt_step(mat, y[h:], theta[h:], stats[h:], PRIOR, scale[h:], nu[h:], iteration=4, seed=5, series_offset=10 + h)
    T_ = lambda x: torch.as_tensor(x, device="cuda:0")
    dv = eng.studentt_step(mat, T_(y), T_(theta), T_(stats), PRIOR, T_(scale), T_(nu), iteration=4, seed=5, series_offset=10)
    for key in ("v", "scale", "nu", "W", "accepted", "loglik"):
        assert np.array_equal(full[key], np.concatenate([a[key], b[key]]), equal_nan=True), key
        assert np.array_equal(full[key], dv[key].cpu().numpy(), equal_nan=True), key


@pytest.mark.gpu
def test_nonfinite_inputs_are_flagged(eng):
    N, T = 6, 30
    mat, y, theta, stats, scale, nu = _inputs(1, N, T, 9)
    nu[1] = 0; scale[2] = np.nan; theta[3, 7, 0] = np.inf
    out = eng.studentt_step(mat, y, theta, stats, PRIOR, scale, nu, iteration=0, seed=1)
    assert list(out["status"]) == [0, 1, 1, 1, 0, 0]
    for n in (1, 2, 3):
        assert np.isnan(out["v"][n]).all() and np.isnan(out["scale"][n]) and np.isnan(out["loglik"][n]) and out["nu"][n] == nu[n]
    assert np.isfinite(out["v"][[0, 4, 5]]).all()


def _simulate_local_level(N, T, s, W, nu, seed):
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.normal(0.0, math.sqrt(W), (N, T)), axis=1)
    v = (nu * s / 2) / rng.gamma(nu / 2, 1.0, (N, T))
    return x + rng.standard_normal((N, T)) * np.sqrt(v)


@pytest.mark.gpu
@pytest.mark.parametrize("simsmooth", [False, True])
def test_end_to_end_recovers_the_simulation(eng, simsmooth):
    """512 local-level series, T = 400, s = 3, W = 0.1, nu = 3.  Series-averaged posterior means after 100 iterations of burn-in.
    Tolerances: the averages over 512 series leave little Monte Carlo noise (each series' posterior sd of s is ~0.5, of W ~0.03,
    of nu ~1: /sqrt(512) gives 0.02, 0.0015, 0.05); what remains is the posterior's own shrinkage towards the priors at T = 400
    (W ~ InverseGamma(2, 0.2): +1 %, s: its shape + 1, nu: Poisson(3) centred on the truth), a few per cent.  15 % on s and W and
    0.5 on nu leave room for both and still fail a sampler that targets the wrong law (literal Q10-Q15 moves s by 30 % here)."""
    N, T = 512, 400
    y = _simulate_local_level(N, T, 3.0, 0.1, 3.0, seed=12)
    p0 = DlmParameters([[1.0]], [[1.0]], [0.0], [[10.0]])
    ss_, ww, nn = [], [], []
    for k, st in enumerate(StudentT.sample(y, InverseGamma(2.0, 0.2), Poisson(3.0), NegativeBinomialProposal(1.0), Dlm.polynomial(1),
                                           p0, eng, n_iter=300, seed=2, simulation_smoother=simsmooth)):
        assert (st.status == 0).all()
        if k >= 100:
            ss_.append(st.p.scale); ww.append(st.p.w_diag()[:, 0]); nn.append(st.nu)
    s_m, w_m, n_m = np.mean(ss_), np.mean(ww), np.mean(nn)
    print(f"posterior means: s {s_m:.4f}  W {w_m:.5f}  nu {n_m:.3f}  accepted {st.accepted.mean():.1f} / 300")
    assert abs(s_m - 3.0) < 0.45 and abs(w_m - 0.1) < 0.015 and abs(n_m - 3.0) < 0.5, (s_m, w_m, n_m)
    assert 10 < st.accepted.mean() < 290


@pytest.mark.gpu
def test_c3_shape_runs_and_stays_finite(eng):
    import torch
    N, T = 64, 200
    rng = np.random.default_rng(4)
    y = torch.as_tensor(rng.standard_t(3, (N, T)).cumsum(axis=1) * 0.1, device="cuda:0")
    p0 = DlmParameters([[1.0]], np.eye(13) * 0.1, np.zeros(13), np.eye(13) * 10)
    for st in StudentT.sample(y, InverseGamma(3.0, 3.0), Poisson(3.0), NegativeBinomialProposal(1.0), _c3(), p0, eng, n_iter=4,
                              seed=1, keep_theta=True, keep_variances=True):
        assert st.theta.shape == (N, T + 1, 13) and st.variances.shape == (N, T) and st.p.w_diag().shape == (N, 13)
        assert np.isfinite(st.theta).all() and np.isfinite(st.variances).all() and np.isfinite(st.p.scale).all()
        assert (st.status == 0).all() and (st.nu >= 1).all()


@pytest.mark.gpu
def test_refusals(eng):
    N, T = 4, 20
    rng = np.random.default_rng(0)
    mat2 = materialise(Dlm.polynomial(1).outer(Dlm.polynomial(1)), np.arange(1, T + 1, dtype=np.float64))   # p = 2
    with pytest.raises(EngineError):
        eng.studentt_step(mat2, rng.standard_normal((N, T)), np.zeros((N, T + 1, 2)), np.ones((N, 7)), PRIOR, np.ones(N),
                          np.full(N, 3, np.int32), iteration=0)
    import ctypes
    md = _lib.ModelDesc(2, 2, T, N, ctypes.c_void_p(mat2.F.ctypes.data).value, 0, None, 1, None, None)
    y = np.zeros(N * T * 2); th = np.zeros(N * (T + 1) * 2); stt = np.ones(N * 7); sc = np.ones(N); nu = np.full(N, 3, np.int32)
    outs = [np.zeros(N * T), np.zeros(N), np.zeros(N, np.int32), np.zeros(N * 4), np.zeros(N, np.int32)]
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    pr = _lib.StudentTPrior(*PRIOR)
    rc = eng.lib.dlm_studentt_step_batch(eng.h, md, P(y), P(th), P(stt), pr, P(sc), P(nu), 0, _lib.Options(0, _lib.DLM_MEM_HOST, 0, 0),
                                         *[P(o) for o in outs], None, None)
    assert rc == -3     # DLM_ERR_UNSUPPORTED
    mat, y, theta, stats, scale, nu = _inputs(1, N, T, 2, tv_f=True)
    assert mat.f_stride != 0
    with pytest.raises(EngineError, match="Q11"):
        eng.studentt_step(mat, y, theta, stats, PRIOR, scale, nu, iteration=0, literal=True)
    out = eng.studentt_step(mat, y, theta, stats, PRIOR, scale, nu, iteration=0)     # the corrected mode takes it
    assert (out["status"] == 0).all()
