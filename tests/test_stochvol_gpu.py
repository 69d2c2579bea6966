"""dlm_sv_mixture_batch / dlm_sv_params_batch on the GPU (StochasticVolatility.sampleKt, samplePhiConjugate / samplePhi, sampleMu,
sampleSigma) and the StochasticVolatility.sample_uni / sample_beta drivers.

First a NumPy restatement of both kernels (bayesian_dlms_amd/csrc/dlm_sv.hip), operation for operation and in the same summation
order: the mixture call's is here, the parameter call's (`params_step`) and the draws it is built on come from
tests/sampler_restatement.py.  The tests compare the kernels with it draw for draw, then check the distributions, the Beta chain's
target, the invariances and the drivers.

On the shapes of the draw-for-draw parameter test: with T = 2 the default sums hold the two pairs (alpha_0, alpha_1), (alpha_1, alpha_2)
and the literal ones the single pair (alpha_1, alpha_2) that `alphas.tail.init zip alphas.drop(2)` leaves -- the smallest T the
reference does not throw on."""
import math

import numpy as np
import pytest

from bayesian_dlms_amd import _lib
from bayesian_dlms_amd.engine import Engine, EngineError
from bayesian_dlms_amd.gibbs import InverseGamma
from bayesian_dlms_amd.stochvol import Beta, Gaussian, StochasticVolatility, SvParameters
from sampler_restatement import KEY_SV, gibbs_rand, params_step
from sampler_restatement import sv_prior as prior, sv_prior_tuple as as_tuple

# the mixture of Kim, Shephard & Chib as StochasticVolatility.scala:42-44 has it
PIS = np.array([0.0073, 0.1056, 0.00002, 0.044, 0.34, 0.2457, 0.2575])
MEANS = np.array([-11.4, -5.24, -9.84, 1.51, -0.65, 0.53, -2.36])
VARS = np.array([5.8, 2.61, 5.18, 0.17, 0.64, 0.34, 1.26])
LP = np.array([math.log(p) for p in PIS])
C = np.array([math.log(p) - 0.5 * math.log(2.0 * math.pi * v) for p, v in zip(PIS, VARS)])
H = 1.0 / (2.0 * VARS)
RTOL, ATOL = 1e-11, 1e-12


# ------------------------------------------------------------------------------------------------------------------------------
# the restatement
def mixture_weights(y, alpha):
    """(ly, obs, degenerate, p [N][T][7]): the cumulative weights p_j = w_0 + ... + w_j of every element."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ly = np.log(y * y)
    seen = ~np.isnan(y)
    degenerate = seen & ~np.isfinite(ly)
    obs = seen & ~degenerate
    x = alpha[:, 1:]
    with np.errstate(invalid="ignore"):
        r = (ly[..., None] - MEANS) - x[..., None]
        lw = np.where(obs[..., None], C - r * r * H, LP)
    mx = lw.max(axis=-1)
    p = np.empty_like(lw)
    c = np.zeros(y.shape)
    for j in range(7):
        c = c + np.exp(lw[..., j] - mx)
        p[..., j] = c
    return ly, obs, degenerate, p


def mixture(y, alpha, *, seed, series_offset, it):
    """-> (ystar, v, k, status, margin): margin = min_j |u S - p_j| / S, how far the draw stands from a boundary."""
    N, T = y.shape
    ly, obs, degenerate, p = mixture_weights(y, alpha)
    u = np.stack([gibbs_rand(seed, series_offset + n, it, np.arange(T), 0, 0, KEY_SV)[1] for n in range(N)])
    us = u * p[..., 6]
    k = (us[..., None] >= p[..., :6]).sum(axis=-1)
    margin = np.abs(us[..., None] - p[..., :6]).min(axis=-1) / p[..., 6]
    ystar = np.where(obs, ly - MEANS[k], np.nan)
    return ystar, VARS[k], k, np.where(degenerate.any(axis=1), _lib.ST_NONFINITE, 0), margin


# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def shared_alpha():
    """One simulated state path (T = 65, phi = 0.8, mu = 1, sigma = 0.3): the tests of the conditionals share it."""
    _, alpha = StochasticVolatility.simulate(SvParameters(0.8, 1.0, 0.3), 65, 1, seed=5)
    alpha.setflags(write=False)
    return alpha[0]


def _mixture_inputs(N, T, seed):
    rng = np.random.default_rng(seed)
    y = np.exp(rng.uniform(math.log(1e-8), math.log(1e3), (N, T))) * rng.choice([-1.0, 1.0], (N, T))
    y[rng.random((N, T)) < 0.1] = np.nan
    alpha = rng.uniform(-12.0, 6.0, (N, T + 1))
    zero, tiny = (0, 0), (N - 1, T - 1)
    y[zero] = 0.0
    y[tiny] = 1e-200
    return y, alpha, zero, tiny


@pytest.mark.gpu
@pytest.mark.parametrize("N,T", [(1, 2), (3, 64), (67, 129)])
def test_mixture_draw_for_draw(eng, N, T):
    seed, it, off = 77, 5, 1000
    y, alpha, zero, tiny = _mixture_inputs(N, T, 3 + N)
    out = eng.sv_mixture(y, alpha, iteration=it, seed=seed, series_offset=off, want_k=True)
    assert eng.last_variant == "sv-mixture"
    ystar, v, k, status, margin = mixture(y, alpha, seed=seed, series_offset=off, it=it)
    assert out["k"].dtype == np.int8
    # the device's exp / log may differ from NumPy's in the last bits: k is compared where the draw stands clear of a boundary
    # (expected number of elements inside the band: 7 x 2e-9 x N T < 1e-4)
    clear = margin > 1e-9
    print(f"N={N} T={T}: {(~clear).sum()} element(s) within 1e-9 S of a boundary, smallest margin {margin.min():.3e}")
    assert (~clear).sum() <= 1
    assert np.array_equal(out["k"][clear], k[clear])
    same = clear & (out["k"] == k)
    np.testing.assert_allclose(out["ystar"][same], ystar[same], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(out["v"][same], v[same], rtol=RTOL, atol=ATOL)
    assert np.isin(out["v"], VARS).all() and ((out["k"] >= 0) & (out["k"] <= 6)).all()
    # missing steps (and the two degenerate observations, treated as missing): ystar NaN, k drawn from the prior weights
    missing = np.isnan(y)
    missing[zero] = missing[tiny] = True
    assert np.isnan(out["ystar"][missing]).all() and not np.isnan(out["ystar"][~missing]).any()
    _, _, _, p = mixture_weights(y, alpha)
    np.testing.assert_allclose(p[missing] / p[missing][:, 6:], np.broadcast_to(np.cumsum(PIS) / PIS.sum(), p[missing].shape), rtol=1e-12)
    want = np.zeros(N, np.int32)
    want[zero[0]] = want[tiny[0]] = _lib.ST_NONFINITE
    assert np.array_equal(out["status"], want) and np.array_equal(status, want)
    # alpha = None: the initial transform
    init = eng.sv_mixture(y, None, iteration=it, seed=seed, series_offset=off, want_k=True)
    with np.errstate(divide="ignore"):
        np.testing.assert_allclose(init["ystar"][~missing], np.log(y[~missing] ** 2) + 1.27, rtol=RTOL, atol=ATOL)
    assert np.isnan(init["ystar"][missing]).all() and init["k"] is None
    assert (init["v"] == math.pi ** 2 / 2).all() and np.array_equal(init["status"], want)


@pytest.mark.gpu
def test_mixture_frequencies(eng):
    n, T = 8192, 4
    alpha_row = np.array([0.0, -1.0, 0.5, 2.0, -3.0])
    gaps = np.array([-9.0, -3.0, 0.0, 1.5])                       # log y^2 - alpha: every component carries weight somewhere
    y_row = np.exp(0.5 * (alpha_row[1:] + gaps))
    y, alpha = np.tile(y_row, (n, 1)), np.tile(alpha_row, (n, 1))
    out = eng.sv_mixture(y, alpha, iteration=0, seed=5, want_k=True)
    _, _, _, p = mixture_weights(y[:1], alpha[:1])
    w = np.diff(np.concatenate([np.zeros((T, 1)), p[0]], axis=1), axis=1) / p[0][:, 6:]
    for t in range(T):
        freq = np.bincount(out["k"][:, t], minlength=7) / n
        bound = 5.0 * np.sqrt(w[t] * (1.0 - w[t]) / n) + 2.0 / n
        print(f"t={t} freq={np.round(freq, 4)} p={np.round(w[t], 4)}")
        assert (np.abs(freq - w[t]) <= bound).all(), (t, freq, w[t])


def _params_inputs(N, T, seed, flat=False):
    rng = np.random.default_rng(seed)
    sv = np.stack([rng.uniform(0.1, 0.95, N), rng.uniform(-1.0, 2.0, N), rng.uniform(0.1, 0.5, N)], axis=1)
    alpha = np.empty((N, T + 1))
    alpha[:, 0] = sv[:, 1] + sv[:, 2] * rng.standard_normal(N)
    for t in range(T):
        alpha[:, t + 1] = sv[:, 1] + sv[:, 0] * (alpha[:, t] - sv[:, 1]) + sv[:, 2] * rng.standard_normal(N)
    if flat:      # next to no information about phi: its conditional is its prior
        alpha = sv[:, 1:2] + 1e-3 * sv[:, 2:3] * rng.standard_normal((N, T + 1))
    return alpha, sv


def _compare_params(eng, alpha, sv, pr, *, seed, it, off):
    N = alpha.shape[0]
    acc0 = np.arange(N, dtype=np.int32)
    out = eng.sv_params(alpha, sv, as_tuple(pr), iteration=it, accepted=acc0.copy(), seed=seed, series_offset=off)
    assert eng.last_variant == "sv-params"
    ref = [params_step(alpha[n], sv[n], pr, seed=seed, series=off + n, it=it) for n in range(N)]
    np.testing.assert_allclose(out["sv"], np.array([r[:3] for r in ref]), rtol=RTOL)
    assert np.array_equal(out["accepted"], acc0 + np.array([r[3] for r in ref]))
    assert np.array_equal(out["status"], np.array([r[4] for r in ref]))
    return out, ref


@pytest.mark.gpu
@pytest.mark.parametrize("N,T", [(5, 2), (67, 65), (4, 129), (3, 1000)])
@pytest.mark.parametrize("phi_update,literal", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_params_draw_for_draw(eng, N, T, phi_update, literal):
    alpha, sv = _params_inputs(N, T, 11 + T)
    pr = prior(phi_update, literal, 5.0, 2.0) if phi_update else prior(phi_update, literal, 0.8, 0.3)
    out, ref = _compare_params(eng, alpha, sv, pr, seed=77, it=5, off=1000)
    assert np.isfinite(out["sv"]).all() and (out["sv"][:, 2] > 0.0).all()
    if not literal:
        assert (np.abs(out["sv"][:, 0]) < 1.0).all()
    if phi_update:
        assert ((out["sv"][:, 0] > 0.0) & (out["sv"][:, 0] < 1.0)).all()


@pytest.mark.gpu
def test_params_rejection_of_nonstationary_phi_and_the_literal_draw_beyond_one(eng):
    N, T = 67, 65
    alpha, sv = _params_inputs(N, T, 3, flat=True)
    # corrected: the conditional is about N(0.99, 0.5^2), so that the restriction to (-1, 1) rejects about every second attempt
    out, ref = _compare_params(eng, alpha, sv, prior(0, 0, 0.99, 0.5), seed=9, it=2, off=0)
    attempts = np.array([r[5] for r in ref])
    assert (attempts > 1).sum() >= 10 and attempts.max() >= 3
    assert (np.abs(out["sv"][:, 0]) < 1.0).all() and (out["status"] == 0).all()
    # literal (Q19): the same conditional unrestricted; the FFBS that follows flags the chains it sent beyond the unit interval
    lit, _ = _compare_params(eng, alpha, sv, prior(0, 1, 0.99, 0.5), seed=9, it=2, off=0)
    beyond = np.abs(lit["sv"][:, 0]) >= 1.0
    assert 5 <= beyond.sum() <= N - 5 and (lit["status"] == 0).all()
    y = np.random.default_rng(1).standard_normal((N, T))
    f = eng.ar1_ffbs(y, np.ones((N, T)), lit["sv"], seed=1, want_filt=False)
    assert np.array_equal((f["status"] & _lib.ST_NOT_PD) != 0, beyond)


@pytest.mark.gpu
@pytest.mark.parametrize("phi_update", [0, 1])
def test_params_in_place_and_bad_rows(eng, phi_update):
    import torch
    N, T = 67, 65
    alpha, sv = _params_inputs(N, T, 4)
    pr = as_tuple(prior(1, 0, 5.0, 2.0) if phi_update else prior(0, 0, 0.8, 0.3))
    ref = eng.sv_params(alpha, sv, pr, iteration=1, seed=3)
    # in place: host arrays, then device tensors
    svh = sv.copy()
    out = eng.sv_params(alpha, svh, pr, iteration=1, seed=3, out={"sv": svh})
    assert out["sv"] is svh and np.array_equal(svh, ref["sv"])
    ad, svd = torch.as_tensor(alpha, device="cuda:0"), torch.as_tensor(sv, device="cuda:0")
    out = eng.sv_params(ad, svd, pr, iteration=1, seed=3, out={"sv": svd})
    assert out["sv"] is svd and np.array_equal(svd.cpu().numpy(), ref["sv"])
    # bad rows: status and NaN, the neighbours untouched
    bad = sv.copy()
    bad[1, 0] = np.nan; bad[3, 2] = 0.0; bad[5, 2] = -0.3; bad[7, 1] = np.inf; bad[9, 2] = np.inf
    rows = [1, 3, 5, 7, 9]
    if phi_update:
        bad[11, 0] = 1.2; bad[13, 0] = -0.5; bad[15, 0] = 0.0
        rows += [11, 13, 15]
    out = eng.sv_params(alpha, bad, pr, iteration=1, seed=3)
    good = np.setdiff1d(np.arange(N), rows)
    assert (out["status"][rows] == _lib.ST_NONFINITE).all() and np.isnan(out["sv"][rows]).all() and (out["accepted"][rows] == 0).all()
    assert (out["status"][good] == 0).all() and np.array_equal(out["sv"][good], ref["sv"][good])


@pytest.mark.gpu
def test_argument_errors(eng):
    alpha, sv = _params_inputs(4, 8, 1)
    y = np.ones((4, 8))
    ok = prior(0, 0, 0.8, 0.3)
    with pytest.raises(EngineError):
        eng.sv_mixture(y[:, :1], alpha[:, :2], iteration=0)                       # T < 2
    with pytest.raises(EngineError):
        eng.sv_params(alpha[:, :2], sv, as_tuple(ok), iteration=0)                # T < 2
    for change in (dict(phi_update=2), dict(literal=2), dict(phi_b=0.0), dict(mu_sd=-1.0), dict(sigma_shape=0.0), dict(sigma_scale=-2.0),
                   dict(phi_update=1, phi_a=0.0), dict(phi_update=1, phi_a=2.0, phi_b=-1.0), dict(phi_update=1, phi_a=2.0, phi_b=2.0, prop_tau=0.0),
                   dict(phi_update=1, phi_a=2.0, phi_b=2.0, prop_lambda=-1.0)):
        with pytest.raises(EngineError):
            eng.sv_params(alpha, sv, as_tuple({**ok, **change}), iteration=0)
    lib, h = eng.lib, eng.h
    op = _lib.Options(0, _lib.DLM_MEM_HOST, 0, 0)
    assert lib.dlm_sv_mixture_batch(h, 4, (1 << 21) - 8, None, None, 0, op, None, None, None, None) == -1
    assert lib.dlm_sv_params_batch(h, 4, (1 << 21) - 8, None, None, _lib.SvPrior(*as_tuple(ok)), 0, op, None, None, None) == -1
    assert lib.dlm_sv_mixture_batch(h, 0, 8, None, None, 0, op, None, None, None, None) == -1


@pytest.mark.gpu
def test_params_follow_their_conditionals(eng, shared_alpha):
    from scipy import stats as ss
    n, T = 8192, 65
    al = shared_alpha
    alpha = np.tile(al, (n, 1))
    phi0, mu0, sig0 = 0.8, 1.0, 0.3
    sv = np.tile([phi0, mu0, sig0], (n, 1))
    pr = prior(0, 0, 0.8, 0.2, mu=(1.0, 1.0), sigma=(5.0, 0.5))
    out = eng.sv_params(alpha, sv, as_tuple(pr), iteration=0, seed=12)
    assert (out["status"] == 0).all()
    phi, mu, sig = out["sv"].T
    s2 = sig0 * sig0
    prev, cur = al[:-1], al[1:]
    # phi: N(mean, 1 / prec) restricted to (-1, 1)
    prec = 1.0 / 0.2 ** 2 + ((prev - mu0) ** 2).sum() / s2
    mean = (0.8 / 0.2 ** 2 + ((prev - mu0) * (cur - mu0)).sum() / s2) / prec
    sd = 1.0 / math.sqrt(prec)
    m, var, _, kurt = ss.truncnorm.stats((-1.0 - mean) / sd, (1.0 - mean) / sd, loc=mean, scale=sd, moments="mvsk")
    se_m, se_v = math.sqrt(var / n), math.sqrt(((kurt + 3.0) * var * var - var * var) / n)
    print(f"phi: mean {phi.mean():.5f} (target {m:.5f}, se {se_m:.1e}), var {phi.var():.3e} (target {var:.3e}, se {se_v:.1e})")
    assert abs(phi.mean() - m) <= 5 * se_m and abs(phi.var() - var) <= 5 * se_v
    # mu against its own drawn phi, standardised
    mprec = 1.0 + T * (1.0 - phi) ** 2 / s2
    mmean = (1.0 + (1.0 - phi) / s2 * (cur[None, :] - phi[:, None] * prev[None, :]).sum(axis=1)) / mprec
    z = (mu - mmean) * np.sqrt(mprec)
    print(f"mu: standardised mean {z.mean():.4f}, var {z.var():.4f}")
    assert abs(z.mean()) <= 5 / math.sqrt(n) and abs(z.var() - 1.0) <= 5 * math.sqrt(2.0 / n)
    # 1 / sigma^2 ~ Gamma(shape', rate = scale') given the drawn phi and mu: g = scale' / sigma^2 ~ Gamma(shape', 1)
    r = (cur[None, :] - mu[:, None]) - phi[:, None] * (prev[None, :] - mu[:, None])
    k = 5.0 + T / 2.0
    g = (0.5 + 0.5 * (r * r).sum(axis=1)) / (sig * sig)
    print(f"1/sigma^2: standardised mean {g.mean():.4f} (shape {k}), var {g.var():.4f}")
    assert abs(g.mean() - k) <= 5 * math.sqrt(k / n) and abs(g.var() - k) <= 5 * math.sqrt((2.0 * k * k + 6.0 * k) / n)


@pytest.mark.gpu
def test_beta_metropolis_hastings_leaves_its_target_invariant(eng, shared_alpha):
    n, T = 8192, 65
    al = shared_alpha
    mu, sig, a, b = 1.0, 0.3, 5.0, 2.0
    s2 = sig * sig
    grid = np.linspace(0.0, 1.0, 20001)
    g = grid[1:-1]
    d = al - mu
    Q = ((d[1:, None] - g[None, :] * d[:-1, None]) ** 2).sum(axis=0)
    lt = ((a - 1.0) * np.log(g) + (b - 1.0) * np.log(1.0 - g) + 0.5 * np.log(1.0 - g * g) - 0.5 * d[0] ** 2 * (1.0 - g * g) / s2
          - 0.5 * Q / s2)
    dens = np.concatenate([[0.0], np.exp(lt - lt.max()), [0.0]])
    cdf = np.concatenate([[0.0], np.cumsum(0.5 * (dens[1:] + dens[:-1]))])
    cdf /= cdf[-1]
    w = dens / dens.sum()
    m1, m2 = (w * grid).sum(), (w * grid ** 2).sum()
    se1, se2 = math.sqrt(((w * grid ** 2).sum() - m1 ** 2) / n), math.sqrt(((w * grid ** 4).sum() - m2 ** 2) / n)
    start = np.interp(np.random.default_rng(8).random(n), cdf, grid)
    assert abs(start.mean() - m1) <= 5 * se1
    sv = np.stack([start, np.full(n, mu), np.full(n, sig)], axis=1)
    out = eng.sv_params(np.tile(al, (n, 1)), sv, as_tuple(prior(1, 0, a, b)), iteration=0, seed=31)
    assert (out["status"] == 0).all()
    phi = out["sv"][:, 0]
    acc = int(out["accepted"].sum())
    print(f"phi: mean {phi.mean():.5f} (target {m1:.5f}, se {se1:.1e}), mean of squares {np.mean(phi ** 2):.5f} (target {m2:.5f}, "
          f"se {se2:.1e}), accepted {acc} of {n}")
    assert abs(phi.mean() - m1) <= 5 * se1 and abs(np.mean(phi ** 2) - m2) <= 5 * se2
    assert 0 < acc < n
    moved = phi != start
    assert np.array_equal(moved, out["accepted"] == 1)


@pytest.mark.gpu
def test_invariances_bit_for_bit(eng):
    import torch
    N, T, seed, it = 160, 129, 6, 3
    y, alpha, _, _ = _mixture_inputs(N, T, 21)
    full = eng.sv_mixture(y, alpha, iteration=it, seed=seed, want_k=True)
    part = eng.sv_mixture(y[100:], alpha[100:], iteration=it, seed=seed, series_offset=100, want_k=True)
    again = eng.sv_mixture(y, alpha, iteration=it, seed=seed, want_k=True)
    dev = eng.sv_mixture(torch.as_tensor(y, device="cuda:0"), torch.as_tensor(alpha, device="cuda:0"), iteration=it, seed=seed, want_k=True)
    for key in ("ystar", "v", "k", "status"):
        assert np.array_equal(full[key][100:], part[key], equal_nan=key == "ystar"), key
        assert np.array_equal(full[key], again[key], equal_nan=key == "ystar"), key
        assert np.array_equal(full[key], dev[key].cpu().numpy(), equal_nan=key == "ystar"), key
    other = eng.sv_mixture(y, alpha, iteration=it + 1, seed=seed, want_k=True)
    assert (other["k"] != full["k"]).mean() > 0.2
    alpha, sv = _params_inputs(N, T, 22)
    for pr in (as_tuple(prior(0, 0, 0.8, 0.3)), as_tuple(prior(1, 0, 5.0, 2.0)), as_tuple(prior(0, 1, 0.8, 0.3)), as_tuple(prior(1, 1, 5.0, 2.0))):
        full = eng.sv_params(alpha, sv, pr, iteration=it, seed=seed)
        part = eng.sv_params(alpha[100:], sv[100:], pr, iteration=it, seed=seed, series_offset=100)
        again = eng.sv_params(alpha, sv, pr, iteration=it, seed=seed)
        dev = eng.sv_params(torch.as_tensor(alpha, device="cuda:0"), torch.as_tensor(sv, device="cuda:0"), pr, iteration=it, seed=seed)
        for key in ("sv", "accepted", "status"):
            assert np.array_equal(full[key][100:], part[key]), key
            assert np.array_equal(full[key], again[key]), key
            assert np.array_equal(full[key], dev[key].cpu().numpy()), key


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["uni", "beta"])
def test_driver_equals_the_three_calls_composed_by_hand(eng, kind):
    N, T, seed, off, n_iter = 67, 129, 5, 40, 3
    y, _ = StochasticVolatility.simulate(SvParameters(0.8, 1.0, 0.3), T, N, seed=2)
    y[3, 10:14] = np.nan
    y[5, 7] = 0.0                              # Q20: a status the mixture call reports at every iteration
    p0 = SvParameters(0.7, 0.5, 0.4)
    pmu, psig = Gaussian(1.0, 2.0), InverseGamma(3.0, 0.5)
    if kind == "uni":
        gen = StochasticVolatility.sample_uni(y, Gaussian(0.8, 0.3), pmu, psig, eng, n_iter=n_iter, seed=seed, params0=p0,
                                              series_offset=off, keep_alpha=True)
        pr = as_tuple(prior(0, 0, 0.8, 0.3, mu=(1.0, 2.0), sigma=(3.0, 0.5)))
    else:
        gen = StochasticVolatility.sample_beta(y, Beta(5.0, 2.0), pmu, psig, eng, n_iter=n_iter, seed=seed, params0=p0,
                                               series_offset=off, keep_alpha=True)
        pr = as_tuple(prior(1, 0, 5.0, 2.0, mu=(1.0, 2.0), sigma=(3.0, 0.5)))
    states = list(gen)
    assert len(states) == n_iter
    sv = np.tile([0.7, 0.5, 0.4], (N, 1))
    mix = eng.sv_mixture(y, None, iteration=0, seed=seed, series_offset=off)
    f = eng.ar1_ffbs(mix["ystar"], mix["v"], sv, seed=seed * 1000003, series_offset=off, want_filt=False)
    alpha, acc = f["theta"], np.zeros(N, np.int32)
    status = mix["status"] | f["status"]
    for it in range(n_iter):
        mix = eng.sv_mixture(y, alpha, iteration=it, seed=seed, series_offset=off)
        f = eng.ar1_ffbs(mix["ystar"], mix["v"], sv, seed=seed * 1000003 + it + 1, series_offset=off, want_filt=False)
        alpha = f["theta"]
        res = eng.sv_params(alpha, sv, pr, iteration=it, accepted=acc, seed=seed, series_offset=off)
        sv, acc = res["sv"], res["accepted"]
        status = status | mix["status"] | f["status"] | res["status"]
        assert np.array_equal(states[it].params, sv) and np.array_equal(states[it].alpha, alpha)
        assert np.array_equal(states[it].accepted, acc) and np.array_equal(states[it].status, status)
        assert states[it].status[5] & _lib.ST_NONFINITE
        status = np.zeros(N, np.int32)
    assert np.isfinite(states[-1].params).all()
    if kind == "beta":
        assert 0 < states[-1].accepted.sum() < n_iter * N
    else:
        assert (states[-1].accepted == 0).all()
    nokeep = next(StochasticVolatility.sample_uni(y, Gaussian(0.8, 0.3), pmu, psig, eng, n_iter=1, seed=seed, params0=p0, series_offset=off))
    assert nokeep.alpha is None


@pytest.mark.gpu
def test_driver_recovers_simulated_parameters_printed_only(eng):
    """Not asserted beyond finiteness: the posterior means of a 64-series, T = 500, 300-iteration run on data simulated at
    (phi, mu, sigma) = (0.8, 1.0, 0.3) are printed."""
    N, T, n_iter, burn = 64, 500, 300, 100
    y, _ = StochasticVolatility.simulate(SvParameters(0.8, 1.0, 0.3), T, N, seed=4)
    for kind in ("uni", "beta"):
        if kind == "uni":
            gen = StochasticVolatility.sample_uni(y, Gaussian(0.8, 0.1), Gaussian(1.0, 1.0), InverseGamma(2.0, 2.0), eng, n_iter=n_iter, seed=1)
        else:
            gen = StochasticVolatility.sample_beta(y, Beta(5.0, 2.0), Gaussian(1.0, 1.0), InverseGamma(2.0, 2.0), eng, n_iter=n_iter, seed=1)
        draws = np.stack([s.params for s in gen])
        post = draws[burn:].mean(axis=0)
        print(f"sample_{kind}: posterior means over {N} series: phi {post[:, 0].mean():.3f} (sd over series {post[:, 0].std():.3f}), "
              f"mu {post[:, 1].mean():.3f} ({post[:, 1].std():.3f}), sigma {post[:, 2].mean():.3f} ({post[:, 2].std():.3f}); simulated at 0.8, 1.0, 0.3")
        assert np.isfinite(draws).all()


# ------------------------------------------------------------------------------------------------------------------------------
# the pairing of the mixture draw with the state draw: y[t] belongs to alpha[t + 1] across dlm_sv_mixture_batch -> dlm_ar1_ffbs_batch
INV_SV = (0.8, 1.0, 0.3)


def _invariance_data(N=16384, T=17, seed=2024):
    """(y [N][T], alpha [N][T+1]) from the model the mixture sampler targets, on the host: alpha the stationary AR(1) path,
    k_t ~ pi (the weights as the kernel normalises them), log y_t^2 = alpha_{t+1} + m_k + sqrt(v_k) eps, y_t = +- exp(log y_t^2 / 2)."""
    phi, mu, sigma = INV_SV
    rng = np.random.default_rng(seed)
    alpha = np.empty((N, T + 1))
    alpha[:, 0] = mu + sigma / math.sqrt(1.0 - phi * phi) * rng.standard_normal(N)
    for t in range(T):
        alpha[:, t + 1] = mu + phi * (alpha[:, t] - mu) + sigma * rng.standard_normal(N)
    k = rng.choice(7, size=(N, T), p=PIS / PIS.sum())
    ly = alpha[:, 1:] + MEANS[k] + np.sqrt(VARS[k]) * rng.standard_normal((N, T))
    return rng.choice([-1.0, 1.0], (N, T)) * np.exp(0.5 * ly), alpha


def _invariance_checks(y, alpha_new):
    """The assertions of test_mixture_then_state_draw_leaves_the_joint_law_invariant on a new state draw (tools and rehearsals call it too)."""
    from scipy import special, stats as ss
    phi, mu, sigma = INV_SV
    N, T = y.shape
    e = np.empty_like(alpha_new)                  # whitened: iid N(0, 1) under the stationary AR(1) law
    e[:, 0] = (alpha_new[:, 0] - mu) * math.sqrt(1.0 - phi * phi) / sigma
    e[:, 1:] = (alpha_new[:, 1:] - mu - phi * (alpha_new[:, :-1] - mu)) / sigma
    mean, var, lag = e.mean(axis=0), e.var(axis=0), (e[:, 1:] * e[:, :-1]).mean(axis=0)
    se = 1.0 / math.sqrt(N)
    print(f"whitened residuals, in standard errors: largest |mean| {np.abs(mean).max() / se:.2f}, largest |var - 1| "
          f"{np.abs(var - 1.0).max() / (math.sqrt(2.0) * se):.2f}, largest |lag-one product| {np.abs(lag).max() / se:.2f}")
    assert (np.abs(mean) <= 5.0 * se).all(), mean
    assert (np.abs(var - 1.0) <= 5.0 * math.sqrt(2.0) * se).all(), var
    assert (np.abs(lag) <= 5.0 * se).all(), lag
    # not a no-op, and paired the right way round: log y_t^2 - alpha_new[t + 1] is the seven-component mixture, - alpha_new[t] is not
    w = PIS / PIS.sum()
    cdf = lambda x: (w * special.ndtr((np.asarray(x)[..., None] - MEANS) / np.sqrt(VARS))).sum(axis=-1)
    ly = np.log(y * y)
    right = ss.kstest((ly - alpha_new[:, 1:]).reshape(-1), cdf)
    wrong = ss.kstest((ly - alpha_new[:, :-1]).reshape(-1), cdf)
    print(f"KS against the mixture: log y_t^2 - alpha[t+1]: D {right.statistic:.5f} p {right.pvalue:.3g};  - alpha[t]: D {wrong.statistic:.5f} p {wrong.pvalue:.3g}")
    assert right.pvalue > 1e-3
    assert wrong.pvalue < 1e-3


@pytest.mark.gpu
def test_mixture_then_state_draw_leaves_the_joint_law_invariant(eng):
    """sv_mixture then ar1_ffbs is a Gibbs block on (k, alpha) given y: it leaves p(alpha | y) invariant, so with (alpha, y) drawn from
    the model the new alpha is again a stationary AR(1) path -- exactly, in one sweep, with N independent replicates -- and
    (alpha_new, y) has the joint law of (alpha, y).  A shift of the pairing y[t] <-> alpha[t + 1] in either kernel breaks both.
    Whitened residuals within five standard errors; the observation residual by Kolmogorov-Smirnov.  Rehearsed on the CPU with
    this file's restatement of the mixture kernel and the oracle's AR(1) FFBS (profiles/r10_notes.md)."""
    y, alpha = _invariance_data()
    N, T = y.shape
    mix = eng.sv_mixture(y, alpha, iteration=0, seed=41)
    out = eng.ar1_ffbs(mix["ystar"], mix["v"], np.asarray(INV_SV), seed=43)
    assert eng.last_variant == "ar1-lane" and (mix["status"] == 0).all() and (out["status"] == 0).all()
    assert np.abs(out["theta"] - alpha).mean() > 0.05        # a new draw, not the old path
    _invariance_checks(y, out["theta"])
