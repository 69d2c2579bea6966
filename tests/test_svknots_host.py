"""The knot block sampler of the stochastic-volatility state on the host: the knots (stochvol.sample_knots), the driver's argument
checks, the restatement's draws, and the exact-invariance check on the restatement (tests/svknots_restatement.py) -- the same check
tests/test_svknots_gpu.py holds the device to."""
import numpy as np
import pytest

from bayesian_dlms_amd.gibbs import InverseGamma
from bayesian_dlms_amd.stochvol import Beta, Gaussian, StochasticVolatility, StochasticVolatilityKnots, knots_rng, sample_knots
from sampler_restatement import gibbs_rand, normal
from svknots_restatement import (INV_KNOTS, INV_SV, KEY_SVKNOT, invariance_checks, invariance_data, invariance_figures, knot_inputs,
                                 normals, sweep, uniforms)

INV_SEED = 41


@pytest.mark.parametrize("lo,hi,T", [(10, 100, 1000), (3, 9, 40), (1, 1, 5), (1, 4, 2), (50, 60, 7), (7, 7, 20)])
def test_sample_knots_properties(lo, hi, T):
    for seed in range(20):
        k = sample_knots(lo, hi, T, knots_rng(seed, 3))
        assert k.dtype == np.int32 and k[0] == 0 and k[-1] == T + 1
        d = np.diff(k)
        assert (d > 0).all()
        assert ((d[:-1] >= lo) & (d[:-1] <= hi)).all() and 1 <= d[-1] <= hi
        assert np.array_equal(k, sample_knots(lo, hi, T, knots_rng(seed, 3)))          # deterministic in (seed, iteration)
    ks = [tuple(sample_knots(lo, hi, T, knots_rng(s, i))) for s in (0, 1) for i in (0, 1)]
    if hi > lo and T > hi:
        assert len(set(ks)) > 1                                                        # ... and a function of both


def test_sample_knots_sizes_are_uniform():
    d = np.concatenate([np.diff(sample_knots(3, 6, 4000, knots_rng(s, 0)))[:-1] for s in range(5)])
    freq = np.bincount(d, minlength=7)[3:] / d.size
    assert d.size > 3000 and np.abs(freq - 0.25).max() < 5.0 * np.sqrt(0.25 * 0.75 / d.size)


def test_argument_checks():
    with pytest.raises(ValueError):
        sample_knots(0, 5, 10, knots_rng(0, 0))
    with pytest.raises(ValueError):
        sample_knots(6, 5, 10, knots_rng(0, 0))
    y = np.ones((2, 8))
    pmu, psig = Gaussian(0.0, 1.0), InverseGamma(3.0, 0.5)
    with pytest.raises(TypeError):
        StochasticVolatilityKnots.sample_ar(y, Beta(5.0, 2.0), pmu, psig, None, n_iter=1)
    with pytest.raises(TypeError):
        StochasticVolatilityKnots.sample_ar_beta(y, Gaussian(0.8, 0.1), pmu, psig, None, n_iter=1)
    with pytest.raises(ValueError):
        StochasticVolatilityKnots.sample_ar(y, Gaussian(0.8, 0.1), pmu, psig, None, n_iter=1, min_size=0)
    with pytest.raises(ValueError):
        StochasticVolatilityKnots.sample_ar_beta(y, Beta(5.0, 2.0), pmu, psig, None, n_iter=1, min_size=5, max_size=4)
    with pytest.raises(ValueError):
        StochasticVolatilityKnots.sample_ar(y, Gaussian(0.8, 0.1), pmu, psig, None, n_iter=1, min_size=2.5)
    assert StochasticVolatilityKnots.State is StochasticVolatility.State
    assert StochasticVolatility.State(np.zeros((1, 3)), None, np.zeros(1), np.zeros(1)).accepted_blocks is None


def test_the_restatement_draws_what_the_scalar_helpers_draw():
    seed, it = (7 << 32) | 5, 9
    series = np.array([0, 3, (1 << 33) + 2], dtype=np.uint64)
    for slot in (0, 17, 0x1FFFF6):
        z = normals(seed, series, it, slot)
        for k, s in enumerate(series):
            assert z[k] == normal(KEY_SVKNOT, seed, int(s), it, slot)
            u1, u2 = gibbs_rand(seed, int(s), it, [slot], 0, 1, KEY_SVKNOT)
            v1, v2 = uniforms(seed, series[k:k + 1], it, slot, 1)
            assert u1[0] == v1[0] and u2[0] == v2[0]


def test_a_sweep_moves_what_it_should_and_nothing_else():
    y, alpha, sv = knot_inputs(9, 30, 3)
    sv[2, 0] = 1.2
    alpha[4, 7] = np.inf
    knots = [0, 1, 9, 10, 25, 31]
    out = sweep(y, alpha, sv, knots, seed=5, iteration=2, series_offset=11, accepted=np.arange(9))
    assert out["status"][2] == 2 and out["status"][4] == 1
    for n in (2, 4):
        assert np.array_equal(out["alpha"][n], alpha[n]) and out["accepted"][n] == n
    for n in (0, 1, 3, 5, 6, 7, 8):
        assert out["accepted"][n] == n + out["accept"][n].sum()
        for i in range(5):
            same = np.array_equal(out["alpha"][n, knots[i]:knots[i + 1]], alpha[n, knots[i]:knots[i + 1]])
            assert same != out["accept"][n, i]
    assert out["accept"][[0, 1, 3, 5, 6, 7, 8], 0].all()          # the block {alpha_0} observes nothing
    part = sweep(y[5:], alpha[5:], sv[5:], knots, seed=5, iteration=2, series_offset=16)
    assert np.array_equal(part["alpha"], out["alpha"][5:])


def test_one_sweep_leaves_the_exact_posterior_invariant_and_the_unchecked_proposal_does_not():
    """(alpha, y) from the exact model at (0.8, 1.0, 0.3), N = 16384, T = 17, knots [0, 1, 6, 12, 18]: after one call the whitened AR(1)
    residuals stay within five standard errors and log y_t^2 - alpha_new[t+1] is log chi^2_1.  The same sweep with every block
    accepted -- the Gaussian approximation's own posterior -- fails the Kolmogorov-Smirnov test: the Metropolis step is what the
    check sees."""
    y, alpha = invariance_data()
    out = sweep(y, alpha, INV_SV, INV_KNOTS, seed=INV_SEED, iteration=0)
    rate = out["accept"].mean(axis=0)
    print("block acceptance rates", np.round(rate, 3))
    assert (out["status"] == 0).all() and rate[0] == 1.0 and (rate[1:] > 0.5).all() and (rate[1:] < 0.95).all()
    assert np.abs(out["alpha"] - alpha).mean() > 0.05
    invariance_checks(y, out["alpha"])
    forced = sweep(y, alpha, INV_SV, INV_KNOTS, seed=INV_SEED, iteration=0, force_accept=True)
    errs, right, wrong = invariance_figures(y, forced["alpha"])
    print(f"every block accepted: residuals {errs}, KS p {right:.3g}")
    assert right < 1e-3
