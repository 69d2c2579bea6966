"""The knot block sampler of the stochastic-volatility state on the device (dlm_sv_knots_batch, Engine.sv_knots,
stochvol.StochasticVolatilityKnots): draw for draw against tests/svknots_restatement.py, the exact-invariance check of
tests/test_svknots_host.py on the device's output, what a rejected block, a bad row and a bad argument do, the bit-for-bit
invariances, and the drivers against the two calls composed by hand."""
import numpy as np
import pytest

from bayesian_dlms_amd import _lib
from bayesian_dlms_amd.engine import Engine, EngineError
from bayesian_dlms_amd.gibbs import InverseGamma
from bayesian_dlms_amd.stochvol import (Beta, Gaussian, StochasticVolatility, StochasticVolatilityKnots, SvParameters, knots_rng,
                                        sample_knots)
from sampler_restatement import sv_prior as prior, sv_prior_tuple as as_tuple
from svknots_restatement import INV_KNOTS, INV_SV, invariance_checks, invariance_data, knot_inputs, sweep

RTOL, ATOL = 1e-11, 1e-12
MARGIN = 1e-9          # a block whose |log u - Delta| is smaller may be decided the other way by a last-bit difference of exp or log
UNEVEN = [0, 1, 2, 70, 75, 100, 130]          # T = 129: two blocks of one state, one of 68 (above a wave's 64), ragged ends
# (N, T, knots, seed): seeds for which the restatement has no block under MARGIN (checked on the host)
CASES = [(1, 2, [0, 3], 1), (3, 5, [0, 1, 2, 3, 4, 5, 6], 2), (67, 129, UNEVEN, 3), (5, 1000, None, 4)]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _blocks_changed(new, old, knots):
    """[N][B] bool: block i of series n differs from the input somewhere."""
    return np.stack([(new[:, knots[i]:knots[i + 1]] != old[:, knots[i]:knots[i + 1]]).any(axis=1) for i in range(len(knots) - 1)], axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("N,T,knots,seed", CASES)
def test_sweep_draw_for_draw(eng, N, T, knots, seed):
    if knots is None:
        knots = sample_knots(10, 100, T, knots_rng(seed, 0))
    y, alpha, sv = knot_inputs(N, T, seed)
    acc0 = np.arange(N, dtype=np.int32)
    ref = sweep(y, alpha, sv, knots, seed=seed, iteration=7, series_offset=9, accepted=acc0)
    out = eng.sv_knots(y, alpha, sv, knots, iteration=7, seed=seed, series_offset=9, accepted=acc0.copy())
    assert eng.last_variant == "sv-knots-lane"
    close = ref["margin"] < MARGIN
    print(f"N {N} T {T} B {len(knots) - 1}: acceptance {ref['accept'].mean():.3f}, smallest margin {ref['margin'].min():.3g}, blocks skipped {close.sum()}")
    assert close.sum() <= close.size / 1000.0
    keep = ~close.any(axis=1)
    assert np.array_equal(out["status"], ref["status"])
    assert np.array_equal(out["accepted"][keep], ref["accepted"][keep])
    assert np.array_equal(_blocks_changed(out["alpha"], alpha, knots)[keep], ref["accept"][keep])
    np.testing.assert_allclose(out["alpha"][keep], ref["alpha"][keep], rtol=RTOL, atol=ATOL)
    if N * T >= 4:
        assert out["status"][N // 2] & _lib.ST_NONFINITE and out["status"][N - 1] & _lib.ST_NONFINITE          # Q20: y = 0, y = 1e-200


@pytest.mark.gpu
def test_one_sweep_leaves_the_exact_posterior_invariant(eng):
    """test_svknots_host.py's check on the device's output: (alpha, y) from the exact model, one call, N = 16384 replicates."""
    y, alpha = invariance_data()
    out = eng.sv_knots(y, alpha, np.asarray(INV_SV), INV_KNOTS, iteration=0, seed=41)
    assert (out["status"] == 0).all()
    rate = out["accepted"].mean() / (len(INV_KNOTS) - 1)
    print(f"block acceptance rate {rate:.3f}")
    assert np.abs(out["alpha"] - alpha).mean() > 0.05
    invariance_checks(y, out["alpha"])


@pytest.mark.gpu
def test_rejected_blocks_are_the_input_bit_for_bit(eng):
    N, T = 200, 129
    y, alpha, sv = knot_inputs(N, T, 11)
    out = eng.sv_knots(y, alpha, sv, UNEVEN, iteration=1, seed=3)
    new = out["alpha"]
    changed = _blocks_changed(new, alpha, UNEVEN)
    for i in range(len(UNEVEN) - 1):          # a block moves as a whole or not at all
        every = (new[:, UNEVEN[i]:UNEVEN[i + 1]] != alpha[:, UNEVEN[i]:UNEVEN[i + 1]]).all(axis=1)
        assert np.array_equal(every, changed[:, i])
    assert np.array_equal(out["accepted"], changed.sum(axis=1))
    assert changed[:, 0].all() and 0.3 < changed[:, 2:].mean() < 0.98          # {alpha_0} observes nothing; the others do reject


@pytest.mark.gpu
def test_bad_rows_come_back_untouched_with_their_flags(eng):
    N, T = 67, 129
    y, alpha, sv = knot_inputs(N, T, 12)
    good = eng.sv_knots(y, alpha, sv, UNEVEN, iteration=1, seed=3)
    sv2, alpha2 = sv.copy(), alpha.copy()
    sv2[5, 0] = 1.2
    sv2[6, 2] = 0.0
    alpha2[64, 99] = np.nan          # inside an odd block: the even blocks of the row must stay too
    alpha2[65, 0] = np.inf
    acc = np.full(N, 3, np.int32)
    out = eng.sv_knots(y, alpha2, sv2, UNEVEN, iteration=1, seed=3, accepted=acc)
    bad = [5, 6, 64, 65]
    assert (out["status"][[5, 6]] == _lib.ST_NOT_PD).all() and (out["status"][[64, 65]] == _lib.ST_NONFINITE).all()
    assert np.array_equal(out["alpha"][bad], alpha2[bad], equal_nan=True) and (out["accepted"][bad] == 3).all()
    rest = np.setdiff1d(np.arange(N), bad)
    assert np.array_equal(out["alpha"][rest], good["alpha"][rest]) and np.array_equal(out["status"][rest], good["status"][rest])
    assert np.array_equal(out["accepted"][rest], good["accepted"][rest] + 3)


@pytest.mark.gpu
def test_invariances_bit_for_bit(eng):
    import torch
    N, T, seed, it = 160, 129, 6, 3
    y, alpha, sv = knot_inputs(N, T, 13)
    full = eng.sv_knots(y, alpha, sv, UNEVEN, iteration=it, seed=seed)
    again = eng.sv_knots(y, alpha, sv, UNEVEN, iteration=it, seed=seed)
    head = eng.sv_knots(y[:100], alpha[:100], sv[:100], UNEVEN, iteration=it, seed=seed)
    tail = eng.sv_knots(y[100:], alpha[100:], sv[100:], UNEVEN, iteration=it, seed=seed, series_offset=100)
    dev = eng.sv_knots(torch.as_tensor(y, device="cuda:0"), torch.as_tensor(alpha, device="cuda:0"), torch.as_tensor(sv, device="cuda:0"),
                       UNEVEN, iteration=it, seed=seed)
    for key in ("alpha", "accepted", "status"):
        assert np.array_equal(full[key], again[key]), key
        assert np.array_equal(full[key][:100], head[key]) and np.array_equal(full[key][100:], tail[key]), key
        assert np.array_equal(full[key], dev[key].cpu().numpy()), key
    one = np.array([0.8, 1.0, 0.3])
    shared = eng.sv_knots(y, alpha, one, UNEVEN, iteration=it, seed=seed)
    per = eng.sv_knots(y, alpha, np.tile(one, (N, 1)), UNEVEN, iteration=it, seed=seed)
    for key in ("alpha", "accepted", "status"):
        assert np.array_equal(shared[key], per[key]), key
    other = eng.sv_knots(y, alpha, sv, UNEVEN, iteration=it + 1, seed=seed)
    assert (other["alpha"] != full["alpha"]).mean() > 0.3
    # in place: out["alpha"] the input itself
    buf = alpha.copy()
    same = eng.sv_knots(y, buf, sv, UNEVEN, iteration=it, seed=seed, out={"alpha": buf})
    assert same["alpha"] is buf and np.array_equal(buf, full["alpha"])


@pytest.mark.gpu
def test_argument_errors(eng):
    y, alpha, sv = knot_inputs(4, 9, 14)
    for knots in ([1, 5, 10], [0, 5, 9], [0, 5, 11], [0, 5, 5, 10], [0, 6, 5, 10], [0, -1, 10], [0, 12, 10]):
        with pytest.raises(EngineError, match=r"\(-1\)"):
            eng.sv_knots(y, alpha, sv, knots, iteration=0)
    with pytest.raises(EngineError):          # B = 0
        eng.sv_knots(y, alpha, sv, [0], iteration=0)
    with pytest.raises(EngineError):          # T = 1
        eng.sv_knots(y[:, :1], alpha[:, :2], sv, [0, 2], iteration=0)
    with pytest.raises(EngineError):
        eng.sv_knots(y, alpha[:, :-1], sv, [0, 5, 10], iteration=0)
    with pytest.raises(EngineError):
        eng.sv_knots(y, alpha, sv[:, :2], [0, 5, 10], iteration=0)
    # the C ABI itself: B = 0 and T = 1 are DLM_ERR_ARG
    import ctypes
    op = _lib.Options(0, _lib.DLM_MEM_HOST, 0, 0)
    kn = np.array([0, 2], np.int32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    st = np.zeros(4, np.int32)
    a2 = np.ascontiguousarray(alpha[:, :2])
    y1 = np.ascontiguousarray(y[:, :1])
    assert eng.lib.dlm_sv_knots_batch(eng.h, 4, 1, p(y1), p(kn), 1, p(sv), 3, 0, op, p(a2), None, p(st)) == -1
    assert eng.lib.dlm_sv_knots_batch(eng.h, 4, 9, p(y), p(kn), 0, p(sv), 3, 0, op, p(alpha), None, p(st)) == -1
    assert eng.lib.dlm_sv_knots_batch(eng.h, 4, 9, p(y), None, 1, p(sv), 3, 0, op, p(alpha), None, p(st)) == -1
    ok = eng.sv_knots(y, alpha, sv, [0, 5, 10], iteration=0)          # the engine is usable after the refusals
    assert np.isfinite(ok["alpha"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ar", "ar_beta"])
def test_driver_equals_the_two_calls_composed_by_hand(eng, kind):
    N, T, seed, off, n_iter = 5, 40, 5, 40, 3
    y, _ = StochasticVolatility.simulate(SvParameters(0.8, 1.0, 0.3), T, N, seed=2)
    y[3, 10:14] = np.nan
    y[4, 7] = 0.0
    p0 = SvParameters(0.7, 0.5, 0.4)
    pmu, psig = Gaussian(1.0, 2.0), InverseGamma(3.0, 0.5)
    common = dict(n_iter=n_iter, min_size=3, max_size=9, seed=seed, params0=p0, series_offset=off, keep_alpha=True)
    if kind == "ar":
        gen = StochasticVolatilityKnots.sample_ar(y, Gaussian(0.8, 0.3), pmu, psig, eng, **common)
        pr = as_tuple(prior(0, 0, 0.8, 0.3, mu=(1.0, 2.0), sigma=(3.0, 0.5)))
    else:
        gen = StochasticVolatilityKnots.sample_ar_beta(y, Beta(5.0, 2.0), pmu, psig, eng, **common)
        pr = as_tuple(prior(1, 0, 5.0, 2.0, mu=(1.0, 2.0), sigma=(3.0, 0.5)))
    states = list(gen)
    assert len(states) == n_iter
    sv = np.tile([0.7, 0.5, 0.4], (N, 1))
    mix = eng.sv_mixture(y, None, iteration=0, seed=seed, series_offset=off)
    f = eng.ar1_ffbs(mix["ystar"], mix["v"], sv, seed=seed * 1000003, series_offset=off, want_filt=False)
    alpha, acc, blocks = f["theta"], np.zeros(N, np.int32), np.zeros(N, np.int32)
    status = mix["status"] | f["status"]
    n_blocks = 0
    for it in range(n_iter):
        knots = sample_knots(3, 9, T, knots_rng(seed, it))
        n_blocks += len(knots) - 1
        sw = eng.sv_knots(y, alpha, sv, knots, iteration=it, accepted=blocks, seed=seed, series_offset=off)
        alpha, blocks = sw["alpha"], sw["accepted"]
        res = eng.sv_params(alpha, sv, pr, iteration=it, accepted=acc, seed=seed, series_offset=off)
        sv, acc = res["sv"], res["accepted"]
        status = status | sw["status"] | res["status"]
        assert np.array_equal(states[it].params, sv) and np.array_equal(states[it].alpha, alpha)
        assert np.array_equal(states[it].accepted, acc) and np.array_equal(states[it].accepted_blocks, blocks)
        assert np.array_equal(states[it].status, status)
        assert states[it].status[4] & _lib.ST_NONFINITE
        status = np.zeros(N, np.int32)
    assert np.isfinite(states[-1].params).all()
    assert (states[-1].accepted_blocks > 0).all() and (states[-1].accepted_blocks <= n_blocks).all()
    if kind == "ar":
        assert (states[-1].accepted == 0).all()


@pytest.mark.gpu
def test_driver_recovers_simulated_parameters_printed_only(eng):
    """Not asserted beyond finiteness: the posterior means of a 64-series, T = 300, 200-iteration run on data simulated at
    (phi, mu, sigma) = (0.8, 1.0, 0.3) are printed, with the block acceptance rate."""
    N, T, n_iter, burn = 64, 300, 200, 80
    y, _ = StochasticVolatility.simulate(SvParameters(0.8, 1.0, 0.3), T, N, seed=4)
    for kind in ("ar", "ar_beta"):
        if kind == "ar":
            gen = StochasticVolatilityKnots.sample_ar(y, Gaussian(0.8, 0.1), Gaussian(1.0, 1.0), InverseGamma(2.0, 2.0), eng, n_iter=n_iter, seed=1)
        else:
            gen = StochasticVolatilityKnots.sample_ar_beta(y, Beta(5.0, 2.0), Gaussian(1.0, 1.0), InverseGamma(2.0, 2.0), eng, n_iter=n_iter, seed=1)
        states = list(gen)
        draws = np.stack([s.params for s in states])
        post = draws[burn:].mean(axis=0)
        n_blocks = sum(len(sample_knots(10, 100, T, knots_rng(1, it))) - 1 for it in range(n_iter))
        print(f"sample_{kind}: posterior means over {N} series: phi {post[:, 0].mean():.3f} (sd over series {post[:, 0].std():.3f}), "
              f"mu {post[:, 1].mean():.3f} ({post[:, 1].std():.3f}), sigma {post[:, 2].mean():.3f} ({post[:, 2].std():.3f}); simulated at 0.8, 1.0, 0.3; "
              f"block acceptance {states[-1].accepted_blocks.mean() / n_blocks:.3f}")
        assert np.isfinite(draws).all()
