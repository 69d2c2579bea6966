"""The stochastic-volatility driver (bayesian_dlms_amd/stochvol.py) without a GPU: what it passes to its three engine calls (injected
fakes), the initial parameters, and the code object of the two kernels (dlm_sv.o: no scratch, no spills)."""
import numpy as np
import pytest

from bayesian_dlms_amd import _lib
from bayesian_dlms_amd.gibbs import InverseGamma
from bayesian_dlms_amd.stochvol import Beta, Gaussian, StochasticVolatility, SvParameters, initial_parameters
from code_object import kernel_resources


class _Fakes:
    """mixture / ffbs / params stand-ins that record their inputs in call order; outputs are distinct per call and per series."""

    def __init__(self, N, T):
        self.N, self.T = N, T
        self.calls = []

    def mixture(self, y, alpha, *, iteration, seed, series_offset, out=None):
        self.calls.append(("mixture", dict(alpha=None if alpha is None else np.array(alpha), iteration=iteration, seed=seed,
                                           series_offset=series_offset, out=out)))
        k = len(self.calls)
        return {"ystar": np.full((self.N, self.T), float(k)), "v": np.full((self.N, self.T), 10.0 + k), "k": None,
                "status": np.zeros(self.N, np.int32)}

    def ffbs(self, y, v, sv, *, seed, series_offset, want_filt, want_theta):
        self.calls.append(("ffbs", dict(y=np.array(y), v=np.array(v), sv=np.array(sv), seed=seed, series_offset=series_offset,
                                        want_filt=want_filt, want_theta=want_theta)))
        k = len(self.calls)
        st = np.zeros(self.N, np.int32)
        st[1] = 2 if k == 2 else 0            # the initial FFBS flags series 1
        return {"theta": np.full((self.N, self.T + 1), 100.0 * k) + np.arange(self.N)[:, None], "filt": None, "status": st}

    def params(self, alpha, sv, prior, *, iteration, accepted, seed, series_offset, out=None):
        self.calls.append(("params", dict(alpha=np.array(alpha), sv=np.array(sv), prior=prior, iteration=iteration,
                                          accepted=np.array(accepted), seed=seed, series_offset=series_offset)))
        st = np.zeros(self.N, np.int32)
        st[0] = 1 if iteration == 1 else 0
        new = np.array(sv) * 0.5 + iteration
        return {"sv": new, "accepted": np.array(accepted) + 1, "status": st}


def _run(kind="uni", literal=False, n_iter=3, keep_alpha=False, **kw):
    N, T = 5, 7
    fk = _Fakes(N, T)
    y = np.random.default_rng(1).standard_normal((N, T))
    common = dict(n_iter=n_iter, seed=4, series_offset=11, literal=literal, keep_alpha=keep_alpha, ffbs=fk.ffbs, mixture=fk.mixture,
                  params=fk.params, **kw)
    if kind == "uni":
        gen = StochasticVolatility.sample_uni(y, Gaussian(0.8, 0.1), Gaussian(1.0, 2.0), InverseGamma(2.0, 3.0), None,
                                              params0=SvParameters(0.7, 0.5, 0.2), **common)
    else:
        gen = StochasticVolatility.sample_beta(y, Beta(5.0, 2.0), Gaussian(1.0, 2.0), InverseGamma(2.0, 3.0), None,
                                               params0=SvParameters(0.7, 0.5, 0.2), **common)
    return fk, list(gen), N, T


def test_call_order_and_iteration_numbers():
    fk, states, N, T = _run(n_iter=3)
    assert [c[0] for c in fk.calls] == ["mixture", "ffbs"] + ["mixture", "ffbs", "params"] * 3
    mix = [c[1] for c in fk.calls if c[0] == "mixture"]
    par = [c[1] for c in fk.calls if c[0] == "params"]
    ff = [c[1] for c in fk.calls if c[0] == "ffbs"]
    assert mix[0]["alpha"] is None and mix[0]["iteration"] == 0            # the initial transform
    assert [m["iteration"] for m in mix[1:]] == [0, 1, 2] and [p["iteration"] for p in par] == [0, 1, 2]
    assert all(m["alpha"] is not None for m in mix[1:])
    assert all(c["seed"] == 4 and c["series_offset"] == 11 for c in mix + par)
    # every FFBS call its own seed (its normals are keyed by seed, series and step alone), none the chain's
    seeds = [f["seed"] for f in ff]
    assert len(set(seeds)) == 4 and all(f["series_offset"] == 11 for f in ff)
    assert all(f["want_filt"] is False and f["want_theta"] is True for f in ff)
    assert len(states) == 3


def test_state_and_parameters_are_passed_forward():
    fk, states, N, T = _run(n_iter=3, keep_alpha=True)
    calls = fk.calls
    sv0 = np.tile([0.7, 0.5, 0.2], (N, 1))
    np.testing.assert_array_equal(calls[1][1]["sv"], sv0)                   # the initial FFBS
    np.testing.assert_array_equal(calls[1][1]["y"], np.full((N, T), 1.0))   # ... on the initial transform's outputs
    np.testing.assert_array_equal(calls[1][1]["v"], np.full((N, T), 11.0))
    sv = sv0
    for it in range(3):
        m, f, p = (calls[2 + 3 * it + j][1] for j in range(3))
        # (the fakes number their outputs by the position of the call: the FFBS call before this mixture call was number 2 or 1 + 3 it)
        np.testing.assert_array_equal(m["alpha"], 100.0 * (2 if it == 0 else 1 + 3 * it) + np.arange(N)[:, None] + np.zeros((N, T + 1)))
        np.testing.assert_array_equal(f["sv"], sv)
        np.testing.assert_array_equal(f["y"], np.full((N, T), float(3 + 3 * it)))
        np.testing.assert_array_equal(p["sv"], sv)
        np.testing.assert_array_equal(p["alpha"], 100.0 * (4 + 3 * it) + np.arange(N)[:, None] + np.zeros((N, T + 1)))
        np.testing.assert_array_equal(p["accepted"], it)
        sv = sv * 0.5 + it
        np.testing.assert_array_equal(states[it].params, sv)
        np.testing.assert_array_equal(states[it].alpha, p["alpha"])
        np.testing.assert_array_equal(states[it].accepted, it + 1)
    # the mixture call writes into the previous iteration's buffers
    mix = [c[1] for c in calls if c[0] == "mixture"]
    assert mix[0]["out"] is None and all(set(m["out"]) == {"ystar", "v"} for m in mix[1:])
    # status: the initial FFBS's flag lands in the first state, the parameter call's in the second
    assert states[0].status.tolist() == [0, 2, 0, 0, 0] and states[1].status.tolist() == [1, 0, 0, 0, 0]
    assert _run(n_iter=1)[1][0].alpha is None


@pytest.mark.parametrize("kind,literal", [("uni", False), ("uni", True), ("beta", False), ("beta", True)])
def test_the_prior_struct_carries_mode_and_fields(kind, literal):
    fk, states, N, T = _run(kind=kind, literal=literal, n_iter=1)
    pr = [c[1] for c in fk.calls if c[0] == "params"][0]["prior"]
    assert isinstance(pr, _lib.SvPrior)
    assert pr.phi_update == (1 if kind == "beta" else 0) and pr.literal == int(literal)
    assert (pr.phi_a, pr.phi_b) == ((5.0, 2.0) if kind == "beta" else (0.8, 0.1))
    assert (pr.mu_mean, pr.mu_sd, pr.sigma_shape, pr.sigma_scale, pr.prop_lambda, pr.prop_tau) == (1.0, 2.0, 2.0, 3.0, 100.0, 0.05)


def test_prior_families_the_device_does_not_evaluate_are_refused():
    y = np.zeros((2, 5))
    g, ig = Gaussian(0.0, 1.0), InverseGamma(2.0, 2.0)
    with pytest.raises(TypeError):
        StochasticVolatility.sample_uni(y, Beta(2.0, 2.0), g, ig, None, n_iter=1)
    with pytest.raises(TypeError):
        StochasticVolatility.sample_beta(y, g, g, ig, None, n_iter=1)
    with pytest.raises(TypeError):
        StochasticVolatility.sample_uni(y, g, g, Gaussian(1.0, 1.0), None, n_iter=1)
    with pytest.raises(TypeError):
        StochasticVolatility.sample_beta(y, Beta(2.0, 2.0), ig, ig, None, n_iter=1)
    with pytest.raises(ValueError):     # |phi| >= 1 given
        next(StochasticVolatility.sample_uni(y, g, g, ig, None, n_iter=1, params0=(1.2, 0.0, 1.0), ffbs=1, mixture=1, params=1))
    with pytest.raises(ValueError):     # the Beta proposal lives on (0, 1)
        next(StochasticVolatility.sample_beta(y, Beta(2.0, 2.0), g, ig, None, n_iter=1, params0=(-0.5, 0.0, 1.0), ffbs=1, mixture=1, params=1))
    with pytest.raises(ValueError):     # T = 1
        next(StochasticVolatility.sample_uni(np.zeros((2, 1)), g, g, ig, None, n_iter=1, ffbs=1, mixture=1, params=1))


def test_initial_parameters_are_stationary_and_do_not_depend_on_the_sharding():
    wide = Gaussian(0.9, 1.5)            # P(|phi| >= 1) about one half: many redraws
    full = initial_parameters(wide, Gaussian(1.0, 2.0), InverseGamma(3.0, 1.0), 400, seed=9)
    assert (np.abs(full[:, 0]) < 1.0).all() and (full[:, 2] > 0.0).all() and np.isfinite(full).all()
    assert (full[:, 0] < 0.0).any() and len(np.unique(full[:, 0])) == 400
    halves = np.concatenate([initial_parameters(wide, Gaussian(1.0, 2.0), InverseGamma(3.0, 1.0), 150, seed=9),
                             initial_parameters(wide, Gaussian(1.0, 2.0), InverseGamma(3.0, 1.0), 250, seed=9, series_offset=150)])
    np.testing.assert_array_equal(full, halves)
    b = initial_parameters(Beta(5.0, 1.0), Gaussian(1.0, 2.0), InverseGamma(3.0, 1.0), 200, seed=9)
    assert ((b[:, 0] > 0.0) & (b[:, 0] < 1.0)).all()
    # the driver starts its chains there
    N, T = 5, 7
    fk = _Fakes(N, T)
    next(StochasticVolatility.sample_uni(np.zeros((N, T)), wide, Gaussian(1.0, 2.0), InverseGamma(3.0, 1.0), None, n_iter=1, seed=9,
                                         series_offset=3, ffbs=fk.ffbs, mixture=fk.mixture, params=fk.params))
    np.testing.assert_array_equal(fk.calls[1][1]["sv"], full[3:3 + N])


def test_simulate_has_the_models_moments():
    p = SvParameters(0.8, 1.0, 0.3)
    y, alpha = StochasticVolatility.simulate(p, 400, 200, seed=2)
    assert y.shape == (200, 400) and alpha.shape == (200, 401)
    sd = 0.3 / np.sqrt(1 - 0.64)
    assert abs(alpha.mean() - 1.0) < 5 * sd / np.sqrt(200 * 400 * (1 - 0.8) / (1 + 0.8))
    assert abs(alpha[:, 0].std() - sd) < 0.1 * sd
    r = alpha[:, 1:] - 1.0 - 0.8 * (alpha[:, :-1] - 1.0)
    assert abs(r.std() - 0.3) < 0.01
    assert abs(np.mean((y * np.exp(-0.5 * alpha[:, 1:])) ** 2) - 1.0) < 0.03


def test_sv_kernels_have_no_scratch_and_no_spills():
    """dlm_sv.o's code object: k_sv_mixture and k_sv_params keep everything in registers (read as tests/test_studentt_host.py reads
    dlm_studentt.o)."""
    for kernel in ("k_sv_mixture", "k_sv_params"):
        assert kernel_resources("dlm_sv.o", kernel)[:2] == (0, 0), kernel
