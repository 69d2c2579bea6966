"""The Ornstein-Uhlenbeck stochastic-volatility driver (StochasticVolatility.sample_ou / simulate_ou) without a GPU: what it passes
to its three engine calls (injected fakes), the prior struct against include/dlm_engine.h, simulate_ou's moments, and the
restated arithmetic of k_sv_ou_params (tests/test_stochvol_ou_gpu.py) against the model's log density written out term by term."""
import math
import os
import re

import numpy as np
import pytest

from bayesian_dlms_amd import _lib
from bayesian_dlms_amd.gibbs import InverseGamma
from bayesian_dlms_amd.stochvol import Beta, Gaussian, StochasticVolatility, SvParameters, initial_parameters
from code_object import kernel_resources
from sampler_restatement import ou_params_inputs as params_inputs, ou_params_step, ou_prior as prior

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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

    def ffbs(self, y, v, sv, *, seed, series_offset, want_filt, want_theta, times):
        self.calls.append(("ffbs", dict(y=np.array(y), v=np.array(v), sv=np.array(sv), seed=seed, series_offset=series_offset,
                                        want_filt=want_filt, want_theta=want_theta, times=np.array(times))))
        k = len(self.calls)
        st = np.zeros(self.N, np.int32)
        st[1] = 2 if k == 2 else 0            # the initial FFBS flags series 1
        return {"theta": np.full((self.N, self.T + 1), 100.0 * k) + np.arange(self.N)[:, None], "filt": None, "status": st}

    def params(self, times, alpha, sv, prior, *, iteration, accepted, seed, series_offset, out=None):
        self.calls.append(("params", dict(times=np.array(times), alpha=np.array(alpha), sv=np.array(sv), prior=prior, iteration=iteration,
                                          accepted=np.array(accepted), seed=seed, series_offset=series_offset)))
        st = np.zeros(self.N, np.int32)
        st[0] = 1 if iteration == 1 else 0
        return {"sv": np.array(sv) * 0.5 + iteration, "accepted": np.array(accepted) + np.array([1, 2, 3], np.int32), "status": st}


TIMES = np.array([0.0, 0.4, 0.4, 1.7, 2.0, 5.5, 6.0])


def _run(literal=False, n_iter=3, keep_alpha=False, **kw):
    N, T = 5, TIMES.size
    fk = _Fakes(N, T)
    y = np.random.default_rng(1).standard_normal((N, T))
    gen = StochasticVolatility.sample_ou(TIMES, y, Beta(5.0, 2.0), Gaussian(1.0, 2.0), InverseGamma(2.0, 3.0), None, n_iter=n_iter, seed=4,
                                         series_offset=11, literal=literal, keep_alpha=keep_alpha, params0=SvParameters(0.7, 0.5, 0.2),
                                         ffbs=fk.ffbs, mixture=fk.mixture, params=fk.params, **kw)
    return fk, list(gen), N, T


def test_call_order_seeds_and_the_grid():
    fk, states, N, T = _run(n_iter=3)
    assert [c[0] for c in fk.calls] == ["mixture", "ffbs"] + ["mixture", "ffbs", "params"] * 3
    mix = [c[1] for c in fk.calls if c[0] == "mixture"]
    par = [c[1] for c in fk.calls if c[0] == "params"]
    ff = [c[1] for c in fk.calls if c[0] == "ffbs"]
    assert mix[0]["alpha"] is None and mix[0]["iteration"] == 0            # initialStateOu: the initial transform, then the OU FFBS
    assert [m["iteration"] for m in mix[1:]] == [0, 1, 2] and [p["iteration"] for p in par] == [0, 1, 2]
    assert all(c["seed"] == 4 and c["series_offset"] == 11 for c in mix + par)
    # the _seed_ffbs convention: a seed per FFBS call, k = 0 the initial state's
    assert [f["seed"] for f in ff] == [StochasticVolatility._seed_ffbs(4, k) for k in range(4)] and len({f["seed"] for f in ff}) == 4
    assert all(f["series_offset"] == 11 and f["want_filt"] is False and f["want_theta"] is True for f in ff)
    # every FFBS call and every parameter call gets the grid
    for c in ff + par:
        np.testing.assert_array_equal(c["times"], TIMES)
    assert len(states) == 3


def test_state_parameters_counters_and_status_are_passed_forward():
    fk, states, N, T = _run(n_iter=3, keep_alpha=True)
    calls = fk.calls
    sv0 = np.tile([0.7, 0.5, 0.2], (N, 1))
    np.testing.assert_array_equal(calls[1][1]["sv"], sv0)
    np.testing.assert_array_equal(calls[1][1]["y"], np.full((N, T), 1.0))
    sv = sv0
    for it in range(3):
        m, f, p = (calls[2 + 3 * it + j][1] for j in range(3))
        np.testing.assert_array_equal(m["alpha"], 100.0 * (2 if it == 0 else 1 + 3 * it) + np.arange(N)[:, None] + np.zeros((N, T + 1)))
        np.testing.assert_array_equal(f["sv"], sv)
        np.testing.assert_array_equal(p["sv"], sv)
        np.testing.assert_array_equal(p["alpha"], 100.0 * (4 + 3 * it) + np.arange(N)[:, None] + np.zeros((N, T + 1)))
        assert p["accepted"].shape == (N, 3) and p["accepted"].dtype == np.int32
        np.testing.assert_array_equal(p["accepted"], np.tile([1, 2, 3], (N, 1)) * it)
        sv = sv * 0.5 + it
        np.testing.assert_array_equal(states[it].params, sv)
        np.testing.assert_array_equal(states[it].alpha, p["alpha"])
        np.testing.assert_array_equal(states[it].accepted, np.tile([1, 2, 3], (N, 1)) * (it + 1))
    mix = [c[1] for c in calls if c[0] == "mixture"]
    assert mix[0]["out"] is None and all(set(m["out"]) == {"ystar", "v"} for m in mix[1:])
    # status: the initial FFBS's flag lands in the first state, the parameter call's in the second
    assert states[0].status.tolist() == [0, 2, 0, 0, 0] and states[1].status.tolist() == [1, 0, 0, 0, 0]
    assert _run(n_iter=1)[1][0].alpha is None


def _header_fields(name):
    src = open(os.path.join(ROOT, "include", "dlm_engine.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            out += [(n.strip(), ctype) for n in names.split(",")]
    return out


def _struct_fields(cls):
    return [(n, "int32_t" if t is _lib.ctypes.c_int32 else "double") for n, t in cls._fields_]


@pytest.mark.parametrize("name,cls,count", [("dlm_sv_prior", _lib.SvPrior, 10), ("dlm_studentt_prior", _lib.StudentTPrior, 4)])
def test_the_other_samplers_prior_structs_follow_the_header(name, cls, count):
    want = _header_fields(name)
    assert _struct_fields(cls) == want and len(want) == count


def test_the_prior_struct_follows_the_header_and_carries_the_arguments():
    want = _header_fields("dlm_sv_ou_prior")
    got = _struct_fields(_lib.SvOuPrior)
    assert got == want and len(want) == 11
    fk, _, _, _ = _run(n_iter=1, prop_lambda=7.0, prop_tau=0.1, delta_sigma=0.2, delta_mu=0.3)
    pr = [c[1] for c in fk.calls if c[0] == "params"][0]["prior"]
    assert isinstance(pr, _lib.SvOuPrior)
    assert tuple(getattr(pr, n) for n, _ in want) == (0, 5.0, 2.0, 1.0, 2.0, 2.0, 3.0, 7.0, 0.1, 0.2, 0.3)
    fk, _, _, _ = _run(n_iter=1)       # the signatures' own defaults
    pr = [c[1] for c in fk.calls if c[0] == "params"][0]["prior"]
    assert (pr.literal, pr.prop_lambda, pr.prop_tau, pr.delta_sigma, pr.delta_mu) == (0, 10.0, 0.05, 0.05, 0.05)
    fk, _, _, _ = _run(n_iter=1, literal=True)       # Q22: stepOu hands 0.05 to `lambda`
    pr = [c[1] for c in fk.calls if c[0] == "params"][0]["prior"]
    assert (pr.literal, pr.prop_lambda, pr.prop_tau, pr.delta_sigma, pr.delta_mu) == (1, 0.05, 0.05, 0.05, 0.05)


def test_value_and_type_errors():
    y = np.zeros((2, 5))
    t5 = np.arange(5.0)
    b, g, ig = Beta(2.0, 2.0), Gaussian(0.0, 1.0), InverseGamma(2.0, 2.0)
    for priors in ((g, g, ig), (b, ig, ig), (b, g, g)):
        with pytest.raises(TypeError):
            StochasticVolatility.sample_ou(t5, y, *priors, None, n_iter=1)
    for p0 in ((1.2, 0.0, 1.0), (0.0, 0.0, 1.0), (-0.5, 0.0, 1.0), (0.5, 0.0, 0.0), (0.5, 0.0, -1.0)):
        with pytest.raises(ValueError):
            next(StochasticVolatility.sample_ou(t5, y, b, g, ig, None, n_iter=1, params0=p0, ffbs=1, mixture=1, params=1))
    with pytest.raises(ValueError):     # T = 1
        next(StochasticVolatility.sample_ou(t5[:1], np.zeros((2, 1)), b, g, ig, None, n_iter=1, ffbs=1, mixture=1, params=1))
    with pytest.raises(ValueError):     # a grid of another length
        next(StochasticVolatility.sample_ou(t5[:4], y, b, g, ig, None, n_iter=1, params0=(0.5, 0.0, 1.0), ffbs=1, mixture=1, params=1))


def test_initial_parameters_take_the_prior_on_sigma_itself():
    N, T = 5, TIMES.size
    fk = _Fakes(N, T)
    pri = (Beta(5.0, 2.0), Gaussian(1.0, 2.0), InverseGamma(3.0, 1.0))
    next(StochasticVolatility.sample_ou(TIMES, np.zeros((N, T)), *pri, None, n_iter=1, seed=9, series_offset=3, ffbs=fk.ffbs,
                                        mixture=fk.mixture, params=fk.params))
    on_sigma = initial_parameters(*pri, 20, seed=9, sigma_squared=False)
    on_variance = initial_parameters(*pri, 20, seed=9)
    np.testing.assert_array_equal(fk.calls[1][1]["sv"], on_sigma[3:3 + N])
    np.testing.assert_array_equal(on_sigma[:, :2], on_variance[:, :2])
    np.testing.assert_allclose(on_sigma[:, 2], on_variance[:, 2] ** 2, rtol=1e-14)
    assert ((on_sigma[:, 0] > 0.0) & (on_sigma[:, 0] < 1.0)).all()


def test_simulate_ou_on_a_unit_grid_is_the_ar1_model():
    phi, mu, sig, T, N = 0.4, 1.0, 0.3, 200, 400
    y, alpha = StochasticVolatility.simulate_ou(SvParameters(phi, mu, sig), np.arange(float(T)), N, seed=2)
    assert y.shape == (N, T) and alpha.shape == (N, T + 1)
    assert np.array_equal(alpha[:, 1], alpha[:, 0])
    assert abs(alpha[:, 0].mean() - mu) < 5 * sig / math.sqrt(N) and abs(alpha[:, 0].std() - sig) < 0.1 * sig
    phi_ar, sig_ar = math.exp(-phi), sig * math.sqrt((1.0 - math.exp(-2.0 * phi)) / (2.0 * phi))
    prev, cur = alpha[:, 1:-1] - mu, alpha[:, 2:] - mu
    slope = (prev * cur).sum() / (prev * prev).sum()
    n = prev.size
    assert abs(slope - phi_ar) < 5 * sig_ar / math.sqrt((prev * prev).sum())
    r = cur - phi_ar * prev
    assert abs(r.mean()) < 5 * sig_ar / math.sqrt(n) and abs(r.std() - sig_ar) < 5 * sig_ar / math.sqrt(2 * n)
    assert abs(np.mean((y * np.exp(-0.5 * alpha[:, 1:])) ** 2) - 1.0) < 5 * math.sqrt(2.0 / (N * T))
    # an irregular grid with a repeated time: the state does not move across dt = 0
    _, a2 = StochasticVolatility.simulate_ou(SvParameters(phi, mu, sig), TIMES, 50, seed=3)
    assert np.array_equal(a2[:, 3], a2[:, 2]) and not np.array_equal(a2[:, 4], a2[:, 3])


def _log_density(times, al, phi, mu, sig, pr, *, initial_state):
    """log [Beta(a, b)(phi) InverseGamma(shape, scale)(sigma) N(mean, sd)(mu) N(alpha_0; mu, sigma^2)^initial_state
    prod_{dt_t > 0} N(alpha_t; mu + e^(-phi dt_t) (alpha_{t-1} - mu), sigma^2 (1 - e^(-2 phi dt_t)) / (2 phi))], each density whole."""
    from scipy import stats as ss
    lp = ss.beta(pr["phi_a"], pr["phi_b"]).logpdf(phi) + ss.invgamma(pr["sigma_shape"], scale=pr["sigma_scale"]).logpdf(sig)
    lp += ss.norm(pr["mu_mean"], pr["mu_sd"]).logpdf(mu)
    if initial_state:
        lp += ss.norm(mu, sig).logpdf(al[0])
    for t in range(2, al.size):
        dt = times[t - 1] - times[t - 2]
        if dt != 0.0:
            sd = math.sqrt(sig * sig * (1.0 - math.exp(-2.0 * phi * dt)) / (2.0 * phi))
            lp += ss.norm(mu + math.exp(-phi * dt) * (al[t - 1] - mu), sd).logpdf(al[t])
    return lp


@pytest.mark.parametrize("literal", [0, 1])
def test_the_restated_ratios_are_the_models(literal):
    """The three log acceptance ratios of the restatement (which the GPU test holds the kernel to, draw for draw) against differences of
    the model's log density written out with scipy's densities, term by term: in the default mode the density with the initial state's
    N(alpha_0; mu, sigma^2) (Q24) plus the proposal ratios (Q23); in the literal mode prior.logPdf + ouLikelihood and nothing else.
    Each move starts from the incoming value and sees the earlier moves' outcomes (Q25).  1e-9 relative to max(1, |ratio|): the ratios
    are differences of sums of 64 terms of order 1 to 100, which leaves rounding of the order of 1e-13."""
    from scipy import stats as ss
    N, T = 24, 65
    times, alpha, sv = params_inputs(N, T, 31)
    pr = prior(literal)
    seen = np.zeros(3, int)
    for n in range(N):
        phi0, mu0, sig0 = sv[n]
        phi, mu, sig, acc, status, _, moves = ou_params_step(times, alpha[n], sv[n], pr, seed=5, series=n, it=2)
        assert status == 0
        ld = lambda f, m, s: _log_density(times, alpha[n], f, m, s, pr, initial_state=not literal)
        (phip, d_phi), (sigp, d_sig), (mup, d_mu) = moves
        lam, tau = pr["prop_lambda"], pr["prop_tau"]
        want = ld(phip, mu0, sig0) - ld(phi0, mu0, sig0)
        if not literal:
            want += (ss.beta(lam * phip + tau, lam * (1.0 - phip) + tau).logpdf(phi0)
                     - ss.beta(lam * phi0 + tau, lam * (1.0 - phi0) + tau).logpdf(phip))
        assert abs(d_phi - want) < 1e-9 * max(1.0, abs(want)), (n, d_phi, want)
        want = ld(phi, mu0, sigp) - ld(phi, mu0, sig0) + (0.0 if literal else math.log(sigp / sig0))
        assert abs(d_sig - want) < 1e-9 * max(1.0, abs(want)), (n, d_sig, want)
        want = ld(phi, mup, sig) - ld(phi, mu0, sig)
        assert abs(d_mu - want) < 1e-9 * max(1.0, abs(want)), (n, d_mu, want)
        assert (phi, sig, mu) == (phip if acc[0] else phi0, sigp if acc[1] else sig0, mup if acc[2] else mu0)
        seen += acc
    assert (seen > 0).all() and (seen < N).all()          # later moves were checked behind both outcomes of the earlier ones


def test_the_kernel_has_no_scratch_and_no_spills():
    """dlm_sv_ou.o's code object, read as tests/test_stochvol_host.py reads dlm_sv.o: k_sv_ou_params keeps everything in registers."""
    scratch, spills, vgprs = kernel_resources("dlm_sv_ou.o", "k_sv_ou_params")
    assert (scratch, spills) == (0, 0) and vgprs <= 128, (scratch, spills, vgprs)          # (128 VGPRs: four waves per SIMD)
