"""Gibbs sampler of the stochastic-volatility model with AR(1) latent log-volatility on the device
(StochasticVolatility.sampleUni / sampleBeta, StochasticVolatility.scala:269-341).

  y_t = eps_t exp(alpha_t / 2),   alpha_t = mu + phi (alpha_{t-1} - mu) + eta_t,   eta_t ~ N(0, sigma_eta^2)

log y_t^2 = alpha_t + log eps_t^2 with log eps^2 approximated by the seven-component normal mixture of Kim, Shephard & Chib.  Every
series runs its own chain -- the reference's semantics for one series, N at once -- and one iteration is three engine calls:

  dlm_sv_mixture_batch  k_t | (y_t, alpha_t);  ystar_t = log y_t^2 - m_{k_t},  v_t = v_{k_t}
  dlm_ar1_ffbs_batch    alpha | (ystar, v, phi, mu, sigma)
  dlm_sv_params_batch   phi (Gaussian conjugate, or Beta-proposal Metropolis-Hastings), mu | phi, sigma | (phi, mu)

y, alpha, ystar, v and the parameters stay on the device across iterations whatever the input type; per iteration only the [N][3]
parameters, `accepted` and `status` cross to the host, plus alpha when asked for.  The chain starts as initialStateAr does
(StochVolKnots.scala:345-352): ystar = log y^2 + 1.27, v = pi^2 / 2 at every step, one FFBS.

The default is the corrected sampler; literal=True runs the reference's arithmetic (Q16-Q19).  The priors
are the families the device evaluates: `Gaussian` for mu and for the conjugate phi, `Beta` for the Metropolis-Hastings phi,
`InverseGamma` for sigma_eta^2; the reference's arbitrary ContinuousDistr of sampleBeta is not offered.

StochasticVolatilityKnots.sample_ar / sample_ar_beta are the same chains with the state drawn by the knot block sampler
(StochVolKnots.scala): per iteration the knots are drawn on the host (sample_knots) and ONE dlm_sv_knots_batch sweep replaces the
mixture and FFBS calls -- every block proposed from log y^2 + 1.27 ~ N(alpha, pi^2 / 2) given its neighbours and corrected by a
Metropolis step, so the invariant law is the posterior of the model itself.

sample_ou is the same chain with an Ornstein-Uhlenbeck log-volatility observed at arbitrary times (StochasticVolatility.sampleOu,
:343-500):  alpha(t + dt) | alpha(t) ~ N(mu + e^(-phi dt) (alpha(t) - mu), sigma_eta^2 (1 - e^(-2 phi dt)) / (2 phi)),  phi the
mean-reversion rate.  Its three calls are dlm_sv_mixture_batch, dlm_ou_ffbs_batch and dlm_sv_ou_params_batch (Metropolis moves of phi,
sigma_eta, mu).  Its `InverseGamma` prior is on sigma_eta ITSELF, as the reference evaluates it -- the one
difference between the two samplers' priors.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Iterator, Optional

import numpy as np

from . import _lib
from ._chain import host, or_status, place
from .gibbs import InverseGamma

MASK64 = (1 << 64) - 1


@dataclass(frozen=True)
class SvParameters:
    """SvParameters(phi, mu, sigmaEta) (StochasticVolatility.scala:12-25)."""
    phi: float
    mu: float
    sigma_eta: float


@dataclass(frozen=True)
class Gaussian:
    """Gaussian(mean, sd) as Breeze takes it: the second argument is the standard deviation."""
    mean: float
    sd: float

    def draw(self, rng: np.random.Generator):
        return self.mean + self.sd * rng.standard_normal()


@dataclass(frozen=True)
class Beta:
    a: float
    b: float

    def draw(self, rng: np.random.Generator):
        return rng.beta(self.a, self.b)


def initial_parameters(prior_phi, prior_mu: Gaussian, prior_sigma: InverseGamma, n_series: int, *, seed: int = 0,
                       series_offset: int = 0, sigma_squared: bool = True) -> np.ndarray:
    """(phi, mu, sigma_eta) [N][3] drawn from the priors on the host (sampleUni / sampleBeta, StochasticVolatility.scala:308-340) by a
    generator keyed by (seed, global series index) -- a sharded run starts where the single-GPU run does.  phi is redrawn until
    |phi| < 1 (inside (0, 1) for a Beta prior): the FFBS needs a stationary state.  sigma_squared=False: the InverseGamma is the
    prior of sigma_eta itself (sample_ou), not of its square."""
    beta = isinstance(prior_phi, Beta)
    out = np.empty((n_series, 3))
    for k in range(n_series):
        rng = np.random.default_rng([int(seed), int(series_offset) + k, 0x5356])
        phi = float(prior_phi.draw(rng))
        while not ((0.0 < phi < 1.0) if beta else (abs(phi) < 1.0)):
            phi = float(prior_phi.draw(rng))
        mu = float(prior_mu.draw(rng))
        sig = float(prior_sigma.draw(rng))
        out[k] = (phi, mu, np.sqrt(sig) if sigma_squared else sig)
    return out


def sample_knots(min_size: int, max_size: int, T: int, rng: np.random.Generator) -> np.ndarray:
    """The knots of one sweep of the block sampler over the T + 1 states alpha[0..T]: block sizes uniform on [min_size, max_size],
    accumulated until they cover every state -> int32 [B+1], 0 = knots[0] < ... < knots[B] = T + 1, block i the states
    knots[i] .. knots[i+1] - 1 (the last block may be shorter than min_size).  The corrected sampleKnots (StochVolKnots.scala:237-256;
    DESIGN.md 2, Q64-Q65): the reference's knots end at n - 1 and come from scala.util.Random."""
    if not 1 <= int(min_size) <= int(max_size):
        raise ValueError(f"block sizes need 1 <= min_size <= max_size, got {min_size}, {max_size}")
    if T < 1:
        raise ValueError("T must be >= 1")
    knots = [0]
    while knots[-1] < T + 1:
        knots.append(min(knots[-1] + int(rng.integers(int(min_size), int(max_size) + 1)), T + 1))
    return np.asarray(knots, dtype=np.int32)


def knots_rng(seed: int, iteration: int) -> np.random.Generator:
    """The host generator of iteration `iteration`'s knots: keyed by (seed, iteration) alone, so every shard of a batch cuts its paths
    at the same places."""
    return np.random.default_rng([int(seed) & MASK64, int(iteration), 0x4B4E])


class StochasticVolatility:
    @dataclass
    class State:
        """StochVolState (StochasticVolatility.scala), batched: params [N][3] = (phi, mu, sigma_eta) on the host, alpha [N][T+1] a host
        copy when asked for (keep_alpha) else None, accepted [N] (the Beta proposal's acceptances so far; zeros for sample_uni;
        [N][3] for sample_ou: the acceptances of phi, sigma_eta, mu), status [N]: the three calls' flags or'ed."""
        params: np.ndarray
        alpha: Optional[np.ndarray]
        accepted: np.ndarray
        status: np.ndarray
        accepted_blocks: Optional[np.ndarray] = None   # StochasticVolatilityKnots: [N], the blocks of the state sweeps accepted so far

    @staticmethod
    def simulate(p: SvParameters, T: int, N: int, seed: int = 0):
        """StochasticVolatility.simulate (:66-72) for N series with NumPy: (y [N][T], alpha [N][T+1]), alpha[:, 0] the stationary
        initial state.  For tests and benchmarks."""
        rng = np.random.default_rng(seed)
        alpha = np.empty((N, T + 1))
        alpha[:, 0] = p.mu + p.sigma_eta / np.sqrt(1.0 - p.phi * p.phi) * rng.standard_normal(N)
        eta = rng.standard_normal((N, T)) * p.sigma_eta
        for t in range(T):
            alpha[:, t + 1] = p.mu + p.phi * (alpha[:, t] - p.mu) + eta[:, t]
        y = rng.standard_normal((N, T)) * np.exp(0.5 * alpha[:, 1:])
        return y, alpha

    @staticmethod
    def simulate_ou(p: SvParameters, times, N: int, seed: int = 0):
        """StochasticVolatility.simOu for N series with NumPy on the grid times [T]: (y [N][T], alpha [N][T+1]) in the layout of
        dlm_ou_ffbs_batch's theta -- alpha[:, 0] ~ N(mu, sigma_eta^2) and alpha[:, 1] = alpha[:, 0] both sit at times[0], alpha[:, t]
        at times[t-1].  For tests and benchmarks."""
        times = np.asarray(times, dtype=np.float64)
        T = times.size
        rng = np.random.default_rng(seed)
        alpha = np.empty((N, T + 1))
        alpha[:, 0] = p.mu + p.sigma_eta * rng.standard_normal(N)
        alpha[:, 1] = alpha[:, 0]
        z = rng.standard_normal((N, T))
        for t in range(2, T + 1):
            dt = times[t - 1] - times[t - 2]
            if dt == 0.0:          # a repeated time: the state stays, bit for bit
                alpha[:, t] = alpha[:, t - 1]
                continue
            sd = p.sigma_eta * np.sqrt(-np.expm1(-2.0 * p.phi * dt) / (2.0 * p.phi))
            alpha[:, t] = p.mu + np.exp(-p.phi * dt) * (alpha[:, t - 1] - p.mu) + sd * z[:, t - 1]
        y = rng.standard_normal((N, T)) * np.exp(0.5 * alpha[:, 1:])
        return y, alpha

    @staticmethod
    def _seed_ffbs(seed, k):
        # the FFBS normals are keyed by (seed, series, t) alone: a seed per FFBS call, k = 0 the initial state's
        return (int(seed) * 1000003 + k) & MASK64

    @staticmethod
    def initial_state_ar(y, sv, engine, *, seed: int = 0, series_offset: int = 0, ffbs: Optional[Callable] = None,
                         mixture: Optional[Callable] = None, out=None, times=None):
        """initialStateAr (StochVolKnots.scala:345-352): one FFBS on ystar = log y^2 + 1.27 with v = pi^2 / 2 at every step.
        Returns {"alpha" [N][T+1], "ystar", "v", "status"}.  times [T]: initialStateOu (StochasticVolatility.scala:480-487), the
        Ornstein-Uhlenbeck FFBS on that grid."""
        grid = {} if times is None else {"times": times}
        run_mix = mixture if mixture is not None else engine.sv_mixture
        run_ffbs = ffbs if ffbs is not None else engine.ar1_ffbs
        mix = run_mix(y, None, iteration=0, seed=seed, series_offset=series_offset, out=out)
        f = run_ffbs(mix["ystar"], mix["v"], sv, seed=StochasticVolatility._seed_ffbs(seed, 0), series_offset=series_offset,
                     want_filt=False, want_theta=True, **grid)
        return {"alpha": f["theta"], "ystar": mix["ystar"], "v": mix["v"], "status": or_status(mix.get("status"), f.get("status"))}

    @staticmethod
    def sample_state_ar(y, alpha, sv, engine, *, iteration: int, seed: int = 0, series_offset: int = 0,
                        ffbs: Optional[Callable] = None, mixture: Optional[Callable] = None, out=None, times=None):
        """sampleStateAr (StochasticVolatility.scala:142-162): the mixture indicators given alpha, then the FFBS draw of alpha.
        Returns {"alpha" [N][T+1], "ystar", "v", "status"}; out: the "ystar" / "v" buffers to reuse.  times [T]: sampleStateOu
        (:433-452), the Ornstein-Uhlenbeck FFBS on that grid."""
        grid = {} if times is None else {"times": times}
        run_mix = mixture if mixture is not None else engine.sv_mixture
        run_ffbs = ffbs if ffbs is not None else engine.ar1_ffbs
        mix = run_mix(y, alpha, iteration=iteration, seed=seed, series_offset=series_offset, out=out)
        f = run_ffbs(mix["ystar"], mix["v"], sv, seed=StochasticVolatility._seed_ffbs(seed, iteration + 1), series_offset=series_offset,
                     want_filt=False, want_theta=True, **grid)
        return {"alpha": f["theta"], "ystar": mix["ystar"], "v": mix["v"], "status": or_status(mix.get("status"), f.get("status"))}

    @staticmethod
    def _sample(ys, prior, beta, prior_phi, prior_mu, prior_sigma, engine, *, n_iter, seed, params0, series_offset, keep_alpha,
                ffbs, mixture, params, times=None, knots=None, sweep=None):
        # times [T]: the Ornstein-Uhlenbeck chain on that grid (sample_ou) -- the FFBS calls take the grid, the parameter call is
        # sv_ou_params with the grid in front and `accepted` is [N][3]; everything else is the AR(1) chain's plumbing
        # knots = (min_size, max_size): the state step is ONE sv_knots sweep (StochasticVolatilityKnots) over knots drawn on the host
        # from a generator keyed by (seed, iteration) -- the same for every shard -- and its acceptances are counted apart
        ou = times is not None
        N, T = int(ys.shape[0]), int(ys.shape[1])
        if T < 2:
            raise ValueError("the stochastic-volatility sampler needs T >= 2 (the reference's sums throw on a single observation)")
        run_params = params if params is not None else (engine.sv_ou_params if ou else engine.sv_params)
        put, y = place(ys, engine, N, T)
        if params0 is None:
            sv_h = initial_parameters(prior_phi, prior_mu, prior_sigma, N, seed=seed, series_offset=series_offset, sigma_squared=not ou)
        else:
            p0 = (params0.phi, params0.mu, params0.sigma_eta) if isinstance(params0, SvParameters) else params0
            sv_h = np.broadcast_to(np.asarray(p0, dtype=np.float64), (N, 3)).copy()
            bad = ~((sv_h[:, 0] > 0.0) & (sv_h[:, 0] < 1.0)) if beta else ~(np.abs(sv_h[:, 0]) < 1.0)
            if bad.any() or not (sv_h[:, 2] > 0.0).all():
                raise ValueError("initial parameters need a stationary phi (inside (0, 1) for the Beta proposal) and sigma_eta > 0")
        sv = put(sv_h)
        acc = put(np.zeros((N, 3) if ou else N, dtype=np.int32), np.int32)
        grid, lead = {}, ()
        if ou:
            tgrid = host(times).astype(np.float64)
            if tgrid.shape != (T,):
                raise ValueError(f"times must be [T] = {(T,)}, got {tgrid.shape}")
            tgrid = put(tgrid)
            grid, lead = {"times": tgrid}, (tgrid,)
        st = StochasticVolatility.initial_state_ar(y, sv, engine, seed=seed, series_offset=series_offset, ffbs=ffbs, mixture=mixture,
                                                   **grid)
        alpha, bufs, status0 = st["alpha"], {"ystar": st["ystar"], "v": st["v"]}, st["status"]
        blocks = put(np.zeros(N, dtype=np.int32), np.int32) if knots is not None else None
        for it in range(n_iter):
            if knots is not None:
                kn = sample_knots(knots[0], knots[1], T, knots_rng(seed, it))
                run_sweep = sweep if sweep is not None else engine.sv_knots
                st = run_sweep(y, alpha, sv, kn, iteration=it, accepted=blocks, seed=seed, series_offset=series_offset,
                               out={"alpha": alpha})
                alpha, blocks = st["alpha"], st["accepted"]
            else:
                st = StochasticVolatility.sample_state_ar(y, alpha, sv, engine, iteration=it, seed=seed, series_offset=series_offset,
                                                          ffbs=ffbs, mixture=mixture, out=bufs, **grid)
                alpha, bufs = st["alpha"], {"ystar": st["ystar"], "v": st["v"]}
            res = run_params(*lead, alpha, sv, prior, iteration=it, accepted=acc, seed=seed, series_offset=series_offset,
                             out={"sv": sv})
            sv, acc = res["sv"], res["accepted"]
            status = or_status(st["status"], res.get("status"))
            if it == 0:
                status = or_status(status, status0)
            yield StochasticVolatility.State(host(sv).copy(), host(alpha).copy() if keep_alpha else None,
                                             host(acc).astype(np.int32), status,
                                             None if blocks is None else host(blocks).astype(np.int32))

    @staticmethod
    def sample_uni(ys, prior_phi: Gaussian, prior_mu: Gaussian, prior_sigma: InverseGamma, engine, *, n_iter: int, seed: int = 0,
                   params0=None, literal: bool = False, series_offset: int = 0, keep_alpha: bool = False,
                   ffbs: Optional[Callable] = None, mixture: Optional[Callable] = None,
                   params: Optional[Callable] = None) -> Iterator["StochasticVolatility.State"]:
        """StochasticVolatility.sampleUni (:323-341) for N independent series: ys [N][T] (NaN = missing; numpy or a torch device
        tensor).  phi is drawn from its Gaussian conjugate conditional, restricted to (-1, 1) unless literal.  Yields one State per
        iteration.  params0: the initial (phi, mu, sigma_eta) -- an SvParameters, a triple or an [N][3] array; None draws them from
        the priors (initial_parameters).  ffbs= / mixture= / params= replace engine.ar1_ffbs / sv_mixture / sv_params, for tests."""
        if not isinstance(prior_phi, Gaussian) or not isinstance(prior_mu, Gaussian) or not isinstance(prior_sigma, InverseGamma):
            raise TypeError("the device evaluates a Gaussian prior of phi and of mu and an InverseGamma prior of sigma_eta^2 only")
        prior = _lib.SvPrior(0, 1 if literal else 0, prior_phi.mean, prior_phi.sd, prior_mu.mean, prior_mu.sd, prior_sigma.shape,
                             prior_sigma.scale, 100.0, 0.05)
        return StochasticVolatility._sample(ys, prior, False, prior_phi, prior_mu, prior_sigma, engine, n_iter=n_iter, seed=seed,
                                            params0=params0, series_offset=series_offset, keep_alpha=keep_alpha, ffbs=ffbs,
                                            mixture=mixture, params=params)

    @staticmethod
    def sample_beta(ys, prior_phi: Beta, prior_mu: Gaussian, prior_sigma: InverseGamma, engine, *, n_iter: int, seed: int = 0,
                    params0=None, literal: bool = False, series_offset: int = 0, keep_alpha: bool = False,
                    prop_lambda: float = 100.0, prop_tau: float = 0.05, ffbs: Optional[Callable] = None,
                    mixture: Optional[Callable] = None, params: Optional[Callable] = None) -> Iterator["StochasticVolatility.State"]:
        """StochasticVolatility.sampleBeta (:303-321): as sample_uni with phi in (0, 1) moved by Metropolis-Hastings, proposal
        Beta(lambda phi + tau, lambda (1 - phi) + tau) (the reference passes 100, 0.05), prior Beta(a, b)."""
        if not isinstance(prior_phi, Beta) or not isinstance(prior_mu, Gaussian) or not isinstance(prior_sigma, InverseGamma):
            raise TypeError("the device evaluates a Beta prior of phi, a Gaussian prior of mu and an InverseGamma prior of sigma_eta^2 only")
        prior = _lib.SvPrior(1, 1 if literal else 0, prior_phi.a, prior_phi.b, prior_mu.mean, prior_mu.sd, prior_sigma.shape,
                             prior_sigma.scale, float(prop_lambda), float(prop_tau))
        return StochasticVolatility._sample(ys, prior, True, prior_phi, prior_mu, prior_sigma, engine, n_iter=n_iter, seed=seed,
                                            params0=params0, series_offset=series_offset, keep_alpha=keep_alpha, ffbs=ffbs,
                                            mixture=mixture, params=params)

    @staticmethod
    def sample_ou(times, ys, prior_phi: Beta, prior_mu: Gaussian, prior_sigma: InverseGamma, engine, *, n_iter: int, seed: int = 0,
                  params0=None, literal: bool = False, series_offset: int = 0, keep_alpha: bool = False, prop_lambda: float = 10.0,
                  prop_tau: float = 0.05, delta_sigma: float = 0.05, delta_mu: float = 0.05, ffbs: Optional[Callable] = None,
                  mixture: Optional[Callable] = None, params: Optional[Callable] = None) -> Iterator["StochasticVolatility.State"]:
        """StochasticVolatility.sampleOu (:489-500) for N independent series observed at the shared times [T]: ys [N][T] (NaN = missing),
        the log-volatility an Ornstein-Uhlenbeck process with rate phi in (0, 1), mean mu and volatility sigma_eta.  Per iteration
        sv_mixture, ar1_ffbs(times=...), sv_ou_params: Metropolis moves of phi (Beta(lambda phi + tau, lambda (1 - phi) + tau) proposal,
        Beta prior), sigma_eta (log-normal walk of sd delta_sigma; the InverseGamma prior is on sigma_eta ITSELF, where
        sample_uni / sample_beta take it on sigma_eta^2) and mu (Gaussian walk of sd delta_mu), State.accepted [N][3] in that order.
        The proposal arguments default to the reference signatures' own (10, 0.05, 0.05, 0.05).  literal=True runs the reference's
        arithmetic and passes lambda = 0.05, as stepOu does by handing 0.05 to the `lambda` parameter (Q22).
        Everything else as sample_uni; ffbs= / mixture= / params= replace engine.ar1_ffbs / sv_mixture / sv_ou_params, for tests."""
        if not isinstance(prior_phi, Beta) or not isinstance(prior_mu, Gaussian) or not isinstance(prior_sigma, InverseGamma):
            raise TypeError("the device evaluates a Beta prior of phi, a Gaussian prior of mu and an InverseGamma prior of sigma_eta only")
        prior = _lib.SvOuPrior(1 if literal else 0, prior_phi.a, prior_phi.b, prior_mu.mean, prior_mu.sd, prior_sigma.shape,
                               prior_sigma.scale, 0.05 if literal else float(prop_lambda), float(prop_tau), float(delta_sigma),
                               float(delta_mu))
        return StochasticVolatility._sample(ys, prior, True, prior_phi, prior_mu, prior_sigma, engine, n_iter=n_iter, seed=seed,
                                            params0=params0, series_offset=series_offset, keep_alpha=keep_alpha, ffbs=ffbs,
                                            mixture=mixture, params=params, times=times)



class StochasticVolatilityKnots:
    """The stochastic-volatility sampler whose state step is the knot block sampler (StochasticVolatilityKnots.sampleParametersAr /
    sampleArBeta, StochVolKnots.scala:291-379): per iteration the knots are drawn on the host (sample_knots from knots_rng(seed,
    iteration)), ONE dlm_sv_knots_batch sweep moves alpha in place -- every block proposed from the Gaussian approximation
    log y^2 + 1.27 ~ N(alpha, pi^2 / 2) given its neighbours and corrected by a Metropolis step, so the chain's invariant law is the
    posterior of the model itself, not of the seven-component mixture -- and dlm_sv_params_batch draws (phi, mu, sigma) as in
    StochasticVolatility.sample_uni / sample_beta.  The chain starts from initial_state_ar.  State.accepted keeps its meaning (the
    Beta proposal's acceptances); State.accepted_blocks [N] counts the accepted blocks.  There is no literal mode of the state step
    (DESIGN.md 2, Q63-Q66); literal=True is the parameter step's (Q16-Q19)."""

    State = StochasticVolatility.State

    @staticmethod
    def _check_sizes(min_size, max_size):
        if int(min_size) != min_size or int(max_size) != max_size or not 1 <= min_size <= max_size:
            raise ValueError(f"block sizes need integers 1 <= min_size <= max_size, got {min_size}, {max_size}")
        return int(min_size), int(max_size)

    @staticmethod
    def sample_ar(ys, prior_phi: Gaussian, prior_mu: Gaussian, prior_sigma: InverseGamma, engine, *, n_iter: int, min_size: int = 10,
                  max_size: int = 100, seed: int = 0, params0=None, literal: bool = False, series_offset: int = 0,
                  keep_alpha: bool = False, ffbs: Optional[Callable] = None, mixture: Optional[Callable] = None,
                  params: Optional[Callable] = None, sweep: Optional[Callable] = None) -> Iterator["StochasticVolatility.State"]:
        """sampleParametersAr (:354-369) for N independent series: ys [N][T] (NaN = missing; numpy or a torch device tensor), phi from
        its Gaussian conjugate conditional on (-1, 1).  min_size / max_size: the block sizes of sample_knots (the reference passes 10,
        100).  Everything else as StochasticVolatility.sample_uni; sweep= replaces engine.sv_knots, for tests."""
        if not isinstance(prior_phi, Gaussian) or not isinstance(prior_mu, Gaussian) or not isinstance(prior_sigma, InverseGamma):
            raise TypeError("the device evaluates a Gaussian prior of phi and of mu and an InverseGamma prior of sigma_eta^2 only")
        knots = StochasticVolatilityKnots._check_sizes(min_size, max_size)
        prior = _lib.SvPrior(0, 1 if literal else 0, prior_phi.mean, prior_phi.sd, prior_mu.mean, prior_mu.sd, prior_sigma.shape,
                             prior_sigma.scale, 100.0, 0.05)
        return StochasticVolatility._sample(ys, prior, False, prior_phi, prior_mu, prior_sigma, engine, n_iter=n_iter, seed=seed,
                                            params0=params0, series_offset=series_offset, keep_alpha=keep_alpha, ffbs=ffbs,
                                            mixture=mixture, params=params, knots=knots, sweep=sweep)

    @staticmethod
    def sample_ar_beta(ys, prior_phi: Beta, prior_mu: Gaussian, prior_sigma: InverseGamma, engine, *, n_iter: int, min_size: int = 10,
                       max_size: int = 100, seed: int = 0, params0=None, literal: bool = False, series_offset: int = 0,
                       keep_alpha: bool = False, prop_lambda: float = 100.0, prop_tau: float = 0.05, ffbs: Optional[Callable] = None,
                       mixture: Optional[Callable] = None, params: Optional[Callable] = None,
                       sweep: Optional[Callable] = None) -> Iterator["StochasticVolatility.State"]:
        """sampleArBeta (:371-379): as sample_ar with phi in (0, 1) moved by Metropolis-Hastings, proposal
        Beta(lambda phi + tau, lambda (1 - phi) + tau) (the reference passes 100, 0.05), prior Beta(a, b)."""
        if not isinstance(prior_phi, Beta) or not isinstance(prior_mu, Gaussian) or not isinstance(prior_sigma, InverseGamma):
            raise TypeError("the device evaluates a Beta prior of phi, a Gaussian prior of mu and an InverseGamma prior of sigma_eta^2 only")
        knots = StochasticVolatilityKnots._check_sizes(min_size, max_size)
        prior = _lib.SvPrior(1, 1 if literal else 0, prior_phi.a, prior_phi.b, prior_mu.mean, prior_mu.sd, prior_sigma.shape,
                             prior_sigma.scale, float(prop_lambda), float(prop_tau))
        return StochasticVolatility._sample(ys, prior, True, prior_phi, prior_mu, prior_sigma, engine, n_iter=n_iter, seed=seed,
                                            params0=params0, series_offset=series_offset, keep_alpha=keep_alpha, ffbs=ffbs,
                                            mixture=mixture, params=params, knots=knots, sweep=sweep)
