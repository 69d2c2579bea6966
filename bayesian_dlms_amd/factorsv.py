"""Gibbs sampler of the factor stochastic-volatility model on the device (FactorSv.sampleAr, FactorSv.scala:546-562, :622-645).

  y_t = beta f_t + eps_t,  eps_t ~ N(0, diag(v)),  f_{j,t} ~ N(0, exp(alpha_{j,t})),  alpha_j AR(1) with SvParameters (phi, mu, sigma_eta)_j
  beta p x k: beta_ii = 1, beta_ij = 0 for j > i, beta_ij ~ Gaussian(mean, sd) elsewhere;  v = sigma^2 1_p, sigma^2 ~ InverseGamma

A batch is N independent panels of p series, T times and k factors (1 <= k <= 8, k <= p <= 64); ys is [N][T][p], NaN = missing, and a
partially missing time is wholly missing (encodePartiallyMissing, :150-157).  One iteration is five engine calls, in sampleStep's order:

  dlm_sv_mixture_batch, dlm_ar1_ffbs_batch, dlm_sv_params_batch   on the N k factor series f viewed as [N k][T]: chain (n, j) is the
                                                                  series (series_offset + n) k + j of those calls
  dlm_fsv_factors_batch                                           f_t | (y_t, beta, v, alpha_{t+1})
  dlm_fsv_loadings_batch                                          sigma^2 | (y, f, beta), then beta | (y, f, sigma^2) row by row

The chain state -- f [N][k][T], alpha [N][k][T+1], sv [N][k][3], beta [N][p][k], v [N][p] -- never leaves the device between
iterations; per iteration the parameters and the status cross to the host, plus f and alpha when asked for (keep_factors).

The default is the corrected sampler (DESIGN.md 2, Q27-Q30, and Q16-Q19 of the volatility parameters); literal=True runs the
reference's arithmetic in all five calls.  Q31: the reference's sampleStep draws the volatility state with the knot block sampler,
which is not offered; the driver uses the reference's own alternative FactorSv.sampleVolatilityAr (:415-435), the mixture and FFBS
draw of StochasticVolatility.sampleStateAr.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterator, Optional, Sequence

import numpy as np

from . import _lib
from ._chain import host, or_status, place
from .gibbs import InverseGamma
from .stochvol import MASK64, Gaussian, StochasticVolatility, SvParameters

MAX_K, MAX_P = 8, 64
# the iteration index of initialiseFactors' normals: they share the stream of the iterations' factor draws, whose indices count from 0
INIT_ITERATION = MASK64


@dataclass
class FsvParameters:
    """FsvParameters(v, beta, factorParams) (FactorSv.scala:20-60): v a scalar (sigma^2) or the diagonal [p] of the observation
    variance, beta [p][k], factor_params k SvParameters (or a [k][3] array of (phi, mu, sigma_eta))."""
    v: object
    beta: np.ndarray
    factor_params: Sequence

    def __post_init__(self):
        self.beta = np.asarray(self.beta, dtype=np.float64)
        if self.beta.ndim != 2:
            raise ValueError(f"beta must be [p][k], got the shape {self.beta.shape}")
        p, k = self.beta.shape
        if not (1 <= k <= MAX_K and k <= p <= MAX_P):
            raise ValueError(f"1 <= k <= {MAX_K} and k <= p <= {MAX_P}: got p = {p}, k = {k}")
        v = np.asarray(self.v, dtype=np.float64)
        if v.ndim == 2:
            v = np.diagonal(v)
        self.v = np.broadcast_to(v, (p,)).copy()
        if not (self.v > 0.0).all():
            raise ValueError("the observation variances must be positive")
        sv = np.asarray([(q.phi, q.mu, q.sigma_eta) if isinstance(q, SvParameters) else q for q in self.factor_params], dtype=np.float64)
        if sv.shape != (k, 3):
            raise ValueError(f"factor_params must hold k = {k} (phi, mu, sigma_eta) triples, got the shape {sv.shape}")
        if not ((np.abs(sv[:, 0]) < 1.0).all() and (sv[:, 2] > 0.0).all()):
            raise ValueError("every factor needs a stationary phi and sigma_eta > 0")
        self.factor_params = [SvParameters(*row) for row in sv]

    @property
    def p(self):
        return self.beta.shape[0]

    @property
    def k(self):
        return self.beta.shape[1]

    def sv(self):
        """[k][3] = (phi, mu, sigma_eta) per factor."""
        return np.asarray([(q.phi, q.mu, q.sigma_eta) for q in self.factor_params], dtype=np.float64)


def panel_dims(ys):
    """(N, T, p) of a batch of panels ys [N][T][p], as every sampler with a factor stochastic-volatility part takes it."""
    if len(ys.shape) != 3:
        raise ValueError(f"ys must be [N][T][p], got the shape {tuple(ys.shape)}")
    N, T, p = (int(x) for x in ys.shape)
    if T < 2:
        raise ValueError("the factor stochastic-volatility sampler needs T >= 2 (the reference's sums throw on a single observation)")
    return N, T, p


class FactorSv:
    @dataclass
    class State:
        """FactorSv.State (FactorSv.scala:62-66), batched.  params: {"beta" [N][p][k], "v" [N][p], "sv" [N][k][3]} on the host;
        factors [N][k][T] and volatility [N][k][T+1] host copies when asked for (keep_factors) else None; status [N]: the five calls'
        flags or'ed (the factor chains' flags folded onto their panel)."""
        params: dict
        factors: Optional[np.ndarray]
        volatility: Optional[np.ndarray]
        status: np.ndarray

    @staticmethod
    def make_beta(p: int, k: int) -> np.ndarray:
        """makeBeta (:295-304): ones on the diagonal, zeros elsewhere."""
        return FactorSv.build_beta(p, k, lambda: 0.0)

    @staticmethod
    def build_beta(p: int, k: int, prior) -> np.ndarray:
        """buildBeta (:94-106): beta_ii = 1, beta_ij = 0 for j > i, one call of prior() for every entry below the diagonal (row by
        row); prior may also be a number."""
        if not (1 <= k <= MAX_K and k <= p <= MAX_P):
            raise ValueError(f"1 <= k <= {MAX_K} and k <= p <= {MAX_P}: got p = {p}, k = {k}")
        draw = prior if callable(prior) else (lambda: prior)
        beta = np.zeros((p, k))
        for i in range(p):
            for j in range(k):
                beta[i, j] = 1.0 if i == j else (float(draw()) if i > j else 0.0)
        return beta

    @staticmethod
    def simulate(params: FsvParameters, T: int, N: int, seed: int = 0):
        """FactorSv.simulate (:108-142) for N panels with NumPy: (y [N][T][p], f [N][k][T], alpha [N][k][T+1]), alpha[:, j, 0] the
        stationary initial state of factor j.  For tests and benchmarks."""
        rng = np.random.default_rng(seed)
        p, k = params.p, params.k
        sv = params.sv()
        phi, mu, sig = sv[:, 0], sv[:, 1], sv[:, 2]
        alpha = np.empty((N, k, T + 1))
        alpha[:, :, 0] = mu + sig / np.sqrt(1.0 - phi * phi) * rng.standard_normal((N, k))
        for t in range(T):
            alpha[:, :, t + 1] = mu + phi * (alpha[:, :, t] - mu) + sig * rng.standard_normal((N, k))
        f = rng.standard_normal((N, k, T)) * np.exp(0.5 * alpha[:, :, 1:])
        y = np.einsum("ij,njt->nti", params.beta, f) + np.sqrt(params.v) * rng.standard_normal((N, T, p))
        return y, f, alpha

    @staticmethod
    def _shape(ys, init_p):
        N, T, p = panel_dims(ys)
        if p != init_p.p:
            raise ValueError(f"ys has p = {p} series, the initial beta {init_p.p} rows")
        return N, T, p, init_p.k

    @staticmethod
    def initialise_state_ar(ys, init_p: FsvParameters, engine, *, seed: int = 0, series_offset: int = 0, literal: bool = False):
        """initialiseStateAr (:595-610): initialiseFactors (:571-590; the factor draw with unit factor variances), then
        StochasticVolatility.initial_state_ar on every factor series.  Returns the device-resident chain state {"y", "f" [N][k][T],
        "alpha" [N][k][T+1], "sv" [N][k][3], "beta" [N][p][k], "v" [N][p], "ystar", "v_mix" (the mixture call's buffers), "status"}."""
        N, T, p, k = FactorSv._shape(ys, init_p)
        put, y = place(ys, engine, N, T * p)
        y = y.reshape(N, T, p)
        beta = put(np.broadcast_to(init_p.beta, (N, p, k)))
        v = put(np.broadcast_to(init_p.v, (N, p)))
        sv = put(np.broadcast_to(init_p.sv(), (N, k, 3)))
        fac = engine.fsv_factors(y, beta, v, None, iteration=INIT_ITERATION, seed=seed, series_offset=series_offset, literal=literal)
        f = fac["f"]
        st = StochasticVolatility.initial_state_ar(f.reshape(N * k, T), sv.reshape(N * k, 3), engine, seed=seed,
                                                   series_offset=series_offset * k)
        status = or_status(fac["status"], FactorSv._fold(st["status"], N, k))
        return {"y": y, "f": f, "alpha": st["alpha"].reshape(N, k, T + 1), "sv": sv, "beta": beta, "v": v, "ystar": st["ystar"],
                "v_mix": st["v"], "status": status}

    @staticmethod
    def _fold(status, N, k):
        """The [N k] flags of the factor chains or'ed onto their panels."""
        return None if status is None else np.bitwise_or.reduce(host(status).astype(np.int32).reshape(N, k), axis=1)

    @staticmethod
    def sample_ar(prior_beta: Gaussian, prior_sigma_eta: InverseGamma, prior_mu: Gaussian, prior_phi: Gaussian, prior_sigma: InverseGamma,
                  ys, init_p: FsvParameters, engine, *, n_iter: int, seed: int = 0, series_offset: int = 0, literal: bool = False,
                  keep_factors: bool = True) -> Iterator["FactorSv.State"]:
        """FactorSv.sampleAr (:622-645) for N independent panels: ys [N][T][p] (NaN = missing; numpy or a torch device tensor), every
        panel started at init_p.  prior_beta: the Gaussian(mean, sd) of the free loadings; prior_sigma_eta, prior_mu, prior_phi: the
        priors of sample_uni for every factor's (sigma_eta^2, mu, phi); prior_sigma: the InverseGamma of sigma^2.  Yields one State per
        iteration."""
        priors = pack_priors(prior_beta, prior_sigma_eta, prior_mu, prior_phi, prior_sigma, literal)
        if not isinstance(init_p, FsvParameters):
            raise TypeError("init_p must be an FsvParameters")
        FactorSv._shape(ys, init_p)
        return FactorSv._run(ys, init_p, engine, priors, n_iter, seed, series_offset, literal, keep_factors)

    @staticmethod
    def _run(ys, init_p, engine, priors, n_iter, seed, series_offset, literal, keep_factors):
        c = FactorSv.initialise_state_ar(ys, init_p, engine, seed=seed, series_offset=series_offset, literal=literal)
        N, k = int(c["f"].shape[0]), int(c["f"].shape[1])
        for it in range(n_iter):
            st = factor_half(engine, c, c["y"], priors, iteration=it, seed=seed, series_offset=series_offset, literal=literal,
                             factors_last=True)
            status = fold_status(st, N, k, c["status"] if it == 0 else None)
            params = {"beta": host(c["beta"]).copy(), "v": host(c["v"]).copy(), "sv": host(c["sv"]).copy()}
            yield FactorSv.State(params, *(host(c[key]).copy() if keep_factors else None for key in ("f", "alpha")), status)

    @staticmethod
    def forecast(draws, horizon: int, engine, *, n_paths: int = 64, prob: float = 0.75, probs=None, seed: int = 0, series_offset: int = 0,
                 budget=None):
        """The posterior predictive of y_{T+1 .. T+horizon} from kept draws: given a draw and a future log-volatility
        path, y_{T+h} ~ N(0, beta diag(exp(alpha_{.,T+h})) beta^T + diag(v)); the paths start at the draw's alpha_T and follow
        StochasticVolatility.stepState, n_paths per draw.  draws: a list of the States of sample_ar kept with their factors, or a dict
        of stacked arrays {"beta" [M][N][p][k], "v" [M][N][p], "sv" [M][N][k][3], "alpha" [M][N][k][T+1]}.  Returns {"mean" [N][H][p]
        (zeros), "cov" [N][H][p][p] the predictive covariance matrices, "lower", "upper" [N][H][p] the exact mixture quantiles at
        1 - prob and prob (Dlm.summariseForecast's interval), "quantiles" [N][H][p][len(probs)] or None, "status" [N]}.  A pure
        forecast: no test data is taken.  budget: bytes of device memory the call may use (default: 60 % of what is free)."""
        from . import _dlmfsv
        return _dlmfsv.forecast(None, None, None, draws, horizon, engine, n_paths=n_paths, prob=prob, probs=probs, seed=seed,
                                series_offset=series_offset, budget=budget)


def pack_priors(prior_beta, prior_sigma_eta, prior_mu, prior_phi, prior_sigma, literal, also=None):
    """The priors of the factor part, checked and packed for the device: (_lib.SvPrior of every factor's (phi, mu, sigma_eta^2) with the
    conjugate phi update, _lib.FsvPrior of the loadings and sigma^2).  also: (name, prior) of one more InverseGamma the caller's sampler
    takes, checked with them."""
    inverse_gammas = (prior_sigma_eta, prior_sigma) + (() if also is None else (also[1],))
    if not (all(isinstance(q, Gaussian) for q in (prior_beta, prior_mu, prior_phi)) and all(isinstance(q, InverseGamma) for q in inverse_gammas)):
        raise TypeError("the device evaluates Gaussian priors of beta, mu and phi and InverseGamma priors of sigma_eta^2"
                        + (" and sigma^2" if also is None else f", sigma^2 and {also[0]}") + " only")
    lit = 1 if literal else 0
    sv_prior = _lib.SvPrior(0, lit, prior_phi.mean, prior_phi.sd, prior_mu.mean, prior_mu.sd, prior_sigma_eta.shape, prior_sigma_eta.scale,
                            100.0, 0.05)
    return sv_prior, _lib.FsvPrior(lit, prior_beta.mean, prior_beta.sd, prior_sigma.shape, prior_sigma.scale)


def factor_half(engine, c, x, priors, *, iteration, seed, series_offset, literal, factors_last):
    """The factor model's part of one iteration on the chain state c (initialise_state_ar's dict) and the factor model's data x
    [N][T][p], c updated in place with the buffers c holds reused:

      f | x, alpha, beta, v                     before the volatility draw, or after the parameters of the volatility (factors_last:
                                                sampleStep's order, where the next volatility draw conditions on this f)
      alpha | f, then (phi, mu, sigma_eta) | alpha      on the N k factor series
      sigma^2, beta | x, f

    priors: pack_priors' pair.  Returns the calls' status flags by name, not yet or'ed: "factors" and "loadings" [N]; "volatility" (the
    mixture and the FFBS call of sample_state_ar, or'ed there) and "sv_params" [N k], which fold_status folds onto their panels."""
    sv_prior, fsv_prior = priors
    N, k, T = (int(n) for n in c["f"].shape)
    it, so = iteration, series_offset

    def draw_factors():
        return engine.fsv_factors(x, c["beta"], c["v"], c["alpha"], iteration=it, seed=seed, series_offset=so, literal=literal,
                                  out={"f": c["f"]})

    fac = None if factors_last else draw_factors()
    sv2 = c["sv"].reshape(N * k, 3)
    vol = StochasticVolatility.sample_state_ar(c["f"].reshape(N * k, T), c["alpha"].reshape(N * k, T + 1), sv2, engine, iteration=it,
                                               seed=seed, series_offset=so * k, out={"ystar": c["ystar"], "v": c["v_mix"]})
    c.update(alpha=vol["alpha"].reshape(N, k, T + 1), ystar=vol["ystar"], v_mix=vol["v"])
    res = engine.sv_params(vol["alpha"], sv2, sv_prior, iteration=it, seed=seed, series_offset=so * k, out={"sv": sv2})
    if factors_last:
        fac = draw_factors()
    load = engine.fsv_loadings(x, c["f"], c["beta"], fsv_prior, iteration=it, seed=seed, series_offset=so, v=c["v"],
                               out={"beta": c["beta"], "v": c["v"]})
    return {"factors": fac["status"], "volatility": vol["status"], "sv_params": res.get("status"), "loadings": load["status"]}


def fold_status(st, N, k, status0=None):
    """One iteration's status [N] from its calls' flags by name (factor_half's and whatever a driver adds): the factor chains' flags
    folded onto their panel, the panels' or'ed, and status0, the initialisation's, on top."""
    chains, status = or_status(st["volatility"], st["sv_params"]), status0
    for name, flags in st.items():
        if name not in ("volatility", "sv_params"):
            status = or_status(status, flags)
    return or_status(FactorSv._fold(chains, N, k), status)
