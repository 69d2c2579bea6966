"""Dynamic generalised linear models, the bootstrap particle filter, the particle-marginal Metropolis sampler built on it, the
Storvik filter, which learns the variances online, the Liu-West and auxiliary particle filters, the Rao-Blackwellised filter of a
Gaussian DLM and particle Gibbs (`ParticleGibbs`: conditional SMC with ancestor sampling, then the conjugate variance draws) (the reference's Dglm.scala, ParticleFilter.scala, Metropolis.dglm, MetropolisHastings.scala:142-154, Storvik.scala,
LiuAndWest.scala, AuxFilter.scala and RaoBlackwellFilter.scala).

A `Dglm` is a `Dlm` with one of six observation models for its scalar observation; V(0, 0) = v is what each family makes of it
(include/dlm_engine.h, dlm_pf_batch).  `ParticleFilter(n, n0).filter` runs the engine's filter for one series or a batch of them, with one
parameter set or one per series; `Metropolis.dglm` is a generator of particle-marginal Metropolis states, one chain per series, one engine
call per iteration, the proposal and the accept draws on the host.

The initial cloud sits AT the first observation time (ParticleFilter.initialiseState, ParticleFilter.scala:63-70: time = the smallest
observation time), so the first increment is 0 and the first step weights the initial cloud without advancing it -- the descriptor's dt == 0
convention (the reference multiplies by g(0) and draws with covariance 0 there: DESIGN.md 2, Q40)."""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from functools import reduce
from typing import Callable, Optional

import numpy as np

from . import _lib
from .api import pack_observations
from .dlm import Dlm, DlmParameters, MaterialisedModel, materialise
from .engine import (EngineError, check_pf_forecast_learned_lds, check_pf_ranks, check_pf_resample, check_pf_shape, check_rb_lds,
                     check_shrinkage)


def logistic_function(upper: float, number):
    """Dglm.logisticFunction (Dglm.scala:33-41): 0 below -5, `upper` above 5."""
    x = np.asarray(number, dtype=np.float64)
    with np.errstate(over="ignore"):
        mid = upper / (1.0 + np.exp(-x))
    return np.where(x < -5.0, 0.0, np.where(x > 5.0, upper, mid))


@dataclass(frozen=True)
class Dglm:
    """Dglm(observation, f, g, link, conditionalLikelihood) (Dglm.scala:14-23) with the observation model named instead of passed as
    closures: `family` one of _lib.OBS_*, `nu` the degrees of freedom of the Student-t family."""

    f: Callable[[float], np.ndarray]
    g: Callable[[float], np.ndarray]
    family: int = _lib.OBS_GAUSSIAN
    nu: Optional[float] = None

    @staticmethod
    def gaussian(mod: Dlm) -> "Dglm":
        """dlm2dglm (package.scala:13-28): y ~ N(eta, v)."""
        return Dglm(mod.f, mod.g, _lib.OBS_GAUSSIAN)

    @staticmethod
    def poisson(mod: Dlm) -> "Dglm":
        """Dglm.poisson (Dglm.scala:166-175): y ~ Poisson(exp(eta))."""
        return Dglm(mod.f, mod.g, _lib.OBS_POISSON)

    @staticmethod
    def negative_binomial(mod: Dlm) -> "Dglm":
        """Dglm.negativeBinomial (Dglm.scala:100-124): mean exp(eta), size exp(v)."""
        return Dglm(mod.f, mod.g, _lib.OBS_NEGBIN)

    @staticmethod
    def zip(mod: Dlm) -> "Dglm":
        """Dglm.zip (Dglm.scala:70-95): a zero with probability expit(v), else Poisson(exp(eta))."""
        return Dglm(mod.f, mod.g, _lib.OBS_ZIP)

    @staticmethod
    def student_t(nu: float, mod: Dlm) -> "Dglm":
        """Dglm.studentT (Dglm.scala:46-57): location eta, scale sqrt(v), nu degrees of freedom."""
        if not nu > 0:
            raise ValueError(f"the degrees of freedom must be positive, got {nu}")
        return Dglm(mod.f, mod.g, _lib.OBS_STUDENTT, float(nu))

    @staticmethod
    def beta(mod: Dlm) -> "Dglm":
        """Dglm.beta (Dglm.scala:132-161): mean logisticFunction(1)(eta), variance v < mean (1 - mean)."""
        return Dglm(mod.f, mod.g, _lib.OBS_BETA)

    @property
    def dlm(self) -> Dlm:
        return Dlm(self.f, self.g)

    def link(self, eta):
        """The mean function the reference calls `link`: eta for the Gaussian and Student-t families, exp(eta) for the counts, the logistic
        function for Beta."""
        eta = np.asarray(eta, dtype=np.float64)
        if self.family in (_lib.OBS_GAUSSIAN, _lib.OBS_STUDENTT):
            return eta
        if self.family == _lib.OBS_BETA:
            return logistic_function(1.0, eta)
        return np.exp(eta)

    def observation(self, eta: float, v: float, rng: np.random.Generator) -> float:
        """One draw of y | eta, v (the `observation` closures of Dglm.scala)."""
        fam = self.family
        if fam == _lib.OBS_GAUSSIAN:
            return float(rng.normal(eta, np.sqrt(v)))
        if fam == _lib.OBS_POISSON:
            return float(rng.poisson(np.exp(eta)))
        if fam == _lib.OBS_NEGBIN:
            size, mu = np.exp(v), np.exp(eta)
            prob = mu / (size + mu)
            return float(rng.poisson(rng.gamma(size, prob / (1.0 - prob))))
        if fam == _lib.OBS_ZIP:
            p = np.exp(v) / (1.0 + np.exp(v))
            u, nonzero = rng.uniform(), rng.poisson(np.exp(eta))
            return 0.0 if u < p else float(nonzero)
        if fam == _lib.OBS_STUDENTT:
            return float(eta + np.sqrt(v) * rng.standard_t(self.nu))
        mean = float(logistic_function(1.0, eta))
        a = mean * (1.0 - mean) / v
        return float(rng.beta(mean * (a - 1.0), (1.0 - mean) * (a - 1.0)))

    @staticmethod
    def interval_ranks(n: int, prob: float):
        """The indices Dglm.meanAndIntervals / medianAndIntervals read in a sorted sample of n (Dglm.scala:263-285): index = floor(n prob),
        upper = sorted[index], lower = sorted[n - index], median = sorted[floor(n / 2)] -> (lower, median, upper).  A prob whose indices fall
        outside [0, n) -- floor(n prob) = 0 reads sorted[n], floor(n prob) >= n reads sorted[index] past the end -- is refused with a ValueError;
        the reference indexes out of bounds there (Q73).  The same rule gives the ranks `forecast_particles` passes to the kernel."""
        n = int(n)
        index = int(math.floor(n * prob)) if math.isfinite(prob) else -1
        if n < 1 or not (0 <= index < n and 0 <= n - index < n):
            raise ValueError(f"prob = {prob!r} with n = {n} samples reads sorted[{index}] and sorted[{n - index}]: outside [0, {n}) "
                             "(the reference indexes out of bounds there)")
        return n - index, n // 2, index

    @staticmethod
    def _sorted_samples(samples):
        x = np.asarray(samples, dtype=np.float64)
        x = x[:, None] if x.ndim == 1 else x
        if x.ndim != 2 or x.shape[0] < 1:
            raise ValueError(f"samples: n vectors of one length, got an array of shape {x.shape}")
        return x, np.sort(x, axis=0)

    @staticmethod
    def mean_and_intervals(prob: float):
        """Dglm.meanAndIntervals(prob)(samples) (Dglm.scala:263-272): samples [n][k], n draws of a vector -> (mean [k], lower [k], upper [k]),
        the mean as the reference forms it (the samples added in order, times 1 / n), the interval by `interval_ranks`."""
        def summarise(samples):
            x, srt = Dglm._sorted_samples(samples)
            lo, _, up = Dglm.interval_ranks(x.shape[0], prob)
            return reduce(np.add, x) * (1.0 / x.shape[0]), srt[lo], srt[up]
        return summarise

    @staticmethod
    def median_and_intervals(prob: float):
        """Dglm.medianAndIntervals(prob)(samples) (Dglm.scala:274-285): (median [k] = sorted[floor(n / 2)], lower [k], upper [k])."""
        def summarise(samples):
            x, srt = Dglm._sorted_samples(samples)
            lo, med, up = Dglm.interval_ranks(x.shape[0], prob)
            return srt[med], srt[lo], srt[up]
        return summarise

    @staticmethod
    def forecast_particles(mod: "Dglm", cloud, p, ys, eng, *, weights=None, prob: float = 0.75, summary: str = "mean", time0=None,
                           n_particles: Optional[int] = None, slot_offset: int = 0, seed: int = 0, iteration: int = 0,
                           series_offset: int = 0, literal: bool = False, return_draws: bool = False):
        """Dglm.forecastParticles(mod, xt, p, ys) (Dglm.scala:297-331) on the engine (dlm_pf_forecast_particles), summarised as
        Dglm.meanAndIntervals / medianAndIntervals summarise it, on the device: the cloud is pushed through the times of ys, every particle
        draws one observation per time, and per time the mean (or the median) and the interval of `interval_ranks(n, prob)` of those draws
        come back.  cloud [N][d][n] (or [d][n]: one series) with optional weights [N][n] (given: resampled once at entry); cloud=None draws it
        from (m0, C0) -- a prior-predictive simulation, n_particles needed.  ys: the test period, Vector[Data] or (times, y [H] or [N][H]);
        NaN = "forecast, do not update", an observed value updates the cloud and resamples it, as the reference does.  p as in
        ParticleFilter.filter.  time0: the time of the cloud, the first step advances over times[0] - time0; None is the reference's scan, whose
        first step has dt = 0 (the cloud sits AT the first forecast time, Q71).  slot_offset: the Philox slot of the first step (the number of
        steps already filtered).  Returns {"time" [H], "mean" or "median" [N][H], "lower", "upper" [N][H], "state_mean" [N][H][d], "ll" [N],
        "cloud" [N][d][n], "status" [N]} and "draws" [N][H][n] with return_draws."""
        if summary not in ("mean", "median"):
            raise ValueError(f'summary: "mean" or "median", got {summary!r}')
        if cloud is None:
            if weights is not None:
                raise EngineError("weights need the cloud they weigh: pass cloud too")
            if n_particles is None:
                raise EngineError("cloud=None draws the cloud from (m0, C0): say how many particles with n_particles")
            n = int(n_particles)
        else:
            cloud = cloud if hasattr(cloud, "data_ptr") else np.asarray(cloud, dtype=np.float64)
            cloud = cloud[None] if cloud.ndim == 2 else cloud
            if cloud.ndim != 3:
                raise EngineError(f"cloud must be [N][d][n] or [d][n], got the shape {tuple(cloud.shape)}")
            n = int(cloud.shape[2])
            if weights is not None and np.ndim(weights) == 1:
                weights = weights[None]
        times, y = _observations(ys)
        f0 = np.atleast_2d(np.asarray(mod.f(float(times[0])), dtype=np.float64))
        check_pf_shape(f0.shape[0], f0.shape[1], n)
        lo, med, up = Dglm.interval_ranks(n, prob)
        ranks = check_pf_ranks((lo, up) if summary == "mean" else (lo, med, up), n)
        mat = materialise_forecast(mod, times, time0)
        N, y, params = _bank(p, y)
        if cloud is not None and y.shape[0] == 1 and cloud.shape[0] > 1 and isinstance(p, DlmParameters):
            N, y = int(cloud.shape[0]), np.repeat(y, cloud.shape[0], axis=0)
        if cloud is not None and cloud.shape[0] != N:
            raise EngineError(f"{cloud.shape[0]} clouds for {N} series")
        out = _numpy(eng.pf_forecast(mat, params, y, family=mod.family, n_particles=n, ranks=ranks, cloud=cloud, weights=weights,
                                     slot_offset=slot_offset, literal=literal, obs_param=mod.nu, iteration=iteration, seed=seed,
                                     series_offset=series_offset, want_draws=return_draws))
        q = out["fquant"]
        res = {"time": times, "lower": q[:, :, 0], "upper": q[:, :, -1], "state_mean": out["mean"], "ll": out["ll"], "cloud": out["cloud"],
               "status": out["status"]}
        res[summary] = out["fmean"] if summary == "mean" else q[:, :, 1]
        if return_draws:
            res["draws"] = out["draws"]
        return res

    @staticmethod
    def forecast_learned(mod: "Dglm", cloud, var_w, var_v, times, p, eng, *, var_kind: int, shapes=None, weights=None, prob: float = 0.75,
                         summary: str = "mean", time0=None, slot_offset: int = 0, seed: int = 0, iteration: int = 0,
                         series_offset: int = 0, return_draws: bool = False):
        """`forecast_particles` from the cloud of a LEARNING filter, whose particles carry their own variances (dlm_pf_forecast_learned):
        cloud [N][d][n] (or [d][n]: one series), var_w [N][d][n] the rows of the state variances and var_v [N][n] the row of the observation
        scale (None: every particle takes p.v), read by var_kind -- _lib.FC_VAR variances, _lib.FC_LOGVAR log-variances (the filters'
        "psi"), _lib.FC_IG_SCALE the Storvik filter's "scales" with `shapes` [d+1] or [N][d+1] (V's last): every particle then draws its
        variances ONCE and keeps them over the horizon.  weights [N][n]: the tuples are resampled once at entry.  times [H]: the forecast
        times; a pure forecast -- there are no test-period observations in this call: to fold them in, run the filter over them first.  p:
        only its V is read, and only without var_v.  prob, summary, time0, slot_offset as in forecast_particles.  Returns forecast_particles'
        dict without "ll", plus "var_w" [N][d][n] and "var_v" [N][n]: the variances the steps used."""
        if summary not in ("mean", "median"):
            raise ValueError(f'summary: "mean" or "median", got {summary!r}')
        if cloud is None or var_w is None:
            raise EngineError("the forecast from a learning filter needs its cloud and the particles' variance rows var_w")
        as_array = lambda a: a if a is None or hasattr(a, "data_ptr") else np.asarray(a, dtype=np.float64)
        cloud, var_w, var_v, weights = as_array(cloud), as_array(var_w), as_array(var_v), as_array(weights)
        if cloud.ndim == 2:
            cloud, var_w = cloud[None], var_w[None]
            var_v = var_v[None] if var_v is not None and var_v.ndim == 1 else var_v
            weights = weights[None] if weights is not None and weights.ndim == 1 else weights
        if cloud.ndim != 3:
            raise EngineError(f"cloud must be [N][d][n] or [d][n], got the shape {tuple(cloud.shape)}")
        n = int(cloud.shape[2])
        times = np.asarray(times, dtype=np.float64).reshape(-1)
        f0 = np.atleast_2d(np.asarray(mod.f(float(times[0])), dtype=np.float64))
        check_pf_shape(f0.shape[0], f0.shape[1], n)
        check_pf_forecast_learned_lds(f0.shape[0], n)
        lo, med, up = Dglm.interval_ranks(n, prob)
        ranks = check_pf_ranks((lo, up) if summary == "mean" else (lo, med, up), n)
        mat = materialise_forecast(mod, times, time0)
        params = p if isinstance(p, DlmParameters) else BatchedParameters.of(p, int(cloud.shape[0])).packed()
        out = _numpy(eng.pf_forecast_learned(mat, params, cloud, var_w, var_v, family=mod.family, var_kind=var_kind, shapes=shapes,
                                             weights=weights, ranks=ranks, slot_offset=slot_offset, obs_param=mod.nu, iteration=iteration,
                                             seed=seed, series_offset=series_offset, want_draws=return_draws))
        q = out["fquant"]
        res = {"time": times, "lower": q[:, :, 0], "upper": q[:, :, -1], "state_mean": out["mean"], "cloud": out["cloud"],
               "var_w": out["var_w"], "var_v": out["var_v"], "status": out["status"]}
        res[summary] = out["fmean"] if summary == "mean" else q[:, :, 1]
        if return_draws:
            res["draws"] = out["draws"]
        return res

    def simulate_regular(self, params: DlmParameters, n_steps: int, dt: float = 1.0, *, rng=None):
        """Dglm.simulateRegular (Dglm.scala:224-232) on the host: x_0 ~ N(m0, C0) at time 0, then n_steps steps of length dt.  Returns
        (times [n], y [n], x [n][d]).  (F is taken at the observation's time; the reference's `observation` evaluates f(1.0).)"""
        rng = np.random.default_rng() if rng is None else rng
        x = rng.multivariate_normal(params.m0, params.c0)
        times = dt * np.arange(1, n_steps + 1, dtype=np.float64)
        ys, xs = np.empty(n_steps), np.empty((n_steps, x.size))
        g = np.atleast_2d(self.g(dt))
        for k, t in enumerate(times):
            x = g @ x + rng.multivariate_normal(np.zeros(x.size), params.w * dt)
            eta = float(np.atleast_2d(self.f(float(t)))[:, 0] @ x)
            ys[k] = self.observation(eta, float(params.v[0, 0]), rng)
            xs[k] = x
        return times, ys, xs


def materialise_pf(mod, times) -> MaterialisedModel:
    """The model's tables on the observation times with the initial state AT the first of them: dt_0 = 0 (no advance, its G is not read)."""
    times = np.asarray(times, dtype=np.float64).reshape(-1)
    mat = materialise(Dlm(mod.f, mod.g), times)
    if times.size == 1:
        return replace(mat, G=mat.G[:mat.d * mat.d], n_g=1, g_index=None, dt=np.zeros(1))
    dts = np.concatenate([[0.0], np.diff(times)])
    uniq = np.unique(dts[1:])
    table, remap = [], []
    for u in uniq:
        gm = np.ascontiguousarray(np.atleast_2d(mod.g(float(u))).T).reshape(-1)
        for k, have in enumerate(table):
            if np.array_equal(have, gm):
                remap.append(k)
                break
        else:
            remap.append(len(table)); table.append(gm)
    gi = np.concatenate([[0], np.asarray(remap, dtype=np.int32)[np.searchsorted(uniq, dts[1:])]]).astype(np.int32)
    return replace(mat, G=np.concatenate(table), n_g=len(table), g_index=None if len(table) == 1 else gi, dt=dts)


def materialise_forecast(mod, times, time0=None) -> MaterialisedModel:
    """The model's tables on the forecast times with the cloud at time0: dt_0 = times[0] - time0.  time0=None is the reference's scan
    (Dglm.scala:302-311): the cloud sits AT the first forecast time and dt_0 = 0, which is materialise_pf (Q71)."""
    times = np.asarray(times, dtype=np.float64).reshape(-1)
    if time0 is None:
        return materialise_pf(mod, times)
    mat = materialise(Dlm(mod.f, mod.g), times)
    dts = np.diff(np.concatenate([[float(time0)], times]))
    if not np.all(dts >= 0.0):
        raise ValueError("the forecast times must not decrease, and the first must not lie before time0")
    nz = dts != 0.0
    uniq = np.unique(dts[nz]) if nz.any() else np.array([1.0])
    table, remap = [], []
    for u in uniq:
        gm = np.ascontiguousarray(np.atleast_2d(mod.g(float(u))).T).reshape(-1)
        for k, have in enumerate(table):
            if np.array_equal(have, gm):
                remap.append(k)
                break
        else:
            remap.append(len(table)); table.append(gm)
    gi = np.zeros(times.size, dtype=np.int32)          # (a step with dt = 0 does not advance: its G is not read)
    gi[nz] = np.asarray(remap, dtype=np.int32)[np.searchsorted(uniq, dts[nz])]
    return replace(mat, G=np.concatenate(table), n_g=len(table), g_index=None if len(table) == 1 else gi, dt=dts)


@dataclass
class BatchedParameters:
    """DlmParameters of N chains side by side: v [N][1][1], w [N][d][d], m0 [N][d], c0 [N][d][d]."""

    v: np.ndarray
    w: np.ndarray
    m0: np.ndarray
    c0: np.ndarray

    @staticmethod
    def of(p, n: Optional[int] = None) -> "BatchedParameters":
        if isinstance(p, BatchedParameters):
            return p
        plist = [p] * (n or 1) if isinstance(p, DlmParameters) else list(p)
        if n is not None and len(plist) != n:
            raise ValueError(f"need {n} DlmParameters, got {len(plist)}")
        return BatchedParameters(np.stack([q.v for q in plist]), np.stack([q.w for q in plist]), np.stack([q.m0 for q in plist]),
                                 np.stack([q.c0 for q in plist]))

    @property
    def n(self) -> int:
        return int(self.m0.shape[0])

    def copy(self) -> "BatchedParameters":
        return BatchedParameters(self.v.copy(), self.w.copy(), self.m0.copy(), self.c0.copy())

    def where(self, take, other: "BatchedParameters") -> "BatchedParameters":
        """Chain by chain: `other` where take, self elsewhere."""
        t = np.asarray(take, dtype=bool)
        return BatchedParameters(np.where(t[:, None, None], other.v, self.v), np.where(t[:, None, None], other.w, self.w),
                                 np.where(t[:, None], other.m0, self.m0), np.where(t[:, None, None], other.c0, self.c0))

    def packed(self):
        """The tuple Engine.prepare takes: flat column-major arrays and their strides in doubles."""
        N, d = self.m0.shape
        cm = lambda a: np.ascontiguousarray(np.transpose(a, (0, 2, 1))).reshape(-1)
        return (cm(self.v), int(self.v.shape[1] * self.v.shape[2]), cm(self.w), d * d, np.ascontiguousarray(self.m0).reshape(-1), d,
                cm(self.c0), d * d, 0, 0)

    def __getitem__(self, n: int) -> DlmParameters:
        return DlmParameters(self.v[n], self.w[n], self.m0[n], self.c0[n])


def _observations(ys):
    """Vector[Data], a batch of them, or (times [T], y [T] or [N][T]) -> (times, y [N][T])."""
    if isinstance(ys, tuple) and len(ys) == 2 and not hasattr(ys[0], "time"):
        times, y = np.asarray(ys[0], dtype=np.float64), np.asarray(ys[1], dtype=np.float64)
        y = y[None, :] if y.ndim == 1 else y
        if y.ndim == 3 and y.shape[2] != 1:
            raise EngineError(f"the particle filter takes a univariate observation (p = 1), got p = {y.shape[2]}")
        return times, y.reshape(y.shape[0], -1)
    times, y, _ = pack_observations(ys)
    if y.shape[2] != 1:
        raise EngineError(f"the particle filter takes a univariate observation (p = 1), got p = {y.shape[2]}")
    return times, y[:, :, 0]


def _filter_inputs(mod, ys, n, grid=materialise_pf):
    """Model and observations of a filter of n particles -> (times, y [N][T], d, mat), after the check of the shape.  grid: materialise_pf
    (the initial cloud AT the first observation) or materialise (one step before it: particle Gibbs)."""
    times, y = _observations(ys)
    f0 = np.atleast_2d(np.asarray(mod.f(float(times[0])), dtype=np.float64))
    check_pf_shape(f0.shape[0], f0.shape[1], n)
    return times, y, f0.shape[0], grid(Dlm(mod.f, mod.g), times)


def _bank(p, y):
    """(N, y [N][T], what Engine.prepare takes) of one DlmParameters, one per series or a BatchedParameters; ONE series is repeated for
    N parameter sets, else the counts must agree."""
    if isinstance(p, DlmParameters):
        return y.shape[0], y, p
    bp = BatchedParameters.of(p)
    if y.shape[0] == 1 and bp.n > 1:
        y = np.repeat(y, bp.n, axis=0)
    if y.shape[0] != bp.n:
        raise EngineError(f"{bp.n} parameter sets for {y.shape[0]} series")
    return bp.n, y, bp.packed()


def _numpy(out):
    """An engine call's dict with every output as a NumPy array (None stays None)."""
    return {k: None if v is None else np.asarray(v) for k, v in out.items()}


def _lognormal_means(out, d):
    """out with "w_mean" [N][T][d] and "v_mean" [N][T]: the means of the variances from the moments of their logs."""
    with np.errstate(invalid="ignore", over="ignore"):
        moments = np.exp(out["psi_mean"] + out["psi_var"] / 2.0)
    out["w_mean"], out["v_mean"] = moments[:, :, :d], moments[:, :, d]
    return out


def _prior_rows(prior_w, d, first, second, noun):
    """One prior or d of them -> [d][2], the attributes `first` and `second` of each; `noun` names the prior in the message."""
    pws = [prior_w] * d if hasattr(prior_w, first) and hasattr(prior_w, second) else list(prior_w)
    if len(pws) != d:
        raise EngineError(f"prior_w: one {noun} or d = {d} of them, got {len(pws)}")
    return np.array([[getattr(q, first), getattr(q, second)] for q in pws], dtype=np.float64)


def _forecast_from_filter(mod, filt, var_w, var_v, ys_train, times_test, p, eng, *, cloud=None, **kw):
    """What the `forecast` of the three learning filters share: Dglm.forecast_learned from the filter's cloud (or `cloud`) and weights with
    time0 = the last training time and slot_offset = len(ys_train), so that the forecast continues the filter's Philox slots; "filter": the
    filter's own dict."""
    times = _observations(ys_train)[0]
    gmod = mod if isinstance(mod, Dglm) else Dglm.gaussian(mod)
    out = Dglm.forecast_learned(gmod, filt["cloud"] if cloud is None else cloud, var_w, var_v, times_test, p, eng, weights=filt["weights"],
                                time0=float(times[-1]), slot_offset=len(times), **kw)
    out["filter"] = filt
    return out


@dataclass(frozen=True)
class Resampling:
    """The `resample` argument of the reference's ParticleFilter(n, n0, resample) (ParticleFilter.scala:26-30, 140-216), named instead of
    passed as a function: Resampling.multinomial, .stratified, .systematic and .metropolis(b) (dlm_resample_desc, include/dlm_engine.h).
    The first three keep the likelihood estimate unbiased; stratified and systematic resampling lower its variance, and systematic draws
    one uniform per step.  metropolis(b) is the reference's metropolisResampling(b): b Metropolis steps per particle on the weights, BIASED
    for every finite b -- fit for filtering, not for a likelihood a sampler accepts on."""

    scheme: int = _lib.RESAMPLE_MULTINOMIAL
    mh_steps: int = 0

    def __post_init__(self):
        check_pf_resample(self.scheme, self.mh_steps)

    @staticmethod
    def metropolis(b: int) -> "Resampling":
        """ParticleFilter.metropolisResampling(b) (ParticleFilter.scala:159-181), 1 <= b <= _lib.PF_MAX_MH_STEPS."""
        return Resampling(_lib.RESAMPLE_METROPOLIS, b)

    @property
    def unbiased(self) -> bool:
        return self.scheme != _lib.RESAMPLE_METROPOLIS

    @staticmethod
    def of(resample) -> "Resampling":
        """A Resampling as it is; one of _lib.RESAMPLE_* as the scheme without steps."""
        return resample if isinstance(resample, Resampling) else Resampling(resample, 0)


Resampling.multinomial = Resampling(_lib.RESAMPLE_MULTINOMIAL)
Resampling.stratified = Resampling(_lib.RESAMPLE_STRATIFIED)
Resampling.systematic = Resampling(_lib.RESAMPLE_SYSTEMATIC)


class ParticleFilter:
    """ParticleFilter(n, n0, resample) (ParticleFilter.scala:26-71) on the engine: n particles, resampling when ESS < n0 (negative:
    floor(n / 5), what ParticleFilter.likelihood passes) by the scheme `resample`, a `Resampling` (default: multinomial)."""

    def __init__(self, n: int, n0: int = -1, resample: Resampling = Resampling.multinomial):
        check_pf_shape(1, 1, int(n))
        self.n, self.n0, self.resample = int(n), int(n0), Resampling.of(resample)

    def filter(self, mod: Dglm, ys, p, eng, *, seed: int = 0, iteration: int = 0, series_offset: int = 0, literal: bool = False):
        """ys: Vector[Data], a batch of them on one time grid, or (times, y).  p: one DlmParameters, one per series, or a
        BatchedParameters; with ONE series and several parameter sets every set filters that series (a bank of parameters, as the
        particle-marginal sampler needs).  Returns {"ll" [N], "mean" [N][T][d], "ess" [N][T], "cloud" [N][d][n], "weights" [N][n],
        "status" [N]} as NumPy arrays."""
        times, y, d, mat = _filter_inputs(mod, ys, self.n)
        N, y, params = _bank(p, y)
        return _numpy(eng.particle_filter(mat, params, y, family=mod.family, n_particles=self.n, n0=self.n0, literal=literal, obs_param=mod.nu,
                                          iteration=iteration, seed=seed, series_offset=series_offset, resample=self.resample.scheme,
                                          mh_steps=self.resample.mh_steps))

    def forecast(self, mod: Dglm, ys_train, ys_test, p, eng, *, seed: int = 0, iteration: int = 0, series_offset: int = 0,
                 literal: bool = False, **kw):
        """Filter the training period, then forecast the test period from the filter's cloud AND its weights (the end of the reference's
        worked examples: TrafficModel.scala:185-191, Temperature.scala:288, NoModel.scala:203): Dglm.forecast_particles with
        slot_offset = len(ys_train), so that the forecast continues the filter's Philox stream, and time0 = the last training time.
        The training period is filtered with the filter's own resampling scheme; the forecast kernel's resampling (of the weighted entry
        cloud, and after an observed test value) stays multinomial whatever the scheme.
        kw: prob, summary, return_draws.  Returns forecast_particles' dict and "filter": the filter's own."""
        filt = self.filter(mod, ys_train, p, eng, seed=seed, iteration=iteration, series_offset=series_offset, literal=literal)
        times = _observations(ys_train)[0]
        out = Dglm.forecast_particles(mod, filt["cloud"], p, ys_test, eng, weights=filt["weights"], time0=float(times[-1]),
                                      slot_offset=len(times), seed=seed, iteration=iteration, series_offset=series_offset, literal=literal, **kw)
        out["filter"] = filt
        return out

    @staticmethod
    def likelihood(mod: Dglm, ys, n: int, p, eng, *, resample: Resampling = Resampling.multinomial, **kw):
        """ParticleFilter.likelihood(mod, ys, n)(p) (ParticleFilter.scala:78-85): the log-likelihood estimate(s) with n0 = floor(n / 5),
        resampling by `resample` (unbiased under every scheme but Resampling.metropolis)."""
        return ParticleFilter(n, -1, resample).filter(mod, ys, p, eng, **kw)["ll"]


class StorvikFilter:
    """StorvikFilter.filterTs(model, ys, p, priorV, priorW, n, n0) (Storvik.scala:179-189) on the engine (dlm_storvik_batch): a particle
    filter whose particles carry the InverseGamma statistics of their own variances -- the diagonal of W, and V for the Gaussian family --
    and draw them afresh at every step.  One pass gives the filtering distribution, the posterior of the variances at every time and an
    unbiased estimate of the evidence p(y_1:T) (the reference's filter has no likelihood; its other departures are DESIGN.md 2, Q42-Q48)."""

    def __init__(self, n: int, n0: int = -1):
        check_pf_shape(1, 1, int(n))
        self.n, self.n0 = int(n), int(n0)

    def filter(self, mod: Dglm, ys, p: DlmParameters, prior_v, prior_w, eng, *, learn_v: Optional[bool] = None, seed: int = 0,
               iteration: int = 0, series_offset: int = 0, literal: bool = False):
        """ys as ParticleFilter.filter takes them; p: m0 and C0 of the initial cloud (and V when it is not learned; p.w is not read);
        prior_v an InverseGamma (None when V is not learned), prior_w one InverseGamma for every component or d of them.  learn_v
        defaults to "the family is Gaussian"; a family other than the Gaussian learns W alone.  Returns what ParticleFilter.filter
        returns plus "scale_mean" [N][T][d+1] (the weighted means of the statistics' scales, V's last), "scales" [N][d+1][n], the shapes
        "shape_w" [N][T][d] and "shape_v" [N][T] of the posteriors after step t (prior + 0.5 per advance / per observation: the time grid
        and the missing pattern fix them, the kernel does not write them), and the Rao-Blackwellised posterior means "w_mean" [N][T][d] =
        scale_mean / (shape - 1) and "v_mean" [N][T], NaN where the shape is <= 1 (and v_mean where V is not learned)."""
        times, y, d, mat = _filter_inputs(mod, ys, self.n)
        learn_v = mod.family == _lib.OBS_GAUSSIAN if learn_v is None else bool(learn_v)
        pw = _prior_rows(prior_w, d, "shape", "scale", "InverseGamma")
        pv = np.array([prior_v.shape, prior_v.scale], dtype=np.float64) if learn_v else None
        out = _numpy(eng.storvik_filter(mat, p, y, pw, family=mod.family, n_particles=self.n, prior_v=pv, learn_v=learn_v, n0=self.n0,
                                        literal=literal, obs_param=mod.nu, iteration=iteration, seed=seed, series_offset=series_offset))
        N, T = y.shape
        advances = np.cumsum(mat.dt != 0.0) if mat.dt is not None else np.arange(1, T + 1)
        out["shape_w"] = np.broadcast_to((pw[None, :, 0] + 0.5 * advances[:, None].astype(np.float64))[None], (N, T, d)).copy()
        out["shape_v"] = pv[0] + 0.5 * np.cumsum(~np.isnan(y), axis=1).astype(np.float64) if learn_v else np.full((N, T), np.nan)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["w_mean"] = np.where(out["shape_w"] > 1.0, out["scale_mean"][:, :, :d] / (out["shape_w"] - 1.0), np.nan)
            out["v_mean"] = np.where(out["shape_v"] > 1.0, out["scale_mean"][:, :, d] / (out["shape_v"] - 1.0), np.nan)
        return out

    def forecast(self, mod: Dglm, ys_train, times_test, p: DlmParameters, prior_v, prior_w, eng, *, learn_v: Optional[bool] = None,
                 seed: int = 0, iteration: int = 0, series_offset: int = 0, literal: bool = False, **kw):
        """Filter the training period, then forecast the times times_test [H] from the filter's cloud, its weights and every particle's OWN
        InverseGamma posterior -- "scales" with the final shapes shape_w[:, -1] and shape_v[:, -1] --, so that the band carries the
        uncertainty of the variances (Dglm.forecast_learned with _lib.FC_IG_SCALE, time0 = the last training time and slot_offset =
        len(ys_train)).  To fold in test-period observations, filter them too.  kw: prob, summary, return_draws.  Returns
        forecast_learned's dict and "filter": the filter's own."""
        filt = self.filter(mod, ys_train, p, prior_v, prior_w, eng, learn_v=learn_v, seed=seed, iteration=iteration,
                           series_offset=series_offset, literal=literal)
        d = filt["cloud"].shape[1]
        learned = mod.family == _lib.OBS_GAUSSIAN if learn_v is None else bool(learn_v)          # (else V is p.v, and its shape is not read)
        shapes = np.concatenate([filt["shape_w"][:, -1], (filt["shape_v"][:, -1] if learned else np.ones(len(filt["ll"])))[:, None]], axis=1)
        return _forecast_from_filter(mod, filt, filt["scales"][:, :d], filt["scales"][:, d] if learned else None, ys_train, times_test, p, eng,
                                     var_kind=_lib.FC_IG_SCALE, shapes=shapes, seed=seed, iteration=iteration, series_offset=series_offset, **kw)


class LiuAndWestFilter:
    """LiuAndWestFilter(n, prior, a, n0) (LiuAndWest.scala:26-82; Liu & West 2001) on the engine (dlm_lw_batch): an auxiliary particle
    filter whose particles carry their own log-variances -- the diagonal of W, and V for the Gaussian, Student-t and Beta families --
    shrunk towards their weighted mean by `a` and jittered with the kernel variance (1 - a^2) s^2 at every step.  It needs no conjugacy;
    for a < 1 it is an approximation.  The priors are independent `stochvol.Gaussian`s on the LOG-variances (the reference draws the
    variances from a Rand[DlmParameters] and takes logs); the reference's other departures are DESIGN.md 2, Q49-Q56."""

    def __init__(self, n: int, a: float, n0: int = -1):
        check_pf_shape(1, 1, int(n))
        check_shrinkage(a, ValueError)
        self.n, self.a, self.n0 = int(n), float(a), int(n0)

    def filter(self, mod: Dglm, ys, p: DlmParameters, prior_v, prior_w, eng, *, learn_v: Optional[bool] = None, seed: int = 0,
               iteration: int = 0, series_offset: int = 0, literal: bool = False):
        """ys as ParticleFilter.filter takes them; p: m0 and C0 of the initial cloud (and V when it is not learned; p.w is not read);
        prior_v a Gaussian(mean, sd) on log V (None when V is not learned), prior_w one Gaussian on log W_kk for every component or d of
        them; sd = 0 is a known variance.  learn_v defaults to "the family is Gaussian, Student-t or Beta".  Returns what
        ParticleFilter.filter returns plus the raw "psi_mean" and "psi_var" [N][T][d+1] (mean and variance of the log-variances under the
        weights of step t, V's last), "psi" [N][d+1][n], and the posterior means of the variances from the log-normal moments,
        "w_mean" [N][T][d] = exp(psi_mean + psi_var / 2) and "v_mean" [N][T] (NaN where V is not learned)."""
        times, y, d, mat = _filter_inputs(mod, ys, self.n)
        learn_v = mod.family in (_lib.OBS_GAUSSIAN, _lib.OBS_STUDENTT, _lib.OBS_BETA) if learn_v is None else bool(learn_v)
        pw = _prior_rows(prior_w, d, "mean", "sd", "Gaussian")
        pv = np.array([prior_v.mean, prior_v.sd], dtype=np.float64) if learn_v else None
        out = eng.lw_filter(mat, p, y, pw, family=mod.family, n_particles=self.n, a=self.a, prior_v=pv, learn_v=learn_v, n0=self.n0,
                            literal=literal, obs_param=mod.nu, iteration=iteration, seed=seed, series_offset=series_offset)
        return _lognormal_means(_numpy(out), d)

    def forecast(self, mod: Dglm, ys_train, times_test, p: DlmParameters, prior_v, prior_w, eng, *, learn_v: Optional[bool] = None,
                 seed: int = 0, iteration: int = 0, series_offset: int = 0, literal: bool = False, **kw):
        """Filter the training period, then forecast the times times_test [H] from the filter's cloud, its weights and every particle's OWN
        log-variances "psi" (Dglm.forecast_learned with _lib.FC_LOGVAR, time0 = the last training time and slot_offset = len(ys_train)):
        the band carries the uncertainty of the variances.  To fold in test-period observations, filter them too.  kw: prob, summary,
        return_draws.  Returns forecast_learned's dict and "filter": the filter's own."""
        filt = self.filter(mod, ys_train, p, prior_v, prior_w, eng, learn_v=learn_v, seed=seed, iteration=iteration,
                           series_offset=series_offset, literal=literal)
        d = filt["cloud"].shape[1]
        learned = mod.family in (_lib.OBS_GAUSSIAN, _lib.OBS_STUDENTT, _lib.OBS_BETA) if learn_v is None else bool(learn_v)   # (else V is p.v)
        return _forecast_from_filter(mod, filt, filt["psi"][:, :d], filt["psi"][:, d] if learned else None, ys_train, times_test, p, eng,
                                     var_kind=_lib.FC_LOGVAR, seed=seed, iteration=iteration, series_offset=series_offset, **kw)


class AuxFilter:
    """AuxFilter(n) (AuxFilter.scala:12-66; Pitt & Shephard 1999) on the engine: the auxiliary particle filter for KNOWN parameters, which
    is dlm_lw_batch with a = 1, prior standard deviations of 0 and means log diag(W); V is p.v.  Unlike the reference's, its second stage
    divides by the first-stage density, resamples only when ESS < n0 and carries its weights otherwise, and its likelihood counts both
    stages: exp(ll) is unbiased for p(y_1:T), so `likelihood` can stand in for ParticleFilter.likelihood."""

    def __init__(self, n: int, n0: int = -1):
        check_pf_shape(1, 1, int(n))
        self.n, self.n0 = int(n), int(n0)

    def filter(self, mod: Dglm, ys, p: DlmParameters, eng, *, seed: int = 0, iteration: int = 0, series_offset: int = 0,
               literal: bool = False):
        """ys as ParticleFilter.filter takes them; p: one DlmParameters with a DIAGONAL W (ValueError otherwise).  Returns what
        LiuAndWestFilter.filter returns."""
        return LiuAndWestFilter(self.n, 1.0, self.n0).filter(mod, ys, p, None, self._known(p), eng, learn_v=False, seed=seed, iteration=iteration,
                                                             series_offset=series_offset, literal=literal)

    def _known(self, p: DlmParameters):
        """p.w as the Liu-West filter's known log-variances: Gaussian(log W_kk, 0) per component."""
        w = np.atleast_2d(np.asarray(p.w, dtype=np.float64))
        if np.any(w != np.diag(np.diag(w))):
            raise ValueError("AuxFilter takes a diagonal W: the kernel's state noise is independent by component")
        from .stochvol import Gaussian
        return [Gaussian(float(np.log(v)), 0.0) for v in np.diag(w)]

    def forecast(self, mod: Dglm, ys_train, times_test, p: DlmParameters, eng, *, seed: int = 0, iteration: int = 0, series_offset: int = 0,
                 literal: bool = False, **kw):
        """Filter the training period, then forecast times_test [H] from the filter's cloud and weights: LiuAndWestFilter.forecast with the
        known variances of p.  kw: prob, summary, return_draws."""
        return LiuAndWestFilter(self.n, 1.0, self.n0).forecast(mod, ys_train, times_test, p, None, self._known(p), eng, learn_v=False, seed=seed,
                                                               iteration=iteration, series_offset=series_offset, literal=literal, **kw)

    def likelihood(self, mod: Dglm, ys, p: DlmParameters, eng, **kw):
        """AuxFilter.likelihood(mod, ys, n)(p) (AuxFilter.scala:69-75): the log-likelihood estimate of every series."""
        return self.filter(mod, ys, p, eng, **kw)["ll"]


class RaoBlackwellFilter:
    """RaoBlackwellFilter(n, prior, a, n0) (RaoBlackwellFilter.scala) on the engine (dlm_rb_batch): the Liu-West filter for a GAUSSIAN DLM
    whose particles carry, in place of a drawn state, the Kalman mean and covariance of the state given their own log-variances.  The state
    is integrated out exactly; only the d + 1 variances are left to the particles, and with every variance known (sd = 0) the filter is the
    Kalman filter.  The priors are independent `stochvol.Gaussian`s on the LOG-variances as in LiuAndWestFilter; the reference's departures
    are DESIGN.md 2, Q57-Q62.  Every particle's covariance lives in LDS, so the particle count shrinks with d (engine.check_rb_lds)."""

    def __init__(self, n: int, a: float, n0: int = -1):
        check_pf_shape(1, 1, int(n))
        check_shrinkage(a, ValueError)
        self.n, self.a, self.n0 = int(n), float(a), int(n0)

    def filter(self, mod, ys, p: DlmParameters, prior_v, prior_w, eng, *, learn_v: bool = True, seed: int = 0, iteration: int = 0,
               series_offset: int = 0, literal: bool = False):
        """mod: a Dlm or a Gaussian Dglm (any other family: EngineError).  ys, p, prior_v, prior_w as LiuAndWestFilter.filter takes them;
        learn_v defaults to True.  Returns the engine's outputs as NumPy arrays -- "ll" [N], "mean" [N][T][d], "cov" [N][T][d][d], "ess"
        [N][T], "psi_mean", "psi_var" [N][T][d+1], "means" [N][d][n], "covs" [N][d(d+1)/2][n], "weights" [N][n], "psi" [N][d+1][n],
        "status" [N] -- plus the posterior means of the variances from the log-normal moments, "w_mean" [N][T][d] =
        exp(psi_mean + psi_var / 2) and "v_mean" [N][T] (NaN where V is not learned)."""
        family = getattr(mod, "family", _lib.OBS_GAUSSIAN)
        if family != _lib.OBS_GAUSSIAN:
            raise EngineError(f"the Rao-Blackwellised filter takes a Gaussian DLM (the Kalman step integrates the state out), got family {family!r}")
        times, y, d, mat = _filter_inputs(mod, ys, self.n)
        check_rb_lds(d, self.n)
        learn_v = bool(learn_v)
        pw = _prior_rows(prior_w, d, "mean", "sd", "Gaussian")
        pv = np.array([prior_v.mean, prior_v.sd], dtype=np.float64) if learn_v else None
        out = eng.rb_filter(mat, p, y, pw, n_particles=self.n, a=self.a, prior_v=pv, learn_v=learn_v, n0=self.n0, literal=literal,
                            iteration=iteration, seed=seed, series_offset=series_offset)
        return _lognormal_means(_numpy(out), d)

    def forecast(self, mod, ys_train, times_test, p: DlmParameters, prior_v, prior_w, eng, *, learn_v: bool = True, seed: int = 0,
                 iteration: int = 0, series_offset: int = 0, literal: bool = False, **kw):
        """Filter the training period, draw a state per particle from its Kalman moments (Engine.rb_state_draw: x_i = m_i + chol(C_i) z_i,
        at the Philox slot len(ys_train)), then forecast times_test [H] from that cloud, the filter's weights and every particle's OWN
        log-variances "psi" (Dglm.forecast_learned with _lib.FC_LOGVAR, time0 = the last training time, slot_offset = len(ys_train)).  To
        fold in test-period observations, filter them too.  kw: prob, summary, return_draws.  Returns forecast_learned's dict, "filter":
        the filter's own, and "cloud0" [N][d][n]: the drawn states."""
        filt = self.filter(mod, ys_train, p, prior_v, prior_w, eng, learn_v=learn_v, seed=seed, iteration=iteration,
                           series_offset=series_offset, literal=literal)
        d, T = filt["means"].shape[1], len(_observations(ys_train)[0])
        drawn = _numpy(eng.rb_state_draw(filt["means"], filt["covs"], slot=T, iteration=iteration, seed=seed, series_offset=series_offset))
        out = _forecast_from_filter(mod, filt, filt["psi"][:, :d], filt["psi"][:, d] if learn_v else None, ys_train, times_test, p, eng,
                                    cloud=drawn["cloud"], var_kind=_lib.FC_LOGVAR, seed=seed, iteration=iteration,
                                    series_offset=series_offset, **kw)
        out["cloud0"] = drawn["cloud"]
        return out


INIT_ITERATION = 0xFFFFFFFF   # the Philox iteration of Metropolis.dglm's evaluation of the initial parameters


@dataclass
class MetropolisState:
    """Metropolis.State(parameters, ll, accepted) (MetropolisHastings.scala) for N chains: ll is log-likelihood estimate + log prior."""

    parameters: BatchedParameters
    ll: np.ndarray
    accepted: np.ndarray


class Metropolis:
    @staticmethod
    def symmetric_proposal(delta: float):
        """Metropolis.symmetricProposal (MetropolisHastings.scala:57-74): the diagonals of v, w and c0 move on the log scale, diag * exp(sqrt(delta) z),
        and come back as DIAGONAL matrices; m0 moves additively, m0 + delta z.  Returns proposal(parameters, rng) -> parameters; the normals
        are drawn in the order v, w, m0, c0, each [N][k] in one call."""
        if not delta > 0:
            raise ValueError(f"delta must be positive, got {delta}")
        sd = float(np.sqrt(delta))

        def diagonal(m, rng):
            dg = np.diagonal(m, axis1=1, axis2=2)
            new = dg * np.exp(sd * rng.standard_normal(dg.shape))
            out = np.zeros_like(m)
            idx = np.arange(m.shape[1])
            out[:, idx, idx] = new
            return out

        def proposal(p: BatchedParameters, rng: np.random.Generator) -> BatchedParameters:
            v = diagonal(p.v, rng)
            w = diagonal(p.w, rng)
            m0 = p.m0 + delta * rng.standard_normal(p.m0.shape)
            c0 = diagonal(p.c0, rng)
            return BatchedParameters(v, w, m0, c0)
        return proposal

    @staticmethod
    def dglm(mod: Dglm, ys, proposal, prior, init_p, n: int, eng, n_iter: int, seed: int = 0, *, n_chains: Optional[int] = None,
             literal: bool = False, evaluate_init: bool = False, resample: Resampling = Resampling.multinomial):
        """Metropolis.dglm (MetropolisHastings.scala:142-154): particle-marginal Metropolis, one chain per series.  ys: one series (every
        chain targets its posterior) or one per chain.  proposal(parameters, rng) -> parameters (symmetric: no Hastings term, as mStep);
        prior(parameters) -> [N] log densities; init_p one DlmParameters (with n_chains), a sequence of them or a BatchedParameters.
        Iteration k proposes, calls the particle filter ONCE for all chains (n particles, n0 = floor(n / 5), Philox iteration k and seed
        `seed`), draws N uniforms and accepts where log u < (ll' + prior') - ll.  The host draws come from np.random.default_rng(seed), the
        proposal's first.  Like the reference the chains start at ll = -1e99: the first proposal is accepted.  evaluate_init=True
        starts them at the particle filter's estimate for init_p instead (Philox iteration INIT_ITERATION): chains that start in the
        posterior then stay in it from the first iteration on.  resample: the filter's resampling scheme, one of the three UNBIASED ones
        (stratified and systematic lower the variance of the estimate, which is what governs the mixing); Resampling.metropolis(b) is
        refused with an EngineError: its estimate is biased, and the chain would target another posterior.  Yields a MetropolisState per
        iteration."""
        resample = Resampling.of(resample)
        if not resample.unbiased:
            raise EngineError(f"Metropolis.dglm needs an unbiased likelihood estimate: Metropolis resampling with {resample.mh_steps} steps is "
                              "biased for every finite number of steps, and particle-marginal Metropolis on a biased estimate targets the "
                              "wrong posterior; use Resampling.multinomial, .stratified or .systematic")

        def chain():          # (the refusal above is raised by the call, not by the first next())
            state = BatchedParameters.of(init_p, n_chains).copy()
            N = state.n
            rng = np.random.default_rng(seed)
            ll = np.full(N, -1e99)
            accepted = np.zeros(N, dtype=np.int64)
            pf = ParticleFilter(n, -1, resample)
            if evaluate_init:
                ll = pf.filter(mod, ys, state, eng, seed=seed, iteration=INIT_ITERATION, literal=literal)["ll"] + np.asarray(prior(state), dtype=np.float64)
            for k in range(n_iter):
                prop = proposal(state, rng)
                prop_ll = pf.filter(mod, ys, prop, eng, seed=seed, iteration=k, literal=literal)["ll"] + np.asarray(prior(prop), dtype=np.float64)
                with np.errstate(invalid="ignore"):
                    take = np.log(rng.uniform(size=N)) < prop_ll - ll
                state = state.where(take, prop)
                ll = np.where(take, prop_ll, ll)
                accepted = accepted + take
                yield MetropolisState(state.copy(), ll.copy(), accepted.copy())
        return chain()


@dataclass
class ParticleGibbsState:
    """One iteration of ParticleGibbs.sample: the state paths [N][T+1][d], the observation variances [N] and the diagonals of W [N][d]
    behind them (device tensors), the conditional filter's log-likelihood figure of the sweep [N] and the worst status of the sweep."""

    path: object
    v: object
    w: object
    ll: object
    status: int
    m0: np.ndarray          # [N][d] and [N][d][d]: the initial parameters', which the sampler does not move
    c0: np.ndarray

    @property
    def params(self) -> BatchedParameters:
        """The chains' parameters as NumPy arrays (a copy off the device)."""
        v = self.v.detach().cpu().numpy().reshape(-1, 1, 1)
        w = self.w.detach().cpu().numpy()
        N, d = w.shape
        W = np.zeros((N, d, d)); idx = np.arange(d); W[:, idx, idx] = w
        return BatchedParameters(v, W, self.m0.copy(), self.c0.copy())


class ParticleGibbs:
    """Particle Gibbs for a DGLM on the engine (dlm_pg_batch): what ParticleGibbs.scala and the commented-out ParticleGibbsAncestor.scala aim
    at, built as the textbook algorithm (Andrieu, Doucet & Holenstein 2010; ancestor sampling: Lindsten, Jordan & Schoen 2014) -- the
    reference's own step is not a valid kernel.  n particles, the conditioned path among them; one sweep leaves the
    law of the state path given y and the parameters invariant for any n >= 2.

    The time grid is the FFBS one (`materialise`, as gibbs_dinvgamma_device): the path has T + 1 records, record 0 the state one step
    before the first observation, y_t belongs to record t + 1, and every one of the T transitions has dt_t != 0 -- which is what makes
    dlm_dinvgamma_step_batch's InverseGamma(shape + T / 2, .) the exact conditional of W_ii.  (The particle FILTERS put the initial cloud AT
    the first observation, `materialise_pf`; a path on that grid has one transition less than records.)"""

    def __init__(self, n: int, ancestor_sampling: bool = True):
        check_pf_shape(1, 1, int(n))
        self.n, self.ancestor_sampling = int(n), bool(ancestor_sampling)

    def initial_path(self, mod: Dglm, ys, p, eng, *, seed: int = 0, series_offset: int = 0):
        """A path to start from, [N][T+1][d]: the FILTERING MEANS of one bootstrap-filter run with n particles (record t + 1 = the mean
        after y_t; record 0 = m0).  It is not a draw of the smoothing law -- no start has to be: the sweeps forget it geometrically fast,
        and with ancestor sampling within a few iterations."""
        times, y, d, mat = _filter_inputs(mod, ys, self.n, materialise)
        N, y, params = _bank(p, y)
        out = eng.particle_filter(mat, params, y, family=mod.family, n_particles=self.n, obs_param=mod.nu, iteration=INIT_ITERATION, seed=seed,
                                  series_offset=series_offset, want_ess=False, want_cloud=False, want_weights=False)
        if np.any(np.asarray(out["status"]) != 0):
            raise EngineError("the bootstrap filter of the initial path failed for some series (status != 0)")
        m0 = np.asarray(p.m0 if isinstance(p, DlmParameters) else BatchedParameters.of(p).m0, dtype=np.float64)
        first = np.broadcast_to(m0.reshape(-1, mat.d), (N, mat.d))[:, None, :]
        return np.concatenate([first, np.asarray(out["mean"])], axis=1)

    def sample_state(self, mod: Dglm, ys, p, ref, eng, *, seed: int = 0, iteration: int = 0, series_offset: int = 0, **want):
        """One sweep: a new path [N][T+1][d] given the path `ref`, the data and the parameters.  Returns Engine.pg_sweep's dict as NumPy
        arrays ("ll", "path", "stats", "status" and the traces asked for through want_path_index / want_trace / want_step_weights)."""
        times, y, d, mat = _filter_inputs(mod, ys, self.n, materialise)
        N, y, params = _bank(p, y)
        return _numpy(eng.pg_sweep(mat, params, y, np.asarray(ref, dtype=np.float64), family=mod.family, n_particles=self.n,
                                   ancestor_sampling=self.ancestor_sampling, obs_param=mod.nu, iteration=iteration, seed=seed,
                                   series_offset=series_offset, **want))

    def sample(self, mod: Dglm, ys, prior_w, init_p, eng, n_iter: int, prior_v=None, seed: int = 0, *, init_path=None,
               series_offset: int = 0):
        """The Gibbs sampler, a generator of ParticleGibbsState: iteration k is ONE dlm_pg_batch (the path given the parameters; Philox
        iteration k under `seed`) and ONE dlm_dinvgamma_step_batch on its statistics (the diagonal of W given the path, and for the
        Gaussian family V given the path and y), everything device-resident.  prior_w, prior_v: InverseGamma (shape, scale) pairs or objects
        with .shape / .scale; prior_v applies to the Gaussian family only (any other family keeps init_p's V, and giving one is an error).
        init_p: one DlmParameters for every chain, one per series or a BatchedParameters (its W is read on the diagonal; m0 and C0 stay).
        init_path [N][T+1][d]: the first reference path (default: `initial_path`)."""
        import torch
        if prior_v is not None and mod.family != _lib.OBS_GAUSSIAN:
            raise EngineError("prior_v applies to the Gaussian family only: no other family's V has a conjugate draw")
        times, y, d, mat = _filter_inputs(mod, ys, self.n, materialise)
        bp = BatchedParameters.of(init_p, y.shape[0] if isinstance(init_p, DlmParameters) else None)
        N, y, _ = _bank(bp, y)
        T = mat.T
        path0 = self.initial_path(mod, (times, y), bp, eng, seed=seed, series_offset=series_offset) if init_path is None else init_path
        dev = torch.device("cuda", eng.device)
        put = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
        yd, path = put(y), put(path0)
        if tuple(path.shape) != (N, T + 1, d):
            raise EngineError(f"init_path must be [N][T+1][d] = {(N, T + 1, d)}, got {tuple(path.shape)}")
        idx = np.arange(d)
        V, Wd = put(bp.v.reshape(N, 1)), put(bp.w[:, idx, idx])
        m0, C0 = put(bp.m0.reshape(-1)), put(np.transpose(bp.c0, (0, 2, 1)).reshape(-1))
        learn_v = prior_v is not None
        for it in range(n_iter):
            W = torch.diag_embed(Wd).reshape(N, d * d).contiguous()
            packed = (V.reshape(-1), 1, W.reshape(-1), d * d, m0, d, C0, d * d)
            out = eng.pg_sweep(mat, packed, yd, path, family=mod.family, n_particles=self.n, ancestor_sampling=self.ancestor_sampling,
                               obs_param=mod.nu, iteration=it, seed=seed, series_offset=series_offset)
            Vn, Wn = eng.dinvgamma_step(d, 1, out["stats"], prior_v if learn_v else (1.0, 1.0), prior_w, iteration=it, seed=seed,
                                        series_offset=series_offset)
            bad = out["status"] != 0
            worst = int(out["status"].max().item())
            path = torch.where(bad[:, None, None], path, out["path"]) if worst else out["path"]          # a failed series keeps its path and its parameters
            if learn_v:
                V = torch.where(bad[:, None], V, Vn.reshape(N, 1))
            Wd = torch.where(bad[:, None], Wd, Wn.reshape(N, d, d)[:, idx, idx])
            yield ParticleGibbsState(path, V.reshape(-1), Wd, out["ll"], worst, bp.m0, bp.c0)
