"""Gibbs sampler of the DLM with Student-t observations on the device (StudentT.sample / step, StudentTGibbs.scala:182-232).

The observation noise is the scale mixture y_t ~ N(F_t^T theta_t, v_t), v_t ~ InverseGamma(nu / 2, nu s / 2), so that
y_t | theta_t ~ ScaledStudentsT(nu, F_t^T theta_t, sqrt(s)).  Every series runs its own chain -- the reference's semantics for
one series, N at once -- and one iteration is two engine calls:

  dlm_ffbs_batch           theta | v, W     the per-series V_t stream v and per-series W, through the 10-field parameter tuple
  dlm_studentt_step_batch  W | theta;  nu | (theta, s) by Metropolis-Hastings;  v | (theta, nu, s);  s | (v, nu)

y, theta, the V stream, s, nu and W stay on the device across iterations whatever the input type; per iteration only the
[N]-sized summaries (s, nu, accepted, log-likelihood, status) cross to the host, plus theta or v when asked for.

The default is the corrected sampler.  literal=True runs the reference's arithmetic: the kernel's
DLM_OPT_STUDENTT_LITERAL (Q11-Q15) and, here, every step from the INITIAL s and W (Q10: `step` closes over the initial params).
Neither mode starts a chain at nu = 0, which Poisson(3).draw can give and which turns the reference's chain into NaN.

The prior of nu and its proposal are the example's (examples/.../StudentT.scala:59-80): `Poisson(rate)` and
`NegativeBinomialProposal(size)`, nu' = NegativeBinomial(size, nu / (size + nu)) + 1.  These are the only families the
device evaluates; the reference's arbitrary closures are not offered.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Iterator, Optional

import numpy as np

from . import _lib
from ._chain import host, or_status, place
from .dlm import Dlm, DlmParameters, materialise
from .gibbs import InverseGamma


@dataclass(frozen=True)
class Poisson:
    """The prior of nu: Poisson(rate) (breeze.stats.distributions.Poisson)."""
    rate: float

    def log_pmf(self, k):
        k = np.asarray(k, dtype=np.float64)
        return k * math.log(self.rate) - self.rate - np.vectorize(math.lgamma)(k + 1.0)

    def draw(self, rng: np.random.Generator, size=None):
        return rng.poisson(self.rate, size=size)


@dataclass(frozen=True)
class NegativeBinomialProposal:
    """The proposal of nu: to = NegativeBinomial(size, from / (size + from)).draw + 1, where Breeze's NegativeBinomial(r, q)
    draws Poisson(Gamma(r, q / (1 - q))).  Its density in the corrected sampler is that of the draw (the pmf at to - 1);
    the literal mode evaluates the pmf at `to`, as the example's propNuP does (Q12)."""
    size: float


def initial_nu(prior_nu: Poisson, n_series: int, *, seed: int = 0, series_offset: int = 0) -> np.ndarray:
    """nu_0 per series drawn from the prior on the host by a generator keyed by (seed, global series index) -- a sharded run
    starts where the single-GPU run does -- and redrawn while it is 0 (a chain at nu = 0 is NaN from its first step)."""
    out = np.empty(n_series, dtype=np.int32)
    for k in range(n_series):
        rng = np.random.default_rng([int(seed), int(series_offset) + k, 0x4E55])
        v = 0
        while v == 0:
            v = int(prior_nu.draw(rng))
        out[k] = v
    return out


class StudentT:
    @dataclass
    class Params:
        """The chain's parameters after an iteration: scale [N] (s = the observation variance scale, host) and W [N][d*d]
        (dense diagonal, column-major; stays where the chain runs -- `w_diag()` copies the diagonals to the host)."""
        scale: np.ndarray
        W: object
        d: int

        def w_diag(self) -> np.ndarray:
            w = host(self.W).reshape(-1, self.d, self.d)
            return np.diagonal(w, axis1=1, axis2=2).copy()

    @dataclass
    class State:
        """StudentT.State (StudentTGibbs.scala:21-25), batched.  variances [N][T] and theta [N][T+1][d] are host copies when
        asked for (keep_variances / keep_theta), else None; nu and accepted [N] int32; loglik [N]: the Student-t
        log-likelihood of the state draw at the chain's nu (Q14 as the mode says); status [N]: the FFBS call's flags or'ed
        with the step's."""
        p: "StudentT.Params"
        variances: Optional[np.ndarray]
        nu: np.ndarray
        theta: Optional[np.ndarray]
        accepted: np.ndarray
        loglik: Optional[np.ndarray] = None
        status: Optional[np.ndarray] = None

    @staticmethod
    def sample(ys, prior_w: InverseGamma, prior_nu: Poisson, prop_nu: NegativeBinomialProposal, mod: Dlm, params: DlmParameters,
               engine, *, n_iter: int, seed: int = 0, nu0=None, literal: bool = False, series_offset: int = 0,
               keep_theta: bool = False, keep_variances: bool = False, simulation_smoother: bool = False, times=None,
               ffbs: Optional[Callable] = None, step: Optional[Callable] = None) -> Iterator["StudentT.State"]:
        """StudentT.sample (StudentTGibbs.scala:215-232) for N independent series: ys [N][T] or [N][T][1] (NaN = missing;
        numpy or a torch device tensor), params the initial DlmParameters shared by the series (v = [[s]]).  Yields one State
        per iteration.  The chain starts from v = 1 everywhere and nu0 (None: drawn from the prior, see initial_nu; an int or
        an [N] array otherwise).  simulation_smoother=True draws theta with the Durbin-Koopman simulation smoother
        (DLM_OPT_FFBS_SIMSMOOTH, as GibbsSampling.sample offers it): it takes a V_t stream only at d <= 15.
        ffbs= / step= replace engine.ffbs / engine.studentt_step (same signatures), for tests."""
        if not isinstance(prior_nu, Poisson) or not isinstance(prop_nu, NegativeBinomialProposal):
            raise TypeError("the device evaluates a Poisson prior of nu and a NegativeBinomialProposal only")
        times = np.arange(1, int(ys.shape[1]) + 1, dtype=np.float64) if times is None else times
        mat = materialise(mod, times)
        d, T, N = mat.d, mat.T, int(ys.shape[0])
        if mat.p != 1:
            raise ValueError("StudentT.sample is univariate (the reference reads y(0) and v(0,0)): p must be 1")
        if simulation_smoother and d > 15:
            raise ValueError(f"simulation_smoother=True takes the V_t stream of the Student-t sampler only at d <= 15 (d = {d}); "
                             "use the default reference-form sampler")
        if literal and mat.f_stride:
            raise ValueError("literal=True needs a time-invariant F (SURVEY Q11 pairs y_t with F at t0 - 1)")
        run_ffbs = ffbs if ffbs is not None else engine.ffbs
        run_step = step if step is not None else engine.studentt_step

        # where the chain lives: a torch device (an engine, or a device tensor given), else host arrays (injected callables)
        put, y = place(ys, engine, N, T)

        if nu0 is None:
            nu_h = initial_nu(prior_nu, N, seed=seed, series_offset=series_offset)
        else:
            nu_h = np.broadcast_to(np.asarray(nu0, dtype=np.int32), (N,)).copy()
            if (nu_h < 1).any():
                raise ValueError("nu0 must be >= 1")
        s0 = float(np.asarray(params.v, dtype=np.float64).reshape(-1)[0])
        w0 = np.ascontiguousarray(np.asarray(params.w, dtype=np.float64).T).reshape(-1)
        S0 = put(np.full(N, s0)); W0 = put(np.tile(w0, (N, 1)))
        m0 = put(np.asarray(params.m0, dtype=np.float64).reshape(-1))
        C0 = put(np.ascontiguousarray(np.asarray(params.c0, dtype=np.float64).T).reshape(-1))
        nu = put(nu_h, np.int32)
        acc = put(np.zeros(N, dtype=np.int32), np.int32)
        vs = put(np.ones((N, T)))                    # iteration 0: v = 1 everywhere (StudentTGibbs.scala:224)
        s, W = S0, W0
        prior = (prior_nu.rate, prop_nu.size, prior_w.shape, prior_w.scale)
        flags = _lib.OPT_FFBS_SIMSMOOTH if simulation_smoother else 0
        for it in range(n_iter):
            s_in, W_in = (S0, W0) if literal else (s, W)     # Q10: the reference's step closes over the initial params
            packed = (vs.reshape(-1), T, W_in.reshape(-1), d * d, m0, 0, C0, 0, 1, 0)
            out = run_ffbs(mat, packed, y, seed=seed * 1000003 + it, series_offset=series_offset, flags=flags,
                           want_theta=True, want_stats=True, want_filt=False)
            theta, stats, fstatus = out["theta"], out["stats"], out.get("status")
            del out
            res = run_step(mat, y, theta, stats, prior, s_in, nu, iteration=it, accepted=acc, seed=seed,
                           series_offset=series_offset, literal=literal)
            vs, s, nu, W, acc = res["v"], res["scale"], res["nu"], res["W"], res["accepted"]
            status = or_status(fstatus, res.get("status"))
            yield StudentT.State(StudentT.Params(host(s).copy(), W, d), host(vs).copy() if keep_variances else None,
                                 host(nu).astype(np.int32), host(theta).copy() if keep_theta else None,
                                 host(acc).astype(np.int32),
                                 host(res["loglik"]).copy() if res.get("loglik") is not None else None, status)
