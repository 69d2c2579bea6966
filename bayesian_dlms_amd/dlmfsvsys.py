"""Gibbs sampler of the DLM whose system noise is a factor stochastic-volatility process (DlmFsvSystem.sample, DlmFsvSystem.scala:215-344).

  theta_0 ~ N(m0, C0),  theta_t = G theta_{t-1} + beta f_t + eps_t,  eps_t ~ N(0, diag(v)),  f_{j,t} ~ N(0, exp(alpha_{j,t}))
  y_t = F_t^T theta_t + nu_t,  nu_t ~ N(0, V),  V diagonal, V_ii ~ InverseGamma(prior_v)      the FSV part as factorsv.py has it, with p := d

A batch is N independent panels: ys [N][T][p], NaN = missing, one model (F, G) on the regular unit time grid (the AR(1) volatility has
no dt).  The innovation w[t] = theta[t+1] - G theta[t] belongs to alpha[..][t+1], as y[t] does in dlmfsv.py.  One iteration in the default
order, everything device-resident:

  1 dlm_dlmfsvsys_innovations_batch   w_t = theta_{t+1} - G theta_t                          (factorState, :109-117)
  2 dlm_fsv_factors_batch on w        f | w, alpha, beta, v
  3 dlm_sv_mixture_batch, dlm_ar1_ffbs_batch, dlm_sv_params_batch on f      alpha | f, then (phi, mu, sigma_eta) | alpha
  4 dlm_fsv_loadings_batch on (w, f)  sigma^2, beta
  5 dlm_dlmfsv_variance_batch (p := d)  W_t = beta diag(exp(alpha_{.,t+1})) beta^T + diag(v)   (calculateVariance, :126-131), [N][T][d d]
  6 dlm_ffbs_batch                    theta | y, W_{1:T}, V with f integrated out (the W_t stream, per-panel diagonal V)
  7 dlm_dinvgamma_step_batch          V | theta, y                                           (sampleObservationMatrix, :246)

The innovations are never missing, so nothing is completed before the factor calls (no analogue of Q34); a missing y, whole or in part,
is the state draw's business alone.

Q35: DlmFsvSystem.sampleStep runs 1, 3, 2, 4, 5, 6, 7 -- FactorSv.sampleStep (FactorSv.scala:546-562) begins with the
volatility draw given the factors, and those factors were drawn before theta was redrawn with f integrated out: a partially collapsed
Gibbs sampler in the wrong order (Q32's mistake), which does not leave the posterior invariant.  With the factor draw in front, step 6
and the next steps 1 and 2 are one joint draw of (theta, f).  literal_order=True keeps the reference's order.
Q36: initialise (:306-320) draws the first theta under W_t = 0.1 I whatever the initial parameters say; that is reproduced (it only
moves the starting point).  ffbsSvd / sampleStateAr are not reproduced, for Q33's reason; theta is drawn with the reference-form
dlm_ffbs_batch.  literal=True is the reference's arithmetic in the five factor calls (Q16-Q19, Q27-Q30).

The checks, the initialisation and the sweep are _dlmfsv.py's, shared with dlmfsv.py (steps 2-4 are factorsv.factor_half); what is this
sampler's own -- step 1, which variance is the stream, the first draw's W_t -- is KIND at the end of this file.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterator

import numpy as np

from . import _dlmfsv
from .dlm import Dlm, DlmParameters
from .factorsv import FactorSv, FsvParameters
from .gibbs import InverseGamma
from .stochvol import Gaussian

INIT_W = 0.1          # initialise (:311-312): the first state draw runs under W_t = 0.1 I


@dataclass
class DlmFsvSystemParameters:
    """DlmFsvParameters(dlm, fsv) as DlmFsvSystem reads it (:36-50): fsv is the factor model of the d state innovations (beta d x k,
    v [d]), dlm.v the diagonal observation variance.  dlm.w is not read: the system variance is the factor part's."""
    dlm: DlmParameters
    fsv: FsvParameters

    def __post_init__(self):
        if not isinstance(self.dlm, DlmParameters) or not isinstance(self.fsv, FsvParameters):
            raise TypeError("DlmFsvSystemParameters takes a DlmParameters and an FsvParameters")
        v = self.dlm.v
        if v.ndim != 2 or v.shape[0] != v.shape[1] or np.count_nonzero(v - np.diag(np.diagonal(v))) or not (np.diagonal(v) > 0.0).all():
            raise ValueError("V must be a diagonal matrix with a positive diagonal (V_ii ~ InverseGamma)")
        d = self.dlm.m0.shape[0]
        if self.fsv.p != d:
            raise ValueError(f"the factor model is the system noise's: beta must have d = {d} rows (m0 has {d} entries), got {self.fsv.p}")


class DlmFsvSystem:
    State = _dlmfsv.State

    @staticmethod
    def _model(mod, T, times=None):
        mat = _dlmfsv.unit_grid_model("DlmFsvSystem", mod, T, times)
        if mat.n_g != 1 or mat.g_index is not None or mat.dt is not None:
            raise ValueError("DlmFsvSystem takes a model with one G on the regular unit time grid")
        return mat

    @staticmethod
    def _shape(dims, mat, init_p):
        N, T, p = dims
        d, k = mat.d, init_p.fsv.k
        if p != mat.p or init_p.dlm.v.shape != (p, p):
            raise ValueError(f"ys has p = {p} series, the model's F {mat.p} columns and V is {init_p.dlm.v.shape[0]} x {init_p.dlm.v.shape[1]}")
        if d != init_p.fsv.p or init_p.dlm.m0.shape != (d,) or init_p.dlm.c0.shape != (d, d):
            raise ValueError(f"the model has d = {d} states: beta must have d rows, C0 must be d x d and m0 [d]")
        if d > 64:
            raise ValueError(f"d = {d}: the innovations kernel takes d <= 64")
        if k > d:
            raise ValueError(f"k = {k} factors for d = {d} states: the factor model needs k <= d")
        return k, d

    @staticmethod
    def simulate(mod: Dlm, params: DlmFsvSystemParameters, T: int, N: int, seed: int = 0):
        """DlmFsvSystem.simulateRegular (:63-101) for N panels with NumPy: (y [N][T][p], theta [N][T+1][d], f [N][k][T], alpha
        [N][k][T+1]) on the times 1 .. T, alpha[:, j, 0] the stationary initial state of factor j (FactorSv.simulate's; the reference
        starts it at N(0, 1)).  For tests and benchmarks."""
        mat = DlmFsvSystem._model(mod, T)
        d, p = mat.d, mat.p
        if d != params.fsv.p or params.dlm.v.shape != (p, p):
            raise ValueError(f"the model has d = {d} states and p = {p} series: beta has {params.fsv.p} rows, V is {params.dlm.v.shape}")
        w, f, alpha = FactorSv.simulate(params.fsv, T, N, seed=seed)
        rng = np.random.default_rng([int(seed), 0x444C53])
        G = mat.G.reshape(d, d).T
        theta = np.empty((N, T + 1, d))
        theta[:, 0] = params.dlm.m0 + rng.standard_normal((N, d)) @ np.linalg.cholesky(params.dlm.c0).T
        sv = np.sqrt(np.diagonal(params.dlm.v))
        y = np.empty((N, T, p))
        for t in range(T):
            theta[:, t + 1] = theta[:, t] @ G.T + w[:, t]
            Ft = mat.F[t * mat.f_stride:t * mat.f_stride + d * p].reshape(p, d).T
            y[:, t] = theta[:, t + 1] @ Ft + sv * rng.standard_normal((N, p))
        return y, theta, f, alpha

    @staticmethod
    def _packed(V, p, W, T, d, m0, C0):
        """The parameter tuple of Engine.ffbs: per-panel V [N][p p] and the W_t stream [N][T][d d] (or one shared d x d matrix, T = 0)."""
        return (V.reshape(-1), p * p, W.reshape(-1), T * d * d, m0, 0, C0, 0, 0, d * d if T else 0)

    @staticmethod
    def _data(engine, c, it, seed, series_offset):
        """Step 1: the innovations of theta into c["y"] (it = None: initialise's)."""
        inn = engine.dlmfsvsys_innovations(c["mat"], c["theta"], out={"w": c["y"]} if "y" in c else None)
        c["y"] = inn["w"]
        return {"innovations": inn["status"]}

    @staticmethod
    def initialise_state(ys, mod, init_p: DlmFsvSystemParameters, engine, *, seed: int = 0, series_offset: int = 0, literal: bool = False,
                         times=None):
        """initialise (:306-320): one FFBS under W_t = 0.1 I (Q36), the innovations of that theta, then FactorSv.initialise_state_ar on
        them.  Returns the device-resident chain state: FactorSv's dict (its "y" is w, the innovations [N][T][d]) plus {"ys", "theta"
        [N][T+1][d], "V" [N][p*p], "m0", "C0", "W" [N][T][d*d] (not yet written), "mat"}.  Refuses a W_t stream that does not fit the
        device."""
        return _dlmfsv.initialise(KIND, ys, mod, init_p, engine, seed=seed, series_offset=series_offset, literal=literal, times=times)

    @staticmethod
    def sample(prior_beta: Gaussian, prior_sigma_eta: InverseGamma, prior_phi: Gaussian, prior_mu: Gaussian, prior_sigma: InverseGamma,
               prior_v: InverseGamma, ys, mod: Dlm, init_p: DlmFsvSystemParameters, engine, *, n_iter: int, seed: int = 0,
               series_offset: int = 0, literal: bool = False, literal_order: bool = False, keep_states: bool = True,
               times=None) -> Iterator["DlmFsvSystem.State"]:
        """DlmFsvSystem.sample (:322-344) for N independent panels: ys [N][T][p] (NaN = missing; numpy or a torch device tensor), every
        panel started at init_p.  The priors are FactorSv.sample_ar's (in the reference's order here: sigma_eta, phi, mu) and prior_v, the
        InverseGamma of every V_ii.  literal: the reference's arithmetic in the five factor calls; literal_order: the reference's order
        of the steps (Q35).  times: None (1 .. T) or a regular unit grid.  Yields one State per iteration."""
        return _dlmfsv.sample(KIND, DlmFsvSystemParameters, (prior_beta, prior_sigma_eta, prior_mu, prior_phi, prior_sigma), prior_v, ys, mod,
                              init_p, engine, n_iter=n_iter, seed=seed, series_offset=series_offset, literal=literal,
                              literal_order=literal_order, keep_states=keep_states, times=times)

    @staticmethod
    def forecast(mod: Dlm, ys, draws, horizon: int, engine, *, m0, c0, n_paths: int = 64, prob: float = 0.75, probs=None, seed: int = 0,
                 series_offset: int = 0, times=None, budget=None):
        """DlmFsvSystem.forecast (DlmFsvSystem.scala:441-486) as a PURE forecast of y_{T+1 .. T+horizon} from kept draws (Q77-Q82 for what
        the reference's own does).  Per draw: (m_T, C_T) from the Kalman filter over ys under the draw's own W_t stream (its theta is
        integrated out), n_paths log-volatility paths from the draw's alpha_T, W_h = beta diag(exp(alpha_{.,T+h})) beta^T + diag(v),
        and the Kalman forecast under it with the draw's diagonal V.  draws: a list of the States of sample kept with their states, or a dict
        of stacked arrays {"beta", "v", "sv", "V" [M][N][.], "alpha" [M][N][k][T+1]}.  m0, c0: the prior of theta_0 the sampler
        ran with (init_p.dlm.m0, init_p.dlm.c0).  Returns {"mean" [N][H][p], "cov" [N][H][p][p] (the total predictive covariance),
        "lower", "upper" [N][H][p] the exact mixture quantiles at 1 - prob and prob (Dlm.summariseForecast's interval), "quantiles"
        [N][H][p][len(probs)] or None, "status" [N]}.  times: the training grid (a non-unit grid raises the sampler's error).
        budget: bytes of device memory the call may use (default: 60 % of what is free)."""
        return _dlmfsv.forecast(KIND, mod, ys, draws, horizon, engine, m0=m0, c0=c0, n_paths=n_paths, prob=prob, probs=probs, seed=seed,
                                series_offset=series_offset, times=times, budget=budget)


# the factor part is the system noise: W_t is the stream, V static; the first state draw runs under W_t = INIT_W I
KIND = _dlmfsv.Kind(stream="W", param="V", first=INIT_W, model=DlmFsvSystem._model, shape=DlmFsvSystem._shape,
                    data=DlmFsvSystem._data,
                    packed=lambda c, T: DlmFsvSystem._packed(c["V"], c["mat"].p, c["W"], T, c["mat"].d, c["m0"], c["C0"]))
