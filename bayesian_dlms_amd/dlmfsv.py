"""Gibbs sampler of the DLM whose observation noise is a factor stochastic-volatility process (DlmFsv.sample, DlmFsv.scala:64-318).

  theta_0 ~ N(m0, C0),  theta_t = G theta_{t-1} + w_t,  w_t ~ N(0, W),  W diagonal, W_ii ~ InverseGamma(prior_w)
  y_t = F_t^T theta_t + beta f_t + eps_t,  eps_t ~ N(0, diag(v)),  f_{j,t} ~ N(0, exp(alpha_{j,t}))         the FSV part as factorsv.py has it

A batch is N independent panels: ys [N][T][p], NaN = missing, one model (F, G) on the regular unit time grid (the AR(1) volatility has
no dt).  y[t] belongs to theta[t+1] and to alpha[..][t+1].  One iteration in the default order, everything device-resident:

  1 dlm_dlmfsv_center_batch      r_t = y_t - F_t^T theta_{t+1}, NaN kept                     (factorObs, :173-185)
    dlm_dlmfsv_impute_batch      the missing components of a partially missing r_t | its observed ones, alpha, beta, v      (Q34)
  2 dlm_fsv_factors_batch on r   f | r, alpha, beta, v
  3 dlm_sv_mixture_batch, dlm_ar1_ffbs_batch, dlm_sv_params_batch on f      alpha | f, then (phi, mu, sigma_eta) | alpha
  4 dlm_fsv_loadings_batch on (r, f)   sigma^2, beta
  5 dlm_dlmfsv_variance_batch    V_t = beta diag(exp(alpha_{.,t+1})) beta^T + diag(v)         (DlmFsvSystem.calculateVariance)
  6 dlm_ffbs_batch               theta | y, V_{1:T}, W with f integrated out (the V_t stream, per-panel W)
  7 dlm_dinvgamma_step_batch     W | theta                                                   (GibbsSampling.sampleSystemMatrix)

A wholly missing time is missing for every step; V_t is written for every t.  A time with SOME components missing is partially
observed for step 6, while the factor calls of steps 2-4 take a time with any component missing as wholly missing.  Q34: in the
reference the factor half therefore draws without observations the state draw uses, which is not a draw from its full conditionals
(the variance of the whitened residuals stands 6 standard errors off after three sweeps from the joint law).  By default the driver
completes such a time first: the missing components are drawn given the observed ones, which with the factor draw that follows is one
joint draw of (the missing components, f_t), and steps 2-4 read the completed panel.  literal_missing=True is the reference's treatment.

Q32: DlmFsv.sampleStep runs 3, 2, 4, 5, 6, 7, so its next step 3 conditions on the f drawn before theta was redrawn with f
integrated out -- a partially collapsed Gibbs sampler in the wrong order, which does not leave the posterior invariant.  With the
factor draw in front, step 6 and the next step 2 are one joint draw of (theta, f).  literal_order=True keeps the reference's order.
Q33: ffbsSvd (:208-228) is not reproduced -- initialiseState stores sqrtSvd(W), sampleStep then stores the raw InverseGamma draw where
that square root sat, and Q2 applies on top; theta is drawn with the standard-form dlm_ffbs_batch, the same law.  No literal mode.
literal=True is the reference's arithmetic in the five factor calls (Q16-Q19, Q27-Q30).

The checks, the initialisation and the sweep are _dlmfsv.py's, shared with dlmfsvsys.py (steps 2-4 are factorsv.factor_half); what is
this sampler's own -- step 1, which variance is the stream, the first draw's V_t -- is KIND at the end of this file.
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


@dataclass
class DlmFsvParameters:
    """DlmFsvParameters(dlm, fsv) (DlmFsv.scala:20-58).  dlm.v is not read: the observation variance is the factor part's."""
    dlm: DlmParameters
    fsv: FsvParameters

    def __post_init__(self):
        if not isinstance(self.dlm, DlmParameters) or not isinstance(self.fsv, FsvParameters):
            raise TypeError("DlmFsvParameters takes a DlmParameters and an FsvParameters")
        w = self.dlm.w
        if w.ndim != 2 or np.count_nonzero(w - np.diag(np.diagonal(w))) or not (np.diagonal(w) > 0.0).all():
            raise ValueError("W must be a diagonal matrix with a positive diagonal (W_ii ~ InverseGamma)")


class DlmFsv:
    State = _dlmfsv.State
    _seed_theta = staticmethod(_dlmfsv.seed_theta)

    @staticmethod
    def _model(mod, T, times=None):
        return _dlmfsv.unit_grid_model("DlmFsv", mod, T, times)

    @staticmethod
    def _shape(dims, mat, init_p):
        N, T, p = dims
        d = mat.d
        if p != init_p.fsv.p or p != mat.p:
            raise ValueError(f"ys has p = {p} series, the initial beta {init_p.fsv.p} rows and the model's F {mat.p} columns")
        if init_p.dlm.w.shape != (d, d) or init_p.dlm.m0.shape != (d,) or init_p.dlm.c0.shape != (d, d):
            raise ValueError(f"the model has d = {d} states: W and C0 must be d x d and m0 [d]")
        if d > 64:
            raise ValueError(f"d = {d}: the centring kernel takes d <= 64")
        return init_p.fsv.k, d

    @staticmethod
    def simulate(mod: Dlm, params: DlmFsvParameters, T: int, N: int, seed: int = 0):
        """DlmFsv.simulate (:140-148) for N panels with NumPy: (y [N][T][p], theta [N][T+1][d], f [N][k][T], alpha [N][k][T+1]) on the
        times 1 .. T, alpha[:, j, 0] the stationary initial state of factor j.  For tests and benchmarks."""
        mat = DlmFsv._model(mod, T)
        d, p = mat.d, mat.p
        if p != params.fsv.p:
            raise ValueError(f"the model's F has {p} columns, beta {params.fsv.p} rows")
        e, f, alpha = FactorSv.simulate(params.fsv, T, N, seed=seed)
        rng = np.random.default_rng([int(seed), 0x444C4D])
        G = mat.G.reshape(mat.n_g, d, d).transpose(0, 2, 1)[0]
        theta = np.empty((N, T + 1, d))
        theta[:, 0] = params.dlm.m0 + rng.standard_normal((N, d)) @ np.linalg.cholesky(params.dlm.c0).T
        sw = np.sqrt(np.diagonal(params.dlm.w))
        y = np.empty((N, T, p))
        for t in range(T):
            theta[:, t + 1] = theta[:, t] @ G.T + sw * rng.standard_normal((N, d))
            Ft = mat.F[t * mat.f_stride:t * mat.f_stride + d * p].reshape(p, d).T
            y[:, t] = theta[:, t + 1] @ Ft + e[:, t]
        return y, theta, f, alpha

    @staticmethod
    def _packed(V, T, p, W, d, m0, C0):
        """The parameter tuple of Engine.ffbs: the V_t stream [N][T][p p] (or one shared p x p matrix, T = 0) and per-panel W."""
        return (V.reshape(-1), T * p * p, W.reshape(-1), d * d, m0, 0, C0, 0, p * p if T else 0, 0)

    @staticmethod
    def _data(engine, c, it, seed, series_offset, literal_missing=False):
        """Step 1: the centred panel into c["y"]; its partially missing times completed (Q34) unless literal_missing or at the start
        (it = None: initialiseState's, before there is an alpha)."""
        cen = engine.dlmfsv_center(c["mat"], c["ys"], c["theta"], out={"r": c["y"]} if "y" in c else None)
        c["y"], st = cen["r"], {"center": cen["status"]}
        if it is not None and not literal_missing:
            st["impute"] = engine.dlmfsv_impute(c["y"], c["beta"], c["v"], c["alpha"], iteration=it, seed=seed, series_offset=series_offset,
                                                out={"r": c["y"]})["status"]
        return st

    @staticmethod
    def initialise_state(ys, mod, init_p: DlmFsvParameters, engine, *, seed: int = 0, series_offset: int = 0, literal: bool = False,
                         times=None):
        """initialiseState (:267-286): one FFBS under V_t = I, the panel centred on that theta, then FactorSv.initialise_state_ar on it.
        Returns the device-resident chain state: FactorSv's dict (its "y" is r, the centred panel) plus {"ys", "theta" [N][T+1][d],
        "W" [N][d*d], "m0", "C0", "V" [N][T][p*p] (not yet written), "mat"}.  Refuses a V_t stream that does not fit the device."""
        return _dlmfsv.initialise(KIND, ys, mod, init_p, engine, seed=seed, series_offset=series_offset, literal=literal, times=times)

    @staticmethod
    def sample(prior_beta: Gaussian, prior_sigma_eta: InverseGamma, prior_phi: Gaussian, prior_mu: Gaussian, prior_sigma: InverseGamma,
               prior_w: InverseGamma, ys, mod: Dlm, init_p: DlmFsvParameters, engine, *, n_iter: int, seed: int = 0, series_offset: int = 0,
               literal: bool = False, literal_order: bool = False, keep_states: bool = True, times=None,
               literal_missing: bool = False) -> Iterator["DlmFsv.State"]:
        """DlmFsv.sample (:291-318) for N independent panels: ys [N][T][p] (NaN = missing; numpy or a torch device tensor), every panel
        started at init_p.  The priors are FactorSv.sample_ar's (in the reference's order here: sigma_eta, phi, mu) and prior_w, the
        InverseGamma of every W_ii.  literal: the reference's arithmetic in the five factor calls; literal_order: the reference's order
        of the steps (Q32); literal_missing: a partially missing time is wholly missing for the factor calls (Q34).  times: None (1 .. T) or a
        regular unit grid.  Yields one State per iteration."""
        return _dlmfsv.sample(KIND, DlmFsvParameters, (prior_beta, prior_sigma_eta, prior_mu, prior_phi, prior_sigma), prior_w, ys, mod, init_p,
                              engine, n_iter=n_iter, seed=seed, series_offset=series_offset, literal=literal, literal_order=literal_order,
                              keep_states=keep_states, times=times, literal_missing=literal_missing)

    @staticmethod
    def forecast(mod: Dlm, ys, draws, horizon: int, engine, *, m0, c0, n_paths: int = 64, prob: float = 0.75, probs=None, seed: int = 0,
                 series_offset: int = 0, times=None, budget=None):
        """DlmFsv.forecast (DlmFsv.scala:483-529) as a PURE forecast of y_{T+1 .. T+horizon} from kept draws (Q77-Q82 for what
        the reference's own does).  Per draw: (m_T, C_T) from the Kalman filter over ys under the draw's own V_t stream (its theta is
        integrated out), n_paths log-volatility paths from the draw's alpha_T, V_h = beta diag(exp(alpha_{.,T+h})) beta^T + diag(v),
        and the Kalman forecast under it with the draw's W.  draws: a list of the States of sample kept with their states, or a dict
        of stacked arrays {"beta", "v", "sv", "w" [M][N][.], "alpha" [M][N][k][T+1]}.  m0, c0: the prior of theta_0 the sampler
        ran with (init_p.dlm.m0, init_p.dlm.c0).  Returns {"mean" [N][H][p], "cov" [N][H][p][p] (the total predictive covariance),
        "lower", "upper" [N][H][p] the exact mixture quantiles at 1 - prob and prob (Dlm.summariseForecast's interval), "quantiles"
        [N][H][p][len(probs)] or None, "status" [N]}.  times: the training grid (a non-unit grid raises the sampler's error).
        budget: bytes of device memory the call may use (default: 60 % of what is free)."""
        return _dlmfsv.forecast(KIND, mod, ys, draws, horizon, engine, m0=m0, c0=c0, n_paths=n_paths, prob=prob, probs=probs, seed=seed,
                                series_offset=series_offset, times=times, budget=budget)


# the factor part is the observation noise: V_t is the stream, W static; the first state draw runs under V_t = I
KIND = _dlmfsv.Kind(stream="V", param="w", first=1.0, model=DlmFsv._model, shape=DlmFsv._shape, data=DlmFsv._data,
                    packed=lambda c, T: DlmFsv._packed(c["V"], T, c["mat"].p, c["W"], c["mat"].d, c["m0"], c["C0"]))
