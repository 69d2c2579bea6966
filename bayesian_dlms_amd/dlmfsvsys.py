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
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterator, Optional

import numpy as np

from . import _lib
from ._chain import host, is_torch, or_status, place
from .dlm import Dlm, DlmParameters, materialise
from .dlmfsv import DlmFsv
from .factorsv import FactorSv, FsvParameters
from .gibbs import InverseGamma
from .stochvol import Gaussian, StochasticVolatility

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
    @dataclass
    class State:
        """DlmFsvSystem.State (:24-29), batched.  params: {"beta" [N][d][k], "v" [N][d], "sv" [N][k][3], "V" [N][p]} on the host; theta
        [N][T+1][d], factors [N][k][T] and volatility [N][k][T+1] host copies when asked for (keep_states) else None; status [N]: the
        flags of the iteration's calls or'ed (the factor chains' folded onto their panel)."""
        params: dict
        theta: Optional[np.ndarray]
        factors: Optional[np.ndarray]
        volatility: Optional[np.ndarray]
        status: np.ndarray

    @staticmethod
    def _model(mod, T, times=None):
        grid = np.arange(1, T + 1, dtype=np.float64) if times is None else np.asarray(host(times), dtype=np.float64).reshape(-1)
        if grid.shape != (T,) or not np.array_equal(np.diff(grid), np.ones(T - 1)):
            raise ValueError("DlmFsvSystem runs on a regular unit time grid (times[t+1] - times[t] = 1 for all t): the AR(1) log-volatility "
                             "of the factors has no dt")
        mat = materialise(mod, grid)
        if mat.n_g != 1 or mat.g_index is not None or mat.dt is not None:
            raise ValueError("DlmFsvSystem takes a model with one G on the regular unit time grid")
        return mat

    @staticmethod
    def _shape(ys, mat, init_p):
        if len(ys.shape) != 3:
            raise ValueError(f"ys must be [N][T][p], got the shape {tuple(ys.shape)}")
        N, T, p = (int(x) for x in ys.shape)
        d, k = mat.d, init_p.fsv.k
        if p != mat.p or init_p.dlm.v.shape != (p, p):
            raise ValueError(f"ys has p = {p} series, the model's F {mat.p} columns and V is {init_p.dlm.v.shape[0]} x {init_p.dlm.v.shape[1]}")
        if d != init_p.fsv.p or init_p.dlm.m0.shape != (d,) or init_p.dlm.c0.shape != (d, d):
            raise ValueError(f"the model has d = {d} states: beta must have d rows, C0 must be d x d and m0 [d]")
        if d > 64:
            raise ValueError(f"d = {d}: the innovations kernel takes d <= 64")
        if k > d:
            raise ValueError(f"k = {k} factors for d = {d} states: the factor model needs k <= d")
        if T < 2:
            raise ValueError("the factor stochastic-volatility sampler needs T >= 2 (the reference's sums throw on a single observation)")
        return N, T, p, k, d

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
    def initialise_state(ys, mod, init_p: DlmFsvSystemParameters, engine, *, seed: int = 0, series_offset: int = 0, literal: bool = False,
                         times=None):
        """initialise (:306-320): one FFBS under W_t = 0.1 I (Q36), the innovations of that theta, then FactorSv.initialise_state_ar on
        them.  Returns the device-resident chain state: FactorSv's dict (its "y" is w, the innovations [N][T][d]) plus {"ys", "theta"
        [N][T+1][d], "V" [N][p*p], "m0", "C0", "W" [N][T][d*d] (not yet written), "mat"}.  Refuses a W_t stream that does not fit the
        device."""
        if len(ys.shape) != 3:
            raise ValueError(f"ys must be [N][T][p], got the shape {tuple(ys.shape)}")
        mat = DlmFsvSystem._model(mod, int(ys.shape[1]), times)
        N, T, p, k, d = DlmFsvSystem._shape(ys, mat, init_p)
        nbytes = 8 * N * T * d * d
        if engine is not None:
            free, _ = engine.mem_info()
            if nbytes > free:
                raise MemoryError(f"the W_t stream of {N} panels x {T} times x {d} x {d} doubles takes {nbytes / 1e9:.2f} GB, the device has "
                                  f"{free / 1e9:.2f} GB free: run fewer panels per call (series_offset keeps the draws)")
        put, y = place(ys, engine, N, T * p)
        y = y.reshape(N, T, p)
        V = put(np.broadcast_to(np.ascontiguousarray(init_p.dlm.v.T).reshape(-1), (N, p * p)))
        m0 = put(init_p.dlm.m0.reshape(-1))
        C0 = put(np.ascontiguousarray(init_p.dlm.c0.T).reshape(-1))
        w0 = put((INIT_W * np.eye(d)).reshape(-1))
        out = engine.ffbs(mat, DlmFsvSystem._packed(V, p, w0, 0, d, m0, C0), y, seed=DlmFsv._seed_theta(seed, 0), series_offset=series_offset,
                          want_theta=True, want_stats=False, want_filt=False)
        theta = out["theta"]
        inn = engine.dlmfsvsys_innovations(mat, theta)
        c = FactorSv.initialise_state_ar(inn["w"], init_p.fsv, engine, seed=seed, series_offset=series_offset, literal=literal)
        c["status"] = or_status(or_status(out["status"], inn["status"]), c["status"])
        W = theta.new_empty((N, T, d * d)) if is_torch(theta) else np.empty((N, T, d * d))
        c.update(ys=y, theta=theta, V=V, m0=m0, C0=C0, W=W, mat=mat)
        return c

    @staticmethod
    def sample(prior_beta: Gaussian, prior_sigma_eta: InverseGamma, prior_phi: Gaussian, prior_mu: Gaussian, prior_sigma: InverseGamma,
               prior_v: InverseGamma, ys, mod: Dlm, init_p: DlmFsvSystemParameters, engine, *, n_iter: int, seed: int = 0,
               series_offset: int = 0, literal: bool = False, literal_order: bool = False, keep_states: bool = True,
               times=None) -> Iterator["DlmFsvSystem.State"]:
        """DlmFsvSystem.sample (:322-344) for N independent panels: ys [N][T][p] (NaN = missing; numpy or a torch device tensor), every
        panel started at init_p.  The priors are FactorSv.sample_ar's (in the reference's order here: sigma_eta, phi, mu) and prior_v, the
        InverseGamma of every V_ii.  literal: the reference's arithmetic in the five factor calls; literal_order: the reference's order
        of the steps (Q35).  times: None (1 .. T) or a regular unit grid.  Yields one State per iteration."""
        if not (isinstance(prior_beta, Gaussian) and isinstance(prior_mu, Gaussian) and isinstance(prior_phi, Gaussian)
                and isinstance(prior_sigma_eta, InverseGamma) and isinstance(prior_sigma, InverseGamma) and isinstance(prior_v, InverseGamma)):
            raise TypeError("the device evaluates Gaussian priors of beta, phi and mu and InverseGamma priors of sigma_eta^2, sigma^2 and V_ii only")
        if not isinstance(init_p, DlmFsvSystemParameters):
            raise TypeError("init_p must be a DlmFsvSystemParameters")
        if len(ys.shape) != 3:
            raise ValueError(f"ys must be [N][T][p], got the shape {tuple(ys.shape)}")
        mat = DlmFsvSystem._model(mod, int(ys.shape[1]), times)
        DlmFsvSystem._shape(ys, mat, init_p)
        lit = 1 if literal else 0
        sv_prior = _lib.SvPrior(0, lit, prior_phi.mean, prior_phi.sd, prior_mu.mean, prior_mu.sd, prior_sigma_eta.shape,
                                prior_sigma_eta.scale, 100.0, 0.05)
        fsv_prior = _lib.FsvPrior(lit, prior_beta.mean, prior_beta.sd, prior_sigma.shape, prior_sigma.scale)
        return DlmFsvSystem._run(ys, mod, init_p, engine, sv_prior, fsv_prior, prior_v, n_iter, seed, series_offset, literal, literal_order,
                                 keep_states, times)

    @staticmethod
    def _run(ys, mod, init_p, engine, sv_prior, fsv_prior, prior_v, n_iter, seed, series_offset, literal, literal_order, keep_states, times):
        c = DlmFsvSystem.initialise_state(ys, mod, init_p, engine, seed=seed, series_offset=series_offset, literal=literal, times=times)
        mat, y, theta, V, m0, C0, W = c["mat"], c["ys"], c["theta"], c["V"], c["m0"], c["C0"], c["W"]
        w, f, alpha, sv, beta, v = c["y"], c["f"], c["alpha"], c["sv"], c["beta"], c["v"]
        bufs, status0 = {"ystar": c["ystar"], "v": c["v_mix"]}, c["status"]
        N, T, p = (int(x) for x in y.shape)
        k, d = int(beta.shape[2]), mat.d
        so = series_offset
        for it in range(n_iter):
            inn = engine.dlmfsvsys_innovations(mat, theta, out={"w": w})
            fac = None
            if not literal_order:
                fac = engine.fsv_factors(w, beta, v, alpha, iteration=it, seed=seed, series_offset=so, literal=literal, out={"f": f})
            sv2 = sv.reshape(N * k, 3)
            st = StochasticVolatility.sample_state_ar(f.reshape(N * k, T), alpha.reshape(N * k, T + 1), sv2, engine, iteration=it,
                                                      seed=seed, series_offset=so * k, out=bufs)
            alpha, bufs = st["alpha"].reshape(N, k, T + 1), {"ystar": st["ystar"], "v": st["v"]}
            res = engine.sv_params(alpha.reshape(N * k, T + 1), sv2, sv_prior, iteration=it, seed=seed, series_offset=so * k, out={"sv": sv2})
            if literal_order:
                fac = engine.fsv_factors(w, beta, v, alpha, iteration=it, seed=seed, series_offset=so, literal=literal, out={"f": f})
            load = engine.fsv_loadings(w, f, beta, fsv_prior, iteration=it, seed=seed, series_offset=so, v=v, out={"beta": beta, "v": v})
            var = engine.dlmfsv_variance(beta, v, alpha, out={"V": W})
            out = engine.ffbs(mat, DlmFsvSystem._packed(V, p, W, T, d, m0, C0), y, seed=DlmFsv._seed_theta(seed, it + 1), series_offset=so,
                              want_theta=True, want_stats=True, want_filt=False)
            theta = out["theta"]
            V, _ = engine.dinvgamma_step(d, p, out["stats"], prior_v, prior_v, iteration=it, seed=seed, series_offset=so)
            status = or_status(FactorSv._fold(or_status(st["status"], res.get("status")), N, k), or_status(fac["status"], load["status"]))
            status = or_status(status, or_status(or_status(inn["status"], var["status"]), out["status"]))
            if it == 0:
                status = or_status(status, status0)
            params = {"beta": host(beta).copy(), "v": host(v).copy(), "sv": host(sv).copy(),
                      "V": np.diagonal(host(V).reshape(N, p, p), axis1=1, axis2=2).copy()}
            keep = keep_states
            yield DlmFsvSystem.State(params, host(theta).copy() if keep else None, host(f).copy() if keep else None,
                                     host(alpha).copy() if keep else None, status)
