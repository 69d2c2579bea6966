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
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterator, Optional

import numpy as np

from . import _lib
from ._chain import host, is_torch, or_status, place
from .dlm import Dlm, DlmParameters, materialise
from .factorsv import FactorSv, FsvParameters
from .gibbs import InverseGamma
from .stochvol import MASK64, Gaussian, StochasticVolatility


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
    @dataclass
    class State:
        """DlmFsv.State (:159-164), batched.  params: {"beta" [N][p][k], "v" [N][p], "sv" [N][k][3], "w" [N][d]} on the host; theta
        [N][T+1][d], factors [N][k][T] and volatility [N][k][T+1] host copies when asked for (keep_states) else None; status [N]: the
        flags of the iteration's calls or'ed (the factor chains' folded onto their panel)."""
        params: dict
        theta: Optional[np.ndarray]
        factors: Optional[np.ndarray]
        volatility: Optional[np.ndarray]
        status: np.ndarray

    @staticmethod
    def _seed_theta(seed, k):
        # dlm_ffbs_batch and dlm_ar1_ffbs_batch key their normals by (seed, series, t) alone: a seed per call (studentt.py's rule,
        # k = 0 the initial state's), with the top bit flipped so that no state draw shares its normals with a factor chain's
        # volatility draw (StochasticVolatility._seed_ffbs of the same seed)
        return ((int(seed) * 1000003 + k) ^ (1 << 63)) & MASK64

    @staticmethod
    def _model(mod, T, times=None):
        grid = np.arange(1, T + 1, dtype=np.float64) if times is None else np.asarray(host(times), dtype=np.float64).reshape(-1)
        if grid.shape != (T,) or not np.array_equal(np.diff(grid), np.ones(T - 1)):
            raise ValueError("DlmFsv runs on a regular unit time grid (times[t+1] - times[t] = 1 for all t): the AR(1) log-volatility of the "
                             "factors has no dt")
        return materialise(mod, grid)

    @staticmethod
    def _shape(ys, mat, init_p):
        if len(ys.shape) != 3:
            raise ValueError(f"ys must be [N][T][p], got the shape {tuple(ys.shape)}")
        N, T, p = (int(x) for x in ys.shape)
        d = mat.d
        if p != init_p.fsv.p or p != mat.p:
            raise ValueError(f"ys has p = {p} series, the initial beta {init_p.fsv.p} rows and the model's F {mat.p} columns")
        if init_p.dlm.w.shape != (d, d) or init_p.dlm.m0.shape != (d,) or init_p.dlm.c0.shape != (d, d):
            raise ValueError(f"the model has d = {d} states: W and C0 must be d x d and m0 [d]")
        if d > 64:
            raise ValueError(f"d = {d}: the centring kernel takes d <= 64")
        if T < 2:
            raise ValueError("the factor stochastic-volatility sampler needs T >= 2 (the reference's sums throw on a single observation)")
        return N, T, p, init_p.fsv.k, d

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
    def initialise_state(ys, mod, init_p: DlmFsvParameters, engine, *, seed: int = 0, series_offset: int = 0, literal: bool = False,
                         times=None):
        """initialiseState (:267-286): one FFBS under V_t = I, the panel centred on that theta, then FactorSv.initialise_state_ar on it.
        Returns the device-resident chain state: FactorSv's dict (its "y" is r, the centred panel) plus {"ys", "theta" [N][T+1][d],
        "W" [N][d*d], "m0", "C0", "V" [N][T][p*p] (not yet written), "mat"}.  Refuses a V_t stream that does not fit the device."""
        if len(ys.shape) != 3:
            raise ValueError(f"ys must be [N][T][p], got the shape {tuple(ys.shape)}")
        mat = DlmFsv._model(mod, int(ys.shape[1]), times)
        N, T, p, k, d = DlmFsv._shape(ys, mat, init_p)
        nbytes = 8 * N * T * p * p
        if engine is not None:
            free, _ = engine.mem_info()
            if nbytes > free:
                raise MemoryError(f"the V_t stream of {N} panels x {T} times x {p} x {p} doubles takes {nbytes / 1e9:.2f} GB, the device has "
                                  f"{free / 1e9:.2f} GB free: run fewer panels per call (series_offset keeps the draws)")
        put, y = place(ys, engine, N, T * p)
        y = y.reshape(N, T, p)
        W = put(np.broadcast_to(np.ascontiguousarray(init_p.dlm.w.T).reshape(-1), (N, d * d)))
        m0 = put(init_p.dlm.m0.reshape(-1))
        C0 = put(np.ascontiguousarray(init_p.dlm.c0.T).reshape(-1))
        eye = put(np.eye(p).reshape(-1))
        out = engine.ffbs(mat, DlmFsv._packed(eye, 0, p, W, d, m0, C0), y, seed=DlmFsv._seed_theta(seed, 0), series_offset=series_offset,
                          want_theta=True, want_stats=False, want_filt=False)
        theta = out["theta"]
        cen = engine.dlmfsv_center(mat, y, theta)
        c = FactorSv.initialise_state_ar(cen["r"], init_p.fsv, engine, seed=seed, series_offset=series_offset, literal=literal)
        c["status"] = or_status(or_status(out["status"], cen["status"]), c["status"])
        V = theta.new_empty((N, T, p * p)) if is_torch(theta) else np.empty((N, T, p * p))
        c.update(ys=y, theta=theta, W=W, m0=m0, C0=C0, V=V, mat=mat)
        return c

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
        if not (isinstance(prior_beta, Gaussian) and isinstance(prior_mu, Gaussian) and isinstance(prior_phi, Gaussian)
                and isinstance(prior_sigma_eta, InverseGamma) and isinstance(prior_sigma, InverseGamma) and isinstance(prior_w, InverseGamma)):
            raise TypeError("the device evaluates Gaussian priors of beta, phi and mu and InverseGamma priors of sigma_eta^2, sigma^2 and W_ii only")
        if not isinstance(init_p, DlmFsvParameters):
            raise TypeError("init_p must be a DlmFsvParameters")
        if len(ys.shape) != 3:
            raise ValueError(f"ys must be [N][T][p], got the shape {tuple(ys.shape)}")
        mat = DlmFsv._model(mod, int(ys.shape[1]), times)
        DlmFsv._shape(ys, mat, init_p)
        lit = 1 if literal else 0
        sv_prior = _lib.SvPrior(0, lit, prior_phi.mean, prior_phi.sd, prior_mu.mean, prior_mu.sd, prior_sigma_eta.shape,
                                prior_sigma_eta.scale, 100.0, 0.05)
        fsv_prior = _lib.FsvPrior(lit, prior_beta.mean, prior_beta.sd, prior_sigma.shape, prior_sigma.scale)
        return DlmFsv._run(ys, mod, init_p, engine, sv_prior, fsv_prior, prior_w, n_iter, seed, series_offset, literal, literal_order,
                           keep_states, times, literal_missing)

    @staticmethod
    def _run(ys, mod, init_p, engine, sv_prior, fsv_prior, prior_w, n_iter, seed, series_offset, literal, literal_order, keep_states, times,
             literal_missing=False):
        c = DlmFsv.initialise_state(ys, mod, init_p, engine, seed=seed, series_offset=series_offset, literal=literal, times=times)
        mat, y, theta, W, m0, C0, V = c["mat"], c["ys"], c["theta"], c["W"], c["m0"], c["C0"], c["V"]
        r, f, alpha, sv, beta, v = c["y"], c["f"], c["alpha"], c["sv"], c["beta"], c["v"]
        bufs, status0 = {"ystar": c["ystar"], "v": c["v_mix"]}, c["status"]
        N, T, p = (int(x) for x in y.shape)
        k, d = int(beta.shape[2]), mat.d
        so = series_offset
        for it in range(n_iter):
            cen = engine.dlmfsv_center(mat, y, theta, out={"r": r})
            if not literal_missing:
                imp = engine.dlmfsv_impute(r, beta, v, alpha, iteration=it, seed=seed, series_offset=so, out={"r": r})
                cen["status"] = or_status(cen["status"], imp["status"])
            fac = None
            if not literal_order:
                fac = engine.fsv_factors(r, beta, v, alpha, iteration=it, seed=seed, series_offset=so, literal=literal, out={"f": f})
            sv2 = sv.reshape(N * k, 3)
            st = StochasticVolatility.sample_state_ar(f.reshape(N * k, T), alpha.reshape(N * k, T + 1), sv2, engine, iteration=it,
                                                      seed=seed, series_offset=so * k, out=bufs)
            alpha, bufs = st["alpha"].reshape(N, k, T + 1), {"ystar": st["ystar"], "v": st["v"]}
            res = engine.sv_params(alpha.reshape(N * k, T + 1), sv2, sv_prior, iteration=it, seed=seed, series_offset=so * k, out={"sv": sv2})
            if literal_order:
                fac = engine.fsv_factors(r, beta, v, alpha, iteration=it, seed=seed, series_offset=so, literal=literal, out={"f": f})
            load = engine.fsv_loadings(r, f, beta, fsv_prior, iteration=it, seed=seed, series_offset=so, v=v, out={"beta": beta, "v": v})
            var = engine.dlmfsv_variance(beta, v, alpha, out={"V": V})
            out = engine.ffbs(mat, DlmFsv._packed(V, T, p, W, d, m0, C0), y, seed=DlmFsv._seed_theta(seed, it + 1), series_offset=so,
                              want_theta=True, want_stats=True, want_filt=False)
            theta = out["theta"]
            _, W = engine.dinvgamma_step(d, p, out["stats"], prior_w, prior_w, iteration=it, seed=seed, series_offset=so)
            status = or_status(FactorSv._fold(or_status(st["status"], res.get("status")), N, k), or_status(fac["status"], load["status"]))
            status = or_status(status, or_status(or_status(cen["status"], var["status"]), out["status"]))
            if it == 0:
                status = or_status(status, status0)
            params = {"beta": host(beta).copy(), "v": host(v).copy(), "sv": host(sv).copy(),
                      "w": np.diagonal(host(W).reshape(N, d, d), axis1=1, axis2=2).copy()}
            keep = keep_states
            yield DlmFsv.State(params, host(theta).copy() if keep else None, host(f).copy() if keep else None,
                               host(alpha).copy() if keep else None, status)
