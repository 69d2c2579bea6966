"""What the two Gibbs samplers of a DLM with a factor stochastic-volatility part share (dlmfsv.py: the part is the observation noise;
dlmfsvsys.py: it is the system noise): the State, the checks, the initialisation, one sweep and the generator around it.

`forecast` at the end is the posterior-predictive forecast of all three factor-SV models (FactorSv.forecast calls it without a Kind).

One of the two variances is the time stream V_t or W_t = beta diag(exp(alpha_{.,t+1})) beta^T + diag(v), the other one is static,
diagonal and drawn from its InverseGamma.  What tells the samplers apart is a Kind; the chain state is FactorSv.initialise_state_ar's
dict, whose "y" is the factor model's data, plus {"ys", "theta" [N][T+1][d], "m0", "C0", "mat", "V", "W"}: a V is p x p, a W d x d, the
stream [N][T][.] and the static one [N][.].
"""
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from ._chain import host, is_torch, or_status, place
from .dlm import materialise
from .factorsv import FactorSv, factor_half, fold_status, pack_priors, panel_dims
from .stochvol import StochasticVolatility


@dataclass(frozen=True)
class Kind:
    """What DlmFsv and DlmFsvSystem differ in."""
    stream: str             # "V" or "W": the variance that is the time stream; the other one is the static, diagonal one
    param: str              # the static variance's diagonal in State.params
    first: float            # the first state draw runs under the stream = first * I
    model: Callable         # (mod, T, times) -> the materialised model
    shape: Callable         # ((N, T, p), mat, init_p) -> (k, d), or a ValueError
    data: Callable          # (engine, c, it, seed, series_offset, **options): writes the factor model's data c["y"] from c["theta"] (into a
    #                         new buffer when c has none) and returns the statuses of its calls by name
    packed: Callable        # (c, T) -> the parameter tuple of Engine.ffbs, T = 0: c's stream is one matrix shared by all times

    @property
    def static(self):
        return "W" if self.stream == "V" else "V"


@dataclass
class State:
    """DlmFsv.State (DlmFsv.scala:159-164) and DlmFsvSystem.State (DlmFsvSystem.scala:24-29), batched.  params: {"beta", "v", "sv"
    [N][k][3]} and the diagonal of the static variance, "w" [N][d] (DlmFsv) or "V" [N][p] (DlmFsvSystem), on the host; theta [N][T+1][d],
    factors [N][k][T] and volatility [N][k][T+1] host copies when asked for (keep_states) else None; status [N]: the flags of the
    iteration's calls or'ed (the factor chains' folded onto their panel)."""
    params: dict
    theta: Optional[np.ndarray]
    factors: Optional[np.ndarray]
    volatility: Optional[np.ndarray]
    status: np.ndarray


def seed_theta(seed, k):
    # dlm_ffbs_batch and dlm_ar1_ffbs_batch key their normals by (seed, series, t) alone: a seed per call (studentt.py's rule,
    # k = 0 the initial state's), with the top bit flipped so that no state draw shares its normals with a factor chain's
    # volatility draw (StochasticVolatility._seed_ffbs of the same seed)
    return StochasticVolatility._seed_ffbs(seed, k) ^ (1 << 63)


def unit_grid_model(name, mod, T, times=None):
    grid = np.arange(1, T + 1, dtype=np.float64) if times is None else np.asarray(host(times), dtype=np.float64).reshape(-1)
    if grid.shape != (T,) or not np.array_equal(np.diff(grid), np.ones(T - 1)):
        raise ValueError(f"{name} runs on a regular unit time grid (times[t+1] - times[t] = 1 for all t): the AR(1) log-volatility of the "
                         "factors has no dt")
    return materialise(mod, grid)


def checked(kind, ys, mod, init_p, times):
    """(mat, N, T, p, k, d) of a call that may run."""
    dims = panel_dims(ys)
    mat = kind.model(mod, dims[1], times)
    return (mat,) + dims + kind.shape(dims, mat, init_p)


def initialise(kind, ys, mod, init_p, engine, *, seed, series_offset, literal, times):
    """One FFBS under the stream = kind.first I, the factor model's data of that theta (kind.data with it = None), then
    FactorSv.initialise_state_ar on it.  Refuses a stream that does not fit the device."""
    mat, N, T, p, k, d = checked(kind, ys, mod, init_p, times)
    side = {"V": p, "W": d}
    q, s = side[kind.stream], side[kind.static]
    nbytes = 8 * N * T * q * q
    if engine is not None:
        free, _ = engine.mem_info()
        if nbytes > free:
            raise MemoryError(f"the {kind.stream}_t stream of {N} panels x {T} times x {q} x {q} doubles takes {nbytes / 1e9:.2f} GB, the device "
                              f"has {free / 1e9:.2f} GB free: run fewer panels per call (series_offset keeps the draws)")
    put, y = place(ys, engine, N, T * p)
    static = getattr(init_p.dlm, kind.static.lower())
    c = {"ys": y.reshape(N, T, p), "mat": mat, "m0": put(init_p.dlm.m0.reshape(-1)), "C0": put(np.ascontiguousarray(init_p.dlm.c0.T).reshape(-1)),
         kind.static: put(np.broadcast_to(np.ascontiguousarray(static.T).reshape(-1), (N, s * s))), kind.stream: put((kind.first * np.eye(q)).reshape(-1))}
    out = engine.ffbs(mat, kind.packed(c, 0), c["ys"], seed=seed_theta(seed, 0), series_offset=series_offset, want_theta=True, want_stats=False,
                      want_filt=False)
    del c[kind.stream]
    c["theta"] = out["theta"]
    st = kind.data(engine, c, None, seed, series_offset)
    c.update(FactorSv.initialise_state_ar(c["y"], init_p.fsv, engine, seed=seed, series_offset=series_offset, literal=literal))
    for flags in (out["status"], *st.values()):
        c["status"] = or_status(c["status"], flags)
    return chain(kind, **c)


def chain(kind, *, ys, theta, beta, v, alpha, sv, m0, C0, mat, **rest):
    """The chain state of `sweep` from given arrays, all where the chain lives: ys [N][T][p], theta [N][T+1][d], the factor part's beta,
    v, alpha [N][k][T+1] and sv [N][k][3], the static variance V [N][p p] or W [N][d d] by its name, m0, C0 and the materialised model.
    The buffers a sweep writes -- the stream, "y" (the factor model's data), "f" and the mixture call's "ystar" and "v_mix" -- are
    allocated where they are not given; the default order reads none of them."""
    N, k, T1 = (int(n) for n in alpha.shape)
    q = int(beta.shape[1])
    new = (lambda *shape: theta.new_empty(shape)) if is_torch(theta) else (lambda *shape: np.empty(shape))
    c = dict(rest, ys=ys, theta=theta, beta=beta, v=v, alpha=alpha, sv=sv, m0=m0, C0=C0, mat=mat)
    c.setdefault("status", None)
    for name, shape in ((kind.stream, (N, T1 - 1, q * q)), ("y", (N, T1 - 1, q)), ("f", (N, k, T1 - 1)), ("ystar", (N * k, T1 - 1)),
                        ("v_mix", (N * k, T1 - 1))):
        if c.get(name) is None:
            c[name] = new(*shape)
    return c


def sweep(kind, engine, c, it, priors, prior, *, seed=0, series_offset=0, literal=False, literal_order=False, **options):
    """Iteration `it` of the sampler on the chain state c, updated in place (the steps of dlmfsv.py's and dlmfsvsys.py's docstrings):
    the factor model's data from theta, the factor half (its factor draw in front, or in the reference's place with literal_order), the
    variance stream, theta | y with f integrated out, and the static variance from its InverseGamma `prior`.  priors: pack_priors' pair;
    options: kind.data's.  Returns the status flags of the calls by name, not yet or'ed (fold_status does that)."""
    mat, y = c["mat"], c["ys"]
    T = int(y.shape[1])
    st = kind.data(engine, c, it, seed, series_offset, **options)
    st.update(factor_half(engine, c, c["y"], priors, iteration=it, seed=seed, series_offset=series_offset, literal=literal,
                          factors_last=literal_order))
    var = engine.dlmfsv_variance(c["beta"], c["v"], c["alpha"], out={"V": c[kind.stream]})
    out = engine.ffbs(mat, kind.packed(c, T), y, seed=seed_theta(seed, it + 1), series_offset=series_offset, want_theta=True, want_stats=True,
                      want_filt=False)
    c["theta"] = out["theta"]
    drawn = engine.dinvgamma_step(mat.d, mat.p, out["stats"], prior, prior, iteration=it, seed=seed, series_offset=series_offset)
    c[kind.static] = drawn["VW".index(kind.static)]
    st.update(variance=var["status"], ffbs=out["status"])
    return st


def sample(kind, params_type, fsv_priors, prior, ys, mod, init_p, engine, *, n_iter, seed, series_offset, literal, literal_order, keep_states,
           times, **options):
    """DlmFsv.sample and DlmFsvSystem.sample: the checks, made before the generator is returned.  fsv_priors: pack_priors' five; prior:
    the InverseGamma of the static variance's diagonal."""
    priors = pack_priors(*fsv_priors, literal, also=(kind.static + "_ii", prior))
    if not isinstance(init_p, params_type):
        raise TypeError(f"init_p must be a {params_type.__name__}")
    checked(kind, ys, mod, init_p, times)
    return _run(kind, ys, mod, init_p, engine, priors, prior, n_iter, seed, series_offset, literal, literal_order, keep_states, times, options)


def _run(kind, ys, mod, init_p, engine, priors, prior, n_iter, seed, series_offset, literal, literal_order, keep_states, times, options):
    c = initialise(kind, ys, mod, init_p, engine, seed=seed, series_offset=series_offset, literal=literal, times=times)
    N, k = int(c["f"].shape[0]), int(c["f"].shape[1])
    s = {"V": c["mat"].p, "W": c["mat"].d}[kind.static]
    for it in range(n_iter):
        st = sweep(kind, engine, c, it, priors, prior, seed=seed, series_offset=series_offset, literal=literal, literal_order=literal_order,
                   **options)
        status = fold_status(st, N, k, c["status"] if it == 0 else None)
        params = {"beta": host(c["beta"]).copy(), "v": host(c["v"]).copy(), "sv": host(c["sv"]).copy(),
                  kind.param: np.diagonal(host(c[kind.static]).reshape(N, s, s), axis1=1, axis2=2).copy()}
        yield State(params, *(host(c[key]).copy() if keep_states else None for key in ("theta", "f", "alpha")), status)


# ---- posterior-predictive forecasts ------------------------------------------------------------------------------------
def stack_draws(draws, static=None):
    """The kept draws as stacked host arrays {"beta" [M][N][q][k], "v" [M][N][q], "sv" [M][N][k][3], "alpha" [M][N][k][T+1]} and, with
    `static` (Kind.param), the static variance's diagonal under that name: from a dict of such arrays, or from a list of the samplers'
    States kept with their states (their volatility is the alpha)."""
    names = ("beta", "v", "sv") + (() if static is None else (static,))
    if isinstance(draws, dict):
        missing = [key for key in names + ("alpha",) if key not in draws]
        if missing:
            raise ValueError(f"draws lacks {missing}")
        out = {key: np.asarray(host(draws[key]), dtype=np.float64) for key in names + ("alpha",)}
    else:
        draws = list(draws)
        if not draws:
            raise ValueError("draws is empty")
        if any(s.volatility is None for s in draws):
            raise ValueError("the forecast starts the volatility paths at alpha_T: keep the states with the draws (keep_states / keep_factors)")
        out = {key: np.stack([np.asarray(s.params[key], dtype=np.float64) for s in draws]) for key in names}
        out["alpha"] = np.stack([np.asarray(s.volatility, dtype=np.float64) for s in draws])
    beta, alpha = out["beta"], out["alpha"]
    if beta.ndim != 4 or alpha.ndim != 4:
        raise ValueError(f"beta must be [M][N][q][k] and alpha [M][N][k][T+1], got the shapes {beta.shape} and {alpha.shape}")
    M, N, q, k = beta.shape
    if out["v"].shape != (M, N, q) or out["sv"].shape != (M, N, k, 3) or alpha.shape[:3] != (M, N, k) or alpha.shape[3] < 2:
        raise ValueError(f"v must be [M][N][q] = {(M, N, q)}, sv [M][N][k][3] = {(M, N, k, 3)} and alpha [M][N][k][T+1], got the shapes "
                         f"{out['v'].shape}, {out['sv'].shape} and {alpha.shape}")
    if static is not None and (out[static].ndim != 3 or out[static].shape[:2] != (M, N)):
        raise ValueError(f"{static} must be [M][N][.] (the static variance's diagonal), got the shape {out[static].shape}")
    return out


def check_forecast(horizon, n_paths, prob, probs):
    """The quantile levels of a forecast: [1 - prob, prob] (Dlm.summariseForecast's interval) followed by `probs`."""
    from .engine import EngineError, check_mixture_shape, check_sv_paths_shape
    try:
        check_sv_paths_shape(1, int(horizon), int(n_paths))
        levels = check_mixture_shape(1, 1, 1, 1, [1.0 - float(prob), float(prob)] + [float(x) for x in (() if probs is None else probs)])
    except EngineError as e:
        raise ValueError(str(e)) from None
    return levels


def forecast_bytes(dlm, M, R, H, T, p, d, q, k):
    """What `forecast` sizes its chunks by, in bytes: (what the summary of ONE panel reads -- the stream itself without a DLM, else the (f, Q)
    records --, a (draw, path) row of the horizon: paths, stream, repeated parameters and with a DLM the filter's records and data, a (panel,
    draw) row of the training filter).  The least budget a call needs is the first + R times the second + the third (without a DLM: M R
    times the second)."""
    rec, frec = p + p * p, d + d * d
    row_h = 8 * (H * q * q + k * (H + 1) + q * k + q + ((H + 1) * (frec + rec) + H * p + 2 * frec if dlm else 0))
    row_t = 8 * (T * q * q + (T + 1) * frec + T * p + q * k + q + k * (T + 1) + frec) if dlm else 0
    return 8 * M * R * ((H + 1) * rec if dlm else H * p * p), row_h, row_t


def forecast(kind, mod, ys, draws, horizon, engine, *, m0=None, c0=None, n_paths=64, prob=0.75, probs=None, seed=0, series_offset=0, times=None,
             budget=None):
    """The posterior predictive of the next `horizon` unit steps as the equal-weight Gaussian mixture over the M kept draws x n_paths
    future log-volatility paths.  kind: dlmfsv.KIND, dlmfsvsys.KIND or None (FactorSv: no DLM, mean zero).  Per draw:
    the training filter under the draw's own stream for (m_T, C_T) (the draw's theta integrated out), sv_paths from alpha_T,
    dlmfsv_variance on the paths, the filter on all-NaN data for the (f, Q) records, then ONE summary per panel.  Rows are worked in
    chunks that fit `budget` bytes (default: 60 % of the device's free memory); draw m of panel n draws at the Philox series
    series_offset + n and iteration m, so chunking changes no number.  Returns {"mean" [N][H][p], "cov" [N][H][p][p], "lower", "upper"
    [N][H][p] (the quantiles at 1 - prob and prob), "quantiles" [N][H][p][len(probs)] or None, "status" [N]}."""
    H, R = int(horizon), int(n_paths)
    levels = check_forecast(H, R, prob, probs)
    dr = stack_draws(draws, None if kind is None else kind.param)
    beta, vv, sv, alpha = dr["beta"], dr["v"], dr["sv"], dr["alpha"]
    M, N, q, k = beta.shape
    T = alpha.shape[3] - 1
    if kind is None:
        p = d = q
    else:
        dims = panel_dims(ys)
        if dims[0] != N or dims[1] != T:
            raise ValueError(f"ys is {dims[0]} panels x {dims[1]} times, the draws hold {N} panels and alpha has T + 1 = {T + 1} entries")
        mat = kind.model(mod, T, times)
        grid = np.arange(1, T + 1, dtype=np.float64) if times is None else np.asarray(host(times), dtype=np.float64).reshape(-1)
        fmat = kind.model(mod, H, grid[-1] + np.arange(1, H + 1, dtype=np.float64))
        p, d = mat.p, mat.d
        if dims[2] != p or q != (p if kind.stream == "V" else d) or dr[kind.param].shape[2] != (d if kind.stream == "V" else p):
            raise ValueError(f"ys has {dims[2]} series and the model p = {p}, d = {d}: beta has {q} rows and {kind.param} "
                             f"{dr[kind.param].shape[2]} entries")
        if m0 is None or c0 is None:
            raise ValueError("m0 and c0, the prior of theta_0 the sampler ran with, are required")
        m0 = np.asarray(m0, dtype=np.float64).reshape(-1)
        c0 = np.asarray(c0, dtype=np.float64)
        if m0.shape != (d,) or c0.shape != (d, d):
            raise ValueError(f"the model has d = {d} states: m0 must be [d] and c0 d x d")
    rec, frec, C = p + p * p, d + d * d, M * R
    put, probe = place(np.zeros((1, 1)), engine, 1, 1)
    new = (lambda *shape: probe.new_empty(shape)) if is_torch(probe) else (lambda *shape: np.empty(shape))
    if budget is None:
        budget = int(0.6 * engine.mem_info()[0])
    keep, row_h, row_t = forecast_bytes(kind is not None, M, R, H, T, p, d, q, k)
    if kind is None and M * R * row_h > budget:
        raise MemoryError(f"the variance stream of one panel ({M} draws x {R} paths x {H} steps x {p} x {p} doubles, {keep / 1e9:.2f} GB) "
                          f"does not fit the budget of {budget / 1e9:.2f} GB: forecast fewer draws or paths")
    if keep + R * row_h + row_t > budget:
        raise MemoryError(f"the forecast records of one panel ({keep / 1e9:.2f} GB) and one draw's streams do not fit the budget of "
                          f"{budget / 1e9:.2f} GB: forecast fewer draws or paths")
    nc = max(1, min(N, budget // (keep + M * R * row_h if kind is None else 2 * keep)))           # panels per summary call
    out = {"mean": np.empty((N, H, p)), "cov": np.empty((N, H, p, p)), "quant": np.empty((N, H, p, len(levels))), "status": np.zeros(N, np.int32)}

    def note(n0, n1, flags, fold):
        """or the flags [rows] of a call on the panels n0 .. n1 - 1, `fold` rows per panel, onto the panels"""
        if flags is not None:
            out["status"][n0:n1] |= np.bitwise_or.reduce(host(flags).astype(np.int32).reshape(n1 - n0, fold), axis=1)

    for n0 in range(0, N, nc):
        n1 = min(N, n0 + nc)
        L = n1 - n0
        so = series_offset + n0
        if kind is None:
            mc = M                                                                   # the summary reads the stream itself: all draws at once
        else:
            left = max(budget - L * keep, L * (R * row_h + row_t))
            mc = max(1, min(M, left // (L * (R * row_h + row_t))))
            fq_all = new(L, M, R, H + 1, rec)
        for a0 in range(0, M, mc):
            a1 = min(M, a0 + mc)
            A = a1 - a0
            tr = lambda x: np.ascontiguousarray(np.moveaxis(x[a0:a1, n0:n1], 0, 1))          # [A][L][..] of the draws -> [L][A][..]
            b_, v_, sv_, al_ = tr(beta), tr(vv), tr(sv), tr(alpha)
            if kind is not None:
                # 1 the training filter per (panel, draw): the last record is (m_T, C_T)
                st_ = tr(dr[kind.param])
                s = st_.shape[2]
                static = np.zeros((L * A, s, s))
                static[:, np.arange(s), np.arange(s)] = st_.reshape(L * A, s)
                static = put(static.reshape(L * A, s * s))
                var = engine.dlmfsv_variance(put(b_.reshape(L * A, q, k)), put(v_.reshape(L * A, q)), put(al_.reshape(L * A, k, T + 1)))
                yrep = put(np.repeat(np.asarray(host(ys), dtype=np.float64)[n0:n1], A, axis=0))
                m0d, c0d = put(m0), put(np.ascontiguousarray(c0.T).reshape(-1))
                par = ((var["V"].reshape(-1), T * p * p, static.reshape(-1), d * d, m0d, 0, c0d, 0, p * p, 0) if kind.stream == "V" else
                       (static.reshape(-1), p * p, var["V"].reshape(-1), T * d * d, m0d, 0, c0d, 0, 0, d * d))
                tf = engine.filter(mat, par, yrep)
                last = tf["filt"].reshape(L * A, T + 1, frec)[:, T]
                note(n0, n1, var["status"], A); note(n0, n1, tf["status"], A)
                del var, yrep
                rep = lambda x: x.repeat_interleave(R, dim=0) if is_torch(x) else np.repeat(x, R, axis=0)
                mT, CT, static_r = rep(last[:, :d]), rep(last[:, d:]), rep(static)
                del tf
            # 2 the paths from alpha_T: one call per draw (the draw is the Philox iteration), panel n the series series_offset + n
            # (parameters and starts go up once, draw-major, and every call writes its own slice of one buffer)
            sv_d, start_d = put(np.moveaxis(sv_, 0, 1)), put(np.moveaxis(al_[..., T], 0, 1))          # [A][L][k][3], [A][L][k]
            paths = new(A, L, R, k, H + 1)
            for a in range(A):
                pa = engine.sv_paths(sv_d[a], H, R, alpha0=start_d[a], iteration=a0 + a, seed=seed, series_offset=so, out={"alpha": paths[a]})
                note(n0, n1, pa["status"], 1)
            if L > 1:                                                                                 # rows are (panel, draw, path)
                paths = paths.transpose(0, 1).contiguous() if is_torch(paths) else np.ascontiguousarray(np.swapaxes(paths, 0, 1))
            # 3 the stream, beta and v repeated over the paths
            rows = L * A * R
            var = engine.dlmfsv_variance(put(np.repeat(b_.reshape(L * A, q, k), R, axis=0)), put(np.repeat(v_.reshape(L * A, q), R, axis=0)),
                                         paths.reshape(rows, k, H + 1))
            note(n0, n1, var["status"], A * R)
            del paths
            if kind is None:
                stream = var["V"]
                continue
            # 4 the Kalman forecast from (m_T, C_T) under the stream: the filter on all-NaN data, its (f, Q) records
            nan = new(rows, H, p)
            nan[...] = np.nan
            par = ((var["V"].reshape(-1), H * p * p, static_r.reshape(-1), d * d, mT.reshape(-1), d, CT.reshape(-1), d * d, p * p, 0) if kind.stream == "V"
                   else (static_r.reshape(-1), p * p, var["V"].reshape(-1), H * d * d, mT.reshape(-1), d, CT.reshape(-1), d * d, 0, d * d))
            ff = engine.filter(fmat, par, nan, want_fq=True)
            note(n0, n1, ff["status"], A * R)
            fq_all[:, a0:a1] = ff["fq"].reshape(L, A, R, H + 1, rec)
            del var, ff, nan
        # 5 one summary per panel over all M R components, read in place
        sm = (engine.gaussian_mixture_summary(L, C, H, p, Q=stream, probs=levels) if kind is None else
              engine.gaussian_mixture_summary(L, C, H, p, fq=fq_all, probs=levels))
        out["mean"][n0:n1] = host(sm["mean"])
        out["cov"][n0:n1] = host(sm["cov"]).reshape(L, H, p, p)
        out["quant"][n0:n1] = host(sm["quant"])
        note(n0, n1, sm["status"], 1)
    quant = out.pop("quant")
    out.update(lower=quant[..., 0].copy(), upper=quant[..., 1].copy(), quantiles=quant[..., 2:].copy() if probs is not None else None)
    return out
