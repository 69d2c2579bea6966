"""What the two Gibbs samplers of a DLM with a factor stochastic-volatility part share (dlmfsv.py: the part is the observation noise;
dlmfsvsys.py: it is the system noise): the State, the checks, the initialisation, one sweep and the generator around it.

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
