"""The inputs of the particle-Gibbs tests, made from seeds: the table of shapes dlm_pg_batch is held to its restatement on
(tests/test_pg_gpu.py; tests/test_pg_host.py checks the margins of the same table on the restatement alone), and how a set of inputs
reaches the restatement and the engine.  Every entry is the smallest shape at which its part of the kernel can go wrong:

  P   64 one slot of particles, 128 a carry between two slots (the reference particle sits in the LAST slot);
  d   1, 2, 3, 8 (the last D with two waves per SIMD) and the limit 16, with a dense G and a full W (the forward substitution of the
      ancestor-sampling density runs over a full factor);
  T   1, 4, 6 and 12;  y_0 and y_{T-1} missing;  an irregular grid with three distinct G through g_index and a dt = 0 first and inside
      the series, and regular grids whose first step does advance;
  N   2 .. 6;  shared and per-series parameters;  the six families;  ancestor sampling on and off.

The reference path of an entry is the state path its data were simulated from."""
import functools

import numpy as np

import pf_cases as pc
import pf_restatement as pr
import pg_restatement as gr
from bayesian_dlms_amd.dglm import Dglm


def case(name, d, P, T, N, family=pr.GAUSSIAN, missing=(), irregular=False, per_series=False, ancestor_sampling=True, dt0=1.0, seed=1):
    return dict(name=name, d=d, P=P, T=T, N=N, family=family, missing=tuple(missing), irregular=irregular, per_series=per_series,
                ancestor_sampling=ancestor_sampling, dt0=dt0, seed=seed)


TABLE = [
    case("d1-p64", 1, 64, 12, 5),
    case("d2-p128-missing-per-series", 2, 128, 12, 5, missing=(0, 11), per_series=True),
    case("d3-p128-irregular", 3, 128, 12, 5, irregular=True),
    case("d8-p64", 8, 64, 6, 3),
    case("d16-p64", 16, 64, 4, 2),
    case("d16-p128-irregular-per-series", 16, 128, 6, 2, irregular=True, per_series=True),
    case("t1-first-dt0", 2, 128, 1, 5, dt0=0.0),
    case("plain-d2-irregular", 2, 64, 12, 6, irregular=True, ancestor_sampling=False),
    case("plain-d3-missing-per-series", 3, 128, 12, 4, missing=(0, 11), per_series=True, ancestor_sampling=False),
] + [case("family-" + pc.FAMILY_NAMES[f], 2, 128 if f % 2 else 64, 12, 5, family=f, irregular=f in (1, 4), per_series=f in (2, 4, 5),
          missing=(11,) if f == 3 else ()) for f in range(6)]


def by_name(name):
    return next(c for c in TABLE if c["name"] == name)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The arrays of a table entry: what the restatement's `run` takes, and through `engine_run` the engine."""
    c = by_name(name)
    rng = np.random.default_rng(2800 + c["seed"] * 7919 + sum(map(ord, name)))
    d, T, N, fam = c["d"], c["T"], c["N"], c["family"]
    G0, W, F = pc.dense_model(d, rng)
    G, gi, dt = pc.time_grid(c, G0, c["dt0"])
    shift = np.zeros(d); shift[0] = pc.FAMILY_LEVEL[fam] / F[0]
    m0 = rng.standard_normal(d) * 0.3
    C0 = 0.5 * W + 0.2 * np.eye(d)
    V = pc.FAMILY_V[fam]
    if c["per_series"]:
        scale = np.exp(0.3 * rng.standard_normal(N))
        Wn, C0n = W[None] * scale[:, None, None], C0[None] * scale[::-1, None, None]
        m0n = m0[None] + 0.2 * rng.standard_normal((N, d))
        Vn = V * np.exp(0.2 * rng.standard_normal(N)) if fam in (pr.GAUSSIAN, pr.STUDENTT) else np.full(N, V)
    else:
        Wn, C0n, m0n, Vn = W, C0, m0, V
    mod = Dglm(lambda t: F[:, None], lambda s: G0, fam, 5.0 if fam == pr.STUDENTT else None)
    y, ref = np.empty((N, T)), np.empty((N, T + 1, d))
    for n in range(N):
        Wk = Wn[n] if c["per_series"] else W
        x = (m0n[n] if c["per_series"] else m0) + shift + np.linalg.cholesky(C0n[n] if c["per_series"] else C0) @ rng.standard_normal(d)
        ref[n, 0] = x
        for t in range(T):
            if dt[t] != 0.0:
                x = G[0 if gi is None else gi[t]] @ x + np.sqrt(dt[t]) * (np.linalg.cholesky(Wk) @ rng.standard_normal(d))
            ref[n, t + 1] = x
            y[n, t] = mod.observation(float(F @ x), float(Vn[n] if c["per_series"] else V), rng)
    for t in c["missing"]:
        y[:, t] = np.nan
    nu = 5.0 + np.arange(N) if fam == pr.STUDENTT else None
    return dict(F=F, G=G, g_index=gi, dt=dt, V=Vn, W=Wn, m0=m0n + shift, C0=C0n, y=y, ref=ref, nu=nu)


def run_args(name, **over):
    c, a = by_name(name), inputs(name)
    kw = dict(a, family=c["family"], P=c["P"], ancestor_sampling=c["ancestor_sampling"], seed=40 + c["seed"], series_offset=3, iteration=5)
    kw.update(over)
    return kw


@functools.lru_cache(maxsize=None)
def reference(name):
    return gr.run(**run_args(name))


TRACES = dict(want_path_index=True, want_trace=True, want_step_weights=True)


def engine_run(eng, kw, device=False, traces=True, **over):
    """Engine.pg_sweep on the arguments the restatement's `run` takes -> NumPy arrays (every trace unless traces=False)."""
    import torch
    N = kw["y"].shape[0]
    put = (lambda a: torch.as_tensor(np.array(a), device="cuda")) if device else (lambda a: a)          # (a copy: the cached inputs are read-only)
    want = dict(TRACES if traces else {}, **over)
    out = eng.pg_sweep(pc.materialised(kw), pc.packed_params(kw, N), put(kw["y"]), put(kw["ref"]), family=kw["family"], n_particles=kw["P"],
                       ancestor_sampling=kw["ancestor_sampling"], obs_param=kw.get("nu"), iteration=kw["iteration"], seed=kw["seed"],
                       series_offset=kw["series_offset"], **want)
    return {k: None if v is None else (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in out.items()}


def path_stats(kw, path):
    """[ssy | n | ss (d) | T] of a path [N][T+1][d] in plain NumPy: what `stats` must equal"""
    y, F, G = np.asarray(kw["y"]), np.asarray(kw["F"], dtype=np.float64), np.asarray(kw["G"], dtype=np.float64)
    N, T = y.shape
    d = G.shape[1]
    dt = np.ones(T) if kw["dt"] is None else np.asarray(kw["dt"], dtype=np.float64)
    gi = np.zeros(T, dtype=int) if kw["g_index"] is None else np.asarray(kw["g_index"])
    Ft = np.broadcast_to(F, (T, d)) if F.ndim == 1 else F
    diff = path[:, 1:] - np.einsum("tij,ntj->nti", G[gi], path[:, :-1])
    adv = dt != 0.0
    ss = (diff[:, adv] ** 2 / dt[adv][None, :, None]).sum(axis=1)
    if kw["family"] == pr.GAUSSIAN:
        res = y - np.einsum("td,ntd->nt", Ft, path[:, 1:])
        seen = ~np.isnan(y)
        ssy, n = np.where(seen, np.nan_to_num(res) ** 2, 0.0).sum(axis=1), seen.sum(axis=1).astype(np.float64)
    else:
        ssy, n = np.zeros(N), np.zeros(N)
    return np.concatenate([ssy[:, None], n[:, None], ss, np.full((N, 1), float(T))], axis=1)
