"""Gibbs sampler of the DLM with factor stochastic-volatility noise at 512 panels of p = 20 series, k = 3 factors and 1000 times; the DLM
is p local levels under |*| (d = 20: dlm_ffbs_batch takes its per-wave kernels), simulated at W = 0.05 I, free loadings 0.5,
sigma^2 = 0.25 and (phi, mu, sigma_eta) = (0.8, 0, 0.3) for every factor, --missing of the single components then set missing
(default 0.02: a third of the times are partially missing at p = 20).  One iteration is the steps of
bayesian_dlms_amd/dlmfsv.py in the default order; everything stays in HBM.  Prints one JSON line: ms per iteration and the wall time of
each synchronous call (median over --iters iterations after --warmup), and for the centring and the variance call their algorithmic bytes over their wall
time as a rate:
  center    reads y (8 N T p), theta (8 N (T + 1) d), F; writes r (8 N T p)
  impute    reads r (8 N T p), alpha, beta, v; writes the missing components of the partially missing times
  variance  reads beta, v, alpha (8 N k (T + 1)); writes V (8 N T p^2)
beside a dlm_buffer_fill of the V stream's bytes on the same box (what plain device writes reach there).  DLM_ENGINE_LIB selects another
build of the library, e.g. the one with -DDLM_DLMFSV_NT_STORES=1 (bayesian_dlms_amd.build.build_tu_variant).

    python tools/dlmfsv_bench.py [--n 512] [--t 1000] [--p 20] [--k 3] [--missing 0.02] [--iters 30] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayesian_dlms_amd.dlm import Dlm, DlmParameters  # noqa: E402
from bayesian_dlms_amd.dlmfsv import DlmFsv, DlmFsvParameters  # noqa: E402
from bayesian_dlms_amd.engine import Engine  # noqa: E402
from bayesian_dlms_amd.factorsv import FactorSv, FsvParameters  # noqa: E402
from bayesian_dlms_amd.stochvol import MASK64, SvParameters  # noqa: E402

STEPS = ("center", "impute", "factors", "mixture", "ar1_ffbs", "sv_params", "loadings", "variance", "ffbs", "w")


def run(eng, ys, mod, init, iters, warmup):
    import torch
    c = DlmFsv.initialise_state(ys, mod, init, eng, seed=1)
    mat, y, theta, W, m0, C0, V = c["mat"], c["ys"], c["theta"], c["W"], c["m0"], c["C0"], c["V"]
    r, f, alpha, beta, v = c["y"], c["f"], c["alpha"], c["beta"], c["v"]
    N, T, p = (int(x) for x in y.shape)
    k, d = init.fsv.k, mat.d
    sv = c["sv"].reshape(N * k, 3)
    bufs = {"ystar": c["ystar"], "v": c["v_mix"]}
    sv_prior = (0, 0, 0.8, 0.1, 0.0, 1.0, 3.0, 0.3, 100.0, 0.05)
    fsv_prior = (0, 0.0, 1.0, 3.0, 1.0)
    prior_w = (3.0, 0.5)
    rows, status = [], 0
    for it in range(warmup + iters):
        torch.cuda.synchronize()
        t = [time.perf_counter()]
        cen = eng.dlmfsv_center(mat, y, theta, out={"r": r}); t.append(time.perf_counter())
        imp = eng.dlmfsv_impute(r, beta, v, alpha, iteration=it, seed=1, out={"r": r}); t.append(time.perf_counter())
        fac = eng.fsv_factors(r, beta, v, alpha, iteration=it, seed=1, out={"f": f}); t.append(time.perf_counter())
        mix = eng.sv_mixture(f.reshape(N * k, T), alpha.reshape(N * k, T + 1), iteration=it, seed=1, out=bufs); t.append(time.perf_counter())
        ff = eng.ar1_ffbs(mix["ystar"], mix["v"], sv, seed=1000004 + it, want_filt=False); t.append(time.perf_counter())
        alpha = ff["theta"].reshape(N, k, T + 1)
        res = eng.sv_params(ff["theta"], sv, sv_prior, iteration=it, seed=1, out={"sv": sv}); t.append(time.perf_counter())
        ld = eng.fsv_loadings(r, f, beta, fsv_prior, iteration=it, seed=1, v=v, out={"beta": beta, "v": v}); t.append(time.perf_counter())
        var = eng.dlmfsv_variance(beta, v, alpha, out={"V": V}); t.append(time.perf_counter())
        out = eng.ffbs(mat, DlmFsv._packed(V, T, p, W, d, m0, C0), y, seed=((1000003 + it + 1) ^ (1 << 63)) & MASK64, want_theta=True,
                       want_stats=True, want_filt=False); t.append(time.perf_counter())
        variant = eng.last_variant
        theta = out["theta"]
        W = eng.dinvgamma_step(d, p, out["stats"], prior_w, prior_w, iteration=it, seed=1)[1]; t.append(time.perf_counter())
        for st in (cen, imp, fac, mix, ff, res, ld, var, out):
            status |= int(st["status"].max().item())
        if it >= warmup:
            rows.append([t[-1] - t[0]] + [b - a for a, b in zip(t[:-1], t[1:])])
    med = np.median(np.array(rows) * 1e3, axis=0)
    res = {"ms_per_iter": round(float(med[0]), 3), "ffbs_variant": variant}
    res.update({name + "_ms": round(float(x), 3) for name, x in zip(STEPS, med[1:])})
    nbytes = {"center": 16 * N * T * p + 8 * N * (T + 1) * d + 8 * d * p, "variance": 8 * N * T * p * p + 8 * N * k * (T + 1) + 8 * N * p * (k + 1)}
    for name in ("center", "variance"):
        res[name + "_bytes"] = nbytes[name]
        res[name + "_gbs"] = round(nbytes[name] / (res[name + "_ms"] * 1e-3) / 1e9, 1)
    # the same bytes written by dlm_buffer_fill into the V stream's buffer
    fills = []
    for _ in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng._check(eng.lib.dlm_buffer_fill(eng.h, V.data_ptr(), 0, 0, 8 * N * T * p * p))
        eng.sync()
        fills.append(time.perf_counter() - t0)
    fill_ms = float(np.median(fills[warmup:]) * 1e3)
    res["fill_v_bytes"], res["fill_v_ms"], res["fill_v_gbs"] = 8 * N * T * p * p, round(fill_ms, 3), round(8 * N * T * p * p / (fill_ms * 1e-3) / 1e9, 1)
    res["variance_write_gbs"] = round(8 * N * T * p * p / (res["variance_ms"] * 1e-3) / 1e9, 1)
    res["last_draw_mean"] = {"free_beta": round(float(beta.cpu().numpy()[:, np.tril(np.ones((p, k), bool), -1)].mean()), 3),
                             "sigma2": round(float(v.mean().item()), 3),
                             "w": round(float(np.diagonal(W.cpu().numpy().reshape(N, d, d), axis1=1, axis2=2).mean()), 4)}
    res["status_or"] = status
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--t", type=int, default=1000)
    ap.add_argument("--p", type=int, default=20)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--missing", type=float, default=0.02)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    mod = Dlm.polynomial(1)
    for _ in range(a.p - 1):
        mod = mod * Dlm.polynomial(1)
    sv = [SvParameters(0.8, 0.0, 0.3)] * a.k
    truth = DlmFsvParameters(DlmParameters(np.eye(a.p), 0.05 * np.eye(a.p), np.zeros(a.p), np.eye(a.p)),
                             FsvParameters(0.25, FactorSv.build_beta(a.p, a.k, 0.5), sv))
    y_h = DlmFsv.simulate(mod, truth, a.t, a.n, seed=1)[0]
    y_h[np.random.default_rng(2).random(y_h.shape) < a.missing] = np.nan
    init = DlmFsvParameters(DlmParameters(np.eye(a.p), np.eye(a.p), np.zeros(a.p), np.eye(a.p)), FsvParameters(1.0, FactorSv.make_beta(a.p, a.k), sv))
    eng = Engine(0)
    out = {"shape": {"N": a.n, "T": a.t, "p": a.p, "k": a.k, "d": a.p}, "iters": a.iters, "warmup": a.warmup, "missing": a.missing,
           "lib": os.path.basename(os.environ.get("DLM_ENGINE_LIB") or "libdlm_engine.so")}
    out.update(run(eng, torch.as_tensor(y_h, device="cuda:0"), mod, init, a.iters, a.warmup))
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
