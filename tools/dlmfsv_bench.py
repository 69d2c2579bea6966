"""Gibbs sampler of the DLM with factor stochastic-volatility noise at 512 panels of p = 20 series, k = 3 factors and 1000 times; the DLM
is p local levels under |*| (d = 20: dlm_ffbs_batch takes its per-wave kernels), simulated at W = 0.05 I, free loadings 0.5,
sigma^2 = 0.25 and (phi, mu, sigma_eta) = (0.8, 0, 0.3) for every factor, --missing of the single components then set missing
(default 0.02: a third of the times are partially missing at p = 20).  One iteration is the steps of
bayesian_dlms_amd/dlmfsv.py in the default order -- the driver's own sweep, run on a timing wrapper of the engine (tools/timed_engine.py);
everything stays in HBM.  Prints one JSON line: ms per iteration (the sum of the calls' wall times) and the wall time of each synchronous call
(median over --iters iterations after --warmup), and for the centring and the variance call their algorithmic bytes over their wall
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

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayesian_dlms_amd import _dlmfsv  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters  # noqa: E402
from bayesian_dlms_amd.dlmfsv import KIND, DlmFsv, DlmFsvParameters  # noqa: E402
from bayesian_dlms_amd.engine import Engine  # noqa: E402
from bayesian_dlms_amd.factorsv import FactorSv, FsvParameters, pack_priors  # noqa: E402
from bayesian_dlms_amd.gibbs import InverseGamma  # noqa: E402
from bayesian_dlms_amd.stochvol import Gaussian, SvParameters  # noqa: E402
from timed_engine import time_fill, time_sweeps  # noqa: E402

STEPS = ("center", "impute", "factors", "mixture", "ar1_ffbs", "sv_params", "loadings", "variance", "ffbs", "w")
# the engine's methods behind them, in the order of the driver's sweep
METHODS = ("dlmfsv_center", "dlmfsv_impute", "fsv_factors", "sv_mixture", "ar1_ffbs", "sv_params", "fsv_loadings", "dlmfsv_variance", "ffbs",
           "dinvgamma_step")


def run(eng, ys, mod, init, iters, warmup):
    c = DlmFsv.initialise_state(ys, mod, init, eng, seed=1)
    N, T, p = (int(x) for x in c["ys"].shape)
    k, d = init.fsv.k, c["mat"].d
    priors = pack_priors(Gaussian(0.0, 1.0), InverseGamma(3.0, 0.3), Gaussian(0.0, 1.0), Gaussian(0.8, 0.1), InverseGamma(3.0, 1.0), False)
    sweep = lambda timed, it: _dlmfsv.sweep(KIND, timed, c, it, priors, InverseGamma(3.0, 0.5), seed=1)
    med, variant, status = time_sweeps(eng, sweep, METHODS, iters, warmup)
    beta, v, W, V = c["beta"], c["v"], c["W"], c["V"]
    res = {"ms_per_iter": round(float(med[0]), 3), "ffbs_variant": variant}
    res.update({name + "_ms": round(float(x), 3) for name, x in zip(STEPS, med[1:])})
    nbytes = {"center": 16 * N * T * p + 8 * N * (T + 1) * d + 8 * d * p, "variance": 8 * N * T * p * p + 8 * N * k * (T + 1) + 8 * N * p * (k + 1)}
    for name in ("center", "variance"):
        res[name + "_bytes"] = nbytes[name]
        res[name + "_gbs"] = round(nbytes[name] / (res[name + "_ms"] * 1e-3) / 1e9, 1)
    # the same bytes written by dlm_buffer_fill into the V stream's buffer
    fill_ms = time_fill(eng, V, 8 * N * T * p * p, iters, warmup)
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
