"""Gibbs sampler of the DLM with factor stochastic-volatility SYSTEM noise at 512 panels of d = 20 states, k = 3 factors and 1000 times; the
DLM is 20 local levels under |*| (p = 20, d = 20), simulated at V = 0.25 I, free loadings 0.5, sigma^2 = 0.05 and
(phi, mu, sigma_eta) = (0.8, -1, 0.3) for every factor, --missing of the single components of y then set missing (default 0.02).  One
iteration is the steps of bayesian_dlms_amd/dlmfsvsys.py in the default order -- the driver's own sweep, run on a timing wrapper of the engine
(tools/timed_engine.py); everything stays in HBM.  Prints one JSON line: ms per iteration (the sum of the calls' wall times) and the wall
time of each synchronous call (median over --iters iterations after --warmup), the fraction of the iteration that is
the state draw, and for the innovations and the variance call their algorithmic bytes over their wall time as a rate:
  innovations  reads theta (8 N (T + 1) d) and G; writes w (8 N T d): 16 bytes per element
  variance     reads beta, v, alpha (8 N k (T + 1)); writes W (8 N T d^2)
beside a dlm_buffer_fill of the W stream's bytes on the same box (what plain device writes reach there).  Run it under a time limit of
its own, e.g.

    timeout -k 10 600 python tools/dlmfsvsys_bench.py [--n 512] [--t 1000] [--d 20] [--k 3] [--missing 0.02] [--iters 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayesian_dlms_amd import _dlmfsv  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters  # noqa: E402
from bayesian_dlms_amd.dlmfsvsys import KIND, DlmFsvSystem, DlmFsvSystemParameters  # noqa: E402
from bayesian_dlms_amd.engine import Engine  # noqa: E402
from bayesian_dlms_amd.factorsv import FactorSv, FsvParameters, pack_priors  # noqa: E402
from bayesian_dlms_amd.gibbs import InverseGamma  # noqa: E402
from bayesian_dlms_amd.stochvol import Gaussian, SvParameters  # noqa: E402
from timed_engine import time_fill, time_sweeps  # noqa: E402

STEPS = ("innovations", "factors", "mixture", "ar1_ffbs", "sv_params", "loadings", "variance", "ffbs", "v")
# the engine's methods behind them, in the order of the driver's sweep
METHODS = ("dlmfsvsys_innovations", "fsv_factors", "sv_mixture", "ar1_ffbs", "sv_params", "fsv_loadings", "dlmfsv_variance", "ffbs", "dinvgamma_step")


def run(eng, ys, mod, init, iters, warmup):
    c = DlmFsvSystem.initialise_state(ys, mod, init, eng, seed=1)
    N, T, p = (int(x) for x in c["ys"].shape)
    k, d = init.fsv.k, c["mat"].d
    priors = pack_priors(Gaussian(0.0, 1.0), InverseGamma(3.0, 0.3), Gaussian(0.0, 1.0), Gaussian(0.8, 0.1), InverseGamma(3.0, 1.0), False)
    sweep = lambda timed, it: _dlmfsv.sweep(KIND, timed, c, it, priors, InverseGamma(3.0, 0.5), seed=1)
    med, variant, status = time_sweeps(eng, sweep, METHODS, iters, warmup)
    beta, v, V, W = c["beta"], c["v"], c["V"], c["W"]
    res = {"ms_per_iter": round(float(med[0]), 3), "ffbs_variant": variant}
    res.update({name + "_ms": round(float(x), 3) for name, x in zip(STEPS, med[1:])})
    res["ffbs_fraction"] = round(res["ffbs_ms"] / res["ms_per_iter"], 4)
    nbytes = {"innovations": 8 * N * (T + 1) * d + 8 * N * T * d + 8 * d * d, "variance": 8 * N * T * d * d + 8 * N * k * (T + 1) + 8 * N * d * (k + 1)}
    for name in ("innovations", "variance"):
        res[name + "_bytes"] = nbytes[name]
        res[name + "_gbs"] = round(nbytes[name] / (res[name + "_ms"] * 1e-3) / 1e9, 1)
    # the same bytes written by dlm_buffer_fill into the W stream's buffer
    fill_ms = time_fill(eng, W, 8 * N * T * d * d, iters, warmup)
    res["fill_w_bytes"], res["fill_w_ms"], res["fill_w_gbs"] = 8 * N * T * d * d, round(fill_ms, 3), round(8 * N * T * d * d / (fill_ms * 1e-3) / 1e9, 1)
    res["last_draw_mean"] = {"free_beta": round(float(beta.cpu().numpy()[:, np.tril(np.ones((d, k), bool), -1)].mean()), 3),
                             "sigma2": round(float(v.mean().item()), 3),
                             "V": round(float(np.diagonal(V.cpu().numpy().reshape(N, p, p), axis1=1, axis2=2).mean()), 4)}
    res["status_or"] = status
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--t", type=int, default=1000)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--missing", type=float, default=0.02)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    mod = Dlm.polynomial(1)
    for _ in range(a.d - 1):
        mod = mod * Dlm.polynomial(1)
    sv = [SvParameters(0.8, -1.0, 0.3)] * a.k
    dlm = lambda v: DlmParameters(v * np.eye(a.d), np.eye(a.d), np.zeros(a.d), np.eye(a.d))
    truth = DlmFsvSystemParameters(dlm(0.25), FsvParameters(0.05, FactorSv.build_beta(a.d, a.k, 0.5), sv))
    y_h = DlmFsvSystem.simulate(mod, truth, a.t, a.n, seed=1)[0]
    y_h[np.random.default_rng(2).random(y_h.shape) < a.missing] = np.nan
    init = DlmFsvSystemParameters(dlm(1.0), FsvParameters(0.1, FactorSv.make_beta(a.d, a.k), sv))
    eng = Engine(0)
    out = {"shape": {"N": a.n, "T": a.t, "p": a.d, "k": a.k, "d": a.d}, "iters": a.iters, "warmup": a.warmup, "missing": a.missing,
           "lib": os.path.basename(os.environ.get("DLM_ENGINE_LIB") or "libdlm_engine.so")}
    out.update(run(eng, torch.as_tensor(y_h, device="cuda:0"), mod, init, a.iters, a.warmup))
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
