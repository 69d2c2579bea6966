"""Factor stochastic-volatility Gibbs at 512 panels of p = 20 series, k = 3 factors and 1000 times, simulated at free loadings 0.5,
sigma^2 = 0.25 and (phi, mu, sigma_eta) = (0.8, 0, 0.3) for every factor.  One iteration = dlm_sv_mixture_batch, dlm_ar1_ffbs_batch,
dlm_sv_params_batch on the N k factor series, then dlm_fsv_factors_batch and dlm_fsv_loadings_batch -- the driver's own
factorsv.factor_half, run on a timing wrapper of the engine (tools/timed_engine.py); everything stays in HBM.
Prints one JSON line per arithmetic (default, literal): ms per iteration (the sum of the calls' wall times; median over --iters iterations
after --warmup), the wall time of each of the five synchronous calls, and for the two new calls their algorithmic bytes over their wall time, as a rate and
as a share of the 8 TB/s nominal HBM peak DESIGN.md 4.5 prices against (a plain device copy reaches 4.6-5.3 TB/s there):
  factors   reads y (8 N T p), alpha (8 N k (T + 1)), beta and v; writes f (8 N k T)
  loadings  reads y (8 N T p), f (8 N k T), beta; writes beta and v

    python tools/fsv_bench.py [--n 512] [--t 1000] [--p 20] [--k 3] [--iters 10] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayesian_dlms_amd.engine import Engine  # noqa: E402
from bayesian_dlms_amd.factorsv import FactorSv, FsvParameters, factor_half, pack_priors  # noqa: E402
from bayesian_dlms_amd.gibbs import InverseGamma  # noqa: E402
from bayesian_dlms_amd.stochvol import Gaussian, SvParameters  # noqa: E402
from timed_engine import time_sweeps  # noqa: E402

HBM_NOMINAL = 8.0e12
METHODS = ("sv_mixture", "ar1_ffbs", "sv_params", "fsv_factors", "fsv_loadings")          # sampleStep's order


def call_bytes(N, T, p, k):
    small = 8 * N * p * k + 8 * N * p
    return {"factors": 8 * N * T * p + 8 * N * k * (T + 1) + small + 8 * N * k * T,
            "loadings": 8 * N * T * p + 8 * N * k * T + 8 * N * p * k + small}


def run(eng, y, init, iters, warmup, literal):
    N, T, p = (int(x) for x in y.shape)
    k = init.k
    c = FactorSv.initialise_state_ar(y, init, eng, seed=1, literal=literal)
    priors = pack_priors(Gaussian(0.0, 1.0), InverseGamma(3.0, 0.3), Gaussian(0.0, 1.0), Gaussian(0.8, 0.1), InverseGamma(3.0, 1.0), literal)
    sweep = lambda timed, it: factor_half(timed, c, c["y"], priors, iteration=it, seed=1, series_offset=0, literal=literal, factors_last=True)
    r, _, status = time_sweeps(eng, sweep, METHODS, iters, warmup)
    beta, v = c["beta"], c["v"]
    nb = call_bytes(N, T, p, k)
    out = {"arithmetic": "literal" if literal else "default", "ms_per_iter": round(float(r[0]), 3), "mixture_ms": round(float(r[1]), 3),
           "ffbs_ms": round(float(r[2]), 3), "params_ms": round(float(r[3]), 3), "factors_ms": round(float(r[4]), 3),
           "loadings_ms": round(float(r[5]), 3)}
    for name, ms in (("factors", r[4]), ("loadings", r[5])):
        rate = nb[name] / (ms * 1e-3)
        out[name + "_bytes"] = nb[name]
        out[name + "_gbs"] = round(rate / 1e9, 1)
        out[name + "_frac_of_hbm_nominal"] = round(rate / HBM_NOMINAL, 4)
    out["last_draw_mean"] = {"free_beta": round(float(beta.cpu().numpy()[:, np.tril(np.ones((p, k), bool), -1)].mean()), 3),
                             "sigma2": round(float(v.mean().item()), 3)}
    out["status_or"] = status
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--t", type=int, default=1000)
    ap.add_argument("--p", type=int, default=20)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    truth = FsvParameters(0.25, FactorSv.build_beta(a.p, a.k, 0.5), [SvParameters(0.8, 0.0, 0.3)] * a.k)
    y_h, _, _ = FactorSv.simulate(truth, a.t, a.n, seed=1)
    init = FsvParameters(1.0, FactorSv.make_beta(a.p, a.k), [SvParameters(0.8, 0.0, 0.3)] * a.k)
    eng = Engine(0)
    y = torch.as_tensor(y_h, device="cuda:0")
    for literal in (False, True):
        out = {"shape": {"N": a.n, "T": a.t, "p": a.p, "k": a.k}, "iters": a.iters, "warmup": a.warmup}
        out.update(run(eng, y, init, a.iters, a.warmup, literal))
        print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
