"""Factor stochastic-volatility Gibbs at 512 panels of p = 20 series, k = 3 factors and 1000 times, simulated at free loadings 0.5,
sigma^2 = 0.25 and (phi, mu, sigma_eta) = (0.8, 0, 0.3) for every factor.  One iteration = dlm_sv_mixture_batch, dlm_ar1_ffbs_batch,
dlm_sv_params_batch on the N k factor series, then dlm_fsv_factors_batch and dlm_fsv_loadings_batch; everything stays in HBM.
Prints one JSON line per arithmetic (default, literal): ms per iteration (median over --iters iterations after --warmup), the wall
time of each of the five synchronous calls, and for the two new calls their algorithmic bytes over their wall time, as a rate and
as a share of the 8 TB/s nominal HBM peak DESIGN.md 4.5 prices against (a plain device copy reaches 4.6-5.3 TB/s there):
  factors   reads y (8 N T p), alpha (8 N k (T + 1)), beta and v; writes f (8 N k T)
  loadings  reads y (8 N T p), f (8 N k T), beta; writes beta and v

    python tools/fsv_bench.py [--n 512] [--t 1000] [--p 20] [--k 3] [--iters 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayesian_dlms_amd.engine import Engine  # noqa: E402
from bayesian_dlms_amd.factorsv import FactorSv, FsvParameters  # noqa: E402
from bayesian_dlms_amd.stochvol import SvParameters  # noqa: E402

HBM_NOMINAL = 8.0e12


def call_bytes(N, T, p, k):
    small = 8 * N * p * k + 8 * N * p
    return {"factors": 8 * N * T * p + 8 * N * k * (T + 1) + small + 8 * N * k * T,
            "loadings": 8 * N * T * p + 8 * N * k * T + 8 * N * p * k + small}


def run(eng, y, init, iters, warmup, literal):
    import torch
    N, T, p = (int(x) for x in y.shape)
    k = init.k
    lit = 1 if literal else 0
    c = FactorSv.initialise_state_ar(y, init, eng, seed=1, literal=literal)
    f, alpha, sv, beta, v = c["f"], c["alpha"], c["sv"].reshape(N * k, 3), c["beta"], c["v"]
    bufs = {"ystar": c["ystar"], "v": c["v_mix"]}
    sv_prior = (0, lit, 0.8, 0.1, 0.0, 1.0, 3.0, 0.3, 100.0, 0.05)
    fsv_prior = (lit, 0.0, 1.0, 3.0, 1.0)
    rows, status = [], 0
    for it in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mix = eng.sv_mixture(f.reshape(N * k, T), alpha.reshape(N * k, T + 1), iteration=it, seed=1, out=bufs)
        t1 = time.perf_counter()
        ff = eng.ar1_ffbs(mix["ystar"], mix["v"], sv, seed=1000004 + it, want_filt=False)
        t2 = time.perf_counter()
        alpha = ff["theta"].reshape(N, k, T + 1)
        res = eng.sv_params(ff["theta"], sv, sv_prior, iteration=it, seed=1, out={"sv": sv})
        t3 = time.perf_counter()
        fac = eng.fsv_factors(y, beta, v, alpha, iteration=it, seed=1, literal=literal, out={"f": f})
        t4 = time.perf_counter()
        ld = eng.fsv_loadings(y, f, beta, fsv_prior, iteration=it, seed=1, v=v, out={"beta": beta, "v": v})
        t5 = time.perf_counter()
        status |= int((mix["status"] | ff["status"] | res["status"]).max().item()) | int((fac["status"] | ld["status"]).max().item())
        if it >= warmup:
            rows.append((t5 - t0, t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4))
    r = np.median(np.array(rows) * 1e3, axis=0)
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
