"""AR(1) stochastic-volatility Gibbs at 10 000 series x 1000 steps simulated at (phi, mu, sigma) = (0.8, 1.0, 0.3) (the example's,
examples/.../StochVol.scala).  One iteration = dlm_sv_mixture_batch, dlm_ar1_ffbs_batch, dlm_sv_params_batch; everything stays in
HBM.  Prints one JSON line per phi update: ms per iteration (median over --iters iterations after --warmup), the wall time of each of
the three synchronous calls, and the mixture call's algorithmic bytes (y and alpha read, ystar and v written: 32 B per element)
over its wall time.

--ou times the Ornstein-Uhlenbeck chain on an irregular grid instead (gaps uniform on [0.1, 3], data simulated at rate 0.3):
dlm_sv_mixture_batch, dlm_ou_ffbs_batch, dlm_sv_ou_params_batch, in the default and in the literal arithmetic.

    python tools/sv_bench.py [--ou] [--n 10000] [--t 1000] [--iters 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayesian_dlms_amd.engine import Engine  # noqa: E402
from bayesian_dlms_amd.stochvol import StochasticVolatility, SvParameters  # noqa: E402


def run(eng, y, N, T, iters, warmup, phi_update):
    import torch
    dev = y.device
    sv = torch.as_tensor(np.tile([0.8, 1.0, 0.3], (N, 1)), device=dev)
    acc = torch.zeros(N, dtype=torch.int32, device=dev)
    prior = (1, 0, 5.0, 2.0, 1.0, 1.0, 2.0, 2.0, 100.0, 0.05) if phi_update else (0, 0, 0.8, 0.1, 1.0, 1.0, 2.0, 2.0, 100.0, 0.05)
    mix = eng.sv_mixture(y, None, iteration=0, seed=1)
    alpha = eng.ar1_ffbs(mix["ystar"], mix["v"], sv, seed=1000003, want_filt=False)["theta"]
    bufs = {"ystar": mix["ystar"], "v": mix["v"]}
    rows, status = [], 0
    for it in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mix = eng.sv_mixture(y, alpha, iteration=it, seed=1, out=bufs)
        t1 = time.perf_counter()
        f = eng.ar1_ffbs(mix["ystar"], mix["v"], sv, seed=1000004 + it, want_filt=False)
        t2 = time.perf_counter()
        alpha = f["theta"]
        res = eng.sv_params(alpha, sv, prior, iteration=it, accepted=acc, seed=1, out={"sv": sv})
        t3 = time.perf_counter()
        status |= int((mix["status"] | f["status"] | res["status"]).max().item())
        if it >= warmup:
            rows.append((t3 - t0, t1 - t0, t2 - t1, t3 - t2))
    r = np.median(np.array(rows) * 1e3, axis=0)
    mix_bytes = 32 * N * T + 8 * N          # alpha rows are T + 1 long
    post = sv.cpu().numpy().mean(axis=0)
    return {"phi_update": "beta-mh" if phi_update else "conjugate", "ms_per_iter": round(float(r[0]), 3),
            "mixture_ms": round(float(r[1]), 3), "ffbs_ms": round(float(r[2]), 3), "params_ms": round(float(r[3]), 3),
            "mixture_gbs": round(mix_bytes / (r[1] * 1e-3) / 1e9, 1),
            "accept_rate": round(float(acc.float().mean().item()) / (warmup + iters), 3),
            "last_draw_mean": [round(float(x), 3) for x in post], "status_or": status}


def run_ou(eng, times, y, N, T, iters, warmup, literal):
    import torch
    dev = y.device
    sv = torch.as_tensor(np.tile([0.3, 1.0, 0.3], (N, 1)), device=dev)
    acc = torch.zeros((N, 3), dtype=torch.int32, device=dev)
    prior = (1 if literal else 0, 5.0, 2.0, 1.0, 1.0, 2.0, 2.0, 0.05 if literal else 10.0, 0.05, 0.05, 0.05)
    mix = eng.sv_mixture(y, None, iteration=0, seed=1)
    alpha = eng.ar1_ffbs(mix["ystar"], mix["v"], sv, seed=1000003, want_filt=False, times=times)["theta"]
    bufs = {"ystar": mix["ystar"], "v": mix["v"]}
    rows, status = [], 0
    for it in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mix = eng.sv_mixture(y, alpha, iteration=it, seed=1, out=bufs)
        t1 = time.perf_counter()
        f = eng.ar1_ffbs(mix["ystar"], mix["v"], sv, seed=1000004 + it, want_filt=False, times=times)
        t2 = time.perf_counter()
        alpha = f["theta"]
        res = eng.sv_ou_params(times, alpha, sv, prior, iteration=it, accepted=acc, seed=1, out={"sv": sv})
        t3 = time.perf_counter()
        status |= int((mix["status"] | f["status"] | res["status"]).max().item())
        if it >= warmup:
            rows.append((t3 - t0, t1 - t0, t2 - t1, t3 - t2))
    r = np.median(np.array(rows) * 1e3, axis=0)
    row_bytes = 8 * N * (T + 1)             # the parameter call reads every alpha row once
    post = sv.cpu().numpy().mean(axis=0)
    return {"model": "ou", "arithmetic": "literal" if literal else "default", "ms_per_iter": round(float(r[0]), 3),
            "mixture_ms": round(float(r[1]), 3), "ffbs_ms": round(float(r[2]), 3), "params_ms": round(float(r[3]), 3),
            "params_row_gbs": round(row_bytes / (r[3] * 1e-3) / 1e9, 1),
            "params_ns_per_pair": round(float(r[3]) * 1e6 / (N * (T - 1)), 4),
            "accept_rate": [round(float(x) / (warmup + iters), 3) for x in acc.float().mean(dim=0).tolist()],
            "last_draw_mean": [round(float(x), 3) for x in post], "status_or": status}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ou", action="store_true", help="the Ornstein-Uhlenbeck chain on an irregular grid")
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--t", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    N, T = a.n, a.t
    eng = Engine(0)
    if a.ou:
        t_h = np.cumsum(np.random.default_rng(1).uniform(0.1, 3.0, T))
        y_h, _ = StochasticVolatility.simulate_ou(SvParameters(0.3, 1.0, 0.3), t_h, N, seed=1)
        y, times = torch.as_tensor(y_h, device="cuda:0"), torch.as_tensor(t_h, device="cuda:0")
        for literal in (False, True):
            out = {"shape": {"N": N, "T": T}, "iters": a.iters, "warmup": a.warmup}
            out.update(run_ou(eng, times, y, N, T, a.iters, a.warmup, literal))
            print(json.dumps(out))
        eng.close()
        return
    y_h, _ = StochasticVolatility.simulate(SvParameters(0.8, 1.0, 0.3), T, N, seed=1)
    y = torch.as_tensor(y_h, device="cuda:0")
    for phi_update in (0, 1):
        out = {"shape": {"N": N, "T": T}, "iters": a.iters, "warmup": a.warmup}
        out.update(run(eng, y, N, T, a.iters, a.warmup, phi_update))
        print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
