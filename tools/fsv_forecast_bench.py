"""One predictive band of DlmFsvSystem.forecast at the size of the reference's AqMesh example: p = 7 series, each a local level and three
harmonics of a daily cycle (d = 49 states), k = 2 factors of the system noise, M = 1000 kept draws, R = 64 volatility paths per draw and
H = 36 steps, from one panel of --t training times.  The draws are synthetic (the band's cost does not depend on where they came from).
The driver's own code runs on a timing wrapper of the engine (tools/timed_engine.py), so the time is split by engine call:
  dlmfsv_variance, filter           the training filter per draw, then the horizon's W_t stream and the Kalman forecast on it
  sv_paths, gaussian_mixture_summary   the two calls of dlm_fsv_forecast.hip
Prints one JSON line: the wall time of the band (median over --iters runs after --warmup), the sum and the count of each engine call's wall
times in the median run, and the share of the two new calls beside the existing filter.  Run it under a time limit of its own, e.g.

    timeout -k 10 900 python tools/fsv_forecast_bench.py [--m 1000] [--paths 64] [--h 36] [--t 200] [--iters 3] [--warmup 1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayesian_dlms_amd import _dlmfsv  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm  # noqa: E402
from bayesian_dlms_amd.dlmfsvsys import KIND  # noqa: E402
from bayesian_dlms_amd.engine import Engine  # noqa: E402
from timed_engine import TimedEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--paths", type=int, default=64)
    ap.add_argument("--h", type=int, default=36)
    ap.add_argument("--t", type=int, default=200)
    ap.add_argument("--series", type=int, default=7)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    import torch
    one = Dlm.polynomial(1) + Dlm.seasonal(24, 3)
    mod = one
    for _ in range(a.series - 1):
        mod = mod * one
    p, d, M, k, T = a.series, 7 * a.series, a.m, a.k, a.t
    rng = np.random.default_rng(1)
    draws = {"beta": 0.3 * rng.normal(size=(M, 1, d, k)), "v": rng.uniform(0.02, 0.05, (M, 1, d)),
             "sv": np.stack([rng.uniform(0.7, 0.9, (M, 1, k)), rng.normal(-1.0, 0.2, (M, 1, k)), rng.uniform(0.2, 0.4, (M, 1, k))], axis=3),
             "alpha": rng.normal(-1.0, 0.5, (M, 1, k, T + 1)), "V": rng.uniform(0.2, 0.3, (M, 1, p))}
    ys = rng.normal(size=(1, T, p))
    eng = Engine(0)
    timed = TimedEngine(eng)
    runs = []
    for it in range(a.warmup + a.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = _dlmfsv.forecast(KIND, mod, ys, draws, a.h, timed, m0=np.zeros(d), c0=np.eye(d), n_paths=a.paths, prob=0.75, seed=1)
        wall = time.perf_counter() - t0
        calls, timed.calls = timed.calls, []
        if it >= a.warmup:
            runs.append((wall, calls))
    wall, calls = sorted(runs, key=lambda r: r[0])[len(runs) // 2]
    by = {}
    for name, s in calls:
        ms, n = by.get(name, (0.0, 0))
        by[name] = (ms + s * 1e3, n + 1)
    res = {"shape": {"p": p, "d": d, "k": k, "M": M, "R": a.paths, "H": a.h, "T": T}, "iters": a.iters, "warmup": a.warmup,
           "band_ms": round(wall * 1e3, 2), "engine_ms": round(sum(ms for ms, _ in by.values()), 2)}
    res.update({name + "_ms": round(ms, 3) for name, (ms, _) in by.items()})
    res.update({name + "_calls": n for name, (_, n) in by.items()})
    new = by.get("sv_paths", (0.0, 0))[0] + by.get("gaussian_mixture_summary", (0.0, 0))[0]
    res["new_kernels_over_filter"] = round(new / by["filter"][0], 4)
    res["new_kernels_share_of_engine"] = round(new / res["engine_ms"], 4)
    res["status_or"] = int(out["status"].max())
    res["upper_minus_lower_mean"] = round(float((out["upper"] - out["lower"]).mean()), 4)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
