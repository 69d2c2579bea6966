"""The state draw of the AR(1) stochastic-volatility chain by the knot block sampler (dlm_sv_knots_batch) at 10 000 series x 1000 steps
simulated at (phi, mu, sigma) = (0.8, 1.0, 0.3), knots drawn with block sizes uniform on [--min-size, --max-size] (the reference's 10,
100) afresh for every iteration; everything stays in HBM.  The chain starts as the drivers do (initial_state_ar) and the parameters
stay at the simulated values: this times the state draw alone.  Beside it, alternating in the same process on the same state, the
state draw of the mixture sampler (dlm_sv_mixture_batch + dlm_ar1_ffbs_batch: StochasticVolatility.sample_state_ar).
Prints one JSON line: the wall time of one synchronous sv_knots call (median, smallest, largest over --iters iterations after
--warmup), the same for mixture + FFBS, the mean number of blocks, the block acceptance rate over the timed iterations, and the knot
call's algorithmic bytes (y and alpha read, alpha written: 24 B per state; its scratch traffic is not counted) over its median time.

    python tools/svknots_bench.py [--n 10000] [--t 1000] [--min-size 10] [--max-size 100] [--iters 20] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayesian_dlms_amd.engine import Engine  # noqa: E402
from bayesian_dlms_amd.stochvol import StochasticVolatility, SvParameters, knots_rng, sample_knots  # noqa: E402


def run(eng, y, N, T, lo, hi, iters, warmup):
    import torch
    dev = y.device
    sv = torch.as_tensor(np.tile([0.8, 1.0, 0.3], (N, 1)), device=dev)
    mix = eng.sv_mixture(y, None, iteration=0, seed=1)
    alpha = eng.ar1_ffbs(mix["ystar"], mix["v"], sv, seed=1000003, want_filt=False)["theta"]
    alpha_mix = alpha.clone()
    bufs = {"ystar": mix["ystar"], "v": mix["v"]}
    acc = torch.zeros(N, dtype=torch.int32, device=dev)
    rows, blocks, accepted, status = [], 0, 0, 0
    for it in range(warmup + iters):
        knots = torch.as_tensor(sample_knots(lo, hi, T, knots_rng(1, it)), device=dev)
        before = int(acc.sum().item())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = eng.sv_knots(y, alpha, sv, knots, iteration=it, accepted=acc, seed=1, out={"alpha": alpha})
        t1 = time.perf_counter()
        mix = eng.sv_mixture(y, alpha_mix, iteration=it, seed=1, out=bufs)
        f = eng.ar1_ffbs(mix["ystar"], mix["v"], sv, seed=1000004 + it, want_filt=False)
        t2 = time.perf_counter()
        alpha_mix = f["theta"]
        status |= int((res["status"] | mix["status"] | f["status"]).max().item())
        if it >= warmup:
            rows.append((t1 - t0, t2 - t1))
            blocks += int(knots.numel()) - 1
            accepted += int(acc.sum().item()) - before
    r = np.array(rows) * 1e3
    med = np.median(r, axis=0)
    return {"knots_ms": round(float(med[0]), 3), "knots_ms_min_max": [round(float(r[:, 0].min()), 3), round(float(r[:, 0].max()), 3)],
            "mixture_ffbs_ms": round(float(med[1]), 3), "mixture_ffbs_ms_min_max": [round(float(r[:, 1].min()), 3), round(float(r[:, 1].max()), 3)],
            "mean_blocks": round(blocks / iters, 1), "block_accept_rate": round(accepted / (N * blocks), 3),
            "knots_gbs": round(24 * N * (T + 1) / (med[0] * 1e-3) / 1e9, 1), "status_or": status}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--t", type=int, default=1000)
    ap.add_argument("--min-size", type=int, default=10)
    ap.add_argument("--max-size", type=int, default=100)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    y_h, _ = StochasticVolatility.simulate(SvParameters(0.8, 1.0, 0.3), a.t, a.n, seed=1)
    eng = Engine(0)
    y = torch.as_tensor(y_h, device="cuda:0")
    out = {"shape": {"N": a.n, "T": a.t}, "block_sizes": [a.min_size, a.max_size], "iters": a.iters, "warmup": a.warmup}
    out.update(run(eng, y, a.n, a.t, a.min_size, a.max_size, a.iters, a.warmup))
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
