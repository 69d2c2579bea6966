"""Particle forecast at the size of a posterior-predictive band: 1024 parameter sets (one per posterior draw), P = 512 particles, H = 200 steps of
tools/pf_bench.py's model (Poisson, a linear trend and one seasonal harmonic, d = 4).  One call of dlm_pf_forecast_particles, everything in HBM,
with the mean and the three order statistics of a median band wanted (no draws, no cloud): first with every y missing (a pure forecast: no
weighting, no resampling), then with every y observed (the forecast's draws and sort on top of a whole filter step).  In the same run
dlm_pf_batch at the same shape: with n0 = P + 1, which resamples at every step as the observed forecast does, and with its default n0.
Prints one JSON line per timed call -- ms per call (median over --iters calls after --warmup, a host clock around a synchronous call),
particle-steps per second and the share of series that stopped (an unobserved trend extrapolated over H steps takes a few parameter sets'
rates beyond the 1e15 the samplers accept) -- and a last line with the ratios of the forecast to the filter, and of a forecast without ranks (no sort) to
one with them.

    python tools/pf_forecast_bench.py [--n 1024] [--h 200] [--particles 512] [--iters 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pf_bench import problem  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dglm import Dglm, materialise_pf  # noqa: E402
from bayesian_dlms_amd.engine import Engine  # noqa: E402


def timed(call, iters, warmup):
    import torch
    rows, out = [], None
    for it in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call(it)
        torch.cuda.synchronize()
        if it >= warmup:
            rows.append(time.perf_counter() - t0)
    return float(np.median(rows) * 1e3), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--h", type=int, default=200)
    ap.add_argument("--particles", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    N, H, P = a.n, a.h, a.particles
    mod, times, y_h, bp = problem(N, H)
    mat = materialise_pf(mod, times)
    eng = Engine(0)
    y_obs = torch.as_tensor(np.tile(y_h, (N, 1)), device="cuda:0")
    y_nan = torch.full_like(y_obs, float("nan"))
    packed = bp.packed()
    lo, med, up = Dglm.interval_ranks(P, 0.75)
    fkw = dict(family=_lib.OBS_POISSON, n_particles=P, seed=1, want_mean=False, want_cloud=False)
    pkw = dict(family=_lib.OBS_POISSON, n_particles=P, seed=1, want_mean=False, want_ess=False, want_cloud=False, want_weights=False)
    runs = {
        "forecast-all-missing": lambda it: eng.pf_forecast(mat, packed, y_nan, ranks=(lo, med, up), iteration=it, **fkw),
        "forecast-all-observed": lambda it: eng.pf_forecast(mat, packed, y_obs, ranks=(lo, med, up), iteration=it, **fkw),
        "forecast-all-missing-no-ranks": lambda it: eng.pf_forecast(mat, packed, y_nan, iteration=it, **fkw),
        "filter-always-resampling": lambda it: eng.particle_filter(mat, packed, y_obs, n0=P + 1, iteration=it, **pkw),
        "filter": lambda it: eng.particle_filter(mat, packed, y_obs, iteration=it, **pkw),
    }
    ms = {}
    for name, call in runs.items():
        ms[name], out = timed(call, a.iters, a.warmup)
        print(json.dumps({"run": name, "shape": {"N": N, "H": H, "d": mat.d, "P": P}, "family": "poisson", "iters": a.iters, "warmup": a.warmup,
                          "variant": eng.last_variant, "ms_per_call": round(ms[name], 3),
                          "particle_steps_per_s": round(N * P * H / (ms[name] * 1e-3), 1), "status_or": int(out["status"].max().item()),
                          "stopped_share": round(float((out["status"] != 0).double().mean().item()), 4)}))
    print(json.dumps({"ratio_forecast_missing_to_filter_always": round(ms["forecast-all-missing"] / ms["filter-always-resampling"], 3),
                      "ratio_forecast_observed_to_filter_always": round(ms["forecast-all-observed"] / ms["filter-always-resampling"], 3),
                      "ratio_forecast_observed_to_filter_default": round(ms["forecast-all-observed"] / ms["filter"], 3),
                      "ratio_sort_share_of_missing_forecast": round(1.0 - ms["forecast-all-missing-no-ranks"] / ms["forecast-all-missing"], 3)}))
    eng.close()


if __name__ == "__main__":
    main()
