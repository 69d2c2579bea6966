"""The forecast from a learning filter's cloud at the size of a posterior-predictive band, against the bootstrap filter's forecast: tools/pf_forecast_bench.py's
shape -- 1024 series, P = 512 particles, H = 200 steps of tools/pf_bench.py's model (Poisson, a linear trend and one seasonal harmonic, d = 4) --,
everything in HBM, the mean and the three order statistics of a median band wanted (no draws, no cloud, no state mean).  The baseline is
dlm_pf_forecast_particles from the same cloud with every y missing (a pure forecast; that kernel's W is each series' diagonal W); the new call
runs from the same cloud with that diagonal as every particle's own variance rows (FC_VAR: the same law, and per particle and step d more LDS
reads), with its logarithms (FC_LOGVAR) and with InverseGamma scales whose mean it is (FC_IG_SCALE: d Gamma draws per particle at entry).
The calls ALTERNATE inside one loop, so that a drift of the clocks meets all of them alike.  Prints one JSON line per call -- ms per call (the
median over --iters rounds after --warmup, a host clock around a synchronous call), particle-steps per second, the share of series that
stopped -- and a last line with the ratios to the baseline.

    python tools/pf_forecast_learned_bench.py [--n 1024] [--h 200] [--particles 512] [--iters 10] [--warmup 3]
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
    d = mat.d
    eng = Engine(0)
    rng = np.random.default_rng(2)
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda:0")
    wd = bp.w[:, np.arange(d), np.arange(d)]                                        # [N][d]: each series' diagonal W
    cloud = dev(bp.m0[:, :, None] + np.sqrt(np.diagonal(bp.c0, axis1=1, axis2=2))[:, :, None] * rng.standard_normal((N, d, P)))
    rows = np.broadcast_to(wd[:, :, None], (N, d, P))
    shape = 6.0
    var_rows, log_rows, ig_rows = dev(rows), dev(np.log(rows)), dev(rows * (shape - 1.0))
    shapes = np.full(d + 1, shape)
    y_nan = torch.full((N, H), float("nan"), dtype=torch.float64, device="cuda:0")
    packed = bp.packed()
    ranks = Dglm.interval_ranks(P, 0.75)
    common = dict(family=_lib.OBS_POISSON, ranks=ranks, seed=1, want_mean=False, want_cloud=False)
    learned = lambda pw, kind, **kw: (lambda it: eng.pf_forecast_learned(mat, packed, cloud, pw, None, var_kind=kind, iteration=it, want_var=False,
                                                                         **common, **kw))
    runs = {
        "bootstrap-forecast": lambda it: eng.pf_forecast(mat, packed, y_nan, n_particles=P, cloud=cloud, iteration=it, **common),
        "learned-var": learned(var_rows, _lib.FC_VAR),
        "learned-logvar": learned(log_rows, _lib.FC_LOGVAR),
        "learned-ig-scale": learned(ig_rows, _lib.FC_IG_SCALE, shapes=shapes),
    }
    rows_ms, outs, variants = {name: [] for name in runs}, {}, {}
    for it in range(a.warmup + a.iters):
        for name, call in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[name] = call(it)
            torch.cuda.synchronize()
            variants[name] = eng.last_variant
            if it >= a.warmup:
                rows_ms[name].append((time.perf_counter() - t0) * 1e3)
    ms = {name: float(np.median(v)) for name, v in rows_ms.items()}
    for name in runs:
        out = outs[name]
        print(json.dumps({"run": name, "shape": {"N": N, "H": H, "d": d, "P": P}, "family": "poisson", "iters": a.iters, "warmup": a.warmup,
                          "variant": variants[name], "ms_per_call": round(ms[name], 3), "ms_min_max": [round(min(rows_ms[name]), 3), round(max(rows_ms[name]), 3)],
                          "particle_steps_per_s": round(N * P * H / (ms[name] * 1e-3), 1), "status_or": int(out["status"].max().item()),
                          "stopped_share": round(float((out["status"] != 0).double().mean().item()), 4),
                          "lds_bytes": _lib.pf_forecast_learned_lds_bytes(d, P) if name != "bootstrap-forecast" else ((d + 2) * P + d * d) * 8 + 4 * P}))
    filled = lambda name, k: torch.nan_to_num(outs[name][k], nan=-1.0)          # (a stopped series has NaN on both sides)
    same = all(torch.equal(filled("bootstrap-forecast", k), filled("learned-var", k)) for k in ("fmean", "fquant"))
    print(json.dumps({"ratio_learned_var_to_bootstrap": round(ms["learned-var"] / ms["bootstrap-forecast"], 3),
                      "ratio_learned_logvar_to_bootstrap": round(ms["learned-logvar"] / ms["bootstrap-forecast"], 3),
                      "ratio_learned_ig_scale_to_bootstrap": round(ms["learned-ig-scale"] / ms["bootstrap-forecast"], 3),
                      "learned_var_equals_bootstrap_bit_for_bit": same}))
    eng.close()


if __name__ == "__main__":
    main()
