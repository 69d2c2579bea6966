"""One particle-Gibbs sweep (dlm_pg_batch) beside one bootstrap-filter call (dlm_pf_batch) at the same (N, T, d, P): tools/pf_bench.py's
problem and sizes -- 1024 series with per-series parameters, 500 times, a Poisson model with a linear trend and one seasonal harmonic
(d = 4), at P = 512, 64 and 1024 particles.  The reference path of the sweep is the filtering means of one filter run; only ll, path and
stats are asked of the sweep (its clouds and ancestors go to the engine's workspace), only ll of the filter.
Prints one JSON line per P: ms per call of either (medians over --iters calls after --warmup, a host clock around a synchronous call), their
ratio, the bytes of clouds and ancestors a sweep writes with the time they would take at the HBM bandwidth given by --hbm-gbs (the share of the
sweep that the writes can account for at most), the launches the workspace cap split the batch into, and the worst status.

    python tools/pg_bench.py [--n 1024] [--t 500] [--particles 512,64,1024] [--iters 10] [--warmup 3] [--hbm-gbs 8000] [--plain]
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
from bayesian_dlms_amd.dlm import Dlm, materialise  # noqa: E402
from bayesian_dlms_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--t", type=int, default=500)
    ap.add_argument("--particles", default="512,64,1024")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM bandwidth the cloud writes are judged against, GB/s")
    ap.add_argument("--plain", action="store_true", help="plain conditional SMC: no ancestor sampling")
    a = ap.parse_args()
    import torch
    mod, times, y_h, bp = problem(a.n, a.t)
    mat = materialise(Dlm(mod.f, mod.g), times)
    d, T = mat.d, mat.T
    eng = Engine(0)
    y = torch.as_tensor(np.tile(y_h, (a.n, 1)), device="cuda:0")
    packed = bp.packed()

    def clock(call):
        rows = []
        for it in range(a.warmup + a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = call(it)
            torch.cuda.synchronize()
            if it >= a.warmup:
                rows.append(time.perf_counter() - t0)
        return float(np.median(rows) * 1e3), out

    for P in (int(x) for x in a.particles.split(",")):
        pf_kw = dict(family=_lib.OBS_POISSON, n_particles=P, seed=1, want_ess=False, want_cloud=False, want_weights=False)
        start = eng.particle_filter(mat, packed, y, iteration=0, want_mean=True, **pf_kw)
        ref = torch.cat([torch.as_tensor(bp.m0, device="cuda:0")[:, None, :], start["mean"]], dim=1).contiguous()
        pf_ms, _ = clock(lambda it: eng.particle_filter(mat, packed, y, iteration=it, want_mean=False, **pf_kw))
        pg_ms, out = clock(lambda it: eng.pg_sweep(mat, packed, y, ref, family=_lib.OBS_POISSON, n_particles=P, ancestor_sampling=not a.plain,
                                                   iteration=it, seed=1))
        per_series = (T + 1) * d * P * 8 + T * P * 4
        launches = -(-a.n // max(1, min(a.n, _lib.PG_WORKSPACE_CAP // per_series)))
        write_ms = a.n * per_series / (a.hbm_gbs * 1e9) * 1e3
        print(json.dumps({"shape": {"N": a.n, "T": a.t, "d": d, "P": P}, "family": "poisson", "ancestor_sampling": not a.plain, "iters": a.iters,
                          "warmup": a.warmup, "variant": eng.last_variant, "pg_ms_per_sweep": round(pg_ms, 3), "pf_ms_per_call": round(pf_ms, 3),
                          "pg_over_pf": round(pg_ms / pf_ms, 3), "particle_steps_per_s": round(a.n * P * a.t / (pg_ms * 1e-3), 1),
                          "trace_bytes": a.n * per_series, "trace_write_ms_at_hbm": round(write_ms, 3), "trace_share_of_sweep": round(write_ms / pg_ms, 3),
                          "launches": launches, "ll_mean": round(float(out["ll"].mean().item()), 3), "status_or": int(out["status"].max().item())}))
    eng.close()


if __name__ == "__main__":
    main()
