"""Student-t DLM Gibbs at a C3-like shape: Dlm.polynomial(1) + Dlm.seasonal(24, 6) (d = 13), 10 000 series x 1000 steps simulated
on the device with Student-t noise (nu = 4).  One iteration = dlm_ffbs_batch with the per-series V_t stream and W, then
dlm_studentt_step_batch; everything stays in HBM.  Prints one JSON line: ms per iteration, split into the FFBS call (its
forward / backward kernels from dlm_last_timing, and the call's wall time) and the step call (wall time of the synchronous call),
the step's effective bandwidth, for the reference-form sampler and for simulation_smoother=True.

    python tools/studentt_bench.py [--n 10000] [--t 1000] [--iters 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters, materialise  # noqa: E402
from bayesian_dlms_amd.engine import Engine  # noqa: E402


def run(eng, mat, y, N, T, d, iters, warmup, simsmooth):
    import torch
    dev = y.device
    vs = torch.ones((N, T), dtype=torch.float64, device=dev)
    W = torch.as_tensor(np.tile(np.eye(d).T.reshape(-1) * 0.1, (N, 1)), device=dev)
    m0 = torch.zeros(d, dtype=torch.float64, device=dev)
    C0 = torch.as_tensor(np.eye(d).reshape(-1) * 10.0, device=dev)
    s = torch.ones(N, dtype=torch.float64, device=dev)
    nu = torch.full((N,), 3, dtype=torch.int32, device=dev)
    acc = torch.zeros(N, dtype=torch.int32, device=dev)
    prior = (3.0, 1.0, 3.0, 3.0)
    flags = _lib.OPT_FFBS_SIMSMOOTH if simsmooth else 0
    rows = []
    for it in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = eng.ffbs(mat, (vs.reshape(-1), T, W.reshape(-1), d * d, m0, 0, C0, 0, 1, 0), y, seed=it, flags=flags,
                       want_theta=True, want_stats=True, want_filt=False)
        t1 = time.perf_counter()
        fwd, bwd = eng.last_timing()
        res = eng.studentt_step(mat, y, out["theta"], out["stats"], prior, s, nu, iteration=it, accepted=acc,
                                out={"v": vs, "scale": s, "nu": nu, "W": W})
        t2 = time.perf_counter()
        del out
        if it >= warmup:
            rows.append((t2 - t0, t1 - t0, fwd + bwd, t2 - t1))
    r = np.median(np.array(rows) * np.array([1e3, 1e3, 1.0, 1e3]), axis=0)
    # algorithmic traffic of the step: theta and y read once, v written, the parked residual written and read back
    step_bytes = N * (T + 1) * d * 8 + N * T * 8 + 3 * N * T * 8
    return {"ms_per_iter": round(float(r[0]), 3), "ffbs_ms": round(float(r[1]), 3), "ffbs_kernels_ms": round(float(r[2]), 3),
            "step_ms": round(float(r[3]), 3), "step_gbs": round(step_bytes / (r[3] * 1e-3) / 1e9, 1),
            "accept_rate": round(float(acc.float().mean().item()) / (warmup + iters), 3),
            "variant_ffbs_status_ok": bool(int(res["status"].abs().sum().item()) == 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--t", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    N, T = a.n, a.t
    mod = Dlm.polynomial(1) + Dlm.seasonal(24, 6)
    mat = materialise(mod, np.arange(1, T + 1, dtype=np.float64))
    d = mat.d
    eng = Engine(0)
    w = np.diag([0.01] + [0.05] * (d - 1))
    sim = eng.simulate(mat, DlmParameters([[1.0]], w, np.zeros(d), np.eye(d)), N, seed=1, device=True, want_x=False)
    g = torch.Generator(device="cuda:0").manual_seed(3)
    # Student-t noise with nu = 4, s = 1: y = F^T x + z sqrt(v), v ~ InverseGamma(2, 2); the simulated unit-variance noise is z
    v = 2.0 / torch.distributions.Gamma(torch.full((N, T), 2.0, dtype=torch.float64, device="cuda:0"), 1.0).sample()
    y = sim["y"].reshape(N, T)
    del sim
    y = (y + (torch.sqrt(v) - 1.0) * torch.randn((N, T), dtype=torch.float64, device="cuda:0", generator=g)).contiguous()
    out = {"shape": {"N": N, "T": T, "d": d}, "iters": a.iters, "warmup": a.warmup}
    out["reference_form"] = run(eng, mat, y, N, T, d, a.iters, a.warmup, False)
    out["simulation_smoother"] = run(eng, mat, y, N, T, d, a.iters, a.warmup, True)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
