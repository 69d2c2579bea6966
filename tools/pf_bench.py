"""Bootstrap particle filter at the size of a particle-marginal Metropolis step: 1024 series (chains) with per-series parameters, 500 times,
a Poisson model with a linear trend and one seasonal harmonic (d = 4), at P = 512, 64 and 1024 particles.  One call of dlm_pf_batch per
iteration, everything in HBM; only the [N] log-likelihoods are wanted (no means, ESS, cloud or weights).
Prints one JSON line per P: ms per call (median over --iters calls after --warmup, a host clock around a synchronous call), particle-steps
per second (N P T / time), the share of observed steps that resampled (from one extra call that asks for the ESS) and the worst status.
The kernel is ONE kernel (k_pf<4>): a kernel trace has no phases to tell apart; how its time splits is not measured here.

--resample chooses the ancestor step of the resampling (dlm_pf_resampled; --mh-steps with metropolis); the default is multinomial.

    python tools/pf_bench.py [--n 1024] [--t 500] [--particles 512,64,1024] [--iters 10] [--warmup 3]
                             [--resample {multinomial,stratified,systematic,metropolis}] [--mh-steps B]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dglm import BatchedParameters, Dglm, materialise_pf  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters  # noqa: E402
from bayesian_dlms_amd.engine import Engine  # noqa: E402


SCHEMES = {"multinomial": _lib.RESAMPLE_MULTINOMIAL, "stratified": _lib.RESAMPLE_STRATIFIED, "systematic": _lib.RESAMPLE_SYSTEMATIC,
           "metropolis": _lib.RESAMPLE_METROPOLIS}


def problem(N, T, seed=1):
    """One simulated series, and N parameter sets around the truth (what N chains of a sampler would hold)."""
    rng = np.random.default_rng(seed)
    mod = Dglm.poisson(Dlm.polynomial(2) + Dlm.seasonal(24, 1))
    truth = DlmParameters(np.eye(1), np.diag([0.01, 1e-8, 0.005, 0.005]), np.array([2.0, 0.0, 0.5, 0.0]), np.diag([0.1, 1e-6, 0.1, 0.1]))
    times, y, _ = mod.simulate_regular(truth, T, rng=rng)
    bp = BatchedParameters.of(truth, N).copy()
    idx = np.arange(4)
    bp.w[:, idx, idx] *= np.exp(0.2 * rng.standard_normal((N, 4)))
    bp.m0 += 0.05 * rng.standard_normal((N, 4))
    return mod, times, y, bp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--t", type=int, default=500)
    ap.add_argument("--particles", default="512,64,1024")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--resample", choices=list(SCHEMES), default="multinomial")
    ap.add_argument("--mh-steps", type=int, default=None, help="steps of a Metropolis chain (default 10 with --resample metropolis)")
    a = ap.parse_args()
    mh_steps = (10 if a.mh_steps is None else a.mh_steps) if a.resample == "metropolis" else (a.mh_steps or 0)
    import torch
    mod, times, y_h, bp = problem(a.n, a.t)
    mat = materialise_pf(mod, times)
    eng = Engine(0)
    y = torch.as_tensor(np.tile(y_h, (a.n, 1)), device="cuda:0")
    packed = bp.packed()
    for P in (int(x) for x in a.particles.split(",")):
        kw = dict(family=_lib.OBS_POISSON, n_particles=P, seed=1, want_mean=False, want_cloud=False, want_weights=False,
                  resample=SCHEMES[a.resample], mh_steps=mh_steps)
        rows = []
        for it in range(a.warmup + a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = eng.particle_filter(mat, packed, y, iteration=it, want_ess=False, **kw)
            torch.cuda.synchronize()
            if it >= a.warmup:
                rows.append(time.perf_counter() - t0)
        ms = float(np.median(rows) * 1e3)
        chk = eng.particle_filter(mat, packed, y, iteration=0, want_ess=True, **kw)
        ess = chk["ess"].cpu().numpy()
        print(json.dumps({"shape": {"N": a.n, "T": a.t, "d": mat.d, "P": P}, "family": "poisson", "resample": a.resample, "mh_steps": mh_steps, "iters": a.iters, "warmup": a.warmup,
                          "variant": eng.last_variant, "ms_per_call": round(ms, 3),
                          "particle_steps_per_s": round(a.n * P * a.t / (ms * 1e-3), 1),
                          "resampled_share": round(float((ess < P // 5).mean()), 3),
                          "ll_mean": round(float(out["ll"].mean().item()), 3), "ll_sd_across_chains": round(float(out["ll"].std().item()), 3),
                          "status_or": int(chk["status"].max().item())}))
    eng.close()


if __name__ == "__main__":
    main()
