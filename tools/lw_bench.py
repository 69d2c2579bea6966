"""Liu-West filter at the size of tools/storvik_bench.py, next to the bootstrap filter and the Storvik filter in the same run: 1024 series,
500 times, a Poisson model with a linear trend and one seasonal harmonic (d = 4), at P = 512 particles (more with --particles).  The Liu-West
filter learns the diagonal of W from Gaussian(log W_kk, 0.5) priors on the log-variances with the shrinkage a = 0.98 (the Poisson family has
no V to learn); the Storvik filter from InverseGamma(4, 3 W_kk) priors; the bootstrap filter runs at the W those priors are centred on.  One
call per iteration, everything in HBM; only the [N] log-likelihoods are wanted.
Prints one JSON line per P: ms per call of dlm_lw_batch, dlm_pf_batch and dlm_storvik_batch (medians over --iters calls after --warmup, a
host clock around a synchronous call), the ratios, particle-steps per second, the share of observed steps whose second stage resampled and
the worst status.  With --gaussian the model is the Gaussian one and V is learned too.  With --aux the filter runs as the auxiliary particle
filter for known parameters (a = 1, every prior sd 0).

    python tools/lw_bench.py [--n 1024] [--t 500] [--particles 512] [--iters 10] [--warmup 3] [--gaussian] [--aux]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pf_bench import problem  # noqa: E402
from storvik_bench import clock  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dglm import Dglm, materialise_pf  # noqa: E402
from bayesian_dlms_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--t", type=int, default=500)
    ap.add_argument("--particles", default="512")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--a", type=float, default=0.98)
    ap.add_argument("--gaussian", action="store_true")
    ap.add_argument("--aux", action="store_true")
    a = ap.parse_args()
    import torch
    mod, times, y_h, bp = problem(a.n, a.t)
    family = _lib.OBS_POISSON
    if a.gaussian:
        mod, family, y_h = Dglm.gaussian(mod.dlm), _lib.OBS_GAUSSIAN, np.log1p(y_h)
    mat = materialise_pf(mod, times)
    d = mat.d
    eng = Engine(0)
    y = torch.as_tensor(np.tile(y_h, (a.n, 1)), device="cuda:0")
    packed = bp.packed()
    idx = np.arange(d)
    sd = 0.0 if a.aux else 0.5
    shrink = 1.0 if a.aux else a.a
    lw_prior_w = np.stack([np.log(bp.w[:, idx, idx]), np.full((a.n, d), sd)], axis=2)          # [N][d][2] = (mean, sd) of log W_kk
    lw_prior_v = np.array([0.0, sd]) if a.gaussian else None
    st_prior_w = np.stack([np.full((a.n, d), 4.0), 3.0 * bp.w[:, idx, idx]], axis=2)          # [N][d][2] = (shape, scale)
    st_prior_v = np.array([4.0, 3.0]) if a.gaussian else None
    for P in (int(x) for x in a.particles.split(",")):
        none = dict(want_mean=False, want_cloud=False, want_weights=False)
        kw = dict(family=family, n_particles=P, a=shrink, seed=1, prior_v=lw_prior_v, want_psi_mean=False, want_psi_var=False, want_psi=False, **none)
        ms, out = clock(lambda it: eng.lw_filter(mat, packed, y, lw_prior_w, iteration=it, want_ess=False, **kw), a.iters, a.warmup)
        variant = eng.last_variant
        chk = eng.lw_filter(mat, packed, y, lw_prior_w, iteration=0, want_ess=True, **kw)
        ess = chk["ess"].cpu().numpy()
        ms_pf, _ = clock(lambda it: eng.particle_filter(mat, packed, y, family=family, n_particles=P, seed=1, iteration=it, want_ess=False, **none),
                         a.iters, a.warmup)
        skw = dict(family=family, n_particles=P, seed=1, prior_v=st_prior_v, want_scale_mean=False, want_scales=False, **none)
        ms_st, _ = clock(lambda it: eng.storvik_filter(mat, packed, y, st_prior_w, iteration=it, want_ess=False, **skw), a.iters, a.warmup)
        print(json.dumps({"shape": {"N": a.n, "T": a.t, "d": d, "P": P}, "family": "gaussian" if a.gaussian else "poisson",
                          "learn_v": bool(a.gaussian), "a": shrink, "prior_sd": sd, "iters": a.iters, "warmup": a.warmup, "variant": variant,
                          "ms_per_call": round(ms, 3), "ms_per_call_pf": round(ms_pf, 3), "ms_per_call_storvik": round(ms_st, 3),
                          "ratio_to_pf": round(ms / ms_pf, 2), "ratio_to_storvik": round(ms / ms_st, 2),
                          "particle_steps_per_s": round(a.n * P * a.t / (ms * 1e-3), 1),
                          "resampled_share": round(float((ess < P // 5).mean()), 3),
                          "ll_mean": round(float(out["ll"].mean().item()), 3), "ll_sd_across_series": round(float(out["ll"].std().item()), 3),
                          "status_or": int(chk["status"].max().item())}))
    eng.close()


if __name__ == "__main__":
    main()
