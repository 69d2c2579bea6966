"""Rao-Blackwellised filter next to the Liu-West filter in the same run: 1024 series, 500 times, Gaussian models with V and the diagonal of W
learned from Gaussian(log variance, 0.5) priors at the shrinkage a = 0.98, at (d, P) = (1, 512) a local level, (4, 512) a linear trend with
one seasonal harmonic and (13, 64) a level with six harmonics -- P the count dlm_rb_batch admits at that d or below it.  One call per
iteration, everything in HBM; only the [N] log-likelihoods are wanted.
Prints one JSON line per shape: ms per call of dlm_rb_batch and dlm_lw_batch (medians over --iters calls after --warmup, a host clock around
a synchronous call), their ratio, particle-steps per second, the smallest ESS / P of the Rao-Blackwellised filter and the worst status.

    python tools/rb_bench.py [--n 1024] [--t 500] [--shapes 1x512,4x512,13x64] [--iters 10] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from storvik_bench import clock  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dglm import Dglm, materialise_pf  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters  # noqa: E402
from bayesian_dlms_amd.engine import Engine  # noqa: E402

MODELS = {1: lambda: Dlm.polynomial(1), 4: lambda: Dlm.polynomial(2) + Dlm.seasonal(24, 1), 13: lambda: Dlm.polynomial(1) + Dlm.seasonal(24, 6)}


def problem(d, T, seed=1):
    """One simulated series of the model of dimension d and the parameters it was simulated at."""
    rng = np.random.default_rng(seed)
    dlm = MODELS[d]()
    wd = np.full(d, 0.005); wd[0] = 0.05
    truth = DlmParameters(np.eye(1), np.diag(wd), np.zeros(d), 0.1 * np.eye(d))
    times, y, _ = Dglm.gaussian(dlm).simulate_regular(truth, T, rng=rng)
    return dlm, times, y, truth, wd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--t", type=int, default=500)
    ap.add_argument("--shapes", default="1x512,4x512,13x64")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--a", type=float, default=0.98)
    a = ap.parse_args()
    import torch
    eng = Engine(0)
    for d, P in (tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")):
        dlm, times, y_h, truth, wd = problem(d, a.t)
        mat = materialise_pf(dlm, times)
        y = torch.as_tensor(np.tile(y_h, (a.n, 1)), device="cuda:0")
        prior_w, prior_v = np.stack([np.log(wd), np.full(d, 0.5)], axis=1), np.array([0.0, 0.5])
        kw = dict(n_particles=P, a=a.a, seed=1, prior_v=prior_v, learn_v=True, want_mean=False, want_psi_mean=False, want_psi_var=False,
                  want_weights=False, want_psi=False)
        rb = dict(kw, want_cov=False, want_means=False, want_covs=False)
        ms, out = clock(lambda it: eng.rb_filter(mat, truth, y, prior_w, iteration=it, want_ess=False, **rb), a.iters, a.warmup)
        variant = eng.last_variant
        chk = eng.rb_filter(mat, truth, y, prior_w, iteration=0, want_ess=True, **rb)
        lw = dict(kw, family=_lib.OBS_GAUSSIAN, want_cloud=False)
        ms_lw, out_lw = clock(lambda it: eng.lw_filter(mat, truth, y, prior_w, iteration=it, want_ess=False, **lw), a.iters, a.warmup)
        print(json.dumps({"shape": {"N": a.n, "T": a.t, "d": d, "P": P}, "a": a.a, "iters": a.iters, "warmup": a.warmup, "variant": variant,
                          "ms_per_call": round(ms, 3), "ms_per_call_lw": round(ms_lw, 3), "ratio_to_lw": round(ms / ms_lw, 2),
                          "particle_steps_per_s": round(a.n * P * a.t / (ms * 1e-3), 1),
                          "smallest_ess_over_p": round(float(chk["ess"].min().item()) / P, 3),
                          "ll_mean": round(float(out["ll"].mean().item()), 3), "ll_sd_across_series": round(float(out["ll"].std().item()), 3),
                          "ll_mean_lw": round(float(out_lw["ll"].mean().item()), 3), "ll_sd_across_series_lw": round(float(out_lw["ll"].std().item()), 3),
                          "status_or": int(chk["status"].max().item())}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
