"""The oracle standing in for the engine's FFBS call (the ffbs= argument of the Gibbs drivers), and a toy problem for it: what the
host tests of the Gibbs logic and the GPU test that compares the engine's chain with the oracle's share."""
import numpy as np

import oracle
from bayesian_dlms_amd.dlm import Dlm, DlmParameters


def oracle_ffbs(mat, params, y, *, seed=0, series_offset=0, flags=0, want_theta=True, want_stats=True, **kw):
    om = oracle.Model(mat.d, mat.p, mat.T, mat.F, mat.G, mat.g_index, mat.dt, mat.f_stride)
    plist = [params] * y.shape[0] if isinstance(params, DlmParameters) else list(params)
    outer = bool(flags & 16)
    thetas, stats = [], []
    for n in range(y.shape[0]):
        p = plist[n]
        f = oracle.kf_filter(om, p.v, p.w, p.m0, p.c0, y[n])
        z = oracle.normals(seed, series_offset + n, mat.T + 1, mat.d)
        th = oracle.backward_sample(om, p.w, f, z, factor="chol")["theta"]
        st = oracle.gibbs_stats(om, y[n], th, want_outer=outer)
        body = st["outer"] if outer else st["ss"]
        stats.append(np.concatenate([st["ssy"], st["n"], body, [mat.T]]))
        thetas.append(th)
    return {"theta": np.stack(thetas), "stats": np.stack(stats)}


def toy(N=6, T=40, seed=0):
    mod = Dlm.polynomial(2)
    times = np.arange(1, T + 1, dtype=np.float64)
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((N, T, 1)).cumsum(axis=1)
    y[rng.random(y.shape) < 0.1] = np.nan
    p = DlmParameters([[2.0]], np.diag([0.5, 0.2]), [0.0, 0.0], np.eye(2) * 10)
    return mod, times, y, p
