"""The inputs of the tests of the forecast from a learning filter's cloud (tests/test_pf_forecast_learned_host.py,
tests/test_pf_forecast_learned_gpu.py), made from seeds, the exact laws they are held to, and the one runner of the engine call.  Every shape is
the smallest at which its part of the kernel can go wrong:

  P   64 one slot of particles, 128 a carry between two slots of the resampling's running sums, 192 a sort padded from 192 to 256, 512 with
      d = 16 the LDS boundary;  d 1, 2, 3 (a dense G) and every d up to 16;  H 2 .. 8;  the six families;  the three kinds of variance rows;
      a dt = 0 first step and an irregular grid with three G.

The law tests (LOGVAR_LAW, IG_LAW) are deterministic -- fixed seeds --; their threshold is the project's p > 1e-4, and the host tests run them on
the restatement and on its two mutants, so that the threshold is known to separate a right sampler from a wrong one at these very sizes."""
import functools

import numpy as np
from scipy import stats

import pf_cases as pc
import pf_restatement as pr
import pffl_restatement as lr

P_VALUE = 1e-4
ANCHOR_H = 5
ANCHOR = [dict(name="anchor-" + pc.FAMILY_NAMES[f], family=f, d=(1, 2, 3)[f % 3], P=(64, 128, 192, 128, 192, 64)[f], N=3, seed=f) for f in range(6)]
ANCHOR_NAMES = [c["name"] for c in ANCHOR]
KINDS = {"var": lr.FC_VAR, "logvar": lr.FC_LOGVAR, "ig": lr.FC_IG_SCALE}
DRAW_CASES = [(pc.FAMILY_NAMES[f], kind) for f in range(6) for kind in KINDS]
DISCRETE = (pr.POISSON, pr.NEGBIN, pr.ZIP)
MARGIN, EXCUSED_SHARE = 1e-9, 1e-4          # tests/pff_cases.py's rule for the discrete draws


def _model(name, family, d, P, N, H, seed, irregular=True):
    """A dense G, F with every entry nonzero, the grid (irregular: dt = 0 first and in the middle, three G), a cloud around the family's
    level, positive weights, and the common keywords of the runs."""
    rng = np.random.default_rng(7000 + 7919 * seed + sum(map(ord, name)))
    G0, Wfull, F = pc.dense_model(d, rng)
    G, gi, dt = pc.time_grid(dict(T=H, irregular=irregular), G0, dt0=1.0)
    shift = np.zeros(d); shift[0] = pc.FAMILY_LEVEL[family] / F[0]
    cloud = shift[None, :, None] + 0.3 * rng.standard_normal((N, d, P))
    weights = rng.uniform(0.1, 1.0, (N, P))
    nu = 5.0 + np.arange(N) if family == pr.STUDENTT else None
    kw = dict(F=F, G=G, g_index=gi, dt=dt, family=family, nu=nu, seed=50 + seed, series_offset=3, iteration=5, P=P, literal=False,
              y=np.full((N, H), np.nan), m0=np.zeros(d), C0=np.eye(d))
    return rng, kw, cloud, weights, np.diag(Wfull).copy()


@functools.lru_cache(maxsize=None)
def anchor(name):
    """Every particle carries diag(W) and V: (the keywords of pff_cases.forecast_run with that W, the cloud, the weights, pw, pv)."""
    c = next(c for c in ANCHOR if c["name"] == name)
    rng, kw, cloud, weights, wd = _model(name, c["family"], c["d"], c["P"], c["N"], ANCHOR_H, c["seed"])
    V = pc.FAMILY_V[c["family"]]
    kw = dict(kw, W=np.diag(wd), V=V)
    pw = np.broadcast_to(wd[None, :, None], cloud.shape).copy()
    return kw, cloud, weights, pw, np.full(weights.shape, V)


@functools.lru_cache(maxsize=None)
def draws_case(family_name, kind):
    """A cloud whose particles carry unequal rows of the given kind, with entry weights: (kw, cloud, weights, pw, pv or None, shapes or None).
    pv of the count families is no variance: with the kinds other than "var" they take the shared V."""
    f = pc.FAMILY_NAMES.index(family_name)
    name = f"draws-{family_name}-{kind}"
    rng, kw, cloud, weights, wd = _model(name, f, 2, 128, 3, 5, 10 + f)
    N, d, P = cloud.shape
    V = pc.FAMILY_V[f]
    kw = dict(kw, V=V, W=np.diag(wd))
    jit_w, jit_v = np.exp(0.4 * rng.standard_normal((N, d, P))), np.exp(0.2 * rng.standard_normal((N, P)))
    scale_family = f in lr.SCALE_FAMILIES
    shapes = None
    if kind == "var":
        pw, pv = wd[None, :, None] * jit_w, (V * jit_v if scale_family else np.full((N, P), V))
    elif kind == "logvar":
        pw, pv = np.log(wd[None, :, None] * jit_w), (np.log(V * jit_v) if scale_family else None)
    else:
        shapes = np.array([[0.7, 3.5, 6.0], [2.5, 0.9, 4.0], [8.0, 1.5, 5.0]])[:N]          # (shapes below 1: the Gamma's boost)
        if f == pr.BETA:
            shapes = shapes + 3.0          # (a state noise without a variance walks eta out of the range where a Beta with this variance exists)
        pw = wd[None, :, None] * jit_w * (np.maximum(shapes[:, :d], 1.2) - 1.0)[:, :, None]
        pv = V * jit_v * (shapes[:, d] - 1.0)[:, None] if scale_family else None
        if f == pr.BETA:
            pv = pv * 0.05          # (a Beta variance has to stay below mean (1 - mean): the InverseGamma's tail must not reach it)
    return kw, cloud, weights, pw, pv, shapes


def restated(kw, cloud, pw, pv, *, kind, shapes=None, weights=None, slot_offset=0, H=None, mutant=None):
    """pffl_restatement.forecast on a case's keywords."""
    return lr.forecast(F=kw["F"], G=kw["G"], g_index=kw["g_index"], dt=kw["dt"], family=kw["family"], cloud0=cloud, pw=pw, pv=pv, V=kw.get("V"),
                       var_kind=kind, shapes=shapes, weights0=weights, nu=kw["nu"], H=kw["y"].shape[1] if H is None else H, seed=kw["seed"],
                       series_offset=kw["series_offset"], iteration=kw["iteration"], slot_offset=slot_offset, mutant=mutant)


@functools.lru_cache(maxsize=None)
def draws_reference(family_name, kind):
    kw, cloud, weights, pw, pv, shapes = draws_case(family_name, kind)
    return restated(kw, cloud, pw, pv, kind=KINDS[kind], shapes=shapes, weights=weights, slot_offset=4)


@functools.lru_cache(maxsize=None)
def dims_case(d, P=64, N=2, H=2):
    """Every D once: Gaussian, log-variances with unequal rows, a dense G on the unit grid."""
    rng, kw, cloud, weights, wd = _model(f"dims-{d}-{P}", pr.GAUSSIAN, d, P, N, H, 100 + d, irregular=False)
    psi_w = -1.0 + 0.5 * rng.standard_normal((N, d, P))
    psi_v = 0.5 * rng.standard_normal((N, P))
    return dict(kw, V=1.0, W=np.eye(d)), cloud, weights, psi_w, psi_v


def learned_run(eng, kw, cloud, pw, pv, *, kind, shapes=None, weights=None, slot_offset=0, ranks=(), want_draws=True, device=False, flags=0):
    """Engine.pf_forecast_learned on a case's keywords -> NumPy arrays."""
    import torch
    N = cloud.shape[0]
    dev = lambda a: None if a is None else (torch.as_tensor(np.ascontiguousarray(a), device="cuda") if device else a)
    out = eng.pf_forecast_learned(pc.materialised(kw), pc.packed_params(kw, N), dev(cloud), dev(pw), dev(pv), family=kw["family"], var_kind=kind,
                                  shapes=shapes, weights=dev(weights), ranks=ranks, slot_offset=slot_offset, obs_param=kw.get("nu"),
                                  iteration=kw["iteration"], seed=kw["seed"], series_offset=kw["series_offset"], want_draws=want_draws, flags=flags)
    return {k: None if v is None else (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in out.items()}


def series(kw, lo, hi):
    """The series lo .. hi - 1 of a batch's keywords as a batch of its own."""
    cut = dict(kw, y=kw["y"][lo:hi], series_offset=kw["series_offset"] + lo)
    if kw.get("nu") is not None and np.ndim(kw["nu"]) == 1:
        cut["nu"] = kw["nu"][lo:hi]
    return cut


# ---- the exact conditional law with log-variances (Gaussian, polynomial(d)) ------------------------------------------------------------------
LOGVAR_N, LOGVAR_P, LOGVAR_H = 8, 128, 6


@functools.lru_cache(maxsize=None)
def logvar_law(d):
    """polynomial(d): F = e_1, G upper bidiagonal of ones; x_i, psi_w,i ~ N(-1, 0.5^2), psi_v,i ~ N(0, 0.5^2) drawn on the host."""
    rng = np.random.default_rng(400 + d)
    N, P, H = LOGVAR_N, LOGVAR_P, LOGVAR_H
    F = np.zeros(d); F[0] = 1.0
    G = np.eye(d) + np.diag(np.ones(d - 1), 1)
    cloud = rng.standard_normal((N, d, P))
    psi_w, psi_v = -1.0 + 0.5 * rng.standard_normal((N, d, P)), 0.5 * rng.standard_normal((N, P))
    kw = dict(F=F, G=G[None], g_index=None, dt=np.ones(H), family=pr.GAUSSIAN, nu=None, seed=21 + d, series_offset=5, iteration=1, P=P, literal=False,
              y=np.full((N, H), np.nan), m0=np.zeros(d), C0=np.eye(d), V=1.0, W=np.eye(d))
    return kw, cloud, psi_w, psi_v


def logvar_pvalues(d, draws):
    """Given the cloud, ytilde_h,i ~ N(F^T G^h x_i, F^T C_h,i F + v_i), C_h,i = G C_{h-1,i} G^T + diag(w_i), C_0 = 0: the Kolmogorov-Smirnov
    p-values of the probability integral transforms of draws [N][H][P] at h = 1 and h = H against the uniform law."""
    kw, cloud, psi_w, psi_v = logvar_law(d)
    G, F = kw["G"][0], kw["F"]
    N, _, P = cloud.shape
    w, v = np.exp(psi_w), np.exp(psi_v)
    m = np.transpose(cloud, (0, 2, 1))                  # [N][P][d]
    C = np.zeros((N, P, d, d))
    out = []
    for h in range(1, LOGVAR_H + 1):
        m = m @ G.T
        C = G @ C @ G.T
        C[:, :, np.arange(d), np.arange(d)] += np.transpose(w, (0, 2, 1))
        if h in (1, LOGVAR_H):
            sd = np.sqrt(np.einsum("i,npij,j->np", F, C, F) + v)
            u = stats.norm.cdf((draws[:, h - 1] - m @ F) / sd)
            out.append(float(stats.kstest(u.reshape(-1), "uniform").pvalue))
    return out


# ---- the exact law with InverseGamma scales, drawn once (d = 1, F = G = 1) -------------------------------------------------------------------------
IG_N, IG_P, IG_H, IG_SHAPE = 64, 256, 8, 1.5


@functools.lru_cache(maxsize=None)
def ig_law():
    rng = np.random.default_rng(500)
    N, P, H = IG_N, IG_P, IG_H
    cloud = rng.standard_normal((N, 1, P))
    bw, bv = np.exp(0.3 * rng.standard_normal((N, 1, P))), np.exp(0.3 * rng.standard_normal((N, P)))
    kw = dict(F=np.ones(1), G=np.ones((1, 1, 1)), g_index=None, dt=np.ones(H), family=pr.GAUSSIAN, nu=None, seed=31, series_offset=2, iteration=4,
              P=P, literal=False, y=np.full((N, H), np.nan), m0=np.zeros(1), C0=np.eye(1), V=1.0, W=np.eye(1))
    return kw, cloud, bw, bv, np.array([IG_SHAPE, IG_SHAPE])


def ig_pvalues(cloud_H, draws):
    """With w_i = b_i / Gamma(a, 1) held over the horizon, (x_H,i - x_0,i) / sqrt(H b_i / a) is Student-t with 2 a degrees of freedom, and
    (ytilde_H,i - x_H,i) / sqrt(bv_i / av) with 2 av: the Kolmogorov-Smirnov p-values of the two, from cloud_H [N][1][P] and draws [N][H][P]."""
    kw, cloud, bw, bv, shapes = ig_law()
    a, av = shapes
    tx = (cloud_H[:, 0] - cloud[:, 0]) / np.sqrt(IG_H * bw[:, 0] / a)
    ty = (draws[:, IG_H - 1] - cloud_H[:, 0]) / np.sqrt(bv / av)
    return [float(stats.kstest(tx.reshape(-1), stats.t(2.0 * a).cdf).pvalue), float(stats.kstest(ty.reshape(-1), stats.t(2.0 * av).cdf).pvalue)]


# ---- the Rao-Blackwellised state draw ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def state_draw_case(d, P=64, N=3):
    """Means and covariances with condition number <= 100 (eigenvalues log-uniform in [0.05, 5]) in the layout dlm_rb_batch leaves."""
    rng = np.random.default_rng(600 + d)
    means = rng.standard_normal((N, d, P))
    covs = np.empty((N, d * (d + 1) // 2, P))
    for n in range(N):
        for i in range(P):
            q, _ = np.linalg.qr(rng.standard_normal((d, d)))
            C = (q * np.exp(rng.uniform(np.log(0.05), np.log(5.0), d))) @ q.T
            C = 0.5 * (C + C.T)
            covs[n, :, i] = C[np.tril_indices(d)]
    return means, covs
