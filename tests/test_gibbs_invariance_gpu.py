"""Exact-invariance tests of the DLM and Student-t Gibbs samplers on the GPU (tests/gibbs_invariance.py has the method).

(V, W, theta, y) is drawn from the model's own joint law on the host; K sweeps of a sampler later the parameters must still follow
their priors and the whitened transitions and residuals must still be white -- exactly, with N independent replicates per call.
Unlike the draw-for-draw comparisons this does not depend on a restatement of the kernels: a mistake that kernel and restatement share
(a shape off by 1/2, a transition left out of ss, ss not divided by dt, a missing component counted in n, y_t paired with theta_t, a
Philox block used twice in an iteration) moves these laws by dozens of orders of magnitude in p (profiles/r13_notes.md).

Two drivers per case: the device-resident loop (Engine.ffbs -> Engine.dinvgamma_step on packed per-series parameters, the seed
arithmetic of gibbs_dinvgamma_device) and the host-draw drivers (GibbsSampling.sample / sample_svd, GibbsWishart.sample), which draw
V and W in NumPy from the kernel's statistics and so separate the statistics from the device Gamma draws."""
import os
import sys

import numpy as np
import pytest

from bayesian_dlms_amd.gibbs import GibbsSampling, GibbsWishart

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gibbs_invariance as gi  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 7


@pytest.fixture(scope="module")
def eng():
    from bayesian_dlms_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def starts():
    """The exact start of every case, made once and shared by its tests (never written to)."""
    out = {}

    def get(case, student=False):
        key = (case.name, student)
        if key not in out:
            out[key] = gi.st_exact_start(case, case.N) if student else gi.exact_start(case, case.N)
            for a in out[key].values():
                a.setflags(write=False)
        return out[key]
    return get


def _report(label, case, route, m):
    """One row of the table of profiles/r13_notes.md (shown with -s)."""
    print(f"| {label} | {route} | {m['N']} | {case.K} | {m['p_min']:.3g} | {m['dev_max']:.2f} |")


DEVICE_ROUTES = [(n, r) for n in gi.DIAGONAL_CASES for r in gi.CASES[n].routes]


@pytest.mark.parametrize("name,label", DEVICE_ROUTES, ids=[f"{n}-{r}" for n, r in DEVICE_ROUTES])
def test_device_resident_loop(eng, starts, name, label):
    import torch
    case = gi.CASES[name]
    flags, route = case.routes[label]
    start = starts(case)
    mat, d, p, N = case.mat, case.mat.d, case.mat.p, case.N
    dev = torch.device("cuda", 0)
    put = lambda a: torch.as_tensor(np.array(a, order="C"), device=dev)          # (a copy: the shared start is read-only)
    dense = lambda diag: put((diag[:, :, None] * np.eye(diag.shape[1])).reshape(N, -1))          # [N][n*n] dense diagonal matrices
    V, W = dense(start["V"]), dense(start["W"])
    m0, C0, y = put(case.m0), put(case.c0.T.reshape(-1)), put(start["y"])
    status = torch.zeros(N, dtype=torch.int32, device=dev)
    for it in range(case.K):
        last = it == case.K - 1
        packed = (V.reshape(-1), p * p, W.reshape(-1), d * d, m0, 0, C0, 0)
        out = eng.ffbs(mat, packed, y, seed=SEED * 1000003 + it, flags=flags, want_theta=last, want_stats=True, want_filt=False)
        assert eng.last_variant == route, (name, label, eng.last_variant)
        status |= out["status"]
        theta = out["theta"]
        V, W = eng.dinvgamma_step(d, p, out["stats"], case.prior_v, case.prior_w, iteration=it, seed=SEED)
    assert int(status.abs().max()) == 0, np.nonzero(status.cpu().numpy())[0][:8]
    diag = lambda M, n: M.reshape(N, n, n).diagonal(dim1=1, dim2=2).cpu().numpy()
    m = gi.checks(case, diag(V, p), diag(W, d), theta.cpu().numpy(), start["y"], start)
    _report(f"device loop {name}-{label}", case, route, m)


def _with_flags(eng, extra):
    return lambda mat, params, y, **kw: eng.ffbs(mat, params, y, **dict(kw, flags=kw["flags"] | extra))


# one row per (case, route) of the case table, plus sample_svd: the only place where the kernel's statistics row is compared with the
# helper's sums over the kernel's own theta
HOST_DRIVERS = ([(n, "wishart" if c.wishart else "sample", r) for n, c in gi.CASES.items() for r in c.routes] + [("c2", "sample_svd", None)])


@pytest.mark.parametrize("name,driver,label", HOST_DRIVERS, ids=[f"{n}-{d}-{r or 'svd'}" for n, d, r in HOST_DRIVERS])
def test_host_draw_driver(eng, starts, name, driver, label):
    case = gi.CASES[name]
    flags, route = case.routes[label] if label else (0, "svd-jacobi")
    start = starts(case)
    init = case.params_list(start["V"], start["W"])
    args = (case.mod, case.prior_v, case.prior_w, init, case.times, np.array(start["y"]), eng)
    if driver == "sample_svd":
        chain = GibbsSampling.sample_svd(*args, n_iter=case.K, seed=SEED, keep_theta=True)
    else:
        extra = flags & ~(gi._lib.OPT_STATS_OUTER | gi._lib.OPT_FFBS_SIMSMOOTH)          # (the driver sets those two itself)
        run = (GibbsWishart if driver == "wishart" else GibbsSampling).sample
        chain = run(*args, n_iter=case.K, seed=SEED, keep_theta=True, ffbs=_with_flags(eng, extra) if extra else None,
                    simulation_smoother=bool(flags & gi._lib.OPT_FFBS_SIMSMOOTH))
    n_states = 0
    for state in chain:
        assert eng.last_variant == route, (name, driver, eng.last_variant)
        assert (np.asarray(state.status) == 0).all(), np.nonzero(np.asarray(state.status))[0][:8]
        n_states += 1
    assert n_states == case.K and len(state.p) == case.N
    # the kernel's statistics are the sums of include/dlm_engine.h over the kernel's own theta (a handful of fp64 terms each: 1e-10)
    ssy, n, ss, outer, T = gi.statistics(case, np.asarray(state.theta), start["y"])
    body = outer.transpose(0, 2, 1).reshape(case.N, -1) if case.wishart else ss
    np.testing.assert_allclose(np.asarray(state.stats), np.concatenate([ssy, n, body, np.full((case.N, 1), T)], axis=1), rtol=1e-10, atol=1e-12)
    V = np.stack([np.diag(q.v) for q in state.p])
    W = np.stack([q.w if case.wishart else np.diag(q.w) for q in state.p])
    m = gi.checks(case, V, W, np.asarray(state.theta), start["y"], start)
    _report(f"{driver} {name}-{label or 'svd'}", case, route, m)


ST_ROUTES = [(n, r) for n, c in gi.ST_CASES.items() for r in c.routes]


@pytest.mark.parametrize("name,label", ST_ROUTES, ids=[f"{n}-{r}" for n, r in ST_ROUTES])
def test_studentt_with_the_scale_held_fixed(eng, starts, name, label):
    """Engine.ffbs with the V_t stream v and per-series W, then Engine.studentt_step with the same scale_in in every call (scale_out
    ignored): a partially collapsed Gibbs sampler of p(theta, W, nu, v | y, s), started from that law."""
    import torch
    case = gi.ST_CASES[name]
    flags, route = case.routes[label]
    start = starts(case, student=True)
    mat, d, T, N = case.mat, case.mat.d, case.mat.T, case.N
    dev = torch.device("cuda", 0)
    put = lambda a: torch.as_tensor(np.array(a, order="C"), device=dev)          # (a copy: the shared start is read-only)
    W = put((start["W"][:, :, None] * np.eye(d)).reshape(N, -1))
    v, nu, y = put(start["v"]), put(start["nu"]), put(start["y"])
    m0, C0, s = put(case.m0), put(case.c0.T.reshape(-1)), put(np.full(N, case.scale))
    status = torch.zeros(N, dtype=torch.int32, device=dev)
    for it in range(case.K):
        packed = (v.reshape(-1), T, W.reshape(-1), d * d, m0, 0, C0, 0, 1, 0)
        out = eng.ffbs(mat, packed, y, seed=SEED * 1000003 + it, flags=flags, want_theta=True, want_stats=True, want_filt=False)
        assert eng.last_variant == route, (name, label, eng.last_variant)
        theta = out["theta"]
        res = eng.studentt_step(mat, y, theta, out["stats"], case.prior, s, nu, iteration=it, seed=SEED)
        status |= out["status"] | res["status"]
        v, nu, W = res["v"], res["nu"], res["W"]
    assert int(status.abs().max()) == 0, np.nonzero(status.cpu().numpy())[0][:8]
    Wd = W.reshape(N, d, d).diagonal(dim1=1, dim2=2).cpu().numpy()
    m = gi.st_checks(case, nu.cpu().numpy(), Wd, v.cpu().numpy(), theta.cpu().numpy(), start["y"], start)          # (with the new-draw floors)
    _report(f"student-t {name}-{label}", case, route, m)
