"""Every sampler kernel's draws against the dense joint posterior (tests/joint_posterior.py): the case table of the host test
through Engine.ffbs (dlm_ffbs_batch, dlm_backward_sample_batch), Engine.svd_ffbs and Engine.ar1_ffbs with injected normals.

One engine call per case: N = n_normals + 1 series that share y and all parameters, z = [0; I], so that theta = s + L z gives s
and L; s must be the smoothing mean of the whole path and L L^T its full joint covariance, from 50-digit dense linear algebra.
The bound is relative to the oracle's own error on the same case, e_kernel <= 100 max(e_oracle, n 2^-53) with n the length of the
stacked path: kernel and oracle evaluate the same recursions in fp64 and differ in operation order, FMA contraction, MFMA
accumulation order and the device's exp / sqrt, which moves a result by a small multiple of the same conditioning-driven error;
what the test exists to catch is >= 1e-3.  The measured table is in profiles/r10_notes.md."""
import os
import sys

import numpy as np
import pytest

import oracle
from bayesian_dlms_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import joint_posterior as jp  # noqa: E402

pytestmark = pytest.mark.gpu
FACTOR = 100.0


@pytest.fixture(scope="module")
def eng():
    from bayesian_dlms_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def kernel_affine_map(eng, case, device=False):
    """(s, L, route, status, counters) of the case's kernel: one call on n_normals + 1 series."""
    if device:
        import torch
        put = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")
    else:
        put = lambda a: a
    info = {}

    def draw(z):
        N = z.shape[0]
        if case.kind in ("ar1", "ou"):
            T = case.y.size
            v = np.tile(case.v, (N, 1)) if case.per_series == "v" else case.v
            sv = np.tile(np.asarray(case.sv, dtype=np.float64), (N, 1)) if case.per_series == "sv" else np.asarray(case.sv, dtype=np.float64)
            out = eng.ar1_ffbs(put(np.tile(case.y, (N, 1))), v, sv, z=put(z.reshape(N, T + 1)), times=case.times)
        else:
            mat, p = case.mat, case.p
            d, q, T = mat.d, mat.p, mat.T
            y = put(np.tile(case.y.reshape(1, T, q), (N, 1, 1)))
            zz = put(z.reshape(N, T + 1, -1))
            if case.kind == "svd":
                out = eng.svd_ffbs(mat, p, y, z=zz, flags=case.flags)
            elif case.entry == "records":
                out = eng.ffbs(mat, p, y, z=zz, flags=case.flags, filt=eng.filter(mat, p, y)["filt"])
            else:
                out = eng.ffbs(mat, p, y, z=zz, flags=case.flags | (_lib.OPT_COUNT_STEPS if case.own is not None else 0),
                               want_filt=case.entry != "no_filt")
        info["route"], info["status"] = eng.last_variant, _host(out["status"])
        info["counters"] = eng.last_counters()[2:] if case.own is not None else None     # (series on the shared factors, series on their own)
        return _host(out["theta"]).reshape(N, -1)

    s, L = jp.affine_map(draw, case.n_normals)
    return s, L, info["route"], info["status"], info["counters"]


def measure_case(eng, case, device=False):
    """The figures of one case: route, status, (e_mean, e_cov) of the kernel and of the oracle's construction, the bounds."""
    mean, cov, _ = case.reference()
    s, L, route, status, counters = kernel_affine_map(eng, case, device)
    e_kernel = jp.measure(s, L, mean, cov)
    e_oracle = jp.measure(*jp.affine_map(case.oracle_draw(), case.n_normals), mean, cov)
    floor = case.n_state * 2.0 ** -53
    bound = tuple(FACTOR * max(e, floor) for e in e_oracle)
    print(f"{case.name:40s} {'device' if device else 'host':6s} {route:24s} e_kernel {e_kernel[0]:.2e} {e_kernel[1]:.2e}  "
          f"e_oracle {e_oracle[0]:.2e} {e_oracle[1]:.2e}  bound {bound[0]:.2e} {bound[1]:.2e}")
    return {"route": route, "status": status, "counters": counters, "e_kernel": e_kernel, "e_oracle": e_oracle, "bound": bound}


def _assert_case(case, r):
    assert np.all(r["status"] == 0), (case.name, r["status"])
    assert r["route"] == case.route, (case.name, r["route"])
    if case.own is not None:
        N = case.n_normals + 1
        assert r["counters"] == ((0, N) if case.own else (N, 0)), (case.name, r["counters"])
    assert r["e_kernel"][0] <= r["bound"][0] and r["e_kernel"][1] <= r["bound"][1], (case.name, r["e_kernel"], r["e_oracle"], r["bound"])


@pytest.mark.parametrize("case", jp.CASES, ids=jp.CASE_IDS)
def test_kernel_draw_is_the_joint_posterior(eng, case):
    _assert_case(case, measure_case(eng, case))


@pytest.mark.parametrize("case", [c for c in jp.CASES if c.device], ids=lambda c: c.name)
def test_kernel_draw_is_the_joint_posterior_with_device_tensors(eng, case):
    _assert_case(case, measure_case(eng, case, device=True))


def measure_moments(eng, case):
    """Engine.filter_smooth and Engine.loglik of one series against the same dense reference: (e_s, e_S, e_loglik) of the engine
    and of the oracle, relative as in joint_posterior.measure (the log-likelihood relative to max(1, |loglik|))."""
    mat, p, y = case.mat, case.p, case.y
    d, q, T = mat.d, mat.p, mat.T
    mean, cov, ll = case.reference()
    scale_m, scale_c = max(1.0, np.abs(mean).max()), np.abs(cov).max()
    blocks = np.stack([cov[t * d:(t + 1) * d, t * d:(t + 1) * d] for t in range(T + 1)])

    def errs(s, S, loglik):      # S [T+1][d*d] column-major (symmetric: the order does not matter)
        return (float(np.abs(s.reshape(-1) - mean).max() / scale_m), float(np.abs(S.reshape(T + 1, d, d) - blocks).max() / scale_c),
                float(abs(loglik - ll) / max(1.0, abs(ll))))

    out = eng.filter_smooth(mat, p, y.reshape(1, T, q))
    route = eng.last_variant
    lk = eng.loglik(mat, p, y.reshape(1, T, q))
    status = np.concatenate([out["status"], lk["status"]])
    e_kernel = errs(out["smooth"][0, :, :d], out["smooth"][0, :, d:], float(lk["loglik"][0]))
    om = jp.omodel(mat)
    f = oracle.kf_filter(om, p.v, p.w, p.m0, p.c0, y)
    sm = oracle.smoother(om, f)
    e_oracle = errs(sm["s"], sm["S"], oracle.loglik(om, f, y))
    floor = case.n_state * 2.0 ** -53
    bound = tuple(FACTOR * max(e, floor) for e in e_oracle)
    print(f"{case.name:40s} {route:16s} s, S, loglik: e_kernel {e_kernel[0]:.2e} {e_kernel[1]:.2e} {e_kernel[2]:.2e}  "
          f"e_oracle {e_oracle[0]:.2e} {e_oracle[1]:.2e} {e_oracle[2]:.2e}")
    return {"route": route, "status": status, "e_kernel": e_kernel, "e_oracle": e_oracle, "bound": bound}


@pytest.mark.parametrize("case", jp.DLM_MODELS, ids=lambda c: c.name)
def test_smoother_and_loglik_are_the_dense_ones(eng, case):
    r = measure_moments(eng, case)
    assert np.all(r["status"] == 0)
    assert all(e <= b for e, b in zip(r["e_kernel"], r["bound"])), (case.name, r["e_kernel"], r["e_oracle"], r["bound"])
