"""Dynamic LDS above 64 KB is granted per function AND device (csrc/dlm_internal.h: launch, lds_opt_in): HIP keeps the attribute per
device, and a process may hold engines on several.  In one process an engine on device 0 and then one on device 1 each make the smallest
call that needs the grant on each path that has one; both must succeed and agree bit for bit.  (A process-wide one-shot asks on the first
engine's device only: the second engine's launch then fails.)  Skipped where the machine shows a single device."""
import numpy as np
import pytest

from bayesian_dlms_amd import _lib
from bayesian_dlms_amd.dlm import Dlm, DlmParameters, materialise

pytestmark = pytest.mark.gpu


def _calls():
    """name -> f(engine): the arrays of one call, as numpy (host-staged calls: nothing here lives on a device of its own)."""
    rng = np.random.default_rng(9)
    A = rng.standard_normal((17, 17)); G17 = 0.9 * A / np.abs(np.linalg.eigvals(A)).max()
    grid3 = np.arange(1, 4, dtype=np.float64)
    # k_svd_filter<48>, k_svd_sampler<48>: d = 17, p = 1, T = 3, N = 2
    F1 = rng.standard_normal((17, 1))
    svd_mat = materialise(Dlm(lambda t: F1, lambda dt: G17), grid3)
    svd_p = DlmParameters([[0.8]], np.eye(17) * 0.3, np.zeros(17), np.eye(17))
    svd_y = rng.standard_normal((2, 3, 1))
    # k_filter_tiled, k_smoother_tiled: a dense G at d = 17, T = 3, N = 2
    F3 = rng.standard_normal((17, 3))
    til_mat = materialise(Dlm(lambda t: F3, lambda dt: G17), grid3)
    til_p = DlmParameters(np.eye(3), np.eye(17) * 0.3, np.zeros(17), np.eye(17))
    til_y = rng.standard_normal((2, 3, 3))
    # k_spd_inverse_logdet at d = 64 (66 560 bytes), T = 2, N = 1
    mod = Dlm.polynomial(4)
    for _ in range(15):
        mod = mod + Dlm.polynomial(4)
    q7_mat = materialise(mod, np.arange(1, 3, dtype=np.float64))
    A2 = rng.standard_normal((64, 64))
    q7_p = DlmParameters([[0.8]], A2 @ A2.T / 64 + 0.2 * np.eye(64), np.zeros(64), np.eye(64))
    q7_y = rng.standard_normal((1, 2, 1))
    # the shared RTS route (its table run takes a whole CU's LDS): d = 2, T = 3, N = 5
    rts_mat = materialise(Dlm.polynomial(2), grid3)
    rts_p = DlmParameters([[1.3]], np.diag([0.5, 0.2]), np.zeros(2), np.eye(2))
    rts_y = rng.standard_normal((5, 3, 1))
    rts_flags = _lib.OPT_SMOOTHER_COMPAT_Q1 | _lib.OPT_NO_SMALL_BATCH | _lib.OPT_NO_LANE

    def svd(e):
        out = e.svd_ffbs(svd_mat, svd_p, svd_y, seed=5)
        assert e.last_variant == "svd-jacobi"
        return out

    def tiled(e):
        out = e.filter_smooth(til_mat, til_p, til_y)
        assert e.last_variant == "tiled-mfma"
        return out

    def q7(e):
        return e.loglik(q7_mat, q7_p, q7_y, flags=_lib.OPT_LOGLIK_LITERAL_Q7)

    def rts(e):
        out = e.filter_smooth(rts_mat, rts_p, rts_y, flags=rts_flags)
        assert e.last_variant == "sparse16-rts-shared"
        return out

    return {"svd": svd, "tiled": tiled, "loglik_q7": q7, "rts_shared": rts}


def test_an_engine_on_a_second_device_gets_its_own_lds_grants():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    from bayesian_dlms_amd.engine import Engine
    calls = _calls()
    results = []
    for dev in (0, 1):
        e = Engine(dev)
        try:
            results.append({name: f(e) for name, f in calls.items()})
        finally:
            e.close()
    for name in calls:
        first, second = results
        assert set(first[name]) == set(second[name])
        for key, a in first[name].items():
            if a is None:
                assert second[name][key] is None
                continue
            a, b = np.asarray(a), np.asarray(second[name][key])
            assert np.array_equal(a, b, equal_nan=True), (name, key)
