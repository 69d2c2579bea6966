"""The real library agrees with tests/test_engine_calls_host.py: the five calls that used to let a converted input go under DLM_OPT_ASYNC
give, from inputs that `put` has to convert (float32 device tensors, a NumPy z beside a device y), bit for bit what the same call gives
synchronously from float64 inputs -- with fresh torch tensors of the inputs' sizes allocated and filled before sync(), which is what
would take the memory of a copy that nothing held.  One pass: the deterministic check is the host test."""
import numpy as np
import pytest

from bayesian_dlms_amd import _lib
from bayesian_dlms_amd.dlm import Dlm, DlmParameters, materialise

pytestmark = pytest.mark.gpu


def test_async_calls_hold_their_converted_inputs_until_sync():
    import torch
    from bayesian_dlms_amd.engine import Engine
    d, T, N = 2, 6, 3
    mat = materialise(Dlm.polynomial(d), np.arange(1.0, T + 1))
    par = DlmParameters(np.eye(1), 0.1 * np.eye(d), np.zeros(d), np.eye(d))
    rng = np.random.default_rng(5)
    y32 = torch.as_tensor(rng.standard_normal((N, T, 1)).cumsum(axis=1), dtype=torch.float32, device="cuda:0")
    z = rng.standard_normal((N, T + 1, d))
    eng = Engine(0)
    try:
        y64 = y32.double()
        filt32 = eng.filter(mat, par, y64)["filt"].float()
        filt64 = filt32.double()
        calls = {"loglik": lambda y, filt, **kw: eng.loglik(mat, par, y, **kw),
                 "smooth": lambda y, filt, **kw: eng.smooth(mat, par, filt, **kw),
                 "svd_filter": lambda y, filt, **kw: eng.svd_filter(mat, par, y, **kw),
                 "svd_ffbs": lambda y, filt, **kw: eng.svd_ffbs(mat, par, y, z=z, **kw),
                 "ffbs(filt=...)": lambda y, filt, **kw: eng.ffbs(mat, par, y, z=z, filt=filt, **kw)}
        for name, call in calls.items():
            want = call(y64, filt64)
            got = call(y32, filt32, flags=_lib.OPT_ASYNC)
            fresh = [torch.full(shape, float("nan"), dtype=torch.float64, device="cuda:0")
                     for shape in (y32.shape, filt32.shape, z.shape) for _ in range(3)]
            eng.sync()
            assert eng._keep == [] and len(fresh) == 9
            assert list(got) == list(want) and int(want["status"].abs().sum().item()) == 0, name
            for key in want:          # (ffbs(filt=...) hands back the float64 records it read: they are an output like the others)
                if want[key] is None:
                    assert got[key] is None, f"{name}: {key}"
                else:
                    np.testing.assert_array_equal(got[key].cpu().numpy(), want[key].cpu().numpy(), err_msg=f"{name}: {key}")
    finally:
        eng.close()
