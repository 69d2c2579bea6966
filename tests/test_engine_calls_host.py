"""Engine's one call path without a GPU or the library: every entry point that reaches a dlm_*_batch symbol is driven once against a
recording stub of the C ABI.  The stub holds each call to _lib.SYMBOLS (the symbol exists, the argument count matches, every argument
converts to its declared argtype), so a swapped or missing argument fails here and not on the device; and it records every address it
was handed -- the pointer arguments and the pointers inside a ModelDesc / ParamsDesc.

What is asserted: under DLM_OPT_ASYNC every array the C call was given the address of is reachable from Engine._keep until sync() -- the
inputs first (the assertion that names what went wrong where a method forgot one: a converted copy nobody else references goes back
to the allocator while the kernels may still read it), then every address, the outputs included; without the flag nothing is kept.
The inputs are float32, so `put` has to make the float64 copy that only the engine knows of."""
import ctypes

import numpy as np
import pytest

from bayesian_dlms_amd import _lib
from bayesian_dlms_amd.dglm import materialise_pf
from bayesian_dlms_amd.dlm import Dlm, DlmParameters, materialise
from bayesian_dlms_amd.engine import Engine

SYMBOLS = {name: (res, args) for name, res, args in _lib.SYMBOLS}
BATCH = {name for name in SYMBOLS if name.endswith("_batch")}
ASYNC = _lib.OPT_ASYNC
d, p, T, N, P, k = 2, 1, 6, 3, 64, 1          # the smallest legal shapes; the factor calls have p = 2, the knots B = 2 blocks


class Stub:
    """Every symbol of _lib.SYMBOLS as a function that checks its arguments against the declaration, records (name, arguments, addresses)
    and returns 0 (the two lengths: a small int)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name not in SYMBOLS:
            raise AttributeError(f"{name} is not a symbol of include/dlm_engine.h")
        res, argtypes = SYMBOLS[name]

        def call(*args):
            assert len(args) == len(argtypes), f"{name} takes {len(argtypes)} arguments, got {len(args)}"
            addresses = set()
            for i, (t, a) in enumerate(zip(argtypes, args)):
                try:
                    t.from_param(a)
                except (TypeError, ctypes.ArgumentError) as e:
                    raise AssertionError(f"{name}: argument {i} ({a!r}) is not a {t.__name__}: {e}") from None
                if t is ctypes.c_void_p:
                    addresses.add(a.value if isinstance(a, ctypes.c_void_p) else a)
                desc = getattr(a, "_obj", a)          # byref(struct), or the struct itself
                if isinstance(desc, (_lib.ModelDesc, _lib.ParamsDesc)):
                    addresses.update(getattr(desc, f) for f, ft in desc._fields_ if ft is ctypes.c_void_p)
            addresses.discard(None)
            self.calls.append((name, args, addresses))
            return 5 if name in ("dlm_stats_len", "dlm_packed_record_doubles") else 0
        return call

    def seen(self):
        return {name for name, _, _ in self.calls}

    def address(self, name, index):
        """The address the call `name` got as its argument `index` (0 is the handle)."""
        a = next(args for n, args, _ in self.calls if n == name)[index]
        return a.value if isinstance(a, ctypes.c_void_p) else a


def _engine():
    eng = Engine.__new__(Engine)
    eng.lib, eng.h, eng.device, eng._keep = Stub(), None, 0, []
    return eng


def _addresses(obj):
    """The data addresses of every NumPy array reachable through tuples, lists and dicts."""
    if isinstance(obj, np.ndarray):
        return {obj.ctypes.data}
    if isinstance(obj, (tuple, list, dict)):
        return set().union(*(_addresses(v) for v in (obj.values() if isinstance(obj, dict) else obj)))
    return set()


# ---- the inputs: float32, so that every one of them crosses as a copy that `put` made -------------------------------------------------------
f32 = lambda *shape: np.random.default_rng(len(shape) + sum(shape)).uniform(0.5, 1.5, shape).astype(np.float32)
MAT = materialise(Dlm.polynomial(d), np.arange(1.0, T + 1))
MAT_PF = materialise_pf(Dlm.polynomial(d), np.arange(1.0, T + 1))
MAT2 = materialise(Dlm.polynomial(1) * Dlm.polynomial(1), np.arange(1.0, T + 1))          # d = 2, p = 2: the factor models' panel
PAR = DlmParameters(np.eye(p), np.eye(d), np.zeros(d), np.eye(d))
Y, Y1, Y2, Z = f32(N, T, p), f32(N, T), f32(N, T, 2), f32(N, T + 1, d)
FILT, THETA, ALPHA, SV = f32(N, T + 1, d + d * d), f32(N, T + 1, d), f32(N, T + 1), f32(N, 3)
BETA, V2, ALPHA_K, F = f32(N, 2, k), f32(N, 2), f32(N, k, T + 1), f32(N, k, T)
TIMES, KNOTS = np.arange(1.0, T + 1, dtype=np.float32), np.array([0, 3, T + 1], dtype=np.int64)
PRIOR_W, PRIOR_V = f32(d, 2), f32(2)
pf = dict(n_particles=P, family=_lib.OBS_STUDENTT, obs_param=5.0)
learn = dict(n_particles=P, prior_v=PRIOR_V)

# name -> call(engine, flags); the entry points that take no flags (no DLM_OPT_ASYNC) are in SYNC_ONLY
CALLS = {
    "filter": lambda e, f: e.filter(MAT, PAR, Y, want_prior=True, want_fq=True, flags=f),
    "loglik": lambda e, f: e.loglik(MAT, PAR, Y, flags=f),
    "smooth": lambda e, f: e.smooth(MAT, PAR, FILT, flags=f),
    "filter_smooth": lambda e, f: e.filter_smooth(MAT, PAR, Y, flags=f),
    "ffbs": lambda e, f: e.ffbs(MAT, PAR, Y, z=Z, want_cond=True, flags=f),
    "ffbs(filt=...)": lambda e, f: e.ffbs(MAT, PAR, Y, z=Z, filt=FILT, flags=f),
    "svd_filter": lambda e, f: e.svd_filter(MAT, PAR, Y, flags=f),
    "svd_ffbs": lambda e, f: e.svd_ffbs(MAT, PAR, Y, z=Z, flags=f),
    "studentt_step": lambda e, f: e.studentt_step(MAT, Y1, THETA, f32(N, d + 3), (1.0, 2.0, 3.0, 4.0), f32(N), np.full(N, 4, np.int64),
                                                  iteration=0, flags=f),
    "sv_mixture": lambda e, f: e.sv_mixture(Y1, ALPHA, iteration=0, want_k=True, flags=f),
    "sv_params": lambda e, f: e.sv_params(ALPHA, SV, (0, 0) + (1.0,) * 8, iteration=0, flags=f),
    "sv_ou_params": lambda e, f: e.sv_ou_params(TIMES, ALPHA, SV, (0,) + (1.0,) * 10, iteration=0, flags=f),
    "fsv_factors": lambda e, f: e.fsv_factors(Y2, BETA, V2, ALPHA_K, iteration=0, flags=f),
    "fsv_loadings": lambda e, f: e.fsv_loadings(Y2, F, BETA, (0, 0.0, 1.0, 2.0, 1.0), iteration=0, v=V2, flags=f),
    "dlmfsv_center": lambda e, f: e.dlmfsv_center(MAT2, Y2, THETA, flags=f),
    "dlmfsv_impute": lambda e, f: e.dlmfsv_impute(Y2, BETA, V2, ALPHA_K, iteration=0, flags=f),
    "dlmfsv_variance": lambda e, f: e.dlmfsv_variance(BETA, V2, ALPHA_K, flags=f),
    "dlmfsvsys_innovations": lambda e, f: e.dlmfsvsys_innovations(MAT_PF, THETA, flags=f),          # (MAT_PF: it has a dt table too)
    "particle_filter": lambda e, f: e.particle_filter(MAT_PF, PAR, Y1, flags=f, **pf),
    "storvik_filter": lambda e, f: e.storvik_filter(MAT_PF, PAR, Y1, PRIOR_W, family=_lib.OBS_GAUSSIAN, flags=f, **learn),
    "lw_filter": lambda e, f: e.lw_filter(MAT_PF, PAR, Y1, PRIOR_W, a=0.9, flags=f, **dict(pf, **learn)),
    "rb_filter": lambda e, f: e.rb_filter(MAT_PF, PAR, Y1, PRIOR_W, a=0.9, flags=f, **learn),
    "pg_sweep": lambda e, f: e.pg_sweep(MAT, PAR, Y1, THETA, want_path_index=True, want_trace=True, want_step_weights=True, flags=f, **pf),
    "ar1_ffbs": lambda e, f: e.ar1_ffbs(Y1, f32(N, T), SV, z=f32(N, T + 1)),
    "ar1_ffbs(times=...)": lambda e, f: e.ar1_ffbs(Y1, 0.5, SV[0], times=TIMES),
    "sv_knots": lambda e, f: e.sv_knots(Y1, ALPHA, SV, KNOTS, iteration=0),
    "dinvgamma_step": lambda e, f: e.dinvgamma_step(d, p, f32(N, 2 * p + d + 1), (2.0, 1.0), (2.0, 1.0), iteration=0),
    "simulate": lambda e, f: e.simulate(MAT, PAR, N),
    "unpack_records": lambda e, f: e.unpack_records(d, f32(N, T + 1, 5)),
    "stats_pool": lambda e, f: e.stats_pool(f32(N, 5)),
}
SYNC_ONLY = {"ar1_ffbs", "ar1_ffbs(times=...)", "sv_knots", "dinvgamma_step", "simulate", "unpack_records", "stats_pool"}


@pytest.mark.parametrize("name", sorted(set(CALLS) - SYNC_ONLY))
def test_async_call_keeps_every_array_it_passed_until_sync(name):
    eng = _engine()
    result = CALLS[name](eng, ASYNC)
    kept, own = _addresses(eng._keep), _addresses(result)
    for symbol, _, addresses in eng.lib.calls:
        if symbol in BATCH:
            assert addresses, symbol
            # the inputs: what the call was given and the caller does not get back
            assert addresses - own <= kept, f"{name}: {symbol} may still be reading {len(addresses - own - kept)} input array(s) nothing keeps alive"
            assert addresses <= kept, f"{name}: {symbol} was handed {len(addresses - kept)} array(s) that Engine._keep does not hold"
    eng.sync()
    assert eng._keep == [] and "dlm_engine_sync" in eng.lib.seen()


@pytest.mark.parametrize("name", sorted(CALLS))
def test_synchronous_call_keeps_nothing(name):
    eng = _engine()
    CALLS[name](eng, 0)
    assert eng._keep == [] and eng.lib.seen() & (BATCH | {"dlm_unpack_records", "dlm_stats_pool"})


def _kept_and_lib(name):
    eng = _engine()
    CALLS[name](eng, ASYNC)
    return _addresses(eng._keep), eng.lib


# The five paths that let a converted input go before there was one call path: `put` made a float64 copy of the float32 input, the C
# call got its address (argument 3, 4 or 5; 0 is the handle), and the method did not hold it -- under DLM_OPT_ASYNC the copy could go
# back to the allocator with the kernels still to read it.  One assertion each.
def test_loglik_keeps_its_converted_y():
    kept, lib = _kept_and_lib("loglik")
    assert lib.address("dlm_loglik_batch", 3) in kept


def test_smooth_keeps_its_converted_filt():
    kept, lib = _kept_and_lib("smooth")
    assert lib.address("dlm_smooth_batch", 3) in kept


def test_svd_filter_keeps_its_converted_y():
    kept, lib = _kept_and_lib("svd_filter")
    assert lib.address("dlm_svd_filter_batch", 3) in kept


def test_svd_ffbs_keeps_its_converted_y_and_z():
    kept, lib = _kept_and_lib("svd_ffbs")
    assert {lib.address("dlm_svd_ffbs_batch", 3), lib.address("dlm_svd_ffbs_batch", 4)} <= kept


def test_backward_sampling_keeps_its_converted_filt():
    kept, lib = _kept_and_lib("ffbs(filt=...)")          # (y and z, arguments 3 and 5, were held; filt only came back in the dict)
    assert lib.address("dlm_backward_sample_batch", 4) in kept


def test_every_batch_symbol_is_reached_through_the_one_call_path():
    """A new entry point has to be added to CALLS; one that goes round Engine._call is not checked by its own arguments here."""
    seen = set()
    for name, call in CALLS.items():
        eng = _engine()
        call(eng, 0)
        seen |= eng.lib.seen()
    assert BATCH <= seen, sorted(BATCH - seen)
    assert len(BATCH) == 28 and {"dlm_backward_sample_batch", "dlm_ou_ffbs_batch", "dlm_unpack_records", "dlm_stats_pool"} <= seen


def test_stub_refuses_a_swapped_or_missing_argument():
    lib = Stub()
    md, pd, op = _lib.ModelDesc(), _lib.ParamsDesc(), _lib.Options()
    y = ctypes.c_void_p(Y.ctypes.data)
    assert lib.dlm_loglik_batch(None, md, pd, y, op, y, y) == 0
    with pytest.raises(AssertionError, match="takes 7 arguments, got 6"):
        lib.dlm_loglik_batch(None, md, pd, y, op, y)
    with pytest.raises(AssertionError, match="argument 1"):
        lib.dlm_loglik_batch(None, pd, md, y, op, y, y)
    with pytest.raises(AssertionError, match="argument 3"):
        lib.dlm_loglik_batch(None, md, pd, op, y, y, y)
    with pytest.raises(AttributeError):
        lib.dlm_no_such_batch
