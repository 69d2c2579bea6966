"""The shared RTS tables are kept across calls and reused where nothing they were computed from has changed.

J_t and S_t (`RtsTabs::jrows`, `srec`, `need`, the zero series' status) are a function of d, T, F, G, V, W, C0 and the semantics, not of the
data.  The engine keeps those of the last call that made them together with a copy of every byte the two one-wave kernels read, and a later call
uses them when `k_rts_key_check` finds that copy equal to its own inputs, byte for byte, on the device.  `dlm_last_table_reuse` tells what a call
did: built (a miss), reused (a hit), skipped (most series have a gap: no tables, the kept ones untouched), none (another route).

Every comparison here is equality of bits of the whole `filt` / `smooth` / `status` with the same call under `DLM_OPT_NO_TABLE_REUSE` on a fresh
engine, and every call's hit or miss is asserted."""
import numpy as np
import pytest

from bayesian_dlms_amd import _lib
from bayesian_dlms_amd.dlm import Dlm, DlmParameters, materialise

pytestmark = pytest.mark.gpu

TB = _lib.OPT_NO_SMALL_BATCH          # (the route starts at 6144 / 2048 series; the flag takes a few hundred there)
Q1 = _lib.OPT_SMOOTHER_COMPAT_Q1
NONE, BUILT, REUSED, SKIPPED = _lib.TABLES_NONE, _lib.TABLES_BUILT, _lib.TABLES_REUSED, _lib.TABLES_SKIPPED
W_C2 = np.array([0.01, 0.2, 0.4, 0.5, 0.2, 0.1, 0.4, 0.2, 0.4, 0.5, 0.2, 0.1, 0.4])
N0 = 300


def new_engine():
    from bayesian_dlms_amd.engine import Engine
    return Engine(0)


@pytest.fixture()
def eng():
    e = new_engine()
    yield e
    e.close()


def c2(T=200):
    mat = materialise(Dlm.polynomial(1) + Dlm.seasonal(24, 6), np.arange(1, T + 1, dtype=np.float64))
    return mat, DlmParameters([[1.0]], np.diag(W_C2), np.zeros(13), np.eye(13))


def ring(d, T=200, g=0.7, f_last=1.0):
    Gm = g * np.eye(d) + 0.25 * np.roll(np.eye(d), 1, axis=1)
    Fv = np.ones((d, 1)); Fv[1::2] = 0.5; Fv[d - 1, 0] = f_last
    mat = materialise(Dlm(lambda t: Fv, lambda dt: Gm), np.arange(1, T + 1, dtype=np.float64))
    return mat, DlmParameters([[0.7]], np.diag(np.linspace(0.1, 0.5, d)), np.zeros(d), np.eye(d))


def data(N, T, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, T, 1)).cumsum(axis=1) * 0.3 + rng.standard_normal((N, T, 1))


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def same(a, b, what):
    a, b = host(a), host(b)
    assert a.shape == b.shape, what
    if np.array_equal(a, b, equal_nan=True):
        return
    ne = np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))
    raise AssertionError(f"{what}: {len(ne)} values differ; first at {ne[0].tolist()}: {a[tuple(ne[0])]!r} vs {b[tuple(ne[0])]!r}")


def reference(mat, p, y, flags, want_filt=True):
    """The same call with DLM_OPT_NO_TABLE_REUSE on a fresh engine: its tables are made in that call."""
    e = new_engine()
    try:
        out = e.filter_smooth(mat, p, y, flags=flags | _lib.OPT_NO_TABLE_REUSE, want_filt=want_filt)
        assert e.last_table_reuse() in (BUILT, SKIPPED, NONE)
        return {k: (None if v is None else np.array(host(v))) for k, v in out.items()}
    finally:
        e.close()


def call(eng, mat, p, y, flags, expect, what, want_filt=True, variant="sparse16-rts-shared"):
    out = eng.filter_smooth(mat, p, y, flags=flags, want_filt=want_filt)
    got = eng.last_table_reuse()
    print(f"{what}: variant {eng.last_variant}, tables {got} (expected {expect})")
    assert eng.last_variant == variant, (what, eng.last_variant)
    assert got == expect, f"{what}: dlm_last_table_reuse = {got}, expected {expect}"
    ref = reference(mat, p, y, flags, want_filt)
    if want_filt:
        same(out["filt"], ref["filt"], what + ": filtered records")
    same(out["smooth"], ref["smooth"], what + ": smoothed records")
    same(out["status"], ref["status"], what + ": status")
    return out


@pytest.mark.parametrize("sem,want_filt", [(0, True), (Q1, True), (0, False), (Q1, False)])
def test_new_data_under_the_same_parameters_is_a_miss_then_a_hit(eng, sem, want_filt):
    mat, p = c2()
    call(eng, mat, p, data(N0, mat.T, 1), sem | TB, BUILT, "first call", want_filt)
    call(eng, mat, p, data(N0, mat.T, 2), sem | TB, REUSED, "new data", want_filt)
    call(eng, mat, p, data(N0 + 37, mat.T, 3), sem | TB, REUSED, "new data, another batch size", want_filt)


def test_no_table_reuse_builds_afresh_and_keeps_nothing(eng):
    mat, p = c2()
    call(eng, mat, p, data(N0, mat.T, 1), TB, BUILT, "first call")
    call(eng, mat, p, data(N0, mat.T, 2), TB | _lib.OPT_NO_TABLE_REUSE, BUILT, "opt-out")
    call(eng, mat, p, data(N0, mat.T, 3), TB, BUILT, "after the opt-out: nothing was kept")
    call(eng, mat, p, data(N0, mat.T, 4), TB, REUSED, "again")


def test_every_single_change_of_what_the_tables_depend_on_is_a_miss(eng):
    """One entry of W, V, C0 moved by one unit in the last place, one entry of G (same sparsity pattern), F, T, d, the semantics -- each against
    the call before it; then back to the first set: a miss (the kept tables are the last call's), then a hit."""
    mat, p = ring(9)
    d = mat.d
    y = data(N0, mat.T, 5)
    call(eng, mat, p, y, TB, BUILT, "first set")
    call(eng, mat, p, y, TB, REUSED, "first set again")

    def bump(a, idx):
        b = np.array(a, dtype=np.float64, copy=True)
        b[idx] = np.nextafter(b[idx], np.inf)
        return b
    pw = DlmParameters(p.v, bump(p.w, (d - 1, d - 1)), p.m0, p.c0)
    call(eng, mat, pw, y, TB, BUILT, "one entry of W, last bit")
    call(eng, mat, pw, y, TB, REUSED, "that W again")
    pv = DlmParameters(bump(p.v, (0, 0)), pw.w, p.m0, p.c0)
    call(eng, mat, pv, y, TB, BUILT, "V, last bit")
    pc = DlmParameters(pv.v, pw.w, p.m0, bump(p.c0, (3, 3)))
    call(eng, mat, pc, y, TB, BUILT, "one entry of C0, last bit")
    pc2 = DlmParameters(pv.v, pw.w, p.m0, bump(pc.c0, (0, d - 1)))      # an off-diagonal entry, from zero to the smallest subnormal
    call(eng, mat, pc2, y, TB, BUILT, "one off-diagonal entry of C0")
    call(eng, mat, pc2, y, TB, REUSED, "the same again")
    matg, _ = ring(9, g=np.nextafter(0.7, 1.0))
    call(eng, matg, pc2, y, TB, BUILT, "one value of G, the same sparsity pattern")
    matf, _ = ring(9, g=np.nextafter(0.7, 1.0), f_last=np.nextafter(1.0, 2.0))
    call(eng, matf, pc2, y, TB, BUILT, "one entry of F, last bit")
    call(eng, matf, pc2, y, TB, REUSED, "the same again")
    matT, _ = ring(9, T=mat.T - 1)
    call(eng, matT, p, y[:, :-1], TB, BUILT, "T")
    call(eng, mat, p, y, TB, BUILT, "T back (first set)")
    call(eng, mat, p, y, TB | Q1, BUILT, "textbook -> literal Q1")
    call(eng, mat, p, y, TB | Q1, REUSED, "literal Q1 again")
    call(eng, mat, p, y, TB, BUILT, "literal Q1 -> textbook")
    mat8, p8 = ring(8)
    call(eng, mat8, p8, y, TB, BUILT, "d")
    call(eng, mat, p, y, TB, BUILT, "back to the first set: a miss")
    call(eng, mat, p, y, TB, REUSED, "and a hit")


def test_per_series_prior_means_and_new_data_alone_are_hits(eng):
    from bayesian_dlms_amd.engine import pack_params
    mat, p = c2()
    N = N0
    call(eng, mat, p, data(N, mat.T, 6), TB, BUILT, "first call")
    V, vs, W, ws, m0, ms, C0, cs, vts, wts = pack_params(p, N)
    m0s = np.random.default_rng(7).standard_normal((N, 13))
    packed = (V, 0, W, 0, m0s.reshape(-1), 13, C0, 0, 0, 0)
    call(eng, mat, packed, data(N, mat.T, 8), TB, REUSED, "per-series m0, new data")
    call(eng, mat, p, data(N, mat.T, 9), TB, REUSED, "shared m0 again, new data")


def test_what_may_come_between_two_hits(eng):
    """Other users of the engine between two calls of one parameter set: none of them costs the tables, none of them sees stale ones."""
    import torch
    from bayesian_dlms_amd.engine import EngineError
    mat, p = c2()
    T = mat.T
    call(eng, mat, p, data(N0, T, 10), TB, BUILT, "first call")
    call(eng, mat, p, data(N0, T, 11), TB, REUSED, "second call")
    # the backward sampler's shared factors (the workspace the tables used to share)
    out = eng.ffbs(mat, p, data(N0, T, 12), seed=3, flags=TB)
    assert eng.last_variant == "sparse16-sampler-shared", eng.last_variant
    assert np.all(np.asarray(out["status"]) == 0)
    call(eng, mat, p, data(N0, T, 13), TB, REUSED, "after dlm_ffbs_batch")
    # most series with a gap: no tables, the kept ones untouched
    yg = data(N0, T, 14)
    yg[: N0 // 2 + 1, 40, 0] = np.nan
    call(eng, mat, p, yg, TB, SKIPPED, "gap-majority call")
    call(eng, mat, p, data(N0, T, 15), TB, REUSED, "after the gap-majority call")
    # gaps in a few series: a hit, those series by the per-series kernel
    yf = data(N0, T, 16)
    yf[3, 50:60, 0] = np.nan; yf[N0 - 1, T - 1, 0] = np.nan; yf[17, 0, 0] = np.nan
    eng.filter_smooth(mat, p, yf, flags=TB | _lib.OPT_COUNT_STEPS)
    assert eng.last_counters()[2:] == (N0 - 3, 3) and eng.last_table_reuse() == REUSED
    call(eng, mat, p, yf, TB, REUSED, "gaps in three series")
    # a batch below the threshold: another route
    call(eng, mat, p, data(40, T, 17), 0, NONE, "a batch below the threshold", variant="sparse16")
    call(eng, mat, p, data(N0, T, 18), TB, REUSED, "after the small batch")
    # an error exit behind the table launches
    with pytest.raises(EngineError):
        eng.filter_smooth(mat, p, data(N0, T, 19), flags=TB | _lib.OPT_TEST_FAIL_AFTER_TABLES)
    call(eng, mat, p, data(N0, T, 20), TB, REUSED, "after DLM_OPT_TEST_FAIL_AFTER_TABLES")
    # ... and one that fails while it is building other tables: they are complete and valid afterwards (the stream was joined)
    mat2, p2 = c2(T + 50)
    with pytest.raises(EngineError):
        eng.filter_smooth(mat2, p2, data(N0, T + 50, 21), flags=TB | _lib.OPT_TEST_FAIL_AFTER_TABLES)
    call(eng, mat2, p2, data(N0, T + 50, 22), TB, REUSED, "the tables a failing call made")
    call(eng, mat, p, data(N0, T, 23), TB, BUILT, "first set after them")
    # a DLM_OPT_ASYNC pair, device memory
    ya, yb = (torch.as_tensor(data(N0, T, s), device="cuda:0") for s in (24, 25))
    oa = eng.filter_smooth(mat, p, ya, flags=TB | _lib.OPT_ASYNC)
    ob = eng.filter_smooth(mat, p, yb, flags=TB | _lib.OPT_ASYNC)
    eng.sync()
    assert eng.last_table_reuse() == REUSED
    for o, yy in ((oa, ya), (ob, yb)):
        ref = reference(mat, p, yy, TB)
        for k in ("filt", "smooth", "status"):
            same(o[k], ref[k], "asynchronous pair: " + k)
    call(eng, mat, p, torch.as_tensor(data(N0, T, 26), device="cuda:0"), TB, REUSED, "device memory")
    call(eng, mat, p, data(N0, T, 27), TB, REUSED, "host memory")


def test_asynchronous_miss_then_hit_without_a_host_wait_in_between(eng):
    import torch
    mat, p = c2(150)
    ya, yb = (torch.as_tensor(data(N0, mat.T, s), device="cuda:0") for s in (30, 31))
    oa = eng.filter_smooth(mat, p, ya, flags=TB | _lib.OPT_ASYNC)       # builds
    ob = eng.filter_smooth(mat, p, yb, flags=TB | _lib.OPT_ASYNC)       # its key check runs behind the first call's commit
    eng.sync()
    assert eng.last_table_reuse() == REUSED
    for o, yy in ((oa, ya), (ob, yb)):
        ref = reference(mat, p, yy, TB)
        for k in ("filt", "smooth", "status"):
            same(o[k], ref[k], "asynchronous miss then hit: " + k)


def test_a_larger_T_after_a_smaller_one_and_back(eng):
    """The workspace is re-sized for the larger T (the kept tables go with the old one), and carved anew for the smaller."""
    small, ps = c2(100)
    large, pl = c2(450)
    call(eng, small, ps, data(N0, 100, 40), TB, BUILT, "T = 100")
    call(eng, large, pl, data(N0, 450, 41), TB, BUILT, "T = 450: the workspace grows")
    call(eng, large, pl, data(N0, 450, 42), TB, REUSED, "T = 450 again")
    call(eng, small, ps, data(N0, 100, 43), TB, BUILT, "T = 100 in the larger workspace")
    call(eng, small, ps, data(N0, 100, 44), TB, REUSED, "T = 100 again")
    call(eng, large, pl, data(N0, 450, 45), TB, BUILT, "T = 450 once more")


def test_full_size_c2_miss_then_hit_by_digest():
    """The bench workload (10 000 series x T = 1000, d = 13) on the device: the second call reuses the first call's tables; both against
    DLM_OPT_NO_TABLE_REUSE on a fresh engine, by per-record digests of the whole outputs (tests/counted_waits_cases.py: digest)."""
    import os
    import sys
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from counted_waits_cases import digest
    from bench import seasonal_c2, simulate
    mod, p = seasonal_c2()
    mat = materialise(mod, np.arange(1, 1001, dtype=np.float64))
    e, fresh = new_engine(), new_engine()
    try:
        for seed, expect in ((20261101, BUILT), (20261102, REUSED)):
            y = torch.as_tensor(simulate(mat, p, 10000, seed=seed), device="cuda:0")
            out = e.filter_smooth(mat, p, y)
            got = e.last_table_reuse()
            print(f"full size, seed {seed}: tables {got} (expected {expect})")
            assert e.last_variant == "sparse16-rts-shared" and got == expect, (e.last_variant, got)
            dg = {k: digest(out[k]) for k in ("filt", "smooth", "status")}
            del out
            torch.cuda.empty_cache()
            ref = fresh.filter_smooth(mat, p, y, flags=_lib.OPT_NO_TABLE_REUSE)
            assert fresh.last_table_reuse() == BUILT
            for k in ("filt", "smooth", "status"):
                assert np.array_equal(dg[k], digest(ref[k])), k
            del ref, y
            torch.cuda.empty_cache()
    finally:
        e.close(); fresh.close()
        torch.cuda.empty_cache()
