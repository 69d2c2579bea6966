"""The two writers of a smoothed record on the shared RTS route: `k_rts_broadcast` writes S_t from the tables, beside
the forward pass, `k_mean_rts16` the 128-byte lines that hold s_t.  Which of the two writes a 16-byte piece depends on where the record
lies against the 128-byte lines of memory -- on the base address of the output, the series, the step and the record size -- so every
case here puts the output at several offsets into an allocation whose bytes are a NaN payload no result can have, with guards of the
same payload around it: afterwards no payload is left inside, both guards are whole, and the words are those of the per-series kernels."""
import numpy as np
import pytest
import torch

from bayesian_dlms_amd import _lib
from bayesian_dlms_amd.dlm import Dlm, DlmParameters, materialise

pytestmark = pytest.mark.gpu

NSB = _lib.OPT_NO_SMALL_BATCH | _lib.OPT_NO_LANE
SEMS = [0, _lib.OPT_SMOOTHER_COMPAT_Q1]
PAYLOAD = 0x7FF8DEAD0BADBEEF          # a quiet NaN with a payload: arithmetic makes the default NaN, never this one
GUARD = 4096
OFFSETS = (0, 16, 48, 112)
SHAPES = [(1, 1), (1, 5), (2, 3), (3, 4), (9, 7), (65, 6), (130, 37)]
W_C2 = np.array([0.01, 0.2, 0.4, 0.5, 0.2, 0.1, 0.4, 0.2, 0.4, 0.5, 0.2, 0.1, 0.4])


@pytest.fixture(scope="module")
def eng():
    from bayesian_dlms_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def model(d, T, wscale=1.0):
    """d = 13: the C2 model (two nonzeros per row of G); d = 6 and 15: three per row, as tests/test_shared_rts_gpu.py builds them.
    Records of 1456, 336 and 1920 bytes."""
    times = np.arange(1, T + 1, dtype=np.float64)
    if d == 13:
        mat = materialise(Dlm.polynomial(1) + Dlm.seasonal(24, 6), times)
        return mat, DlmParameters([[1.0]], np.diag(W_C2 * wscale), np.zeros(13), np.eye(13))
    rng = np.random.default_rng(80 + 16 * 3 + d)
    Gm = np.zeros((d, d))
    for i in range(d):
        for s_, cf in enumerate([0.6, 0.25, -0.2]):
            Gm[i, (i + s_) % d] += cf
    Fv = rng.choice([1.0, 0.0, 0.5, -0.5], size=d).reshape(-1, 1)
    Fv[0, 0] = 1.0
    mat = materialise(Dlm(lambda t: Fv, lambda dt: Gm), times)
    return mat, DlmParameters([[0.7]], np.diag(rng.uniform(0.1, 0.5, d) * wscale), rng.standard_normal(d), np.eye(d))


def series(T, N, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, T, 1)).cumsum(axis=1) * 0.3 + rng.standard_normal((N, T, 1))


def words(t):
    return t.contiguous().view(torch.int64)


class Guarded:
    """The smoothed records as a view that starts GUARD + offset bytes into one 256-byte-aligned allocation filled with PAYLOAD."""

    def __init__(self, N, T, rec, offset):
        self.nbytes = N * (T + 1) * rec * 8
        raw = torch.empty(GUARD + 256 + self.nbytes + GUARD + 256, dtype=torch.uint8, device="cuda:0")
        self.skew = (-raw.data_ptr()) % 256
        self.raw = raw
        self.all = raw[self.skew:self.skew + GUARD + 128 + self.nbytes + GUARD].view(torch.int64)
        self.all.fill_(PAYLOAD)
        self.start = self.skew + GUARD + offset
        self.offset = offset
        self.smooth = raw[self.start:self.start + self.nbytes].view(torch.float64).view(N, T + 1, rec)
        assert self.smooth.data_ptr() % 256 == offset

    def check(self, what):
        w0 = (GUARD + self.offset) // 8
        inside = self.all[w0:w0 + self.nbytes // 8]
        left = int((inside == PAYLOAD).sum().item())
        assert left == 0, f"{what}: {left} words of the output were never written; first at byte {8 * int(torch.nonzero(inside == PAYLOAD)[0].item())} of {self.nbytes}"
        assert bool((self.all[:w0] == PAYLOAD).all()), f"{what}: bytes in front of the output were written"
        assert bool((self.all[w0 + self.nbytes // 8:] == PAYLOAD).all()), f"{what}: bytes behind the output were written"


def same(a, b, what):
    a, b = words(a), words(b)
    if torch.equal(a, b):
        return
    ne = torch.nonzero(a != b)
    raise AssertionError(f"{what}: {len(ne)} words differ; first at {ne[0].tolist()}, last at {ne[-1].tolist()} of {list(a.shape)}; "
                         f"last index among {torch.unique(ne[:, -1])[:12].tolist()}")


def reference(eng, mat, p, y, sem, gaps=()):
    """What the parent's per-series kernels give, as tests/test_shared_rts_gpu.py builds it.  Literal Q1: the same call with
    DLM_OPT_SMOOTHER_PER_SERIES.  Textbook: dlm_smooth_batch (the per-series RTS kernel) on the call's filter records, and for a series with
    a gap the per-series information-form kernel's records."""
    own = eng.filter_smooth(mat, p, y, flags=sem | NSB | _lib.OPT_SMOOTHER_PER_SERIES)
    if sem:
        return own["smooth"]
    ref = eng.smooth(mat, p, own["filt"])["smooth"].clone()
    for n in gaps:
        ref[n] = own["smooth"][n]
    return ref


def shared_call(eng, mat, p, y, sem, offset, flags=0):
    N, T, rec = int(y.shape[0]), mat.T, mat.d + mat.d * mat.d
    g = Guarded(N, T, rec, offset)
    out = {"filt": torch.empty((N, T + 1, rec), dtype=torch.float64, device="cuda:0"), "smooth": g.smooth,
           "status": torch.empty((N,), dtype=torch.int32, device="cuda:0")}
    eng.filter_smooth(mat, p, y, flags=sem | NSB | _lib.OPT_COUNT_STEPS | flags, out=out)
    return g, out


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("d", [6, 13, 15])
def test_every_byte_is_written_once_at_every_line_phase(eng, d, sem):
    for T, N in SHAPES:
        mat, p = model(d, T)
        y = torch.as_tensor(series(T, N, 100 * T + N + d), device="cuda:0")
        ref = reference(eng, mat, p, y, sem)
        for offset in OFFSETS:
            what = f"d={d} T={T} N={N} offset={offset}"
            g, out = shared_call(eng, mat, p, y, sem, offset)
            assert eng.last_variant == "sparse16-rts-shared" and eng.last_counters()[2:] == (N, 0), (what, eng.last_variant, eng.last_counters())
            g.check(what)
            same(g.smooth, ref, what)
            assert int(out["status"].abs().sum().item()) == 0


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("d,T,N", [(13, 9, 13), (6, 9, 13), (15, 3, 12), (13, 130, 37)])
def test_routed_series_and_the_records_next_to_them(eng, d, T, N, sem):
    """Gaps in the first and the last series, in two adjacent ones and in a lone one in the middle: their records are the per-series kernels',
    and so are the first and last records of their neighbours -- the lines that the writers of two series meet on."""
    mat, p = model(d, T)
    yh = series(T, N, 7 * T + N + d)
    gaps = (0, N // 2 - 2, N // 2 - 1, N // 2 + 2, N - 1)
    for i, n in enumerate(gaps):
        yh[n, (i * 3) % T, 0] = np.nan
    y = torch.as_tensor(yh, device="cuda:0")
    ref = reference(eng, mat, p, y, sem, gaps)
    for offset in OFFSETS:
        what = f"d={d} T={T} N={N} offset={offset}"
        g, _ = shared_call(eng, mat, p, y, sem, offset)
        assert eng.last_counters()[2:] == (N - len(gaps), len(gaps)), (what, eng.last_counters())
        g.check(what)
        for n in gaps:
            same(g.smooth[n], ref[n], f"{what}: routed series {n}")
            for m in (n - 1, n + 1):
                if 0 <= m < N:
                    same(g.smooth[m, [0, T]], ref[m, [0, T]], f"{what}: first and last record of series {m}, next to routed series {n}")
        same(g.smooth, ref, what)


@pytest.mark.parametrize("sem", SEMS)
def test_first_call_repeat_call_and_changed_parameters(sem):
    """A fresh engine: the first call builds the tables (the broadcast starts behind the table run), the second finds them (it runs beside the
    forward pass), a third with another W builds again.  Each equals the call that keeps no tables, bit for bit."""
    from bayesian_dlms_amd.engine import Engine
    e, e2 = Engine(0), Engine(0)
    try:
        T, N, d = 130, 37, 13
        y = torch.as_tensor(series(T, N, 5), device="cuda:0")
        for wscale, want in ((1.0, _lib.TABLES_BUILT), (1.0, _lib.TABLES_REUSED), (1.5, _lib.TABLES_BUILT)):
            mat, p = model(d, T, wscale)
            g, _ = shared_call(e, mat, p, y, sem, 48)
            assert e.last_table_reuse() == want, (wscale, e.last_table_reuse())
            g.check(f"wscale={wscale}")
            g2, _ = shared_call(e2, mat, p, y, sem, 48, _lib.OPT_NO_TABLE_REUSE)
            same(g.smooth, g2.smooth, f"wscale={wscale}: against the call that keeps no tables")
            same(g.smooth, reference(e2, mat, p, y, sem), f"wscale={wscale}: against the per-series kernels")
    finally:
        e.close()
        e2.close()


@pytest.mark.parametrize("sem", SEMS)
def test_a_batch_whose_series_mostly_have_gaps_is_left_to_the_per_series_kernels(eng, sem):
    T, N, d = 65, 9, 13
    mat, p = model(d, T)
    yh = series(T, N, 11)
    gaps = tuple(range(5))
    for n in gaps:
        yh[n, 7 + n, 0] = np.nan
    y = torch.as_tensor(yh, device="cuda:0")
    own = eng.filter_smooth(mat, p, y, flags=sem | NSB | _lib.OPT_SMOOTHER_PER_SERIES)
    for offset in OFFSETS:
        g, _ = shared_call(eng, mat, p, y, sem, offset)
        assert eng.last_counters()[2:] == (0, N), eng.last_counters()
        g.check(f"offset={offset}")
        same(g.smooth, own["smooth"], f"offset={offset}")
