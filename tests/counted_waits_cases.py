"""Case matrix of tests/test_counted_waits_gpu.py: the default build against the one whose hand-counted vmcnt waits are drained.

Every LDS-DMA prefetch of the d <= 15 smoother, the shared-table routes and the SVD mean filter is waited for by a hand count
(vm_wait<N> in csrc/dlm_internal.h).  A count that is too large on some path reads an LDS slot before its DMA has landed and
returns a stale record without any fault.  libdlm_engine_drain.so (build.build_drain_variant, -DDLM_DRAIN_WAITS=1) waits
vmcnt(0) instead and is otherwise the same code (tests/test_counted_waits_host.py checks the code objects), so both builds must
give the same bits on every case below.

Each case names the kernel instantiations that the launchers' dispatch rules (restated here: rts_inst, mean_np, sampler_nr,
svd_ns, smoother_inst) send it to; tests/test_counted_waits_host.py compares that set with the symbol table of the code object.
Run as a script, the module runs the whole matrix on the library DLM_ENGINE_LIB names and writes one .npz per case to the
directory given, a .err for a case whose route assertion failed."""
import os
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters, materialise  # noqa: E402

PIPE_MAX = 3072          # DLM_PIPE_MAX (dlm_sparse16.hip, with_smoother_variant)
W_C2 = np.array([0.01, 0.2, 0.4, 0.5, 0.2, 0.1, 0.4, 0.2, 0.4, 0.5, 0.2, 0.1, 0.4])
CNT = _lib.OPT_COUNT_STEPS
EDGES = [(1, 5), (2, 3), (3, 1), (63, 4), (64, 6), (65, 7), (1000, 37)]   # (T, N): prologue / epilogue, the 64-step branch, long T


# ---- the launchers' dispatch rules -------------------------------------------------------------------------------------------
def rts_inst(d, K):            # launch_mean_rts (dlm_sampler16.hip)
    np_, nrs, nrj = (2, 1, 1) if d <= 7 else (4, 1, 2) if d <= 10 else (6, 2, 2) if d <= 13 else (8, 2, 2) if d == 14 else (8, 2, 3)
    return f"k_mean_rts16<{K}, {np_}, {nrs}, {nrj}>"


def mean_np(d):                # with_mean_np (dlm_sparse16.hip)
    return 4 if d <= 10 else 6 if d <= 13 else 8


def sampler_nr(d):             # launch_mean_sampler: ceil(17 d / 64) DMA instructions per table row
    return min(4, (17 * d + 63) // 64)


def svd_ns(d):                 # launch_svd_filter_shared: ceil(4 srec / 64), srec = 2 d + d^2
    ns = (4 * (2 * d + d * d) + 63) // 64
    return 4 if ns <= 4 else 8 if ns <= 8 else 13 if ns <= 13 else 18


def smoother_inst(K, irregular, N, flags):   # with_smoother_variant (dlm_sparse16.hip)
    b = lambda v: "true" if v else "false"
    if irregular:
        irr, pipe, plain = True, False, False
    elif (flags & _lib.OPT_NO_STEADY) and N > PIPE_MAX:
        irr, pipe, plain = False, False, True
    elif N <= PIPE_MAX and not (flags & _lib.OPT_NO_PIPE):
        irr, pipe, plain = False, True, False
    else:
        irr, pipe, plain = False, False, False
    return f"k_smoother_sp16<{K}, {b(irr)}, {b(pipe)}, {b(plain)}>"


# instantiations in the code object that no call reaches
UNREACHABLE = {
    "k_svd_mean_filter": "launched only in a -DDLM_SVD_MEAN_ONE_PER_WAVE build (diagnostic)",
    "k_mean_sampler_sp16<4, 1, false>": "NR = 1 means d <= 3: no row of a d x d G has four nonzeros",
    "k_mean_sampler_sp16<4, 1, true>": "NR = 1 means d <= 3: no row of a d x d G has four nonzeros",
}


# ---- models ------------------------------------------------------------------------------------------------------------------
def c2(T, irregular=False):
    times = np.cumsum(np.array([1.0, 2.0, 1.0] * (T // 3 + 1))[:T]) if irregular else np.arange(1, T + 1, dtype=np.float64)
    mat = materialise(Dlm.polynomial(1) + Dlm.seasonal(24, 6), times)
    return mat, DlmParameters([[1.0]], np.diag(W_C2), np.zeros(13), np.eye(13))


def ring(d, knz, T, seed, irregular=False):
    """d states, exactly min(knz, d) nonzeros in every row and column of G (K = min(knz, d))."""
    rng = np.random.default_rng(seed)
    knz = min(knz, d)
    Gm = np.zeros((d, d))
    for s_, cf in enumerate({1: [0.9], 2: [0.7, 0.25], 3: [0.6, 0.25, -0.2], 4: [0.5, 0.3, -0.2, 0.15]}[knz]):
        for i in range(d):
            Gm[i, (i + s_) % d] += cf
    Fv = rng.choice([1.0, 0.0, 0.5, -0.5], size=d).reshape(-1, 1)
    Fv[0, 0] = 1.0
    times = np.cumsum(np.array([1.0, 2.0, 1.0] * (T // 3 + 1))[:T]) if irregular else np.arange(1, T + 1, dtype=np.float64)
    mat = materialise(Dlm(lambda t: Fv, lambda dt: Gm), times)
    return mat, DlmParameters([[0.7]], np.diag(rng.uniform(0.1, 0.5, d)), rng.standard_normal(d), np.eye(d))


def band(d, T, seed):
    """A dense-enough model for the SVD filter (which takes any G)."""
    rng = np.random.default_rng(seed)
    Gm = 0.8 * np.eye(d) + 0.15 * np.eye(d, k=1)
    Fv = rng.standard_normal((d, 1))
    mat = materialise(Dlm(lambda t: Fv, lambda dt: Gm), np.arange(1, T + 1, dtype=np.float64))
    A = rng.standard_normal((d, d))
    return mat, DlmParameters([[0.9]], A @ A.T / d + 0.1 * np.eye(d), rng.standard_normal(d), np.eye(d) * 2)


def observations(N, T, seed, gaps):
    """A random walk plus noise; with gaps, series 1 misses t = T // 2 (and series 4 its first step, where N > 4)."""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((N, T, 1)).cumsum(axis=1) * 0.3 + rng.standard_normal((N, T, 1))
    ngap = 0
    if gaps and N > 1:
        y[1, T // 2, 0] = np.nan
        ngap = 1
        if N > 4:
            y[4, 0, 0] = np.nan
            ngap = 2
    return y, ngap


# ---- outputs: exact copies, or per-record digests computed on the device -----------------------------------------------------
def digest(x):
    """[..., R] -> [...] int64: a wrapping weighted sum of the 64-bit patterns of each record, odd weights (so that any one changed
    value changes the sum).  Computed on the device, in blocks of series."""
    import torch
    v = x.contiguous().view(torch.int64) if x.dtype == torch.float64 else x.to(torch.int64)
    if v.dim() == 1:
        return v.cpu().numpy()
    w = torch.arange(v.shape[-1], device=v.device, dtype=torch.int64) * 2 + 0x1E3779B97F4A7C15
    out = torch.empty(v.shape[:-1], dtype=torch.int64, device=v.device)
    for lo in range(0, v.shape[0], 256):
        out[lo:lo + 256] = (v[lo:lo + 256] * w).sum(dim=-1)
    return out.cpu().numpy()


def host(out, keys):
    return {k: (digest(out[k]) if not isinstance(out[k], np.ndarray) else np.array(out[k])) for k in keys if out[k] is not None}


def large(N, T, d):
    """A call whose record arrays would pass about 64 MB together on the host: it runs device-resident and is compared by digests."""
    return N * (T + 1) * (d + d * d) * 8 > 24e6


def on_device(y, big):
    if not big:
        return y
    import torch
    return torch.as_tensor(y, device="cuda:0")


def check_route(eng, variant, served=None, own=None, at_least=False):
    got = eng.last_variant
    assert got == variant, f"route {got!r}, expected {variant!r}"
    cnt = eng.last_counters()
    if served is not None:
        ok = (cnt[2] >= served and cnt[3] >= own) if at_least else (cnt[2] == served and cnt[3] == own)
        assert ok, f"counters {cnt}: expected {served} series on the shared kernels, {own} on their own ({'at least' if at_least else 'exactly'})"
    return np.array(cnt, dtype=np.uint64)


# ---- cases -------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, cid, claims, fn, T, N):
        self.id, self.claims, self.fn, self.T, self.N = cid, tuple(claims), fn, T, N

    def run(self, eng):
        return self.fn(eng)


def rts_case(cid, mat, p, K, N, seed, q1, gaps=True):
    y, ngap = observations(N, mat.T, seed, gaps)
    big = large(N, mat.T, mat.d)

    def fn(eng):
        fl = _lib.OPT_NO_SMALL_BATCH | _lib.OPT_NO_LANE | CNT | (_lib.OPT_SMOOTHER_COMPAT_Q1 if q1 else 0)
        out = eng.filter_smooth(mat, p, on_device(y, big), flags=fl)
        r = host(out, ("filt", "smooth", "status"))
        r["counters"] = check_route(eng, "sparse16-rts-shared", N - ngap, ngap)
        return r
    return Case(cid, [rts_inst(mat.d, K)], fn, mat.T, N)


def smoother_case(cid, mat, p, K, N, seed, flags=0, gaps=True, irregular=False):
    """The per-series fused filter + smoother (k_smoother_sp16): below 2048 series by default, above with DLM_OPT_SMOOTHER_PER_SERIES."""
    y, _ = observations(N, mat.T, seed, gaps)
    big = large(N, mat.T, mat.d)
    fl = flags | _lib.OPT_NO_LANE | CNT | (_lib.OPT_SMOOTHER_PER_SERIES if N >= 2048 else 0)

    def fn(eng):
        out = eng.filter_smooth(mat, p, on_device(y, big), flags=fl)
        r = host(out, ("filt", "smooth", "status"))
        r["counters"] = check_route(eng, "sparse16", 0, 0)
        return r
    return Case(cid, [smoother_inst(K, irregular, N, fl)], fn, mat.T, N)


def cov_case(cid, mat, p, K, N, seed, flags=0, gaps=True):
    """DLM_OPT_SHARED_COV: dlm_filter_batch (mean filter MODE 1), then the fused call (MODE 2, the covariance smoother, the mean smoother)."""
    y, ngap = observations(N, mat.T, seed, gaps)
    fl = flags | _lib.OPT_SHARED_COV | _lib.OPT_NO_LANE | CNT
    np_ = mean_np(mat.d)
    big = large(N, mat.T, mat.d)

    def fn(eng):
        f = host(eng.filter(mat, p, on_device(y, big), flags=fl), ("filt", "status"))
        r = {"filter_only_filt": f["filt"], "filter_only_status": f["status"], "filter_only_counters": check_route(eng, "sparse16", N - ngap, ngap)}
        out = eng.filter_smooth(mat, p, on_device(y, big), flags=fl)
        r.update(host(out, ("filt", "smooth", "status")))
        r["counters"] = check_route(eng, "sparse16", N - ngap, ngap)
        return r
    return Case(cid, [f"k_mean_filter_sp16<{K}, {np_}, 1>", f"k_mean_filter_sp16<{K}, {np_}, 2>",
                      f"k_cov_smoother_sp16<{K}>", f"k_mean_smoother_sp16<{K}, {np_}, true>"], fn, mat.T, N)


def sampler_case(cid, mat, p, K, N, seed, inject, want_filt, gaps=True):
    """The shared-factor draw (sparse16-sampler-shared); without filter records the forward pass is the mean filter's MODE 0."""
    y, ngap = observations(N, mat.T, seed, gaps)
    big = large(N, mat.T, mat.d)
    z = np.random.default_rng(seed + 1).standard_normal((N, mat.T + 1, mat.d)) if inject else None
    claims = [f"k_mean_sampler_sp16<{K}, {sampler_nr(mat.d)}, {'false' if inject else 'true'}>"]
    if not want_filt:
        claims.append(f"k_mean_filter_sp16<{K}, {mean_np(mat.d)}, 0>")

    def fn(eng):
        out = eng.ffbs(mat, p, on_device(y, big), z=on_device(z, big) if inject else None, seed=seed, series_offset=3,
                       flags=_lib.OPT_NO_LANE | CNT, want_filt=want_filt)
        r = host(out, ("theta", "stats", "filt", "status"))
        # (without records the mean-only forward kernel counts its series too)
        r["counters"] = check_route(eng, "sparse16-sampler-shared", N - ngap, ngap, at_least=not want_filt)
        return r
    return Case(cid, claims, fn, mat.T, N)


def svd_case(cid, mat, p, N, seed, gaps=True):
    y, ngap = observations(N, mat.T, seed, gaps)
    big = large(N, mat.T, mat.d)

    def fn(eng):
        out = eng.svd_filter(mat, p, on_device(y, big), flags=CNT)
        r = host(out, ("svd", "status"))
        r["counters"] = check_route(eng, "svd-jacobi", N - ngap, ngap)
        return r
    return Case(cid, [f"k_svd_mean_filter4<{svd_ns(mat.d)}>"], fn, mat.T, N)


def full_size_cases():
    """C2, C3 and C5 at full size (10 000 series x T = 1000), device-resident, compared by per-record digests."""
    T, N = 1000, 10000
    mat, p = c2(T)

    def sim(seed):
        from bench import simulate
        return simulate(mat, p, N, seed=seed)

    def c2_shared(eng):
        out = eng.filter_smooth(mat, p, on_device(sim(2), True), flags=CNT)
        r = host(out, ("filt", "smooth", "status"))
        r["counters"] = check_route(eng, "sparse16-rts-shared", N, 0)
        return r

    def c2_own_v(eng):   # per-series V: no shared factors, every series through k_smoother_sp16
        plist = [DlmParameters(p.v * (1.0 + 1e-3 * (n % 7)), p.w, p.m0, p.c0) for n in range(N)]
        out = eng.filter_smooth(mat, plist, on_device(sim(2), True), flags=CNT)
        r = host(out, ("filt", "smooth", "status"))
        r["counters"] = check_route(eng, "sparse16", 0, 0)
        return r

    def c3(eng):
        out = eng.ffbs(mat, p, on_device(sim(3), True), seed=9, flags=CNT)
        r = host(out, ("theta", "stats", "filt", "status"))
        r["counters"] = check_route(eng, "sparse16-sampler-shared", N, 0)
        return r

    def c5(eng):
        out = eng.svd_filter(mat, p, on_device(sim(5), True), flags=CNT)
        r = host(out, ("svd", "status"))
        r["counters"] = check_route(eng, "svd-jacobi", N, 0)
        return r
    return [Case("full-c2-rts-shared", [rts_inst(13, 2)], c2_shared, T, N),
            Case("full-c2-per-series-v", [smoother_inst(2, False, N, 0)], c2_own_v, T, N),
            Case("full-c3-sampler-shared", [f"k_mean_sampler_sp16<2, {sampler_nr(13)}, true>"], c3, T, N),
            Case("full-c5-svd-shared", [f"k_svd_mean_filter4<{svd_ns(13)}>"], c5, T, N)]


def build_cases():
    cases = []
    # k_mean_rts16: every d band x K, then the pipeline edges on C2 (literal Q1 and textbook)
    for d in (6, 9, 12, 14, 15):
        for K in (1, 2, 3, 4):
            mat, p = ring(d, K, 150, seed=10 * d + K)
            cases.append(rts_case(f"rts-d{d}-k{K}", mat, p, K, 7, seed=d + K, q1=K % 2 == 1))
    for T, N in EDGES:
        for q1 in (True, False):
            mat, p = c2(T)
            cases.append(rts_case(f"rts-c2-T{T}-N{N}-{'q1' if q1 else 'tb'}", mat, p, 2, N, seed=T + N, q1=q1))
    # k_smoother_sp16: K x (IRR, PIPE, plain, PLAIN), then the edges on C2
    for K in (1, 2, 3, 4):
        mat, p = ring(8, K, 150, seed=200 + K, irregular=True)
        cases.append(smoother_case(f"smoother-irr-k{K}", mat, p, K, 7, seed=K, irregular=True))
        mat, p = ring(8, K, 150, seed=210 + K)
        cases.append(smoother_case(f"smoother-pipe-k{K}", mat, p, K, 9, seed=K))
        mat, p = ring(6, K, 40, seed=220 + K)
        cases.append(smoother_case(f"smoother-plain-k{K}", mat, p, K, PIPE_MAX + 29, seed=K))
        cases.append(smoother_case(f"smoother-noSteady-k{K}", mat, p, K, PIPE_MAX + 30, seed=K, flags=_lib.OPT_NO_STEADY))
    for T, N in EDGES:
        mat, p = c2(T)
        cases.append(smoother_case(f"smoother-c2-T{T}-N{N}", mat, p, 2, N, seed=T + N))
    for T, N, fl in ((1, PIPE_MAX + 1, 0), (3, PIPE_MAX + 3, 0), (65, PIPE_MAX + 5, 0), (2, PIPE_MAX + 2, _lib.OPT_NO_STEADY),
                     (64, PIPE_MAX + 4, _lib.OPT_NO_STEADY)):
        mat, p = c2(T)
        cases.append(smoother_case(f"smoother-c2-T{T}-N{N}-{'noSteady' if fl else 'plain'}", mat, p, 2, N, seed=T, flags=fl))
    mat, p = c2(200, irregular=True)
    cases.append(smoother_case("smoother-c2-irregular", mat, p, 2, 5, seed=3, irregular=True))
    # DLM_OPT_SHARED_COV: K x the three NP bands, then the edges on C2 (and without the steady shortcut)
    for d in (8, 12, 15):
        for K in (1, 2, 3, 4):
            mat, p = ring(d, K, 150, seed=300 + 10 * d + K)
            cases.append(cov_case(f"cov-d{d}-k{K}", mat, p, K, 7, seed=d * K))
    for T, N in EDGES:
        mat, p = c2(T)
        cases.append(cov_case(f"cov-c2-T{T}-N{N}", mat, p, 2, N, seed=T + N))
    for T, N in ((65, 7), (1000, 37)):
        mat, p = c2(T)
        cases.append(cov_case(f"cov-c2-T{T}-N{N}-noSteady", mat, p, 2, N, seed=T, flags=_lib.OPT_NO_STEADY))
    # k_mean_sampler_sp16: K x the four NR bands x (drawn normals, with and without records; injected normals), then the edges on C2
    for d in (3, 7, 11, 15):
        for K in (1, 2, 3, 4):
            if K > d:
                continue
            mat, p = ring(d, K, 150, seed=400 + 10 * d + K)
            for inject, wf in ((False, True), (False, False), (True, True)):
                cases.append(sampler_case(f"sampler-d{d}-k{K}-{'z' if inject else 'draw'}-{'rec' if wf else 'norec'}", mat, p, K, 9,
                                          seed=d + K, inject=inject, want_filt=wf))
    for T, N in EDGES:
        mat, p = c2(T)
        for wf in (True, False):
            cases.append(sampler_case(f"sampler-c2-T{T}-N{N}-{'rec' if wf else 'norec'}", mat, p, 2, N, seed=T + N, inject=False, want_filt=wf))
    for T, N in ((65, 7), (1000, 37)):
        mat, p = c2(T)
        cases.append(sampler_case(f"sampler-c2-T{T}-N{N}-z", mat, p, 2, N, seed=T, inject=True, want_filt=True))
    # k_svd_mean_filter4: the four NS bands, then the edges on C2
    for d in (6, 9, 12, 16):
        mat, p = band(d, 90, seed=500 + d)
        cases.append(svd_case(f"svd-d{d}", mat, p, 7, seed=d))
    for T, N in EDGES:
        mat, p = c2(T)
        cases.append(svd_case(f"svd-c2-T{T}-N{N}", mat, p, N, seed=T + N))
    return cases + full_size_cases()


CASES = build_cases()


def main(outdir):
    """Runs every case on the library that _lib loads (DLM_ENGINE_LIB) and writes <id>.npz, or <id>.err for a failed route
    assertion.  Any other error ends the run with a non-zero status: no further call is made after an engine error."""
    from bayesian_dlms_amd.engine import Engine
    os.makedirs(outdir, exist_ok=True)
    t0 = time.perf_counter()
    eng = Engine(0)
    for c in CASES:
        try:
            out = c.run(eng)
        except AssertionError:
            with open(os.path.join(outdir, c.id + ".err"), "w") as f:
                f.write(traceback.format_exc())
            continue
        np.savez(os.path.join(outdir, c.id + ".npz"), **out)
    eng.close()
    wall = time.perf_counter() - t0
    with open(os.path.join(outdir, "wall_seconds"), "w") as f:
        f.write(f"{wall:.1f}\n")
    print(f"{len(CASES)} cases on {_lib.LIB_PATH} in {wall:.1f} s")


if __name__ == "__main__":
    main(sys.argv[1])
