"""The hand-counted vmcnt waits against a build that drains them.

ONE child process runs the whole case matrix of counted_waits_cases.py on libdlm_engine_drain.so (every hand-counted wait is
vmcnt(0) there, and nothing else differs: test_counted_waits_host.py); this process runs the same cases on the default build and
compares the bits, NaN patterns included.  A wait whose count is too large on some path reads an LDS slot before its DMA has landed:
the two builds then differ on that case.  Each case asserts in both processes that its route ran (the variant and the series count
of DLM_OPT_COUNT_STEPS), so that a quiet fall-back cannot make the comparison vacuous.  The full-size C2, C3 and C5 calls stay on
the device and are compared by per-record digests."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import counted_waits_cases as cw  # noqa: E402

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT = 900


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """Runs the drained build's side once.  Never relaunched: a failure is recorded and every test of the module reports it."""
    from bayesian_dlms_amd import build
    lib = build.DRAIN_LIB
    if not os.path.exists(lib):
        lib = build.build_drain_variant()
    outdir = str(tmp_path_factory.mktemp("drained"))
    env = dict(os.environ, DLM_ENGINE_LIB=lib)
    state = {"outdir": outdir, "error": None}
    try:
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.join(HERE, "counted_waits_cases.py"), outdir],
                           env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT + 60)
        if r.returncode != 0:
            state["error"] = f"the drained build's child exited with status {r.returncode}:\n{r.stderr[-6000:]}"
        else:
            print(r.stdout.strip())
    except subprocess.TimeoutExpired as e:
        state["error"] = f"the drained build's child did not finish in {CHILD_TIMEOUT + 60} s:\n{(e.stderr or b'')[-6000:]!r}"
    return state


@pytest.fixture(scope="module")
def eng(child):
    if child["error"]:      # no GPU process of this module after the child failed
        yield None
        return
    from bayesian_dlms_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


_engine_error = []


def first_difference(key, a, b):
    """None when a and b hold the same bits; else where they first differ (series, t, entry)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"{key}: shape / type {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
    if a.dtype.itemsize == 8:
        a, b = a.view(np.uint64), b.view(np.uint64)
    ne = np.argwhere(a != b)
    if len(ne) == 0:
        return None
    i = tuple(ne[0])
    names = ("series", "t", "entry")[:a.ndim] if key != "counters" else ("counter",)
    at = ", ".join(f"{n} {v}" for n, v in zip(names, i))
    return (f"{key}: {len(ne)} of {a.size} values differ; first at {at}: default {a[i]:#x} vs drained {b[i]:#x}; "
            f"series {np.unique(ne[:, 0])[:8].tolist()}")


@pytest.mark.parametrize("case", cw.CASES, ids=[c.id for c in cw.CASES])
def test_drained_waits_give_the_same_bits(child, eng, case):
    if child["error"]:
        pytest.fail(child["error"], pytrace=False)
    if _engine_error:
        pytest.fail(f"not run: case {_engine_error[0]} ended in an engine error", pytrace=False)
    err = os.path.join(child["outdir"], case.id + ".err")
    if os.path.exists(err):
        pytest.fail("drained build: " + open(err).read(), pytrace=False)
    try:
        got = case.run(eng)
    except AssertionError:
        raise
    except Exception:
        _engine_error.append(case.id)
        raise
    ref = np.load(os.path.join(child["outdir"], case.id + ".npz"))
    assert sorted(got) == sorted(ref.files), (sorted(got), ref.files)
    diffs = [m for m in (first_difference(k, got[k], ref[k]) for k in sorted(got)) if m]
    assert not diffs, f"{case.id} (kernels {', '.join(case.claims)}): " + "; ".join(diffs)
