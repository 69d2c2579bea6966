"""The launch layer of csrc/, as a source lint (below the table of variants): every kernel launch goes through launch
(dlm_internal.h), which alone asks for dynamic LDS above 64 KB -- per function AND device, in one guarded book of dlm_engine.hip --; and
the arguments of every table run (one wave on a series of zeros) start from table_run_args, whose whitelist partitions struct KArgs
together with the list of per-call fields beside it."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from source_lint import CSRC, body, builder_copies, kargs_fields, read, strip  # noqa: E402

SOURCES = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))


def _src(name):
    return strip(read("bayesian_dlms_amd", "csrc", name))


def _functions(src):
    """(head, body) of every brace-balanced block at namespace level or below that follows a ')' -- function definitions, lambdas included
    in the function that holds them."""
    out, i = [], 0
    for m in re.finditer(r"\)\s*(?:const\s*)?(?:->\s*[\w:]+\s*)?\{", src):
        if m.start() < i:
            continue   # inside the body taken last
        b = body(src, "{", m.end() - 1)
        out.append((src[max(0, m.start() - 200):m.start()], b))
        i = m.end() - 1 + len(b)
    return out


def test_every_kernel_launch_goes_through_launch():
    assert len(SOURCES) >= 15
    for name in SOURCES:
        src = _src(name)
        n = len(re.findall(r"\bhipLaunchKernelGGL\b|<<<", src))
        if name == "dlm_internal.h":
            assert n == 1 and "hipLaunchKernelGGL(kernel, grid, block, lds_bytes, s, args...);" in body(src, "inline hipError_t launch("), name
        else:
            assert n == 0, name
    fn = body(_src("dlm_internal.h"), "inline hipError_t launch(")
    # at or below 64 KB: one comparison and nothing else in front of the launch
    assert re.match(r"\{\s*if \(lds_bytes > 64 \* 1024\) \{\s*const hipError_t err = lds_opt_in\(\(const void\*\)kernel, lds_bytes\);\s*"
                    r"if \(err != hipSuccess\) return err;\s*\}\s*hipLaunchKernelGGL\(", fn), fn


def test_lds_is_asked_for_in_one_place_per_function_and_device():
    for name in SOURCES:
        src = _src(name)
        if name != "dlm_engine.hip":
            assert not re.search(r"\bhipFuncSetAttribute\b|\bhipFuncGetAttributes\b", src), name
        assert not re.search(r"160\s*\*\s*1024|163840|\b160u?\s*<<\s*10", src), name          # the device says what it has
        assert not re.search(r"\blds_opt_in\s*\(", src) or name in ("dlm_internal.h", "dlm_engine.hip"), name
    eng = _src("dlm_engine.hip")
    assert eng.count("hipFuncSetAttribute") == 1 and "hipFuncSetAttribute" in body(eng, "hipError_t opt_in_locked(")
    assert eng.count("hipFuncGetAttributes") == 1 and "hipFuncGetAttributes" in body(eng, "size_t whole_cu_lds(const void* fn)")
    assert "hipDeviceAttributeMaxSharedMemoryPerBlock" in body(eng, "size_t limit_locked(int dev)")
    assert "bytes > limit_locked(dev)" in body(eng, "hipError_t opt_in_locked(")
    # the record: one map keyed by (function, device), every access under the one mutex
    assert re.search(r"std::map<std::pair<const void\*, int>, LdsEntry> lds_book;", eng)
    for head in ("hipError_t lds_opt_in(const void* fn, size_t bytes)", "size_t whole_cu_lds(const void* fn)", "size_t lds_limit()"):
        fn = body(eng, head)
        assert "hipGetDevice(&dev)" in fn and "std::lock_guard<std::mutex> lock(lds_mutex);" in fn, head
    for head in ("size_t limit_locked(int dev)", "hipError_t opt_in_locked("):
        assert "lds_book[{" in body(eng, head)
    assert len(re.findall(r"\blds_book\b", eng)) == 4   # the declaration, the two helpers, whole_cu_lds
    # no process-wide one-shots in the launchers: a static set on the first call knows nothing of a second device
    for name in SOURCES:
        for head, b in _functions(_src(name)):
            if re.search(r"\blaunch\w*\s*\(", b):
                assert not re.search(r"\bstatic\s+(?:const\s+)?(?:hipError_t|size_t|bool|int)\s+\w+\s*=", b), (name, head[-80:])


def test_every_table_run_starts_from_the_builder():
    users = 0
    for name in SOURCES:
        for head, b in _functions(_src(name)):
            users += len(re.findall(r"\btable_run_args\(a\)", b)) if "inline KArgs table_run_args" not in head else 0
            # a copy of a call's arguments that is then cut down to one series by hand
            for m in re.finditer(r"\bKArgs\s+(\w+)\s*=\s*(\w+)\s*;", b):
                assert not re.search(r"\b%s\.N\s*=\s*1\b" % m.group(1), b[m.end():]), (name, m.group(0))
            assert not re.search(r"\.N\s*=\s*1\b", b) or "inline KArgs table_run_args" in head, (name, head[-80:])
    assert users == 6   # wave48 tables, sampler tables, sampler tables from records, RTS tables, cov_args, SVD shared factors


def test_the_builder_s_whitelist_and_the_per_call_list_partition_kargs():
    hdr = read("bayesian_dlms_amd", "csrc", "dlm_internal.h")
    lists = {}
    for kind in ("carried", "per call"):
        m = re.search(r"//\s+TABLE-RUN %s:\s+([\w ]+)\n" % kind, hdr)
        assert m, kind
        lists[kind] = m.group(1).split()
    fields = kargs_fields()
    named = lists["carried"] + lists["per call"]
    assert len(fields) >= 45 and len(set(fields)) == len(fields)
    assert len(named) == len(set(named)), sorted(f for f in named if named.count(f) > 1)
    assert set(named) == set(fields), f"in neither list: {sorted(set(fields) - set(named))}; not in KArgs: {sorted(set(named) - set(fields))}"
    copies, others = builder_copies()
    assert sorted(copies) == sorted(lists["carried"]) and len(set(copies)) == len(copies), (copies, lists["carried"])
    assert others == ["N"]
    fn = body(strip(hdr), "inline KArgs table_run_args(const KArgs& a)")
    assert re.search(r"\{\s*KArgs k\{\};\s*k\.N = 1;", fn) and re.search(r"return k;\s*\}$", fn)
    # the whitelist the model and the shared parameters make up (a longer one is a decision to write down here)
    assert lists["carried"] == ("d p T F f_stride G n_g g_index dt V v_stride W w_stride v_tstride w_tstride C0 c0_stride "
                                "spb spb_k spf spf_k flags stretches").split()
