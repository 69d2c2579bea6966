"""The hand-counted vmcnt waits of the LDS-DMA prefetches, on the CPU (the GPU side: test_counted_waits_gpu.py).

- every counted wait in the sources goes through vm_wait<N> (dlm_internal.h), the one switch that DLM_DRAIN_WAITS=1 drains;
- the default and the drained code objects of the three units differ in exactly those waits, each one drained to vmcnt(0), and in
  every instantiation of the eight kernel families that use them: the GPU comparison of the two builds then tests the counts and
  nothing else;
- the GPU case matrix (counted_waits_cases.py) reaches every such instantiation, or lists it as unreachable with a reason."""
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import counted_waits_cases as cw  # noqa: E402

CSRC = os.path.join(ROOT, "bayesian_dlms_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
FAMILIES = ("k_smoother_sp16", "k_cov_smoother_sp16", "k_mean_filter_sp16", "k_mean_smoother_sp16", "k_mean_sampler_sp16",
            "k_mean_rts16", "k_svd_mean_filter4", "k_svd_mean_filter")


def test_every_counted_wait_goes_through_the_switch():
    """No `s_waitcnt vmcnt(N)` with N other than 0 (a number or an asm operand) outside vm_wait's one definition."""
    found = []
    for name in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, name)).read()
        for m in re.finditer(r"s_waitcnt\s+vmcnt\(\s*([^)\s]*)\s*\)", text, re.IGNORECASE):
            if m.group(1) != "0":
                found.append((name, text.count("\n", 0, m.start()) + 1, m.group(0)))
        assert "__builtin_amdgcn_s_waitcnt" not in text, name
    assert len(found) == 1 and found[0][0] == "dlm_internal.h", found
    hdr = open(os.path.join(CSRC, "dlm_internal.h")).read()
    assert re.search(r'void vm_wait\(\) \{[^}]*"s_waitcnt vmcnt\(%0\)" ::"n"\(DLM_DRAIN_WAITS \? 0 : N\)', hdr), "vm_wait must honour DLM_DRAIN_WAITS"


def _objects():
    from bayesian_dlms_amd import build as b
    pairs = [(os.path.join(ROOT, "bayesian_dlms_amd", "build", s.replace(".hip", ".o")), b.drain_object(s)) for s in b.DRAIN_SOURCES]
    if not all(os.path.exists(o) for pair in pairs for o in pair):
        b.build_drain_variant()
    return pairs


def _listing(obj, tmp_path):
    """The gfx950 code object's disassembly as [(function, instruction)], encodings and addresses left out."""
    tag = os.path.basename(os.path.dirname(obj)) + "_" + os.path.basename(obj)
    fat, co = str(tmp_path / (tag + ".fat")), str(tmp_path / (tag + ".co"))
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "-C", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    out, fn = [], None
    for line in dis.splitlines():
        lab = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if lab:
            m = re.search(r"\b(k_\w+(?:<[^()]*>)?)\(", lab.group(1))
            fn = m.group(1) if m else lab.group(1)
            continue
        ins = line.split("//")[0].strip()
        if ins and fn is not None and not ins.startswith("Disassembly of"):
            out.append((fn, ins))
    return out


def family(inst):
    return inst.split("<")[0]


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("co")
    return [(_listing(d, tmp), _listing(x, tmp)) for d, x in _objects()]


def test_the_drained_build_differs_only_in_the_hand_counted_waits(listings):
    per_inst = {}
    for default, drained in listings:
        assert len(default) == len(drained)
        for (fa, a), (fb, b) in zip(default, drained):
            assert fa == fb
            if a == b:
                continue
            assert a.startswith("s_waitcnt") and b.startswith("s_waitcnt"), (fa, a, b)
            assert re.fullmatch(r"s_waitcnt vmcnt\([1-9]\d*\)", a), (fa, a)
            assert b == "s_waitcnt vmcnt(0)", (fa, a, b)
            per_inst[fa] = per_inst.get(fa, 0) + 1
    assert {family(i) for i in per_inst} == set(FAMILIES), sorted(per_inst)
    # ... and in EVERY instantiation of the eight families
    kernels = {f for default, _ in listings for f, _ in default if family(f) in FAMILIES}
    assert kernels == set(per_inst), sorted(kernels ^ set(per_inst))


def test_the_gpu_cases_reach_every_instantiation_with_counted_waits(listings):
    kernels = {f for default, _ in listings for f, _ in default if family(f) in FAMILIES}
    assert len(kernels) >= 100, len(kernels)          # (the parse found the symbol table)
    claimed = {i for c in cw.CASES for i in c.claims}
    unreachable = set(cw.UNREACHABLE)
    assert not claimed & unreachable, sorted(claimed & unreachable)
    assert claimed | unreachable <= kernels, sorted((claimed | unreachable) - kernels)      # no claim of a kernel that does not exist
    assert kernels <= claimed | unreachable, f"instantiations without a GPU case: {sorted(kernels - claimed - unreachable)}"


def test_every_family_sees_the_pipeline_edges():
    """T in {1, 2, 3} (prologue / epilogue), {63, 64, 65} (the every-64th-step branch), one T >= 700; N = 1 and N not a multiple of 4."""
    for fam in FAMILIES:
        if fam == "k_svd_mean_filter":
            continue
        cases = [c for c in cw.CASES if any(family(i) == fam for i in c.claims)]
        Ts, Ns = {c.T for c in cases}, {c.N for c in cases}
        assert {1, 2, 3, 63, 64, 65} <= Ts and max(Ts) >= 700, (fam, sorted(Ts))
        assert 1 in Ns and any(n % 4 for n in Ns if n > 1), (fam, sorted(Ns))


def test_case_ids_are_unique_and_the_dispatch_rules_match_the_launchers():
    ids = [c.id for c in cw.CASES]
    assert len(ids) == len(set(ids))
    assert [cw.rts_inst(d, 1) for d in (7, 8, 13, 14, 15)] == ["k_mean_rts16<1, 2, 1, 1>", "k_mean_rts16<1, 4, 1, 2>", "k_mean_rts16<1, 6, 2, 2>",
                                                               "k_mean_rts16<1, 8, 2, 2>", "k_mean_rts16<1, 8, 2, 3>"]
    assert [cw.sampler_nr(d) for d in (3, 4, 7, 8, 11, 12, 15)] == [1, 2, 2, 3, 3, 4, 4]
    assert [cw.svd_ns(d) for d in (1, 7, 8, 10, 11, 13, 14, 16)] == [4, 4, 8, 8, 13, 13, 18, 18]
    assert [cw.mean_np(d) for d in (1, 10, 11, 13, 14, 15)] == [4, 4, 6, 6, 8, 8]
    src = open(os.path.join(CSRC, "dlm_sparse16.hip")).read()
    assert "#define DLM_PIPE_MAX 3072" in src and cw.PIPE_MAX == 3072
