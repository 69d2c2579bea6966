"""The wave-level device primitives live in csrc/dlm_wave.h, each defined once, on the CPU, by regex over csrc/:

- no kernel file defines, at namespace scope, a function whose name the header defines;
- the instructions the primitives wrap -- the LDS-DMA asm, the raw buffer builtins, the permlane swaps, ds_bpermute, a hand-issued
  ds_read -- appear nowhere else;
- no file redefines one of the header's vector typedefs, under its name or another.

A use that has to stay local goes on ALLOWED below, with its reason."""
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "bayesian_dlms_amd", "csrc")
HEADER = "dlm_wave.h"
KERNEL_FILES = ("dlm_sparse16.hip", "dlm_sampler16.hip", "dlm_wave48.hip", "dlm_tiled.hip", "dlm_svd.hip", "dlm_mfma16.hip")

# (file, name): why this definition or use stays outside the header
ALLOWED = {
    ("dlm_wave48.hip", "mmT"): "w48::mmT<KT, MT, NT, UP> is the product over ARRAYS of tiles (its own signature and loop nest); the header's is the single-tile chain",
    ("dlm_svd.hip", "__builtin_amdgcn_make_buffer_rsrc"): "k_svd_mean_filter, once: through mk_rsrc its register allocation changes (two SGPRs trade names), and the code objects are held identical",
}

# a function definition or declaration at namespace scope: these files indent nothing there, and everything inside a body is indented
DEF = re.compile(r"^(?:static\s+|inline\s+)*(?:__host__\s+)?__device__[^\n(;]*?\b(\w+)\s*\(", re.MULTILINE)
TYPEDEF = re.compile(r"typedef\s+(\w+)\s+(\w+)\s+__attribute__\(\(ext_vector_type\((\d+)\)\)\)\s*;")
WRAPPED = {
    "the LDS-DMA asm": re.compile(r'"[^"\n]*buffer_load_dword[^"\n]*\blds\b'),
    "__builtin_amdgcn_make_buffer_rsrc": re.compile(r"__builtin_amdgcn_make_buffer_rsrc"),
    "__builtin_amdgcn_raw_buffer_": re.compile(r"__builtin_amdgcn_raw_buffer_"),
    "permlane16_swap": re.compile(r"permlane16_swap"),
    "permlane32_swap": re.compile(r"permlane32_swap"),
    "ds_bpermute": re.compile(r"ds_bpermute"),
    "an inline-asm ds_read_b": re.compile(r'"[^"\n]*ds_read_b'),
}


def _code(name):
    """The file without its comments (prose may name an instruction)."""
    text = open(os.path.join(CSRC, name)).read()
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.DOTALL)
    return re.sub(r"//[^\n]*", "", text)


def _others():
    return [n for n in sorted(os.listdir(CSRC)) if n != HEADER]


def _header_functions():
    names = set(DEF.findall(_code(HEADER)))
    assert {"wave_sync", "sum_g", "row_sum", "wave_max", "wave_max2f", "dpp_mov", "row_ror", "readlane_d", "row_pick", "fast_rcp", "mmT",
            "mk_rsrc", "bld", "bst", "bst128", "bld128", "rsrc_words", "lds_addr_of", "lds_dma", "lds_read64", "lds_read128", "lds_fence",
            "lds_wait", "stamp", "row_lane0", "pair_rows", "lds_dma_issue"} <= names, sorted(names)
    return names


def test_no_kernel_file_defines_a_primitive_of_the_header():
    names = _header_functions()
    found, seen = [], 0
    for f in _others():
        for m in DEF.finditer(_code(f)):
            seen += 1
            if m.group(1) in names and (f, m.group(1)) not in ALLOWED:
                found.append((f, m.group(1)))
    assert seen >= 100, seen          # (the pattern finds the files' device functions)
    assert not found, found
    assert len(ALLOWED) <= 3


def test_the_wrapped_instructions_appear_in_the_header_only():
    hdr = _code(HEADER)
    for what, pat in WRAPPED.items():
        assert pat.search(hdr), what          # (the pattern matches the real thing)
    found = [(f, what) for f in _others() for what, pat in WRAPPED.items() if pat.search(_code(f)) and (f, what) not in ALLOWED]
    assert not found, found
    for (f, what) in ALLOWED:          # an exception is one use, and none is stale
        n = len(WRAPPED[what].findall(_code(f))) if what in WRAPPED else DEF.findall(_code(f)).count(what)
        assert n == 1, (f, what, n)


def test_no_file_redefines_a_vector_typedef_of_the_header():
    mine = {(base, n): name for base, name, n in TYPEDEF.findall(_code(HEADER))}
    assert set(mine.values()) == {"d4", "d2", "u2", "u4", "i4"}, mine
    found = []
    for f in _others():
        for base, name, n in TYPEDEF.findall(_code(f)):
            if name in mine.values() or (base, n) in mine:          # the same name, or the same type under another (u2v, i4s)
                found.append((f, name))
    assert not found, found


def test_each_primitive_is_defined_once_and_the_header_goes_where_it_belongs():
    hdr = _code(HEADER)
    overloads = {"lds_fence": 2, "lds_wait": 5, "bst128": 2}          # one definition per argument list
    counts = {}
    for name in DEF.findall(hdr):
        counts[name] = counts.get(name, 0) + 1
    assert {n: c for n, c in counts.items() if c != overloads.get(n, 1)} == {}
    assert re.search(r"^namespace dlm \{", hdr, re.MULTILINE) and "__global__" not in hdr
    for f in KERNEL_FILES:
        assert '#include "dlm_wave.h"' in _code(f), f
    assert "dlm_wave.h" not in open(os.path.join(CSRC, "dlm_engine.hip")).read()
    # vm_wait stays in dlm_internal.h (test_counted_waits_host.py); the generic kernels' __syncthreads() hand-off is not the header's wave_sync
    assert "void vm_wait()" not in hdr and "vm_wait<N>" in open(os.path.join(CSRC, HEADER)).read()
    gen = _code("dlm_generic.hip")
    assert "wave_sync" not in gen and re.search(r"void block_sync\(\) \{ __syncthreads\(\); \}", gen)
    from bayesian_dlms_amd import build as b
    assert os.path.join(CSRC, HEADER) in [os.path.normpath(h) for h in b.HEADERS]
