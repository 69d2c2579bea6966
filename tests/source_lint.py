"""What the source lints of csrc/ share (test_rts_table_reuse_host.py, test_launch_layer_host.py): reading a source without its comments,
the body of a function, the fields of struct KArgs, and what table_run_args carries over from a call."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesian_dlms_amd", "csrc")


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def strip(src):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def body(src, head, start=0):
    """The brace-balanced body that follows the first occurrence of `head` (at or after `start`)."""
    i = src.index(head, start)
    i = src.index("{", i)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(src[j], 0)
        if depth == 0:
            return src[i:j + 1]
        j += 1


def kargs_fields():
    hdr = strip(read("bayesian_dlms_amd", "csrc", "dlm_internal.h"))
    fields = []
    for decl in body(hdr, "struct KArgs").strip("{}").split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(","):
            name = re.search(r"(\w+)\s*$", part.strip())
            assert name, decl
            fields.append(name.group(1))
    return fields


def builder_copies():
    """The fields table_run_args copies from the call (k.f = a.f), and everything else it assigns."""
    fn = body(strip(read("bayesian_dlms_amd", "csrc", "dlm_internal.h")), "inline KArgs table_run_args(const KArgs& a)")
    copies = re.findall(r"\bk\.(\w+)\s*=\s*a\.(\w+)\s*;", fn)
    assert all(l == r for l, r in copies), copies
    assigned = re.findall(r"\bk\.(\w+)\s*=", fn)
    return [l for l, _ in copies], [f for f in assigned if f not in dict(copies)]
