"""The two host-side rules of the engine, read from dlm_engine.hip with its comments stripped:

- B: device memory is freed in one place that drains the three streams first (ensure), and at the end of the engine's life
  (dlm_engine_destroy, behind drain_all); dlm_buffer_free frees the caller's own buffers;
- A: the flags "work of this call is in flight on an auxiliary stream" are written by the fork, the join and drain_all alone --
  no entry point sets or clears them by hand."""
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(os.path.dirname(HERE), "bayesian_dlms_amd", "csrc", "dlm_engine.hip")


def _code():
    text = open(SRC).read()
    text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _body(code, name):
    """(start, end) of the braces of the function `name` (its one definition: the head is followed by `{`, a declaration by `;`)."""
    found = []
    for m in re.finditer(r"\b%s\s*\(" % re.escape(name), code):
        depth, i = 0, m.end() - 1
        while True:                                    # the closing parenthesis of the parameter list
            depth += {"(": 1, ")": -1}.get(code[i], 0)
            i += 1
            if depth == 0:
                break
        head = re.match(r"\s*(?:const\s*)?\{", code[i:])
        if not head or not re.search(r"[\w*&>]\s+$", code[:m.start()]):   # a call or a declaration
            continue
        start = i + head.end() - 1
        depth, j = 0, start
        while True:
            depth += {"{": 1, "}": -1}.get(code[j], 0)
            j += 1
            if depth == 0:
                break
        found.append((start, j))
    assert len(found) == 1, (name, found)
    return found[0]


def _inside(pos, spans):
    return any(a <= pos < b for a, b in spans)


def test_the_parser_finds_what_it_looks_for():
    code = _code()
    assert "Rule B" not in code and "hipFree(" in code
    for name in ("ensure", "aux_fork", "aux_join_one", "drain_all", "dlm_engine_destroy", "dlm_buffer_free"):
        a, b = _body(code, name)
        assert code[a] == "{" and code[b - 1] == "}" and b - a > 40, name


def test_device_memory_is_freed_by_the_workspace_helper_and_at_the_end_alone():
    code = _code()
    allowed = [_body(code, n) for n in ("ensure", "dlm_engine_destroy", "dlm_buffer_free")]
    sites = [m.start() for m in re.finditer(r"\bhipFree\s*\(", code)]
    assert len(sites) >= 3
    outside = [code.count("\n", 0, s) + 1 for s in sites if not _inside(s, allowed)]
    assert not outside, f"hipFree outside ensure / dlm_engine_destroy / dlm_buffer_free, lines {outside}"
    # hipMalloc'ed workspaces are re-sized nowhere else either: no second helper of the same kind
    assert not re.search(r"_bytes\s*=\s*need", code)


def test_the_workspace_helper_drains_before_it_frees():
    code = _code()
    a, b = _body(code, "ensure")
    body = code[a:b]
    assert body.count("hipFree(") == 1 and body.count("hipMalloc(") == 1
    drain, free, alloc = body.index("drain_all(e)"), body.index("hipFree("), body.index("hipMalloc(")
    assert drain < free < alloc
    # ... and a failed drain returns before the free
    assert re.search(r"drain_all\(e\);\s*if \(rc\) return rc;\s*HIP_TRY\(e, hipFree\(", body), body


def test_the_busy_flags_are_written_by_fork_join_and_drain_alone():
    code = _code()
    fork, join, drain = _body(code, "aux_fork"), _body(code, "aux_join_one"), _body(code, "drain_all")
    # the two helpers write the flag through a reference parameter ...
    assert re.search(r"\bbusy = true;", code[fork[0]:fork[1]]) and re.search(r"\bbusy = false;", code[join[0]:join[1]])
    assert "e->cov_busy = e->rng_busy = false;" in code[drain[0]:drain[1]]
    # ... which nobody else takes: the flags are named as arguments of those two, and with the stream they belong to
    for flag, stream in (("cov_busy", "cov_stream"), ("rng_busy", "rng_stream")):
        for m in re.finditer(r"\b%s\b" % flag, code):
            if _inside(m.start(), [drain]):
                continue
            line = code[code.rfind("\n", 0, m.start()) + 1:code.find("\n", m.end())]
            if line.strip() == "bool cov_busy = false, rng_busy = false;":   # the members
                continue
            rest = code[m.end():m.end() + 8]
            written = re.match(r"\s*(=[^=]|\+=|-=|\|=|&=|\^=|\+\+|--)", rest) or re.search(r"(\+\+|--|&)\s*(e->)?$", code[:m.start()])
            assert not written, line
            if re.match(r"\s*,", rest) and "bool " not in line:          # handed to a function
                assert re.search(r"\b(aux_fork|aux_join_one)\(e, e->%s, e->%s," % (stream, flag), line), line


def test_destroy_drains_before_anything_is_freed_or_destroyed():
    code = _code()
    a, b = _body(code, "dlm_engine_destroy")
    body = code[a:b]
    drain = body.index("drain_all(e)")
    first = min(m.start() for m in re.finditer(r"\b(hipFree|hipHostFree|hipEventDestroy|hipStreamDestroy|ncclCommDestroy)\s*\(", body))
    assert drain < first
    # every workspace is on the list the loop walks: a Ws member cannot be constructed without it
    assert re.search(r"for \(Workspace\* w = e->workspaces; w; w = w->next\) if \(w->p\) \(void\)hipFree\(w->p\);", body)
    assert re.search(r"explicit Workspace\(Workspace\*& list\) : next\(list\) \{ list = this; \}", code)
