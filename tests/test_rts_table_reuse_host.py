"""The kept RTS tables, on the CPU (the GPU side: test_rts_table_reuse_gpu.py): the new option bit and export agree across
the header, the ctypes table, the JNI glue and the Scala shim; and a source lint of the key -- the list in csrc/dlm_internal.h that says what
becomes of every field of KArgs in the two one-wave table kernels is held against the struct, the key's code, sampler_shared_model_ok and
the launchers, so that a field added to KArgs, or one the launchers start to pass through, cannot stay out of the key unnoticed."""
import ctypes
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from source_lint import body as _body, builder_copies, kargs_fields as _kargs_fields, read as _read, strip as _strip  # noqa: E402


def test_flag_and_indicator_agree_between_header_python_jni_and_scala():
    from bayesian_dlms_amd import _lib
    hdr = _read("include", "dlm_engine.h")
    m = re.search(r"DLM_OPT_NO_TABLE_REUSE\s*=\s*1u\s*<<\s*(\d+)", hdr)
    assert m and int(m.group(1)) in (13, 14, 15, 29, 31)
    assert _lib.OPT_NO_TABLE_REUSE == 1 << int(m.group(1))
    assert re.search(r"val NoTableReuse = 1 << %s\b" % m.group(1), _read("integration", "scala", "Batched.scala"))
    vals = {k: int(v) for k, v in re.findall(r"DLM_TABLES_(\w+)\s*=\s*(\d+)", hdr)}
    assert vals == {"NONE": _lib.TABLES_NONE, "BUILT": _lib.TABLES_BUILT, "REUSED": _lib.TABLES_REUSED, "SKIPPED": _lib.TABLES_SKIPPED}
    assert len(set(vals.values())) == 4
    assert re.search(r"int\s+dlm_last_table_reuse\s*\(\s*dlm_engine\s*\*\s*e\s*,\s*int32_t\s*\*\s*out\s*\)", _strip(hdr))
    proto = {name: (res, args) for name, res, args in _lib.SYMBOLS}["dlm_last_table_reuse"]
    assert proto[0] is ctypes.c_int and len(proto[1]) == 2 and proto[1][1] == ctypes.POINTER(ctypes.c_int32)
    assert "@native def lastTableReuse(h: Long): Int" in _read("integration", "scala", "Batched.scala")
    assert re.search(r"Native_lastTableReuse\(JNIEnv\* env, jobject, jlong h\)", _read("integration", "jni", "dlm_jni.cpp"))
    from bayesian_dlms_amd.engine import Engine
    assert callable(Engine.last_table_reuse)


def test_the_library_exports_the_indicator():
    from bayesian_dlms_amd import _lib
    assert hasattr(_lib.load(), "dlm_last_table_reuse")


def _key_lists():
    hdr = _read("bayesian_dlms_amd", "csrc", "dlm_internal.h")
    out = {}
    for kind in ("keyed", "fixed", "replaced", "unread"):
        m = re.search(r"//\s+RTS-KEY %s:\s+([\w ]+)\n" % kind, hdr)
        assert m, kind
        out[kind] = m.group(1).split()
    return out


def test_the_key_list_names_every_field_of_kargs_once():
    fields, lists = _kargs_fields(), _key_lists()
    assert len(fields) >= 45 and len(set(fields)) == len(fields), fields
    named = [f for kind in lists.values() for f in kind]
    assert len(named) == len(set(named)), sorted(f for f in named if named.count(f) > 1)
    assert set(named) == set(fields), f"not in the list: {sorted(set(fields) - set(named))}; not in KArgs: {sorted(set(named) - set(fields))}"


def test_keyed_fields_are_compared_fixed_ones_refused_replaced_ones_set_by_the_launchers():
    lists = _key_lists()
    hdr = _strip(_read("bayesian_dlms_amd", "csrc", "dlm_internal.h"))
    s16 = _strip(_read("bayesian_dlms_amd", "csrc", "dlm_sampler16.hip"))
    sp16 = _strip(_read("bayesian_dlms_amd", "csrc", "dlm_sparse16.hip"))
    # keyed: a member of RtsKeySrc, filled from the call by rts_key_of, read by rts_key_word (G: as its tables `sp` and their K)
    src_struct, fill, word = _body(hdr, "struct RtsKeySrc"), _body(s16, "static RtsKeySrc rts_key_of"), _body(s16, "unsigned rts_key_word")
    for f in lists["keyed"]:
        members = ("sp", "K") if f == "G" else (f,)
        for mname in members:
            assert re.search(r"\b%s\b" % mname, src_struct), (f, "RtsKeySrc")
            assert re.search(r"\bs\.%s\s*=" % mname, fill), (f, "rts_key_of")
            assert re.search(r"\bs\.%s\b" % mname, word), (f, "rts_key_word")
    for f in ("d", "T", "F", "V", "W", "C0"):
        assert re.search(r"s\.%s\s*=\s*a\.%s\s*;" % (f, f), fill), f
    assert re.search(r"s\.flags\s*=\s*a\.flags\s*&\s*RTS_KEY_FLAGS\s*;", fill)
    # ... every word of it by both small kernels, and compared for equality: no checksum
    check, commit = _body(s16, "void k_rts_key_check"), _body(s16, "void k_rts_key_commit")
    assert re.search(r"kept\[i\]\s*!=\s*rts_key_word\(s, i\)", check) and "rts_key_words(s.d)" in check
    assert re.search(r"kept\[i\]\s*=\s*rts_key_word\(s, i\)", commit) and "rts_key_words(s.d)" in commit
    # the flags of the key are the flags the two kernels test
    m = re.search(r"RTS_KEY_FLAGS\s*=\s*\(1u << (\d+)\) \| \(1u << (\d+)\)", hdr)
    pub = _read("include", "dlm_engine.h")
    bit = lambda name: int(re.search(name + r"\s*=\s*1u\s*<<\s*(\d+)", pub).group(1))
    assert {int(m.group(1)), int(m.group(2))} == {bit("DLM_OPT_SMOOTHER_COMPAT_Q1"), bit("DLM_OPT_NO_STEADY")}
    kernels = _body(s16, "void k_smoother_rts16") + _body(sp16, "void filter_body")
    assert set(re.findall(r"DLM_OPT_\w+", kernels)) == {"DLM_OPT_SMOOTHER_COMPAT_Q1", "DLM_OPT_NO_STEADY"}
    # fixed: sampler_shared_model_ok refuses any other value (rts_shared_eligible starts with it)
    ok = _body(s16, "bool sampler_shared_model_ok")
    for f in lists["fixed"]:
        assert re.search(r"\ba\.%s\b" % f, ok), f
    assert re.search(r"return\s+sampler_shared_model_ok\(a\)\s*&&", _body(s16, "bool rts_shared_eligible"))
    # the arguments of both table runs start from table_run_args: whatever it carries over from the call is keyed, fixed or unread ...
    for fn, var in (("hipError_t launch_rts_shared_tables", "kp"), ("static KArgs cov_args", "k")):
        assert re.search(r"KArgs %s = table_run_args\(a\);" % var, _body(s16 if "rts" in fn else sp16, fn)), fn
    assert re.search(r"KArgs k = cov_args\(a, tb\);", _body(sp16, "static hipError_t launch_cf"))
    assert re.search(r"launch\(k_cov_filter_sp16<K>, [^;]*, s, k, sp,", _body(sp16, "static hipError_t launch_cf"))
    assert re.search(r"launch\(kernel, [^;]*, s, kp, tabs_dev, tb\)", _body(s16, "hipError_t launch_rts_shared_tables"))
    copies, others = builder_copies()
    assert others == ["N"] and copies, (copies, others)
    for f in copies:
        assert f in lists["keyed"] + lists["fixed"] + lists["unread"], f
    # ... replaced: not carried over, or assigned by one of the launchers on the way to the two kernels
    launch = (_body(s16, "hipError_t launch_rts_shared_cov") + _body(s16, "hipError_t launch_rts_shared_tables") +
              _body(sp16, "static KArgs cov_args") + _body(sp16, "static hipError_t launch_cf"))
    for f in lists["replaced"]:
        assert f not in copies or re.search(r"\bk[cp]?\.%s\s*=" % f, launch), f
    # ... and nothing but `a` reaches the covariance-only filter on the RTS route (no copy with fields of its own in between)
    assert re.search(r"return launch_sparse16_cov_filter\(a, K, tabs_dev, cs, s\);", _body(s16, "hipError_t launch_rts_shared_cov"))
    # ... and the two kernels take the gate for RtsTabs::skip / CovTabs::skip
    assert re.search(r"cs\.skip\s*=\s*gate\s*;", _body(s16, "hipError_t launch_rts_shared_cov"))
    assert re.search(r"tb\.skip\s*=\s*const_cast<int\*>\(gate\)\s*;", _body(s16, "hipError_t launch_rts_shared_tables"))


def test_the_key_has_room_for_the_largest_model_of_the_route():
    hdr = _strip(_read("bayesian_dlms_amd", "csrc", "dlm_internal.h"))
    s16 = _strip(_read("bayesian_dlms_amd", "csrc", "dlm_sampler16.hip"))
    assert "RTS_KEY_WORDS = 8 + 2 * (15 + 1 + 2 * 15 * 15) + 2 * (int)(sizeof(SparseT) / 4)" in hdr
    assert "return 8 + 2 * (d + 1 + 2 * d * d) + 2 * (int)(sizeof(SparseT) / 4);" in s16
    assert re.search(r"a\.d <= 15", _body(s16, "bool sampler_shared_model_ok"))
    assert s16.count("if (a.d < 1 || a.d > 15) return hipErrorInvalidValue;") == 2
