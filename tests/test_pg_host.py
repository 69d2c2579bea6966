"""Particle Gibbs without a GPU: the restatement (tests/pg_restatement.py), the exact grid smoother (tests/pg_grid_reference.py), the
rehearsals of what tests/test_pg_gpu.py asks of the kernel, and the build and API.

The statistical checks of the GPU file (2 invariance, 3 ancestor law, 4 trace, 6 renewal: tests/pg_checks.py) run here FIRST, on the
restatement, at the same N = 4096, K = 3, P = 64 and seeds, and print their figures.  Then the mutants: ONE mistake of derivation each, put
into the restatement's inputs or arithmetic and never into the engine; each must miss at least one of those bounds, which is what gives the
passing checks their meaning.  The table is in profiles/r28_notes.md."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pf_grid_reference as gr  # noqa: E402
import pg_cases as gc  # noqa: E402
import pg_checks as ck  # noqa: E402
import pg_grid_reference as gs  # noqa: E402
import pg_restatement as rs  # noqa: E402

from bayesian_dlms_amd import _lib, build  # noqa: E402
from bayesian_dlms_amd.dglm import Dglm, ParticleGibbs  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters  # noqa: E402
from bayesian_dlms_amd.engine import EngineError  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-8          # no search of the draw-for-draw table comes this close to a running sum: the tolerance of the comparison is 1e-11


# ---- the inputs of the draw-for-draw comparison ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in gc.TABLE])
def test_table_entry_runs_with_margins_and_its_statistics_are_the_path_s(name):
    r, kw = gc.reference(name), gc.run_args(name)
    print(f"{name}: margin of the searches {r['margin_search']:.2e}")
    assert np.all(r["status"] == 0) and np.all(np.isfinite(r["ll"])) and np.all(np.isfinite(r["path"]))
    assert r["margin_search"] >= MARGIN          # (an entry that fails: change its seed, not the bound)
    ck.hold_trace(kw, r)


def test_table_covers_the_shapes():
    t = gc.TABLE
    assert {c["P"] for c in t} == {64, 128} and {c["d"] for c in t} == {1, 2, 3, 8, 16} and max(c["T"] for c in t) <= 12 and max(c["N"] for c in t) <= 6
    assert {c["family"] for c in t} == set(range(6)) and {c["ancestor_sampling"] for c in t} == {False, True}
    assert any(c["per_series"] for c in t) and any(not c["per_series"] for c in t)
    assert any(set(c["missing"]) >= {0, c["T"] - 1} for c in t)
    irr = gc.inputs("d3-p128-irregular")
    assert irr["G"].shape[0] == 3 and irr["dt"][0] == 0.0 and (irr["dt"][1:] == 0.0).sum() == 1 and len(set(irr["g_index"])) == 3
    assert np.all(irr["G"] != 0.0) and np.all(irr["W"] != 0.0)          # dense G, full W
    assert gc.inputs("d1-p64")["dt"][0] != 0.0 and gc.inputs("t1-first-dt0")["dt"][0] == 0.0


def test_restatement_reports_failures_and_leaves_the_neighbours_alone():
    kw, good = gc.run_args("d2-p128-missing-per-series"), gc.reference("d2-p128-missing-per-series")
    W = kw["W"].copy(); W[1] = np.array([[1.0, 2.0], [2.0, 1.0]])
    ref = kw["ref"].copy(); ref[2, 6, 1] = np.nan
    r = rs.run(**dict(kw, W=W, ref=ref))
    assert r["status"].tolist() == [0, rs.ST_NOT_PD, rs.ST_NONFINITE, 0, 0]
    assert np.all(r["ll"][[1, 2]] == -np.inf) and np.all(np.isnan(r["path"][[1, 2]])) and np.all(np.isnan(r["stats"][[1, 2]]))
    for k in ("ll", "path", "stats", "path_index", "clouds", "ancestors", "step_weights"):
        np.testing.assert_array_equal(r[k][[0, 3, 4]], good[k][[0, 3, 4]], err_msg=k)


def test_restatement_s_search_is_the_first_index_above_the_target():
    rng = np.random.default_rng(3)
    cum = np.cumsum(rng.uniform(size=(7, 128)), axis=1)
    target = rng.uniform(size=(7, 50)) * cum[:, -1:]
    target[:, 0], target[:, 1] = 0.0, cum[:, -1]          # the ends: the first particle, and P - 1 when no running sum exceeds the target
    want = np.minimum((cum[:, None, :] <= target[:, :, None]).sum(axis=2), 127)
    np.testing.assert_array_equal(rs.search(cum, target), want)


# ---- the exact smoothing law ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gr.NAMES)
def test_grid_smoother_does_not_move_when_the_spacing_is_halved_and_its_forward_pass_is_the_grid_filter_s(name):
    for q, ex in enumerate(gr.exact(name)):
        err = gs.spacing_error(name, q)
        sm = gs.smoothing(name, q)
        print(f"{name} [{q}]: halving the spacing moves the smoothing moments by {err:.1e} posterior sd")
        assert err < 1e-6
        np.testing.assert_allclose(sm["filt_mean"], ex[1], rtol=0.0, atol=1e-9)          # pf_grid_reference's own recursion
        assert np.all(sm["var"] > 0.0) and np.all(sm["mu4"] > sm["var"] ** 2) and np.all(sm["cross_var"] > 0.0)
        np.testing.assert_allclose(sm["mean"][-1], ex[1][-1], rtol=0.0, atol=1e-9)          # the last record: smoothing = filtering
        np.testing.assert_allclose(np.sqrt(sm["var"][-1]), ex[2][-1], rtol=1e-9)
        same = np.nonzero(gs.DT == 0.0)[0]
        np.testing.assert_allclose(sm["mean"][same], sm["mean"][same + 1], rtol=0.0, atol=1e-12)          # dt = 0: two records, one state
        np.testing.assert_allclose(sm["cross"][same], sm["var"][same] + sm["mean"][same] ** 2, rtol=1e-12)


# ---- checks 2, 3, 4 and 6 on the restatement ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _restatement(name):
    """(the arguments, the first sweep with its traces, the path after K sweeps, the kept share without ancestor sampling)"""
    kw = ck.invariance_args(name)
    path = kw["ref"]
    for k in range(ck.K):
        out = rs.run(**dict(kw, ref=path, iteration=k))
        assert np.all(out["status"] == 0)
        path = out["path"]
        if k == 0:
            first = out
    off = rs.run(**dict(kw, ancestor_sampling=False))
    return kw, first, path, ck.kept_share(off["path_index"], ck.P)


@pytest.mark.parametrize("name", ck.INVARIANCE_NAMES)
def test_rehearsal_the_restatement_passes_the_checks_of_the_gpu_file(name):
    kw, first, path, off = _restatement(name)
    ck.hold_invariance(name, kw["ref"], "the exact start itself")          # the yardstick sees a sample of the law as one
    ck.hold_invariance(name, path, f"restatement, {ck.K} sweeps")
    ck.hold_trace(kw, first)
    on = ck.kept_share(first["path_index"], ck.P)
    ck.hold_renewal(name, on, off)
    assert (round(on, 4), round(off, 4)) == ck.RESTATEMENT_KEPT[name]          # the table IS this measurement
    if name in ck.ANCESTOR_NAMES:
        ck.hold_ancestor_law(kw, first, f"{name}, restatement")
    assert np.all(first["path"][:, np.nonzero(gs.DT == 0.0)[0]] == first["path"][:, np.nonzero(gs.DT == 0.0)[0] + 1])


# ---- the mutants ----------------------------------------------------------------------------------------------------------------------------
# (mutant, case, the check that must miss it): measured over the three cases of profiles/r28_notes.md, the pair here is where each is plainest
MUTANTS = [
    ("f-one-step-late", "irregular-studentt", "invariance"),
    ("g-index-one-step-late", "irregular-studentt", "invariance"),
    ("noise-without-dt", "irregular-studentt", "invariance"),
    ("ancestor-density-without-dt", "irregular-studentt", "ancestor"),
    ("ancestor-weights-without-w", "irregular-studentt", "ancestor"),
    ("ancestor-density-at-x", "irregular-studentt", "ancestor"),
]


@pytest.mark.parametrize("mutant,name,check", MUTANTS, ids=[m for m, _, _ in MUTANTS])
def test_rehearsal_every_mutant_misses_a_bound(mutant, name, check):
    kw = ck.invariance_args(name)
    if mutant in rs.MUTANTS:
        run, kwm = functools.partial(rs.run, mutant=mutant), kw
    else:
        run, kwm = rs.run, gr.mutant(kw, mutant)
    path = kw["ref"]
    for k in range(ck.K if check == "invariance" else 1):
        out = run(**dict(kwm, ref=path, iteration=k))
        path = out["path"]
        if k == 0:
            first = out
    if check == "invariance":
        z = ck.moment_z(name, path)
        print(f"{mutant} on {name}: invariance misses by means {z['mean']:.1f}, variances {z['var']:.1f}, cross-moments {z['cross']:.1f} standard errors")
        assert max(z.values()) > ck.SIGMAS
    else:
        z = ck.ancestor_z(kw, first)          # the law is the TRUE model's
        print(f"{mutant} on {name}: the ancestor law misses by log p_a {z[0]:.1f}, x_a {z[1]:.1f} standard errors")
        assert max(z) > ck.SIGMAS


# ---- build and API --------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_call_with_the_header_s_signature():
    lib = _lib.load()
    assert hasattr(lib, "dlm_pg_batch")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dlm_engine.h")).read(), flags=re.S)
    decl = re.search(r"int dlm_pg_batch\(([^;]*)\);", hdr).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    name, res, args = next(s for s in _lib.SYMBOLS if s[0] == "dlm_pg_batch")
    assert res is ctypes.c_int and len(args) == len(params) == 17
    for p, a in zip(params, args):
        if "uint64_t" in p and "*" not in p:
            assert a is ctypes.c_uint64, p
        else:
            assert "*" in p and a in (ctypes.c_void_p, _lib._MP, _lib._PP, _lib._OP, ctypes.POINTER(_lib.PgDesc)), p
    fields = re.search(r"typedef struct \{([^}]*)\} dlm_pg_desc;", hdr).group(1)
    assert re.findall(r"int(?:32|64)_t (\w+);", fields) == [f for f, _ in _lib.PgDesc._fields_]
    assert [t for _, t in _lib.PgDesc._fields_] == [ctypes.c_int32] * 3 + [ctypes.c_int64] and ctypes.sizeof(_lib.PgDesc) == 24
    cap = re.search(r"#define DLM_PG_WORKSPACE_CAP \((\d+)ll << (\d+)\)", hdr)
    assert int(cap.group(1)) << int(cap.group(2)) == _lib.PG_WORKSPACE_CAP
    src = open(os.path.join(ROOT, "bayesian_dlms_amd", "csrc", "dlm_draws.h")).read()
    assert f"DLM_KEY_PG = 0x{rs.KEY_PG:08X}u" in src and "DLM_PG_SLOT_INIT = DLM_SLOT_TOP" in src
    assert f"DLM_PG_BLOCK_RESAMPLE = {rs.BLOCK_RESAMPLE}u, DLM_PG_BLOCK_REF = {rs.BLOCK_REF}u, DLM_PG_BLOCK_FINAL = {rs.BLOCK_FINAL}u" in src
    keys = re.findall(r"constexpr unsigned DLM_KEY_\w+ = (0x[0-9A-Fa-f]+)u;", src)
    assert len(keys) == len(set(keys)) >= 12          # one stream per key


def test_call_is_bound_and_built():
    assert "dlm_pg_batch(" in open(os.path.join(ROOT, "integration", "jni", "dlm_jni.cpp")).read()
    assert "@native def pgSweep(" in open(os.path.join(ROOT, "integration", "scala", "Batched.scala")).read()
    assert "dlm_pg.hip" in build.SOURCES and "dlm_pg.hip" not in build.DRAIN_SOURCES
    src = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bayesian_dlms_amd", "csrc", "dlm_pg.hip")).read())
    assert "atomic" not in src.lower() and '#include "dlm_pf_common.h"' in src
    for helper in ("pf_chol", "pf_init_cloud", "pf_running_sums", "pf_search", "pf_ancestor", "pf_gather", "pf_normalise", "pf_no_results", "pf_obs", "pf_logdens"):
        assert re.search(r"\b%s\b" % helper, src), helper
    lib = _lib.load()
    assert lib.dlm_pg_batch(None, None, None, None, None, None, None, 0, None, *([None] * 8)) == -1          # no engine: DLM_ERR_ARG, no crash


def _series(T=6):
    return np.arange(1.0, T + 1), np.zeros(T)


def test_python_layer_refuses_what_the_kernel_does_not_cover():
    for n in (96, 2048, 0, 32):
        with pytest.raises(EngineError, match="multiple of 64 between 64 and 1024"):
            ParticleGibbs(n)
    par = lambda d, p: DlmParameters(np.eye(p), np.eye(d), np.zeros(d), np.eye(d))
    with pytest.raises(EngineError, match="d <= 16, got d = 17"):
        ParticleGibbs(64).sample_state(Dglm.poisson(Dlm.polynomial(17)), _series(), par(17, 1), np.zeros((1, 7, 17)), None)
    two = Dlm.polynomial(1) * Dlm.polynomial(1)
    with pytest.raises(EngineError, match=r"univariate observation \(p = 1"):
        ParticleGibbs(64).sample_state(Dglm.gaussian(two), (np.arange(1.0, 7.0), np.zeros((1, 6, 2))), par(2, 2), np.zeros((1, 7, 2)), None)
    with pytest.raises(EngineError, match="Gaussian family only"):
        next(ParticleGibbs(64).sample(Dglm.poisson(Dlm.polynomial(1)), _series(), (4.0, 1.5), par(1, 1), None, 1, prior_v=(4.0, 6.0)))
