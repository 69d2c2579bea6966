"""The resampling schemes of the particle filter without a GPU: the restatement the kernel is held to (tests/pf_resample_restatement.py)
against what it must compute, and the inputs of the GPU tests (tests/pf_resample_cases.py) against what makes them worth running.

  1  at MULTINOMIAL the new restatement IS tests/pf_restatement.py's, bit for bit;
  2  no comparison the kernel makes on the GPU table is within 1e-11 of flipping: the searches, the ESS test and the Metropolis decisions
     (the tolerance of the GPU comparison; 1 / sum W^2 is 1e-9 away from every integer, as tests/test_pf_host.py asks, and for its reason);
  3  the offspring counts of systematic and stratified resampling obey their bounds (pf_resample_cases.hold_offspring says why they hold),
     and the same check FAILS on multinomial ancestors;
  4  the ancestor of a Metropolis chain of b steps has the law of row `start` of K^b, K the Metropolis kernel with a uniform proposal built
     here from the weights alone: a chi-square test at the 1 - 1e-6 quantile over 4096 series' uniforms, one weight equal to 0;
  5  stratified and systematic resampling leave the likelihood estimate unbiased for the exact grid likelihood of tests/pf_grid_reference.py
     on all nine cases, with its conditions on the largest ratio and the resampled share;
  6  the header, ctypes, the JNI glue and the Scala declaration agree on the new export, dlm_draws.h and the restatement on the blocks, and
     the Python layer refuses what the engine refuses."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pf_cases as pc  # noqa: E402
import pf_grid_reference as gr  # noqa: E402
import pf_resample_cases as rc  # noqa: E402
import pf_resample_restatement as rr  # noqa: E402
import pf_restatement as pr  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dglm import Dglm, Metropolis, ParticleFilter, Resampling  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters  # noqa: E402
from bayesian_dlms_amd.engine import Engine, EngineError, check_pf_resample  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-11
KEYS = ("ll", "mean", "ess", "cloud", "weights")


# ---- 1: the new restatement against the old one -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p128-d2-missing-per-series", "always"])
def test_multinomial_restatement_is_the_bootstrap_filter_s_bit_for_bit(name):
    old, new = pc.reference(name), rr.run(**pc.run_args(name), resample=rr.MULTINOMIAL, mh_steps=0)
    for k in KEYS + ("status",):
        np.testing.assert_array_equal(new[k], old[k], err_msg=k)
    assert new["resample_share"] == old["resample_share"] > 0.0 and new["margin_accept"] == np.inf
    for k in ("margin_search", "margin_n0", "margin_int"):
        assert new[k] == old[k], k


# ---- 2: the margins of the GPU table --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scheme,b", rc.RUNS, ids=[rc.run_id(*r) for r in rc.RUNS])
def test_table_entry_resamples_with_margins(name, scheme, b):
    r = rc.reference(name, scheme, b)
    print(f"{rc.run_id(name, scheme, b)}: share {r['resample_share']:.2f}, margins search {r['margin_search']:.2e}, accept {r['margin_accept']:.2e}, "
          f"n0 {r['margin_n0']:.2e}, integer {r['margin_int']:.2e}")
    assert np.all(r["status"] == 0) and np.all(np.isfinite(r["ll"]))
    assert r["resample_share"] > 0.0          # the scheme is reached
    if rc.by_name(name)["n0"] <= rc.by_name(name)["P"]:
        assert r["resample_share"] < 1.0          # ... and so is the branch around it
    else:
        assert r["resample_share"] == 1.0
    assert r["margin_search"] >= MARGIN and r["margin_n0"] >= MARGIN and r["margin_accept"] >= MARGIN          # (a failure: another seed, not another bound)
    assert r["margin_int"] >= 1e-9
    assert (r["margin_accept"] < np.inf) == (scheme == rr.METROPOLIS) and (r["margin_search"] < np.inf) == (scheme != rr.METROPOLIS)


def test_table_is_the_one_the_kernel_is_held_to():
    shapes = [(c["P"], c["d"], c["T"], c["N"]) for c in rc.TABLE]
    assert shapes == [(64, 1, 12, 5), (128, 3, 12, 5), (192, 2, 12, 5), (1024, 2, 2, 1)]
    assert rc.by_name("p128-d3-always")["n0"] == 129
    c, a = rc.by_name("p192-d2-irregular"), rc.inputs("p192-d2-irregular")
    assert c["per_series"] and a["W"].shape == (5, 2, 2) and a["G"].shape[0] == 3 and (a["dt"][1:] == 0.0).sum() == 1
    assert np.all(np.isnan(a["y"][:, [0, 6, 11]])) and np.isnan(a["y"]).sum() == 15
    mh = lambda name: sorted(b for s, b in rc.SCHEMES[name] if s == rr.METROPOLIS)
    assert [mh(n) for n in rc.NAMES] == [[1, 10, 64], [1, 10, 64], [10], [10]]
    assert all({s for s, _ in rc.SCHEMES[n]} == set(range(4)) for n in rc.NAMES) and {s for _, s, _ in rc.DEVICE_RUNS} == set(range(4))


# ---- 3: offspring counts ------------------------------------------------------------------------------------------------------------------
def _weights(N, P, seed):
    """uneven weights: a few particles carry several offspring, many carry none"""
    w = np.exp(1.5 * np.random.default_rng(seed).standard_normal((N, P)))
    return w / w.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("P", [64, 128])
def test_offspring_counts_of_systematic_and_stratified_resampling(P):
    N = 67
    w = _weights(N, P, 5 + P)
    u = rr.step_uniforms(rr.STRATIFIED, 0, 17, np.arange(N, dtype=np.uint64), 2, 3, P)
    anc = {s: rr.ancestors(s, w, u)[0] for s in (rr.MULTINOMIAL, rr.STRATIFIED, rr.SYSTEMATIC)}
    assert (P * w).max() > 4.0 and ((P * w) < 0.5).mean() > 0.2
    rc.hold_offspring(rr.SYSTEMATIC, anc[rr.SYSTEMATIC], w)
    rc.hold_offspring(rr.STRATIFIED, anc[rr.STRATIFIED], w)
    assert np.any(anc[rr.SYSTEMATIC] != anc[rr.STRATIFIED])
    # the check can fail: multinomial ancestors are not ordered, and ordered they still break either bound
    for s in (rr.SYSTEMATIC, rr.STRATIFIED):
        with pytest.raises(AssertionError, match="decrease"):
            rc.hold_offspring(s, anc[rr.MULTINOMIAL], w)
        with pytest.raises(AssertionError, match="offspring count"):
            rc.hold_offspring(s, np.sort(anc[rr.MULTINOMIAL], axis=1), w)
    # every scheme's counts have the means P W_j: the averages over the series' uniforms of one weight vector
    w1 = np.tile(w[:1], (4096, 1))
    u = rr.step_uniforms(rr.STRATIFIED, 0, 19, np.arange(4096, dtype=np.uint64), 0, 7, P)
    for s in (rr.STRATIFIED, rr.SYSTEMATIC):
        n_j = rc.offspring(rr.ancestors(s, w1, u)[0], P)
        se = n_j.std(axis=0, ddof=1) / np.sqrt(4096) + 1e-12
        assert np.all(np.abs(n_j.mean(axis=0) - P * w[0]) <= 5.0 * se + 1e-9)


# ---- 4: the law of a Metropolis chain -------------------------------------------------------------------------------------------------------
def _metropolis_kernel(w):
    """K[k][j] = P(next = j | now = k): j proposed uniformly, accepted with probability min(1, W_j / W_k) (always from a k of weight 0)."""
    P = len(w)
    with np.errstate(divide="ignore", invalid="ignore"):
        acc = np.where(w[:, None] > 0.0, np.minimum(1.0, w[None, :] / w[:, None]), 1.0)
    K = acc / P
    K[np.arange(P), np.arange(P)] = 0.0
    K[np.arange(P), np.arange(P)] = 1.0 - K.sum(axis=1)
    return K


@pytest.mark.parametrize("b", [1, 10])
def test_metropolis_ancestors_have_the_law_of_the_chain(b):
    P, R, zero = 64, 4096, 5
    w = np.exp(0.5 * np.random.default_rng(8).standard_normal(P))
    w[zero] = 0.0
    w = w / w.sum()
    Kb = np.linalg.matrix_power(_metropolis_kernel(w), b)
    np.testing.assert_allclose(Kb.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    u = rr.step_uniforms(rr.METROPOLIS, b, 29, np.arange(R, dtype=np.uint64), 1, 4, P)
    anc, _, margin = rr.ancestors(rr.METROPOLIS, np.tile(w, (R, 1)), u, b)
    assert margin >= 0.0 and anc.min() >= 0 and anc.max() < P
    for start in (0, zero):          # a particle of positive weight, and the one of weight 0: it always moves
        expect = R * Kb[start]
        seen = np.bincount(anc[:, start], minlength=P)
        cells = expect > 0.0
        assert np.all(seen[~cells] == 0)          # where the chain cannot be: no mass
        chi2 = float((((seen - expect) ** 2)[cells] / expect[cells]).sum())
        bound = float(stats.chi2.ppf(1.0 - 1e-6, cells.sum() - 1))
        print(f"b = {b}, start {start}: chi-square {chi2:.1f} on {cells.sum() - 1} degrees of freedom, bound {bound:.1f}; smallest expected count {expect[cells].min():.1f}")
        assert chi2 <= bound
    assert Kb[0, zero] == 0.0 and np.all(anc[:, np.arange(P) != zero] != zero)          # the weight 0 gets no mass beyond its own start's
    # the check is sharp: the law of another number of steps (2 for 1, 1 for 10) is refused
    other = R * np.linalg.matrix_power(_metropolis_kernel(w), 2 if b == 1 else 1)[0]
    seen = np.bincount(anc[:, 0], minlength=P)
    cells = other > 0.0
    assert float((((seen - other) ** 2)[cells] / other[cells]).sum()) > float(stats.chi2.ppf(1.0 - 1e-6, cells.sum() - 1))


# ---- 5: unbiased for the exact grid likelihood ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [rr.STRATIFIED, rr.SYSTEMATIC], ids=["stratified", "systematic"])
@pytest.mark.parametrize("name", gr.NAMES)
def test_likelihood_estimate_stays_unbiased(name, scheme):
    out = rr.run(**gr.args_of("pf", name), resample=scheme, mh_steps=0)
    gr.hold_likelihood("pf", name, out)


# ---- 6: signatures and refusals -------------------------------------------------------------------------------------------------------------
def _strip(src):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def test_header_ctypes_jni_and_scala_agree_on_the_new_export():
    lib = _lib.load()
    assert hasattr(lib, "dlm_pf_resampled")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dlm_engine.h")).read(), flags=re.S)
    split = lambda name: [" ".join(p.split()) for p in re.search(r"int " + name + r"\(([^;]*)\);", hdr).group(1).split(",")]
    params, base = split("dlm_pf_resampled"), split("dlm_pf_batch")
    assert params[:4] == base[:4] and params[4] == "const dlm_resample_desc* resample" and params[5:] == base[4:]          # then exactly dlm_pf_batch's
    name, res, args = next(s for s in _lib.SYMBOLS if s[0] == "dlm_pf_resampled")
    _, _, base_args = next(s for s in _lib.SYMBOLS if s[0] == "dlm_pf_batch")
    assert res is ctypes.c_int and len(args) == len(params) == 15
    assert args[:4] == base_args[:4] and args[4] == ctypes.POINTER(_lib.ResampleDesc) and args[5:] == base_args[4:]
    fields = re.search(r"typedef struct \{([^}]*)\} dlm_resample_desc;", hdr).group(1)
    assert re.findall(r"int32_t (\w+);", fields) == [f for f, _ in _lib.ResampleDesc._fields_] == ["scheme", "mh_steps"]
    assert ctypes.sizeof(_lib.ResampleDesc) == 8
    enum = re.search(r"enum \{ (DLM_RESAMPLE_MULTINOMIAL[^}]*)\};", hdr).group(1)
    assert [int(x.split("=")[1]) for x in enum.split(",")] == [_lib.RESAMPLE_MULTINOMIAL, _lib.RESAMPLE_STRATIFIED, _lib.RESAMPLE_SYSTEMATIC,
                                                                _lib.RESAMPLE_METROPOLIS] == [rr.MULTINOMIAL, rr.STRATIFIED, rr.SYSTEMATIC, rr.METROPOLIS]
    # the descs cross the JNI as scalars in field order: particleFilter's parameters and the two of dlm_resample_desc behind dlm_pf_desc's
    jni = _strip(open(os.path.join(ROOT, "integration", "jni", "dlm_jni.cpp")).read())
    scala = _strip(open(os.path.join(ROOT, "integration", "scala", "Batched.scala")).read())
    names = lambda text: [p.split()[-1].rstrip(":") for p in text.split(",")]
    jni_of = lambda f: names(re.search(r"Native_" + f + r"\s*\(([^)]*)\)", jni).group(1))[2:]
    scala_of = lambda f: [p.split(":")[0].strip() for p in re.search(r"@native\s+def\s+" + f + r"\s*\(([^)]*)\)", scala).group(1).split(",")]
    old, new = jni_of("particleFilter"), jni_of("particleFilterResampled")
    assert len(new) == 19 and new == old[:8] + ["scheme", "mhSteps"] + old[8:] and scala_of("particleFilterResampled") == new
    assert "dlm_pf_resampled(" in jni and "const dlm_resample_desc rs{scheme, mhSteps}" in jni


def test_scheme_kernel_has_no_scratch_and_no_spills():
    """dlm_pf.o: every instantiation of k_pf_scheme keeps everything in registers, as k_pf does (whose counts tests/test_lw_host.py pins)."""
    from code_object import kernel_resources
    res = [kernel_resources("dlm_pf.o", f"k_pf_schemeILi{d}E") for d in range(1, 17)]
    print("k_pf_scheme registers (VGPRs + AGPRs), d = 1 .. 16:", [r[2] for r in res])
    assert all(r[:2] == (0, 0) for r in res)


def test_blocks_of_the_metropolis_chains_agree_with_dlm_draws():
    src = open(os.path.join(ROOT, "bayesian_dlms_amd", "csrc", "dlm_draws.h")).read()
    assert f"DLM_PF_BLOCK_MH0 = {rr.BLOCK_MH0}u" in src and f"DLM_PF_MAX_MH_STEPS = {rr.MAX_MH_STEPS};" in src
    assert rr.MAX_MH_STEPS == _lib.PF_MAX_MH_STEPS == 64 and rr.BLOCK_MH0 + rr.MAX_MH_STEPS <= 256
    top = re.search(r"DLM_PF_BLOCK_POISSON = (\d+)u", src)          # the forecast's last block: GAMMA_B + GAMMA_ATTEMPTS (its boost)
    assert rr.BLOCK_MH0 > int(top.group(1)) + 32 + 32 + 1 + 32 and "DLM_PF_BLOCK_MH0 > DLM_PF_BLOCK_GAMMA_B + DLM_PF_GAMMA_ATTEMPTS" in src


def test_python_layer_refuses_what_the_engine_refuses():
    for bad in (4, -1, "systematic", None, True, 1.0):
        with pytest.raises(EngineError, match="RESAMPLE_"):
            check_pf_resample(bad, 0)
    for b in (0, 65, -3):
        with pytest.raises(EngineError, match="1 <= mh_steps <= 64"):
            check_pf_resample(_lib.RESAMPLE_METROPOLIS, b)
        with pytest.raises(EngineError, match="1 <= mh_steps <= 64"):
            Resampling.metropolis(b)
    for s in (_lib.RESAMPLE_MULTINOMIAL, _lib.RESAMPLE_STRATIFIED, _lib.RESAMPLE_SYSTEMATIC):
        with pytest.raises(EngineError, match="must be 0 under every other scheme"):
            check_pf_resample(s, 10)
        with pytest.raises(EngineError, match="must be 0 under every other scheme"):
            Resampling(s, 1)
    assert check_pf_resample(_lib.RESAMPLE_METROPOLIS, 64) == (3, 64) and check_pf_resample(np.int64(2), 0) == (2, 0)
    # Engine.particle_filter refuses before it touches its engine, its model or its data
    for kw in (dict(resample=7), dict(resample=_lib.RESAMPLE_METROPOLIS, mh_steps=0), dict(resample=_lib.RESAMPLE_METROPOLIS, mh_steps=65),
               dict(resample=_lib.RESAMPLE_SYSTEMATIC, mh_steps=10), dict(mh_steps=1)):
        with pytest.raises(EngineError, match="RESAMPLE_|mh_steps"):
            Engine.particle_filter(None, None, None, None, family=0, n_particles=64, **kw)
    with pytest.raises(EngineError, match="RESAMPLE_"):
        ParticleFilter(64, -1, 9)


@pytest.mark.parametrize("scheme,b", [(rr.MULTINOMIAL, 0), (rr.STRATIFIED, 0), (rr.SYSTEMATIC, 0), (rr.METROPOLIS, 10)],
                         ids=["multinomial", "stratified", "systematic", "metropolis10"])
def test_binding_reaches_its_export_through_the_one_call_path(scheme, b):
    """tests/test_engine_calls_host.py's recording stub of the C ABI under every scheme: the multinomial scheme goes to dlm_pf_batch, as it
    always has, every other one to dlm_pf_resampled with arguments that convert to the declared types and the descriptor the caller asked
    for; under DLM_OPT_ASYNC every array the call was handed is kept until sync(), and without the flag nothing is."""
    import test_engine_calls_host as calls
    symbol = "dlm_pf_batch" if scheme == rr.MULTINOMIAL else "dlm_pf_resampled"
    eng = calls._engine()
    result = eng.particle_filter(calls.MAT_PF, calls.PAR, calls.Y1, flags=calls.ASYNC, resample=scheme, mh_steps=b, **calls.pf)
    (name, args, addresses), = [c for c in eng.lib.calls if c[0].startswith("dlm_pf")]
    assert name == symbol and addresses
    if scheme != rr.MULTINOMIAL:
        desc = args[4]
        assert isinstance(desc, _lib.ResampleDesc) and (desc.scheme, desc.mh_steps) == (scheme, b)
    kept, own = calls._addresses(eng._keep), calls._addresses(result)
    assert addresses - own <= kept and addresses <= kept
    eng.sync()
    assert eng._keep == []
    eng = calls._engine()
    eng.particle_filter(calls.MAT_PF, calls.PAR, calls.Y1, resample=scheme, mh_steps=b, **calls.pf)
    assert eng._keep == [] and symbol in eng.lib.seen()


def test_resampling_names_mirror_the_reference_s():
    assert (Resampling.multinomial, Resampling.stratified, Resampling.systematic) == (Resampling(0), Resampling(1), Resampling(2))
    assert Resampling.metropolis(10) == Resampling(_lib.RESAMPLE_METROPOLIS, 10) and not Resampling.metropolis(10).unbiased
    assert ParticleFilter(128).resample == Resampling.multinomial and ParticleFilter(128, 5, Resampling.systematic).resample.scheme == 2
    assert ParticleFilter(128, -1, _lib.RESAMPLE_STRATIFIED).resample == Resampling.stratified


def test_metropolis_dglm_refuses_a_biased_likelihood_estimate():
    mod = Dglm.poisson(Dlm.polynomial(1))
    init = DlmParameters(np.eye(1), 0.2 * np.eye(1), np.array([0.3]), 0.5 * np.eye(1))
    ys = (np.arange(1.0, 7.0), np.ones(6))
    with pytest.raises(EngineError, match="biased.*wrong posterior"):          # by the call itself: no engine, nothing filtered
        Metropolis.dglm(mod, ys, Metropolis.symmetric_proposal(0.5), lambda p: 0.0, init, 128, None, 3, resample=Resampling.metropolis(10))
    for ok in (Resampling.multinomial, Resampling.stratified, Resampling.systematic):
        assert hasattr(Metropolis.dglm(mod, ys, Metropolis.symmetric_proposal(0.5), lambda p: 0.0, init, 128, None, 3, resample=ok), "__next__")
