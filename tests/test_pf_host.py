"""The bootstrap particle filter without a GPU: the restatement the kernel is held to (tests/pf_restatement.py) against what it must
compute -- the six log-densities against scipy.stats, the likelihood estimate against the Kalman filter's exact likelihood (unbiased; and
NOT unbiased with one quirk of the reference switched on), the filtering means against the Kalman filter's -- and the inputs of the GPU
tests (tests/pf_cases.py) against what makes them worth running: both branches of the resampling test taken, and no comparison of the
kernel's within a rounding error of flipping.  Then the build and the argument checks of the Python layer.

Bounds.  Densities: 64 * 2^-53 * (sum of the absolute values of the density's terms) -- the terms are each a few roundings off, scipy's
likewise.  Likelihood estimate and means: 5 standard errors, the standard error from the sample of 4096 replicates, the bound of the
project's invariance tests.  Margins: 1e-11, the tolerance of the GPU comparison (four orders of magnitude above double rounding); the
distance of 1 / sum W^2 from ANY integer, which the exact equality of the ESS output rests on, 1e-9: the sum of P <= 1024 squares in a
fixed order is good to 1e-13 relative, 1e-10 absolute at most."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pf_cases as pc  # noqa: E402
import pf_restatement as pr  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dglm import BatchedParameters, Dglm, Metropolis, ParticleFilter  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters  # noqa: E402
from bayesian_dlms_amd.engine import EngineError  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
SIGMAS = 5.0
MARGIN = 1e-11


# ---- densities ---------------------------------------------------------------------------------------------------------------------
def _close(val, ref, scale):
    assert np.all(np.isfinite(ref))
    err = np.abs(val - ref)
    bound = 64 * EPS * scale
    assert np.all(err <= bound), (float((err / bound).max()), float(err.max()))


ETA = np.linspace(-4.5, 4.5, 37)[:, None]


def test_gaussian_density():
    y, v = np.array([-3.0, 0.0, 0.7, 12.5]), 0.3
    val, scale = pr.log_density(pr.GAUSSIAN, y, ETA, v, terms=True)
    _close(val, stats.norm.logpdf(y, ETA, np.sqrt(v)), scale)


def test_poisson_density_truncates_y_to_an_integer():
    y = np.array([0.0, 1.0, 3.0, 17.0, 250.0])
    val, scale = pr.log_density(pr.POISSON, y + 0.6, ETA, 1.0, terms=True)
    _close(val, stats.poisson.logpmf(y, np.exp(ETA)), scale)


def test_negative_binomial_density():
    y, logsize = np.array([0.0, 1.0, 4.0, 60.0]), 1.3
    size, mu = np.exp(logsize), np.exp(ETA)
    val, scale = pr.log_density(pr.NEGBIN, y, ETA, logsize, terms=True)
    _close(val, stats.nbinom.logpmf(y, size, size / (size + mu)), scale)


def test_zero_inflated_poisson_density():
    y, v = np.array([0.0, 5e-6, 1.0, 3.0, 40.0]), -0.4
    p = 1.0 / (1.0 + np.exp(-v))
    pois = stats.poisson.logpmf(np.round(y), np.exp(ETA))
    ref = np.where(np.abs(y) < 1e-5, np.log(p + (1.0 - p) * np.exp(-np.exp(ETA))), np.log1p(-p) + pois)
    val, scale = pr.log_density(pr.ZIP, y, ETA, v, terms=True)
    _close(val, ref, scale)


def test_student_t_density_and_its_literal_normaliser():
    y, v, nu = np.array([-2.0, 0.1, 9.0]), 0.25, 7.0
    val, scale = pr.log_density(pr.STUDENTT, y, ETA, v, nu, terms=True)
    _close(val, stats.t.logpdf(y, nu, loc=ETA, scale=np.sqrt(v)), scale)
    lit = pr.log_density(pr.STUDENTT, y, ETA, v, nu, q39=True)          # Q39: 0.5 log(pi nu scale) where scale^2 belongs
    np.testing.assert_allclose(lit - val, 0.5 * np.log(np.sqrt(v)), rtol=0, atol=1e-13)


def test_beta_density_and_its_clamp():
    y, v = np.array([0.02, 0.4, 0.93]), 0.01
    eta = np.concatenate([ETA[:, 0], [-5.0, 5.0, -5.000001, 5.000001, -40.0, 40.0]])[:, None]
    val, scale = pr.log_density(pr.BETA, y, eta, v, terms=True)
    mean = 1.0 / (1.0 + np.exp(-eta))
    a = mean * (1.0 - mean) / v
    al, be = mean * (a - 1.0), (1.0 - mean) * (a - 1.0)
    inside = (np.abs(eta) <= 5.0) & (al > 0) & (be > 0)
    rows = inside[:, 0]
    assert rows.sum() >= 30 and (~rows).sum() >= 4
    _close(val[rows], stats.beta.logpdf(y, al[rows], be[rows]), scale[rows])
    # beyond the clamp the mean is 0 or 1 and the Beta parameters are not positive: the reference's constructor throws, scipy answers NaN,
    # the filter gives the particle the weight 0 (Q41)
    assert np.all(val[~rows] == -np.inf)
    clamped = np.abs(eta[:, 0]) > 5.0
    assert np.all(np.isnan(stats.beta.logpdf(y, np.where(eta[clamped] > 0, 1.0, 0.0) * -1.0, -1.0)))
    # a y outside (0, 1) has no density for any particle
    assert np.all(np.isnan(pr.log_density(pr.BETA, 1.5, ETA, v)))


# ---- the likelihood estimate, the quirks, the filtering means -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(which, diffuse=False, **over):
        key = (which, diffuse, tuple(sorted(over.items())))
        if key not in cache:
            cache[key] = pr.run(**pc.unbiased_args(which, diffuse, **over))
        return cache[key]
    return get


@pytest.mark.parametrize("which", ["level", "dense"])
def test_likelihood_estimate_is_unbiased(runs, which):
    _, ll = pc.exact(which)
    m, se = pc.unbiasedness(runs(which)["ll"], ll)
    print(f"{which}: mean exp(ll_hat - ll) = {m:.5f} +- {se:.5f}, share of steps resampled {runs(which)['resample_share']:.2f}")
    assert abs(m - 1.0) <= SIGMAS * se
    assert 0.05 < runs(which)["resample_share"] < 0.95          # the estimate went through both branches


@pytest.mark.parametrize("quirk", ["q37", "q38"])
def test_the_same_check_fails_with_one_quirk_switched_on(runs, quirk):
    """Q37: the weights of a step that did not resample are forgotten.  Q38: a missing step does not advance the time (the series has one
    missing value)."""
    _, ll = pc.exact("level")
    m, se = pc.unbiasedness(runs("level", **{quirk: True})["ll"], ll)
    print(f"{quirk}: mean exp(ll_hat - ll) = {m:.5f} +- {se:.5f}")
    assert abs(m - 1.0) > SIGMAS * se


@pytest.mark.parametrize("which", ["level", "dense"])
def test_filtering_means_match_the_kalman_filter(runs, which):
    """(on the diffuse models: tests/pf_cases.py says why)"""
    ms, ll = pc.exact(which, True)
    r = runs(which, True)
    z = pc.mean_z(r["mean"], ms)
    m, se = pc.unbiasedness(r["ll"], ll)
    print(f"{which}: largest |mean - Kalman| = {z.max():.2f} standard errors; mean exp(ll_hat - ll) = {m:.5f} +- {se:.5f}")
    assert np.all(z <= SIGMAS)
    assert abs(m - 1.0) <= SIGMAS * se
    # the check is sharp: the cloud's mean WITHOUT the weights (no observation at all) is tens of standard errors away
    blind = pr.run(**dict(pc.unbiased_args(which, True), y=np.full((256, pc.UNBIASED_T), np.nan)))["mean"].mean(axis=0)
    se_mean = r["mean"].std(axis=0, ddof=1) / np.sqrt(pc.REPLICATES)
    assert (np.abs(ms - blind) / se_mean).max() > 50.0


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in pc.TABLE])
def test_table_entry_takes_both_branches_with_margins(name):
    r = pc.reference(name)
    print(f"{name}: share {r['resample_share']:.2f}, margins search {r['margin_search']:.2e}, n0 {r['margin_n0']:.2e}, integer {r['margin_int']:.2e}")
    assert np.all(r["status"] == 0) and np.all(np.isfinite(r["ll"]))
    if name in pc.FORCED:          # n0 = P, n0 = 0: one branch by construction
        assert r["resample_share"] == pc.FORCED[name]
    else:
        assert 0.10 <= r["resample_share"] <= 0.90
    assert r["margin_search"] >= MARGIN and r["margin_n0"] >= MARGIN          # (an entry that fails: change its seed, not the bound)
    assert r["margin_int"] >= 1e-9


def test_table_covers_the_shapes():
    t = pc.TABLE
    assert {c["P"] for c in t} >= {64, 128, 192, 1024} and {c["d"] for c in t} >= {1, 2, 3, _lib.PF_MAX_D}
    assert {c["T"] for c in t} >= {1, 2, 24} and {c["N"] for c in t} >= {1, 5, 67}
    assert {c["family"] for c in t} == set(range(6)) and {c["literal"] for c in t} == {False, True}
    assert {c["n0"] for c in t} >= {-1, 0, 128} and any(c["per_series"] for c in t) and any(not c["per_series"] for c in t)
    assert any(set(c["missing"]) >= {0, c["T"] - 1} and len(c["missing"]) >= 3 for c in t)
    irr = pc.inputs("p192-d3-irregular")
    assert irr["G"].shape[0] == 3 and (irr["dt"][1:] == 0.0).sum() == 1
    a = pc.inputs("p192-d3-irregular")
    assert np.all(a["G"] != 0.0) and np.all(a["W"] != 0.0)          # dense G, full W


def test_restatement_reports_failures():
    kw = pc.run_args("family-beta")
    y = kw["y"].copy(); y[2, 5] = 1.5
    r = pr.run(**dict(kw, y=y))
    assert r["status"].tolist() == [0, 0, pr.ST_NONFINITE, 0, 0] and r["ll"][2] == -np.inf
    assert np.all(np.isfinite(r["mean"][2, :5])) and np.all(np.isnan(r["mean"][2, 5:])) and np.all(np.isnan(r["weights"][2]))
    good = pc.reference("family-beta")
    for k in ("ll", "mean", "ess", "cloud", "weights"):
        np.testing.assert_array_equal(np.delete(r[k], 2, axis=0), np.delete(good[k], 2, axis=0))
    W = np.array([[1.0, 2.0], [2.0, 1.0]])
    r = pr.run(**dict(kw, W=W))
    assert np.all(r["status"] == pr.ST_NOT_PD) and np.all(r["ll"] == -np.inf)


# ---- build and API ------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_call_with_the_header_s_signature():
    lib = _lib.load()
    assert hasattr(lib, "dlm_pf_batch")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dlm_engine.h")).read(), flags=re.S)
    decl = re.search(r"int dlm_pf_batch\(([^;]*)\);", hdr).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    name, res, args = next(s for s in _lib.SYMBOLS if s[0] == "dlm_pf_batch")
    assert res is ctypes.c_int and len(args) == len(params) == 14
    for p, a in zip(params, args):
        if "uint64_t" in p and "*" not in p:
            assert a is ctypes.c_uint64, p
        else:
            assert "*" in p and a in (ctypes.c_void_p, _lib._MP, _lib._PP, _lib._OP, ctypes.POINTER(_lib.PfDesc)), p
    fields = re.search(r"typedef struct \{([^}]*)\} dlm_pf_desc;", hdr).group(1)
    assert re.findall(r"int32_t (\w+);", fields) == [f for f, _ in _lib.PfDesc._fields_]
    enum = re.search(r"enum \{ (DLM_OBS_GAUSSIAN[^}]*)\};", hdr).group(1)
    assert [int(x.split("=")[1]) for x in enum.split(",")] == [_lib.OBS_GAUSSIAN, _lib.OBS_POISSON, _lib.OBS_NEGBIN, _lib.OBS_ZIP,
                                                                _lib.OBS_STUDENTT, _lib.OBS_BETA]
    src = open(os.path.join(ROOT, "bayesian_dlms_amd", "csrc", "dlm_draws.h")).read()
    assert f"DLM_KEY_PF = 0x{pr.KEY_PF:08X}u" in src and f"DLM_PF_BLOCK_RESAMPLE = {pr.BLOCK_RESAMPLE}u" in src
    assert "DLM_PF_SLOT_INIT = DLM_SLOT_TOP" in src and pr.SLOT_INIT == 0x1FFFFF


def _series(T=6, p=1):
    return np.arange(1.0, T + 1), np.zeros((T, p))[None] if p > 1 else np.zeros(T)


@pytest.mark.parametrize("n", [96, 2048, 0, 32])
def test_python_layer_refuses_particle_counts(n):
    with pytest.raises(EngineError, match="multiple of 64 between 64 and 1024"):
        ParticleFilter(n)


def test_python_layer_refuses_d_17_and_p_2():
    par = lambda d, p: DlmParameters(np.eye(p), np.eye(d), np.zeros(d), np.eye(d))
    with pytest.raises(EngineError, match="d <= 16, got d = 17"):
        ParticleFilter(128).filter(Dglm.poisson(Dlm.polynomial(17)), _series(), par(17, 1), None)
    two = Dlm.polynomial(1) * Dlm.polynomial(1)
    with pytest.raises(EngineError, match=r"univariate observation \(p = 1"):
        ParticleFilter(128).filter(Dglm.gaussian(two), _series(p=2), par(2, 2), None)
    with pytest.raises(ValueError, match="degrees of freedom"):
        Dglm.student_t(0, Dlm.polynomial(1))


def test_symmetric_proposal_keeps_diagonals_positive_and_off_diagonals_zero():
    rng = np.random.default_rng(5)
    N, d = 200, 3
    w = np.tile(np.diag([0.5, 2.0, 1e-3]), (N, 1, 1)); w[:, 0, 1] = w[:, 1, 0] = 0.1          # an off-diagonal entry goes in ...
    p = BatchedParameters(np.full((N, 1, 1), 0.7), w, np.zeros((N, d)), np.tile(np.eye(d), (N, 1, 1)))
    q = Metropolis.symmetric_proposal(0.05)(p, rng)
    idx = np.arange(d)
    for old, new in ((p.v, q.v), (p.w, q.w), (p.c0, q.c0)):
        k = old.shape[1]
        dg = new[:, np.arange(k), np.arange(k)]
        assert np.all(dg > 0) and np.all(new[:, ~np.eye(k, dtype=bool)] == 0.0)          # ... and none comes out
        lr = np.log(dg / old[:, np.arange(k), np.arange(k)])
        assert abs(lr.std() - np.sqrt(0.05)) < 0.03 and abs(lr.mean()) < 0.05          # log-scale moves of standard deviation sqrt(delta)
    step = q.m0 - p.m0
    assert abs(step.std() - 0.05) < 0.01          # additive on m0, standard deviation delta
    assert idx.size == d
    with pytest.raises(ValueError):
        Metropolis.symmetric_proposal(0.0)


def test_simulate_regular_and_the_pf_grid():
    from bayesian_dlms_amd.dglm import materialise_pf
    mod = Dglm.poisson(Dlm.polynomial(2) + Dlm.seasonal(12, 1))
    par = DlmParameters(np.eye(1), 0.01 * np.eye(4), np.array([1.0, 0.0, 0.0, 0.0]), 0.1 * np.eye(4))
    times, y, x = mod.simulate_regular(par, 40, rng=np.random.default_rng(3))
    assert y.shape == (40,) and x.shape == (40, 4) and np.all(y == np.round(y)) and np.all(y >= 0)
    mat = materialise_pf(mod, times)
    assert mat.dt[0] == 0.0 and np.all(mat.dt[1:] == 1.0) and mat.n_g == 1 and mat.g_index is None and mat.p == 1
    mat = materialise_pf(mod, np.array([1.0, 2.0, 4.0, 5.0, 7.0]))          # the seasonal block's G depends on dt
    assert mat.dt.tolist() == [0.0, 1.0, 2.0, 1.0, 2.0] and mat.n_g == 2 and mat.g_index.tolist() == [0, 0, 1, 0, 1]
