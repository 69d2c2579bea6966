"""The forecast of the factor stochastic-volatility models without a device: the NumPy restatement of the two kernels and of
the drivers' composition (tests/fsv_forecast_restatement.py) is held to closed-form laws, scipy and mpmath; every check is shown to reject
the restatement's mutants it is meant to catch; the drivers' argument checks; the engine's call path for the two new exports.

The law tests are conditions at 5 standard errors (about 6e-7 per comparison) computed from the KNOWN laws; their seeds are the constants
LAW_SEEDS below."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fsv_forecast_restatement as rs  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm  # noqa: E402
from bayesian_dlms_amd.dlmfsv import DlmFsv  # noqa: E402
from bayesian_dlms_amd.dlmfsvsys import DlmFsvSystem  # noqa: E402
from bayesian_dlms_amd.engine import EngineError  # noqa: E402
from bayesian_dlms_amd.factorsv import FactorSv  # noqa: E402

LAW_SEEDS = (11, 12, 13)
PHI, MU, SIG, A0, LAW_H, LAW_N, LAW_R = 0.9, -1.0, 0.3, 1.0, 8, 8, 1024


# ---- the mixture quantile ---------------------------------------------------------------------------------------------------------------
def mp_cdf(x, f, q):
    """(F(x), density(x)) of the mixture sum_c N(f_c, q_c) / C in 40 digits."""
    import mpmath as mp
    with mp.workdps(40):
        x = mp.mpf(float(x))
        F = D = mp.mpf(0)
        for fc, qc in zip(f, q):
            s = mp.sqrt(mp.mpf(float(qc)))
            z = (x - mp.mpf(float(fc))) / s
            F += mp.erfc(-z / mp.sqrt(2)) / 2
            D += mp.exp(-z * z / 2) / (s * mp.sqrt(2 * mp.pi))
        return F / len(f), D / len(f)


def residual_ok(x, f, q, prob):
    """The documented stopping rule: |F(q) - prob| <= density(q) spacing(q) + C 2^-52."""
    F, D = mp_cdf(x, f, q)
    return abs(float(F - prob)) <= float(D) * float(np.spacing(abs(x))) + len(f) * 2.0 ** -52


def mixed_scale(C, seed):
    """Components mixed in scale: variances spanning 1e-3 .. 1e3, means spread over +- 3."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-3.0, 3.0, C), 10.0 ** rng.uniform(-3.0, 3.0, C)


@pytest.mark.parametrize("prob", [0.001, 0.25, 0.5, 0.75, 0.975])
def test_one_component_is_the_normal_quantile(prob):
    from scipy.stats import norm
    for f, q in ((0.0, 1.0), (3.5, 1e-3), (-120.0, 1e3)):
        x = rs.mixture_quantile([f], [q], prob)
        want = norm.ppf(prob, loc=f, scale=math.sqrt(q))
        assert abs(x - want) <= 8 * np.spacing(abs(want)) + 4e-16 * math.sqrt(q) * (1.0 + abs(norm.ppf(prob)) / norm.pdf(norm.ppf(prob))), (f, q, x, want)


@pytest.mark.parametrize("C", [2, 63, 65, 1000])
def test_mixture_quantile_meets_the_residual_bound(C):
    f, q = mixed_scale(C, C)
    for prob in (0.025, 0.25, 0.75, 0.99):
        assert residual_ok(rs.mixture_quantile(f, q, prob), f, q, prob), (C, prob)


def test_residual_bound_rejects_the_average_gaussian():
    f, q = mixed_scale(65, 65)
    Q = np.zeros((1, 65, 1, 1, 1)); Q[0, :, 0, 0, 0] = q
    fm = f.reshape(1, 65, 1, 1)
    good = rs.mixture_summary(fm, Q, (0.75,))[2][0, 0, 0, 0]
    bad = rs.mixture_summary(fm, Q, (0.75,), mutant="average")[2][0, 0, 0, 0]
    assert residual_ok(good, f, q, 0.75) and not residual_ok(bad, f, q, 0.75)


def test_covariance_is_the_law_of_total_variance_and_rejects_the_mutant():
    rng = np.random.default_rng(5)
    C, p = 200, 3
    f = rng.normal(size=(1, C, 1, p))
    L = rng.normal(size=(C, p, p))
    Q = (L @ L.transpose(0, 2, 1) + np.eye(p)).reshape(1, C, 1, p, p)
    mean, cov, _, st = rs.mixture_summary(f, Q)
    want = Q[0, :, 0].mean(axis=0) + np.cov(f[0, :, 0].T, bias=True)
    np.testing.assert_allclose(cov[0, 0], want, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(mean[0, 0], f[0, :, 0].mean(axis=0), rtol=1e-13)
    assert st[0] == 0 and np.array_equal(cov[0, 0], cov[0, 0].T)
    assert not np.allclose(rs.mixture_summary(f, Q, mutant="cov")[1][0, 0], want, rtol=1e-3)


def test_bad_components_flag_their_row_and_cell():
    f = np.zeros((2, 4, 1, 2))
    Q = np.tile(np.eye(2), (2, 4, 1, 1, 1))
    Q[1, 2, 0, 1, 1] = 0.0
    f[0, 1, 0, 0] = np.inf
    mean, cov, quant, st = rs.mixture_summary(f, Q, (0.5,))
    assert list(st) == [_lib.ST_NONFINITE, _lib.ST_NOT_PD]
    assert np.isnan(quant[0, 0, 0]).all() and np.isfinite(quant[0, 0, 1]).all() and np.isnan(quant[1, 0, 1]).all() and np.isfinite(quant[1, 0, 0]).all()
    assert np.isnan(mean[0, 0, 0]) and np.isnan(cov[1, 0, 1]).all() and np.isfinite(cov[1, 0, 0, 0])


# ---- the law of the paths ---------------------------------------------------------------------------------------------------------------
def law_figures(seed, mutant=None):
    """The number of standard errors that the sample mean and variance of alpha_H and the sample mean of exp(alpha_H) over N R restated paths
    stand off their laws  N(mu + phi^H (alpha_0 - mu), sigma^2 (1 - phi^2H) / (1 - phi^2))  and its lognormal mean."""
    sv = np.tile([PHI, MU, SIG], (LAW_N, 1, 1))
    al, st = rs.sv_paths(sv, np.full((LAW_N, 1), A0), LAW_H, LAW_R, seed=seed, mutant=mutant)
    assert not st.any()
    x = al[:, :, 0, LAW_H].reshape(-1)
    n = x.size
    m = MU + PHI ** LAW_H * (A0 - MU)
    v = SIG * SIG * (1.0 - PHI ** (2 * LAW_H)) / (1.0 - PHI * PHI)
    lm, lv = math.exp(m + v / 2), (math.exp(v) - 1.0) * math.exp(2 * m + v)
    return (abs(x.mean() - m) / math.sqrt(v / n), abs(x.var(ddof=1) - v) / (v * math.sqrt(2.0 / (n - 1))), abs(np.exp(x).mean() - lm) / math.sqrt(lv / n))


@pytest.mark.parametrize("seed", LAW_SEEDS)
def test_paths_follow_the_ar1_law(seed):
    assert max(law_figures(seed)) < 5.0, law_figures(seed)


@pytest.mark.parametrize("mutant", ["step", "variance", "start"])
def test_law_test_rejects_the_path_mutants(mutant):
    assert max(law_figures(LAW_SEEDS[0], mutant)) > 5.0


def test_stationary_start_has_the_stationary_law():
    sv = np.tile([PHI, MU, SIG], (LAW_N, 1, 1))
    al, _ = rs.sv_paths(sv, None, 2, LAW_R, seed=LAW_SEEDS[1])
    v = SIG * SIG / (1.0 - PHI * PHI)
    for h in (0, 2):
        x = al[:, :, 0, h].reshape(-1)
        assert abs(x.mean() - MU) < 5.0 * math.sqrt(v / x.size) and abs(x.var(ddof=1) - v) < 5.0 * v * math.sqrt(2.0 / (x.size - 1))


def test_paths_are_a_pure_function_of_their_counter():
    """The prefix in R and the sharding through series_offset; and the status rows."""
    rng = np.random.default_rng(3)
    sv = np.stack([rng.uniform(-0.95, 0.95, (4, 2)), rng.normal(size=(4, 2)), rng.uniform(0.1, 0.5, (4, 2))], axis=2)
    a0 = rng.normal(size=(4, 2))
    full, _ = rs.sv_paths(sv, a0, 3, 128, seed=9, iteration=2)
    half, _ = rs.sv_paths(sv, a0, 3, 64, seed=9, iteration=2)
    assert np.array_equal(full[:, :64], half)
    lo, _ = rs.sv_paths(sv[:1], a0[:1], 3, 128, seed=9, iteration=2)
    hi, _ = rs.sv_paths(sv[1:], a0[1:], 3, 128, seed=9, iteration=2, series_offset=1)
    assert np.array_equal(np.concatenate([lo, hi]), full)
    assert not np.array_equal(full, rs.sv_paths(sv, a0, 3, 128, seed=9, iteration=3)[0])
    sv[0, 1, 0], sv[1, 0, 2], sv[2, 0, 1] = 1.0, 0.0, np.nan
    al, st = rs.sv_paths(sv, a0, 3, 64, seed=9)
    assert list(st) == [_lib.ST_NOT_PD, _lib.ST_NOT_PD, _lib.ST_NONFINITE, 0] and np.isnan(al[:3]).all() and np.isfinite(al[3]).all()


# ---- the composition ------------------------------------------------------------------------------------------------------------------
def toy(kind, N=2, M=3, T=6, beta0=False):
    """(mod, ys, draws, what compose takes beside them) of the smallest case: p = 3, d = 2, k = 1 (FactorSv: p = 3, k = 2)."""
    from bayesian_dlms_amd.dlm import materialise
    mod, ys, draws, prior = rs.toy_draws(kind, 3, 2, 2 if kind == "fsv" else 1, N=N, M=M, T=T, beta0=beta0)
    if kind == "fsv":
        return mod, ys, draws, {}
    return mod, ys, draws, dict(prior, train=rs.model_tables(materialise(mod, np.arange(1.0, T + 1))), ys=ys)


@pytest.mark.parametrize("kind", ["obs", "sys"])
def test_zero_loadings_and_one_draw_reduce_to_the_gaussian_forecast(kind):
    """beta = 0: the stream is diag(v) whatever the paths, so all M R components of the restated composition are the SAME Gaussian, and
    the restated summary must collapse to it: mean and cov are that component's (the restatement's own Kalman forecast from (m_T, C_T)) and
    the band is its normal quantile.  This holds the composition's bookkeeping and the summary, not the filter's arithmetic: agreement with
    api.forecast itself needs the device and is tests/test_fsv_forecast_gpu.py's."""
    from scipy.stats import norm
    from bayesian_dlms_amd.dlm import materialise
    H, T = 3, 6
    mod, ys, draws, extra = toy(kind, N=1, M=1, T=T, beta0=True)
    fore = rs.model_tables(materialise(mod, T + np.arange(1.0, H + 1)))
    mean, cov, quant, st = rs.compose(kind, draws, H, 64, fore=fore, probs=(0.25, 0.75), **extra)
    S, static = np.diag(draws["v"][0, 0]), np.diag(draws["static"][0, 0])
    rep = lambda A, L: np.broadcast_to(A, (L,) + A.shape)
    V, W = (S, static) if kind == "obs" else (static, S)
    _, _, mT, CT = rs.kalman(*extra["train"], extra["m0"], extra["C0"], rep(V, T), rep(W, T), ys[0])
    f, Q, _, _ = rs.kalman(*fore, mT, CT, rep(V, H), rep(W, H))
    np.testing.assert_allclose(mean[0], f, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(cov[0], Q, rtol=1e-11, atol=1e-12)
    sd = np.sqrt(np.diagonal(Q, axis1=1, axis2=2))
    np.testing.assert_allclose(quant[0, :, :, 1], f + sd * norm.ppf(0.75), rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(quant[0, :, :, 0], f + sd * norm.ppf(0.25), rtol=1e-11, atol=1e-12)
    assert not st.any()


def test_composition_is_unchanged_by_chunking_the_panels():
    from bayesian_dlms_amd.dlm import materialise
    H = 2
    mod, ys, draws, extra = toy("obs", N=2, M=2)
    fore = rs.model_tables(materialise(mod, 6 + np.arange(1.0, H + 1)))
    whole = rs.compose("obs", draws, H, 64, fore=fore, **extra)
    for n in range(2):
        part = rs.compose("obs", {key: a[:, n:n + 1] for key, a in draws.items()}, H, 64, fore=fore, series_offset=n, **dict(extra, ys=ys[n:n + 1]))
        for a, b in zip(whole[:3], part[:3]):
            assert np.array_equal(a[n:n + 1], b)
    assert not np.array_equal(whole[1][0], whole[1][1])


# ---- the drivers' argument checks (they come before any engine call) -----------------------------------------------------------------------
def test_driver_argument_checks():
    _, _, fsv, _ = toy("fsv")
    with pytest.raises(ValueError, match="multiple of 64"):
        FactorSv.forecast(fsv, 3, None, n_paths=100)
    with pytest.raises(ValueError, match=r"inside \(0, 1\)"):
        FactorSv.forecast(fsv, 3, None, probs=[0.5, 1.0])
    with pytest.raises(ValueError, match=r"inside \(0, 1\)"):
        FactorSv.forecast(fsv, 3, None, prob=1.0)
    with pytest.raises(ValueError, match="horizon"):
        FactorSv.forecast(fsv, 0, None)
    with pytest.raises(ValueError, match="lacks"):
        FactorSv.forecast({key: a for key, a in fsv.items() if key != "alpha"}, 3, None)
    with pytest.raises(ValueError, match=r"sv \[M\]\[N\]\[k\]\[3\]"):
        FactorSv.forecast(dict(fsv, sv=fsv["sv"][..., :2]), 3, None)
    kept = [FactorSv.State({key: fsv[key][m] for key in ("beta", "v", "sv")}, None, None, np.zeros(2, np.int32)) for m in range(3)]
    with pytest.raises(ValueError, match="keep the states"):
        FactorSv.forecast(kept, 3, None)
    for cls, kind, name in ((DlmFsv, "obs", "w"), (DlmFsvSystem, "sys", "V")):
        mod, ys, draws, extra = toy(kind)
        draws[name] = draws.pop("static")
        prior = dict(m0=extra["m0"], c0=extra["C0"])
        with pytest.raises(ValueError, match="regular unit time grid"):
            cls.forecast(mod, ys, draws, 3, None, times=np.array([1.0, 2.0, 3.0, 4.0, 5.0, 7.0]), **prior)
        with pytest.raises(ValueError, match="panels"):
            cls.forecast(mod, ys[:1], draws, 3, None, **prior)
        with pytest.raises(ValueError, match="m0 must be"):
            cls.forecast(mod, ys, draws, 3, None, m0=np.zeros(5), c0=extra["C0"])
        with pytest.raises(ValueError, match="lacks"):
            cls.forecast(mod, ys, {key: a for key, a in draws.items() if key != name}, 3, None, **prior)
        with pytest.raises(ValueError, match="multiple of 64"):
            cls.forecast(mod, ys, draws, 3, None, n_paths=65, **prior)


# ---- the engine's call path for the two exports (tests/test_engine_calls_host.py's stub: the exports are not *_batch symbols) ------------------
def test_engine_calls_keep_their_arrays_and_match_the_declarations():
    from test_engine_calls_host import ASYNC, _addresses, _engine
    sv = np.random.default_rng(0).uniform(0.1, 0.5, (3, 2, 3)).astype(np.float32)
    a0 = np.zeros((3, 2), np.float32)
    fq = np.ones((3 * 4, 2 + 1, 2 + 4), np.float32)
    calls = {"dlm_sv_paths": lambda e, f: e.sv_paths(sv, 5, 64, alpha0=a0, flags=f),
             "dlm_gaussian_mixture_summary": lambda e, f: e.gaussian_mixture_summary(3, 4, 2, 2, fq=fq, probs=(0.25, 0.75), flags=f)}
    for symbol, call in calls.items():
        eng = _engine()
        result = call(eng, ASYNC)
        kept, own = _addresses(eng._keep), _addresses(result)
        (name, args, addresses), = [c for c in eng.lib.calls if c[0] == symbol]
        assert addresses and addresses - own <= kept and addresses <= kept, symbol
        eng.sync()
        assert eng._keep == []
        eng = _engine()
        call(eng, 0)
        assert eng._keep == [] and symbol in eng.lib.seen()
    eng = _engine()
    calls["dlm_gaussian_mixture_summary"](eng, 0)
    desc = eng.lib.calls[-1][1][1]
    rec = 6
    assert (desc.N, desc.C, desc.H, desc.p, desc.nq) == (3, 4, 2, 2, 2) and (desc.f_nstride, desc.f_cstride, desc.f_tstride) == (4 * 3 * rec, 3 * rec, rec)
    assert eng.lib.address("dlm_gaussian_mixture_summary", 3) - eng.lib.address("dlm_gaussian_mixture_summary", 2) == 8 * 2          # Q = f + p doubles
    assert isinstance(eng.lib.calls[-1][1][4], ctypes.Array)
    with pytest.raises(EngineError, match="multiple of 64"):
        _engine().sv_paths(sv, 5, 96)
    with pytest.raises(EngineError, match=r"inside \(0, 1\)"):
        _engine().gaussian_mixture_summary(3, 4, 2, 2, fq=fq, probs=(0.0,))
    with pytest.raises(EngineError, match="either fq"):
        _engine().gaussian_mixture_summary(3, 4, 2, 2, probs=(0.5,))
    with pytest.raises(EngineError, match="smaller than"):
        _engine().gaussian_mixture_summary(3, 4, 2, 2, Q=np.ones(10), probs=(0.5,))
