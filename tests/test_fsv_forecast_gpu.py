"""dlm_sv_paths and dlm_gaussian_mixture_summary on the GPU, and the three forecast drivers built on them.

PATHS against the restatement (tests/fsv_forecast_restatement.py) draw for draw, at the tolerance the factor-SV GPU tests use for draws
(rtol 1e-11, atol 1e-12: the device's log, cos and exp differ from NumPy's in the last bits, and with |phi| <= 0.95 the recursion amplifies a
rounding by at most 1 / (1 - phi) = 20); both start modes, the prefix in R, the sharding, the status rows.

SUMMARY against mpmath (50 digits).  The bounds are derived, not tuned.  With T_ij = sum_c (|Q_c,ij| + |f_ci f_cj|) / C and A_i = sum_c |f_ci| / C:
a sum of C terms in ANY order carries at most (C - 1) 2^-53 sum |terms| (first order), the products, the division by C and the final
subtraction one rounding each, so
  |mean_i - exact| <= C 2^-52 A_i,      |cov_ij - exact| <= C 2^-52 (T_ij + A_i A_j)
(for C = 1 the right sides are exactly the sum of the individual roundings).  Every quantile obeys the documented stopping rule
  |F_mp(q) - prob| <= density(q) spacing(q) + C 2^-52.
cov is symmetric bit for bit; a bad Q flags its row and cell.

DRIVERS against the restated composition at the draws' tolerance, chunked and unchunked bit for bit, and with beta = 0 against api.forecast."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fsv_forecast_restatement as rs  # noqa: E402

from bayesian_dlms_amd import _lib, api  # noqa: E402
from bayesian_dlms_amd.dlm import DlmParameters, materialise  # noqa: E402
from bayesian_dlms_amd.dlmfsv import DlmFsv  # noqa: E402
from bayesian_dlms_amd.dlmfsvsys import DlmFsvSystem  # noqa: E402
from bayesian_dlms_amd.engine import Engine, EngineError  # noqa: E402
from bayesian_dlms_amd.factorsv import FactorSv  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-11, 1e-12
PROBS = (0.25, 0.9)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


# ---- paths ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def path_inputs(k):
    rng = np.random.default_rng([3, k])
    sv = np.stack([rng.uniform(-0.95, 0.95, (3, k)), rng.normal(size=(3, k)), rng.uniform(0.1, 0.5, (3, k))], axis=2)
    sv[0, 0, 0] = 0.95
    a0 = rng.normal(size=(3, k))
    sv.setflags(write=False); a0.setflags(write=False)
    return sv, a0


@pytest.mark.parametrize("H", [1, 2, 8])
@pytest.mark.parametrize("R", [64, 128, 1024])
@pytest.mark.parametrize("k", [1, 2, 8])
def test_paths_against_the_restatement(eng, k, R, H):
    sv, a0 = path_inputs(k)
    for start in (a0, None):
        out = eng.sv_paths(sv, H, R, alpha0=start, iteration=5, seed=77, series_offset=3)
        want, st = rs.sv_paths(sv, start, H, R, seed=77, series_offset=3, iteration=5)
        assert out["alpha"].shape == (3, R, k, H + 1) and not out["status"].any() and not st.any()
        np.testing.assert_allclose(out["alpha"], want, rtol=RTOL, atol=ATOL)
        if start is not None:
            assert np.array_equal(out["alpha"][..., 0], np.broadcast_to(a0[:, None, :], (3, R, k)))


def test_paths_prefix_sharding_and_device_memory(eng):
    import torch
    sv, a0 = path_inputs(2)
    full = eng.sv_paths(sv, 4, 128, alpha0=a0, iteration=1, seed=5)["alpha"]
    assert np.array_equal(eng.sv_paths(sv, 4, 64, alpha0=a0, iteration=1, seed=5)["alpha"], full[:, :64])
    assert np.array_equal(eng.sv_paths(sv, 4, 1024, alpha0=a0, iteration=1, seed=5)["alpha"][:, :128], full)
    parts = [eng.sv_paths(sv[n:n + 1], 4, 128, alpha0=a0[n:n + 1], iteration=1, seed=5, series_offset=n)["alpha"] for n in range(3)]
    assert np.array_equal(np.concatenate(parts), full)
    dev = eng.sv_paths(torch.as_tensor(np.array(sv), device="cuda:0"), 4, 128, alpha0=torch.as_tensor(np.array(a0), device="cuda:0"), iteration=1, seed=5)
    assert np.array_equal(dev["alpha"].cpu().numpy(), full)
    for other in (dict(iteration=2, seed=5), dict(iteration=1, seed=6)):
        assert not np.array_equal(eng.sv_paths(sv, 4, 128, alpha0=a0, **other)["alpha"], full)
    free = eng.sv_paths(sv, 4, 128, iteration=1, seed=5)["alpha"]
    assert np.array_equal(eng.sv_paths(sv, 4, 64, iteration=1, seed=5)["alpha"], free[:, :64]) and not np.array_equal(free[..., 0], full[..., 0])


def test_paths_status_rows_and_argument_errors(eng):
    sv, a0 = (np.array(a) for a in path_inputs(2))
    good = eng.sv_paths(sv, 3, 64, alpha0=a0, seed=9)["alpha"]
    sv = np.concatenate([sv, sv[:2]])
    a0 = np.concatenate([a0, a0[:2]])
    sv[0, 1, 0], sv[1, 0, 2], sv[3, 0, 1], a0[4, 1] = -1.0, 0.0, np.nan, np.inf
    out = eng.sv_paths(sv, 3, 64, alpha0=a0, seed=9)
    assert list(out["status"]) == [_lib.ST_NOT_PD, _lib.ST_NOT_PD, 0, _lib.ST_NONFINITE, _lib.ST_NONFINITE]
    assert np.isnan(out["alpha"][[0, 1, 3, 4]]).all() and np.array_equal(out["alpha"][2], good[2])
    assert list(rs.sv_paths(sv, a0, 3, 64, seed=9)[1]) == list(out["status"])
    for bad in (dict(horizon=3, n_paths=96), dict(horizon=3, n_paths=2048), dict(horizon=0, n_paths=64)):
        with pytest.raises(EngineError):
            eng.sv_paths(sv, **bad)
    with pytest.raises(EngineError, match="1 <= k <= 8"):
        eng.sv_paths(np.zeros((1, 9, 3)), 3, 64)


# ---- summary -----------------------------------------------------------------------------------------------------------------------------
N_ROWS = 2
# (C, p, H, layout): "fq" the filter's records (f and Q inside one buffer, record 0 skipped), "stream" a variance stream with f = NULL.
# 4100 is past the 4096 components a cell holds in LDS
CASES = [(1, 1, 1, "fq"), (1, 3, 3, "stream"), (63, 3, 3, "fq"), (64, 3, 1, "stream"), (64, 1, 3, "fq"), (65, 64, 1, "fq"), (65, 3, 3, "stream"),
         (1000, 3, 3, "fq"), (1000, 1, 1, "stream"), (63, 64, 1, "stream"), (4100, 1, 1, "fq"), (4100, 3, 1, "stream")]


@functools.lru_cache(maxsize=None)
def mixture_case(C, p, H, layout):
    """Inputs mixed in scale (Q_ii spanning 1e-3 .. 1e3) and their 50-digit summary, computed once and read-only."""
    import mpmath as mp
    rng = np.random.default_rng([C, p, H, len(layout)])
    scale = 10.0 ** rng.uniform(-1.5, 1.5, (N_ROWS, C, H, p))
    L = rng.normal(size=(N_ROWS, C, H, p, p)) * 0.3 + np.eye(p)
    Q = (L @ np.swapaxes(L, -1, -2)) * scale[..., :, None] * scale[..., None, :]
    Q = 0.5 * (Q + np.swapaxes(Q, -1, -2))
    f = None if layout == "stream" else rng.uniform(-3.0, 3.0, (N_ROWS, C, H, p)) * scale
    fz = np.zeros((N_ROWS, C, H, p)) if f is None else f
    mean, cov, bm, bc = (np.empty(s) for s in ((N_ROWS, H, p), (N_ROWS, H, p, p), (N_ROWS, H, p), (N_ROWS, H, p, p)))
    with mp.workdps(50):
        for n in range(N_ROWS):
            for h in range(H):
                fm = [[mp.mpf(x) for x in fz[n, :, h, i]] for i in range(p)]
                m = [mp.fsum(col) / C for col in fm]
                A = np.abs(fz[n, :, h]).sum(axis=0) / C
                for i in range(p):
                    mean[n, h, i] = float(m[i])
                    bm[n, h, i] = C * 2.0 ** -52 * A[i]
                    for j in range(i, p):
                        s = mp.fsum(mp.mpf(q) + a * b for q, a, b in zip(Q[n, :, h, i, j], fm[i], fm[j])) / C - m[i] * m[j]
                        cov[n, h, i, j] = cov[n, h, j, i] = float(s)
                        T = (np.abs(Q[n, :, h, i, j]) + np.abs(fz[n, :, h, i] * fz[n, :, h, j])).sum() / C
                        bc[n, h, i, j] = bc[n, h, j, i] = C * 2.0 ** -52 * (T + A[i] * A[j])
    out = {"f": f, "Q": Q, "mean": mean, "cov": cov, "bound_mean": bm, "bound_cov": bc}
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out


def run_summary(eng, case, C, p, H, layout, probs=PROBS):
    if layout == "stream":
        return eng.gaussian_mixture_summary(N_ROWS, C, H, p, Q=np.ascontiguousarray(case["Q"]).reshape(N_ROWS * C, H, p * p), probs=probs)
    fq = np.full((N_ROWS * C, H + 1, p + p * p), np.nan)          # record 0 is never read
    fq[:, 1:, :p] = case["f"].reshape(N_ROWS * C, H, p)
    fq[:, 1:, p:] = case["Q"].reshape(N_ROWS * C, H, p * p)
    return eng.gaussian_mixture_summary(N_ROWS, C, H, p, fq=fq, probs=probs)


def mp_residual(x, f, q, prob):
    """(|F_mp(x) - prob|, density(x)) of the marginal mixture in 50 digits."""
    import mpmath as mp
    with mp.workdps(50):
        x = mp.mpf(float(x))
        F = D = mp.mpf(0)
        for fc, qc in zip(f, q):
            s = mp.sqrt(mp.mpf(float(qc)))
            z = (x - mp.mpf(float(fc))) / s
            F += mp.erfc(-z / mp.sqrt(2)) / 2
            D += mp.exp(-z * z / 2) / (s * mp.sqrt(2 * mp.pi))
        return abs(float(F / len(f) - mp.mpf(prob))), float(D / len(f))


@pytest.mark.parametrize("case_id", CASES, ids=lambda c: f"C{c[0]}-p{c[1]}-H{c[2]}-{c[3]}")
def test_summary_against_mpmath(eng, case_id):
    C, p, H, layout = case_id
    case = mixture_case(*case_id)
    out = run_summary(eng, case, *case_id)
    assert not out["status"].any()
    mean, cov, quant = out["mean"], out["cov"].reshape(N_ROWS, H, p, p), out["quant"]
    em, ec = np.abs(mean - case["mean"]), np.abs(cov - case["cov"])
    worst = lambda e, b: float(np.max(np.where(b > 0, e / np.where(b > 0, b, 1.0), np.where(e > 0, np.inf, 0.0))))
    print(f"mean: worst error / bound {worst(em, case['bound_mean']):.3f}; cov: {worst(ec, case['bound_cov']):.3f}")
    assert (em <= case["bound_mean"]).all() and (ec <= case["bound_cov"]).all()
    assert np.array_equal(cov, np.swapaxes(cov, -1, -2))
    fz = np.zeros((N_ROWS, C, H, p)) if case["f"] is None else case["f"]
    cells = [(n, h, i) for n in range(N_ROWS) for h in range(H) for i in range(p)]
    ratio = 0.0
    for n, h, i in cells:
        for iq, prob in enumerate(PROBS):
            x = quant[n, h, i, iq]
            res, dens = mp_residual(x, fz[n, :, h, i], case["Q"][n, :, h, i, i], prob)
            bound = dens * float(np.spacing(abs(x))) + C * 2.0 ** -52
            ratio = max(ratio, res / bound)
            assert res <= bound, (n, h, i, prob, x, res, bound)
    print(f"quantiles: worst residual / bound {ratio:.3f} over {len(cells)} cells")
    assert np.isfinite(quant).all() and (quant[..., 0] < quant[..., 1]).all()


def test_summary_rows_are_independent_and_layouts_agree(eng):
    """A row alone equals the row in the batch bit for bit; the records layout and separately laid out (f, Q) agree bit for bit; device memory
    equals host memory; no probs: no quantiles."""
    import torch
    C, p, H = 65, 3, 3
    case = mixture_case(C, p, H, "fq")
    whole = run_summary(eng, case, C, p, H, "fq")
    f, Q = (np.ascontiguousarray(case[key]) for key in ("f", "Q"))
    sep = eng.gaussian_mixture_summary(N_ROWS, C, H, p, Q=Q, f=f, probs=PROBS)
    one = eng.gaussian_mixture_summary(1, C, H, p, Q=Q[1:], f=f[1:], probs=PROBS)
    dev = eng.gaussian_mixture_summary(N_ROWS, C, H, p, Q=torch.as_tensor(np.array(Q), device="cuda:0"), f=torch.as_tensor(np.array(f), device="cuda:0"), probs=PROBS)
    for key in ("mean", "cov", "quant"):
        assert np.array_equal(whole[key], sep[key]) and np.array_equal(whole[key][1:], one[key]) and np.array_equal(dev[key].cpu().numpy(), whole[key])
    none = eng.gaussian_mixture_summary(N_ROWS, C, H, p, Q=Q, f=f)
    assert none["quant"] is None and np.array_equal(none["cov"], whole["cov"])


def test_summary_flags_a_bad_component(eng):
    C, p, H = 64, 3, 1
    case = mixture_case(C, p, H, "stream")
    Q = np.array(case["Q"])
    Q[0, 7, 0, 1, 1] = -1.0
    out = eng.gaussian_mixture_summary(N_ROWS, C, H, p, Q=Q, probs=PROBS)
    clean = eng.gaussian_mixture_summary(N_ROWS, C, H, p, Q=np.array(case["Q"]), probs=PROBS)
    assert list(out["status"]) == [_lib.ST_NOT_PD, 0]
    cov = out["cov"].reshape(N_ROWS, H, p, p)
    assert np.isnan(out["quant"][0, 0, 1]).all() and np.isnan(out["mean"][0, 0, 1]) and np.isnan(cov[0, 0, 1]).all() and np.isnan(cov[0, 0, :, 1]).all()
    assert np.array_equal(out["quant"][0, 0, [0, 2]], clean["quant"][0, 0, [0, 2]]) and np.array_equal(cov[0, 0, 0, 0], clean["cov"].reshape(N_ROWS, H, p, p)[0, 0, 0, 0])
    for key in ("mean", "cov", "quant"):
        assert np.array_equal(out[key][1], clean[key][1])
    f = np.zeros((N_ROWS, C, H, p))
    f[1, 3, 0, 2] = np.nan
    out = eng.gaussian_mixture_summary(N_ROWS, C, H, p, Q=np.array(case["Q"]), f=f, probs=PROBS)
    assert list(out["status"]) == [0, _lib.ST_NONFINITE] and np.isnan(out["quant"][1, 0, 2]).all() and np.isfinite(out["quant"][1, 0, :2]).all()
    with pytest.raises(EngineError, match="p <= 64"):
        eng.gaussian_mixture_summary(1, 1, 1, 65, Q=np.ones(65 * 65))


def test_summary_takes_a_million_components(eng):
    """C = 2^20 equal components: the mixture IS the component, so the summary is known in closed form."""
    from scipy.stats import norm
    import torch
    C = 1 << 20
    Q = torch.full((C, 1, 1), 4.0, dtype=torch.float64, device="cuda:0")
    f = torch.full((C, 1, 1), 1.5, dtype=torch.float64, device="cuda:0")
    out = eng.gaussian_mixture_summary(1, C, 1, 1, Q=Q, f=f, probs=(0.75,))
    assert float(out["mean"][0, 0, 0]) == 1.5 and float(out["cov"][0, 0, 0]) == 4.0 and int(out["status"][0]) == 0
    assert abs(float(out["quant"][0, 0, 0, 0]) - norm.ppf(0.75, 1.5, 2.0)) <= 1e-12


# ---- drivers ------------------------------------------------------------------------------------------------------------------------------
T_TRAIN, HORIZON, PATHS = 6, 3, 64


def driver_case(kind, p, d, k, beta0=False, M=3, N=2):
    mod, ys, draws, prior = rs.toy_draws(kind, p, d, k, N=N, M=M, T=T_TRAIN, seed=p * 100 + d * 10 + k, beta0=beta0)
    extra = {}
    if kind != "fsv":
        extra = dict(train=rs.model_tables(materialise(mod, np.arange(1.0, T_TRAIN + 1))),
                     fore=rs.model_tables(materialise(mod, T_TRAIN + np.arange(1.0, HORIZON + 1))), ys=ys, m0=prior["m0"], C0=prior["C0"])
    return mod, ys, draws, prior, extra


def run_driver(eng, kind, mod, ys, draws, prior, **kw):
    if kind == "fsv":
        return FactorSv.forecast(draws, HORIZON, eng, n_paths=PATHS, prob=0.75, probs=[0.1], seed=4, series_offset=2, **kw)
    cls, name = (DlmFsv, "w") if kind == "obs" else (DlmFsvSystem, "V")
    named = {(name if key == "static" else key): a for key, a in draws.items()}
    return cls.forecast(mod, ys, named, HORIZON, eng, m0=prior["m0"], c0=prior["C0"], n_paths=PATHS, prob=0.75, probs=[0.1], seed=4, series_offset=2, **kw)


@pytest.mark.parametrize("kind,p,d,k", [("obs", 3, 2, 1), ("obs", 4, 5, 2), ("sys", 3, 2, 1), ("sys", 4, 5, 2), ("fsv", 3, 3, 2)])
def test_driver_against_the_restated_composition(eng, kind, p, d, k):
    mod, ys, draws, prior, extra = driver_case(kind, p, d, k)
    out = run_driver(eng, kind, mod, ys, draws, prior)
    mean, cov, quant, st = rs.compose(kind, draws, HORIZON, PATHS, probs=(0.25, 0.75, 0.1), seed=4, series_offset=2, **extra)
    assert not out["status"].any() and not st.any() and out["cov"].shape == (2, HORIZON, p, p)
    np.testing.assert_allclose(out["mean"], mean, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(out["cov"], cov, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(out["lower"], quant[..., 0], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(out["upper"], quant[..., 1], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(out["quantiles"][..., 0], quant[..., 2], rtol=RTOL, atol=ATOL)
    assert (out["quantiles"][..., 0] < out["lower"]).all() and (out["lower"] < out["upper"]).all()
    if kind == "fsv":
        assert not out["mean"].any()
    # worked one panel and one draw at a time under a small budget: not a number changes
    from bayesian_dlms_amd._dlmfsv import forecast_bytes
    keep, row_h, row_t = forecast_bytes(kind != "fsv", 3, PATHS, HORIZON, T_TRAIN, p, d, d if kind == "sys" else p, k)
    least = keep + PATHS * row_h + row_t if kind != "fsv" else 3 * PATHS * row_h
    small = run_driver(eng, kind, mod, ys, draws, prior, budget=least)
    with pytest.raises(MemoryError):
        run_driver(eng, kind, mod, ys, draws, prior, budget=least - 1)
    for key in ("mean", "cov", "lower", "upper", "quantiles"):
        assert np.array_equal(small[key], out[key]), key
    # a list of kept States in place of the stacked arrays
    if kind == "fsv":
        kept = [FactorSv.State({key: draws[key][m] for key in ("beta", "v", "sv")}, None, draws["alpha"][m], np.zeros(2, np.int32)) for m in range(3)]
        again = FactorSv.forecast(kept, HORIZON, eng, n_paths=PATHS, prob=0.75, probs=[0.1], seed=4, series_offset=2)
        assert np.array_equal(again["cov"], out["cov"]) and np.array_equal(again["upper"], out["upper"])


@pytest.mark.parametrize("kind,p,d,k", [("obs", 3, 2, 1), ("obs", 4, 5, 2), ("sys", 3, 2, 1), ("sys", 4, 5, 2)])
def test_zero_loadings_give_the_gaussian_forecast_of_the_dlm(eng, kind, p, d, k):
    """beta = 0 and one draw: every component is the same Gaussian, api.forecast's (f, Q) from (m_T, C_T); the component sums are divided by
    C, so mean and cov agree to rounding and the interval is the Gaussian's."""
    from scipy.stats import norm
    mod, ys, draws, prior, extra = driver_case(kind, p, d, k, beta0=True, M=1)
    out = run_driver(eng, kind, mod, ys, draws, prior)
    for n in range(2):
        S, static = np.diag(draws["v"][0, n]), np.diag(draws["static"][0, n])
        par = DlmParameters(S, static, prior["m0"], prior["C0"]) if kind == "obs" else DlmParameters(static, S, prior["m0"], prior["C0"])
        filt = np.asarray(eng.filter(materialise(mod, np.arange(1.0, T_TRAIN + 1)), par, ys[n:n + 1])["filt"])[0, T_TRAIN]
        mT, CT = filt[:d], filt[d:].reshape(d, d).T
        _, f, Q = api.forecast(mod, mT, CT, float(T_TRAIN), par, eng, HORIZON + 1)
        f, Q = f[0, 1:], Q[0, 1:]
        np.testing.assert_allclose(out["mean"][n], f, rtol=1e-13, atol=1e-14)
        np.testing.assert_allclose(out["cov"][n], Q, rtol=1e-12, atol=1e-12)
        sd = np.sqrt(np.diagonal(Q, axis1=1, axis2=2))
        np.testing.assert_allclose(out["upper"][n], f + sd * norm.ppf(0.75), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(out["lower"][n], f + sd * norm.ppf(0.25), rtol=RTOL, atol=ATOL)
