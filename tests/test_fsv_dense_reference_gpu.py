"""The factor stochastic-volatility kernels on the GPU against the 50-digit dense reference (tests/fsv_dense_reference.py): the assertions
of tests/test_fsv_dense_reference_host.py with the engine's outputs in place of the restatements'.  Every k = 1..8 of k_fsv_factors,
k_fsv_loadings, k_dlmfsv_impute and k_dlmfsv_variance is launched, and k_dlmfsv_center and k_dlmfsvsys_innovations, at the layout edges
of the table there; the solve kernels run on the well-conditioned inputs and on the wide ranges (condition numbers up to 1e6 to 1e7).
The bounds are derived in the reference's docstring, not measured; the largest error / bound seen on an MI355X is in
profiles/r18_notes.md.  One call per kernel takes host arrays and must give the device call's bits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fsv_dense_reference as ref  # noqa: E402
import fsv_restatement as fr  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dlm import MaterialisedModel  # noqa: E402
from bayesian_dlms_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu
SETS = [False, True]          # the well-conditioned inputs, the wide ranges
KW = dict(iteration=ref.ITER, seed=ref.SEED, series_offset=ref.OFFSET)
_ids = lambda c: "-".join(str(v) for v in c) if isinstance(c, tuple) else str(c)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _dev(a):
    import torch
    return None if a is None else torch.as_tensor(np.array(a), device="cuda:0")          # (a copy: the shared inputs are read-only)


def _mat(T, F=None, G=None):
    """A materialised model that carries F [T][d][p] (a table) or [d][p] for the centring call, or G [d][d] for the innovations call."""
    if F is None:
        d, p, flat, stride = G.shape[-1], 1, np.zeros(G.shape[-1]), 0
    else:
        d, p = F.shape[-2:]
        flat = np.concatenate([np.ascontiguousarray(Ft.T).reshape(-1) for Ft in (F if F.ndim == 3 else F[None])])
        stride = d * p if F.ndim == 3 else 0
    Gf = np.eye(d).reshape(-1) if G is None else np.ascontiguousarray(G.T).reshape(-1)
    return MaterialisedModel(d=d, p=p, T=T, F=flat, f_stride=stride, G=Gf, n_g=1, g_index=None, dt=None, times=np.arange(1, T + 1, dtype=np.float64))


@pytest.mark.parametrize("wide", SETS)
@pytest.mark.parametrize("case", ref.SOLVE_CASES, ids=_ids)
def test_factors_within_the_bound(eng, case, wide):
    x = ref.solve_inputs("factors", case, wide)
    for with_alpha in (True, False):
        r = ref.factors_ref(case, wide, with_alpha)
        alpha = x["alpha"] if with_alpha else None
        for literal in (False, True):
            out = eng.fsv_factors(_dev(x["y"]), _dev(x["beta"]), _dev(x["v"]), _dev(alpha), literal=literal, **KW)
            assert eng.last_variant == "fsv-factors"
            got = out["f"].cpu().numpy()
            ratio, rel = ref.ratio_factors(r, got, literal)
            print(f"factors {case} wide {wide} alpha {with_alpha} literal {literal}: error / bound {ratio:.3g}, bound / |x*| {rel:.3g}, "
                  f"largest condition number {np.nanmax(r['cond']):.3g}")
            assert not out["status"].cpu().numpy().any() and ratio <= 1.0 and rel <= ref.REL_MAX
            if case == ref.SOLVE_CASES[-1]:          # host arrays: the same bits
                host = eng.fsv_factors(x["y"], x["beta"], x["v"], alpha, literal=literal, **KW)
                assert np.array_equal(host["f"], got, equal_nan=True) and not host["status"].any()


@pytest.mark.parametrize("wide", SETS)
@pytest.mark.parametrize("case", ref.SOLVE_CASES, ids=_ids)
def test_impute_within_the_bound(eng, case, wide):
    x = ref.solve_inputs("impute", case, wide)
    r = ref.impute_ref(case, wide)
    out = eng.dlmfsv_impute(_dev(x["y"]), _dev(x["beta"]), _dev(x["v"]), _dev(x["alpha"]), **KW)
    assert eng.last_variant == "dlmfsv-impute"
    got = out["r"].cpu().numpy()
    ratio, rel = ref.ratio_impute(r, got)
    cond = np.nanmax(r["cond"]) if r["part"].any() else 0.0
    print(f"impute {case} wide {wide}: {int(r['part'].sum())} partially missing times, error / bound {ratio:.3g}, bound / |x*| {rel:.3g}, "
          f"largest condition number {cond:.3g}")
    assert not out["status"].cpu().numpy().any() and ratio <= 1.0 and rel <= ref.REL_MAX
    if case == ref.SOLVE_CASES[-1]:
        host = eng.dlmfsv_impute(x["y"], x["beta"], x["v"], x["alpha"], **KW)
        assert np.array_equal(host["r"], got, equal_nan=True) and not host["status"].any()


@pytest.mark.parametrize("wide", SETS)
@pytest.mark.parametrize("index", range(len(ref.LOADINGS_CASES)), ids=[_ids(c) for c in ref.LOADINGS_CASES])
def test_loadings_within_the_bound(eng, index, wide):
    T, p, k, N = ref.LOADINGS_CASES[index]
    x = ref.loadings_inputs(index, wide)
    for literal in (0, 1):
        r = ref.loadings_ref(index, wide, literal)
        pr = fr.fsv_prior_tuple(dict(x["prior"], literal=literal))
        out = eng.fsv_loadings(_dev(x["y"]), _dev(x["f"]), _dev(x["beta"]), pr, v=_dev(x["v"]), **KW)
        assert eng.last_variant == "fsv-loadings"
        beta, v, st = out["beta"].cpu().numpy(), out["v"].cpu().numpy(), out["status"].cpu().numpy()
        rb, rv, rel = ref.ratio_loadings(r, beta, v)
        cond = np.nanmax(r["cond"]) if p > 1 else 1.0
        print(f"loadings {(T, p, k)} wide {wide} literal {literal}: error / bound rows {rb:.3g} sigma^2 {rv:.3g}, bound / |x*| {rel:.3g}, "
              f"largest condition number {cond:.3g}")
        assert st.tolist() == [0, 0] + [_lib.ST_NONFINITE] * (N - 2)
        assert rb <= 1.0 and rv <= 1.0 and rel <= ref.REL_MAX
        if N == 3:          # the panel without a counted time keeps its inputs
            assert np.array_equal(beta[2], x["beta"][2]) and np.array_equal(v[2], x["v"][2])
        if index == len(ref.LOADINGS_CASES) - 1:
            host = eng.fsv_loadings(x["y"], x["f"], x["beta"], pr, v=x["v"], **KW)
            assert np.array_equal(host["beta"], beta) and np.array_equal(host["v"], v) and not host["status"].any()


@pytest.mark.parametrize("case", ref.VARIANCE_CASES, ids=_ids)
def test_variance_within_the_bound(eng, case):
    T, p, k = case
    x = ref.variance_inputs(case)
    r = ref.variance(x["beta"], x["v"], x["alpha"])
    out = eng.dlmfsv_variance(_dev(x["beta"]), _dev(x["v"]), _dev(x["alpha"]))
    assert eng.last_variant == "dlmfsv-variance"
    got = out["V"].cpu().numpy().reshape(2, T, p, p)
    ratio = float((ref.error(got, r["V"], r["V_lo"]) / r["bound"]).max())
    print(f"variance {case}: error / bound {ratio:.3g}")
    assert not out["status"].cpu().numpy().any() and ratio <= 1.0
    assert np.array_equal(got, np.swapaxes(got, 2, 3))          # symmetric bit for bit
    if case == ref.VARIANCE_CASES[-1]:
        host = eng.dlmfsv_variance(x["beta"], x["v"], x["alpha"])
        assert np.array_equal(host["V"].reshape(2, T, p, p), got) and not host["status"].any()


@pytest.mark.parametrize("case", ref.CENTER_CASES, ids=_ids)
def test_center_within_the_bound(eng, case):
    T = case[0]
    x = ref.center_inputs(case)
    r = ref.center(x["y"], x["theta"], x["F"])
    mat = _mat(T, F=x["F"])
    out = eng.dlmfsv_center(mat, _dev(x["y"]), _dev(x["theta"]))
    assert eng.last_variant == "dlmfsv-center"
    got = out["r"].cpu().numpy()
    m = ~np.isnan(x["y"])
    assert np.array_equal(np.isnan(got), ~m)
    ratio = float((ref.error(got, r["r"], r["r_lo"])[m] / r["bound"][m]).max())
    print(f"center {case}: error / bound {ratio:.3g}")
    assert not out["status"].cpu().numpy().any() and ratio <= 1.0
    if case == ref.CENTER_CASES[-1]:
        host = eng.dlmfsv_center(mat, x["y"], x["theta"])
        assert np.array_equal(host["r"], got, equal_nan=True) and not host["status"].any()


@pytest.mark.parametrize("case", ref.INNOVATION_CASES, ids=_ids)
def test_innovations_within_the_bound(eng, case):
    T = case[0]
    x = ref.innovation_inputs(case)
    r = ref.innovations(x["theta"], x["G"])
    mat = _mat(T, G=x["G"])
    out = eng.dlmfsvsys_innovations(mat, _dev(x["theta"]))
    assert eng.last_variant == "dlmfsvsys-innovations"
    got = out["w"].cpu().numpy()
    ratio = float((ref.error(got, r["w"], r["w_lo"]) / r["bound"]).max())
    print(f"innovations {case}: error / bound {ratio:.3g}")
    assert not out["status"].cpu().numpy().any() and ratio <= 1.0
    if case == ref.INNOVATION_CASES[-1]:
        host = eng.dlmfsvsys_innovations(mat, x["theta"])
        assert np.array_equal(host["w"], got) and not host["status"].any()


# ---- the bounds have teeth on the device too: the engine is given the perturbed inputs, the reference keeps the true ones ---------------------
def test_the_factor_bounds_have_teeth(eng):
    conds = {(c, w): float(np.nanmax(ref.factors_ref(c, w, True)["cond"])) for c in ref.SOLVE_CASES if c[1] >= 2 for w in SETS}
    for case, wide in ref.extremes(conds):
        x, r = ref.solve_inputs("factors", case, wide), ref.factors_ref(case, wide, True)
        for name, beta, v in (("v through float32", x["beta"], ref.through_float32(x["v"])), ("a loading zeroed", ref.zero_last_free(x["beta"]), x["v"])):
            for literal in (False, True):
                got = eng.fsv_factors(x["y"], beta, v, x["alpha"], literal=literal, **KW)["f"]
                hi, lo, bound = (r["f_lit"], r["f_lit_lo"], r["bound_lit"]) if literal else (r["f"], r["f_lo"], r["bound"])
                m = ~np.isnan(bound)
                n = int((np.max(ref.error(got, hi, lo), axis=1)[m] > bound[m]).sum())
                print(f"factors {case} wide {wide} (condition number {conds[case, wide]:.3g}), {name}, literal {literal}: outside the bound at {n} times")
                assert n > 1


def test_the_impute_bounds_have_teeth(eng):
    conds = {(c, w): float(np.nanmax(ref.impute_ref(c, w)["cond"])) for c in ref.SOLVE_CASES if c[1] >= 2 for w in SETS}
    for case, wide in ref.extremes(conds):
        x, r = ref.solve_inputs("impute", case, wide), ref.impute_ref(case, wide)
        for name, beta, v in (("v through float32", x["beta"], ref.through_float32(x["v"])), ("a loading zeroed", ref.zero_last_free(x["beta"]), x["v"])):
            got = eng.dlmfsv_impute(x["y"], beta, v, x["alpha"], **KW)["r"]
            n = int(((ref.error(got, r["r"], r["r_lo"]) > r["bound"]) & (r["bound"] > 0.0)).any(axis=2).sum())
            print(f"impute {case} wide {wide} (condition number {conds[case, wide]:.3g}), {name}: outside the bound at {n} times")
            assert n > 1


def test_the_loadings_bounds_have_teeth(eng):
    """As on the host: v is no input of the loadings step, so the first perturbation rounds the factors through float32 in its place."""
    idx = [i for i, c in enumerate(ref.LOADINGS_CASES) if c[1] >= 2]
    conds = {(i, w): float(np.nanmax(ref.loadings_ref(i, w, 0)["cond"])) for i in idx for w in SETS}
    for index, wide in ref.extremes(conds):
        x = ref.loadings_inputs(index, wide)
        for name, f, beta in (("f through float32", ref.through_float32(x["f"]), x["beta"]), ("a loading zeroed", x["f"], ref.zero_last_free(x["beta"]))):
            for literal in (0, 1):
                r = ref.loadings_ref(index, wide, literal)
                out = eng.fsv_loadings(x["y"], f, beta, fr.fsv_prior_tuple(dict(x["prior"], literal=literal)), v=x["v"], **KW)
                live = ~r["empty"]
                n = int((ref.error(out["beta"], r["beta"], r["beta_lo"]).max(axis=2)[live] > r["bound"][live]).sum())
                sig = bool((ref.error(out["v"][:, 0], r["v"], r["v_lo"])[live] > r["bound_v"][live]).all())
                print(f"loadings {ref.LOADINGS_CASES[index]} wide {wide} (condition number {conds[index, wide]:.3g}), {name}, literal {literal}: "
                      f"{n} rows outside the bound, sigma^2 outside {sig}")
                assert n > 1 and sig
