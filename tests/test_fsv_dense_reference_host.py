"""The 50-digit dense reference of the factor stochastic-volatility kernels (tests/fsv_dense_reference.py), its bounds and its case table,
checked without a GPU: the NumPy restatements (tests/fsv_restatement.py, dlmfsv_restatement.py, dlmfsvsys_restatement.py) stand in for the
kernels.  tests/test_fsv_dense_reference_gpu.py makes the same assertions on the device's outputs.

  every case, both input sets, the default and the literal mode: the restatement within the derived bound (the largest error / bound
  printed), and no asserted bound of a draw above 1e-6 of ||x*||_inf of its system (a condition on the inputs, so the test is not vacuous);
  the bounds have teeth: at the best- and the worst-conditioned case of each solve kernel two perturbed inputs exceed the bound at more
  than one system;
  the not-positive-definite status of the restatement is a rounding event: the reference factorises the same matrix in 50 digits;
  the table launches every k of every template and puts a wholly missing time on each of the four waves of the loadings kernel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dlmfsv_restatement as dr  # noqa: E402
import dlmfsvsys_restatement as sr  # noqa: E402
import fsv_dense_reference as ref  # noqa: E402
import fsv_restatement as fr  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402

SETS = [False, True]          # the well-conditioned inputs, the wide ranges
_ids = lambda c: "-".join(str(v) for v in c) if isinstance(c, tuple) else str(c)


factors_ref, impute_ref, loadings_ref = ref.factors_ref, ref.impute_ref, ref.loadings_ref


@pytest.mark.parametrize("wide", SETS)
@pytest.mark.parametrize("case", ref.SOLVE_CASES, ids=_ids)
def test_factors_restatement_within_the_bound(case, wide):
    x = ref.solve_inputs("factors", case, wide)
    for with_alpha in (True, False):
        r = factors_ref(case, wide, with_alpha)
        for literal in (False, True):
            got, st, _ = fr.factors(x["y"], x["beta"], x["v"], x["alpha"] if with_alpha else None, literal=literal, **ref.KW)
            ratio, rel = ref.ratio_factors(r, got, literal)
            print(f"factors {case} wide {wide} alpha {with_alpha} literal {literal}: error / bound {ratio:.3g}, bound / |x*| {rel:.3g}, "
                  f"largest condition number {np.nanmax(r['cond']):.3g}")
            assert not st.any() and ratio <= 1.0 and rel <= ref.REL_MAX


@pytest.mark.parametrize("wide", SETS)
@pytest.mark.parametrize("case", ref.SOLVE_CASES, ids=_ids)
def test_impute_restatement_within_the_bound(case, wide):
    x = ref.solve_inputs("impute", case, wide)
    r = impute_ref(case, wide)
    got, st, _ = dr.impute(x["y"], x["beta"], x["v"], x["alpha"], **ref.KW)
    ratio, rel = ref.ratio_impute(r, got)
    cond = np.nanmax(r["cond"]) if r["part"].any() else 0.0
    print(f"impute {case} wide {wide}: {int(r['part'].sum())} partially missing times, error / bound {ratio:.3g}, bound / |x*| {rel:.3g}, "
          f"largest condition number {cond:.3g}")
    assert not st.any() and ratio <= 1.0 and rel <= ref.REL_MAX
    assert r["part"].any() or case[1] == 1


@pytest.mark.parametrize("wide", SETS)
@pytest.mark.parametrize("index", range(len(ref.LOADINGS_CASES)), ids=[_ids(c) for c in ref.LOADINGS_CASES])
def test_loadings_restatement_within_the_bound(index, wide):
    T, p, k, N = ref.LOADINGS_CASES[index]
    x = ref.loadings_inputs(index, wide)
    for literal in (0, 1):
        r = loadings_ref(index, wide, literal)
        beta, v, st, _ = fr.loadings(x["y"], x["f"], x["beta"], x["v"], dict(x["prior"], literal=literal), **ref.KW)
        rb, rv, rel = ref.ratio_loadings(r, beta, v)
        cond = np.nanmax(r["cond"]) if p > 1 else 1.0
        print(f"loadings {(T, p, k)} wide {wide} literal {literal}: error / bound rows {rb:.3g} sigma^2 {rv:.3g}, bound / |x*| {rel:.3g}, "
              f"largest condition number {cond:.3g}")
        assert st.tolist() == [0, 0] + [_lib.ST_NONFINITE] * (N - 2) and r["empty"].tolist() == [False, False] + [True] * (N - 2)
        assert rb <= 1.0 and rv <= 1.0 and rel <= ref.REL_MAX
        if N == 3:          # the panel without a counted time keeps its inputs
            assert np.array_equal(beta[2], x["beta"][2]) and np.array_equal(v[2], x["v"][2])


@pytest.mark.parametrize("case", ref.VARIANCE_CASES, ids=_ids)
def test_variance_restatement_within_the_bound(case):
    x = ref.variance_inputs(case)
    r = ref.variance(x["beta"], x["v"], x["alpha"])
    V, st, _ = dr.variance(x["beta"], x["v"], x["alpha"])
    ratio = float((ref.error(V, r["V"], r["V_lo"]) / r["bound"]).max())
    print(f"variance {case}: error / bound {ratio:.3g}")
    assert not st.any() and ratio <= 1.0


@pytest.mark.parametrize("case", ref.CENTER_CASES, ids=_ids)
def test_center_restatement_within_the_bound(case):
    x = ref.center_inputs(case)
    r = ref.center(x["y"], x["theta"], x["F"])
    got, st, _ = dr.center(x["y"], x["theta"], x["F"])
    m = ~np.isnan(x["y"])
    assert np.array_equal(np.isnan(got), ~m) and np.array_equal(np.isnan(r["r"]), ~m)
    ratio = float((ref.error(got, r["r"], r["r_lo"])[m] / r["bound"][m]).max())
    print(f"center {case}: error / bound {ratio:.3g}")
    assert not st.any() and ratio <= 1.0


@pytest.mark.parametrize("case", ref.INNOVATION_CASES, ids=_ids)
def test_innovations_restatement_within_the_bound(case):
    x = ref.innovation_inputs(case)
    r = ref.innovations(x["theta"], x["G"])
    got, st, _ = sr.innovations(x["theta"], x["G"])
    ratio = float((ref.error(got, r["w"], r["w_lo"]) / r["bound"]).max())
    print(f"innovations {case}: error / bound {ratio:.3g}")
    assert not st.any() and ratio <= 1.0


# ---- the bounds have teeth ------------------------------------------------------------------------------------------------------------------
_zero_last_free, _through_float32, _extremes = ref.zero_last_free, ref.through_float32, ref.extremes


def _exceeding_factors(r, got, literal):
    hi, lo, bound = (r["f_lit"], r["f_lit_lo"], r["bound_lit"]) if literal else (r["f"], r["f_lo"], r["bound"])
    m = ~np.isnan(bound)
    return int((np.max(ref.error(got, hi, lo), axis=1)[m] > bound[m]).sum())


def test_the_factor_bounds_have_teeth():
    """Mutant 1: v through float32.  Mutant 2: the last row's last free loading zeroed.  Cases without a free loading (p = 1) are left out."""
    conds = {(c, w): float(np.nanmax(factors_ref(c, w, True)["cond"])) for c in ref.SOLVE_CASES if c[1] >= 2 for w in SETS}
    for case, wide in _extremes(conds):
        x, r = ref.solve_inputs("factors", case, wide), factors_ref(case, wide, True)
        for name, beta, v in (("v through float32", x["beta"], _through_float32(x["v"])), ("a loading zeroed", _zero_last_free(x["beta"]), x["v"])):
            for literal in (False, True):
                n = _exceeding_factors(r, fr.factors(x["y"], beta, v, x["alpha"], literal=literal, **ref.KW)[0], literal)
                print(f"factors {case} wide {wide} (condition number {conds[case, wide]:.3g}), {name}, literal {literal}: outside the bound at {n} times")
                assert n > 1


def test_the_impute_bounds_have_teeth():
    conds = {(c, w): float(np.nanmax(impute_ref(c, w)["cond"])) for c in ref.SOLVE_CASES if c[1] >= 2 for w in SETS}
    for case, wide in _extremes(conds):
        x, r = ref.solve_inputs("impute", case, wide), impute_ref(case, wide)
        for name, beta, v in (("v through float32", x["beta"], _through_float32(x["v"])), ("a loading zeroed", _zero_last_free(x["beta"]), x["v"])):
            got = dr.impute(x["y"], beta, v, x["alpha"], **ref.KW)[0]
            n = int(((ref.error(got, r["r"], r["r_lo"]) > r["bound"]) & (r["bound"] > 0.0)).any(axis=2).sum())
            print(f"impute {case} wide {wide} (condition number {conds[case, wide]:.3g}), {name}: outside the bound at {n} times")
            assert n > 1


def test_the_loadings_bounds_have_teeth():
    """v is no input of the loadings step (it is kept for a panel without a counted time only), so mutant 1 rounds the factors through
    float32 in its place; mutant 2 zeroes the old loading, which reaches the rows through ssy and sigma^2.  Counted: the rows outside."""
    idx = [i for i, c in enumerate(ref.LOADINGS_CASES) if c[1] >= 2]
    conds = {(i, w): float(np.nanmax(loadings_ref(i, w, 0)["cond"])) for i in idx for w in SETS}
    for index, wide in _extremes(conds):
        x = ref.loadings_inputs(index, wide)
        for name, f, beta in (("f through float32", _through_float32(x["f"]), x["beta"]), ("a loading zeroed", x["f"], _zero_last_free(x["beta"]))):
            for literal in (0, 1):
                r = loadings_ref(index, wide, literal)
                b, v, _, _ = fr.loadings(x["y"], f, beta, x["v"], dict(x["prior"], literal=literal), **ref.KW)
                live = ~r["empty"]
                n = int((ref.error(b, r["beta"], r["beta_lo"]).max(axis=2)[live] > r["bound"][live]).sum())
                sig = bool((ref.error(v[:, 0], r["v"], r["v_lo"])[live] > r["bound_v"][live]).all())
                print(f"loadings {ref.LOADINGS_CASES[index]} wide {wide} (condition number {conds[index, wide]:.3g}), {name}, literal {literal}: "
                      f"{n} rows outside the bound, sigma^2 outside {sig}")
                assert n > 1 and sig


# ---- the not-positive-definite status is a rounding event -------------------------------------------------------------------------------------
def test_not_pd_is_a_rounding_event_not_a_model_property():
    x = ref.not_pd_inputs()
    f, st, _ = fr.factors(x["y"], x["beta"], x["v"], x["alpha"], **ref.KW)
    assert st.tolist() == [_lib.ST_NOT_PD, 0]
    assert np.isnan(f[0, :, x["t"]]).all() and np.isfinite(np.delete(f[0], x["t"], axis=1)).all() and np.isfinite(f[1]).all()
    r = ref.factors(x["y"], x["beta"], x["v"], x["alpha"], **ref.KW)          # 50 digits: the same matrix is positive definite
    assert np.isfinite(r["f"]).all()
    print(f"the reference's condition number of the system that the restatement calls not positive definite: {r['cond'][0, x['t']]:.3g}")
    assert 1e31 < r["cond"][0, x["t"]] < 1e34
    part = x["part"]
    out, st, _ = dr.impute(part, x["beta"], x["v"], x["alpha"], **ref.KW)
    assert st.tolist() == [_lib.ST_NOT_PD, 0]
    assert np.array_equal(out[0], part[0], equal_nan=True) and np.isfinite(out[1]).all()
    ri = ref.impute(part, x["beta"], x["v"], x["alpha"], **ref.KW)
    assert np.isfinite(ri["r"]).all() and ri["cond"][0, x["t"]] > 1e15


# ---- the table ----------------------------------------------------------------------------------------------------------------------------
def test_the_table_launches_every_instantiation_and_every_edge():
    every = set(range(1, 9))
    assert {c[2] for c in ref.SOLVE_CASES} == every and {c[2] for c in ref.LOADINGS_CASES} == every and {c[2] for c in ref.VARIANCE_CASES} == every
    assert {c[0] for c in ref.SOLVE_CASES if c[1] == c[2]} == {2, 255, 256, 257}
    ns = lambda k: k * (k + 1) // 2
    assert all((3, k, k) in {c[:3] for c in ref.LOADINGS_CASES} for k in every)          # T = 3: wave 3 has no time; p = k < k (k + 1) / 2 from k = 2
    assert all({(ns(k) - 1, k), (ns(k), k)} <= {c[1:3] for c in ref.LOADINGS_CASES} for k in range(4, 9))
    assert {c[0] for c in ref.LOADINGS_CASES} >= {5, 6, 7, 8, 9}
    waves = set()
    for i, (T, p, k, N) in enumerate(ref.LOADINGS_CASES):
        x = ref.loadings_inputs(i, False)
        gone = np.isnan(x["y"]).all(axis=2)[:2]
        assert np.array_equal(gone, np.isnan(x["f"]).all(axis=1)[:2]) and (gone.sum(axis=1) == (1 if T >= 8 else 0)).all()
        waves |= {int(t) % 4 for t in np.nonzero(gone)[1]}
    assert waves == {0, 1, 2, 3}
    assert {(c[1] ** 2 < 256, c[1] ** 2 == 256, c[1] ** 2 > 256) for c in ref.VARIANCE_CASES} == {(True, False, False), (False, True, False), (False, False, True)}
    assert {c[0] for c in ref.VARIANCE_CASES} >= {63, 64, 65, 129}
    assert all((c[0] * c[1]) % 256 for c in ref.CENTER_CASES[1:]) and all((c[0] * c[1]) % 256 for c in ref.INNOVATION_CASES[1:])
    for kind in ("factors", "impute"):          # from T = 8 on one wholly missing time per panel
        for case in ref.SOLVE_CASES:
            gone = np.isnan(ref.solve_inputs(kind, case, True)["y"]).all(axis=2)
            assert (gone.sum(axis=1) >= 1).all() if case[0] >= 8 else kind == "impute" or not gone.any()
