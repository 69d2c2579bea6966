"""dlm_pg_batch on the GPU: particle Gibbs for a DGLM, conditional SMC with ancestor sampling (k_pg, Engine.pg_sweep, ParticleGibbs).

1  draw for draw against the NumPy restatement (tests/pg_restatement.py) on the table of tests/pg_cases.py, at the tolerance and under the
   rule of tests/test_pf_gpu.py: rtol 1e-11 / atol 1e-12 on the doubles, the ancestors and the path indices EQUAL as integers (no uniform
   of the table lands within 1e-8 of a running sum: tests/test_pg_host.py);
2  exact invariance: reference paths drawn from the exact smoothing law on a grid (tests/pg_grid_reference.py) are still draws of it after
   K = 3 sweeps -- means, variances (standard error from the exact fourth moment) and lag-one cross-moments at every t within 5 se;
3  the ancestor-sampling law read from the trace of one sweep, against scipy.stats;
4  the trace-back, the conditioning and the statistics as exact equalities;
5  Gaussian d = 2 and d = 3 against the Kalman smoother, started from Engine.ffbs draws;
6  renewal: the share of series whose path still starts in the reference particle;
7  the sampler's joint law in the manner of tests/gibbs_invariance.py;
8  the contract: splits, failures, aliasing, refusals.

Every statistical check runs first on the restatement in tests/test_pg_host.py, at the same N, K, P and seeds; the figures of both and the
mutants that each check catches are in profiles/r28_notes.md."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pf_cases as pc  # noqa: E402
import pg_cases as gc  # noqa: E402
import pg_checks as ck  # noqa: E402

from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.engine import Engine, EngineError, _Host  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-11, 1e-12
DOUBLES = ("ll", "path", "stats", "clouds", "step_weights")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _rel(a, b):
    ok = np.isfinite(b)
    return float((np.abs(a[ok] - b[ok]) / (np.abs(b[ok]) + ATOL / RTOL)).max()) if ok.any() else 0.0


# ---- 1: kernel against restatement ----------------------------------------------------------------------------------------------------------
RUNS = [(c["name"], False) for c in gc.TABLE] + [(n, True) for n in ("d2-p128-missing-per-series", "d16-p128-irregular-per-series")]


@pytest.mark.parametrize("name,device", RUNS, ids=[n + ("-device" if dev else "") for n, dev in RUNS])
def test_kernel_matches_restatement(eng, name, device):
    ref = gc.reference(name)
    out = gc.engine_run(eng, gc.run_args(name), device=device)
    assert eng.last_variant == "pg-wave"
    np.testing.assert_array_equal(out["status"], ref["status"])
    assert np.all(ref["status"] == 0)
    np.testing.assert_array_equal(out["ancestors"], ref["ancestors"])
    np.testing.assert_array_equal(out["path_index"], ref["path_index"])
    print(f"{name}: largest relative difference " + ", ".join(f"{k} {_rel(out[k], ref[k]):.2e}" for k in DOUBLES))
    for k in DOUBLES:
        np.testing.assert_allclose(out[k], ref[k], rtol=RTOL, atol=ATOL, err_msg=k)


# ---- 4: trace-back and conditioning, exact equalities -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d3-p128-irregular", "plain-d2-irregular", "family-gaussian", "d2-p128-missing-per-series"])
def test_trace_back_conditioning_and_statistics_are_exact(eng, name):
    kw = gc.run_args(name)
    ck.hold_trace(kw, gc.engine_run(eng, kw))


# ---- 2, 3, 6: the laws, on the cases of the exact grid smoother -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ck.INVARIANCE_NAMES)
def test_sweeps_leave_the_grid_smoothing_law_invariant(eng, name):
    kw = ck.invariance_args(name)
    path = kw["ref"]
    for k in range(ck.K):
        out = gc.engine_run(eng, dict(kw, ref=path, iteration=k), device=True, traces=False)
        assert np.all(out["status"] == 0)
        path = out["path"]
    ck.hold_invariance(name, path)


@pytest.mark.parametrize("name", ck.ANCESTOR_NAMES)
def test_the_reference_s_ancestor_follows_its_law(eng, name):
    kw = ck.invariance_args(name)
    ck.hold_ancestor_law(kw, gc.engine_run(eng, kw, device=True))


@pytest.mark.parametrize("name", ck.INVARIANCE_NAMES)
def test_one_sweep_renews_the_path(eng, name):
    kw = ck.invariance_args(name)
    share = {}
    for on in (True, False):
        out = gc.engine_run(eng, dict(kw, ancestor_sampling=on), device=True, traces=False, want_path_index=True)
        assert np.all(out["status"] == 0)
        share[on] = ck.kept_share(out["path_index"], kw["P"])
    ck.hold_renewal(name, share[True], share[False])


# ---- 5: Gaussian d = 2 and d = 3 against the Kalman smoother ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ck.GAUSSIAN_NAMES)
def test_gaussian_paths_keep_the_kalman_smoother_s_moments(eng, which):
    case = ck.gaussian_case(which)
    start = eng.ffbs(case["mat"], case["params"], case["y3"], seed=ck.SEED, want_theta=True, want_stats=False, want_filt=False)
    path = np.asarray(start["theta"])
    assert np.all(np.asarray(start["status"]) == 0)
    ck.hold_gaussian(which, path, "Engine.ffbs itself")          # the start IS a sample of the law: the yardstick sees it as one
    kw = case["kw"]
    for k in range(ck.K):
        out = gc.engine_run(eng, dict(kw, ref=path, iteration=k), device=True, traces=False)
        assert np.all(out["status"] == 0)
        path = out["path"]
    ck.hold_gaussian(which, path, f"after {ck.K} sweeps")


# ---- 7: the sampler's joint law -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ck.JOINT_NAMES)
def test_the_sampler_leaves_the_joint_law_invariant(eng, which):
    ck.hold_joint(which, ck.run_joint_engine(which, eng))


# ---- 8: the contract ------------------------------------------------------------------------------------------------------------------------
KEYS = ("ll", "path", "stats", "path_index", "status")


def _slice(kw, lo, hi):
    cut = dict(kw, y=kw["y"][lo:hi], ref=kw["ref"][lo:hi], series_offset=kw["series_offset"] + lo)
    for k in ("V", "W", "m0", "C0"):
        cut[k] = kw[k][lo:hi]
    return cut


def test_results_do_not_depend_on_how_the_batch_is_split(eng):
    kw = gc.run_args("d2-p128-missing-per-series")
    N, T, d, P = 5, 12, 2, 128
    whole = gc.engine_run(eng, kw)
    lo, hi = gc.engine_run(eng, _slice(kw, 0, 3)), gc.engine_run(eng, _slice(kw, 3, 5), device=True)
    per_series = (T + 1) * d * P * 8 + T * P * 4
    capped = gc.engine_run(eng, kw, traces=False, want_path_index=True, workspace_cap=2 * per_series)          # three launches: 2 + 2 + 1 series
    one = gc.engine_run(eng, kw, traces=False, want_path_index=True, workspace_cap=1)                          # a cap below one series: five launches
    uncapped = gc.engine_run(eng, kw, traces=False, want_path_index=True)
    for k in KEYS:
        np.testing.assert_array_equal(whole[k], np.concatenate([lo[k], hi[k]]), err_msg=k)
        for other in (capped, one, uncapped):
            np.testing.assert_array_equal(whole[k], other[k], err_msg=k)
    for k in ("clouds", "ancestors", "step_weights"):
        np.testing.assert_array_equal(whole[k], np.concatenate([lo[k], hi[k]]), err_msg=k)
    again = gc.engine_run(eng, dict(kw, iteration=kw["iteration"] + 1))
    assert np.all(again["ll"] != whole["ll"])          # another iteration: other draws for every series


def test_a_failing_series_fails_alone(eng):
    kw = gc.run_args("d2-p128-missing-per-series")
    good = gc.engine_run(eng, kw)
    W = kw["W"].copy(); W[1] = np.array([[1.0, 2.0], [2.0, 1.0]])
    C0 = kw["C0"].copy(); C0[3] = -C0[3]
    ref = kw["ref"].copy(); ref[2, 6, 1] = np.nan
    out = gc.engine_run(eng, dict(kw, W=W, C0=C0, ref=ref))
    assert out["status"].tolist() == [0, _lib.ST_NOT_PD, _lib.ST_NONFINITE, _lib.ST_NOT_PD, 0]
    bad = [1, 2, 3]
    assert np.all(out["ll"][bad] == -np.inf) and np.all(np.isnan(out["path"][bad])) and np.all(np.isnan(out["stats"][bad]))
    for k in KEYS + ("clouds", "ancestors", "step_weights"):
        np.testing.assert_array_equal(out[k][[0, 4]], good[k][[0, 4]], err_msg=k)
    np.testing.assert_array_equal(out["clouds"][2, :6], good["clouds"][2, :6])          # what the series had written before it met the NaN


def test_a_reference_entry_behind_a_step_that_does_not_advance_is_not_read(eng):
    kw = gc.run_args("d3-p128-irregular")
    t0 = int(np.nonzero(kw["dt"][1:] == 0.0)[0][0]) + 1
    ref = kw["ref"].copy(); ref[:, t0 + 1] = np.nan; ref[:, 1] = np.nan          # dt_0 = 0 and dt_t0 = 0
    good, out = gc.engine_run(eng, kw), gc.engine_run(eng, dict(kw, ref=ref))
    assert np.all(out["status"] == 0)
    for k in KEYS + ("clouds", "ancestors", "step_weights"):
        np.testing.assert_array_equal(out[k], good[k], err_msg=k)


def test_path_may_be_the_reference_array(eng):
    import torch
    kw = gc.run_args("d3-p128-irregular")
    good = gc.engine_run(eng, kw, device=True, traces=False)
    N = kw["y"].shape[0]
    ref = torch.as_tensor(kw["ref"].copy(), device="cuda")
    out = eng.pg_sweep(pc.materialised(kw), pc.packed_params(kw, N), torch.as_tensor(kw["y"], device="cuda"), ref, family=kw["family"],
                       n_particles=kw["P"], obs_param=kw.get("nu"), iteration=kw["iteration"], seed=kw["seed"], series_offset=kw["series_offset"],
                       in_place=True)
    assert out["path"].data_ptr() == ref.data_ptr()
    np.testing.assert_array_equal(ref.cpu().numpy(), good["path"])
    np.testing.assert_array_equal(out["stats"].cpu().numpy(), good["stats"])


def test_engine_refuses_what_it_does_not_cover(eng):
    kw = gc.run_args("d1-p64")
    mat, par = pc.materialised(kw), pc.packed_params(kw, 5)
    for P in (96, 2048):
        with pytest.raises(EngineError, match="multiple of 64"):
            eng.pg_sweep(mat, par, kw["y"], kw["ref"], family=0, n_particles=P)
    with pytest.raises(EngineError, match="ref must be"):
        eng.pg_sweep(mat, par, kw["y"], kw["ref"][:, :-1], family=0, n_particles=64)
    # straight at the C ABI: the documented codes, each with a message, no launch
    y, ref = np.ascontiguousarray(kw["y"]), np.ascontiguousarray(kw["ref"])
    ll, path, stats = np.empty(5), np.empty_like(ref), np.empty((5, 4))
    p = _Host.ptr

    def call(desc, d=1, pp=1, refp=ref, clouds=None):
        md, pd, op, keep = eng.prepare(mat, par, 5, _Host())
        md.d, md.p = d, pp
        return eng.lib.dlm_pg_batch(eng.h, md, pd, ctypes.byref(desc), None, p(y), p(refp), 0, op, p(ll), p(path), p(stats), None, p(clouds), None,
                                    None, None)
    err = lambda: eng.lib.dlm_last_error(eng.h)
    assert call(_lib.PgDesc(0, 64, 1, 0), d=17) == -3 and b"d <= 16" in err()          # DLM_ERR_UNSUPPORTED
    assert call(_lib.PgDesc(0, 96, 1, 0)) == -3 and b"multiple of 64" in err()
    assert call(_lib.PgDesc(0, 64, 1, 0), pp=2) == -3 and b"p = 1" in err()
    assert call(_lib.PgDesc(0, 64, 2, 0)) == -1 and b"ancestor_sampling" in err()          # DLM_ERR_ARG
    assert call(_lib.PgDesc(0, 64, 1, -5)) == -1 and b"workspace_cap" in err()
    assert call(_lib.PgDesc(0, 64, 1, 0), refp=None) == -1 and b"ref" in err()
    assert call(_lib.PgDesc(0, 64, 1, 0), clouds=np.empty((5, 13, 1, 64))) == -1 and b"together" in err()
    assert call(_lib.PgDesc(6, 64, 1, 0)) == -1 and b"family" in err()
    assert call(_lib.PgDesc(0, 64, 1, 0)) == 0 and np.all(np.isfinite(ll))          # and the same call inside the limits runs
