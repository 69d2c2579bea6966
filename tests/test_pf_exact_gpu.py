"""k_pf, k_storvik and k_lw on the GPU against the exact grid filter of tests/pf_grid_reference.py, in every observation family.

tests/test_pf_gpu.py, test_storvik_gpu.py and test_lw_gpu.py hold the kernels draw for draw to restatements written from them, and
statistically to the Kalman filter on a regular Gaussian model.  Here the reference is the forward recursion of the state's DENSITY on a
grid of x with scipy.stats' densities: no particles, no restatement, nothing the kernels produced.  It sees what kernel and restatement can
share: F_t, G through g_index and sqrt(dt_t) paired with the wrong step, a dt = 0 advanced, a per-series stride, a density paired with the
wrong V -- for Poisson, negative binomial, zero-inflated Poisson, Student-t and Beta as for the Gaussian family.

Every test is one launch of 4096 series (256 for the means) at d = 1, T = 12: the same inputs, seeds, P and replicate counts as
tests/test_pf_exact_host.py, held to the same numbers with the same bounds (pf_grid_reference.hold_likelihood, hold_means), which that file
derives and rehearses on the restatements: unbiased within 5 standard errors (Storvik: 4), the largest ratio below 2 % of the sum, the
resampled share read from ess < n0, the filtering means within twice the restatement's measured deviation plus 5 standard errors.

The figures measured on an MI355X are in profiles/r24_notes.md."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pf_cases as pc  # noqa: E402
import pf_grid_reference as gr  # noqa: E402

from bayesian_dlms_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu
VARIANT = {"particle_filter": "pf-wave", "storvik_filter": "storvik-wave", "lw_filter": "lw-wave"}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _run(eng, kind, name, means=False):
    method = gr.KINDS[kind]
    out = pc.engine_run(eng, gr.args_of(kind, name, means), method, device=True)
    assert eng.last_variant == VARIANT[method]
    return out


@pytest.mark.parametrize("name", gr.NAMES)
@pytest.mark.parametrize("kind", ["pf", "aux"])
def test_likelihood_estimate_is_unbiased_for_the_grid_likelihood(eng, kind, name):
    """particle_filter, and lw_filter with a = 1 and every prior sd 0 (the auxiliary particle filter with known parameters)"""
    gr.hold_likelihood(kind, name, _run(eng, kind, name))


@pytest.mark.parametrize("name", gr.LEARNER_NAMES)
@pytest.mark.parametrize("kind", ["storvik", "static"])
def test_learners_evidence_is_unbiased_for_the_grid_evidence(eng, kind, name):
    """storvik_filter with W ~ InverseGamma, and lw_filter as a static cloud (a = 1, prior sd 0.5) with log W ~ N: learn_v = 0, the
    non-Gaussian branch of both"""
    gr.hold_likelihood(kind, name, _run(eng, kind, name))


@pytest.mark.parametrize("name", gr.NAMES)
@pytest.mark.parametrize("kind", ["pf", "aux"])
def test_filtering_means_are_the_grid_filter_s(eng, kind, name):
    gr.hold_means(kind, name, _run(eng, kind, name, True))


def test_liu_west_second_stage_takes_both_branches_over_all_its_runs(eng):
    gr.hold_pooled_share(lambda kind, name: _run(eng, kind, name))


def test_per_series_v_is_read_from_its_own_series(eng):
    """The control of the per-series case on the device: with V handed over reversed across the batch the same check misses (the host file
    measures by how much on the restatement), so the pass above does see the stride.  Series n carries parameter set n mod 4: neighbours
    never share a set, so a read that is off by one series is another set's too."""
    name = "per-series-studentt"
    out = pc.engine_run(eng, gr.mutant(gr.args_of("pf", name), "v-reversed"), device=True)
    assert eng.last_variant == VARIANT["particle_filter"] and np.all(out["status"] == 0)
    miss = [abs(m - 1.0) / se for m, se, _ in (gr.ratio_stats(out["ll"][sl], ll) for sl, ll in zip(gr.quarters(name, gr.REPLICATES), gr.exact_lls("pf", name)))]
    print("V reversed: " + ", ".join(f"{z:.1f}" for z in miss) + " standard errors from 1")
    assert max(miss) > gr.SIGMAS
