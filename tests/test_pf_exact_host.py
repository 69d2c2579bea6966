"""The rehearsal of tests/test_pf_exact_gpu.py without a GPU: the exact grid filter of tests/pf_grid_reference.py against itself (does it
converge?) and the three RESTATEMENTS against it (is a pass on these cases worth anything?).  What holds here gives the GPU file its meaning;
every figure below was measured here, on the restatements, and is asserted, not only printed.

Grid convergence.  Halving the state spacing (M -> 2 M - 1) moves ll by <= 1e-6 and every filtered mean by <= 1e-6 posterior standard
deviations: at M = 601 the nine cases measure <= 3.0e-12 and <= 1.7e-10 (M = 401 misses with 1.6e-6 on per-series-studentt and, at
pf_cases' level, 2.7e-6 on irregular-zip; 301 with 1.3e-4 and 1.4e-3).  The learners' evidences (M = 301, 52 points of log W at a spacing of
0.25 over [-8, 4.75], about 2 s a case): halving the state spacing moves log Z by <= 1.5e-7, halving the log W spacing by <= 9.1e-8, the
integrands at the edges are <= 1.4e-32 of their peaks (asserted at 1e-6 and 1e-30; M = 201 moves log Z by 2.4e-5, a spacing of 0.5 by 4e-6).
These are three orders and more below the estimates' standard errors of 4e-3 .. 4e-2.

Unbiasedness.  |mean exp(ll_hat - ll_exact) - 1| <= 5 standard errors of the sample (4096 replicates; each quarter of a per-series case by
itself), the bound of tests/test_pf_host.py; the Storvik runs within its own file's 4.  Measured on the restatements, in standard errors:
bootstrap -1.0 .. +2.3 over the 15 (case, quarter) pairs, auxiliary -1.2 .. +2.1, Storvik -1.4 .. +0.8, static cloud -1.5 .. +0.5;
profiles/r24_notes.md has the table.

What keeps a pass from being luck.  (a) The largest single exp(ll_hat - ll_exact) is below 2 % of the sum: the standard error is not a heavy
tail's.  The auxiliary filter FAILS this at pf_cases' levels for the counts and V for Beta (up to 23 % of the sum in ONE of 4096 replicates),
which is why six cases leave those values: pf_grid_reference.CASES.  (b) The share of observed steps with ESS < n0 lies in (0.05, 0.95) for
every run of the bootstrap and the Storvik filter (0.091 .. 0.627 measured) and for the Liu-West runs that can reach it (0.055 .. 0.616): both
branches of the resampling test are taken.  The Liu-West ESS is the SECOND stage's, behind a first stage that resamples at every observed
step by construction: the better the look-ahead the evener those weights, exactly even at dt_t = 0.  Nine named (kind, case, quarter)
triples -- the counts at the levels (a) allows, one Student-t quarter -- measure 0.000 .. 0.042 and are exempt from the LOWER end alone
(pf_grid_reference.SHARE_BELOW, each with its share).  Their ess output is held otherwise: in every run ess is a finite integer in [1, P]; in
every Liu-West run it is P exactly at the dt = 0 steps and below P at every other observed step; and pooled over all twelve Liu-West runs the
share is inside (0.05, 0.95) (0.101 measured).

Mutants.  One mistake each, in the INPUTS handed to the bootstrap restatement (never in the engine): the same check must miss by more than
5 standard errors.  Measured: MUTANT_MEASURED below (7.9 .. 187).

Filtering means.  The weighted mean is a ratio estimator with a bias ~ 1 / ESS, so: P = 1024, 256 replicates, the average
of the replicates' means at each t against the grid's in units of the grid's posterior standard deviation; the bound is twice the
restatement's own largest deviation (pf_grid_reference.MEANS_MEASURED, measured here) plus 5 standard errors of the average.  The two
"one step late" mutants must exceed it (7.9 and 5.6 times the bound measured)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lw_restatement as lr  # noqa: E402
import pf_grid_reference as gr  # noqa: E402
import pf_restatement as pr  # noqa: E402
import storvik_restatement as sr  # noqa: E402

RESTATEMENT = {"pf": pr.run, "aux": lr.run, "storvik": sr.run, "static": lr.run}


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(kind, name, means=False):
        key = (kind, name, means)
        if key not in cache:
            cache[key] = RESTATEMENT[kind](**gr.args_of(kind, name, means))
        return cache[key]
    return get


# ---- the reference against itself -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gr.NAMES)
def test_state_grid_has_converged(name):
    coarse, fine = gr.exact(name), gr.exact(name, 2 * gr.M_STATE - 1)
    dll = max(abs(a[0] - b[0]) for a, b in zip(coarse, fine))
    dmean = max(float(np.abs((a[1] - b[1]) / b[2]).max()) for a, b in zip(coarse, fine))
    print(f"{name}: halving the state spacing moves ll by {dll:.1e}, the means by {dmean:.1e} posterior sd")
    assert dll <= 1e-6 and dmean <= 1e-6
    assert all(np.isfinite(a[0]) and np.all(np.isfinite(a[1])) and np.all(a[2] > 0.0) for a in coarse)


def test_beta_clamp_cannot_matter():
    """The largest filtering mass over the steps where Q41 gives the weight 0 -- beyond |eta| = 5, in a run WITHOUT that clamp, and where a
    Beta parameter is not positive (|eta| > 4.6 at the case's V = 0.01) -- and what the clamp does to ll: below 1e-12 all three.
    Measured: 4.7e-16 beyond the clamp, 8.5e-14 where no density exists, ll moved by 0.  (V = 0.02 gives 2.5e-9, 0.012 8.8e-13.)"""
    (s,) = gr.parameter_sets("irregular-beta")
    ll_free, (beyond_clamp, no_density) = gr.beta_mass_beyond(gr.F_T, gr.G_VALUES[gr.G_INDEX], gr.DT, s["V"], s["W"], s["m0"], s["C0"], s["y"])
    moved = abs(ll_free - gr.exact("irregular-beta")[0][0])
    print(f"irregular-beta: mass beyond the clamp {beyond_clamp:.1e}, where no density exists {no_density:.1e}; the clamp moves ll by {moved:.1e}")
    assert beyond_clamp < 1e-12 and no_density < 1e-12 and moved < 1e-12


@pytest.mark.parametrize("name", gr.LEARNER_NAMES)
def test_learners_references_have_converged(name):
    for exact in (gr.storvik_exact, gr.static_exact):
        z, edge = exact(name)
        z_state, _ = exact(name, gr.LOG_W_POINTS, 2 * gr.M_LEARNER - 1)
        z_logw, _ = exact(name, 2 * gr.LOG_W_POINTS - 1)
        print(f"{name} {exact.__name__}: log Z {z:.6f}; halving the state spacing moves it by {abs(z - z_state):.1e}, the log W spacing by "
              f"{abs(z - z_logw):.1e}; edge {edge:.1e} of the peak")
        assert abs(z - z_state) <= 1e-6 and abs(z - z_logw) <= 1e-6
        assert edge < 1e-30


# ---- the restatements against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gr.NAMES)
@pytest.mark.parametrize("kind", ["pf", "aux"])
def test_likelihood_estimate_is_unbiased_for_the_grid_likelihood(runs, kind, name):
    gr.hold_likelihood(kind, name, runs(kind, name))


@pytest.mark.parametrize("name", gr.LEARNER_NAMES)
@pytest.mark.parametrize("kind", ["storvik", "static"])
def test_learners_evidence_is_unbiased_for_the_grid_evidence(runs, kind, name):
    gr.hold_likelihood(kind, name, runs(kind, name))


def test_liu_west_second_stage_takes_both_branches_over_all_its_runs(runs):
    gr.hold_pooled_share(runs)


# the distance from 1 in standard errors, measured on the bootstrap restatement
MUTANT_MEASURED = {"noise-without-dt": 28.8, "f-one-step-late": 30.8, "g-index-one-step-late": 46.5, "inner-dt0-advanced": 7.9,
                   "v-reversed": (20.1, 28.2, 187.1, 19.9)}          # (per quarter; the largest is what is asserted)


@pytest.mark.parametrize("which", gr.MUTANTS + ("v-reversed",))
def test_the_same_check_fails_with_one_mistake_in_the_inputs(which):
    name = "per-series-studentt" if which == "v-reversed" else "irregular-poisson"
    kw = gr.args_of("pf", name)
    r = pr.run(**gr.mutant(kw, which))
    worst = 0.0
    for sl, (ll, _, _) in zip(gr.quarters(name, gr.REPLICATES), gr.exact(name)):
        m, se, _ = gr.ratio_stats(r["ll"][sl], ll)
        print(f"{which} on {name}: mean exp(ll_hat - ll) = {m:.4f} +- {se:.4f}, {abs(m - 1.0) / se:.1f} standard errors from 1")
        worst = max(worst, abs(m - 1.0) / se)
    assert worst > gr.SIGMAS


@pytest.mark.parametrize("name", gr.NAMES)
@pytest.mark.parametrize("kind", ["pf", "aux"])
def test_filtering_means_are_the_grid_filter_s(runs, kind, name):
    gr.hold_means(kind, name, runs(kind, name, True))


@pytest.mark.parametrize("which", gr.LATE_MUTANTS)
def test_a_late_f_or_g_index_moves_the_filtering_means_past_the_bound(which):
    kw = gr.mutant(gr.args_of("pf", "irregular-poisson", True), which)
    excess = gr.means_excess("pf", "irregular-poisson", pr.run(**kw))
    print(f"{which}: the largest deviation is {excess:.1f} times its bound")
    assert excess > 1.0
