"""The Student-t Gibbs driver (bayesian_dlms_amd/studentt.py) without a GPU: what it passes to its two engine calls (injected
fakes), the initial nu, and the code object of the step kernel (dlm_studentt.o: no scratch, no spills)."""
import numpy as np
import pytest

from bayesian_dlms_amd import _lib
from bayesian_dlms_amd.dlm import Dlm, DlmParameters
from bayesian_dlms_amd.gibbs import InverseGamma
from bayesian_dlms_amd.studentt import NegativeBinomialProposal, Poisson, StudentT, initial_nu
from code_object import kernel_resources


class _Fakes:
    """ffbs / step stand-ins that record their inputs; the step's outputs are distinct per iteration and per series."""

    def __init__(self, N, T, d):
        self.N, self.T, self.d = N, T, d
        self.ffbs_calls, self.step_calls = [], []

    def ffbs(self, mat, params, y, *, seed, series_offset, flags, want_theta, want_stats, want_filt):
        V, vs, W, ws, m0, m0s, C0, c0s, vts, wts = params
        self.ffbs_calls.append(dict(V=np.array(V).reshape(self.N, self.T), vs=vs, vts=vts, W=np.array(W).reshape(self.N, -1), ws=ws,
                                    flags=flags, want_filt=want_filt, seed=seed, series_offset=series_offset))
        it = len(self.ffbs_calls)
        return {"theta": np.full((self.N, self.T + 1, self.d), float(it)), "stats": np.zeros((self.N, self.d + 3)),
                "status": np.zeros(self.N, np.int32)}

    def step(self, mat, y, theta, stats, prior, scale, nu, *, iteration, accepted, seed, series_offset, literal):
        self.step_calls.append(dict(scale=np.array(scale), nu=np.array(nu), iteration=iteration, literal=literal, prior=prior,
                                    accepted=np.array(accepted)))
        k = iteration + 1
        n = np.arange(self.N)
        W = np.zeros((self.N, self.d * self.d))
        W[:, 0] = 100.0 * k + n
        return {"v": 1000.0 * k + n[:, None] + np.arange(self.T)[None, :] / 1000.0, "scale": 10.0 * k + n,
                "nu": (np.array(nu) + 1).astype(np.int32), "W": W, "accepted": np.array(accepted) + 1,
                "loglik": np.zeros(self.N), "status": np.zeros(self.N, np.int32)}


def _run(literal, n_iter=3, simsmooth=False):
    N, T = 5, 7
    mod = Dlm.polynomial(1)
    p0 = DlmParameters([[2.5]], [[0.7]], [0.0], [[1.0]])
    fk = _Fakes(N, T, 1)
    y = np.random.default_rng(1).standard_normal((N, T))
    states = list(StudentT.sample(y, InverseGamma(3.0, 3.0), Poisson(3.0), NegativeBinomialProposal(1.0), mod, p0, None,
                                  n_iter=n_iter, seed=4, nu0=5, literal=literal, ffbs=fk.ffbs, step=fk.step,
                                  keep_variances=True, simulation_smoother=simsmooth))
    return fk, states, N, T


def test_literal_mode_passes_the_initial_scale_and_w_to_every_call():
    fk, states, N, T = _run(literal=True)
    for c in fk.step_calls:
        np.testing.assert_array_equal(c["scale"], np.full(N, 2.5))
        assert c["literal"] is True
    for c in fk.ffbs_calls:
        np.testing.assert_array_equal(c["W"], np.full((N, 1), 0.7))


def test_corrected_mode_passes_the_previous_draws():
    fk, states, N, T = _run(literal=False)
    np.testing.assert_array_equal(fk.step_calls[0]["scale"], np.full(N, 2.5))
    np.testing.assert_array_equal(fk.ffbs_calls[0]["W"], np.full((N, 1), 0.7))
    for k in range(1, 3):
        np.testing.assert_array_equal(fk.step_calls[k]["scale"], 10.0 * k + np.arange(N))
        np.testing.assert_array_equal(fk.ffbs_calls[k]["W"][:, 0], 100.0 * k + np.arange(N))
        np.testing.assert_array_equal(fk.step_calls[k]["nu"], 5 + k)             # nu moves on in both modes
        np.testing.assert_array_equal(fk.step_calls[k]["accepted"], k)
    assert [c["iteration"] for c in fk.step_calls] == [0, 1, 2]
    np.testing.assert_array_equal(states[-1].p.scale, 30.0 + np.arange(N))
    np.testing.assert_array_equal(states[-1].accepted, 3)


@pytest.mark.parametrize("literal", [False, True])
def test_the_v_stream_is_the_previous_step_output_and_starts_at_one(literal):
    fk, states, N, T = _run(literal=literal)
    np.testing.assert_array_equal(fk.ffbs_calls[0]["V"], np.ones((N, T)))
    for k in range(1, 3):
        np.testing.assert_array_equal(fk.ffbs_calls[k]["V"], states[k - 1].variances)
        np.testing.assert_array_equal(fk.ffbs_calls[k]["V"][:, 0], 1000.0 * k + np.arange(N))
    for c in fk.ffbs_calls:     # per-series V stream (v_stride = T, v_tstride = p * p = 1), per-series W, no filter records
        assert c["vs"] == T and c["vts"] == 1 and c["ws"] == 1 and c["want_filt"] is False
        assert c["flags"] == 0


def test_simulation_smoother_flag_and_its_refusal_above_d15():
    fk, states, N, T = _run(literal=False, n_iter=1, simsmooth=True)
    assert fk.ffbs_calls[0]["flags"] == _lib.OPT_FFBS_SIMSMOOTH
    mod = Dlm.polynomial(1) + Dlm.seasonal(24, 8)        # d = 17
    p0 = DlmParameters([[1.0]], np.eye(17), np.zeros(17), np.eye(17))
    with pytest.raises(ValueError, match="d <= 15"):
        next(StudentT.sample(np.zeros((2, 10)), InverseGamma(3.0, 3.0), Poisson(3.0), NegativeBinomialProposal(1.0), mod, p0, None,
                             n_iter=1, simulation_smoother=True, ffbs=lambda *a, **k: None, step=lambda *a, **k: None))


def test_initial_nu_is_never_zero_and_does_not_depend_on_the_sharding():
    prior = Poisson(0.7)      # P(0) = 0.5: many redraws
    full = initial_nu(prior, 400, seed=9)
    assert (full >= 1).all()
    halves = np.concatenate([initial_nu(prior, 150, seed=9), initial_nu(prior, 250, seed=9, series_offset=150)])
    np.testing.assert_array_equal(full, halves)
    assert len(np.unique(full)) > 2
    fk, states, N, T = _run(literal=False, n_iter=1)
    fk2 = _Fakes(N, T, 1)
    y = np.zeros((N, T))
    next(StudentT.sample(y, InverseGamma(3.0, 3.0), prior, NegativeBinomialProposal(1.0), Dlm.polynomial(1),
                         DlmParameters([[1.0]], [[1.0]], [0.0], [[1.0]]), None, n_iter=1, seed=9, series_offset=3,
                         ffbs=fk2.ffbs, step=fk2.step))
    np.testing.assert_array_equal(fk2.step_calls[0]["nu"], full[3:3 + N])


def test_step_kernel_has_no_scratch_and_no_spills():
    """dlm_studentt.o's code object: k_studentt_step keeps everything in registers (read as test_per_wave_kernels_keep_their_registers
    reads dlm_wave48.o)."""
    assert kernel_resources("dlm_studentt.o", "k_studentt_step")[:2] == (0, 0)
