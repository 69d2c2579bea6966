"""The engine calls that FactorSv.sample_ar, DlmFsv.sample and DlmFsvSystem.sample compose, in their order and with their iteration, seed,
series offset and literal flag, recorded from a stub engine and held to the numbered steps of the three modules' docstrings.  No device: the
stub returns zeros of the right shapes (host tensors: a chain lives where its ys does, and a host array beside an engine would be moved to
the engine's device), so nothing is said about a draw -- the drivers are held draw for draw to their calls composed by hand in the GPU
tests.  This is the check of a driver's order, seeds and offsets that runs without a device."""
import numpy as np
import pytest

from bayesian_dlms_amd.dlm import Dlm, DlmParameters
from bayesian_dlms_amd.dlmfsv import DlmFsv, DlmFsvParameters
from bayesian_dlms_amd.dlmfsvsys import DlmFsvSystem, DlmFsvSystemParameters
from bayesian_dlms_amd.factorsv import INIT_ITERATION, FactorSv, FsvParameters
from bayesian_dlms_amd.gibbs import InverseGamma
from bayesian_dlms_amd.stochvol import Gaussian, SvParameters

N, T, P, K = 2, 3, 3, 2
SEED, OFFSET = 21, 5
VOL_SEED = 21 * 1000003           # the AR(1) FFBS of the volatilities: a seed per call, + 0 at the start and + it + 1 in iteration it
THETA_SEED = VOL_SEED ^ (1 << 63)          # the state's FFBS: the same with the top bit flipped
PRIORS = (Gaussian(0.0, 1.0), InverseGamma(3.0, 0.3), Gaussian(0.8, 0.1), Gaussian(0.0, 1.0), InverseGamma(3.0, 1.0), InverseGamma(3.0, 0.5))


class StubEngine:
    """Records (name, iteration, seed, series_offset, literal) of every call -- None where a call takes no such argument, the literal flag
    of a prior struct where the call takes one -- and returns zeros (a given out= buffer where there is one)."""

    def __init__(self):
        self.calls = []

    def _note(self, name, iteration=None, seed=None, series_offset=None, literal=None, prior=None, **_):
        self.calls.append((name, iteration, seed, series_offset, bool(prior.literal) if prior is not None else literal))

    @staticmethod
    def _out(out, status_n, **shapes):
        import torch
        res = {key: out[key] if out and key in out else torch.zeros(shape, dtype=torch.float64) for key, shape in shapes.items()}
        return dict(res, status=torch.zeros(status_n, dtype=torch.int32))

    def mem_info(self):
        self._note("mem_info")
        return 1 << 40, 1 << 40

    def ffbs(self, mat, params, y, *, want_theta, want_stats, want_filt, **kw):
        self._note("ffbs", **kw)
        n = y.shape[0]
        assert want_theta and not want_filt and len(params) == 10
        return self._out(None, n, theta=(n, mat.T + 1, mat.d), **({"stats": (n, 2 * mat.p + mat.d + 1)} if want_stats else {}))

    def dinvgamma_step(self, d, p, stats, prior_v, prior_w, **kw):
        self._note("dinvgamma_step", **kw)
        out = self._out(None, 0, V=(stats.shape[0], p * p), W=(stats.shape[0], d * d))
        return out["V"], out["W"]

    def dlmfsv_center(self, mat, y, theta, out=None):
        self._note("dlmfsv_center")
        return self._out(out, y.shape[0], r=tuple(y.shape))

    def dlmfsv_impute(self, r, beta, v, alpha, out=None, **kw):
        self._note("dlmfsv_impute", **kw)
        return self._out(out, r.shape[0], r=tuple(r.shape))

    def dlmfsvsys_innovations(self, mat, theta, out=None):
        self._note("dlmfsvsys_innovations")
        return self._out(out, theta.shape[0], w=(theta.shape[0], mat.T, mat.d))

    def dlmfsv_variance(self, beta, v, alpha, out=None):
        self._note("dlmfsv_variance")
        n, q, _ = beta.shape
        return self._out(out, n, V=(n, alpha.shape[2] - 1, q * q))

    def fsv_factors(self, y, beta, v, alpha, out=None, **kw):
        self._note("fsv_factors", **kw)
        return self._out(out, y.shape[0], f=(y.shape[0], beta.shape[2], y.shape[1]))

    def fsv_loadings(self, y, f, beta, prior, v=None, out=None, **kw):
        self._note("fsv_loadings", prior=prior, **kw)
        return self._out(out, y.shape[0], beta=tuple(beta.shape), v=tuple(beta.shape[:2]))

    def sv_mixture(self, y, alpha, out=None, **kw):
        self._note("sv_mixture", **kw)
        return self._out(out, y.shape[0], ystar=tuple(y.shape), v=tuple(y.shape))

    def ar1_ffbs(self, y, v, sv, *, want_filt, want_theta, **kw):
        self._note("ar1_ffbs", **kw)
        assert want_theta and not want_filt
        return self._out(None, y.shape[0], theta=(y.shape[0], y.shape[1] + 1))

    def sv_params(self, alpha, sv, prior, out=None, **kw):
        self._note("sv_params", prior=prior, **kw)
        return self._out(out, alpha.shape[0], sv=(alpha.shape[0], 3))


def row(step, it, literal):
    """The record of one call of iteration `it` (None: the start).  The calls on the N k factor series take the chain (n, j) as the series
    (series_offset + n) k + j: their offset is OFFSET K."""
    c = 0 if it is None else it + 1          # the FFBS calls count from the start's
    return {"mem_info": ("mem_info", None, None, None, None),
            "center": ("dlmfsv_center", None, None, None, None),
            "impute": ("dlmfsv_impute", it, SEED, OFFSET, None),
            "innovations": ("dlmfsvsys_innovations", None, None, None, None),
            "factors": ("fsv_factors", INIT_ITERATION if it is None else it, SEED, OFFSET, literal),
            "mixture": ("sv_mixture", 0 if it is None else it, SEED, OFFSET * K, None),
            "ar1": ("ar1_ffbs", None, VOL_SEED + c, OFFSET * K, None),
            "sv_params": ("sv_params", it, SEED, OFFSET * K, literal),
            "loadings": ("fsv_loadings", it, SEED, OFFSET, literal),
            "variance": ("dlmfsv_variance", None, None, None, None),
            "ffbs": ("ffbs", None, THETA_SEED + c, OFFSET, None),
            "static variance": ("dinvgamma_step", it, SEED, OFFSET, None)}[step]


def expected(start, steps, literal):
    return [row(s, None, literal) for s in start] + [row(s, it, literal) for it in (0, 1) for s in steps]


# initialiseFactors, then initial_state_ar on the factor series
FSV_START = ["factors", "mixture", "ar1"]
# factorsv.py: sampleStep's order
FSV_STEPS = ["mixture", "ar1", "sv_params", "factors", "loadings"]
# dlmfsv.py, steps 1-7; the completion is the second call of step 1
DLMFSV_STEPS = ["center", "impute", "factors", "mixture", "ar1", "sv_params", "loadings", "variance", "ffbs", "static variance"]
# Q32: sampleStep runs 3, 2, 4, 5, 6, 7
DLMFSV_LITERAL_ORDER = ["center", "impute", "mixture", "ar1", "sv_params", "factors", "loadings", "variance", "ffbs", "static variance"]
# dlmfsvsys.py, steps 1-7, and Q35: sampleStep runs 1, 3, 2, 4, 5, 6, 7
SYS_STEPS = ["innovations", "factors", "mixture", "ar1", "sv_params", "loadings", "variance", "ffbs", "static variance"]
SYS_LITERAL_ORDER = ["innovations", "mixture", "ar1", "sv_params", "factors", "loadings", "variance", "ffbs", "static variance"]


def _fsv(rows):
    return FsvParameters(0.5, FactorSv.build_beta(rows, K, 0.3), [SvParameters(0.8, 0.0, 0.3)] * K)


def _ys(p):
    import torch
    return torch.zeros((N, T, p), dtype=torch.float64)          # a host tensor: the chain lives where ys does


def _trace(states, eng, status_n=N):
    states = list(states)
    assert len(states) == 2 and all(s.status.shape == (status_n,) and not s.status.any() for s in states)
    return eng.calls


@pytest.mark.parametrize("literal", [False, True])
def test_factorsv_sample_ar_composes_its_five_calls(literal):
    eng = StubEngine()
    got = _trace(FactorSv.sample_ar(PRIORS[0], PRIORS[1], PRIORS[3], PRIORS[2], PRIORS[4], _ys(P), _fsv(P), eng, n_iter=2, seed=SEED,
                                    series_offset=OFFSET, literal=literal), eng)
    assert got == expected(FSV_START, FSV_STEPS, literal)


@pytest.mark.parametrize("literal_missing", [False, True])
@pytest.mark.parametrize("literal_order", [False, True])
def test_dlmfsv_sample_composes_the_steps_of_its_docstring(literal_order, literal_missing):
    mod = Dlm.polynomial(1) * Dlm.polynomial(1) * Dlm.polynomial(1)          # p = 3 series: d = 3 is the smallest
    par = DlmFsvParameters(DlmParameters(np.eye(P), 0.1 * np.eye(3), np.zeros(3), np.eye(3)), _fsv(P))
    eng = StubEngine()
    got = _trace(DlmFsv.sample(*PRIORS, _ys(P), mod, par, eng, n_iter=2, seed=SEED, series_offset=OFFSET, literal_order=literal_order,
                               literal_missing=literal_missing), eng)
    steps = [s for s in (DLMFSV_LITERAL_ORDER if literal_order else DLMFSV_STEPS) if not (literal_missing and s == "impute")]
    assert got == expected(["mem_info", "ffbs", "center"] + FSV_START, steps, False)


@pytest.mark.parametrize("literal_order", [False, True])
def test_dlmfsvsys_sample_composes_the_steps_of_its_docstring(literal_order):
    mod = Dlm.polynomial(1) * Dlm.polynomial(1) * Dlm.polynomial(1)          # p = 3 series: d = 3 is the smallest, and the factor model's rows
    par = DlmFsvSystemParameters(DlmParameters(0.4 * np.eye(P), np.eye(3), np.zeros(3), np.eye(3)), _fsv(3))
    eng = StubEngine()
    got = _trace(DlmFsvSystem.sample(*PRIORS, _ys(P), mod, par, eng, n_iter=2, seed=SEED, series_offset=OFFSET, literal_order=literal_order), eng)
    assert got == expected(["mem_info", "ffbs", "innovations"] + FSV_START, SYS_LITERAL_ORDER if literal_order else SYS_STEPS, False)
