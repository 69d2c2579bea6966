"""NumPy restatement of the two factor stochastic-volatility kernels (bayesian_dlms_amd/csrc/dlm_fsv.hip), operation for operation and in
the kernels' summation order, vectorised over the panels: `factors` (k_fsv_factors) and `loadings` (k_fsv_loadings), with the small
SPD solve they share (`solve_draw`: fsv_solve_draw).  What the GPU tests hold the kernels to draw for draw (tests/test_factorsv_gpu.py)
and what the host tests check against the model (tests/test_factorsv_host.py).  The Philox counters, the Gamma and the normal are
tests/sampler_restatement.py's.

`literal=True` is the reference's arithmetic; `mutant` injects ONE of the four quirks into the default
arithmetic:  "Q27" the draw P^-1 z for L^-T z;  "Q28" InverseGamma(shape + n / 2, scale + ssy / (2 p));  "Q29" the prior variance
where the precision belongs and no prior mean;  "Q30" the rows i < k regress y_i, not y_i - f_i.

The second half is the exact-invariance setup both test files use: `exact_start` draws (alpha, beta, sigma^2, f, y) from the model's
joint law, one fsv_factors and one fsv_loadings step follow (each a draw from a full conditional, so the joint law is unchanged), and
`figures` / `failed` hold the result against closed-form laws.  Run as a script the module prints the rehearsal table of
profiles/r15_notes.md:  python tests/fsv_restatement.py [N]."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sampler_restatement import SLOT_TOP, gamma_unit, gibbs_rand, normal, philox  # noqa: E402,F401

from bayesian_dlms_amd import _lib  # noqa: E402

KEY_FSV = 0x46535620
FSV_SLOT_SIGMA, FSV_SLOT_ROW0 = SLOT_TOP, SLOT_TOP - 1
MUTANTS = ("Q27", "Q28", "Q29", "Q30")
TWO_PI = 6.283185307179586476925286766559


def normals(seed, series, it, comp, attempt):
    """draw_normal on DLM_KEY_FSV for arrays (series, comp, attempt) of one shape."""
    series, comp, attempt = np.broadcast_arrays(np.asarray(series, np.int64), np.asarray(comp, np.int64), np.asarray(attempt, np.int64))
    u1, u2 = gibbs_rand(seed, series, it, comp, attempt, 0, KEY_FSV)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI * u2)


def gamma_units(a, seed, series, it, comp, key):
    """gamma_unit of sampler_restatement for one shape a [N] and comp per SERIES [N] (the imported one takes one series): the same
    attempts, the same counters (tests/test_factorsv_host.py holds the two against each other)."""
    a = np.array(a, dtype=np.float64).copy()
    series = np.asarray(series, np.int64)
    comp = np.broadcast_to(np.asarray(comp, np.int64), a.shape)
    boost = np.ones_like(a)
    small = a < 1.0
    if small.any():
        u1, _ = gibbs_rand(seed, series[small], it, comp[small], 1023, 0, key)
        boost[small] = u1 ** (1.0 / a[small])
        a[small] += 1.0
    dd = a - 1.0 / 3.0
    cc = 1.0 / np.sqrt(9.0 * dd)
    out = dd * boost
    todo = np.ones(a.shape, bool)
    for k in range(1023):
        idx = np.nonzero(todo)[0]
        if idx.size == 0:
            break
        u1, u2 = gibbs_rand(seed, series[idx], it, comp[idx], k, 0, key)
        x = np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI * u2)
        v = 1.0 + cc[idx] * x
        pos = v > 0.0
        v = np.where(pos, v, 1.0)
        v = v * v * v
        w1, _ = gibbs_rand(seed, series[idx], it, comp[idx], k, 1, key)
        ddi = dd[idx]
        ok = pos & (np.log(w1) < 0.5 * x * x + ddi - ddi * v + ddi * np.log(v))
        out[idx[ok]] = ddi[ok] * v[ok] * boost[idx[ok]]
        todo[idx[ok]] = False
    return out


def solve_draw(P, r, z, lit):
    """fsv_solve_draw over leading batch dimensions: P [..][q][q] (the LOWER triangle is read), r, z [..][q].
    -> (x = P^-1 r + L^-T z, or P^-1 r + P^-1 z with lit; ok: every pivot positive)."""
    with np.errstate(all="ignore"):
        return _solve_draw(P, r, z, lit)


def _solve_draw(P, r, z, lit):
    q = r.shape[-1]
    L = np.zeros_like(P)
    ok = np.ones(r.shape[:-1], bool)
    for j in range(q):
        s = P[..., j, j].copy()
        for m in range(j):
            s = s - L[..., j, m] * L[..., j, m]
        ok &= s > 0.0
        d = np.sqrt(s)
        L[..., j, j] = d
        for i in range(j + 1, q):
            e = P[..., i, j].copy()
            for m in range(j):
                e = e - L[..., i, m] * L[..., j, m]
            L[..., i, j] = e / d
    x = np.array(r, dtype=np.float64)
    for i in range(q):
        s = x[..., i] + z[..., i] if lit else x[..., i].copy()
        for m in range(i):
            s = s - L[..., i, m] * x[..., m]
        x[..., i] = s / L[..., i, i]
    for i in range(q - 1, -1, -1):
        s = x[..., i].copy() if lit else x[..., i] + z[..., i]
        for m in range(i + 1, q):
            s = s - L[..., m, i] * x[..., m]
        x[..., i] = s / L[..., i, i]
    return x, ok


def _cond(P):
    """Largest 2-norm condition number of the symmetric matrices whose lower triangles are P [..][q][q] (0 for none)."""
    if P.size == 0:
        return 0.0
    low = np.tril(P)
    sym = low + np.swapaxes(np.tril(P, -1), -1, -2)
    sym = sym[np.isfinite(sym).all(axis=(-1, -2))]
    return float(np.linalg.cond(sym).max()) if sym.size else 0.0


def factors(y, beta, v, alpha, *, seed, series_offset, it, literal=False, mutant=None):
    """k_fsv_factors.  y [N][T][p], beta [N][p][k], v [N][p], alpha [N][k][T+1] or None.  -> (f [N][k][T], status [N], the largest
    condition number of a P_t)."""
    N, T, p = y.shape
    k = beta.shape[2]
    lit = bool(literal) or mutant == "Q27"
    with np.errstate(all="ignore"):
        iv = 1.0 / v
        A = np.zeros((N, k, k))
        for r in range(k):
            for c in range(k):
                s = np.zeros(N)
                for i in range(p):
                    s = s + (beta[:, i, r] * iv[:, i]) * beta[:, i, c]
                A[:, r, c] = s
        rr = np.zeros((N, T, k))
        for i in range(p):
            w = y[:, :, i] * iv[:, None, i]
            for j in range(k):
                rr[:, :, j] = rr[:, :, j] + beta[:, None, i, j] * w
        if alpha is None:
            d = np.ones((N, T, k))
            abad = np.zeros((N, T), bool)
        else:
            x = np.transpose(alpha[:, :, 1:], (0, 2, 1))
            d = np.exp(-x)
            abad = (~np.isfinite(x) | ~(d < np.inf)).any(axis=2)
        P = np.broadcast_to(A[:, None], (N, T, k, k)).copy()
        for j in range(k):
            P[:, :, j, j] = A[:, None, j, j] + d[:, :, j]
        series = (series_offset + np.arange(N))[:, None, None]
        z = normals(seed, series, it, np.arange(T)[None, :, None], np.arange(k)[None, None, :])
        obs = np.isfinite(y).all(axis=2)
        xs, ok = solve_draw(P, rr, z, lit)
    keep = obs & ~abad & ok
    f = np.where(keep[:, :, None], xs, np.nan)
    status = np.zeros(N, np.int32)
    status[abad.any(axis=1)] |= _lib.ST_NONFINITE
    status[(obs & ~abad & ~ok).any(axis=1)] |= _lib.ST_NOT_PD
    bad = ~np.isfinite(beta).all(axis=(1, 2)) | ~((v > 0.0) & (v < np.inf)).all(axis=1)
    f[bad] = np.nan
    status[bad] = _lib.ST_NONFINITE
    return np.ascontiguousarray(np.transpose(f, (0, 2, 1))), status, _cond(P[keep & ~bad[:, None]])


def loadings(y, f, beta, v_in, prior, *, seed, series_offset, it, mutant=None):
    """k_fsv_loadings.  y [N][T][p], f [N][k][T], beta [N][p][k], v_in [N][p] or None, prior: the five fields of dlm_fsv_prior as a dict.
    -> (beta_out [N][p][k], v_out [N][p], status [N], the largest condition number of a row's precision)."""
    N, T, p = y.shape
    k = beta.shape[2]
    lit = bool(prior["literal"])
    q27, q28, q29, q30 = (lit or mutant == m for m in MUTANTS)
    counted = np.isfinite(y).all(axis=2) & np.isfinite(f).all(axis=1)
    with np.errstate(all="ignore"):
        cw, yw, Sw, nw = [], [], [], []
        for w in range(4):                      # wave w: the times w, w + 4, ... in order
            c, ssy, S, cnt = np.zeros((N, p, k)), np.zeros((N, p)), np.zeros((N, k, k)), np.zeros(N, np.int64)
            for t in range(w, T, 4):
                m = counted[:, t]
                ft, yv = f[:, :, t], y[:, t, :]
                pred = np.zeros((N, p))
                for j in range(k):
                    pred = pred + beta[:, :, j] * ft[:, None, j]
                res = yv - pred
                c = np.where(m[:, None, None], c + ft[:, None, :] * yv[:, :, None], c)
                ssy = np.where(m[:, None], ssy + res * res, ssy)
                S = np.where(m[:, None, None], S + ft[:, :, None] * ft[:, None, :], S)
                cnt = cnt + m
            cw.append(c); yw.append(ssy); Sw.append(S); nw.append(cnt)
        c = ((cw[0] + cw[1]) + cw[2]) + cw[3]
        ssy_l = ((yw[0] + yw[1]) + yw[2]) + yw[3]
        S = ((Sw[0] + Sw[1]) + Sw[2]) + Sw[3]
        nobs = ((nw[0] + nw[1]) + nw[2]) + nw[3]
        tot = np.zeros(N)
        for l in range(p):
            tot = tot + ssy_l[:, l]
        bad = ~np.isfinite(tot) | ~np.isfinite(S).all(axis=(1, 2)) | ~np.isfinite(c).all(axis=(1, 2))
        empty = nobs == 0
        live = ~bad & ~empty
        nd, pd = nobs.astype(np.float64), float(p)
        shape = prior["sigma_shape"] + 0.5 * nd if q28 else prior["sigma_shape"] + 0.5 * (nd * pd)
        scale = prior["sigma_scale"] + tot / (2.0 * pd) if q28 else prior["sigma_scale"] + 0.5 * tot
        series = series_offset + np.arange(N)
        g = np.full(N, np.nan)
        idx = np.nonzero(live)[0]
        if idx.size <= 64:
            for n in idx:
                g[n] = gamma_unit(shape[n], seed, int(series[n]), it, FSV_SLOT_SIGMA, KEY_FSV)[0]
        else:
            g[idx] = gamma_units(shape[idx], seed, series[idx], it, FSV_SLOT_SIGMA, KEY_FSV)
        s2 = scale / g
        sd2 = prior["beta_sd"] * prior["beta_sd"]
        pdiag = sd2 if q29 else 1.0 / sd2
        pmean = 0.0 if q29 else prior["beta_mean"] / sd2
        beta_out = np.zeros((N, p, k))
        status = np.zeros(N, np.int32)
        cond = 0.0
        for i in range(p):
            if i < k:
                beta_out[:, i, i] = 1.0
            qd = min(i, k)
            if qd == 0:
                continue
            P = S[:, :qd, :qd] / s2[:, None, None]
            for a in range(qd):
                P[:, a, a] = S[:, a, a] / s2 + pdiag
            own = c[:, i, :qd] - S[:, :qd, i] if (i < k and not q30) else c[:, i, :qd]
            r = own / s2[:, None] + pmean
            z = normals(seed, series[:, None], it, FSV_SLOT_ROW0 - i, np.arange(qd)[None, :])
            x, ok = solve_draw(P, r, z, q27)
            beta_out[:, i, :qd] = np.where(ok[:, None], x, np.nan)
            status[live & ~ok] |= _lib.ST_NOT_PD
            cond = max(cond, _cond(P[live]))
    v_out = np.broadcast_to(s2[:, None], (N, p)).copy()
    beta_out[bad] = np.nan
    v_out[bad] = np.nan
    status[bad] = _lib.ST_NONFINITE
    beta_out[empty] = beta[empty]
    v_out[empty] = np.nan if v_in is None else v_in[empty]
    status[empty] = _lib.ST_NONFINITE
    return beta_out, v_out, status, cond


def fsv_prior(literal=0, beta=(0.3, 0.7), sigma=(4.0, 1.5)):
    return dict(literal=literal, beta_mean=beta[0], beta_sd=beta[1], sigma_shape=sigma[0], sigma_scale=sigma[1])


def fsv_prior_tuple(pr):
    return tuple(pr[k] for k, _ in _lib.FsvPrior._fields_)


# ---- the exact-invariance setup ---------------------------------------------------------------------------------------------------
SEED = 20261                 # fixed before any run
INV_N, INV_P, INV_K, INV_T, INV_MISSING = 16384, 5, 2, 6, 0.1
INV_SV = (0.8, 0.0, 0.3)     # (phi, mu, sigma_eta) of every factor
INV_PRIOR = fsv_prior()      # beta ~ N(0.3, 0.7^2), sigma^2 ~ InverseGamma(4, 1.5)
SE_BOUND, P_MARGINAL = 5.0, 1e-3          # tests/gibbs_invariance.py
# Mean |new - old| of the free loadings and of the observed factors.  With about 5.4 observed times the conditional standard deviations
# are about 0.27 (beta: precision S / sigma^2 + 1 / 0.49 ~ 6 / 0.5 + 2) and 0.36 (f: beta^T beta / sigma^2 + e^-alpha ~ 3.3 / 0.5 + 1), so a
# fresh conditional draw moves either by a few tenths; a step that returns its input gives 0.
NEW_DRAW_FLOOR = 0.05
CHECKS = ("beta mean", "beta variance", "sigma KS", "factor mean", "factor variance", "residual mean", "residual variance", "new draw")
# the check each quirk is named for (the rehearsal table of profiles/r15_notes.md has every figure)
MUTANT_CHECK = {"Q27": "factor variance", "Q28": "sigma KS", "Q29": "beta variance", "Q30": "beta variance", "literal": "beta variance"}


def free_mask(p, k):
    return np.tril(np.ones((p, k), bool), -1)


def exact_start(N=INV_N, seed=SEED):
    """{"alpha" [N][k][T+1], "beta" [N][p][k], "v" [N][p], "f" [N][k][T], "y" [N][T][p]} from the model's joint law; whole times are then
    masked with probability 0.1 (the mask does not depend on the values)."""
    rng = np.random.default_rng([seed, 0x465356])
    p, k, T = INV_P, INV_K, INV_T
    phi, mu, sig = INV_SV
    alpha = np.empty((N, k, T + 1))
    alpha[:, :, 0] = mu + sig / math.sqrt(1.0 - phi * phi) * rng.standard_normal((N, k))
    for t in range(T):
        alpha[:, :, t + 1] = mu + phi * (alpha[:, :, t] - mu) + sig * rng.standard_normal((N, k))
    beta = np.zeros((N, p, k))
    beta[:, free_mask(p, k)] = INV_PRIOR["beta_mean"] + INV_PRIOR["beta_sd"] * rng.standard_normal((N, int(free_mask(p, k).sum())))
    beta[:, np.arange(k), np.arange(k)] = 1.0
    s2 = INV_PRIOR["sigma_scale"] / rng.gamma(INV_PRIOR["sigma_shape"], 1.0, N)
    f = rng.standard_normal((N, k, T)) * np.exp(0.5 * alpha[:, :, 1:])
    y = np.einsum("nij,njt->nti", beta, f) + np.sqrt(s2)[:, None, None] * rng.standard_normal((N, T, p))
    y[rng.random((N, T)) < INV_MISSING] = np.nan
    return {"alpha": alpha, "beta": beta, "v": np.broadcast_to(s2[:, None], (N, p)).copy(), "f": f, "y": y}


def _se(x, obs):
    """Largest |mean| and |var - 1| over the columns of x [N][..] in standard errors, each column at its observed count (obs [N][..])."""
    n = obs.sum(axis=0).astype(np.float64)
    xm = np.where(obs, x, 0.0)
    mean = xm.sum(axis=0) / n
    var = np.where(obs, (x - mean) ** 2, 0.0).sum(axis=0) / n
    return float((np.abs(mean) * np.sqrt(n)).max()), float((np.abs(var - 1.0) / np.sqrt(2.0 / n)).max())


def figures(start, f_new, beta_new, v_new):
    """The figures of the checks after one factors and one loadings step from `start`."""
    from scipy import stats as ss
    N, T, p = start["y"].shape
    k = beta_new.shape[2]
    fm = free_mask(p, k)
    obs = np.isfinite(start["y"]).all(axis=2)                                  # [N][T]
    zb = (beta_new[:, fm] - INV_PRIOR["beta_mean"]) / INV_PRIOR["beta_sd"]
    out = {"N": N}
    out["beta mean"], out["beta variance"] = _se(zb, np.ones(zb.shape, bool))
    out["sigma KS"] = float(ss.kstest(1.0 / v_new[:, 0], ss.gamma(INV_PRIOR["sigma_shape"], scale=1.0 / INV_PRIOR["sigma_scale"]).cdf).pvalue)
    ft = np.transpose(f_new, (0, 2, 1))                                        # [N][T][k]
    white = ft / np.exp(0.5 * np.transpose(start["alpha"][:, :, 1:], (0, 2, 1)))
    out["factor mean"], out["factor variance"] = _se(white, np.broadcast_to(obs[:, :, None], white.shape))
    res = (start["y"] - np.einsum("nij,ntj->nti", beta_new, ft)) / np.sqrt(v_new)[:, None, :]
    out["residual mean"], out["residual variance"] = _se(res, np.broadcast_to(obs[:, :, None], res.shape))
    out["moved beta"] = float(np.abs(beta_new[:, fm] - start["beta"][:, fm]).mean())
    out["moved f"] = float(np.abs(ft - np.transpose(start["f"], (0, 2, 1)))[obs].mean())
    return out


def failed(fig):
    """The names of the checks `fig` fails, in the order of CHECKS."""
    bad = [c for c in CHECKS[:2] + CHECKS[3:7] if not fig[c] <= SE_BOUND]
    if not fig["sigma KS"] > P_MARGINAL:
        bad.append("sigma KS")
    if not (fig["moved beta"] > NEW_DRAW_FLOOR and fig["moved f"] > NEW_DRAW_FLOOR):
        bad.append("new draw")
    return [c for c in CHECKS if c in bad]


def describe(fig):
    return (f"N {fig['N']}  beta (mean, var) {fig['beta mean']:.2f} {fig['beta variance']:.2f} se  sigma^2 KS p {fig['sigma KS']:.3g}  whitened factors "
            f"{fig['factor mean']:.2f} {fig['factor variance']:.2f} se  residuals {fig['residual mean']:.2f} {fig['residual variance']:.2f} se  "
            f"moved: beta {fig['moved beta']:.3f} f {fig['moved f']:.3f}")


def step_host(start, *, literal=False, mutant=None, seed=SEED):
    """One factors and one loadings step of the restatement from `start`: (f_new, beta_new, v_new)."""
    pr = dict(INV_PRIOR, literal=1 if literal else 0)
    f, st, _ = factors(start["y"], start["beta"], start["v"], start["alpha"], seed=seed, series_offset=0, it=0, literal=literal, mutant=mutant)
    b, v, st2, _ = loadings(start["y"], f, start["beta"], start["v"], pr, seed=seed, series_offset=0, it=0, mutant=mutant)
    assert not st.any() and not st2.any(), (st.max(), st2.max())
    return f, b, v


def rehearse(N=INV_N, out=sys.stdout):
    for seed in (SEED, SEED + 1):
        start = exact_start(N, seed)
        for label, kw in [("default", {})] + [(m, {"mutant": m}) for m in MUTANTS] + [("literal", {"literal": True})]:
            fig = figures(start, *step_host(start, seed=seed, **kw))
            print(f"seed {seed} {label:8s} {describe(fig)}   fails: {failed(fig)}", file=out, flush=True)


if __name__ == "__main__":
    rehearse(*[int(a) for a in sys.argv[1:]])
