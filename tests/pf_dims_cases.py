"""The inputs of the tests that launch every state dimension of the six particle kernels (tests/test_pf_dims_host.py on the restatements,
tests/test_pf_dims_gpu.py on the device), made from seeds, and the exact references they are held to.

`model(d)`, d = 1 .. 16: pf_cases.dense_model (a dense non-symmetric G, a full W) from the seed 100 + d on pf_cases.time_grid's irregular
grid of T = 8 steps -- three distinct G through g_index, dt = 0 first and at t = 4 -- with a time-varying F [T][d] made as
rb_cases.known_inputs("irregular") makes its own, and y_5 missing.  (At d = 2 dense_model's G is a reflection, which is symmetric: model(2)
changes the sign of its second column (a rotation), so that a transposed G is another matrix at every d > 1.)

A  one launch per (kernel, d) against the kernel's restatement: N = 3 series with per-series V, W, m0, C0 (every stride non-zero), P = 128 (k_rb
   from d = 13 on: 64, its LDS rule refuses (13, 128)), Gaussian, n0 = -1.  k_storvik, k_lw and k_rb learn the DIAGONAL of W under the priors of
   their own tables; k_pg's reference path is the state path its data were simulated from; k_pf_forecast's restatement is put together from
   pf_restatement.run (n0 = P + 1: the filter inside the forecast) and pff_restatement.obs_draw -- `forecast_reference`.
B  against the Kalman filter, which restates nothing of the kernels:
   1  k_rb with every prior sd 0 IS the Kalman filter (rb_cases.kalman_moments per series);
   2  k_pf and the auxiliary k_lw (a = 1, every sd 0) on R replicas of one series: exp(ll_hat - ll_Kalman) averages to 1 (informative
      setting), the filtering means average to the Kalman means (diffuse setting);
   3  k_pf_forecast: (a) from its own cloud it is k_pf with n0 = P + 1; (b) with every y missing its draws are i.i.d.
      N(F_t^T a_t, F_t^T R_t F_t + V) with a_t, R_t the Kalman PREDICTION recursion;
   4  k_pg on model(d): pg_checks' Gaussian check against the Kalman smoother (`smoother`, written down here from the textbook recursion and
      compared with the dense joint law in the host test).

The settings of B.2.  Informative: V = INFORMATIVE_V, W = the model's.  Diffuse: V = DIFFUSE_V, W = the model's.  The weighted mean is a
ratio estimator (tests/pf_cases.py explains the bias); over R replicates bias / standard error ~ sqrt(R / ESS) kappa with kappa the shift the
observations give the mean in standard deviations of the cloud: seven observations of variance 50 against F^T C F ~ 0.4 give kappa ~ 0.25,
under one standard error of bias at R = 1024, and put the weighted mean 25 to 108 standard errors from the unweighted one (at V = 150 four
of the thirty-two (kernel, d) stayed below the 20 the check asks for).

MUTANTS: one misreading of the model each, put into the INPUTS of a restatement while the Kalman reference keeps the true ones."""
import functools

import numpy as np

import lw_restatement as lr
import pf_cases as pc
import pf_restatement as pr
import pff_restatement as fr
import pg_restatement as gr
import rb_cases as rc
import rb_restatement as rr
import storvik_restatement as sr

DIMS = tuple(range(1, 17))
T, N_A, MISSING = 8, 3, 5
KERNELS = ("pf", "storvik", "lw", "rb", "pg", "pff")
VARIANT = {"pf": "pf-wave", "storvik": "storvik-wave", "lw": "lw-wave", "rb": "rb-wave", "pg": "pg-wave", "pff": "pf-forecast-wave"}
RANKS = lambda P: (0, P // 2, P - 1)          # the three order statistics of part A's forecast
# what part A compares: (equal as integers / bit for bit, within RTOL / ATOL)
EQUAL = {"pf": ("status", "ess"), "storvik": ("status", "ess"), "lw": ("status", "ess"), "rb": ("status", "ess"),
         "pg": ("status", "ancestors", "path_index"), "pff": ("status",)}
CLOSE = {"pf": ("ll", "mean", "ess", "cloud", "weights"), "storvik": ("ll", "mean", "ess", "scale_mean", "cloud", "weights", "scales"),
         "lw": ("ll", "mean", "ess", "psi_mean", "psi_var", "cloud", "weights", "psi"),
         "rb": ("ll", "mean", "cov", "ess", "psi_mean", "psi_var", "means", "covs", "weights", "psi"),
         "pg": ("ll", "path", "stats", "clouds", "step_weights"), "pff": ("ll", "mean", "cloud", "weights", "draws", "fmean", "fquant")}
# an entry of part A whose margins are too small takes another seed here (never another tolerance): (kernel, d) -> seed
SEED_OF = {("pf", 6): 2, ("pf", 15): 2}          # (seed 1: 1 / sum W^2 of one step is 1 to the last bit, one particle holds all the weight)


def particles_a(kernel, d):
    return 64 if kernel == "rb" and d >= 13 else 128


@functools.lru_cache(maxsize=None)
def model(d):
    rng = np.random.default_rng(100 + d)
    G0, W, F0 = pc.dense_model(d, rng)
    if d == 2:          # a 2 x 2 Householder QR is ONE reflection: dense_model's G is symmetric at d = 2 whatever the seed, and so are its powers
        G0 = G0 * np.array([1.0, -1.0])
    G, gi, dt = pc.time_grid(dict(T=T, irregular=True), G0)
    F = F0[None] * (1.0 + 0.3 * np.sin(0.7 * np.arange(T)))[:, None] + 0.1 * rng.standard_normal((T, d))
    m0 = 0.3 * rng.standard_normal(d)
    C0 = 0.5 * W + 0.2 * np.eye(d)
    return dict(F=F, G=G, g_index=gi, dt=dt, W=W, m0=m0, C0=C0)


def simulate_series(m, V, W, m0, C0, rng):
    """One series of the model at (V, W, m0, C0): (y [T] with y_MISSING = NaN, the state path [T+1][d])"""
    d = m0.size
    Lw = np.linalg.cholesky(W)
    x = m0 + np.linalg.cholesky(C0) @ rng.standard_normal(d)
    y, path = np.empty(T), np.empty((T + 1, d))
    path[0] = x
    for t in range(T):
        if m["dt"][t] != 0.0:
            x = m["G"][m["g_index"][t]] @ x + np.sqrt(m["dt"][t]) * (Lw @ rng.standard_normal(d))
        path[t + 1] = x
        y[t] = m["F"][t] @ x + np.sqrt(V) * rng.standard_normal()
    y[MISSING] = np.nan
    return y, path


# ---- A: every instantiation against its restatement ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def a_args(kernel, d):
    """The keyword arguments the kernel's restatement takes and, through `a_engine`, the engine."""
    m = model(d)
    seed = SEED_OF.get((kernel, d), 1)
    rng = np.random.default_rng([9000, KERNELS.index(kernel), d, seed])
    diagonal = kernel in ("storvik", "lw", "rb")
    W = np.diag(np.diag(m["W"])) if diagonal else m["W"]
    scale = np.exp(0.3 * rng.standard_normal(N_A))
    Wn, C0n = W[None] * scale[:, None, None], m["C0"][None] * scale[::-1, None, None]
    m0n = m["m0"][None] + 0.2 * rng.standard_normal((N_A, d))
    Vn = pc.FAMILY_V[pr.GAUSSIAN] * np.exp(0.2 * rng.standard_normal(N_A))
    sims = [simulate_series(m, Vn[n], Wn[n], m0n[n], C0n[n], rng) for n in range(N_A)]
    y, ref = np.stack([s[0] for s in sims]), np.stack([s[1] for s in sims])
    P = particles_a(kernel, d)
    kw = dict(F=m["F"], G=m["G"], g_index=m["g_index"], dt=m["dt"], V=Vn, W=Wn, m0=m0n, C0=C0n, y=y, P=P, seed=20 + seed, series_offset=3,
              iteration=5)
    Wd = np.stack([np.diag(Wn[n]) for n in range(N_A)])          # [N][d]
    idx = np.arange(N_A)
    if kernel in ("pf", "pff"):
        kw.update(family=pr.GAUSSIAN, n0=P + 1 if kernel == "pff" else -1, literal=False, nu=None)
    elif kernel == "pg":
        kw.update(family=pr.GAUSSIAN, ref=ref, ancestor_sampling=True, nu=None)
    elif kernel == "storvik":          # InverseGamma (shape, scale), centred as tests/storvik_cases.py centres them
        prior_w = np.stack([np.broadcast_to(4.0 + 0.25 * idx[:, None], (N_A, d)), 3.0 * Wd], axis=2)
        prior_v = np.stack([4.0 + 0.5 * (idx % 3), 3.0 * Vn], axis=1)
        kw.update(family=pr.GAUSSIAN, n0=-1, literal=False, nu=None, learn_v=True, prior_w=prior_w, prior_v=prior_v)
    else:                              # Gaussian (mean, sd) of the log-variances, as tests/lw_cases.py and tests/rb_cases.py
        prior_w = np.stack([np.log(Wd), np.broadcast_to(rc.PRIOR_SD + 0.05 * (idx[:, None] % 4), (N_A, d))], axis=2)
        prior_v = np.stack([np.log(Vn), rc.PRIOR_SD + 0.1 * (idx % 3)], axis=1)
        kw.update(n0=-1, literal=False, learn_v=True, a=0.95, prior_w=prior_w, prior_v=prior_v)
        if kernel == "lw":
            kw.update(family=pr.GAUSSIAN, nu=None)
    return kw


def forecast_reference(kw, ranks):
    """k_pf_forecast on an observed series from its own cloud, from the restatements that exist: the filtering outputs are
    pf_restatement.run's with n0 = P + 1; the draws of step t come from the cloud ADVANCED to t and not yet weighted, which is the final
    cloud of the same run cut after t with y_t missing (every observed step before it resampled: the weights are even), through
    pff_restatement.obs_draw at the sites of slot t; fmean and fquant are the fixed-order mean and the order statistics of those draws."""
    y, F = kw["y"], kw["F"]
    N, P = y.shape[0], kw["P"]
    series = np.uint64(kw["series_offset"]) + np.arange(N, dtype=np.uint64)
    out = pr.run(**kw)
    draws = np.empty((N, T, P))
    for t in range(T):
        cut = y[:, :t + 1].copy()
        cut[:, t] = np.nan
        x = pr.run(**dict(kw, y=cut))["cloud"]
        eta = F[t, 0] * x[:, 0]
        for k in range(1, x.shape[1]):
            eta = eta + F[t, k] * x[:, k]
        yd, _ = fr.obs_draw(pr.GAUSSIAN, eta.reshape(-1), np.repeat(kw["V"], P), None, fr.batch_site(kw["seed"], series, kw["iteration"], t, P))
        draws[:, t] = yd.reshape(N, P)
    out["draws"] = draws
    out["fmean"] = np.stack([fr.forecast_mean(draws[:, t]) for t in range(T)], axis=1)
    out["fquant"] = np.sort(draws, axis=2)[:, :, list(ranks)]
    return out


@functools.lru_cache(maxsize=None)
def a_reference(kernel, d):
    kw = a_args(kernel, d)
    if kernel == "pff":
        return forecast_reference(kw, RANKS(kw["P"]))
    return {"pf": pr.run, "storvik": sr.run, "lw": lr.run, "rb": rr.run, "pg": gr.run}[kernel](**kw)


def a_engine(eng, kernel, d):
    import pff_cases as fc
    import pg_cases as gc
    kw = a_args(kernel, d)
    if kernel == "rb":
        return rc.engine_run(eng, kw)
    if kernel == "pg":
        return gc.engine_run(eng, kw)
    if kernel == "pff":
        return fc.forecast_run(eng, kw, ranks=RANKS(kw["P"]), want_draws=True)
    return pc.engine_run(eng, kw, {"pf": "particle_filter", "storvik": "storvik_filter", "lw": "lw_filter"}[kernel])


# ---- B.1: k_rb with known variances ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def b1_args(d):
    """part A's k_rb inputs with every prior sd 0, V known and a = 1: N = 3 Kalman filters with per-series parameters"""
    kw = dict(a_args("rb", d))
    prior_w = kw["prior_w"].copy()
    prior_w[:, :, 1] = 0.0
    kw.update(prior_w=prior_w, prior_v=None, learn_v=False, a=1.0, seed=11, series_offset=0, iteration=0)
    return kw


def series_of(kw, n):
    """what rb_cases.kalman_moments takes: series n of a batch with per-series parameters, alone"""
    return dict(F=kw["F"], G=kw["G"], g_index=kw["g_index"], dt=kw["dt"], V=float(kw["V"][n]), W=kw["W"][n], m0=kw["m0"][n], C0=kw["C0"][n],
                y=kw["y"][n:n + 1])


def kalman_moments_long(a):
    """rb_cases.kalman_moments in np.longdouble: what the float64 recursion's own rounding is measured against"""
    ld = np.longdouble
    F, G, W = np.asarray(a["F"], dtype=ld), np.asarray(a["G"], dtype=ld), np.asarray(a["W"], dtype=ld)
    y, dt, gi, V = np.asarray(a["y"][0], dtype=ld), a["dt"], a["g_index"], ld(a["V"])
    m, C = np.asarray(a["m0"], dtype=ld).copy(), np.asarray(a["C0"], dtype=ld).copy()
    ms, Cs, ll = np.empty((T, m.size), dtype=ld), np.empty((T, m.size, m.size), dtype=ld), ld(0)
    for t in range(T):
        if dt[t] != 0.0:
            Gt = G[gi[t]]
            m, C = Gt @ m, Gt @ C @ Gt.T + W * ld(dt[t])
        if not np.isnan(y[t]):
            f, q = F[t] @ m, F[t] @ C @ F[t] + V
            e = y[t] - f
            ll += -ld(0.5) * np.log(2 * np.pi * q) - ld(0.5) * e * e / q          # (np.pi is a double: 1e-16 relative on one term of many)
            K = C @ F[t] / q
            m, C = m + K * e, C - np.outer(K, K) * q
        ms[t], Cs[t] = m, C
    return ms, Cs, ll


# ---- B.2 and B.3: replicas of one series ---------------------------------------------------------------------------------------------------------
REPLICAS, B_P = 1024, 128
INFORMATIVE_V, DIFFUSE_V = 1.0, 50.0
SIGMAS, TOP_SHARE, SEPARATION = 5.0, 0.02, 20.0
PURE_N, PURE_P = 16, 1024


@functools.lru_cache(maxsize=None)
def b_inputs(d, diffuse, diagonal):
    """One series of model(d) in a setting, shared parameters: the arrays without the replication.  diagonal: the W of k_lw."""
    m = model(d)
    rng = np.random.default_rng([9100, d, int(diffuse)])
    V = DIFFUSE_V if diffuse else INFORMATIVE_V
    y, _ = simulate_series(m, V, m["W"], m["m0"], m["C0"], rng)
    W = np.diag(np.diag(m["W"])) if diagonal else m["W"]
    return dict(F=m["F"], G=m["G"], g_index=m["g_index"], dt=m["dt"], V=V, W=W, m0=m["m0"], C0=m["C0"], y=y)


def b2_args(kernel, d, diffuse, replicas=REPLICAS, mutant=None):
    """pf_restatement.run's ("pf") or lw_restatement.run's ("lw": a = 1, every prior sd 0, V known) arguments for R replicas"""
    a = dict(b_inputs(d, diffuse, kernel == "lw"))
    if mutant:
        a = mutated(a, mutant)
    kw = dict(a, y=np.tile(a["y"], (replicas, 1)), family=pr.GAUSSIAN, P=B_P, n0=-1, literal=False, nu=None, seed=11, series_offset=0, iteration=0)
    if kernel == "lw":
        kw.update(a=1.0, learn_v=False, prior_v=None, prior_w=np.stack([np.log(np.diag(a["W"])), np.zeros(d)], axis=1))
    return kw


@functools.lru_cache(maxsize=None)
def b2_exact(kernel, d, diffuse):
    """(the Kalman filtered means [T][d], the exact log-likelihood) of the setting's series under the TRUE inputs"""
    a = b_inputs(d, diffuse, kernel == "lw")
    return pr.kalman(a["F"], a["G"], a["g_index"], a["dt"], a["V"], a["W"], a["m0"], a["C0"], a["y"])


def likelihood_figures(ll_hat, ll):
    """(mean of exp(ll_hat - ll), its standard error from the sample, the largest ratio's share of the sum)"""
    r = np.exp(np.asarray(ll_hat) - ll)
    return float(r.mean()), float(r.std(ddof=1) / np.sqrt(r.size)), float(r.max() / r.sum())


def likelihood_misses(ll_hat, ll):
    """the bounds of the informative setting that a run misses (an empty list: it holds them)"""
    m, se, top = likelihood_figures(ll_hat, ll)
    return [f"mean ratio {m:.4f} is {abs(m - 1.0) / se:.1f} se from 1"] * (not abs(m - 1.0) <= SIGMAS * se) + \
           [f"top share {top:.4f}"] * (not top < TOP_SHARE)


def blind_means(d, diffuse, diagonal):
    """the means of the cloud WITHOUT its weights: the Kalman prediction recursion of the same series (no update)"""
    a = dict(b_inputs(d, diffuse, diagonal))
    return rc.kalman_moments(dict(a, y=np.full((1, T), np.nan)))[0]


def means_figures(kernel, d, diffuse, means):
    """(the largest |replica average - Kalman mean| over (t, k) in standard errors of that average, the largest distance of the Kalman mean
    from the unweighted cloud's mean in the same standard errors)"""
    ms, _ = b2_exact(kernel, d, diffuse)
    means = np.asarray(means)
    se = means.std(axis=0, ddof=1) / np.sqrt(means.shape[0])
    return float((np.abs(means.mean(axis=0) - ms) / se).max()), float((np.abs(ms - blind_means(d, diffuse, kernel == "lw")) / se).max())


def means_misses(kernel, d, diffuse, means):
    z, sep = means_figures(kernel, d, diffuse, means)
    return [f"a filtering mean is {z:.1f} se from the Kalman mean"] * (not z <= SIGMAS) + \
           [f"the Kalman means are only {sep:.1f} se from the unweighted cloud's"] * (not sep >= SEPARATION)


def b3_args(d, mutant=None):
    """pff_restatement.simulate's arguments (and through pff_cases.forecast_run the engine's) of the pure forecast: the informative
    setting's model, every y missing, PURE_N series of PURE_P particles"""
    a = dict(b_inputs(d, False, False))
    if mutant:
        a = mutated(a, mutant)
    return dict(a, y=np.full((PURE_N, T), np.nan), family=pr.GAUSSIAN, P=PURE_P, literal=False, nu=None, seed=12, series_offset=0, iteration=0)


def simulate_args(kw):
    keys = ("F", "G", "g_index", "dt", "V", "W", "m0", "C0", "family", "P", "nu", "seed", "series_offset", "iteration")
    return dict({k: kw[k] for k in keys}, H=T, N=kw["y"].shape[0])


@functools.lru_cache(maxsize=None)
def predictive_law(d):
    """(F_t^T a_t [T], q_t = F_t^T R_t F_t + V [T]) from the Kalman prediction recursion under the TRUE inputs"""
    a = dict(b_inputs(d, False, False))
    ms, Cs, _ = rc.kalman_moments(dict(a, y=np.full((1, T), np.nan)))
    return np.einsum("td,td->t", a["F"], ms), np.einsum("td,tde,te->t", a["F"], Cs, a["F"]) + a["V"]


def draws_figures(d, draws):
    """(|sample mean - F^T a| / sqrt(q / n), |sample variance - q| / (q sqrt(2 / (n - 1)))), each [T], n = every draw of a step"""
    f, q = predictive_law(d)
    x = np.asarray(draws).transpose(1, 0, 2).reshape(T, -1)
    n = x.shape[1]
    return np.abs(x.mean(axis=1) - f) / np.sqrt(q / n), np.abs(x.var(axis=1, ddof=1) - q) / (q * np.sqrt(2.0 / (n - 1)))


def draws_misses(d, draws):
    zm, zv = draws_figures(d, draws)
    return [f"the draws' mean at t = {int(zm.argmax())} is {zm.max():.1f} se off"] * (not zm.max() <= SIGMAS) + \
           [f"the draws' variance at t = {int(zv.argmax())} is {zv.max():.1f} se off"] * (not zv.max() <= SIGMAS)


# ---- the mutants ---------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("G-transposed", "g_index-one-step-late", "dt-of-the-next-step", "F-of-the-step-before", "LtL-for-LLt", "last-noise-dropped", "W-for-W-dt")
LAST_NOISE = 1e-6          # the last column of chol(W) times this and not 0: the factorisation of a singular W stops with NOT_PD


def mutated(a, mutant):
    """The inputs of a restatement under one misreading of the model"""
    a = dict(a)
    L = np.linalg.cholesky(a["W"])
    if mutant == "G-transposed":
        a["G"] = np.ascontiguousarray(np.swapaxes(a["G"], 1, 2))
    elif mutant == "g_index-one-step-late":
        a["g_index"] = np.concatenate([a["g_index"][:1], a["g_index"][:-1]])
    elif mutant == "dt-of-the-next-step":
        a["dt"] = np.concatenate([a["dt"][1:], a["dt"][-2:-1]])
    elif mutant == "F-of-the-step-before":
        a["F"] = np.concatenate([a["F"][:1], a["F"][:-1]])
    elif mutant == "LtL-for-LLt":
        a["W"] = L.T @ L
    elif mutant == "last-noise-dropped":
        k = np.ones(L.shape[0]); k[-1] = LAST_NOISE
        a["W"] = (L * k) @ L.T
    elif mutant == "W-for-W-dt":
        a["dt"] = np.where(a["dt"] != 0.0, 1.0, 0.0)
    else:
        raise KeyError(mutant)
    return a


# ---- B.4: the Kalman smoother of model(d) --------------------------------------------------------------------------------------------------------
PG_DIMS = (5, 9, 16)


def smoother(a):
    """The Kalman filter and the Rauch-Tung-Striebel smoother of one series on the particle kernels' conventions (dt == 0: no advance, x_{t+1} IS
    x_t; record 0 the prior): means s [T+1][d], covariances S [T+1][d][d], the lag-one cross-covariances Cov(x_t, x_{t+1} | y) = J_t S_{t+1}
    [T][d][d], J_t = C_t G_t^T R_{t+1}^-1 (the identity where dt == 0), and what backward sampling needs."""
    F, G, gi, dt, y = a["F"], a["G"], a["g_index"], a["dt"], a["y"]
    d = a["m0"].size
    m, C = [np.asarray(a["m0"], dtype=np.float64)], [np.asarray(a["C0"], dtype=np.float64)]
    av, R, J = [None], [None], []
    for t in range(T):
        Gt = G[gi[t]] if dt[t] != 0.0 else np.eye(d)
        at, Rt = Gt @ m[t], Gt @ C[t] @ Gt.T + a["W"] * dt[t]
        J.append(np.eye(d) if dt[t] == 0.0 else np.linalg.solve(Rt, Gt @ C[t]).T)
        av.append(at); R.append(Rt)
        if np.isnan(y[t]):
            m.append(at); C.append(Rt)
        else:
            q = F[t] @ Rt @ F[t] + a["V"]
            K = Rt @ F[t] / q
            m.append(at + K * (y[t] - F[t] @ at)); C.append(Rt - np.outer(K, K) * q)
    s, S = [None] * (T + 1), [None] * (T + 1)
    s[T], S[T] = m[T], C[T]
    for t in range(T - 1, -1, -1):
        s[t] = m[t] + J[t] @ (s[t + 1] - av[t + 1])
        S[t] = C[t] + J[t] @ (S[t + 1] - R[t + 1]) @ J[t].T
    S = np.stack(S)
    return dict(mean=np.stack(s), cov=S, cross=np.stack([J[t] @ S[t + 1] for t in range(T)]), m=m, C=C, a=av, R=R, J=J)


@functools.lru_cache(maxsize=None)
def pg_case(d):
    """model(d) at the informative setting with pg_checks' N replicas of one series: the arrays pg_cases.engine_run and pg_restatement.run take
    (the reference paths are exact draws of the smoothing law, by backward sampling on the host) and the smoother's moments."""
    import pg_checks as ck
    a = dict(b_inputs(d, False, False))
    sm = smoother(a)
    rng = np.random.default_rng([9200, d])
    N = ck.N

    def root(M):
        w, v = np.linalg.eigh(0.5 * (M + M.T))
        return v * np.sqrt(np.clip(w, 0.0, None))

    path = np.empty((N, T + 1, d))
    path[:, T] = sm["m"][T] + rng.standard_normal((N, d)) @ root(sm["C"][T]).T
    for t in range(T - 1, -1, -1):
        if a["dt"][t] == 0.0:
            path[:, t] = path[:, t + 1]
            continue
        Jt = sm["J"][t]
        cond = sm["C"][t] - Jt @ sm["R"][t + 1] @ Jt.T
        path[:, t] = sm["m"][t] + (path[:, t + 1] - sm["a"][t + 1]) @ Jt.T + rng.standard_normal((N, d)) @ root(cond).T
    kw = dict(a, y=np.tile(a["y"], (N, 1)), nu=None, family=pr.GAUSSIAN, P=ck.P, ancestor_sampling=True, seed=ck.SEED + 50 + d, series_offset=0, iteration=0)
    return dict(kw=kw, start=path, mean=sm["mean"], cov=sm["cov"], cross=sm["cross"])


def smoother_z(d, path):
    """pg_checks.gaussian_z on pg_case(d): the largest |sample - exact| in standard errors of (means, variances, lag-one cross-covariances).  A
    record behind a step with dt = 0 repeats the one before it and is counted once."""
    c = pg_case(d)
    x = np.asarray(path)
    n = x.shape[0]
    var = np.diagonal(c["cov"], axis1=1, axis2=2)
    xc = x - x.mean(axis=0)
    z_mean = np.abs(x.mean(axis=0) - c["mean"]) / np.sqrt(var / n)
    z_var = np.abs(x.var(axis=0, ddof=1) - var) / (var * np.sqrt(2.0 / n))
    sc = np.einsum("nti,ntj->tij", xc[:, :-1], xc[:, 1:]) / (n - 1)
    se = np.sqrt((var[:-1, :, None] * var[1:, None, :] + c["cross"] ** 2) / n)
    return float(z_mean.max()), float(z_var.max()), float((np.abs(sc - c["cross"]) / se).max())
