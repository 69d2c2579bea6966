"""The draws of every sampler against the dense joint posterior of the whole path (tests/test_joint_posterior_host.py, _gpu.py).

With injected normals every sampler of the engine is affine in them, theta = s + L z: s must be the smoothing mean of the stacked
path (x_0 .. x_T) and L L^T its full (T+1)d x (T+1)d smoothing covariance, cross-time blocks included -- whatever factor the draw
uses (Cholesky, eigen, SVD, simulate-and-correct).  `dense_posterior` obtains both by conditioning ONE big Gaussian with dense
linear algebra in 50 significant digits (Python's decimal module): no filter, no backward recursion, nothing a kernel and its
restatement in the oracle could share.  `affine_map` reads (s, L) off one batched call, `measure` compares.

The model, stated once.  x_0 ~ N(m0, C0); x_t = G_t x_{t-1} + b_t + w_t, Var w_t = Q_t; y_t = F_t^T x_t + v_t, Var v_t = V_t; a NaN
component of y_t drops its row of F_t^T and its row and column of V_t.
  DLM    G_t = the materialised table entry g_index[t], Q_t = W_t dt_t (W_t: the stream entry of the transition INTO observation t,
         or the shared W), b_t = 0.  dt_t = 0 means NO ADVANCE (G_t = I, Q_t = 0), as the reference's forward pass has it
         (KalmanFilter.scala:279-280): for a model whose g(0) is not the identity the reference's backward passes deviate from
         this posterior, which the host test pins.
  AR(1)  x_0 ~ N(mu, sigma^2 / (1 - phi^2)), x_t - mu = phi (x_{t-1} - mu) + eta_t, Var eta_t = sigma^2.
  OU     the literal reference form (FilterOu.scala:34-46): c0 = sigma^2, the initial state at times[0] (the first dt = 0),
         phi_t = exp(-phi dt_t), Q_t = sigma^2 (1 - exp(-2 phi dt_t)) / (2 phi).
Prior mean mu and covariance P of the stacked path by the block recursion, H and R = blockdiag(V_t^obs) from the observed
components, then  S = H P H^T + R,  mean = mu + P H^T S^-1 (y - H mu),  cov = P - P H^T S^-1 H P,  loglik = log N(y; H mu, S).
Inputs are the doubles the engine receives, converted exactly.

Run as a script the module prints the case table."""
import os
import sys
from decimal import Decimal, getcontext

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import oracle  # noqa: E402
from bayesian_dlms_amd import _lib  # noqa: E402
from bayesian_dlms_amd.dlm import Dlm, DlmParameters, materialise  # noqa: E402

PREC = 50
_ZERO = Decimal(0)
_LOG_2PI = None


def _dec(x):
    return x if isinstance(x, Decimal) else Decimal(float(x))      # Decimal(float) is exact


def _mat(a):
    """2-D array (of doubles or Decimals) -> list of rows of Decimals."""
    return [[_dec(v) for v in row] for row in a]


def _mm(A, B):
    Bt = list(zip(*B))
    return [[sum((a * b for a, b in zip(row, col) if a and b), _ZERO) for col in Bt] for row in A]


def dense_posterior(m0, C0, G, Q, F, V, y, b=None):
    """(mean [(T+1)d], cov [(T+1)d][(T+1)d], loglik) of the stacked path given y [T][p] (NaN = missing), rounded to doubles from
    50-digit arithmetic.  G, Q, F, V: one matrix per step t = 0 .. T-1 (G_t d x d, Q_t d x d, F_t d x p used as F_t^T, V_t p x p),
    b: one offset vector per step or None.  Entries may be doubles (taken exactly) or Decimals."""
    global _LOG_2PI
    getcontext().prec = PREC
    if _LOG_2PI is None:      # pi by Machin's formula: decimal has no constant
        def atan_inv(k):
            x = Decimal(1) / k; s, term, n, x2 = x, x, 1, x * x
            while abs(term) > Decimal(10) ** -(PREC + 5):
                term = -term * x2; n += 2; s += term / n
            return s
        getcontext().prec = PREC + 10
        pi = 4 * (4 * atan_inv(5) - atan_inv(239))
        _LOG_2PI = (2 * pi).ln()
        getcontext().prec = PREC
    T = len(G)
    d = len(m0)
    n = (T + 1) * d
    mu = [_dec(v) for v in m0]
    P = [[_ZERO] * n for _ in range(n)]
    C0 = _mat(C0)
    for i in range(d):
        P[i][:d] = C0[i]
    for t in range(T):            # mu_t = G mu_{t-1} + b;  P[t][s] = G P[t-1][s] (s < t),  P[t][t] = G P[t-1][t-1] G^T + Q
        Gt, Qt = _mat(G[t]), _mat(Q[t])
        lo, hi = t * d, (t + 1) * d
        prev = mu[lo:hi]
        bt = [_ZERO] * d if b is None else [_dec(v) for v in b[t]]
        mu += [sum((g * m for g, m in zip(row, prev)), bt[i]) for i, row in enumerate(Gt)]
        rows = _mm(Gt, [P[k][:hi] for k in range(lo, hi)])           # d x hi: covariances with everything up to t-1
        diag = _mm([r[lo:hi] for r in rows], [list(c) for c in zip(*Gt)])
        for i in range(d):
            P[hi + i][:hi] = rows[i]
            for j in range(d):
                P[hi + i][hi + j] = diag[i][j] + Qt[i][j]
            for k in range(hi):
                P[k][hi + i] = rows[i][k]
    # observed components: rows of H (as index lists into the stacked state), R, y
    Hrows, yo, blocks = [], [], []
    for t in range(T):
        Ft = _mat(F[t])
        obs = [j for j in range(len(Ft[0])) if y[t][j] == y[t][j]]
        blocks.append((len(Hrows), obs, _mat(V[t])))
        for j in obs:
            Hrows.append(((t + 1) * d, [Ft[i][j] for i in range(d)]))
            yo.append(_dec(y[t][j]))
    no = len(Hrows)
    HP = [[sum((f * P[off + i][k] for i, f in enumerate(col) if f), _ZERO) for k in range(n)] for off, col in Hrows]     # no x n
    S = [[sum((f * HP[a][off + i] for i, f in enumerate(col) if f), _ZERO) for off, col in Hrows] for a in range(no)]
    for start, obs, Vt in blocks:
        for a, ja in enumerate(obs):
            for c, jc in enumerate(obs):
                S[start + a][start + c] += Vt[ja][jc]
    r = [yo[a] - sum((f * mu[off + i] for i, f in enumerate(col)), _ZERO) for a, (off, col) in enumerate(Hrows)]
    L = [[_ZERO] * no for _ in range(no)]       # S = L L^T
    for j in range(no):
        L[j][j] = (S[j][j] - sum((v * v for v in L[j][:j]), _ZERO)).sqrt()
        for i in range(j + 1, no):
            L[i][j] = (S[i][j] - sum((u * v for u, v in zip(L[i][:j], L[j][:j])), _ZERO)) / L[j][j]
    X, w = [], []                               # X = L^-1 H P (no x n), w = L^-1 r
    for a in range(no):
        row = HP[a]
        for c in range(a):
            lac = L[a][c]
            if lac:
                row = [u - lac * v for u, v in zip(row, X[c])]
        X.append([u / L[a][a] for u in row])
        w.append((r[a] - sum((L[a][c] * w[c] for c in range(a)), _ZERO)) / L[a][a])
    Xt = list(zip(*X)) if no else [()] * n
    mean = [mu[k] + sum((u * v for u, v in zip(Xt[k], w)), _ZERO) for k in range(n)]
    cov = np.empty((n, n))
    for k in range(n):
        for l in range(k + 1):
            cov[k, l] = cov[l, k] = float(P[k][l] - sum((u * v for u, v in zip(Xt[k], Xt[l])), _ZERO))
    ll = -(no * _LOG_2PI + 2 * sum((L[j][j].ln() for j in range(no)), _ZERO) + sum((v * v for v in w), _ZERO)) / 2
    return np.array([float(v) for v in mean]), cov, float(ll)


def dlm_posterior(mat, p, y):
    """dense_posterior of a materialised DLM with its parameters (V / W possibly [T] streams); y [T][p]."""
    d, q, T = mat.d, mat.p, mat.T
    eye, zero = np.eye(d), np.zeros((d, d))
    G, Q, F, V = [], [], [], []
    for t in range(T):
        dt = 1.0 if mat.dt is None else float(mat.dt[t])
        gi = 0 if mat.g_index is None else int(mat.g_index[t])
        W = p.w[t] if p.w.ndim == 3 else p.w
        if dt == 0.0:
            G.append(eye); Q.append(zero)
        else:
            G.append(oracle.from_cm(mat.G[gi * d * d:(gi + 1) * d * d], d, d))
            Q.append([[_dec(v) * _dec(dt) for v in row] for row in W])
        F.append(oracle.from_cm(mat.F[t * mat.f_stride:t * mat.f_stride + d * q], d, q))
        V.append(p.v[t] if p.v.ndim == 3 else p.v)
    return dense_posterior(p.m0, p.c0, G, Q, F, V, np.asarray(y, dtype=np.float64).reshape(T, q))


def ar1_posterior(y, v, phi, mu, sigma):
    getcontext().prec = PREC
    T = len(y)
    ph, m, s2 = _dec(phi), _dec(mu), _dec(sigma) * _dec(sigma)
    return dense_posterior([m], [[s2 / (1 - ph * ph)]], [[[ph]]] * T, [[[s2]]] * T, [[[1.0]]] * T, [[[vt]] for vt in v],
                           np.asarray(y, dtype=np.float64).reshape(T, 1), b=[[m * (1 - ph)]] * T)


def ou_posterior(times, y, v, phi, mu, sigma):
    getcontext().prec = PREC
    T = len(y)
    ph, m, s2 = _dec(phi), _dec(mu), _dec(sigma) * _dec(sigma)
    G, Q, b = [], [], []
    for t in range(T):
        dt = _dec(times[t]) - _dec(times[t - 1] if t else times[0])
        e = (-ph * dt).exp()
        G.append([[e]]); Q.append([[s2 * (1 - (-2 * ph * dt).exp()) / (2 * ph)]]); b.append([m * (1 - e)])
    return dense_posterior([m], [[s2]], G, Q, [[[1.0]]] * T, [[[vt]] for vt in v], np.asarray(y, dtype=np.float64).reshape(T, 1), b=b)


def affine_map(draw, n_normals):
    """(s, L) of theta = s + L z from ONE batched call: draw(z [n_normals + 1][n_normals]) -> theta [n_normals + 1][n_state], the
    series sharing y and all parameters; row 0 of z is zero, row j + 1 the j-th unit vector."""
    z = np.zeros((n_normals + 1, n_normals))
    z[np.arange(1, n_normals + 1), np.arange(n_normals)] = 1.0
    theta = np.asarray(draw(z), dtype=np.float64).reshape(n_normals + 1, -1)
    return theta[0].copy(), (theta[1:] - theta[0]).T.copy()


def measure(s, L, mean, cov):
    """(e_mean, e_cov): max |s - mean| / max(1, max |mean|) and max |L L^T - cov| / max |cov|."""
    return (float(np.abs(s - mean).max() / max(1.0, np.abs(mean).max())),
            float(np.abs(L @ L.T - cov).max() / np.abs(cov).max()))


# ---- the oracle's constructions of the draws ---------------------------------------------------------------------------------
def omodel(mat):
    return oracle.Model(mat.d, mat.p, mat.T, mat.F, mat.G, mat.g_index, mat.dt, mat.f_stride)


def dk_reference_draw(mat, p, y, z):
    """theta = E[x | y - y+] + x+ with (x+, y+) simulated from z [T+1][d+1]; smoothing by the oracle.  p.w / p.v may be [T] streams
    (W_t drives the transition into record t, V_t observation t)."""
    d, T = mat.d, mat.T
    G = oracle.from_cm(mat.G[: d * d], d, d); F = mat.F[:d]
    Lc = np.linalg.cholesky(p.c0)
    Lws = [np.linalg.cholesky(w) for w in p.w] if p.w.ndim == 3 else [np.linalg.cholesky(p.w)] * T
    svs = [np.sqrt(v[0, 0]) for v in p.v] if p.v.ndim == 3 else [np.sqrt(p.v[0, 0])] * T
    x = p.m0 + Lc @ z[0, :d]
    xs, yp = [x], np.empty((T, 1))
    for t in range(1, T + 1):
        x = G @ x + Lws[t - 1] @ z[t, :d]
        xs.append(x)
        yp[t - 1, 0] = F @ x + svs[t - 1] * z[t, d]
    om = omodel(mat)
    f = oracle.kf_filter(om, p.v, p.w, np.zeros(d), p.c0, y - yp)      # zero prior mean
    s = oracle.smoother(om, f, compat_q1=False)
    return s["s"] + np.array(xs)


def dk_reference_draw_mv(mat, p, y, z):
    """Multivariate version of dk_reference_draw: z [T+1][d+p] (state noise, then observation noise)."""
    d, q, T = mat.d, mat.p, mat.T
    G = oracle.from_cm(mat.G[: d * d], d, d); F = oracle.from_cm(mat.F[: d * q], d, q)
    Lc, Lv = np.linalg.cholesky(p.c0), np.linalg.cholesky(p.v)
    Lws = [np.linalg.cholesky(w) for w in p.w] if p.w.ndim == 3 else [np.linalg.cholesky(p.w)] * T     # (a W_t stream: W_t drives the transition into record t)
    x = p.m0 + Lc @ z[0, :d]
    xs, yp = [x], np.empty((T, q))
    for t in range(1, T + 1):
        x = G @ x + Lws[t - 1] @ z[t, :d]
        xs.append(x)
        yp[t - 1] = F.T @ x + Lv @ z[t, d:]
    om = omodel(mat)
    f = oracle.kf_filter(om, p.v, p.w, np.zeros(d), p.c0, y - yp)
    s = oracle.smoother(om, f, compat_q1=False)
    return s["s"] + np.array(xs)


# ---- the case table ----------------------------------------------------------------------------------------------------------
W_C2 = np.array([0.01, 0.2, 0.4, 0.5, 0.2, 0.1, 0.4, 0.2, 0.4, 0.5, 0.2, 0.1, 0.4])


class Case:
    """One named case.  kind: "ffbs" (reference-form sampler; flags may hold DLM_OPT_DRAW_EIG), "simsmooth", "svd", "ar1", "ou".
    DLM kinds: mat, p, y [T][p].  AR(1)/OU: y [T], v [T], sv = (phi, mu, sigma), times (OU).  route: what Engine.last_variant must
    report.  per_series: "v" / "sv" passes the AR(1) variance stream / parameters once per series (replicated, non-zero
    strides).  entry: "ffbs", "no_filt" (filt_ws not requested) or "records" (dlm_backward_sample_batch on the records
    of Engine.filter).  device: also run with device tensors.  own: on a shared-factor route, whether every series
    (True) or none (False) must have computed its own factors (dlm_last_counters under DLM_OPT_COUNT_STEPS)."""

    def __init__(self, name, kind, route, *, mat=None, p=None, y=None, flags=0, per_series=None, entry="ffbs", device=False,
                 v=None, sv=None, times=None, own=None):
        self.name, self.kind, self.route, self.mat, self.p, self.flags = name, kind, route, mat, p, flags
        self.y = np.asarray(y, dtype=np.float64)
        self.per_series, self.entry, self.device, self.v, self.sv, self.times, self.own = per_series, entry, device, v, sv, times, own
        self._ref = None

    @property
    def n_state(self):
        return (self.mat.T + 1) * self.mat.d if self.mat is not None else self.y.size + 1

    @property
    def n_normals(self):
        if self.kind == "simsmooth":
            return (self.mat.T + 1) * (self.mat.d + self.mat.p)
        return self.n_state

    def reference(self):
        """(mean, cov, loglik) in 50 digits; computed once, shared by the tests, never written to."""
        if self._ref is None:
            if self.kind == "ar1":
                ref = ar1_posterior(self.y, self.v, *self.sv)
            elif self.kind == "ou":
                ref = ou_posterior(self.times, self.y, self.v, *self.sv)
            else:
                ref = dlm_posterior(self.mat, self.p, self.y)
            for a in ref[:2]:
                a.setflags(write=False)
            self._ref = ref
        return self._ref

    def oracle_draw(self, factor=None):
        """The oracle's construction of this case's draw: a function z [N][n_normals] -> theta [N][n_state] for affine_map."""
        if self.kind in ("ar1", "ou"):
            phi = self.sv[0]
            if self.kind == "ar1":
                f = oracle.ar1_filter(self.y, self.v, *self.sv)
                return lambda z: np.stack([oracle.ar1_backward_sample(f, phi, zn) for zn in z])
            f = oracle.ou_filter(self.times, self.y, self.v, *self.sv)
            return lambda z: np.stack([oracle.ou_backward_sample(self.times, f, phi, zn) for zn in z])
        mat, p, y = self.mat, self.p, self.y
        d, q, T = mat.d, mat.p, mat.T
        om = omodel(mat)
        if self.kind == "simsmooth":
            dk = dk_reference_draw if q == 1 else dk_reference_draw_mv
            return lambda z: np.stack([dk(mat, p, y, zn.reshape(T + 1, d + q)).reshape(-1) for zn in z])
        if self.kind == "svd":
            sf = oracle.svd_filter(om, p.v, p.w, p.m0, p.c0, y)
            lit = bool(self.flags & _lib.OPT_SVD_SAMPLER_Q9)
            return lambda z: np.stack([oracle.svd_backward_sample(om, p.w, sf, zn, literal_q9=lit)["theta"].reshape(-1) for zn in z])
        f = oracle.kf_filter(om, p.v, p.w, p.m0, p.c0, y)
        factor = factor or ("eig" if self.flags & _lib.OPT_DRAW_EIG else "chol")
        return lambda z: np.stack([oracle.backward_sample(om, p.w, f, zn, factor=factor)["theta"].reshape(-1) for zn in z])


def c2(T, times=None):
    mat = materialise(Dlm.polynomial(1) + Dlm.seasonal(24, 6), np.arange(1, T + 1, dtype=np.float64) if times is None else times)
    rng = np.random.default_rng(1302)
    A, B = rng.standard_normal((13, 13)), rng.standard_normal((13, 13))
    return mat, DlmParameters([[1.0]], np.diag(W_C2) + A @ A.T / 26, rng.standard_normal(13), B @ B.T / 13 + 0.5 * np.eye(13))


def block_model(nblk, T, per=2, seed=0):
    """_block_model of tests/test_engine_gpu.py: |*| of nblk polynomial(per) models, dense V and W."""
    mod = Dlm.polynomial(per)
    for _ in range(nblk - 1):
        mod = mod * Dlm.polynomial(per)
    mat = materialise(mod, np.arange(1, T + 1, dtype=np.float64))
    d, q = mat.d, mat.p
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((d, d)); B = rng.standard_normal((q, q))
    return mat, DlmParameters(B @ B.T / q + 0.5 * np.eye(q), A @ A.T / d + 0.1 * np.eye(d), rng.standard_normal(d) * 0.1,
                              np.diag(np.linspace(0.5, 2.0, d)))


def _spd_stream(rng, T, n, scale=0.3, lo=0.05, hi=0.5):
    out = np.empty((T, n, n))
    for t in range(T):
        A = rng.standard_normal((n, n)) * scale
        out[t] = A @ A.T + np.diag(rng.uniform(lo, hi, n))
    return out


def _walk(rng, T, q):
    return rng.standard_normal((T, q)).cumsum(axis=0)


def _build_cases():
    cases = []
    add = lambda *a, **kw: cases.append(Case(*a, **kw))
    S, E = _lib.OPT_FFBS_SIMSMOOTH, _lib.OPT_DRAW_EIG

    # scalar and d = 2 models: one lane per series
    rng = np.random.default_rng(101)
    mat = materialise(Dlm.polynomial(1), np.arange(1, 18, dtype=np.float64))
    y = _walk(rng, 17, 1); y[0] = y[16] = np.nan
    add("local_level_T17_ends_missing", "ffbs", "lane-sampler", mat=mat, p=DlmParameters([[2.0]], [[3.0]], [0.5], [[10.0]]), y=y)
    rng = np.random.default_rng(102)
    poly2 = DlmParameters([[1.3]], np.array([[0.5, 0.1], [0.1, 0.2]]), [0.3, -0.2], np.array([[4.0, 0.5], [0.5, 2.0]]))
    mat = materialise(Dlm.polynomial(2), np.cumsum([1.0, 2.0, 0.5, 1.0, 3.0, 1.0, 0.25, 2.0, 1.0]))
    add("poly2_T9_irregular", "ffbs", "lane-sampler", mat=mat, p=poly2, y=_walk(rng, 9, 1))

    # the c2 model, dense W and C0: every route of the reference-form sampler for d <= 15, p = 1
    rng = np.random.default_rng(103)
    mat, p = c2(4)
    yc2 = _walk(rng, 4, 1)
    y = yc2
    ygap = y.copy(); ygap[1] = np.nan
    add("c2_T4", "ffbs", "sparse16-sampler-shared", mat=mat, p=p, y=y, device=True, own=False)
    add("c2_T4_per_series", "ffbs", "sparse16-sampler", mat=mat, p=p, y=y, flags=_lib.OPT_SAMPLER_PER_SERIES)
    add("c2_T4_gap", "ffbs", "sparse16-sampler-shared", mat=mat, p=p, y=ygap, own=True)      # (the route of the call: every series has the gap)
    add("c2_T4_generic", "ffbs", "generic", mat=mat, p=p, y=y, flags=_lib.OPT_NO_SAMPLER16)
    add("c2_T4_eig", "ffbs", "generic-eig", mat=mat, p=p, y=y, flags=E)
    add("c2_T4_no_filter_records", "ffbs", "sparse16-sampler-shared", mat=mat, p=p, y=y, entry="no_filt")
    add("c2_T4_from_filter_records", "ffbs", "sparse16-sampler", mat=mat, p=p, y=y, entry="records")
    matr, _ = c2(5, times=np.array([1.0, 2.0, 3.0, 3.0, 4.0]))
    add("c2_T5_repeated_time", "ffbs", "sparse16-sampler", mat=matr, p=p, y=_walk(rng, 5, 1))

    # a dense G (the model of test_ffbs_with_the_references_eigen_factor)
    rng = np.random.default_rng(104)
    A = rng.standard_normal((9, 9)); G1 = 0.9 * A / np.abs(np.linalg.eigvals(A)).max()
    F9 = rng.standard_normal((9, 2)); A2 = rng.standard_normal((9, 9))
    mat = materialise(Dlm(lambda t: F9, lambda dt: G1), np.arange(1, 6, dtype=np.float64))
    p = DlmParameters(np.eye(2) * 0.8, A2 @ A2.T / 9 + 0.2 * np.eye(9), rng.standard_normal(9), np.eye(9) + 0.1 * A2 @ A2.T)
    add("dense_d9_p2_T5", "ffbs", "generic", mat=mat, p=p, y=_walk(rng, 5, 2))

    # small multivariate: time-varying F, V_t and W_t streams, a partially and a fully missing step
    rng = np.random.default_rng(105)
    three = Dlm.polynomial(2) * Dlm.polynomial(2) * Dlm.polynomial(2)
    mat = materialise(Dlm(lambda t: three.f(t) * (1.0 + 0.125 * t), three.g), np.arange(1, 6, dtype=np.float64))
    B = rng.standard_normal((3, 3)); Vb = B @ B.T / 3 + 0.5 * np.eye(3)
    p = DlmParameters(np.stack([Vb * s for s in rng.uniform(0.3, 3.0, 5)]), _spd_stream(rng, 5, 6), rng.standard_normal(6),
                      np.eye(6) * 1.5)
    y = _walk(rng, 5, 3); y[1, 1] = np.nan; y[3, :] = np.nan
    add("d6_p3_T5_tv_F_V_W", "ffbs", "sparse16-sampler", mat=mat, p=p, y=y)

    # 16 <= d <= 48: per-wave (shared factors and per series), workgroup, and the register-tile shapes
    rng = np.random.default_rng(106)
    mat, p = block_model(10, 3, 2, seed=10)
    y = _walk(rng, 3, 10)
    add("blocks_d20_p10_T3_wave_shared", "ffbs", "wave-sampler-shared", mat=mat, p=p, y=y, flags=_lib.OPT_FORCE_WAVE)
    add("blocks_d20_p10_T3_wave", "ffbs", "wave-sampler", mat=mat, p=p, y=y, flags=_lib.OPT_FORCE_WAVE | _lib.OPT_SAMPLER_PER_SERIES)
    add("blocks_d20_p10_T3_workgroup", "ffbs", "generic", mat=mat, p=p, y=y, flags=_lib.OPT_NO_WAVE)     # (no workgroup form of the sampler)
    mat, p = block_model(20, 1, 2, seed=20)
    add("blocks_d40_p20_T1", "ffbs", "wave-sampler-shared", mat=mat, p=p, y=_walk(rng, 1, 20))
    rng = np.random.default_rng(107)
    mod = Dlm.polynomial(2)
    for _ in range(15):
        mod = mod * Dlm.polynomial(2)
    mat = materialise(mod * Dlm.polynomial(1), np.arange(1, 3, dtype=np.float64))
    assert (mat.d, mat.p) == (33, 17)
    B = rng.standard_normal((17, 17))
    p = DlmParameters(B @ B.T / 17 + 0.5 * np.eye(17), _spd_stream(rng, 2, 33, scale=0.15), rng.standard_normal(33) * 0.1,
                      np.diag(np.linspace(0.5, 2.0, 33)))
    add("d33_p17_T2_W_stream", "ffbs", "wave-sampler", mat=mat, p=p, y=_walk(rng, 2, 17), flags=_lib.OPT_FORCE_WAVE)

    # the simulation smoother
    rng = np.random.default_rng(108)
    mat = materialise(Dlm.polynomial(2), np.arange(1, 10, dtype=np.float64))
    add("simsmooth_poly2_T9", "simsmooth", "lane-simsmooth", mat=mat, p=poly2, y=_walk(rng, 9, 1), flags=S)
    mat, p = c2(4)
    ps = DlmParameters(rng.uniform(0.5, 2.0, (4, 1, 1)), _spd_stream(rng, 4, 13), p.m0, p.c0)
    add("simsmooth_c2_T4_streams_gap", "simsmooth", "sparse16-simsmooth", mat=mat, p=ps, y=ygap, flags=S)
    mat, p = block_model(10, 2, 2, seed=11)
    pw = DlmParameters(p.v, _spd_stream(rng, 2, 20, scale=0.2, hi=0.4), p.m0, p.c0)
    add("simsmooth_d20_p10_T2_W_stream", "simsmooth", "wave-simsmooth", mat=mat, p=pw, y=_walk(rng, 2, 10), flags=S | _lib.OPT_FORCE_WAVE)

    # the SVD sampler (corrected mode)
    rng = np.random.default_rng(109)
    mat, p = c2(4)
    add("svd_c2_T4", "svd", "svd-jacobi", mat=mat, p=p, y=yc2)
    mati, _ = c2(4, times=np.cumsum([1.0, 2.0, 0.5, 3.0]))     # an irregular grid: the backward step needs W dt_t (tests/test_gibbs_invariance_gpu.py found it missing)
    add("svd_c2_T4_irregular", "svd", "svd-jacobi", mat=mati, p=p, y=yc2)
    mat, p = block_model(10, 3, 2, seed=12)
    y = _walk(rng, 3, 10); y[1, 4] = np.nan
    add("svd_d20_p10_T3_component_missing", "svd", "svd-jacobi", mat=mat,
        p=DlmParameters(np.diag(np.linspace(1.8, 0.6, 10)), p.w, p.m0, p.c0), y=y)

    # AR(1): the edges of FW_TILE = 16 and AR_TILE = 8 (dlm_ar1.hip); gaps at both ends, a whole backward tile missing at T = 33
    for T in (1, 2, 7, 8, 9, 15, 16, 17, 33):
        for phi in (0.8, -0.95):
            rng = np.random.default_rng(1000 + 2 * T + (phi < 0))
            y = rng.standard_normal(T).cumsum() * 0.3 + 1.0
            if T >= 7:
                y[0] = y[T - 1] = np.nan
                y[T // 2] = np.nan
            if T == 33:
                y[16:24] = np.nan
            add(f"ar1_T{T}_phi{phi}", "ar1", "ar1-lane", y=y, v=rng.uniform(0.2, 2.0, T), sv=(phi, 1.0, 0.3), device=(T == 17 and phi == 0.8))
    rng = np.random.default_rng(1100)
    y = rng.standard_normal(17).cumsum() * 0.3; y[5] = np.nan
    v = rng.uniform(0.2, 2.0, 17)
    add("ar1_T17_sv_per_series", "ar1", "ar1-lane", y=y, v=v, sv=(0.8, 1.0, 0.3), per_series="sv")
    add("ar1_T17_v_per_series", "ar1", "ar1-lane", y=y, v=v, sv=(0.8, 1.0, 0.3), per_series="v")
    for T in (8, 17):
        rng = np.random.default_rng(1200 + T)
        gaps = rng.choice([0.5, 1.0, 2.5], T); gaps[T // 2] = 0.0
        y = rng.standard_normal(T).cumsum() * 0.3; y[T // 2 - 1] = np.nan
        add(f"ou_T{T}_repeated_time", "ou", "ou-lane", y=y, v=rng.uniform(0.2, 2.0, T), sv=(0.4, 0.5, 0.6), times=np.cumsum(gaps) + 1.0)
    return cases


CASES = _build_cases()
CASE_IDS = [c.name for c in CASES]


def _dlm_models():
    """One case per (model, parameters, y): the flags of a case do not reach the filter, the smoother and the log-likelihood."""
    seen, out = set(), []
    for c in CASES:
        key = (id(c.mat), id(c.p), c.y.tobytes())
        if c.mat is not None and key not in seen:
            seen.add(key); out.append(c)
    return out


DLM_MODELS = _dlm_models()


def poly2_repeated_time():
    """polynomial(2) on times 1, 2, 2, 4.5, 5, 9: the case of DESIGN.md 2, Q21 (g(0) != I at a repeated time)."""
    rng = np.random.default_rng(110)
    mat = materialise(Dlm.polynomial(2), np.array([1.0, 2.0, 2.0, 4.5, 5.0, 9.0]))
    p = DlmParameters([[1.3]], np.array([[0.5, 0.1], [0.1, 0.2]]), [0.3, -0.2], np.array([[4.0, 0.5], [0.5, 2.0]]))
    return Case("poly2_repeated_time", "ffbs", "lane-sampler", mat=mat, p=p, y=_walk(rng, 6, 1))


if __name__ == "__main__":
    for c in CASES:
        shape = f"d={c.mat.d} p={c.mat.p} T={c.mat.T}" if c.mat is not None else f"T={c.y.size}"
        print(f"{c.name:40s} {c.kind:10s} {shape:18s} n={c.n_state:4d} normals={c.n_normals:4d} route={c.route}")
