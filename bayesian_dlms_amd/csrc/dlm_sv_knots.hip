// Knot block sampler of the stochastic-volatility state (StochasticVolatilityKnots.sampleBlock / sampleState, StochVolKnots.scala:74-176), one
// sweep over N independent chains in place: the state draw whose invariant law is the posterior of the model itself,
//   y_t = eps_t exp(alpha_t / 2),   alpha_t = mu + phi (alpha_{t-1} - mu) + eta_t,   eta_t ~ N(0, sigma^2),
// not of the seven-component approximation dlm_sv_mixture_batch + dlm_ar1_ffbs_batch target.  alpha rows are [T+1] in the layout of
// dlm_ar1_ffbs_batch's theta: alpha[0] the state before the first observation, state s >= 1 observes y[s-1].
//
// The path is cut at the knots 0 = k_0 < k_1 < ... < k_B = T + 1 (shared by the batch); block i is the states lo..hi = k_i .. k_{i+1} - 1.
// One block:
//   forward    stepUni (FilterAr.scala:17-32) on ystar_s = log y_{s-1}^2 + 1.27 with v = pi^2 / 2 (the Gaussian approximation of
//              log eps^2), from the point mass (alpha[lo-1], 0); lo = 0: from the stationary record (mu, sigma^2 / (1 - phi^2)),
//              which is alpha[0]'s own prior.  The records (m_s, c_s) go to scratch, ystar_s to the proposal's slot.
//   backward   backStepUni (:58-76) from the fixed alpha[hi+1]; hi = T: from a draw of the last filtering distribution.  The proposal
//              alpha'_s replaces ystar_s in its slot.
//   accept     Metropolis.mAccept on exactLl - approxLl:  Delta = sum_{s in block, s >= 1, y_{s-1} observed} [g(alpha'_s) - g(alpha_s)],
//              g(a) = -1/2 (a + y^2 e^{-a}) + (ystar - a)^2 / pi^2;  accepted when log u < Delta, and always when the block observes
//              nothing.  The g(alpha_s) are summed upwards beside the forward pass, the g(alpha'_s) downwards beside the backward pass.
// An observed y whose log y^2 is not finite (y = 0, y^2 underflowing: Q20) is treated as missing in the proposal and in Delta, and the
// series gets DLM_ST_NONFINITE.
//
// Sweep order: red-black.  Given the odd blocks the even blocks are conditionally independent -- each reads alpha[lo-1] and
// alpha[hi+1] only, and those belong to odd blocks -- so the call is k_sv_knots over the even blocks, then over the odd blocks, one
// LANE per (series, block): the grid is (ceil(N / 64), blocks of the parity), a wave's 64 lanes are 64 consecutive series of the SAME
// block (one trip count; they diverge at the accept alone), and a lane streams its own contiguous stretch of y, alpha and scratch as
// k_ar1_ffbs does.  In front of both, k_sv_knots_check (a wave per series) flags the rows that must come back untouched -- a
// non-stationary phi or sigma <= 0 (DLM_ST_NOT_PD), a non-finite alpha anywhere in the row (DLM_ST_NONFINITE): a block's lane sees its
// own stretch only.
//
// Draws: key DLM_KEY_SVKNOT, counter (seed, series_offset + n, iteration, slot): slot s is the normal of state s (draw_normal), the
// acceptance uniform of a block sits at the slot of its first state under which = 1.  Nothing depends on the block-to-wave mapping.
#include "dlm_draws.h"

namespace dlm {

constexpr double SVK_V = 4.934802200544679;          // pi^2 / 2
constexpr double SVK_INV_PI2 = 0.10132118364233778;  // 1 / pi^2
constexpr int SVK_TILE = 4;                          // states per tile (8 costs the second resident wave per SIMD: 255 + 82 registers against 225)

// exactLl - approxLl of one observed state, up to terms free of a
__device__ __forceinline__ double svk_g(double a, double y2, double ystar) {
  const double r = ystar - a;
  return -0.5 * (a + y2 * exp(-a)) + r * r * SVK_INV_PI2;
}

// rowflag[n] = 0, or the flags of a row the sweep leaves alone
__global__ __launch_bounds__(256) void k_sv_knots_check(SvKnotsArgs a) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= a.N) return;   // (whole waves)
  const double* p = a.sv + (size_t)n * a.sv_stride;
  const double phi = p[0], mu = p[1], sig = p[2];
  const double INF = __builtin_inf();
  int st = (fabs(phi) < 1.0 && sig > 0.0 && sig < INF) ? 0 : DLM_ST_NOT_PD;   // a stationary state
  if (!(fabs(mu) < INF)) st |= DLM_ST_NONFINITE;
  const double* al = a.alpha + (size_t)n * (a.T + 1);
  bool bad = false;
  for (int s = lane; s <= a.T; s += 64) bad |= !(fabs(al[s]) < INF);
  if (__any(bad)) st |= DLM_ST_NONFINITE;
  if (lane == 0) {
    a.rowflag[n] = st;
    if (a.status && st) atomicOr(&a.status[n], st);
  }
}

__global__ __launch_bounds__(64) void k_sv_knots(SvKnotsArgs a, int parity, int first) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= a.N) return;
  if (a.rowflag[n]) return;
  const int i = 2 * (first + (int)blockIdx.y) + parity;
  const int T = a.T, lo = a.knots[i], hi = a.knots[i + 1] - 1;
  const double* p = a.sv + (size_t)n * a.sv_stride;
  const double phi = p[0], mu = p[1], sig = p[2], s2 = sig * sig, phi2 = phi * phi;
  const unsigned long long series = a.rs.series_offset + (unsigned long long)n, seed = a.rs.seed, it = a.rs.iteration;
  const double* yn = a.y + (size_t)n * T;
  double* al = a.alpha + (size_t)n * (T + 1);
  double2* f = (double2*)(a.filt + (size_t)n * (T + 1) * 2);
  double* pr = a.prop + (size_t)n * (T + 1);
  const double INF = __builtin_inf(), QNAN = __builtin_nan("");
  int st = 0, nobs = 0;

  // forward: the block's filtering records, ystar, and the old path's sum of g.  Tiles of SVK_TILE states: the (y, alpha) of the next
  // tile are requested before the current one is computed, a tile's results leave in one burst (k_ar1_ffbs's idiom); lo and hi are
  // the wave's, so the guards of a ragged last tile do not diverge
  double m, c, g_old = 0.0;
  int s0 = lo;
  if (lo == 0) { m = mu; c = s2 / (1.0 - phi2); f[0] = make_double2(m, c); s0 = 1; }
  else { m = al[lo - 1]; c = 0.0; }
  {
    double yb[SVK_TILE], ab[SVK_TILE];
    auto request = [&](int t0) {   // states t0 .. t0 + SVK_TILE - 1, clamped at hi
#pragma unroll
      for (int j = 0; j < SVK_TILE; ++j) { const int s = t0 + j < hi ? t0 + j : hi; yb[j] = yn[s - 1]; ab[j] = al[s]; }
    };
    if (s0 <= hi) request(s0);
    for (int t0 = s0; t0 <= hi; t0 += SVK_TILE) {
      double yc[SVK_TILE], ac[SVK_TILE], po[SVK_TILE];
      double2 fo[SVK_TILE];
#pragma unroll
      for (int j = 0; j < SVK_TILE; ++j) { yc[j] = yb[j]; ac[j] = ab[j]; }
      if (t0 + SVK_TILE <= hi) request(t0 + SVK_TILE);
#pragma unroll
      for (int j = 0; j < SVK_TILE; ++j) {
        const bool in = t0 + j <= hi;
        const double yt = yc[j], ao = ac[j];
        const double y2 = yt * yt, ly = log(y2);
        bool obs = yt == yt;
        if (obs && !(fabs(ly) < INF)) { obs = false; if (in) st |= DLM_ST_NONFINITE; }   // Q20
        const double ys = ly + 1.27;
        const double at = mu + phi * (m - mu), rt = phi2 * c + s2;
        double mn = at, cn = rt;
        if (obs) {
          const double kt = rt / (rt + SVK_V);
          mn = at + kt * (ys - at);
          cn = kt * SVK_V;
        }
        if (in) {
          m = mn; c = cn;
          if (obs) { g_old = g_old + svk_g(ao, y2, ys); ++nobs; }
        }
        fo[j] = make_double2(m, c);
        po[j] = obs ? ys : QNAN;
      }
#pragma unroll
      for (int j = 0; j < SVK_TILE; ++j) if (t0 + j <= hi) { f[t0 + j] = fo[j]; pr[t0 + j] = po[j]; }
    }
  }

  // backward: the proposal, and its sum of g; tiles walked downwards, a tile's normals drawn ahead of the chain
  double x, g_new = 0.0;
  int top = hi;
  if (hi == T) {   // the free end: a draw of the last filtering distribution (lo <= T: the record is this block's)
    x = m + sqrt(c) * draw_normal(DLM_KEY_SVKNOT, seed, series, it, (unsigned)T);
    const double ys = pr[T];
    if (ys == ys) { const double yt = yn[T - 1]; g_new = g_new + svk_g(x, yt * yt, ys); }
    pr[T] = x;
    top = T - 1;
  } else {
    x = al[hi + 1];
  }
  {
    double2 fb[SVK_TILE];
    double pb[SVK_TILE], yb[SVK_TILE];
    auto request = [&](int t1) {   // states t1, t1 - 1, ..., clamped at lo (state 0 observes nothing: its slots are read at state 1 and not used)
#pragma unroll
      for (int j = 0; j < SVK_TILE; ++j) {
        const int s = t1 - j > lo ? t1 - j : lo, so = s >= 1 ? s : 1;
        fb[j] = f[s]; pb[j] = pr[so]; yb[j] = yn[so - 1];
      }
    };
    if (top >= lo) request(top);
    for (int t1 = top; t1 >= lo; t1 -= SVK_TILE) {
      double2 fc[SVK_TILE];
      double pc[SVK_TILE], yc[SVK_TILE], zz[SVK_TILE], xo[SVK_TILE];
#pragma unroll
      for (int j = 0; j < SVK_TILE; ++j) { fc[j] = fb[j]; pc[j] = pb[j]; yc[j] = yb[j]; }
      if (t1 - SVK_TILE >= lo) request(t1 - SVK_TILE);
#pragma unroll
      for (int j = 0; j < SVK_TILE; ++j) {
        const int s = t1 - j > lo ? t1 - j : lo;
        zz[j] = draw_normal(DLM_KEY_SVKNOT, seed, series, it, (unsigned)s);
      }
#pragma unroll
      for (int j = 0; j < SVK_TILE; ++j) {
        const int s = t1 - j;
        const double mt = fc[j].x, ct = fc[j].y;
        const double a1 = mu + phi * (mt - mu), r1 = phi2 * ct + s2;
        const double mean = mt + (ct * phi / r1) * (x - a1);
        double cov = ct - (ct * ct) * phi2 / r1;
        cov = cov > 0.0 ? cov : 0.0;
        const double xn = mean + sqrt(cov) * zz[j];
        if (s >= lo) {
          x = xn;
          const double ys = pc[j];
          if (s >= 1 && ys == ys) { const double yt = yc[j]; g_new = g_new + svk_g(x, yt * yt, ys); }
        }
        xo[j] = x;
      }
#pragma unroll
      for (int j = 0; j < SVK_TILE; ++j) if (t1 - j >= lo) pr[t1 - j] = xo[j];
    }
  }

  // Metropolis.mAccept
  double u1, u2;
  gibbs_rand(seed, series, it, (unsigned)lo, 0u, 1u, u1, u2, DLM_KEY_SVKNOT);
  const bool acc = nobs == 0 || log(u1) < g_new - g_old;
  if (acc) {
    for (int t0 = lo; t0 <= hi; t0 += SVK_TILE) {
      double v[SVK_TILE];
#pragma unroll
      for (int j = 0; j < SVK_TILE; ++j) v[j] = pr[t0 + j < hi ? t0 + j : hi];
#pragma unroll
      for (int j = 0; j < SVK_TILE; ++j) if (t0 + j <= hi) al[t0 + j] = v[j];
    }
    if (a.accepted) atomicAdd(&a.accepted[n], 1);
  }
  if (a.status && st) atomicOr(&a.status[n], st);
}

hipError_t launch_sv_knots(const SvKnotsArgs& a, hipStream_t s) {
  hipError_t err = launch(k_sv_knots_check, dim3((unsigned)((a.N + 3) / 4)), dim3(256), 0, s, a);
  for (int parity = 0; parity < 2 && err == hipSuccess; ++parity) {
    const int nb = (a.B - parity + 1) / 2;   // blocks parity, parity + 2, ... < B
    for (int first = 0; first < nb && err == hipSuccess; first += 65535) {   // (the grid's second dimension holds 65535)
      const int ny = nb - first < 65535 ? nb - first : 65535;
      err = launch(k_sv_knots, dim3((unsigned)((a.N + 63) / 64), (unsigned)ny), dim3(64), 0, s, a, parity, first);
    }
  }
  return err;
}

}  // namespace dlm
