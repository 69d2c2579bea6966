// The factor half of the factor stochastic-volatility Gibbs sampler (FactorSv.sampleAr, FactorSv.scala:546-562): N independent panels,
//   y_t = beta f_t + eps_t,  eps_t ~ N(0, diag(v)),  f_{j,t} ~ N(0, exp(alpha_{j,t})),  v = sigma^2 1_p,
//   beta p x k with beta_ii = 1, beta_ij = 0 for j > i and beta_ij ~ N(m, s^2) elsewhere,  sigma^2 ~ InverseGamma(shape, scale).
// The volatility half -- alpha_j and (phi, mu, sigma_eta)_j of the N k factor series -- is dlm_sv.hip and dlm_ar1.hip as they are: f is
// [N][k][T], which viewed as [N k][T] is their y.  The two kernels here:
//   k_fsv_factors    f_t | (y_t, beta, v, alpha_{t+1}) for every (n, t)                          (sampleFactors, :168-186)
//   k_fsv_loadings   sigma^2 | (y, f, beta_old), then beta | (y, f, sigma^2) row by row         (sampleSigmaUni, :516-541; sampleBeta, :253-333)
// Layouts: y [N][T][p] (NaN = missing), f [N][k][T], alpha [N][k][T+1] (alpha[..][t+1] belongs to y[t]), beta [N][p][k] row-major,
// v [N][p].  1 <= k <= 8, k <= p <= 64; the kernels are templates on k, so that the k x k systems stay in registers.
//
// A time is OBSERVED when all p components of y_t are finite (encodePartiallyMissing, :150-157: a partially missing y_t is wholly
// missing); k_fsv_loadings asks for a finite f_t too.  An unobserved time gets f_t = NaN and enters no sum.
//
// The small SPD systems (fsv_solve_draw, dlm_fsv_solve.h).  P = L L^T by the row-oriented Cholesky factorisation, the lower triangle packed by rows:
//   L_jj = sqrt(P_jj - sum_{m<j} L_jm^2),  L_ij = (P_ij - sum_{m<j} L_im L_jm) / L_jj,  the sums subtracted one by one in m order;
//   u = L^-1 r by forward substitution, x = L^-T u by backward substitution (m ascending from i + 1).
//   default:  x = L^-T (L^-1 r + z)      = P^-1 r + L^-T z   ~ N(P^-1 r, P^-1)
//   literal:  x = L^-T L^-1 (r + z)      = P^-1 r + P^-1 z   ~ N(P^-1 r, P^-2)   (Q27: `vt.t * diag(1/d) * z` of rnorm, :222-232)
// A pivot that is not positive gives DLM_ST_NOT_PD and NaN in what the system was to give.
//
// k_fsv_factors: one lane per (n, t), a block takes 256 consecutive t of one panel.  The block first writes beta, 1 / v and
// A = beta^T diag(1 / v) beta into LDS (A_rc = sum_i (beta_ir / v_i) beta_ic in i order); a lane then forms
// r = beta^T (y_t / v) (r_j = sum_i beta_ij (y_ti (1 / v_i)) in i order), P = A + diag(exp(-alpha_{j,t+1})) (alpha == nullptr: + I) and
// draws.  y_t is read straight from global memory, p contiguous doubles per lane at stride p between lanes: every 128-byte line is
// used up by the same wave within its next 16 loads, which the vector L1 serves, and the p loads of a lane are independent of each
// other; staging the block's 256 p doubles through LDS would take 128 KB at p = 64, or a barrier per chunk (not measured against
// each other: DESIGN.md 4.16).  f[n][j][t] is written coalesced over t for each j.
// z_j is draw_normal of slot t, attempt j on DLM_KEY_FSV.
// A non-finite beta or a v that is not positive and finite: the WHOLE panel gets DLM_ST_NONFINITE and NaN.  A non-finite alpha_{j,t+1}
// (or one whose exp(-alpha) overflows): the panel gets DLM_ST_NONFINITE and that time NaN.
//
// k_fsv_loadings: one workgroup of 256 per panel.  Lane l < p of each of the four waves owns row l of beta; wave w takes the times
// t = w, w + 4, ... in order.  Per observed time a lane adds f_j y_l to its c_l (k sums) and (y_l - sum_j beta_old_lj f_j)^2 to its
// share of ssy; lane e < k (k + 1) / 2 adds f_a f_b to its entry (a, b), a >= b, of S = sum f f^T.  The four waves' sums are combined
// through LDS in wave order, ((w0 + w1) + w2) + w3, and ssy is then summed over the rows l = 0 .. p - 1 in order: a fixed order, no
// atomics.  With n the number of observed times:
//   default:  sigma^2 ~ InverseGamma(shape + n p / 2, scale + ssy / 2) = scale' / Gamma(shape', 1)
//   literal:  sigma^2 ~ InverseGamma(shape + n / 2,   scale + ssy / (2 p))                                     (Q28, :525, :537)
//   row i >= 1, q = min(i, k), S_q the leading q x q block, c_i the first q entries:
//   default:  P = S_q / sigma^2 + I / s^2,  r = (c_i - [i < k] S_{0:q, i}) / sigma^2 + m / s^2
//   literal:  P = S_q / sigma^2 + I s^2,    r = c_i / sigma^2                                                  (Q29, Q30; :262-281)
//   beta_{i, 0:q} = fsv_solve_draw(P, r, z),  z_a = draw_normal of slot DLM_FSV_SLOT_ROW0 - i, attempt a.
// Every lane runs the k x k code: a row with q < k pads its system with the identity (rows q .. k - 1: unit diagonal, r = z = 0),
// which leaves the first q unknowns as the q x q system gives them.  The Gamma is drawn on lane 0 at the kernel's one call of
// gamma_unit.  n = 0: DLM_ST_NONFINITE, beta_out = beta_in and v_out = v_in (NaN without a v_in).  Sums that are not finite:
// DLM_ST_NONFINITE and NaN.  beta_old is in registers before the first barrier, so beta_out may be beta_in.
#include "dlm_draws.h"
#include "dlm_fsv_solve.h"
#include "dlm_wave.h"

namespace dlm {

template <int K>
__global__ __launch_bounds__(256) void k_fsv_factors(FsvFactorsArgs a, int blocks_per_panel) {
  __shared__ double sB[DLM_FSV_MAX_P * K], sIv[DLM_FSV_MAX_P], sA[K * K];
  __shared__ int sBad;
  const int tid = threadIdx.x, p = a.p, T = a.T;
  const int n = (int)(blockIdx.x / (unsigned)blocks_per_panel);
  const int t = (int)(blockIdx.x - (unsigned)n * (unsigned)blocks_per_panel) * 256 + tid;
  const double INF = __builtin_inf(), NaN = __builtin_nan("");
  if (tid == 0) sBad = 0;
  __syncthreads();
  bool bad = false;
  for (int e = tid; e < p * K; e += 256) {
    const double b = a.beta[(size_t)n * p * K + e];
    sB[e] = b;
    bad = bad || !(fabs(b) < INF);
  }
  if (tid < p) {
    const double v = a.v[(size_t)n * p + tid];
    bad = bad || !(v > 0.0) || !(v < INF);
    sIv[tid] = 1.0 / v;
  }
  if (bad) sBad = 1;
  __syncthreads();
  if (tid < K * K) {
    const int r = tid / K, c = tid - r * K;
    double s = 0.0;
    for (int i = 0; i < p; ++i) s = s + (sB[i * K + r] * sIv[i]) * sB[i * K + c];
    sA[tid] = s;
  }
  __syncthreads();
  if (t >= T) return;
  double* fo = a.f + (size_t)n * K * T + t;
  if (sBad) {
#pragma unroll
    for (int j = 0; j < K; ++j) fo[(size_t)j * T] = NaN;
    if (t == 0 && a.status) atomicOr(&a.status[n], DLM_ST_NONFINITE);
    return;
  }
  const double* yt = a.y + ((size_t)n * T + t) * p;
  double r[K];
#pragma unroll
  for (int j = 0; j < K; ++j) r[j] = 0.0;
  bool obs = true;
  for (int i = 0; i < p; ++i) {
    const double yi = yt[i];
    obs = obs && fabs(yi) < INF;
    const double w = yi * sIv[i];
#pragma unroll
    for (int j = 0; j < K; ++j) r[j] = r[j] + sB[i * K + j] * w;
  }
  double P[K * (K + 1) / 2];
  bool abad = false;
#pragma unroll
  for (int i = 0; i < K; ++i) {
#pragma unroll
    for (int j = 0; j < i; ++j) P[i * (i + 1) / 2 + j] = sA[i * K + j];
    double d = 1.0;
    if (a.alpha) {
      const double x = a.alpha[((size_t)n * K + i) * (T + 1) + t + 1];
      d = exp(-x);
      abad = abad || !(fabs(x) < INF) || !(d < INF);
    }
    P[i * (i + 1) / 2 + i] = sA[i * K + i] + d;
  }
  bool ok = true;
  if (obs && !abad) {
    const unsigned long long series = a.rs.series_offset + (unsigned long long)n;
    double z[K];
#pragma unroll
    for (int j = 0; j < K; ++j) z[j] = draw_normal(DLM_KEY_FSV, a.rs.seed, series, a.rs.iteration, (unsigned)t, (unsigned)j);
    ok = fsv_solve_draw<K>(P, r, z, a.literal != 0);
  }
  const bool keep = obs && !abad && ok;
#pragma unroll
  for (int j = 0; j < K; ++j) fo[(size_t)j * T] = keep ? r[j] : NaN;
  if (a.status && (abad || !ok)) atomicOr(&a.status[n], abad ? DLM_ST_NONFINITE : DLM_ST_NOT_PD);
}

template <int K>
__global__ __launch_bounds__(256) __attribute__((flatten)) void k_fsv_loadings(FsvLoadingsArgs a) {
  constexpr int NS = K * (K + 1) / 2;
  __shared__ double sPart[4][64][K + 1];   // per wave and lane: c (K) | ssy
  __shared__ double sSp[4][NS];
  __shared__ int sCnt[4];
  __shared__ double sS[K * K], sSsy[64];
  const int n = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int p = a.p, T = a.T;
  const bool active = lane < p;
  const double INF = __builtin_inf(), NaN = __builtin_nan("");
  const double* Y = a.y + (size_t)n * T * p;
  const double* F = a.f + (size_t)n * K * T;
  double b[K], c[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    b[j] = active ? a.beta_in[((size_t)n * p + lane) * K + j] : 0.0;
    c[j] = 0.0;
  }
  int sa = 0, sb = 0;   // this lane's entry (sa, sb), sa >= sb, of S (lanes >= NS: unused)
#pragma unroll
  for (int i = 0; i < K; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      if (lane == i * (i + 1) / 2 + j) { sa = i; sb = j; }
    }
  }
  double ssy = 0.0, sacc = 0.0;
  int cnt = 0;
  // (the loads of the wave's next time are issued before this one's sums: an iteration is a handful of multiply-adds behind a
  //  global load, and a wave has nothing else to hide that latency with)
  double fn[K], yn = 0.0;
#pragma unroll
  for (int j = 0; j < K; ++j) fn[j] = w < T ? F[(size_t)j * T + w] : 0.0;
  if (w < T && active) yn = Y[(size_t)w * p + lane];
  for (int t = w; t < T; t += 4) {
    double ft[K];
    bool fin = true;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      ft[j] = fn[j];
      fin = fin && fabs(ft[j]) < INF;
    }
    const double yv = yn;
    if (t + 4 < T) {
#pragma unroll
      for (int j = 0; j < K; ++j) fn[j] = F[(size_t)j * T + t + 4];
      if (active) yn = Y[(size_t)(t + 4) * p + lane];
    }
    if (!__all(fin && fabs(yv) < INF)) continue;
    cnt += 1;
    double pred = 0.0, fa = ft[0], fb = ft[0];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      c[j] = c[j] + ft[j] * yv;
      pred = pred + b[j] * ft[j];
      fa = sa == j ? ft[j] : fa;
      fb = sb == j ? ft[j] : fb;
    }
    const double res = yv - pred;
    ssy = ssy + res * res;
    sacc = sacc + fa * fb;
  }
#pragma unroll
  for (int j = 0; j < K; ++j) sPart[w][lane][j] = c[j];
  sPart[w][lane][K] = ssy;
  if (lane < NS) sSp[w][lane] = sacc;
  if (lane == 0) sCnt[w] = cnt;
  __syncthreads();
  if (w == 0) {
#pragma unroll
    for (int j = 0; j < K; ++j) c[j] = ((sPart[0][lane][j] + sPart[1][lane][j]) + sPart[2][lane][j]) + sPart[3][lane][j];
    sSsy[lane] = ((sPart[0][lane][K] + sPart[1][lane][K]) + sPart[2][lane][K]) + sPart[3][lane][K];
    if (lane < NS) {
      const double s = ((sSp[0][lane] + sSp[1][lane]) + sSp[2][lane]) + sSp[3][lane];
      sS[sa * K + sb] = s;
      sS[sb * K + sa] = s;
    }
  }
  __syncthreads();
  if (w != 0) return;
  const int nobs = ((sCnt[0] + sCnt[1]) + sCnt[2]) + sCnt[3];
  double* bo = a.beta_out + ((size_t)n * p + lane) * K;
  double* vo = a.v_out + (size_t)n * p + lane;
  if (nobs == 0) {   // nothing to condition on: the inputs stay
    if (active) {
#pragma unroll
      for (int j = 0; j < K; ++j) bo[j] = b[j];
      *vo = a.v_in ? a.v_in[(size_t)n * p + lane] : NaN;
    }
    if (lane == 0 && a.status) atomicOr(&a.status[n], DLM_ST_NONFINITE);
    return;
  }
  double tot = 0.0;
  for (int l = 0; l < p; ++l) tot = tot + sSsy[l];
  bool bad = !(fabs(tot) < INF);
  for (int e = 0; e < K * K; ++e) bad = bad || !(fabs(sS[e]) < INF);
#pragma unroll
  for (int j = 0; j < K; ++j) bad = bad || (active && !(fabs(c[j]) < INF));
  bad = __any(bad);
  const dlm_fsv_prior& pr = a.prior;
  const bool lit = pr.literal != 0;
  const unsigned long long series = a.rs.series_offset + (unsigned long long)n, seed = a.rs.seed, it = a.rs.iteration;
  const double nd = (double)nobs, pd = (double)p;
  const double shape = lit ? pr.sigma_shape + 0.5 * nd : pr.sigma_shape + 0.5 * (nd * pd);   // Q28
  const double scale = lit ? pr.sigma_scale + tot / (2.0 * pd) : pr.sigma_scale + 0.5 * tot;
  double s2 = NaN;
  if (lane == 0 && !bad) s2 = scale / gamma_unit(shape, seed, series, it, DLM_FSV_SLOT_SIGMA, DLM_KEY_FSV);
  s2 = __shfl(s2, 0, 64);
  if (!active) return;
  if (bad) {
#pragma unroll
    for (int j = 0; j < K; ++j) bo[j] = NaN;
    *vo = NaN;
    if (lane == 0 && a.status) atomicOr(&a.status[n], DLM_ST_NONFINITE);
    return;
  }
  const int i = lane, q = i < K ? i : K, ic = i < K ? i : 0;
  const double sd2 = pr.beta_sd * pr.beta_sd;
  const double pdiag = lit ? sd2 : 1.0 / sd2;            // Q29: the prior VARIANCE where the precision belongs
  const double pmean = lit ? 0.0 : pr.beta_mean / sd2;   // Q29: the prior mean dropped
  double P[NS], r[K], z[K];
#pragma unroll
  for (int g = 0; g < K; ++g) {
    const bool in = g < q;
#pragma unroll
    for (int h = 0; h < g; ++h) P[g * (g + 1) / 2 + h] = in ? sS[g * K + h] / s2 : 0.0;
    P[g * (g + 1) / 2 + g] = in ? sS[g * K + g] / s2 + pdiag : 1.0;
    const double own = (!lit && i < K) ? c[g] - sS[g * K + ic] : c[g];   // Q30: rows i < k regress y_i - f_i
    r[g] = in ? own / s2 + pmean : 0.0;
    z[g] = 0.0;
    if (in) z[g] = draw_normal(DLM_KEY_FSV, seed, series, it, DLM_FSV_SLOT_ROW0 - (unsigned)i, (unsigned)g);
  }
  const bool ok = fsv_solve_draw<K>(P, r, z, lit);
#pragma unroll
  for (int j = 0; j < K; ++j) bo[j] = j < q ? (ok ? r[j] : NaN) : (j == i ? 1.0 : 0.0);
  *vo = s2;
  if (!ok && a.status) atomicOr(&a.status[n], DLM_ST_NOT_PD);
}

hipError_t launch_fsv_factors(const FsvFactorsArgs& a, hipStream_t s) {
  const int bpp = (a.T + 255) / 256;
  return pick<1, 2, 3, 4, 5, 6, 7, 8>(a.k, [&](auto k) {
    return launch(k_fsv_factors<k()>, dim3((unsigned)a.N * (unsigned)bpp), dim3(256), 0, s, a, bpp);
  });
}

hipError_t launch_fsv_loadings(const FsvLoadingsArgs& a, hipStream_t s) {
  return pick<1, 2, 3, 4, 5, 6, 7, 8>(a.k, [&](auto k) { return launch(k_fsv_loadings<k()>, dim3((unsigned)a.N), dim3(256), 0, s, a); });
}

}  // namespace dlm
