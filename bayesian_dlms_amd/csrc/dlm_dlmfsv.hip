// What joins the DLM's state draw to the factor stochastic-volatility sampler in the Gibbs sampler of DlmFsv (DlmFsv.scala:64-318):
//   theta_t = G theta_{t-1} + w_t,   y_t = F_t^T theta_t + beta f_t + eps_t,  eps_t ~ N(0, diag(v)),  f_{j,t} ~ N(0, exp(alpha_{j,t}))
// for N independent panels.  dlm_ffbs_batch draws theta given the V_t stream, dlm_fsv.hip and the volatility calls draw (f, alpha,
// beta, v) given the centred panel; the kernels here make the one from the other.  None uses an atomic apart from the or into status:
// a panel's output depends on neither N nor the sharding.  The first and the last draw nothing.
//   k_dlmfsv_center     r_t = y_t - F_t^T theta_{t+1}                                  (factorObs, DlmFsv.scala:173-185)
//   k_dlmfsv_impute     the missing components of a PARTIALLY missing r_t, drawn given its observed ones
//   k_dlmfsv_variance   V_t = beta diag(exp(alpha_{.,t+1})) beta^T + diag(v)          (DlmFsvSystem.calculateVariance, DlmFsvSystem.scala:126-131)
// Layouts: y, r [N][T][p] (NaN = missing), theta [N][T+1][d] (theta[t+1] belongs to y[t]), F d x p column-major (F_ji at j + i d), one
// matrix or the model descriptor's table of T, beta [N][p][k] row-major, v [N][p], alpha [N][k][T+1] (alpha[..][t+1] belongs to y[t]),
// V [N][T][p p] (symmetric, so row- and column-major at once: the v_stride = T p p, v_tstride = p p stream of dlm_ffbs_batch).
// 1 <= k <= 8, k <= p <= 64, d <= 64.
//
// k_dlmfsv_center: one lane per output element (t, i) of a panel; a block takes 2048 consecutive elements, 256 at a time, so y is read and
// r is written fully coalesced -- they are 16 of the 16 + 8 d / p bytes per element that must move -- and the block's copy of F into LDS
// (as many bytes as 256 elements' y and r at d = p = 20) is paid once per 2048.  r_ti = y_ti - s,  s = sum_j F_ji theta_{t+1,j}
// with j ascending from s = 0.  The d loads of theta_{t+1} are the same addresses in the p neighbouring lanes of a time (a wave spans
// 64 / p times): one request per distinct line, served by the vector L1; staging the block's theta rows through LDS would add a barrier
// and save no traffic.  A time-invariant F sits in LDS TRANSPOSED (F_ji at j p + i: the lanes of a time read consecutive doubles, no
// bank conflict whatever d is; 32 KB at d = p = 64); a table of F_t is read from global memory, d consecutive doubles per lane.
// A NaN y_ti stays NaN in r_ti.  A theta_{t+1,j} that is not finite: DLM_ST_NONFINITE for the panel (r_ti is then what the sum gives).
//
// k_dlmfsv_impute<k>: one lane per (n, t), a block takes 256 consecutive t of one panel, beta, 1 / v and sqrt(v) in LDS -- the shape of
// k_fsv_factors, and its reads of r_t (p contiguous doubles per lane, used up by the wave's next loads out of the vector L1).  A time with
// all or none of its components finite is copied through.  For a partially missing one, over its observed components i in order:
//   A = sum_i (beta_i / v_i) beta_i^T (lower triangle),  c = sum_i beta_i (r_ti / v_i),  P = A + diag(exp(-alpha_{.,t+1})),
//   f = P^-1 c + L^-T z (fsv_solve_draw: f_t | the observed components),  then r_ti = sum_j beta_ij f_j + sqrt(v_i) z_i for the missing i.
// Together with the factor draw that follows on the completed panel this is one joint draw of (the missing components, f_t) given the
// observed ones, so the factor calls condition on every observation the state draw conditions on.  z_j is draw_normal of slot t, attempt
// j, z_i of attempt 8 + i, on DLM_KEY_DLMFSV.  A non-finite beta or a v that is not positive and finite: DLM_ST_NONFINITE, the panel
// copied through; a non-finite alpha_{j,t+1} of a partially missing time (or an overflowing exp(-alpha)): DLM_ST_NONFINITE, a pivot
// that is not positive: DLM_ST_NOT_PD, that time copied through.  r_out may be r_in.
//
// k_dlmfsv_variance<k>: one block per (panel, chunk of 64 times).  beta, v and e_{t,l} = exp(alpha_{l,t+1}) of the chunk go into LDS once
// (alpha read coalesced over t for each l).  A lane owns an entry (i, j): it forms b_l = beta_il beta_jl once (k registers) and then
// V_t(i, j) = sum_l b_l e_{t,l} with l ascending from 0, + v_i when i == j, for its times of the chunk.  b_l is the same product for
// (i, j) and (j, i), so V_t is symmetric bit for bit.  With p^2 >= 256 the block's lanes stride over the entries (every time's p^2
// doubles are stored as contiguous runs of 256); with p^2 < 256 the block holds floor(256 / p^2) groups of p^2 lanes, group g taking
// the times g, g + G, ... -- each group's store is one contiguous p^2 run.  The kernel is bound by its 8 p^2 bytes per (n, t) of
// writes; the stores are plain or non-temporal by DLM_DLMFSV_NT_STORES (measured both ways).
// A beta or alpha_{l,t+1} that is not finite, an exp(alpha) that overflows, a v that is not positive and finite: DLM_ST_NONFINITE for the
// panel; V is what the arithmetic gives.
//
// The same model with the factor process as the SYSTEM noise (DlmFsvSystem.scala:215-344): theta_t = G theta_{t-1} + beta f_t + eps_t,
// y_t = F_t^T theta_t + nu_t.  There the factor calls read the state's innovations (p := d) and k_dlmfsv_variance writes the W_t stream.
//   k_dlmfsvsys_innovations   w_t = theta_{t+1} - G theta_t                            (factorState, DlmFsvSystem.scala:109-117)
// theta [N][T+1][d], one G d x d column-major (G_ij at i + j d), w [N][T][d] (w[t] belongs to alpha[..][t+1], as y[t] does above), d <= 64.
// k_dlmfsv_center's shape: one lane per output element (t, i), a block takes 2048 consecutive elements, 256 at a time, so theta_{t+1,i}
// (element e + d of the panel's theta) and w_ti are fully coalesced -- they are the 16 bytes per element that must move: the d loads of
// theta_t fall on the lines that theta_{t+1,i} asked for one time earlier, so HBM sees theta once -- and the block's copy of G
// (32 KB at d = 64) is paid once per 2048.  w_ti = theta_{t+1,i} - s,  s = sum_j G_ij theta_{t,j} with j ascending from s = 0.  G sits in
// LDS as it is: column-major already puts the d lanes of a time on consecutive doubles for every j, so no bank conflict whatever d is,
// and the 64 / d times of a wave read the same words (a broadcast).  The d loads of theta_t are the same addresses in the d neighbouring
// lanes: one request per distinct line, served by the vector L1.  A theta_{t,j} that is not finite, theta_0 and theta_T included (every
// one is read): DLM_ST_NONFINITE for the panel (w is then what the arithmetic gives).  w must not alias theta.
#include "dlm_draws.h"
#include "dlm_fsv_solve.h"

#ifndef DLM_DLMFSV_NT_STORES
#define DLM_DLMFSV_NT_STORES 0
#endif

namespace dlm {

constexpr int DLM_DLMFSV_CHUNK = 64;           // times per block of k_dlmfsv_variance
constexpr int DLM_DLMFSV_CENTER_ELEMS = 2048;   // elements per block of k_dlmfsv_center

__global__ __launch_bounds__(256) void k_dlmfsv_center(DlmFsvCenterArgs a, int blocks_per_panel) {
  extern __shared__ double sFt[];   // the time-invariant F transposed: F_ji at j p + i
  const int tid = threadIdx.x, p = a.p, d = a.d, Tp = a.T * a.p;
  const int n = (int)(blockIdx.x / (unsigned)blocks_per_panel);
  const int e0 = (int)(blockIdx.x - (unsigned)n * (unsigned)blocks_per_panel) * DLM_DLMFSV_CENTER_ELEMS;
  const int e1 = e0 + DLM_DLMFSV_CENTER_ELEMS < Tp ? e0 + DLM_DLMFSV_CENTER_ELEMS : Tp;
  const double INF = __builtin_inf();
  if (!a.f_stride) {
    for (int q = tid; q < d * p; q += 256) {
      const int i = q / d, j = q - i * d;
      sFt[j * p + i] = a.F[q];
    }
    __syncthreads();
  }
  const double* thn = a.theta + (size_t)n * (a.T + 1) * d;
  const size_t on = (size_t)n * Tp;
  bool bad = false;
  for (int e = e0 + tid; e < e1; e += 256) {
    const int t = e / p, i = e - t * p;
    const double* th = thn + (size_t)(t + 1) * d;
    double s = 0.0;
    if (a.f_stride) {
      const double* Ft = a.F + (size_t)t * (size_t)a.f_stride + (size_t)i * d;
#pragma unroll 4
      for (int j = 0; j < d; ++j) {
        const double x = th[j];
        bad = bad || !(fabs(x) < INF);
        s = s + Ft[j] * x;
      }
    } else {
#pragma unroll 4
      for (int j = 0; j < d; ++j) {
        const double x = th[j];
        bad = bad || !(fabs(x) < INF);
        s = s + sFt[j * p + i] * x;
      }
    }
    a.r[on + e] = a.y[on + e] - s;
  }
  if (bad && a.status) atomicOr(&a.status[n], DLM_ST_NONFINITE);
}

__global__ __launch_bounds__(256) void k_dlmfsvsys_innovations(DlmFsvSysInnovationsArgs a, int blocks_per_panel) {
  extern __shared__ double sG[];   // G as it is: G_ij at i + j d
  const int tid = threadIdx.x, d = a.d, Td = a.T * a.d;
  const int n = (int)(blockIdx.x / (unsigned)blocks_per_panel);
  const int e0 = (int)(blockIdx.x - (unsigned)n * (unsigned)blocks_per_panel) * DLM_DLMFSV_CENTER_ELEMS;
  const int e1 = e0 + DLM_DLMFSV_CENTER_ELEMS < Td ? e0 + DLM_DLMFSV_CENTER_ELEMS : Td;
  const double INF = __builtin_inf();
  for (int q = tid; q < d * d; q += 256) sG[q] = a.G[q];
  __syncthreads();
  const double* thn = a.theta + (size_t)n * (a.T + 1) * d;
  double* wn = a.w + (size_t)n * Td;
  bool bad = false;
  for (int e = e0 + tid; e < e1; e += 256) {
    const int t = e / d, i = e - t * d;
    const double* th = thn + (size_t)t * d;
    double s = 0.0;
#pragma unroll 4
    for (int j = 0; j < d; ++j) {
      const double x = th[j];
      bad = bad || !(fabs(x) < INF);
      s = s + sG[i + j * d] * x;
    }
    const double x1 = thn[(size_t)e + d];   // theta_{t+1,i}
    bad = bad || !(fabs(x1) < INF);
    wn[e] = x1 - s;
  }
  if (bad && a.status) atomicOr(&a.status[n], DLM_ST_NONFINITE);
}

template <int K>
__global__ __launch_bounds__(256) void k_dlmfsv_variance(DlmFsvVarianceArgs a, int chunks) {
  constexpr int TC = DLM_DLMFSV_CHUNK;
  __shared__ double sB[DLM_FSV_MAX_P * K], sV[DLM_FSV_MAX_P], sE[TC * K];
  __shared__ int sBad;
  const int tid = threadIdx.x, p = a.p, T = a.T;
  const int n = (int)(blockIdx.x / (unsigned)chunks);
  const int t0 = (int)(blockIdx.x - (unsigned)n * (unsigned)chunks) * TC;
  const int nt = T - t0 < TC ? T - t0 : TC;
  const double INF = __builtin_inf();
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
    sV[tid] = v;
  }
  for (int q = tid; q < nt * K; q += 256) {
    const int l = q / nt, tt = q - l * nt;
    const double x = a.alpha[((size_t)n * K + l) * (T + 1) + t0 + tt + 1];
    const double ex = exp(x);
    bad = bad || !(fabs(x) < INF) || !(ex < INF);
    sE[tt * K + l] = ex;
  }
  if (bad) sBad = 1;
  __syncthreads();
  if (tid == 0 && sBad && a.status) atomicOr(&a.status[n], DLM_ST_NONFINITE);
  const int pp = p * p;
  const int G = pp < 256 ? 256 / pp : 1;
  const int g = tid / pp, e0 = tid - g * pp;
  if (g >= G) return;
  double* Vn = a.V + ((size_t)n * T + t0) * pp;
  for (int e = e0; e < pp; e += 256) {   // (one pass when G > 1: e0 < p^2 <= 256)
    const int i = e / p, j = e - i * p;
    double b[K];
#pragma unroll
    for (int l = 0; l < K; ++l) b[l] = sB[i * K + l] * sB[j * K + l];
    const bool diag = i == j;
    const double vi = sV[i];
    for (int tt = g; tt < nt; tt += G) {
      double s = 0.0;
#pragma unroll
      for (int l = 0; l < K; ++l) s = s + b[l] * sE[tt * K + l];
      if (diag) s = s + vi;
#if DLM_DLMFSV_NT_STORES
      __builtin_nontemporal_store(s, Vn + (size_t)tt * pp + e);
#else
      Vn[(size_t)tt * pp + e] = s;
#endif
    }
  }
}

template <int K>
__global__ __launch_bounds__(256) void k_dlmfsv_impute(DlmFsvImputeArgs a, int blocks_per_panel) {
  constexpr int NS = K * (K + 1) / 2;
  __shared__ double sB[DLM_FSV_MAX_P * K], sIv[DLM_FSV_MAX_P], sSd[DLM_FSV_MAX_P];
  __shared__ int sBad;
  const int tid = threadIdx.x, p = a.p, T = a.T;
  const int n = (int)(blockIdx.x / (unsigned)blocks_per_panel);
  const int t = (int)(blockIdx.x - (unsigned)n * (unsigned)blocks_per_panel) * 256 + tid;
  const double INF = __builtin_inf();
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
    sSd[tid] = sqrt(v);
  }
  if (bad) sBad = 1;
  __syncthreads();
  if (t >= T) return;
  const double* yt = a.r_in + ((size_t)n * T + t) * p;
  double* ot = a.r_out + ((size_t)n * T + t) * p;
  double A[NS], c[K];
#pragma unroll
  for (int e = 0; e < NS; ++e) A[e] = 0.0;
#pragma unroll
  for (int j = 0; j < K; ++j) c[j] = 0.0;
  int nobs = 0;
  for (int i = 0; i < p; ++i) {
    const double yi = yt[i];
    if (!(fabs(yi) < INF)) continue;
    nobs += 1;
    const double iv = sIv[i], w = yi * iv;
#pragma unroll
    for (int g = 0; g < K; ++g) {
      const double bg = sB[i * K + g];
      c[g] = c[g] + bg * w;
      const double bi = bg * iv;
#pragma unroll
      for (int h = 0; h <= g; ++h) A[g * (g + 1) / 2 + h] = A[g * (g + 1) / 2 + h] + bi * sB[i * K + h];
    }
  }
  bool fill = nobs > 0 && nobs < p && !sBad;
  if (sBad && t == 0 && a.status) atomicOr(&a.status[n], DLM_ST_NONFINITE);
  if (fill) {
    bool abad = false;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const double x = a.alpha[((size_t)n * K + j) * (T + 1) + t + 1];
      const double d = exp(-x);
      abad = abad || !(fabs(x) < INF) || !(d < INF);
      A[j * (j + 1) / 2 + j] = A[j * (j + 1) / 2 + j] + d;
    }
    bool ok = true;
    if (!abad) {
      const unsigned long long series = a.rs.series_offset + (unsigned long long)n;
      double z[K];
#pragma unroll
      for (int j = 0; j < K; ++j) z[j] = draw_normal(DLM_KEY_DLMFSV, a.rs.seed, series, a.rs.iteration, (unsigned)t, (unsigned)j);
      ok = fsv_solve_draw<K>(A, c, z, false);
    }
    if (a.status && (abad || !ok)) atomicOr(&a.status[n], abad ? DLM_ST_NONFINITE : DLM_ST_NOT_PD);
    fill = !abad && ok;
  }
  if (!fill && ot == yt) return;
  for (int i = 0; i < p; ++i) {
    double yi = yt[i];
    if (fill && !(fabs(yi) < INF)) {
      double m = 0.0;
#pragma unroll
      for (int j = 0; j < K; ++j) m = m + sB[i * K + j] * c[j];
      yi = m + sSd[i] * draw_normal(DLM_KEY_DLMFSV, a.rs.seed, a.rs.series_offset + (unsigned long long)n, a.rs.iteration, (unsigned)t, 8u + (unsigned)i);
    }
    ot[i] = yi;
  }
}

hipError_t launch_dlmfsv_impute(const DlmFsvImputeArgs& a, hipStream_t s) {
  const int bpp = (a.T + 255) / 256;
  return pick<1, 2, 3, 4, 5, 6, 7, 8>(a.k, [&](auto k) {
    return launch(k_dlmfsv_impute<k()>, dim3((unsigned)a.N * (unsigned)bpp), dim3(256), 0, s, a, bpp);
  });
}

hipError_t launch_dlmfsv_center(const DlmFsvCenterArgs& a, hipStream_t s) {
  const int bpp = (int)(((long long)a.T * a.p + DLM_DLMFSV_CENTER_ELEMS - 1) / DLM_DLMFSV_CENTER_ELEMS);
  const size_t lds = a.f_stride ? 0 : sizeof(double) * (size_t)a.d * a.p;
  return launch(k_dlmfsv_center, dim3((unsigned)a.N * (unsigned)bpp), dim3(256), lds, s, a, bpp);
}

hipError_t launch_dlmfsvsys_innovations(const DlmFsvSysInnovationsArgs& a, hipStream_t s) {
  const int bpp = (int)(((long long)a.T * a.d + DLM_DLMFSV_CENTER_ELEMS - 1) / DLM_DLMFSV_CENTER_ELEMS);
  return launch(k_dlmfsvsys_innovations, dim3((unsigned)a.N * (unsigned)bpp), dim3(256), sizeof(double) * (size_t)a.d * a.d, s, a, bpp);
}

hipError_t launch_dlmfsv_variance(const DlmFsvVarianceArgs& a, hipStream_t s) {
  const int chunks = (a.T + DLM_DLMFSV_CHUNK - 1) / DLM_DLMFSV_CHUNK;
  return pick<1, 2, 3, 4, 5, 6, 7, 8>(a.k, [&](auto k) {
    return launch(k_dlmfsv_variance<k()>, dim3((unsigned)a.N * (unsigned)chunks), dim3(256), 0, s, a, chunks);
  });
}

}  // namespace dlm
