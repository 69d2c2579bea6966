// The two device steps of the posterior-predictive forecast of the factor stochastic-volatility models (FactorSv, DlmFsv, DlmFsvSystem;
// DESIGN.md 4.28) that the sampler's own calls do not already make:
//   k_sv_paths            future log-volatility paths  alpha_{j,h} = mu_j + phi_j (alpha_{j,h-1} - mu_j) + sigma_j z   (StochasticVolatility.stepState)
//   k_mixture_moments     mean and total covariance of the equal-weight mixture of C Gaussians N(f_c, Q_c) per (row, time)
//   k_mixture_quantiles   the exact quantiles of its marginals  sum_c N(f_ci, Q_cii) / C
// dlm_dlmfsv_variance_batch makes the variance stream from the paths and dlm_filter_batch the (f, Q) records from the stream; the summary
// reads either in place through its three strides.  No kernel uses an atomic apart from the or into status, every sum runs in a fixed
// order: a row's output depends on neither N nor its neighbours.
//
// k_sv_paths<k>: one lane per (row, path), a block is the 64 paths r0 .. r0 + 63 of a row; the k <= 8 chains of a path stay in registers.
// alpha [N][R][k][H+1]: entry 0 of a chain is its start -- alpha0[n][j], or with alpha0 == NULL mu + sigma / sqrt(1 - phi^2) z of the slot
// DLM_SVPATH_SLOT_START --, entry h the step above with the normal of slot h, path r in the attempt field, under the key
// DLM_KEY_SVPATH + j (dlm_draws.h): a pure function of (seed, series_offset + n, iteration, h, r, j), so the first 64 paths of an
// R = 128 call are the R = 64 call.  A lane's stores lie k (H + 1) doubles from its neighbour's: the paths are 8 k (H + 1) R bytes per
// row against the 8 p^2 H R of the stream made from them, so they are left uncoalesced.  A row with a non-finite (phi, mu, sigma) or
// alpha0: DLM_ST_NONFINITE; else with |phi| >= 1 or sigma <= 0: DLM_ST_NOT_PD; its paths are NaN either way.
//
// k_mixture_moments: one block per (row, time).  A lane owns an entry (i, j) of the covariance and reads, for its components c in
// ascending order, Q_c(lo, hi) with lo = min(i, j), hi = max(i, j) -- (i, j) and (j, i) read the same word and multiply the same
// f_c,lo f_c,hi, so cov is symmetric bit for bit whatever the input's own symmetry:
//   S = sum_c (Q_c(lo, hi) + f_c,lo f_c,hi),  F_lo = sum_c f_c,lo,  F_hi = sum_c f_c,hi     each from 0, c ascending
//   mean_i = F_i / C,   cov_ij = S / C - (F_lo / C) (F_hi / C)
// With p^2 >= 256 the block's lanes stride over the entries and every lane sums all C components; with p^2 < 256 the block holds
// G = floor(256 / p^2) groups of p^2 lanes, group g sums the components g, g + G, ... and the group-0 lane adds the groups' partial sums
// in ascending g.  The reads of a group are the contiguous p^2 doubles of one record.  One block per (row, time) reads C p^2 doubles:
// with few rows and many components the call is bound by a block's own load stream (not tuned).
// A Q_c,ii that is not positive and finite: DLM_ST_NOT_PD, an f_c,i that is not finite: DLM_ST_NONFINITE, for the row; mean_i and the row
// and column i of cov are NaN.
//
// k_mixture_quantiles: one block per cell (row, time, component i).  The cell's C pairs (f_ci, s_c = sqrt(2 Q_cii)) are read ONCE from
// the strided input and held in LDS (C <= DLM_MIX_LDS_C = 4096: 64 KB) or, beyond it, packed into the engine's workspace [cell][C][2],
// which every evaluation then reads coalesced.  An evaluation at x: every lane takes the components tid, tid + 256, ..., z = (x - f) / s,
//   cdf_c = z > 0 ? 1 - erfc(z) / 2 : erfc(-z) / 2      (the small tail is the one evaluated, so the absolute error is that of 1/2 ulp of 1)
//   pdf_c = exp(-z^2) / s                                 (times 1 / sqrt(pi))
// the lanes' sums go through wave_sum and the four waves' are added in order; F(x) = sum / C.
// STOPPING RULE.  For each prob the bracket starts at [min f - (|z_p| + 1) max s, max f + (|z_p| + 1) max s], z_p = normcdfinv(prob), where
// F(lo) < prob <= F(hi) with a margin of a factor e^|z_p|.  Every evaluation moves one end: lo = x where the computed F(x) < prob, else
// hi = x, so the computed F(lo) < prob <= F(hi) always holds.  The next x is the Newton step from x, overshot by a thousandth of its length
// (so that the iterates straddle the root and BOTH ends close in), or the midpoint where that leaves (lo, hi), the density vanishes, or
// neither of the last two evaluations halved the bracket.  The search ends with q = x at an exact hit F(x) == prob, else with q = hi once hi is the
// double next to lo: q is the smallest double found with F(q) >= prob whose predecessor has F < prob.  Hence
// |F_exact(q) - prob| <= density(q) spacing(q) + the rounding of the computed F, which is below C 2^-52.  The loop is bounded (DLM_MIX_MAX_EVALS = 3500:
// three evaluations per halving, 1075 + 64 halvings from the widest bracket of doubles to the narrowest); nothing is sampled.
// A cell with a bad Q_cii or f_ci (the flags above): its quantiles are NaN.
// Registers: 256 VGPRs + 218 AGPRs, no scratch -- the compiler keeps the double constants of erfc, exp and normcdfinv in registers across
// the search loop; bounded to two or four waves per SIMD it spills 224 / 350 of them instead (900 / 1404 bytes of scratch per lane), so the
// kernel is left at one block of four waves per CU.  A band has N H p cells, of the order of the 256 CUs.
#include "dlm_draws.h"
#include "dlm_wave.h"

namespace dlm {

constexpr int DLM_MIX_MAX_EVALS = 3500;

template <int K>
__global__ __launch_bounds__(64) void k_sv_paths(SvPathsArgs a, int chunks) {
  const int n = (int)(blockIdx.x / (unsigned)chunks);
  const int r = (int)(blockIdx.x - (unsigned)n * (unsigned)chunks) * 64 + (int)threadIdx.x;
  const int H = a.H;
  const double INF = __builtin_inf();
  double phi[K], mu[K], sg[K], al[K];
  bool nonfinite = false, notpd = false;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const double* q = a.sv + ((size_t)n * K + j) * 3;
    phi[j] = q[0]; mu[j] = q[1]; sg[j] = q[2];
    nonfinite = nonfinite || !(fabs(phi[j]) < INF) || !(fabs(mu[j]) < INF) || !(fabs(sg[j]) < INF);
    notpd = notpd || !(fabs(phi[j]) < 1.0) || !(sg[j] > 0.0);
    al[j] = 0.0;
    if (a.alpha0) {
      al[j] = a.alpha0[(size_t)n * K + j];
      nonfinite = nonfinite || !(fabs(al[j]) < INF);
    }
  }
  const bool bad = nonfinite || notpd;
  if (bad && r == 0 && a.status) atomicOr(&a.status[n], nonfinite ? DLM_ST_NONFINITE : DLM_ST_NOT_PD);
  double* out = a.alpha + ((size_t)n * a.R + r) * K * ((size_t)H + 1);
  if (bad) {
    const double nan = __builtin_nan("");
    for (int e = 0; e < K * (H + 1); ++e) out[e] = nan;
    return;
  }
  const unsigned long long series = a.rs.series_offset + (unsigned long long)n;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if (!a.alpha0) {
      const double z = draw_normal(DLM_KEY_SVPATH + (unsigned)j, a.rs.seed, series, a.rs.iteration, DLM_SVPATH_SLOT_START, (unsigned)r);
      al[j] = mu[j] + sg[j] / sqrt(1.0 - phi[j] * phi[j]) * z;
    }
    out[(size_t)j * (H + 1)] = al[j];
  }
  for (int h = 1; h <= H; ++h) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const double z = draw_normal(DLM_KEY_SVPATH + (unsigned)j, a.rs.seed, series, a.rs.iteration, (unsigned)h, (unsigned)r);
      al[j] = mu[j] + phi[j] * (al[j] - mu[j]) + sg[j] * z;
      out[(size_t)j * (H + 1) + h] = al[j];
    }
  }
}

__global__ __launch_bounds__(256) void k_mixture_moments(MixtureArgs a) {
  __shared__ double sS[256], sLo[256], sHi[256];
  __shared__ int sFlag[256];
  const int tid = threadIdx.x, p = a.p, pp = p * p, C = a.C;
  const int n = (int)(blockIdx.x / (unsigned)a.H), h = (int)(blockIdx.x - (unsigned)n * (unsigned)a.H);
  const double INF = __builtin_inf();
  const double* fb = a.f ? a.f + (long long)n * a.f_nstride + (long long)h * a.f_tstride : nullptr;
  const double* qb = a.Q + (long long)n * a.q_nstride + (long long)h * a.q_tstride;
  const int G = pp < 256 ? 256 / pp : 1;
  const int g = pp < 256 ? tid / pp : 0;
  const size_t cell = (size_t)n * a.H + h;
  for (int e0 = 0; e0 < pp; e0 += 256) {   // (one pass when G > 1: p^2 < 256)
    const int e = pp < 256 ? tid - g * pp : e0 + tid;
    const bool act = g < G && e < pp;
    int i = 0, j = 0;
    if (act) { i = e / p; j = e - i * p; }
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    double S = 0.0, Flo = 0.0, Fhi = 0.0;
    int flag = 0;
    if (act) {
      for (int c = g; c < C; c += G) {
        const double* q = qb + (long long)c * a.q_cstride;
        const double qv = q[lo * p + hi], qlo = q[lo * (p + 1)], qhi = q[hi * (p + 1)];
        double flo = 0.0, fhi = 0.0;
        if (fb) {
          const double* f = fb + (long long)c * a.f_cstride;
          flo = f[lo]; fhi = f[hi];
        }
        if (!(qlo > 0.0) || !(qlo < INF) || !(qhi > 0.0) || !(qhi < INF)) flag |= DLM_ST_NOT_PD;
        if (!(fabs(flo) < INF) || !(fabs(fhi) < INF)) flag |= DLM_ST_NONFINITE;
        S = S + (qv + flo * fhi);
        Flo = Flo + flo;
        Fhi = Fhi + fhi;
      }
    }
    if (G > 1) {
      sS[tid] = S; sLo[tid] = Flo; sHi[tid] = Fhi; sFlag[tid] = flag;
      __syncthreads();
      if (act && g == 0) {
        for (int gg = 1; gg < G; ++gg) {
          S = S + sS[e + gg * pp]; Flo = Flo + sLo[e + gg * pp]; Fhi = Fhi + sHi[e + gg * pp]; flag |= sFlag[e + gg * pp];
        }
      }
    }
    if (act && g == 0) {
      const double mlo = Flo / (double)C, mhi = Fhi / (double)C;
      double cv = S / (double)C - mlo * mhi, mn = mlo;
      if (flag) {
        cv = __builtin_nan(""); mn = cv;
        if (a.status) atomicOr(&a.status[n], flag);
      }
      a.cov[cell * pp + e] = cv;
      if (i == j) a.mean[cell * p + i] = mn;
    }
  }
}

// the block's sums of (x, y): wave_sum, then the four waves' in order through the eight doubles at `slot` (the callers alternate two slots,
// so that one barrier per call is enough)
__device__ __forceinline__ void block_sum2(double& x, double& y, double* slot, int tid) {
  x = wave_sum(x); y = wave_sum(y);
  if ((tid & 63) == 0) { slot[(tid >> 6) * 2] = x; slot[(tid >> 6) * 2 + 1] = y; }
  __syncthreads();
  x = ((slot[0] + slot[2]) + slot[4]) + slot[6];
  y = ((slot[1] + slot[3]) + slot[5]) + slot[7];
}

__global__ __launch_bounds__(256) void k_mixture_quantiles(MixtureArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];   // [0, 32): the reductions' slots; behind them the cell's (f, s) pairs when they fit
  const int tid = threadIdx.x, p = a.p, C = a.C, H = a.H;
  const int cell = a.cell_first + (int)blockIdx.x;
  const int i = cell % p, nh = cell / p, h = nh % H, n = nh / H;
  const double INF = __builtin_inf();
  d2* pk = C <= DLM_MIX_LDS_C ? (d2*)(smem + 32) : (d2*)(a.pack + (size_t)blockIdx.x * (size_t)C * 2);
  const double* fb = a.f ? a.f + (long long)n * a.f_nstride + (long long)h * a.f_tstride + i : nullptr;
  const double* qb = a.Q + (long long)n * a.q_nstride + (long long)h * a.q_tstride + (long long)i * (p + 1);
  double fmin = INF, fmax = -INF, smax = 0.0;
  int notpd = 0, nonfinite = 0;
  for (int c = tid; c < C; c += 256) {
    const double q = qb[(long long)c * a.q_cstride];
    const double f = fb ? fb[(long long)c * a.f_cstride] : 0.0;
    if (!(q > 0.0) || !(q < INF)) notpd = 1;
    if (!(fabs(f) < INF)) nonfinite = 1;
    const double s = sqrt(2.0 * q);
    d2 v = {f, s};
    pk[c] = v;
    fmin = fmin < f ? fmin : f; fmax = fmax > f ? fmax : f; smax = smax > s ? smax : s;
  }
  notpd = __syncthreads_or(notpd);
  nonfinite = __syncthreads_or(nonfinite);   // (the barriers also publish the pairs to the block)
  double* qout = a.quant + (size_t)cell * a.nq;
  if (notpd || nonfinite) {
    if (tid < a.nq) qout[tid] = __builtin_nan("");
    if (tid == 0 && a.status) atomicOr(&a.status[n], (notpd ? DLM_ST_NOT_PD : 0) | (nonfinite ? DLM_ST_NONFINITE : 0));
    return;
  }
  fmin = -wave_max(-fmin); fmax = wave_max(fmax); smax = wave_max(smax);
  if ((tid & 63) == 0) { smem[16 + (tid >> 6) * 3] = fmin; smem[17 + (tid >> 6) * 3] = fmax; smem[18 + (tid >> 6) * 3] = smax; }
  __syncthreads();
  for (int w = 0; w < 4; ++w) {
    fmin = fmin < smem[16 + w * 3] ? fmin : smem[16 + w * 3];
    fmax = fmax > smem[17 + w * 3] ? fmax : smem[17 + w * 3];
    smax = smax > smem[18 + w * 3] ? smax : smem[18 + w * 3];
  }
  int parity = 0;
  for (int iq = 0; iq < a.nq; ++iq) {
    const double prob = a.probs[iq];
    const double pad = (fabs(normcdfinv(prob)) + 1.0) * smax;
    double lo = fmin - pad, hi = fmax + pad, x = lo + 0.5 * (hi - lo), res = hi;
    int slow = 0;   // evaluations in a row that did not halve the bracket
    for (int it = 0; it < DLM_MIX_MAX_EVALS; ++it) {
      double sF = 0.0, sD = 0.0;
      for (int c = tid; c < C; c += 256) {
        const d2 v = pk[c];
        const double z = (x - v[0]) / v[1];
        const double ec = 0.5 * erfc(fabs(z));
        sF = sF + (z > 0.0 ? 1.0 - ec : ec);
        sD = sD + exp(-z * z) / v[1];
      }
      block_sum2(sF, sD, smem + parity * 8, tid);
      parity ^= 1;
      const double F = sF / (double)C, D = sD / (double)C * 0.56418958354775628695;   // 1 / sqrt(pi)
      if (F == prob) { res = x; break; }
      const double width = hi - lo;
      if (F < prob) lo = x; else hi = x;
      res = hi;
      if (!(nextafter(lo, INF) < hi)) break;
      slow = hi - lo <= 0.5 * width ? 0 : slow + 1;
      const double step = (F - prob) / D;
      double xn = x - (step + 1e-3 * step);
      if (slow >= 2 || !(xn > lo && xn < hi)) { xn = lo + 0.5 * (hi - lo); slow = 0; }
      if (!(xn > lo && xn < hi)) xn = nextafter(lo, INF);
      x = xn;
    }
    if (tid == 0) qout[iq] = res;
  }
}

hipError_t launch_sv_paths(const SvPathsArgs& a, hipStream_t s) {
  const int chunks = a.R / 64;
  return pick<1, 2, 3, 4, 5, 6, 7, 8>(a.k, [&](auto k) {
    return launch(k_sv_paths<k()>, dim3((unsigned)a.N * (unsigned)chunks), dim3(64), 0, s, a, chunks);
  });
}

hipError_t launch_mixture_moments(const MixtureArgs& a, hipStream_t s) {
  return launch(k_mixture_moments, dim3((unsigned)a.N * (unsigned)a.H), dim3(256), 0, s, a);
}

hipError_t launch_mixture_quantiles(const MixtureArgs& a, int cells, hipStream_t s) {
  const size_t lds = sizeof(double) * (32 + (a.C <= DLM_MIX_LDS_C ? 2 * (size_t)a.C : 0));
  return launch(k_mixture_quantiles, dim3((unsigned)cells), dim3(256), lds, s, a);
}

}  // namespace dlm
