// Posterior-predictive forecast of a dynamic generalised linear model from a particle cloud (Dglm.forecastParticles, Dglm.scala:297-331):
// dlm_pf_forecast_particles.  The layout and the step are k_pf's (dlm_pf.hip): ONE WAVEFRONT PER SERIES, particle i = 64 s + lane, the cloud x[k][i]
// in LDS beside the weights wg, the row `cum`, the ancestors and chol(W).  On top of k_pf's step, at EVERY step and before any weighting, each
// particle draws one observation ytilde_i from the family at eta_i = F^T x_i (dlm_obs_draws.h) into `cum`, which is free between the advance
// and the weighting; their mean is taken in the fixed order of DESIGN.md 4.19 (per lane over its slots, then the xor butterfly), they are
// written out in particle order when asked for, then SORTED IN PLACE in `cum` and the order statistics of the call's ranks are written.  An
// observed step then weighs, accumulates ll, writes the filtering mean and ALWAYS resamples (block 8 of the slot: dlm_pf_batch with n0 > P); a
// missing one carries the cloud on.  The LDS is pf_lds_bytes: nothing beyond k_pf's.
//
// The sort is a bitonic network whose every comparison is ascending (the first substep of a merge compares i with its mirror in the block,
// i ^ (k - 1), the others i with i ^ j): the larger value always goes to the larger index, so the P' - P virtual elements +inf that pad P to the
// next power of two P' never move, and a pair that reaches into them is skipped.  (log2 P')(log2 P' + 1) / 2 passes of P' / 2 pairs, the pairs of
// a pass spread over the lanes, wave_sync between passes; no data-dependent loop bound.  The draws are finite when it runs.
//
// tests/pff_restatement.py restates the draws; the filtering part is bit for bit dlm_pf_batch's (tests/test_pf_forecast_gpu.py).
#include "dlm_obs_draws.h"

namespace dlm {
namespace {

// the two uniforms of block `block` of (slot, particle), and z ~ N(0, I_D): dlm_pf.hip's pf_rand and pf_normals (that file's own, restated
// here so that this kernel's state normals are k_pf's)
template <int D>
__device__ __forceinline__ void fc_normals(const DrawStream& rs, unsigned long long series, unsigned slot, unsigned particle, double (&z)[D]) {
#pragma unroll
  for (int q = 0; q < (D + 1) / 2; ++q) {
    double u1, u2;
    gibbs_rand(rs.seed, series, rs.iteration, slot, particle, 0u, u1, u2, DLM_KEY_PF | (unsigned)q);
    const double r = sqrt(-2.0 * log(u1)), ang = PF_2PI * u2;
    z[2 * q] = r * cos(ang);
    if (2 * q + 1 < D) z[2 * q + 1] = r * sin(ang);
  }
}

template <int D>
__global__ __launch_bounds__(64, D <= 8 ? 2 : 1) void k_pf_forecast(PfForecastArgs a) {
  extern __shared__ double pf_lds[];
  const int n = blockIdx.x, lane = threadIdx.x, P = a.P, T = a.T;
  double* x = pf_lds;              // [D][P]
  double* wg = x + (size_t)D * P;  // [P]
  double* cum = wg + P;            // [P] the draws of a step and their sort, then as in k_pf
  double* sl = cum + P;            // [D][D] row-major
  int* anc = (int*)(sl + D * D);   // [P]
  const unsigned long long series = a.rs.series_offset + (unsigned long long)n;
  const double rP = 1.0 / (double)P;
  const double nan = __builtin_nan("");
  const double* y = a.y + (size_t)n * T;
  double* mean = a.mean ? a.mean + (size_t)n * T * D : nullptr;
  double* fmean = a.fmean + (size_t)n * T;
  double* fquant = a.n_ranks ? a.fquant + (size_t)n * T * a.n_ranks : nullptr;
  double* draws = a.draws ? a.draws + (size_t)n * T * P : nullptr;

  int bad = 0, t_bad = 0;
  double ll = 0.0;

  // ---- the entry cloud: drawn as k_pf draws it, or the caller's (resampled once when it comes with weights); then chol(W)
  if (!a.cloud0) {
    if (!pf_chol<D>(a.C0 + (size_t)n * a.c0_stride, sl, lane)) bad = DLM_ST_NOT_PD;
    if (!bad) {
      pf_init_cloud<D>(a.m0 + (size_t)n * a.m0_stride, sl, x, wg, rP, P, lane,
                       [&](int i, double (&z)[D]) { fc_normals<D>(a.rs, series, DLM_PF_SLOT_INIT, (unsigned)i, z); }, [](int, int) {});
      wave_sync();
    }
  } else {
    const double* c0 = a.cloud0 + (size_t)n * D * P;
    for (int k = 0; k < D; ++k)
      for (int i = lane; i < P; i += 64) x[k * P + i] = c0[(size_t)k * P + i];
    for (int i = lane; i < P; i += 64) wg[i] = a.weights0 ? a.weights0[(size_t)n * P + i] : rP;
    wave_sync();
  }
  if (!bad && !pf_chol<D>(a.W + (size_t)n * a.w_stride, sl, lane)) bad = DLM_ST_NOT_PD;
  if (!bad && a.weights0) {
    double lo = __builtin_inf();
    for (int i = lane; i < P; i += 64) lo = fmin(lo, wg[i]);   // fmin skips a NaN: the total catches it
    const double total = pf_running_sums(wg, cum, P, lane);
    if (!(-wave_max(-lo) >= 0.0) || !(total > 0.0 && total < __builtin_inf())) bad = DLM_ST_NONFINITE;
    else pf_resample(DLM_KEY_PF | DLM_PF_BLOCK_RESAMPLE0, a.rs, series, (unsigned)a.slot_offset, x, D, wg, rP, cum, anc, P, lane);
  }

  if (!bad) {
    const double v = a.V[(size_t)n * a.v_stride], nu = a.obs_param ? a.obs_param[n] : 0.0;
    double dt_held = 0.0;      // Q38, as in k_pf
    for (int t = 0; t < T; ++t) {
      const unsigned slot = (unsigned)(a.slot_offset + t);
      const double yt = y[t];
      const bool missing = yt != yt;
      const double dte = (a.dt ? a.dt[t] : 1.0) + dt_held;
      dt_held = (missing && a.literal && a.n_g == 1) ? dte : 0.0;

      // -- advance: k_pf's loop
      if (dte != 0.0) {
        const double* G = a.G + (size_t)(a.g_index ? a.g_index[t] : 0) * (D * D);
        const double sdt = sqrt(dte);
        for (int i = lane; i < P; i += 64) {
          double z[D], xo[D];
          fc_normals<D>(a.rs, series, slot, (unsigned)i, z);
#pragma unroll
          for (int c = 0; c < D; ++c) xo[c] = x[c * P + i];
#pragma nounroll
          for (int r = 0; r < D; ++r) {
            double gx = G[r] * xo[0];
#pragma unroll
            for (int c = 1; c < D; ++c) gx = gx + G[r + c * D] * xo[c];
            double lz = sl[r * D] * z[0];
#pragma unroll
            for (int c = 1; c < D; ++c) lz = lz + sl[r * D + c] * z[c];
            x[r * P + i] = gx + sdt * lz;
          }
        }
      }

      // -- one observation per particle, before any weighting (Dglm.scala:316-317): the draws into cum, their sum
      const double* F = a.F + (size_t)t * a.f_stride;
      double part = 0.0;
      int finite = 1;
      for (int i = lane; i < P; i += 64) {
        double eta = F[0] * x[i];
#pragma unroll
        for (int k = 1; k < D; ++k) eta = eta + F[k] * x[k * P + i];
        const double yd = pf_obs_draw(a.family, eta, v, nu, PfDrawSite{a.rs.seed, series, a.rs.iteration, slot, (unsigned)i});
        cum[i] = yd;
        part = part + yd;
        if (!(fabs(yd) < __builtin_inf())) finite = 0;
      }
      if (wave_sum_int(finite) != 64) { bad = DLM_ST_NONFINITE; t_bad = t; break; }
      const double fm = wave_sum(part) * rP;
      if (lane == 0) fmean[t] = fm;
      if (draws)
        for (int i = lane; i < P; i += 64) draws[(size_t)t * P + i] = cum[i];
      if (fquant) {
        wave_sync();
        fc_sort(cum, P, lane);
        int rk = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) if (lane == j) rk = a.ranks[j];   // (a select per rank: the ranks are kernel arguments)
        if (lane < a.n_ranks) fquant[(size_t)t * a.n_ranks + lane] = cum[rk];
        wave_sync();
      }

      if (missing) {
        if (mean) pf_means<D>(x, wg, P, lane, mean + (size_t)t * D);
        continue;
      }

      // -- k_pf's weighting of an observed step, then the resampling it does with n0 > P
      const PfObs ob = pf_obs(a.family, a.literal, yt, v, nu);
      double mx = -__builtin_inf();
      for (int i = lane; i < P; i += 64) {
        double eta = F[0] * x[i];
#pragma unroll
        for (int k = 1; k < D; ++k) eta = eta + F[k] * x[k * P + i];
        const double l = pf_logdens(a.family, ob, eta);
        cum[i] = l;
        mx = fmax(mx, l);
      }
      const double m = wave_max(mx);
      if (!(fabs(m) < __builtin_inf())) { bad = DLM_ST_NONFINITE; t_bad = t; break; }
      const double stot = pf_omega(cum, m, wg, a.literal, rP, P, lane);
      if (!(stot > 0.0 && stot < __builtin_inf())) { bad = DLM_ST_NONFINITE; t_bad = t; break; }
      ll = ll + (m + log(stot));
      pf_normalise(wg, stot, P, lane);
      if (mean) pf_means<D>(x, wg, P, lane, mean + (size_t)t * D);
      pf_resample(DLM_KEY_PF | DLM_PF_BLOCK_RESAMPLE, a.rs, series, slot, x, D, wg, rP, cum, anc, P, lane);
    }
  }

  // a step that fails, in its draws or in its weighting, leaves NaN in all of its outputs and in those of the steps after it
  pf_results<D>(a, n, lane, bad, t_bad, ll, x, wg, mean, nullptr, nullptr, nullptr, nullptr, 0);
  if (bad) {
    for (int j = t_bad + lane; j < T; j += 64) fmean[j] = nan;
    if (fquant) for (int j = t_bad * a.n_ranks + lane; j < T * a.n_ranks; j += 64) fquant[j] = nan;
    if (draws) for (size_t j = (size_t)t_bad * P + lane; j < (size_t)T * P; j += 64) draws[j] = nan;
  }
}

}  // namespace

hipError_t launch_pf_forecast(const PfForecastArgs& a, hipStream_t s) {
  return pick<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(a.d, [&](auto D) {
    return launch(k_pf_forecast<decltype(D)::value>, dim3((unsigned)a.N), dim3(64), pf_lds_bytes(a.d, a.P), s, a);
  });
}

}  // namespace dlm
