// Bootstrap particle filter of a dynamic generalised linear model (ParticleFilter.step / likelihood, ParticleFilter.scala:38-85; the observation
// models of Dglm.scala:46-175 and package.scala:13-28): dlm_pf_batch.  ONE WAVEFRONT PER SERIES.  Particle i = 64 s + lane sits in slot s of
// its lane, S = P / 64 slots.  The cloud lives in LDS, component-major x[k][i] -- a lane's accesses are 64 consecutive doubles per slot, free of
// bank conflicts -- next to the weights wg[i], one more row `cum` (the log-weights of a step, then the running sums of the resampling search,
// then the row a component is gathered through), the ancestors and ONE d x d factor (chol(C0) for the initial cloud, chol(W) from then on).
// A particle's state is in registers only while it is advanced: the template argument D makes those arrays registers.
//
// Every reduction runs in a FIXED order (tests/pf_restatement.py follows them operation for operation):
//   max, sum of omega, sum of W^2, weighted means   per lane over its slots s = 0 .. S - 1 in order, then across the lanes: wave_max (a maximum
//                                                   has no order) or the xor butterfly wave_sum (partners 32, 16, 8, 4, 2, 1);
//   inclusive running sums of the weights           per slot the Hillis-Steele scan over the lanes (offsets 1, 2, 4, 8, 16, 32: v = v + v[lane - off]),
//                                                   plus the carry = the running sum at the previous slot's lane 63 (carry + v);
//   matrix-vector products                          index ascending from 0, the first product starts the sum.
// No atomics, no dependence on N or on the neighbours.  The initial cloud, the weights from the log-weights, the resampling and the results
// of a series are dlm_pf_common.h's, shared with k_storvik and k_lw; the paired normals pf_normals, which draw each Philox block once, are
// this kernel's own.
//
// dlm_pf_resampled chooses the ancestor step of the resampling (PfSchemeArgs::resample, DLM_RESAMPLE_*).  The multinomial scheme runs
// k_pf, dlm_pf_batch's kernel as it was; the three others run k_pf_scheme, the same step with pf_resample_by at the resampling site: one
// branch there, the same in every lane, none in the advance or the weighting, and no LDS beyond the rows above -- the Metropolis chains read
// wg and write anc, the stratified and systematic searches read cum as the multinomial one does.  DESIGN.md 4.27;
// tests/pf_resample_restatement.py follows them.
#include "dlm_pf_common.h"

namespace dlm {
namespace {

// the two uniforms of block `block` of (slot, particle): u1 in (0, 1], u2 in [0, 1)
__device__ __forceinline__ void pf_rand(const DrawStream& rs, unsigned long long series, unsigned slot, unsigned particle, unsigned block,
                                        double& u1, double& u2) {
  gibbs_rand(rs.seed, series, rs.iteration, slot, particle, 0u, u1, u2, DLM_KEY_PF | block);
}

// z ~ N(0, I_D) of (slot, particle): block q gives the components 2 q (cosine) and 2 q + 1 (sine)
template <int D>
__device__ __forceinline__ void pf_normals(const DrawStream& rs, unsigned long long series, unsigned slot, unsigned particle, double (&z)[D]) {
#pragma unroll
  for (int q = 0; q < (D + 1) / 2; ++q) {
    double u1, u2;
    pf_rand(rs, series, slot, particle, (unsigned)q, u1, u2);
    const double r = sqrt(-2.0 * log(u1)), ang = PF_2PI * u2;
    z[2 * q] = r * cos(ang);
    if (2 * q + 1 < D) z[2 * q + 1] = r * sin(ang);
  }
}

template <int D>
__global__ __launch_bounds__(64, D <= 8 ? 2 : 1) void k_pf(PfArgs a) {
  extern __shared__ double pf_lds[];
  const int n = blockIdx.x, lane = threadIdx.x, P = a.P, T = a.T;
  double* x = pf_lds;              // [D][P]
  double* wg = x + (size_t)D * P;  // [P] the normalised weights W_t,i
  double* cum = wg + P;            // [P]
  double* sl = cum + P;            // [D][D] row-major
  int* anc = (int*)(sl + D * D);   // [P]
  const unsigned long long series = a.rs.series_offset + (unsigned long long)n;
  const double rP = 1.0 / (double)P;
  const double* y = a.y + (size_t)n * T;
  double* mean = a.mean ? a.mean + (size_t)n * T * D : nullptr;
  double* ess = a.ess ? a.ess + (size_t)n * T : nullptr;

  int bad = 0, t_bad = 0;   // status bits of the series; the first step without results
  double ll = 0.0;

  // ---- the initial cloud x_0,i = m0 + chol(C0) z, then chol(W) for the steps
  if (!pf_chol<D>(a.C0 + (size_t)n * a.c0_stride, sl, lane)) bad = DLM_ST_NOT_PD;
  if (!bad) {
    pf_init_cloud<D>(a.m0 + (size_t)n * a.m0_stride, sl, x, wg, rP, P, lane,
                     [&](int i, double (&z)[D]) { pf_normals<D>(a.rs, series, DLM_PF_SLOT_INIT, (unsigned)i, z); }, [](int, int) {});
    wave_sync();
    if (!pf_chol<D>(a.W + (size_t)n * a.w_stride, sl, lane)) bad = DLM_ST_NOT_PD;
  }

  if (!bad) {
    const double v = a.V[(size_t)n * a.v_stride], nu = a.obs_param ? a.obs_param[n] : 0.0;
    double dt_held = 0.0;      // Q38, literal with one G: the intervals of the missing steps since the last observation
    double ess_last = (double)P;
    for (int t = 0; t < T; ++t) {
      const double yt = y[t];
      const bool missing = yt != yt;
      const double dte = (a.dt ? a.dt[t] : 1.0) + dt_held;
      dt_held = (missing && a.literal && a.n_g == 1) ? dte : 0.0;

      // -- advance: x <- G x + sqrt(dt) L z (dt == 0: no advance, no noise)
      if (dte != 0.0) {
        const double* G = a.G + (size_t)(a.g_index ? a.g_index[t] : 0) * (D * D);
        const double sdt = sqrt(dte);
        for (int i = lane; i < P; i += 64) {
          double z[D], xo[D];
          pf_normals<D>(a.rs, series, (unsigned)t, (unsigned)i, z);
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

      if (missing) {
        if (mean) pf_means<D>(x, wg, P, lane, mean + (size_t)t * D);
        if (ess && lane == 0) ess[t] = ess_last;
        continue;
      }

      // -- log-weights, their maximum
      const PfObs ob = pf_obs(a.family, a.literal, yt, v, nu);
      const double* F = a.F + (size_t)t * a.f_stride;
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

      // -- omega_i = W_{t-1,i} exp(l_i - m), their sum; W_t,i = omega_i / s, sum W^2, the filtering mean
      const double stot = pf_omega(cum, m, wg, a.literal, rP, P, lane);
      if (!(stot > 0.0 && stot < __builtin_inf())) { bad = DLM_ST_NONFINITE; t_bad = t; break; }
      ll = ll + (m + log(stot));
      const double sq = pf_normalise(wg, stot, P, lane);
      if (mean) pf_means<D>(x, wg, P, lane, mean + (size_t)t * D);
      ess_last = floor(1.0 / sq);
      if (ess && lane == 0) ess[t] = ess_last;
      if (!(ess_last < (double)a.n0)) continue;

      pf_resample(DLM_KEY_PF | DLM_PF_BLOCK_RESAMPLE, a.rs, series, (unsigned)t, x, D, wg, rP, cum, anc, P, lane);   // component by component
    }
  }

  pf_results<D>(a, n, lane, bad, t_bad, ll, x, wg, mean, ess, nullptr, nullptr, nullptr, 0);
}

// k_pf under a scheme other than DLM_RESAMPLE_MULTINOMIAL: k_pf's text with pf_resample_by where k_pf has pf_resample.  A kernel of its
// own and a copy, not a branch in k_pf or a body both kernels call: the scheme read at run time costs k_pf 2 to 3 registers at every D and
// 2 % of a call at P = 64, and a shared body, by reference or by value, moves k_pf's register count at some D (profiles/r31_notes.md) --
// dlm_pf_batch is to stay what it was, bit for bit and register for register (tests/test_lw_host.py pins the counts).  A change to the
// step goes into both
template <int D>
__global__ __launch_bounds__(64, D <= 8 ? 2 : 1) void k_pf_scheme(PfSchemeArgs a) {
  extern __shared__ double pf_lds[];
  const int n = blockIdx.x, lane = threadIdx.x, P = a.P, T = a.T;
  double* x = pf_lds;              // [D][P]
  double* wg = x + (size_t)D * P;  // [P] the normalised weights W_t,i
  double* cum = wg + P;            // [P]
  double* sl = cum + P;            // [D][D] row-major
  int* anc = (int*)(sl + D * D);   // [P]
  const unsigned long long series = a.rs.series_offset + (unsigned long long)n;
  const double rP = 1.0 / (double)P;
  const double* y = a.y + (size_t)n * T;
  double* mean = a.mean ? a.mean + (size_t)n * T * D : nullptr;
  double* ess = a.ess ? a.ess + (size_t)n * T : nullptr;

  int bad = 0, t_bad = 0;   // status bits of the series; the first step without results
  double ll = 0.0;

  // ---- the initial cloud x_0,i = m0 + chol(C0) z, then chol(W) for the steps
  if (!pf_chol<D>(a.C0 + (size_t)n * a.c0_stride, sl, lane)) bad = DLM_ST_NOT_PD;
  if (!bad) {
    pf_init_cloud<D>(a.m0 + (size_t)n * a.m0_stride, sl, x, wg, rP, P, lane,
                     [&](int i, double (&z)[D]) { pf_normals<D>(a.rs, series, DLM_PF_SLOT_INIT, (unsigned)i, z); }, [](int, int) {});
    wave_sync();
    if (!pf_chol<D>(a.W + (size_t)n * a.w_stride, sl, lane)) bad = DLM_ST_NOT_PD;
  }

  if (!bad) {
    const double v = a.V[(size_t)n * a.v_stride], nu = a.obs_param ? a.obs_param[n] : 0.0;
    double dt_held = 0.0;      // Q38, literal with one G: the intervals of the missing steps since the last observation
    double ess_last = (double)P;
    for (int t = 0; t < T; ++t) {
      const double yt = y[t];
      const bool missing = yt != yt;
      const double dte = (a.dt ? a.dt[t] : 1.0) + dt_held;
      dt_held = (missing && a.literal && a.n_g == 1) ? dte : 0.0;

      // -- advance: x <- G x + sqrt(dt) L z (dt == 0: no advance, no noise)
      if (dte != 0.0) {
        const double* G = a.G + (size_t)(a.g_index ? a.g_index[t] : 0) * (D * D);
        const double sdt = sqrt(dte);
        for (int i = lane; i < P; i += 64) {
          double z[D], xo[D];
          pf_normals<D>(a.rs, series, (unsigned)t, (unsigned)i, z);
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

      if (missing) {
        if (mean) pf_means<D>(x, wg, P, lane, mean + (size_t)t * D);
        if (ess && lane == 0) ess[t] = ess_last;
        continue;
      }

      // -- log-weights, their maximum
      const PfObs ob = pf_obs(a.family, a.literal, yt, v, nu);
      const double* F = a.F + (size_t)t * a.f_stride;
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

      // -- omega_i = W_{t-1,i} exp(l_i - m), their sum; W_t,i = omega_i / s, sum W^2, the filtering mean
      const double stot = pf_omega(cum, m, wg, a.literal, rP, P, lane);
      if (!(stot > 0.0 && stot < __builtin_inf())) { bad = DLM_ST_NONFINITE; t_bad = t; break; }
      ll = ll + (m + log(stot));
      const double sq = pf_normalise(wg, stot, P, lane);
      if (mean) pf_means<D>(x, wg, P, lane, mean + (size_t)t * D);
      ess_last = floor(1.0 / sq);
      if (ess && lane == 0) ess[t] = ess_last;
      if (!(ess_last < (double)a.n0)) continue;

      pf_resample_by(a.resample, a.mh_steps, DLM_KEY_PF, DLM_PF_BLOCK_RESAMPLE, DLM_PF_BLOCK_MH0, a.rs, series, (unsigned)t, x, D, wg, rP, cum,
                     anc, P, lane);
    }
  }

  pf_results<D>(a, n, lane, bad, t_bad, ll, x, wg, mean, ess, nullptr, nullptr, nullptr, 0);
}

}  // namespace

size_t pf_lds_bytes(int d, int P) { return ((size_t)(d + 2) * P + (size_t)d * d) * sizeof(double) + (size_t)P * sizeof(int); }

hipError_t launch_pf(const PfSchemeArgs& a, hipStream_t s) {
  return pick<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(a.d, [&](auto D) {
    constexpr int d = decltype(D)::value;
    if (a.resample == DLM_RESAMPLE_MULTINOMIAL) return launch(k_pf<d>, dim3((unsigned)a.N), dim3(64), pf_lds_bytes(a.d, a.P), s, (const PfArgs&)a);
    return launch(k_pf_scheme<d>, dim3((unsigned)a.N), dim3(64), pf_lds_bytes(a.d, a.P), s, a);
  });
}

}  // namespace dlm
