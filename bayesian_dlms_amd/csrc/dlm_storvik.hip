// Storvik filter of a dynamic generalised linear model (StorvikFilter.step, Storvik.scala:105-159; Storvik 2002): a particle filter whose
// particles carry the sufficient statistics of the Inverse-Gamma posteriors of their own variances -- the diagonal of W, and V for the
// Gaussian family -- and draw those variances afresh at every step: dlm_storvik_batch.  The layout is k_pf's (dlm_pf.hip): ONE WAVEFRONT PER
// SERIES, particle i = 64 s + lane, everything in LDS, component-major:
//   x [D][P] the cloud | bw [D][P] the scales of the W statistics | bv [P] the scale of the V statistic | wg [P] | cum [P] | sl [D][D] | anc [P] (int)
// = (2 d + 3.5) P + d^2 doubles.  The SHAPES of the statistics are not per particle: every particle gets the same increments, so
// aw_k = prior shape + 0.5 (advances so far) and av = prior shape + 0.5 (observations so far) are scalars of the series, formed by that one
// addition where they are used.  x, bw and bv lie behind one another so that the resampling gathers a particle's whole tuple as 2 d + 1 rows.
//
// The statistics are updated BEFORE the gather, on the particle that made the move: x_{t-1} and x_t of an update are always one particle's
// own (the reference pairs the old cloud with the resampled one, Storvik.scala:139-141, Q42).
//
// The orders of every sum are DESIGN.md 4.19's; the initial cloud (the statistics at their priors are its extra rows), the normals, the weights
// from the log-weights, the resampling and the results of a series are dlm_pf_common.h's.  scale_mean sums like the means.  tests/storvik_restatement.py follows the
// kernel operation for operation.
#include "dlm_pf_common.h"

namespace dlm {
namespace {

// the two uniforms of (slot, particle, block, attempt, which): u1 in (0, 1], u2 in [0, 1)
__device__ __forceinline__ void st_rand(unsigned long long seed, unsigned long long series, unsigned long long iteration, unsigned slot,
                                        unsigned particle, unsigned block, unsigned attempt, unsigned which, double& u1, double& u2) {
  gibbs_rand(seed, series, iteration, slot, particle, which, u1, u2, DLM_KEY_STORVIK | (attempt << 8) | block);
}

// Gamma(shape, 1) of component comp (k < d: W_kk, d: V) of (slot, particle).  The kernel has ONE call site of it, the row loop of a step:
// a second one doubles the rejection loop's registers, and as a function of its own it saves a register to scratch
__device__ __forceinline__ double st_gamma(double shape, const DrawStream& rs, unsigned long long series, unsigned slot, unsigned particle,
                                           unsigned comp) {
  return gamma_unit_from(shape, DLM_STORVIK_GAMMA_ATTEMPTS, [&](unsigned attempt, unsigned which, double& u1, double& u2) {
    st_rand(rs.seed, series, rs.iteration, slot, particle, DLM_STORVIK_BLOCK_GAMMA + comp, attempt, which, u1, u2);
  });
}

template <int D>
__global__ __launch_bounds__(64, D <= 8 ? 2 : 1) void k_storvik(StorvikArgs a) {
  extern __shared__ double st_lds[];
  const int n = blockIdx.x, lane = threadIdx.x, P = a.P, T = a.T;
  double* x = st_lds;               // [D][P]
  double* bw = x + (size_t)D * P;   // [D][P] the scale of the InverseGamma of W_kk
  double* bv = bw + (size_t)D * P;  // [P]    the scale of the InverseGamma of V (learn_v)
  double* wg = bv + P;              // [P] the normalised weights W_t,i
  double* cum = wg + P;             // [P]
  double* sl = cum + P;             // [D][D] row-major chol(C0)
  int* anc = (int*)(sl + D * D);    // [P]
  const unsigned long long series = a.rs.series_offset + (unsigned long long)n;
  const double rP = 1.0 / (double)P, nan = __builtin_nan("");
  const double* y = a.y + (size_t)n * T;
  const double* pw = a.prior_w + (size_t)n * a.prior_w_stride;                        // [D][2]: shape, scale
  const double* pv = a.learn_v ? a.prior_v + (size_t)n * a.prior_v_stride : nullptr;  // [2]
  double* mean = a.mean ? a.mean + (size_t)n * T * D : nullptr;
  double* smean = a.scale_mean ? a.scale_mean + (size_t)n * T * (D + 1) : nullptr;
  double* ess = a.ess ? a.ess + (size_t)n * T : nullptr;

  int bad = 0, t_bad = 0;   // status bits of the series; the first step without results
  double ll = 0.0;

  // the means of a step under the weights it leaves: the state, the scales of W, the scale of V
  auto outputs = [&](int t) {
    if (mean) pf_means<D>(x, wg, P, lane, mean + (size_t)t * D);
    if (smean) {
      pf_means<D>(bw, wg, P, lane, smean + (size_t)t * (D + 1));
      if (a.learn_v) pf_means<1>(bv, wg, P, lane, smean + (size_t)t * (D + 1) + D);
      else if (lane == 0) smean[(size_t)t * (D + 1) + D] = nan;
    }
  };

  // ---- the priors, the initial cloud x_0,i = m0 + chol(C0) z, the statistics at their priors
  for (int k = 0; k < D; ++k)
    if (!(pw[2 * k] > 0.0 && pw[2 * k + 1] > 0.0)) bad = DLM_ST_NOT_PD;
  if (a.learn_v && !(pv[0] > 0.0 && pv[1] > 0.0)) bad = DLM_ST_NOT_PD;
  if (!pf_chol<D>(a.C0 + (size_t)n * a.c0_stride, sl, lane)) bad = DLM_ST_NOT_PD;
  if (!bad) {
    const double bv0 = a.learn_v ? pv[1] : 0.0;
    pf_init_cloud<D>(a.m0 + (size_t)n * a.m0_stride, sl, x, wg, rP, P, lane,
                     [&](int i, double (&z)[D]) {
#pragma unroll
                       for (int c = 0; c < D; ++c) z[c] = pf_normal(DLM_KEY_STORVIK, a.rs, series, DLM_STORVIK_SLOT_INIT, (unsigned)i, 0u, c);
                     },
                     [&](int r, int i) { bw[r * P + i] = r < D ? pw[2 * r + 1] : bv0; });   // (row D of bw is bv)
    wave_sync();
  }

  if (!bad) {
    const double vfix = a.learn_v ? 1.0 : a.V[(size_t)n * a.v_stride], nu = a.obs_param ? a.obs_param[n] : 0.0;
    int n_adv = 0, n_obs = 0;   // the advances and the updates of V so far: the shapes are the prior's + 0.5 of them
    double ess_last = (double)P;
    for (int t = 0; t < T; ++t) {
      const double yt = y[t];
      const bool missing = yt != yt;
      const double dte = a.dt ? a.dt[t] : 1.0;

      // -- one pass over the particles, rows r < D the ADVANCE of component r (dt == 0: none),
      //      w_r ~ InverseGamma(aw_r, bw_r),  x_r <- (G x)_r + sqrt(dt w_r) z_r,  bw_r += 0.5 (x_r - (G x)_r)^2 / dt,
      //    row D the WEIGHT (a missing y: none),
      //      v ~ InverseGamma(av, bv) (learn_v),  l = log p(y | F^T x, v),  bv += 0.5 (y - F^T x)^2.
      //    The rows are one loop so that the Gamma has its one call site; the normal and the Gamma of a row are drawn in it (z[r] of a loop
      //    that is not unrolled is scratch).
      const bool adv = dte != 0.0;
      const double* G = a.G + (size_t)(a.g_index ? a.g_index[t] : 0) * (D * D);
      const double* F = a.F + (size_t)t * a.f_stride;
      const double hadv = 0.5 * (double)n_adv, hobs = 0.5 * (double)n_obs;
      const PfObs ob = pf_obs(a.family, a.literal, missing ? 1.0 : yt, vfix, nu);   // (a missing y: not used; the 1.0 keeps lgamma off a NaN)
      double mx = -__builtin_inf();
      for (int i = lane; i < P; i += 64) {
        double xo[D];
#pragma unroll
        for (int c = 0; c < D; ++c) xo[c] = x[c * P + i];
#pragma nounroll
        for (int r = (adv ? 0 : D); r < (missing ? D : D + 1); ++r) {
          const bool state = r < D;
          double g = 1.0;
          if (state || a.learn_v) g = st_gamma(state ? pw[2 * r] + hadv : pv[0] + hobs, a.rs, series, (unsigned)t, (unsigned)i, (unsigned)r);
          if (state) {
            double gx = G[r] * xo[0];
#pragma unroll
            for (int c = 1; c < D; ++c) gx = gx + G[r + c * D] * xo[c];
            const double z = pf_normal(DLM_KEY_STORVIK, a.rs, series, (unsigned)t, (unsigned)i, 0u, r);
            const double b = bw[r * P + i];
            const double w = b / g;
            const double xn = gx + sqrt(dte * w) * z;
            const double e = xn - gx;
            bw[r * P + i] = b + (0.5 * (e * e)) / dte;
            x[r * P + i] = xn;
          } else {
            double eta = F[0] * x[i];
#pragma unroll
            for (int k = 1; k < D; ++k) eta = eta + F[k] * x[k * P + i];
            PfObs o = ob;
            if (a.learn_v) {
              const double b = bv[i], e = yt - eta;
              o = pf_obs(DLM_OBS_GAUSSIAN, 0, yt, b / g, nu);
              bv[i] = b + 0.5 * (e * e);
            }
            const double l = pf_logdens(a.family, o, eta);
            cum[i] = l;
            mx = fmax(mx, l);
          }
        }
      }
      if (adv) ++n_adv;

      if (missing) {
        outputs(t);
        if (ess && lane == 0) ess[t] = ess_last;
        continue;
      }
      if (a.learn_v) ++n_obs;
      const double m = wave_max(mx);
      if (!(fabs(m) < __builtin_inf())) { bad = DLM_ST_NONFINITE; t_bad = t; break; }

      // -- omega_i = W_{t-1,i} exp(l_i - m), their sum; W_t,i = omega_i / s, sum W^2, the means
      const double stot = pf_omega(cum, m, wg, a.literal, rP, P, lane);
      if (!(stot > 0.0 && stot < __builtin_inf())) { bad = DLM_ST_NONFINITE; t_bad = t; break; }
      ll = ll + (m + log(stot));
      const double sq = pf_normalise(wg, stot, P, lane);
      outputs(t);
      ess_last = floor(1.0 / sq);
      if (ess && lane == 0) ess[t] = ess_last;
      if (!(ess_last < (double)a.n0)) continue;

      // -- multinomial resampling of the whole tuple (x, bw, bv)
      pf_resample(DLM_KEY_STORVIK | DLM_STORVIK_BLOCK_RESAMPLE, a.rs, series, (unsigned)t, x, 2 * D + (a.learn_v ? 1 : 0), wg, rP, cum, anc, P, lane);
    }
  }

  pf_results<D>(a, n, lane, bad, t_bad, ll, x, wg, mean, ess, smean, nullptr, a.scales, D + (a.learn_v ? 1 : 0));
}

}  // namespace

size_t storvik_lds_bytes(int d, int P) { return ((size_t)(2 * d + 3) * P + (size_t)d * d) * sizeof(double) + (size_t)P * sizeof(int); }

hipError_t launch_storvik(const StorvikArgs& a, hipStream_t s) {
  return pick<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(a.d, [&](auto D) {
    return launch(k_storvik<decltype(D)::value>, dim3((unsigned)a.N), dim3(64), storvik_lds_bytes(a.d, a.P), s, a);
  });
}

}  // namespace dlm
