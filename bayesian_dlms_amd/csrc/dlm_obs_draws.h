// Draws of the six observation models of a DGLM (the `observation` closures of Dglm.scala:46-175): pf_obs_draw is the sampling counterpart of
// dlm_pf_common.h's pf_logdens, with its parameterisation.  Used by the two forecast kernels alone (dlm_pf_forecast.hip's k_pf_forecast,
// dlm_pf_forecast_learned.hip's k_pf_forecast_learned), with the sort of a step's draws at its end: the five filtering kernels
// do not include this file, and dlm_pf_common.h is as it was.  tests/pff_restatement.py restates every function here operation for operation.
//
// Randomness: Philox under DLM_KEY_PF in the particle filter's counter layout (seed, series, iteration, slot, particle).  The particle
// occupies the counter's attempt field, so the attempts of a rejection sampler are BLOCKS (the key's low byte, dlm_draws.h):
//   DLM_PF_BLOCK_OBS           (u1, u2): the Box-Muller cosine z of the Gaussian and Student-t families; u1 the zero-inflation uniform of ZIP;
//                              u2 the inversion uniform of a Poisson rate below PF_POISSON_PTRS_FROM
//   DLM_PF_BLOCK_POISSON + j   attempt j of the transformed rejection: u2 - 0.5 its U, u1 its V
//   DLM_PF_BLOCK_GAMMA_A + j   attempt j of the first Gamma of a draw (which 0: the normal's pair, which 1: the accept uniform), j = DLM_PF_GAMMA_ATTEMPTS the boost
//   DLM_PF_BLOCK_GAMMA_B + j   the same for the second Gamma (Beta's)
// EVERY LOOP HAS A CONSTANT BOUND:
//   Poisson, rate < 10     sequential inversion of ONE uniform, at most PF_POISSON_INVERSION_STEPS = 128 steps (P(X >= 128 | rate 10) < 1e-90); it
//                          also ends where the running sum stops growing, and returns the count reached
//   Poisson, rate >= 10    PTRS: W. Hoermann, "The transformed rejection method for generating Poisson random variables", Insurance: Mathematics and
//                          Economics 12 (1993) 39-45, valid from a rate of 10 on, exact; DLM_PF_POISSON_ATTEMPTS = 32 attempts (each accepts with a
//                          probability above 0.8: all fail with less than 1e-22), then floor(rate), the mode
//   Gamma                  Marsaglia & Tsang through dlm_draws.h's gamma_unit_from, DLM_PF_GAMMA_ATTEMPTS = 32 attempts (each accepts with more than
//                          0.95: all fail with less than 1e-41), then its d = a - 1/3 (times the boost)
// A rate that is not finite, negative or above PF_RATE_MAX = 1e15, a NegBin size that is not positive and finite and Beta parameters that are not
// positive (Q41) give NaN: the kernel stops the series with DLM_ST_NONFINITE, as it does for any draw that is not finite.
// pf_gamma_draw and pf_poisson_draw are ONE __noinline__ copy each, as pf_lgamma is: inlined at their call sites in the six
// families they would be held in registers across the loop over the particles.  That is k_pf_forecast's trade, whose weighting loop is live beside
// them.  k_pf_forecast_learned has no weighting and takes the bodies inlined (pf_obs_draw<true>): no call frames, so no scratch,
// and fewer registers than with the calls.
#pragma once
#include "dlm_pf_common.h"

namespace dlm {
namespace {

constexpr double PF_POISSON_PTRS_FROM = 10.0, PF_RATE_MAX = 1e15;
constexpr int PF_POISSON_INVERSION_STEPS = 128;

// where a draw takes its uniforms from: the `source` of pf_obs_draw
struct PfDrawSite { unsigned long long seed, series, iteration; unsigned slot, particle; };

__device__ __forceinline__ void pf_site_rand(const PfDrawSite& s, unsigned block, unsigned which, double& u1, double& u2) {
  gibbs_rand(s.seed, s.series, s.iteration, s.slot, s.particle, which, u1, u2, DLM_KEY_PF | block);
}

// Gamma(a, 1) from the blocks base .. base + DLM_PF_GAMMA_ATTEMPTS: the body, and the ONE __noinline__ copy of it
__device__ __forceinline__ double pf_gamma_draw_body(double a, unsigned base, const PfDrawSite& s) {
  return gamma_unit_from(a, DLM_PF_GAMMA_ATTEMPTS,
                         [&](unsigned attempt, unsigned which, double& u1, double& u2) { pf_site_rand(s, base + attempt, which, u1, u2); });
}
__device__ __noinline__ double pf_gamma_draw(double a, unsigned base, PfDrawSite s) { return pf_gamma_draw_body(a, base, s); }

// Poisson(lam), exactly; NaN for a rate outside [0, PF_RATE_MAX]: the body, and below it the ONE __noinline__ copy of it
__device__ __forceinline__ double pf_poisson_draw_body(double lam, const PfDrawSite& s) {
  if (!(lam >= 0.0 && lam <= PF_RATE_MAX)) return __builtin_nan("");
  if (lam < PF_POISSON_PTRS_FROM) {
    double u1, u;
    pf_site_rand(s, DLM_PF_BLOCK_OBS, 0u, u1, u);
    double p = exp(-lam), cdf = p;
    int k = 0;
    for (int j = 1; j <= PF_POISSON_INVERSION_STEPS; ++j) {
      if (u < cdf) break;
      p = (p * lam) / (double)j;
      const double next = cdf + p;
      if (next == cdf) break;
      cdf = next;
      k = j;
    }
    return (double)k;
  }
  const double slam = sqrt(lam), loglam = log(lam);
  const double b = 0.931 + 2.53 * slam, a = -0.059 + 0.02483 * b;
  const double invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
  for (unsigned j = 0; j < DLM_PF_POISSON_ATTEMPTS; ++j) {
    double V, u2;
    pf_site_rand(s, DLM_PF_BLOCK_POISSON + j, 0u, V, u2);
    const double U = u2 - 0.5, us = 0.5 - fabs(U);
    const double k = floor((((2.0 * a) / us + b) * U + lam) + 0.43);
    if (us >= 0.07 && V <= vr) return k;
    if (k < 0.0 || (us < 0.013 && V > us)) continue;
    if ((log(V) + log(invalpha)) - log(a / (us * us) + b) <= (k * loglam - lam) - pf_lgamma(k + 1.0)) return k;
  }
  return floor(lam);
}
__device__ __noinline__ double pf_poisson_draw(double lam, PfDrawSite s) { return pf_poisson_draw_body(lam, s); }

// one draw of y | eta, v (nu: the degrees of freedom of DLM_OBS_STUDENTT), pf_logdens's parameterisation.  INLINE: the Gamma and Poisson draws
// are inlined into the caller instead of called (k_pf_forecast_learned: a call's frame is scratch); the arithmetic is the same
template <bool INLINE = false>
__device__ __forceinline__ double pf_obs_draw(int family, double eta, double v, double nu, const PfDrawSite& s) {
  const double nan = __builtin_nan("");
  auto pf_gamma_draw = [](double a, unsigned base, const PfDrawSite& at) {
    if constexpr (INLINE) return pf_gamma_draw_body(a, base, at); else return dlm::pf_gamma_draw(a, base, at);
  };
  auto pf_poisson_draw = [](double lam, const PfDrawSite& at) {
    if constexpr (INLINE) return pf_poisson_draw_body(lam, at); else return dlm::pf_poisson_draw(lam, at);
  };
  switch (family) {
    case DLM_OBS_GAUSSIAN: {
      double u1, u2;
      pf_site_rand(s, DLM_PF_BLOCK_OBS, 0u, u1, u2);
      return eta + sqrt(v) * (sqrt(-2.0 * log(u1)) * cos(PF_2PI * u2));
    }
    case DLM_OBS_POISSON: return pf_poisson_draw(exp(eta), s);
    case DLM_OBS_NEGBIN: {   // Dglm.scala:102-109: Poisson(Gamma(size, 1) mu / size)
      const double size = exp(v), mu = exp(eta);
      if (!(size > 0.0 && size < __builtin_inf())) return nan;
      const double g = pf_gamma_draw(size, DLM_PF_BLOCK_GAMMA_A, s);
      return pf_poisson_draw((g * mu) / size, s);
    }
    case DLM_OBS_ZIP: {
      const double ev = exp(v), p0 = ev / (1.0 + ev), lam = exp(eta);
      if (!(lam <= PF_RATE_MAX)) return nan;
      double u1, u2;
      pf_site_rand(s, DLM_PF_BLOCK_OBS, 0u, u1, u2);
      if (u1 < p0) return 0.0;
      return pf_poisson_draw(lam, s);
    }
    case DLM_OBS_STUDENTT: {   // ScaledStudentT.scala:19-28: N(eta, w), w ~ InverseGamma(nu / 2, nu v / 2)
      double u1, u2;
      pf_site_rand(s, DLM_PF_BLOCK_OBS, 0u, u1, u2);
      const double g = pf_gamma_draw(nu * 0.5, DLM_PF_BLOCK_GAMMA_A, s);
      const double w = ((nu * v) * 0.5) / g;
      return eta + sqrt(w) * (sqrt(-2.0 * log(u1)) * cos(PF_2PI * u2));
    }
    default: {   // DLM_OBS_BETA: (mean, variance) -> (alpha, beta) as pf_logdens
      const double mean = eta < -5.0 ? 0.0 : (eta > 5.0 ? 1.0 : 1.0 / (1.0 + exp(-eta)));
      const double aa = (mean * (1.0 - mean)) / v;
      const double al = mean * (aa - 1.0), be = (1.0 - mean) * (aa - 1.0);
      if (!(al > 0.0 && be > 0.0 && al < __builtin_inf() && be < __builtin_inf())) return nan;   // Q41
      const double ga = pf_gamma_draw(al, DLM_PF_BLOCK_GAMMA_A, s), gb = pf_gamma_draw(be, DLM_PF_BLOCK_GAMMA_B, s);
      return ga / (ga + gb);
    }
  }
}

// ---- the sort of a step's draws, in place in an LDS row (k_pf_forecast and k_pf_forecast_learned; described at the head of dlm_pf_forecast.hip) ----
// compare-exchange of the sort: the smaller value to the smaller index; a partner among the virtual +inf is skipped
__device__ __forceinline__ void fc_cmpx(double* v, int i, int l, int P) {
  if (l < P) {
    const double a = v[i], b = v[l];
    if (a > b) { v[i] = b; v[l] = a; }
  }
}

// v[0 .. P) ascending, P a multiple of 64 (any: P2 is the next power of two)
__device__ __forceinline__ void fc_sort(double* v, int P, int lane) {
  int P2 = 64;
  while (P2 < P) P2 <<= 1;   // at most four doublings: P <= 1024
  const int half = P2 >> 1;
  for (int k = 2; k <= P2; k <<= 1) {
    const int hk = k >> 1;
    for (int t = lane; t < half; t += 64) {   // the mirror substep
      const int blk = t / hk, off = t - blk * hk;
      fc_cmpx(v, blk * k + off, blk * k + (k - 1 - off), P);
    }
    wave_sync();
    for (int j = hk >> 1; j >= 1; j >>= 1) {
      for (int t = lane; t < half; t += 64) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        fc_cmpx(v, i, i | j, P);
      }
      wave_sync();
    }
  }
}

}  // namespace
}  // namespace dlm
