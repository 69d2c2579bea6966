// What the particle kernels share (dlm_pf.hip: k_pf, dlm_storvik.hip: k_storvik), each defined here ONCE: the Cholesky factor of the initial
// cloud, the six observation densities of Dglm.scala:46-175, the weighted means over the particles, and the running sums and the search of
// the multinomial resampling.  One wavefront per series, particle i = 64 s + lane, rows of P doubles in LDS; the orders of every sum are
// those of DESIGN.md 4.19.
#pragma once
#include "dlm_wave.h"
#include "dlm_draws.h"

namespace dlm {
namespace {

constexpr double PF_PI = 3.14159265358979323846, PF_2PI = 6.283185307179586476925286766559;

// ocml's lgamma, ONE copy of it: inlined at its nine call sites, its constants are hoisted out of the loops over t and take more registers
// than the wave has
__device__ __noinline__ double pf_lgamma(double v) { return lgamma(v); }

// Lower Cholesky factor of the column-major A (its lower triangle is read) into sl, row-major; lane 0 computes, every lane gets the verdict.
// false: a pivot that is not positive (NaN included)
template <int D>
__device__ __forceinline__ bool pf_chol(const double* A, double* sl, int lane) {
  int ok = 1;
  if (lane == 0) {
    for (int j = 0; j < D && ok; ++j) {
      double s = A[j + j * D];
      for (int k = 0; k < j; ++k) s -= sl[j * D + k] * sl[j * D + k];
      if (!(s > 0.0)) { ok = 0; break; }
      const double dj = sqrt(s);
      sl[j * D + j] = dj;
      for (int c = j + 1; c < D; ++c) sl[j * D + c] = 0.0;   // the products run over whole rows: a zero adds nothing
      for (int i = j + 1; i < D; ++i) {
        double t = A[i + j * D];
        for (int k = 0; k < j; ++k) t -= sl[i * D + k] * sl[j * D + k];
        sl[i * D + j] = t / dj;
      }
    }
  }
  wave_sync();
  return __shfl(ok, 0, 64) != 0;
}

// what a step's log-density needs beyond (eta, the particle): made once per step, the same in every lane
struct PfObs { double y, v, nu, c0, c1, c2; };

__device__ __forceinline__ PfObs pf_obs(int family, int literal, double y, double v, double nu) {
  PfObs o{y, v, nu, 0.0, 0.0, 0.0};
  switch (family) {
    case DLM_OBS_GAUSSIAN: o.c0 = 0.5 * log(PF_2PI * v); break;
    case DLM_OBS_POISSON: o.y = trunc(y); o.c0 = pf_lgamma(o.y + 1.0); break;
    case DLM_OBS_NEGBIN: o.c1 = exp(v); o.c0 = (pf_lgamma(o.c1 + y) - pf_lgamma(y + 1.0)) - pf_lgamma(o.c1); break;
    case DLM_OBS_ZIP: { const double ev = exp(v); o.c1 = ev / (1.0 + ev); o.c2 = log(1.0 + ev); o.c0 = pf_lgamma(y + 1.0); break; }
    case DLM_OBS_STUDENTT: {
      const double sc = sqrt(v);
      o.c1 = nu * sc * sc;
      o.c0 = (pf_lgamma((nu + 1.0) * 0.5) - 0.5 * log(literal ? PF_PI * nu * sc : PF_PI * nu * sc * sc)) - pf_lgamma(nu * 0.5);   // Q39
      break;
    }
    default: o.c1 = log(y); o.c2 = log(1.0 - y); break;   // DLM_OBS_BETA
  }
  return o;
}

// log p(y | eta, v) of the family, as the reference writes it
__device__ __forceinline__ double pf_logdens(int family, const PfObs& o, double eta) {
  switch (family) {
    case DLM_OBS_GAUSSIAN: { const double e = o.y - eta; return -o.c0 - (0.5 * (e * e)) / o.v; }
    case DLM_OBS_POISSON: return (o.y * eta - exp(eta)) - o.c0;
    case DLM_OBS_NEGBIN: {
      const double mu = exp(eta), size = o.c1;
      return (o.c0 + size * log(size / (mu + size))) + o.y * log(mu / (mu + size));
    }
    case DLM_OBS_ZIP:
      if (fabs(o.y) < 1e-5) return log(o.c1 + (1.0 - o.c1) * exp(-exp(eta)));
      return ((o.y * eta - o.c2) - exp(eta)) - o.c0;
    case DLM_OBS_STUDENTT: { const double e = o.y - eta; return o.c0 - ((o.nu + 1.0) * 0.5) * log1p((e * e) / o.c1); }
    default: {   // DLM_OBS_BETA: logisticFunction(1.0) with its clamp, then Dglm.beta's (mean, variance) -> (alpha, beta)
      const double mean = eta < -5.0 ? 0.0 : (eta > 5.0 ? 1.0 : 1.0 / (1.0 + exp(-eta)));
      const double aa = (mean * (1.0 - mean)) / o.v;
      const double al = mean * (aa - 1.0), be = (1.0 - mean) * (aa - 1.0);
      if (!(al > 0.0 && be > 0.0)) return -__builtin_inf();   // Q41
      return ((al - 1.0) * o.c1 + (be - 1.0) * o.c2) - ((pf_lgamma(al) + pf_lgamma(be)) - pf_lgamma(al + be));
    }
  }
}

// sum_i W_i x_k,i for every row k < D of x, lane 0 stores them
template <int D>
__device__ __forceinline__ void pf_means(const double* x, const double* wg, int P, int lane, double* out) {
  double acc[D];
#pragma unroll
  for (int k = 0; k < D; ++k) acc[k] = 0.0;
  for (int i = lane; i < P; i += 64) {
    const double w = wg[i];
#pragma unroll
    for (int k = 0; k < D; ++k) acc[k] = acc[k] + w * x[k * P + i];
  }
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double m = wave_sum(acc[k]);
    if (lane == 0) out[k] = m;
  }
}

// the inclusive running sums of the weights into cum (per slot the Hillis-Steele scan over the lanes, plus the carry of the slot before);
// returns the last one, the total the search scales its uniforms with
__device__ __forceinline__ double pf_running_sums(const double* wg, double* cum, int P, int lane) {
  double carry = 0.0;
  for (int i = lane; i < P; i += 64) {
    double s = wg[i];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double up = __shfl_up(s, off, 64);
      if (lane >= off) s = s + up;
    }
    s = carry + s;
    cum[i] = s;
    carry = __shfl(s, 63, 64);
  }
  return carry;
}

// the first j with cum[j] > target; P - 1 when none is (u total rounding up to the total)
__device__ __forceinline__ int pf_ancestor(const double* cum, int P, double target) {
  int lo = 0, hi = P - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cum[mid] > target) hi = mid; else lo = mid + 1;
  }
  return lo;
}

}  // namespace
}  // namespace dlm
