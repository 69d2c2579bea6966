// What the particle kernels share (dlm_pf.hip: k_pf, dlm_storvik.hip: k_storvik, dlm_lw.hip: k_lw), each defined here ONCE: the Cholesky
// factor of the initial cloud, the six observation densities of Dglm.scala:46-175, the weighted means over the particles, the normal of one
// component (pf_normal), the initial cloud (pf_init_cloud), the two loops that turn log-weights into weights (pf_omega, pf_normalise), the
// multinomial resampling (pf_resample: pf_running_sums, pf_search over pf_ancestor, pf_gather), the same with the ancestor step of another
// scheme (pf_resample_by: pf_search_strata, pf_metropolis; k_pf's alone) and the results of a series (pf_results).
// One wavefront per series, particle i = 64 s + lane, rows of P doubles in LDS; the orders of every sum are those of DESIGN.md 4.19.
// Every helper is inlined into its kernel; k_pf and k_storvik use all of them, k_lw all but pf_init_cloud and pf_results, either of which
// moves its register count at some d (profiles/r23_notes.md).  dlm_rb.hip's k_rb, which carries Kalman moments in place of a cloud, uses
// pf_normal, pf_running_sums, pf_search, pf_gather, pf_resample, pf_normalise and pf_no_results.
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

// z_r ~ N(0, 1), component r of (slot, particle) in the group of blocks of the kernel's `key` that starts at `base`: block base + r / 2 gives
// the Box-Muller pair, the cosine for an even r and the sine for an odd one
__device__ __forceinline__ double pf_normal(unsigned key, const DrawStream& rs, unsigned long long series, unsigned slot, unsigned particle,
                                            unsigned base, int r) {
  double u1, u2;
  gibbs_rand(rs.seed, series, rs.iteration, slot, particle, 0u, u1, u2, key | (base + (unsigned)(r >> 1)));
  const double rad = sqrt(-2.0 * log(u1)), ang = PF_2PI * u2;
  return rad * ((r & 1) ? sin(ang) : cos(ang));
}

// The initial cloud x_0,i = m0 + sl z_i (sl = chol(C0), row-major) with the weights rP = 1 / P.  normals(i, z) draws z_i; row(r, i) fills what
// else the kernel keeps of particle i beside its component r < D, and once more with r = D
template <int D, class Normals, class Row>
__device__ __forceinline__ void pf_init_cloud(const double* m0, const double* sl, double* x, double* wg, double rP, int P, int lane,
                                              Normals&& normals, Row&& row) {
  for (int i = lane; i < P; i += 64) {
    double z[D];
    normals(i, z);
#pragma nounroll
    for (int r = 0; r < D; ++r) {   // (a loop over r in the code: unrolled, the compiler holds every factor of every row in registers across the particles)
      double acc = sl[r * D] * z[0];
#pragma unroll
      for (int c = 1; c < D; ++c) acc = acc + sl[r * D + c] * z[c];
      x[r * P + i] = m0[r] + acc;
      row(r, i);
    }
    row(D, i);
    wg[i] = rP;
  }
}

// omega_i = W_{t-1,i} exp(l_i - m) into wg from the log-weights l_i in cum and their maximum m (the literal filter forgets the weights it
// did not resample and takes rP = 1 / P: Q37, Q43); returns their sum.  (This and pf_normalise are two plain loops: one function with the
// tests between them costs k_pf and k_storvik two registers)
__device__ __forceinline__ double pf_omega(const double* cum, double m, double* wg, int literal, double rP, int P, int lane) {
  double part = 0.0;
  for (int i = lane; i < P; i += 64) {
    const double om = (literal ? rP : wg[i]) * exp(cum[i] - m);
    wg[i] = om;
    part = part + om;
  }
  return wave_sum(part);
}

// W_t,i = omega_i / stot in place; returns sum W^2
__device__ __forceinline__ double pf_normalise(double* wg, double stot, int P, int lane) {
  double part = 0.0;
  for (int i = lane; i < P; i += 64) {
    const double w = wg[i] / stot;
    wg[i] = w;
    part = part + w * w;
  }
  return wave_sum(part);
}

// the ancestors of a multinomial resampling: anc_i = pf_ancestor at u_i total, u_i the second uniform of (slot, particle i) under key_block
__device__ __forceinline__ void pf_search(unsigned key_block, const DrawStream& rs, unsigned long long series, unsigned slot, const double* cum,
                                          double total, int* anc, int P, int lane) {
  for (int i = lane; i < P; i += 64) {
    double u1, u2;
    gibbs_rand(rs.seed, series, rs.iteration, slot, (unsigned)i, 0u, u1, u2, key_block);
    anc[i] = pf_ancestor(cum, P, u2 * total);
  }
}

// the ancestors of a stratified (DLM_RESAMPLE_STRATIFIED) or systematic resampling: anc_i = pf_ancestor at ((i + u) / P) total, u the second
// uniform of (slot, particle i) under key_block, or with `systematic` of (slot, particle 0) for every i -- every lane draws that one block,
// which costs the wave one draw, and no other.  The targets ascend with i, so the ancestors do not decrease
__device__ __forceinline__ void pf_search_strata(unsigned key_block, const DrawStream& rs, unsigned long long series, unsigned slot,
                                                 const double* cum, double total, int* anc, int P, int lane, bool systematic) {
  double u1, u0 = 0.0;
  if (systematic) gibbs_rand(rs.seed, series, rs.iteration, slot, 0u, 0u, u1, u0, key_block);
  for (int i = lane; i < P; i += 64) {
    double u = u0;
    if (!systematic) gibbs_rand(rs.seed, series, rs.iteration, slot, (unsigned)i, 0u, u1, u, key_block);
    anc[i] = pf_ancestor(cum, P, (((double)i + u) / (double)P) * total);
  }
}

// the ancestors of a Metropolis resampling (Murray, Lee & Jacob 2016) of b steps: particle i's chain starts at k = i; step s proposes
// j = min(floor(u2 P), P - 1) and moves there when u1 W_k <= W_j, (u1, u2) the uniforms of (slot, particle i) under key_block0 + s; anc_i is
// the last k.  No running sums and no division: a k of weight 0 always moves.  The reads wg[j] are scattered over the lanes' banks
__device__ __forceinline__ void pf_metropolis(unsigned key_block0, const DrawStream& rs, unsigned long long series, unsigned slot,
                                              const double* wg, int* anc, int P, int b, int lane) {
  for (int i = lane; i < P; i += 64) {
    int k = i;
    double wk = wg[i];
    for (int s = 0; s < b; ++s) {
      double u1, u2;
      gibbs_rand(rs.seed, series, rs.iteration, slot, (unsigned)i, 0u, u1, u2, key_block0 + (unsigned)s);
      const int j = min((int)(u2 * (double)P), P - 1);   // (u2 >= 0: the conversion is the floor; u2 P can round up to P)
      const double wj = wg[j];
      if (u1 * wk <= wj) { k = j; wk = wj; }
    }
    anc[i] = k;
  }
}

// the gather of a particle's tuple, the `rows` rows of P that start at x, by ancestor: row by row through `buf`
__device__ __forceinline__ void pf_gather(double* x, int rows, double* buf, const int* anc, int P, int lane) {
  for (int k = 0; k < rows; ++k) {
    for (int i = lane; i < P; i += 64) buf[i] = x[k * P + anc[i]];
    wave_sync();
    for (int i = lane; i < P; i += 64) x[k * P + i] = buf[i];
    wave_sync();
  }
}

// multinomial resampling of the tuples under the weights wg: the running sums into cum, the searches, the gather, the weights back to rP = 1 / P
__device__ __forceinline__ void pf_resample(unsigned key_block, const DrawStream& rs, unsigned long long series, unsigned slot, double* x,
                                            int rows, double* wg, double rP, double* cum, int* anc, int P, int lane) {
  const double total = pf_running_sums(wg, cum, P, lane);
  wave_sync();
  pf_search(key_block, rs, series, slot, cum, total, anc, P, lane);
  wave_sync();
  pf_gather(x, rows, cum, anc, P, lane);
  for (int i = lane; i < P; i += 64) wg[i] = rP;
  wave_sync();
}

// pf_resample with the ancestor step of a scheme OTHER than the multinomial one (`scheme`: DLM_RESAMPLE_STRATIFIED, _SYSTEMATIC or _METROPOLIS,
// the same in every lane), dlm_pf_resampled's: the stratified and systematic searches read block key | block, the Metropolis chains the
// blocks key | block_mh0 + s, s < mh_steps, and form no running sums.  The gather and the weights are pf_resample's
__device__ __forceinline__ void pf_resample_by(int scheme, int mh_steps, unsigned key, unsigned block, unsigned block_mh0, const DrawStream& rs,
                                               unsigned long long series, unsigned slot, double* x, int rows, double* wg, double rP,
                                               double* cum, int* anc, int P, int lane) {
  if (scheme == DLM_RESAMPLE_METROPOLIS) {
    wave_sync();   // the chains read the other lanes' weights
    pf_metropolis(key | block_mh0, rs, series, slot, wg, anc, P, mh_steps, lane);
  } else {
    const double total = pf_running_sums(wg, cum, P, lane);
    wave_sync();
    pf_search_strata(key | block, rs, series, slot, cum, total, anc, P, lane, scheme == DLM_RESAMPLE_SYSTEMATIC);
  }
  wave_sync();
  pf_gather(x, rows, cum, anc, P, lane);
  for (int i = lane; i < P; i += 64) wg[i] = rP;
  wave_sync();
}

// NaN into the steps t_bad .. T - 1 of a per-step output of `width` doubles a step (a null pointer: nothing)
__device__ __forceinline__ void pf_no_results(double* out, int width, int t_bad, int T, int lane) {
  if (out) for (int j = t_bad * width + lane; j < T * width; j += 64) out[j] = __builtin_nan("");
}

// The results of series n: ll (-inf with a status bit), the status, NaN from the first step without results on in the series' mean, ess
// and the kernel's own per-step outputs step0 and step1 ([T][D + 1]; all four nullable); the cloud (NaN when it was never made), the weights, and into `own`
// ([D + 1][P], nullable) the kernel's rows behind the cloud, the first `valid` of them (the others NaN)
template <int D, class Args>
__device__ __forceinline__ void pf_results(const Args& a, int n, int lane, int bad, int t_bad, double ll, const double* x,
                                           const double* wg, double* mean, double* ess, double* step0, double* step1, double* own,
                                           int valid) {
  const int P = a.P, T = a.T;
  const double nan = __builtin_nan("");
  if (bad) {
    ll = -__builtin_inf();
    pf_no_results(mean, D, t_bad, T, lane);
    pf_no_results(step0, D + 1, t_bad, T, lane);
    pf_no_results(step1, D + 1, t_bad, T, lane);
    pf_no_results(ess, 1, t_bad, T, lane);
  }
  if (lane == 0) {
    a.ll[n] = ll;
    if (a.status && bad) a.status[n] = bad;
  }
  const bool no_cloud = (bad & DLM_ST_NOT_PD) != 0;
  if (a.cloud) {
    double* c = a.cloud + (size_t)n * D * P;
    for (int k = 0; k < D; ++k)
      for (int i = lane; i < P; i += 64) c[(size_t)k * P + i] = no_cloud ? nan : x[k * P + i];
  }
  if (a.weights) {
    double* w = a.weights + (size_t)n * P;
    for (int i = lane; i < P; i += 64) w[i] = bad ? nan : wg[i];
  }
  if (own) {
    double* o = own + (size_t)n * (D + 1) * P;
    const double* rows = x + (size_t)D * P;
    for (int k = 0; k <= D; ++k)
      for (int i = lane; i < P; i += 64) o[(size_t)k * P + i] = (bad || k >= valid) ? nan : rows[k * P + i];
  }
}

}  // namespace
}  // namespace dlm
