// d-Inverse-Gamma conjugate step on the device (GibbsSampling.dinvGammaStep: Gibbs.scala:23-78, :134-151).
//
// The FFBS kernels leave [ssy (p) | n (p) | ss (d) | T] per series on the device; with per-series parameters (the
// reference's semantics for a block-diagonal `|*|` model) the draws
//   V_jj ~ InverseGamma(alpha_v + n_j / 2, beta_v + ssy_j / 2)            Gibbs.scala:41-48
//   W_ii ~ InverseGamma(alpha_w + T / 2,   beta_w + ss_i / 2)             Gibbs.scala:72-77 (shape uses T)
// are N (p + d) independent scalars: one thread each, so that a Gibbs iteration never leaves the GPU (the host loop
// over 10^4 series costs more than the FFBS pass it follows).  InverseGamma(shape, scale).draw = 1 / Gamma(shape,
// 1 / scale).draw (InverseGamma.scala:14) = scale / Gamma(shape, 1).draw; the unit-scale Gamma is Marsaglia-Tsang (2000)
// on Philox normals and uniforms keyed by (seed, global series, iteration, component, attempt): reproducible and
// independent of the sharding.  The reference's generator cannot be seeded: only the distribution is
// comparable with it; oracle/dlm_oracle.c restates this very construction.  gibbs_rand, gamma_unit and the W draw live in dlm_draws.h
// (the Student-t step of dlm_studentt.hip draws W through the same functions and its own variates on a stream of its own).
#include "dlm_draws.h"
#include "../../include/dlm_engine.h"

namespace dlm {

__global__ __launch_bounds__(256) void k_dinvgamma_step(int d, int p, int N, const double* __restrict__ stats, double av, double bv,
                                                        double aw, double bw, DrawStream rs, double* __restrict__ Vout,
                                                        double* __restrict__ Wout) {
  const int per = p + d;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)N * per) return;
  const int n = (int)(gid / per), comp = (int)(gid % per);
  const double* s = stats + (size_t)n * (2 * p + d + 1);
  const bool v = comp < p;
  const InvGammaDraw q = v ? InvGammaDraw{av + 0.5 * s[p + comp], bv + 0.5 * s[comp], (unsigned)comp} : w_draw(s, d, p, comp - p, aw, bw);
  const double g = gamma_unit(q.shape, rs.seed, rs.series_offset + (unsigned long long)n, rs.iteration, q.comp);
  if (v) store_diag_draw(Vout + (size_t)n * p * p, p, comp, q, g);
  else store_diag_draw(Wout + (size_t)n * d * d, d, comp - p, q, g);
}

hipError_t launch_dinvgamma_step(int d, int p, int N, const double* stats, double av, double bv, double aw, double bw,
                                 const DrawStream& rs, double* Vout, double* Wout, hipStream_t s) {
  const long long total = (long long)N * (p + d);
  return launch(k_dinvgamma_step, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d, p, N, stats, av, bv, aw, bw, rs, Vout, Wout);
}

}  // namespace dlm
