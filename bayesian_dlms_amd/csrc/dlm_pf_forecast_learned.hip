// Posterior-predictive forecast of a dynamic generalised linear model from the cloud of a LEARNING filter, whose particles carry their own
// variances: dlm_pf_forecast_learned (the clouds of dlm_storvik_batch, dlm_lw_batch and, after dlm_rb_state_draw, dlm_rb_batch).  The layout
// is k_pf_forecast's (dlm_pf_forecast.hip): ONE WAVEFRONT PER SERIES, particle i = 64 s + lane, rows of P doubles in LDS -- the cloud
// x[k][i], behind it the standard deviations s[k][i] of the state noise and the observation scale pv[i] of every particle, contiguous, so
// that the resampling of a weighted entry cloud gathers the whole tuple with ONE pf_resample(rows = 2 D + 1); then wg, cum and the ancestors.
// (2 d + 3.5) P doubles: pf_forecast_learned_lds_bytes, the Storvik and Liu-West budget.
//
// A PURE forecast: no chol(W), no y, no weighting, no likelihood.  To fold in test-period observations, run the filter over them first and
// forecast from the cloud it leaves.  params->W is never read; params->V only when pv is null.
//
// Entry: the cloud, the rows pw [d][P] and pv [P] as they come; weights0 given: validated as k_pf_forecast validates them, then ONE multinomial
// resampling of the tuple (DLM_KEY_PF | DLM_PF_BLOCK_RESAMPLE0, slot slot_offset: k_pf_forecast's ancestors); then the rows become variances
// by var_kind -- DLM_FC_VAR as they are, DLM_FC_LOGVAR exp(row), DLM_FC_IG_SCALE row / Gamma(shape_k, 1) with ONE Gamma per particle and
// component (DLM_KEY_FCL, dlm_draws.h), held for the whole horizon: the parameters are static, a redraw per step would be another law.  A
// variance that is not finite or is negative, a zero one from a Gamma draw or in pv, or a shape that is not positive and finite: DLM_ST_NOT_PD
// for that series alone.  (pv of DLM_OBS_NEGBIN and DLM_OBS_ZIP is no variance but the family's v, DLM_FC_VAR only: it has to be finite; the
// same holds for params->V.)  The variances go out to var_w / var_v there and then; s = sqrt(w).
//
// Step h (slot slot_offset + h): dt_h != 0: x'_k,i = (G_h x_i)_k + sqrt(dt_h) * (s_k,i * z_k,i), z k_pf_forecast's normals, in EXACTLY this
// association -- a cloud whose particles all carry diag(W) and V reproduces k_pf_forecast bit for bit (chol of a diagonal W has the
// rows (0, .., sqrt(W_kk), .., 0), and its products with z add signed zeros to s z).  Then eta_i = F_h^T x'_i, ytilde_i = pf_obs_draw(family, eta_i,
// v_i, nu) with its Gamma and Poisson draws INLINED (pf_obs_draw<true>: the same arithmetic; a call's frame is scratch, and inlined this kernel holds
// fewer registers than with the calls), and everything as k_pf_forecast does: fmean in the order of DESIGN.md 4.19, the draws, the sort in `cum`, the ranks, the equal-weight
// state mean.  A draw that is not finite stops the series: DLM_ST_NONFINITE, NaN in its per-step outputs from that step on.
//
// k_rb_state_draw, below it: the cloud of the Rao-Blackwellised filter, x_i = m_i + chol(C_i) z_i.
//
// tests/pffl_restatement.py restates both kernels.
#include "dlm_obs_draws.h"

namespace dlm {
namespace {

// z ~ N(0, I_D) of (slot, particle): dlm_pf_forecast.hip's fc_normals (that file's own, restated here so that this kernel's state normals are k_pf's)
template <int D>
__device__ __forceinline__ void fl_normals(const DrawStream& rs, unsigned long long series, unsigned slot, unsigned particle, double (&z)[D]) {
#pragma unroll
  for (int q = 0; q < (D + 1) / 2; ++q) {
    double u1, u2;
    gibbs_rand(rs.seed, series, rs.iteration, slot, particle, 0u, u1, u2, DLM_KEY_PF | (unsigned)q);
    const double r = sqrt(-2.0 * log(u1)), ang = PF_2PI * u2;
    z[2 * q] = r * cos(ang);
    if (2 * q + 1 < D) z[2 * q + 1] = r * sin(ang);
  }
}

// Gamma(shape, 1) of component comp (k < d: W_kk, d: V) of (slot, particle) under DLM_KEY_FCL (one call site, at the entry; inlined:
// a call's frame would be the kernel's only scratch)
__device__ __forceinline__ double fl_gamma(double shape, unsigned long long seed, unsigned long long series, unsigned long long iteration,
                                        unsigned slot, unsigned particle, unsigned comp) {
  return gamma_unit_from(shape, DLM_FCL_GAMMA_ATTEMPTS, [&](unsigned attempt, unsigned which, double& u1, double& u2) {
    gibbs_rand(seed, series, iteration, slot, particle, which, u1, u2, DLM_KEY_FCL | (attempt << 8) | (DLM_FCL_BLOCK_GAMMA + comp));
  });
}

// a row's entry as a variance: DLM_FC_VAR as it is, DLM_FC_LOGVAR its exponential, DLM_FC_IG_SCALE over the particle's Gamma g
__device__ __forceinline__ double fl_variance(int var_kind, double row, double g) {
  return var_kind == DLM_FC_VAR ? row : (var_kind == DLM_FC_LOGVAR ? exp(row) : row / g);
}

template <int D>
__global__ __launch_bounds__(64, D <= 8 ? 2 : 1) void k_pf_forecast_learned(PfForecastLearnedArgs a) {
  extern __shared__ double fl_lds[];
  const int n = blockIdx.x, lane = threadIdx.x, P = a.P, T = a.T;
  double* x = fl_lds;               // [D][P]
  double* sd = x + (size_t)D * P;   // [D][P] the rows of pw, then the standard deviations of the state noise
  double* pv = sd + (size_t)D * P;  // [P]    the row of pv (or V), then the observation scale
  double* wg = pv + P;              // [P]
  double* cum = wg + P;             // [P] the running sums of the entry resampling, then the draws of a step and their sort
  int* anc = (int*)(cum + P);       // [P]
  const unsigned long long series = a.rs.series_offset + (unsigned long long)n;
  const double rP = 1.0 / (double)P;
  const double nan = __builtin_nan("");
  double* mean = a.mean ? a.mean + (size_t)n * T * D : nullptr;
  double* fmean = a.fmean + (size_t)n * T;
  double* fquant = a.n_ranks ? a.fquant + (size_t)n * T * a.n_ranks : nullptr;
  double* draws = a.draws ? a.draws + (size_t)n * T * P : nullptr;
  double* var_w = a.var_w ? a.var_w + (size_t)n * D * P : nullptr;
  double* var_v = a.var_v ? a.var_v + (size_t)n * P : nullptr;

  int bad = 0, t_bad = 0;
  bool made = false;   // the variances of every particle stand in var_w / var_v

  // ---- the entry tuple (x, pw, pv) as it comes, resampled once when it comes with weights
  {
    const double* c0 = a.cloud0 + (size_t)n * D * P;
    const double* w0 = a.pw + (size_t)n * D * P;
    const double v_all = a.pv ? 0.0 : a.V[(size_t)n * a.v_stride];
    for (int k = 0; k < D; ++k)
      for (int i = lane; i < P; i += 64) {
        x[k * P + i] = c0[(size_t)k * P + i];
        sd[k * P + i] = w0[(size_t)k * P + i];
      }
    for (int i = lane; i < P; i += 64) {
      pv[i] = a.pv ? a.pv[(size_t)n * P + i] : v_all;
      wg[i] = a.weights0 ? a.weights0[(size_t)n * P + i] : rP;
    }
    wave_sync();
  }
  if (a.weights0) {
    double lo = __builtin_inf();
    for (int i = lane; i < P; i += 64) lo = fmin(lo, wg[i]);   // fmin skips a NaN: the total catches it
    const double total = pf_running_sums(wg, cum, P, lane);
    if (!(-wave_max(-lo) >= 0.0) || !(total > 0.0 && total < __builtin_inf())) bad = DLM_ST_NONFINITE;
    else pf_resample(DLM_KEY_PF | DLM_PF_BLOCK_RESAMPLE0, a.rs, series, (unsigned)a.slot_offset, x, 2 * D + 1, wg, rP, cum, anc, P, lane);
  }

  // ---- the rows become variances (the Gammas of DLM_FC_IG_SCALE: once per particle, AFTER the resampling), then standard deviations
  if (!bad) {
    const bool ig = a.var_kind == DLM_FC_IG_SCALE;
    const double* shapes = ig ? a.shapes + (size_t)n * a.shapes_stride : nullptr;
    const bool v_is_scale = a.family == DLM_OBS_GAUSSIAN || a.family == DLM_OBS_STUDENTT || a.family == DLM_OBS_BETA;
    int ok = 1;
    for (int k = 0; k <= D; ++k) {
      const bool is_v = k == D;
      const bool drawn = ig && (!is_v || a.pv);   // a Gamma stands under this row
      const double shape = drawn ? shapes[k] : 1.0;
      if (!(shape > 0.0 && shape < __builtin_inf())) { ok = 0; continue; }
      double* row = is_v ? pv : sd + (size_t)k * P;
      double* out = is_v ? var_v : (var_w ? var_w + (size_t)k * P : nullptr);
      for (int i = lane; i < P; i += 64) {
        const double g = drawn ? fl_gamma(shape, a.rs.seed, series, a.rs.iteration, (unsigned)a.slot_offset, (unsigned)i, (unsigned)k) : 1.0;
        const double w = (is_v && !a.pv) ? row[i] : fl_variance(a.var_kind, row[i], g);
        if (is_v) {
          if (!(fabs(w) < __builtin_inf()) || (v_is_scale && !(w > 0.0))) ok = 0;
          row[i] = w;
        } else {
          if (!(w < __builtin_inf()) || !(w >= 0.0) || (drawn && !(w > 0.0))) ok = 0;
          row[i] = sqrt(w);
        }
        if (out) out[i] = w;
      }
    }
    if (wave_sum_int(ok) != 64) bad = DLM_ST_NOT_PD;
    made = !bad;
    wave_sync();
  }

  if (!bad) {
    const double nu = a.obs_param ? a.obs_param[n] : 0.0;
    for (int t = 0; t < T; ++t) {
      const unsigned slot = (unsigned)(a.slot_offset + t);
      const double dte = a.dt ? a.dt[t] : 1.0;

      // -- advance: k_pf_forecast's loop over G, then the particle's own diagonal noise
      if (dte != 0.0) {
        const double* G = a.G + (size_t)(a.g_index ? a.g_index[t] : 0) * (D * D);
        const double sdt = sqrt(dte);
        for (int i = lane; i < P; i += 64) {
          double z[D], xo[D];
          fl_normals<D>(a.rs, series, slot, (unsigned)i, z);
#pragma unroll
          for (int c = 0; c < D; ++c) xo[c] = x[c * P + i];
#pragma nounroll
          for (int r = 0; r < D; ++r) {   // (a loop over r in the code, as in k_pf_forecast: unrolled, every entry of G is held in registers)
            double gx = G[r] * xo[0];
#pragma unroll
            for (int c = 1; c < D; ++c) gx = gx + G[r + c * D] * xo[c];
            x[r * P + i] = gx;
          }
#pragma unroll
          for (int c = 0; c < D; ++c) x[c * P + i] = x[c * P + i] + sdt * (sd[c * P + i] * z[c]);   // (z by a constant index: it stays in registers)
        }
      }

      // -- one observation per particle at its own scale: the draws into cum, their sum
      const double* F = a.F + (size_t)t * a.f_stride;
      double part = 0.0;
      int finite = 1;
      for (int i = lane; i < P; i += 64) {
        double eta = F[0] * x[i];
#pragma unroll
        for (int k = 1; k < D; ++k) eta = eta + F[k] * x[k * P + i];
        const double yd = pf_obs_draw<true>(a.family, eta, pv[i], nu, PfDrawSite{a.rs.seed, series, a.rs.iteration, slot, (unsigned)i});
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
      if (mean) pf_means<D>(x, wg, P, lane, mean + (size_t)t * D);
    }
  }

  // ---- the results: a series that stopped leaves NaN in the per-step outputs from that step on; one without variances has no cloud either
  const bool no_cloud = (bad & DLM_ST_NOT_PD) != 0;
  if (bad) {
    pf_no_results(mean, D, t_bad, T, lane);
    pf_no_results(fmean, 1, t_bad, T, lane);
    pf_no_results(fquant, a.n_ranks, t_bad, T, lane);
    if (draws) for (size_t j = (size_t)t_bad * P + lane; j < (size_t)T * P; j += 64) draws[j] = nan;
    if (lane == 0 && a.status) a.status[n] = bad;
  }
  if (a.cloud) {
    double* c = a.cloud + (size_t)n * D * P;
    for (int k = 0; k < D; ++k)
      for (int i = lane; i < P; i += 64) c[(size_t)k * P + i] = no_cloud ? nan : x[k * P + i];
  }
  if (!made) {   // stopped at the entry: the variances were never (all) made
    if (var_w) for (int j = lane; j < D * P; j += 64) var_w[j] = nan;
    if (var_v) for (int i = lane; i < P; i += 64) var_v[i] = nan;
  }
}

// x_i = m_i + chol(C_i) z_i for the particles i = 64 s + lane of series n, one wavefront per series.  A particle's rows are read coalesced; its
// factor lives in its thread's registers (every loop is unrolled), computed in pf_chol's order of operations; the product runs over c = 0 .. r
// in order, the first product starting the sum.  A pivot that is not positive (NaN included) in ANY particle: DLM_ST_NOT_PD for the series
// and NaN in its whole cloud
template <int D>
__global__ __launch_bounds__(64, D <= 8 ? 2 : 1) void k_rb_state_draw(RbStateDrawArgs a) {
  constexpr int TRI = D * (D + 1) / 2;
  const int n = blockIdx.x, lane = threadIdx.x, P = a.P;
  const unsigned long long series = a.rs.series_offset + (unsigned long long)n;
  const double* m = a.means + (size_t)n * D * P;
  const double* C = a.covs + (size_t)n * TRI * P;
  double* out = a.cloud + (size_t)n * D * P;
  int ok = 1;
  for (int i = lane; i < P; i += 64) {
    double L[TRI], acc[D];
#pragma unroll
    for (int e = 0; e < TRI; ++e) L[e] = C[(size_t)e * P + i];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      double s = L[j * (j + 1) / 2 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[j * (j + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
      if (!(s > 0.0)) ok = 0;
      const double dj = sqrt(s);
      L[j * (j + 1) / 2 + j] = dj;
      const double zj = pf_normal(DLM_KEY_RB, a.rs, series, a.slot, (unsigned)i, DLM_RB_BLOCK_STATE, j);
      if (j == 0) acc[0] = dj * zj; else acc[j] = acc[j] + dj * zj;
#pragma unroll
      for (int r = j + 1; r < D; ++r) {
        double t = L[r * (r + 1) / 2 + j];
#pragma unroll
        for (int k = 0; k < j; ++k) t -= L[r * (r + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
        const double l = t / dj;
        L[r * (r + 1) / 2 + j] = l;
        if (j == 0) acc[r] = l * zj; else acc[r] = acc[r] + l * zj;
      }
    }
#pragma unroll
    for (int k = 0; k < D; ++k) out[(size_t)k * P + i] = m[(size_t)k * P + i] + acc[k];
  }
  if (wave_sum_int(ok) != 64) {
    for (int j = lane; j < D * P; j += 64) out[j] = __builtin_nan("");   // (P is a multiple of 64: a lane overwrites what it wrote itself)
    if (lane == 0 && a.status) a.status[n] = DLM_ST_NOT_PD;
  }
}

}  // namespace

size_t pf_forecast_learned_lds_bytes(int d, int P) { return (size_t)(2 * d + 3) * P * sizeof(double) + (size_t)P * sizeof(int); }

hipError_t launch_pf_forecast_learned(const PfForecastLearnedArgs& a, hipStream_t s) {
  return pick<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(a.d, [&](auto D) {
    return launch(k_pf_forecast_learned<decltype(D)::value>, dim3((unsigned)a.N), dim3(64), pf_forecast_learned_lds_bytes(a.d, a.P), s, a);
  });
}

hipError_t launch_rb_state_draw(const RbStateDrawArgs& a, hipStream_t s) {
  return pick<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(a.d, [&](auto D) {
    return launch(k_rb_state_draw<decltype(D)::value>, dim3((unsigned)a.N), dim3(64), 0, s, a);
  });
}

}  // namespace dlm
