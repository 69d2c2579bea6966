// Liu-West filter of a dynamic generalised linear model (LiuAndWestFilter.step, LiuAndWest.scala:47-81; Liu & West 2001): an auxiliary particle
// filter whose particles carry their own LOG-VARIANCES psi -- the diagonal of W, and with learn_v V -- which every step shrinks towards their
// weighted mean by `a` and jitters with the matching kernel variance (1 - a^2) s^2: dlm_lw_batch.  With a = 1 and prior standard deviations of 0
// it is the auxiliary particle filter of AuxFilter.scala for known parameters.  The layout is k_storvik's (dlm_storvik.hip): ONE WAVEFRONT PER
// SERIES, particle i = 64 s + lane, everything in LDS, component-major:
//   x [D][P] the cloud | psi [D+1][P] log W_kk (rows k < D) and log V (row D) | wg [P] | cum [P] | sl [D][D] | hs [D+1] | anc [P] (int)
// = (2 d + 3.5) P + d^2 + d + 1 doubles.  x and psi lie behind one another so that either resampling gathers a particle's whole tuple in one
// row loop.  A row whose prior standard deviation is 0 is a KNOWN variance: it is neither shrunk nor jittered, and no normal is drawn for it.
//
// The first-stage log-density lambda_i travels with its particle through the auxiliary gather in wg: the running sums of the first-stage
// weights are formed IN PLACE in wg (cum holds lambda meanwhile), and once the ancestors are known wg is free and takes lambda_anc.
//
// The normals, the searches, the gathers, the second stage's normalisation and its resampling are dlm_pf_common.h's; the initial cloud and the
// results of a series are written out here (below).  The orders of every sum are DESIGN.md 4.19's and 4.21's; tests/lw_restatement.py follows
// the kernel operation for operation.
#include "dlm_pf_common.h"

namespace dlm {
namespace {

// z_r ~ N(0, 1) of (slot, particle): pf_normal under the filter's key; the group of blocks `base` is 0 for the state and DLM_LW_BLOCK_PARAM
// for the log-variances
__device__ __forceinline__ double lw_normal(const DrawStream& rs, unsigned long long series, unsigned slot, unsigned particle, unsigned base, int r) {
  return pf_normal(DLM_KEY_LW, rs, series, slot, particle, base, r);
}

// sum_i W_i row_i and, in a second pass, the centred second moment sum_i W_i (row_i - mean)^2: both sum like pf_means
__device__ __forceinline__ void lw_moments(const double* row, const double* wg, int P, int lane, double& mean, double& var) {
  double acc = 0.0;
  for (int i = lane; i < P; i += 64) acc = acc + wg[i] * row[i];
  mean = wave_sum(acc);
  acc = 0.0;
  for (int i = lane; i < P; i += 64) {
    const double e = row[i] - mean;
    acc = acc + wg[i] * (e * e);
  }
  var = wave_sum(acc);
}

template <int D>
__global__ __launch_bounds__(64, D <= 8 ? 2 : 1) void k_lw(LwArgs a) {
  extern __shared__ double lw_lds[];
  const int n = blockIdx.x, lane = threadIdx.x, P = a.P, T = a.T;
  double* x = lw_lds;                  // [D][P]
  double* psi = x + (size_t)D * P;     // [D+1][P] log W_kk, log V
  double* wg = psi + (size_t)(D + 1) * P;   // [P] the normalised weights W_t,i; lambda between the two stages
  double* cum = wg + P;                // [P]
  double* sl = cum + P;                // [D][D] row-major chol(C0)
  double* hs = sl + D * D;             // [D+1] h s_k of the step, 0 for a row that is not learned
  int* anc = (int*)(hs + (D + 1));     // [P]
  const unsigned long long series = a.rs.series_offset + (unsigned long long)n;
  const double rP = 1.0 / (double)P, nan = __builtin_nan("");
  const double* y = a.y + (size_t)n * T;
  const double* pw = a.prior_w + (size_t)n * a.prior_w_stride;                        // [D][2]: mean, sd
  const double* pv = a.learn_v ? a.prior_v + (size_t)n * a.prior_v_stride : nullptr;  // [2]
  double* mean = a.mean ? a.mean + (size_t)n * T * D : nullptr;
  double* pmean = a.psi_mean ? a.psi_mean + (size_t)n * T * (D + 1) : nullptr;
  double* pvar = a.psi_var ? a.psi_var + (size_t)n * T * (D + 1) : nullptr;
  double* ess = a.ess ? a.ess + (size_t)n * T : nullptr;
  const int rows_psi = D + (a.learn_v ? 1 : 0);   // the rows of psi in use
  const double shrink = a.a, keep = 1.0 - a.a, h = sqrt(1.0 - a.a * a.a);

  int bad = 0, t_bad = 0;   // status bits of the series; the first step without results
  double ll = 0.0;

  // (mean, sd) of the prior of row k
  auto prior = [&](int k) { return k < D ? pw + 2 * k : pv; };

  // the means of a step under the weights it leaves: the state, and mean and variance of every log-variance
  auto outputs = [&](int t) {
    if (mean) pf_means<D>(x, wg, P, lane, mean + (size_t)t * D);
    if (pmean || pvar) {
#pragma nounroll
      for (int k = 0; k <= D; ++k) {
        double m = nan, v = nan;
        if (k < rows_psi) lw_moments(psi + (size_t)k * P, wg, P, lane, m, v);
        if (lane == 0) {
          if (pmean) pmean[(size_t)t * (D + 1) + k] = m;
          if (pvar) pvar[(size_t)t * (D + 1) + k] = v;
        }
      }
    }
  };

  // ---- the priors, the initial cloud x_0,i = m0 + chol(C0) z, psi_k,i = mean_k + sd_k z'
  for (int k = 0; k < rows_psi; ++k) {
    const double* q = prior(k);
    if (!(fabs(q[0]) < __builtin_inf() && q[1] >= 0.0)) bad = DLM_ST_NOT_PD;
  }
  if (!pf_chol<D>(a.C0 + (size_t)n * a.c0_stride, sl, lane)) bad = DLM_ST_NOT_PD;
  if (!bad) {
    const double* m0 = a.m0 + (size_t)n * a.m0_stride;
    for (int i = lane; i < P; i += 64) {   // (not pf_init_cloud with psi as its rows: that takes a register off d = 4 and d = 10)
      double z[D];
#pragma unroll
      for (int c = 0; c < D; ++c) z[c] = lw_normal(a.rs, series, DLM_LW_SLOT_INIT, (unsigned)i, 0u, c);
#pragma nounroll
      for (int r = 0; r <= D; ++r) {
        if (r < D) {
          double acc = sl[r * D] * z[0];
#pragma unroll
          for (int c = 1; c < D; ++c) acc = acc + sl[r * D + c] * z[c];
          x[r * P + i] = m0[r] + acc;
        }
        if (r < rows_psi) {
          const double* q = prior(r);
          double v = q[0];
          if (q[1] > 0.0) v = v + q[1] * lw_normal(a.rs, series, DLM_LW_SLOT_INIT, (unsigned)i, DLM_LW_BLOCK_PARAM, r);
          psi[r * P + i] = v;
        }
      }
      wg[i] = rP;
    }
    if (lane <= D) hs[lane] = 0.0;
    wave_sync();
  }

  if (!bad) {
    const double vfix = a.learn_v ? 1.0 : a.V[(size_t)n * a.v_stride], nu = a.obs_param ? a.obs_param[n] : 0.0;
    double ess_last = (double)P;
    for (int t = 0; t < T; ++t) {
      const double yt = y[t];
      const bool missing = yt != yt;
      const double dte = a.dt ? a.dt[t] : 1.0;
      const bool adv = dte != 0.0;
      const double* G = a.G + (size_t)(a.g_index ? a.g_index[t] : 0) * (D * D);
      const double* F = a.F + (size_t)t * a.f_stride;

      // -- a missing y: the cloud advances under every particle's own variances; psi and the weights are carried
      if (missing) {
        if (adv) {
          for (int i = lane; i < P; i += 64) {
            double xo[D];
#pragma unroll
            for (int c = 0; c < D; ++c) xo[c] = x[c * P + i];
#pragma nounroll
            for (int r = 0; r < D; ++r) {
              double gx = G[r] * xo[0];
#pragma unroll
              for (int c = 1; c < D; ++c) gx = gx + G[r + c * D] * xo[c];
              const double z = lw_normal(a.rs, series, (unsigned)t, (unsigned)i, 0u, r);
              x[r * P + i] = gx + sqrt(dte * exp(psi[r * P + i])) * z;
            }
          }
          wave_sync();
        }
        outputs(t);
        if (ess && lane == 0) ess[t] = ess_last;
        continue;
      }

      // -- the kernel moments of every learned row under W_{t-1}, and the shrinkage m = a psi + (1 - a) mean in place
#pragma nounroll
      for (int k = 0; k < rows_psi; ++k) {
        if (!(prior(k)[1] > 0.0)) continue;
        double* row = psi + (size_t)k * P;
        double pbar, s2;
        lw_moments(row, wg, P, lane, pbar, s2);
        if (a.literal) {   // Q50: the unweighted n - 1 variance about the unweighted mean (varParameters, LiuAndWest.scala:51)
          double acc = 0.0;
          for (int i = lane; i < P; i += 64) acc = acc + row[i];
          const double mu = wave_sum(acc) / (double)P;
          acc = 0.0;
          for (int i = lane; i < P; i += 64) {
            const double e = row[i] - mu;
            acc = acc + e * e;
          }
          s2 = wave_sum(acc) / (double)(P - 1);
        }
        for (int i = lane; i < P; i += 64) row[i] = shrink * row[i] + keep * pbar;
        if (lane == 0) hs[k] = h * sqrt(s2);
      }
      wave_sync();

      // -- the look-ahead: mu_i = G x_i, lambda_i = log p(y | F^T mu_i, exp m_d,i or V) into cum
      const PfObs ob = pf_obs(a.family, a.literal, yt, vfix, nu);
      double mx = -__builtin_inf();
      for (int i = lane; i < P; i += 64) {
        double xo[D];
#pragma unroll
        for (int c = 0; c < D; ++c) xo[c] = x[c * P + i];
        double eta = 0.0;
#pragma nounroll
        for (int r = 0; r < D; ++r) {
          double gx = x[r * P + i];
          if (adv) {
            gx = G[r] * xo[0];
#pragma unroll
            for (int c = 1; c < D; ++c) gx = gx + G[r + c * D] * xo[c];
          }
          eta = r == 0 ? F[0] * gx : eta + F[r] * gx;
        }
        PfObs o = ob;
        if (a.learn_v) o = pf_obs(a.family, a.literal, yt, exp(psi[D * P + i]), nu);
        const double l = pf_logdens(a.family, o, eta);
        cum[i] = l;
        mx = fmax(mx, l);
      }
      const double m1 = wave_max(mx);
      if (!(fabs(m1) < __builtin_inf())) { bad = DLM_ST_NONFINITE; t_bad = t; break; }

      // -- the first stage: omega_i = W_{t-1,i} exp(lambda_i - m1), A their sum; it always resamples
      double part = 0.0;
      for (int i = lane; i < P; i += 64) {
        const double om = wg[i] * exp(cum[i] - m1);
        wg[i] = om;
        part = part + om;
      }
      const double A = wave_sum(part);
      if (!(A > 0.0 && A < __builtin_inf())) { bad = DLM_ST_NONFINITE; t_bad = t; break; }
      ll = ll + (m1 + log(A));
      const double total1 = pf_running_sums(wg, wg, P, lane);   // in place: a lane reads and writes its own particle
      wave_sync();
      pf_search(DLM_KEY_LW | DLM_LW_BLOCK_FIRST, a.rs, series, (unsigned)t, wg, total1, anc, P, lane);
      wave_sync();
      for (int i = lane; i < P; i += 64) wg[i] = cum[anc[i]];   // lambda of the ancestor
      wave_sync();
      pf_gather(x, D + rows_psi, cum, anc, P, lane);

      // -- propagate: psi' = m + h s z', x' = mu + sqrt(dt exp psi') z, l = log p(y | F^T x', exp psi'_d or V) - lambda into cum
      mx = -__builtin_inf();
      for (int i = lane; i < P; i += 64) {
        double xo[D];
#pragma unroll
        for (int c = 0; c < D; ++c) xo[c] = x[c * P + i];
        double eta = 0.0, lv = 0.0;
#pragma nounroll
        for (int r = 0; r < rows_psi; ++r) {
          double ps = psi[r * P + i];
          if (prior(r)[1] > 0.0) {
            ps = ps + hs[r] * lw_normal(a.rs, series, (unsigned)t, (unsigned)i, DLM_LW_BLOCK_PARAM, r);
            psi[r * P + i] = ps;
          }
          if (r < D) {
            double xn = x[r * P + i];
            if (adv) {
              double gx = G[r] * xo[0];
#pragma unroll
              for (int c = 1; c < D; ++c) gx = gx + G[r + c * D] * xo[c];
              xn = gx + sqrt(dte * exp(ps)) * lw_normal(a.rs, series, (unsigned)t, (unsigned)i, 0u, r);
              x[r * P + i] = xn;
            }
            eta = r == 0 ? F[0] * xn : eta + F[r] * xn;
          } else {
            lv = ps;
          }
        }
        PfObs o = ob;
        if (a.learn_v) o = pf_obs(a.family, a.literal, yt, exp(lv), nu);
        double l = pf_logdens(a.family, o, eta);
        if (!a.literal) l = l - wg[i];   // Q51: AuxFilter.scala:46 weights with the density alone
        cum[i] = l;
        mx = fmax(mx, l);
      }
      const double m2 = wave_max(mx);
      if (!(fabs(m2) < __builtin_inf())) { bad = DLM_ST_NONFINITE; t_bad = t; break; }

      // -- the second stage: w_j = exp(l_j - m2), B their sum, W_t,j = w_j / B, sum W^2, the outputs
      part = 0.0;
      for (int i = lane; i < P; i += 64) {
        const double w = exp(cum[i] - m2);
        wg[i] = w;
        part = part + w;
      }
      const double B = wave_sum(part);
      if (!(B > 0.0 && B < __builtin_inf())) { bad = DLM_ST_NONFINITE; t_bad = t; break; }
      ll = ll + (m2 + log(B / (double)P));
      const double sq = pf_normalise(wg, B, P, lane);
      outputs(t);
      ess_last = floor(1.0 / sq);
      if (ess && lane == 0) ess[t] = ess_last;
      if (!(ess_last < (double)a.n0)) continue;

      // -- multinomial resampling of the whole tuple (x, psi)
      pf_resample(DLM_KEY_LW | DLM_LW_BLOCK_RESAMPLE, a.rs, series, (unsigned)t, x, D + rows_psi, wg, rP, cum, anc, P, lane);
    }
  }

  // ---- results (not pf_results: that adds a register at d = 9 and takes one off d = 10)
  if (bad) {
    ll = -__builtin_inf();
    if (mean) for (int j = t_bad * D + lane; j < T * D; j += 64) mean[j] = nan;
    if (pmean) for (int j = t_bad * (D + 1) + lane; j < T * (D + 1); j += 64) pmean[j] = nan;
    if (pvar) for (int j = t_bad * (D + 1) + lane; j < T * (D + 1); j += 64) pvar[j] = nan;
    if (ess) for (int j = t_bad + lane; j < T; j += 64) ess[j] = nan;
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
  if (a.psi) {   // [D + 1][P]: the rows of psi (row D NaN without learn_v)
    double* ps = a.psi + (size_t)n * (D + 1) * P;
    for (int k = 0; k <= D; ++k)
      for (int i = lane; i < P; i += 64) ps[(size_t)k * P + i] = (bad || k >= rows_psi) ? nan : psi[k * P + i];
  }
}

}  // namespace

size_t lw_lds_bytes(int d, int P) {
  return ((size_t)(2 * d + 3) * P + (size_t)d * d + (size_t)(d + 1)) * sizeof(double) + (size_t)P * sizeof(int);
}

hipError_t launch_lw(const LwArgs& a, hipStream_t s) {
  return pick<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(a.d, [&](auto D) {
    return launch(k_lw<decltype(D)::value>, dim3((unsigned)a.N), dim3(64), lw_lds_bytes(a.d, a.P), s, a);
  });
}

}  // namespace dlm
