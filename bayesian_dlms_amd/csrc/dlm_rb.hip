// Rao-Blackwellised particle filter of a Gaussian DLM (RaoBlackwellFilter.scala; the (m, C) variant of the Liu-West filter): every particle
// carries its own LOG-VARIANCES psi -- the diagonal of W, and with learn_v V -- and, in place of a drawn state, the Kalman mean m and covariance
// C of the state GIVEN those variances: dlm_rb_batch.  The state is integrated out exactly, so the only draws are the initial psi, the jitter
// and the two resampling uniforms.  The layout is k_lw's (dlm_lw.hip): ONE WAVEFRONT PER SERIES, particle i = 64 s + lane, everything in LDS,
// component-major:
//   m [D][P] | C [D(D+1)/2][P] the lower triangle by rows, entry (r, c) in row r (r + 1) / 2 + c | psi [D+1][P] log W_kk (rows k < D), log V (row D)
//   | wg [P] | cum [P] | scr [D(D+1)/2][64] | gf [D] | mu [D] | hs [D+1] | anc [P] (int)
// = (D(D+1)/2 + 2 D + 3.5) P + 64 D(D+1)/2 + 3 D + 1 doubles.  m, C and psi lie behind one another so that either resampling gathers a particle's
// whole tuple in one row loop.  scr is ONE slot of predicted covariances R = G C G^T + dt diag(exp psi): lane l keeps the R of the particle it
// works on in column l, row by row -- u = (G C)_r. in registers, then R_rc = sum_b u_b G_cb -- because C is read until the last row is done;
// the Kalman update reads R from there and writes C' over C.  Without an advance (dt = 0) R is C and the update runs in place: row r of the
// result needs of C only what lies in the rows from r on.
//
// Both densities of a step, the look-ahead's under the shrunk variances and the propagated particle's under the new ones, come from ONE
// function (rb_predict) on the rows of psi as they stand in LDS: where the variances did not move the two are the same operations on the same
// numbers and the second stage's log-weight is 0 exactly.  The first-stage log-density travels through the auxiliary gather in wg as in k_lw.
//
// The normals, the searches, the gathers, the second stage's normalisation and its resampling are dlm_pf_common.h's.  The orders of every sum
// are DESIGN.md 4.19's and 4.22's; tests/rb_restatement.py follows the kernel operation for operation.
#include "dlm_pf_common.h"

namespace dlm {
namespace {

// z'_r ~ N(0, 1) of (slot, particle): the pairs of the log-variances are the filter's only normals
__device__ __forceinline__ double rb_normal(const DrawStream& rs, unsigned long long series, unsigned slot, unsigned particle, int r) {
  return pf_normal(DLM_KEY_RB, rs, series, slot, particle, DLM_RB_BLOCK_PARAM, r);
}

// sum_i W_i row_i and, in a second pass, the centred second moment sum_i W_i (row_i - mean)^2 (k_lw's lw_moments: that one stays in its file,
// where it holds k_lw's register counts)
__device__ __forceinline__ void rb_moments(const double* row, const double* wg, int P, int lane, double& mean, double& var) {
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

// the row of the packed lower triangle that holds entry (a, b) of a symmetric matrix
__device__ __forceinline__ int rb_sym(int a, int b) { return a >= b ? a * (a + 1) / 2 + b : b * (b + 1) / 2 + a; }

// log N(y; f, Q) as pf_logdens writes the Gaussian family
__device__ __forceinline__ double rb_logn(double y, double f, double Q) {
  const double e = y - f;
  return -(0.5 * log(PF_2PI * Q)) - (0.5 * (e * e)) / Q;
}

// The predictive moments of y for particle i without the observation variance: f = g^T m and s = g^T C g + dte sum_k F_k^2 exp psi_k, g = G^T F
// (gf; F itself without an advance).  psi: the rows as they stand -- the shrunk log-variances in the look-ahead, the new ones after the jitter
template <int D>
__device__ __forceinline__ void rb_predict(const double* m, const double* Cp, const double* psi, const double* gf, const double* F, int P, int i,
                                           bool adv, double dte, double& f, double& s) {
  double fa = 0.0, sa = 0.0;
#pragma nounroll
  for (int a = 0; a < D; ++a) {
    double cg = Cp[rb_sym(a, 0) * P + i] * gf[0];
#pragma unroll
    for (int b = 1; b < D; ++b) cg = cg + Cp[rb_sym(a, b) * P + i] * gf[b];
    const double ga = gf[a];
    fa = a == 0 ? ga * m[i] : fa + ga * m[a * P + i];
    sa = a == 0 ? ga * cg : sa + ga * cg;
  }
  if (adv) {
#pragma nounroll
    for (int k = 0; k < D; ++k) sa = sa + (F[k] * F[k]) * (dte * exp(psi[k * P + i]));
  }
  f = fa;
  s = sa;
}

// a = G m of particle i in place
template <int D>
__device__ __forceinline__ void rb_advance_mean(const double* G, double* m, int P, int i) {
  double mo[D];
#pragma unroll
  for (int c = 0; c < D; ++c) mo[c] = m[c * P + i];
#pragma nounroll
  for (int r = 0; r < D; ++r) {
    double gx = G[r] * mo[0];
#pragma unroll
    for (int c = 1; c < D; ++c) gx = gx + G[r + c * D] * mo[c];
    m[r * P + i] = gx;
  }
}

// R = G C G^T + dte diag(exp psi_k) of particle i into column `lane` of scr, its lower triangle: per row r, u = (G C)_r. then R_rc = sum_b u_b G_cb
template <int D>
__device__ __forceinline__ void rb_predict_cov(const double* G, const double* Cp, const double* psi, double* scr, int P, int i, int lane, double dte) {
#pragma nounroll
  for (int r = 0; r < D; ++r) {
    double u[D];
    const double g0 = G[r];
#pragma unroll
    for (int b = 0; b < D; ++b) u[b] = g0 * Cp[rb_sym(0, b) * P + i];
#pragma nounroll
    for (int a = 1; a < D; ++a) {
      const double g = G[r + a * D];
#pragma unroll
      for (int b = 0; b < D; ++b) u[b] = u[b] + g * Cp[rb_sym(a, b) * P + i];
    }
#pragma nounroll
    for (int c = 0; c <= r; ++c) {
      double acc = u[0] * G[c];
#pragma unroll
      for (int b = 1; b < D; ++b) acc = acc + u[b] * G[c + b * D];
      if (c == r) acc = acc + dte * exp(psi[r * P + i]);
      scr[(r * (r + 1) / 2 + c) * 64 + lane] = acc;
    }
  }
}

// The Kalman update of particle i by the Joseph form (KalmanFilter.scala:89-90), the products with I - K F^T written out: K = R F / Q,
// m' = a + K e, B = (I - K F^T) R = R - K (R F)^T, C' = B (I - K F^T)^T + K v K^T = B - (B F) K^T + (v K) K^T, its lower triangle into Cp.
// R: the lower triangle in rows of `stride`, this particle's column `col` (scr, 64, lane; or Cp, P, i: in place, since row r reads nothing
// above row r that an earlier row wrote); m holds a
template <int D>
__device__ __forceinline__ void rb_update(const double* R, int stride, int col, const double* F, double Q, double v, double e, double* m,
                                          double* Cp, int P, int i) {
  double rf[D], K[D];
#pragma unroll
  for (int r = 0; r < D; ++r) rf[r] = R[rb_sym(r, 0) * stride + col] * F[0];
#pragma nounroll
  for (int c = 1; c < D; ++c) {
    const double fc = F[c];
#pragma unroll
    for (int r = 0; r < D; ++r) rf[r] = rf[r] + R[rb_sym(r, c) * stride + col] * fc;
  }
#pragma unroll
  for (int r = 0; r < D; ++r) K[r] = rf[r] / Q;
#pragma nounroll
  for (int r = 0; r < D; ++r) {
    double row[D];
#pragma unroll
    for (int b = 0; b < D; ++b) row[b] = R[rb_sym(r, b) * stride + col];
    double rfr = row[0] * F[0];
#pragma unroll
    for (int b = 1; b < D; ++b) rfr = rfr + row[b] * F[b];
    const double kr = rfr / Q;
    m[r * P + i] = m[r * P + i] + kr * e;
#pragma unroll
    for (int b = 0; b < D; ++b) row[b] = row[b] - kr * rf[b];
    double bf = row[0] * F[0];
#pragma unroll
    for (int b = 1; b < D; ++b) bf = bf + row[b] * F[b];
    const double vk = v * kr;
#pragma unroll
    for (int c = 0; c < D; ++c)
      if (c <= r) Cp[(r * (r + 1) / 2 + c) * P + i] = (row[c] - bf * K[c]) + vk * K[c];
  }
}

template <int D>
__global__ __launch_bounds__(64, D <= 8 ? 2 : 1) void k_rb(RbArgs a) {
  extern __shared__ double rb_lds[];
  constexpr int TRI = D * (D + 1) / 2;
  const int n = blockIdx.x, lane = threadIdx.x, P = a.P, T = a.T;
  double* m = rb_lds;                       // [D][P]
  double* Cp = m + (size_t)D * P;           // [TRI][P]
  double* psi = Cp + (size_t)TRI * P;       // [D+1][P] log W_kk, log V
  double* wg = psi + (size_t)(D + 1) * P;   // [P] the normalised weights W_t,i; lambda between the two stages
  double* cum = wg + P;                     // [P]
  double* scr = cum + P;                    // [TRI][64] the predicted covariances of the slot at work
  double* gf = scr + TRI * 64;              // [D] G^T F of the step
  double* mu = gf + D;                      // [D] the mean of the step's outputs
  double* hs = mu + D;                      // [D+1] h s_k of the step, 0 for a row that is not learned
  int* anc = (int*)(hs + (D + 1));          // [P]
  const unsigned long long series = a.rs.series_offset + (unsigned long long)n;
  const double rP = 1.0 / (double)P, nan = __builtin_nan("");
  const double* y = a.y + (size_t)n * T;
  const double* pw = a.prior_w + (size_t)n * a.prior_w_stride;                        // [D][2]: mean, sd
  const double* pv = a.learn_v ? a.prior_v + (size_t)n * a.prior_v_stride : nullptr;  // [2]
  double* mean = a.mean ? a.mean + (size_t)n * T * D : nullptr;
  double* cov = a.cov ? a.cov + (size_t)n * T * D * D : nullptr;
  double* pmean = a.psi_mean ? a.psi_mean + (size_t)n * T * (D + 1) : nullptr;
  double* pvar = a.psi_var ? a.psi_var + (size_t)n * T * (D + 1) : nullptr;
  double* ess = a.ess ? a.ess + (size_t)n * T : nullptr;
  const int rows_psi = D + (a.learn_v ? 1 : 0);   // the rows of psi in use
  const double shrink = a.a, keep = 1.0 - a.a, h = sqrt(1.0 - a.a * a.a);

  int bad = 0, t_bad = 0;   // status bits of the series; the first step without results
  double ll = 0.0;

  // (mean, sd) of the prior of row k
  auto prior = [&](int k) { return k < D ? pw + 2 * k : pv; };

  // the moments of a step under the weights it leaves: mean and mixture covariance of the state, mean and variance of every log-variance
  auto outputs = [&](int t) {
    if (mean || cov) {
#pragma nounroll
      for (int k = 0; k < D; ++k) {
        double acc = 0.0;
        for (int i = lane; i < P; i += 64) acc = acc + wg[i] * m[k * P + i];
        const double s = wave_sum(acc);
        if (lane == 0) {
          mu[k] = s;
          if (mean) mean[(size_t)t * D + k] = s;
        }
      }
      wave_sync();
    }
    if (cov) {
#pragma nounroll
      for (int r = 0; r < D; ++r) {
#pragma nounroll
        for (int c = 0; c <= r; ++c) {
          const double mr = mu[r], mc = mu[c];
          const double* row = Cp + (size_t)(r * (r + 1) / 2 + c) * P;
          double acc = 0.0;
          for (int i = lane; i < P; i += 64) acc = acc + wg[i] * (row[i] + (m[r * P + i] - mr) * (m[c * P + i] - mc));
          const double s = wave_sum(acc);
          if (lane == 0) {
            cov[(size_t)t * D * D + r * D + c] = s;
            cov[(size_t)t * D * D + c * D + r] = s;
          }
        }
      }
    }
    if (pmean || pvar) {
#pragma nounroll
      for (int k = 0; k <= D; ++k) {
        double pm = nan, v = nan;
        if (k < rows_psi) rb_moments(psi + (size_t)k * P, wg, P, lane, pm, v);
        if (lane == 0) {
          if (pmean) pmean[(size_t)t * (D + 1) + k] = pm;
          if (pvar) pvar[(size_t)t * (D + 1) + k] = v;
        }
      }
    }
  };

  // ---- the priors, the initial cloud m_0,i = m0, C_0,i = C0, psi_k,i = mean_k + sd_k z'
  for (int k = 0; k < rows_psi; ++k) {
    const double* q = prior(k);
    if (!(fabs(q[0]) < __builtin_inf() && q[1] >= 0.0)) bad = DLM_ST_NOT_PD;
  }
  if (!bad) {
    const double* m0 = a.m0 + (size_t)n * a.m0_stride;
    const double* C0 = a.C0 + (size_t)n * a.c0_stride;
    for (int i = lane; i < P; i += 64) {
#pragma nounroll
      for (int r = 0; r < D; ++r) {
        m[r * P + i] = m0[r];
#pragma nounroll
        for (int c = 0; c <= r; ++c) Cp[(r * (r + 1) / 2 + c) * P + i] = C0[r + c * D];
      }
#pragma nounroll
      for (int r = 0; r < rows_psi; ++r) {
        const double* q = prior(r);
        double v = q[0];
        if (q[1] > 0.0) v = v + q[1] * rb_normal(a.rs, series, DLM_RB_SLOT_INIT, (unsigned)i, r);
        psi[r * P + i] = v;
      }
      wg[i] = rP;
    }
    if (lane <= D) hs[lane] = 0.0;
    wave_sync();
  }

  if (!bad) {
    const double vfix = a.learn_v ? 1.0 : a.V[(size_t)n * a.v_stride];
    double ess_last = (double)P;
    bool first = true;   // C0 has not been through an observed step yet: a Q that is not positive is the prior's
    for (int t = 0; t < T; ++t) {
      const double yt = y[t];
      const bool missing = yt != yt;
      const double dte = a.dt ? a.dt[t] : 1.0;
      const bool adv = dte != 0.0;
      const double* G = a.G + (size_t)(a.g_index ? a.g_index[t] : 0) * (D * D);
      const double* F = a.F + (size_t)t * a.f_stride;

      // -- a missing y: the moments advance under every particle's own variances; psi and the weights are carried
      if (missing) {
        if (adv) {
          for (int i = lane; i < P; i += 64) {
            rb_predict_cov<D>(G, Cp, psi, scr, P, i, lane, dte);
            rb_advance_mean<D>(G, m, P, i);
#pragma nounroll
            for (int e = 0; e < TRI; ++e) Cp[e * P + i] = scr[e * 64 + lane];
          }
          wave_sync();
        }
        outputs(t);
        if (ess && lane == 0) ess[t] = ess_last;
        continue;
      }

      // -- g = G^T F, and the kernel moments of every learned row under W_{t-1} with the shrinkage mshr = a psi + (1 - a) mean in place
      if (lane < D) {
        double g = F[lane];
        if (adv) {
          g = F[0] * G[lane * D];
          for (int r = 1; r < D; ++r) g = g + F[r] * G[r + lane * D];
        }
        gf[lane] = g;
      }
#pragma nounroll
      for (int k = 0; k < rows_psi; ++k) {
        if (!(prior(k)[1] > 0.0)) continue;
        double* row = psi + (size_t)k * P;
        double pbar, s2;
        rb_moments(row, wg, P, lane, pbar, s2);
        if (a.literal) {   // Q50: the unweighted n - 1 variance about the unweighted mean
          double acc = 0.0;
          for (int i = lane; i < P; i += 64) acc = acc + row[i];
          const double mu0 = wave_sum(acc) / (double)P;
          acc = 0.0;
          for (int i = lane; i < P; i += 64) {
            const double e = row[i] - mu0;
            acc = acc + e * e;
          }
          s2 = wave_sum(acc) / (double)(P - 1);
        }
        for (int i = lane; i < P; i += 64) row[i] = shrink * row[i] + keep * pbar;
        if (lane == 0) hs[k] = h * sqrt(s2);
      }
      wave_sync();

      // -- the look-ahead: lambda_i = log N(y; f_i, Q_i) of the Kalman step under the shrunk variances, into cum
      double mx = -__builtin_inf(), qf = 0.0;   // qf: 2 a Q that is not positive (NaN included), 1 one that is not finite
      for (int i = lane; i < P; i += 64) {
        double f, s;
        rb_predict<D>(m, Cp, psi, gf, F, P, i, adv, dte, f, s);
        const double v = a.learn_v ? exp(psi[D * P + i]) : vfix;
        const double Q = a.literal ? v : s + v;   // Q57: RaoBlackwellFilter.scala:68-71 takes the observation variance alone
        qf = fmax(qf, !(Q > 0.0) ? 2.0 : (Q < __builtin_inf() ? 0.0 : 1.0));
        const double l = rb_logn(yt, f, Q);
        cum[i] = l;
        mx = fmax(mx, l);
      }
      const double m1 = wave_max(mx);
      qf = wave_max(qf);
      if (qf != 0.0 || !(fabs(m1) < __builtin_inf())) { bad = (qf == 2.0 && first) ? DLM_ST_NOT_PD : DLM_ST_NONFINITE; t_bad = t; break; }

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
      pf_search(DLM_KEY_RB | DLM_RB_BLOCK_FIRST, a.rs, series, (unsigned)t, wg, total1, anc, P, lane);
      wave_sync();
      for (int i = lane; i < P; i += 64) wg[i] = cum[anc[i]];   // lambda of the ancestor
      wave_sync();
      pf_gather(m, D + TRI + rows_psi, cum, anc, P, lane);

      // -- propagate: psi' = mshr + h s z', l = log N(y; f, Q) under psi' - lambda into cum, then the Kalman step under psi'
      mx = -__builtin_inf();
      qf = 0.0;
      for (int i = lane; i < P; i += 64) {
#pragma nounroll
        for (int r = 0; r < rows_psi; ++r)
          if (prior(r)[1] > 0.0) psi[r * P + i] = psi[r * P + i] + hs[r] * rb_normal(a.rs, series, (unsigned)t, (unsigned)i, r);
        double f, s;
        rb_predict<D>(m, Cp, psi, gf, F, P, i, adv, dte, f, s);
        const double v = a.learn_v ? exp(psi[D * P + i]) : vfix;
        const double Q = s + v;
        qf = fmax(qf, !(Q > 0.0) ? 2.0 : (Q < __builtin_inf() ? 0.0 : 1.0));
        double l = rb_logn(yt, f, Q);
        if (!a.literal) l = l - wg[i];   // Q58: RaoBlackwellFilter.scala:54 weights with the density alone
        cum[i] = l;
        mx = fmax(mx, l);
        if (adv) {
          rb_predict_cov<D>(G, Cp, psi, scr, P, i, lane, dte);
          rb_advance_mean<D>(G, m, P, i);
          rb_update<D>(scr, 64, lane, F, Q, v, yt - f, m, Cp, P, i);
        } else {
          rb_update<D>(Cp, P, i, F, Q, v, yt - f, m, Cp, P, i);
        }
      }
      const double m2 = wave_max(mx);
      qf = wave_max(qf);
      if (qf != 0.0 || !(fabs(m2) < __builtin_inf())) { bad = (qf == 2.0 && first) ? DLM_ST_NOT_PD : DLM_ST_NONFINITE; t_bad = t; break; }
      first = false;

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

      // -- multinomial resampling of the whole tuple (m, C, psi)
      pf_resample(DLM_KEY_RB | DLM_RB_BLOCK_RESAMPLE, a.rs, series, (unsigned)t, m, D + TRI + rows_psi, wg, rP, cum, anc, P, lane);
    }
  }

  // ---- results
  if (bad) {
    ll = -__builtin_inf();
    pf_no_results(mean, D, t_bad, T, lane);
    pf_no_results(cov, D * D, t_bad, T, lane);
    pf_no_results(pmean, D + 1, t_bad, T, lane);
    pf_no_results(pvar, D + 1, t_bad, T, lane);
    pf_no_results(ess, 1, t_bad, T, lane);
  }
  if (lane == 0) {
    a.ll[n] = ll;
    if (a.status && bad) a.status[n] = bad;
  }
  if (a.cloud) {
    double* c = a.cloud + (size_t)n * D * P;
    for (int k = 0; k < D; ++k)
      for (int i = lane; i < P; i += 64) c[(size_t)k * P + i] = bad ? nan : m[k * P + i];
  }
  if (a.covs) {
    double* c = a.covs + (size_t)n * TRI * P;
    for (int k = 0; k < TRI; ++k)
      for (int i = lane; i < P; i += 64) c[(size_t)k * P + i] = bad ? nan : Cp[k * P + i];
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

size_t rb_lds_bytes(int d, int P) {
  const size_t tri = (size_t)d * (d + 1) / 2;
  return ((tri + 2 * (size_t)d + 3) * P + tri * 64 + 3 * (size_t)d + 1) * sizeof(double) + (size_t)P * sizeof(int);
}

hipError_t launch_rb(const RbArgs& a, hipStream_t s) {
  return pick<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(a.d, [&](auto D) {
    return launch(k_rb<decltype(D)::value>, dim3((unsigned)a.N), dim3(64), rb_lds_bytes(a.d, a.P), s, a);
  });
}

}  // namespace dlm
