// Gibbs sampler of the stochastic-volatility model with AR(1) latent log-volatility (StochasticVolatility.sampleUni / sampleBeta,
// StochasticVolatility.scala:269-341): the two conditional draws around the AR(1) FFBS call (dlm_ar1.hip).
//   y_t = eps_t exp(alpha_t / 2),   alpha_t = mu + phi (alpha_{t-1} - mu) + eta_t,   eta_t ~ N(0, sigma^2)
// Kim, Shephard & Chib (1998): log y_t^2 = alpha_t + log eps_t^2, log eps^2 approximated by a mixture of seven normals
// (weights, means, variances: StochasticVolatility.scala:42-44).  One iteration of a chain:
//   k_sv_mixture   k_t | (y_t, alpha_t) ~ Categorical(pi_j N(log y_t^2 - m_j; alpha_t, v_j)),  ystar_t = log y_t^2 - m_{k_t},  v_t = v_{k_t}
//                  (sampleKt, :112-140; sampleStateAr, :151-157).  alpha == nullptr: ystar = log y^2 + 1.27, v = pi^2 / 2, no draw
//                  (initialStateAr, StochVolKnots.scala:345-352)
//   k_ar1_ffbs     alpha | (ystar, v, phi, mu, sigma)       dlm_ar1_ffbs_batch with v_stride = T, sv_stride = 3, as it is
//   k_sv_params    phi | (alpha, mu, sigma), then mu | (alpha, phi', sigma), then sigma | (alpha, phi', mu')
//                  (samplePhiConjugate, StochVolKnots.scala:25-43, or the Beta-proposal Metropolis-Hastings samplePhi, :189-202;
//                   sampleMu, :212-229; sampleSigma, :238-252)
// alpha rows are [T+1]: alpha[0] the state before the first observation, alpha[t+1] the state of y[t] (dlm_ar1_ffbs_batch's theta).
//
// k_sv_mixture is parallel over the N T elements, one per thread: one log, the exps of the weights (the largest is exp(0) = 1), one
// Philox block.  With lw_j the log weights, w_j = exp(lw_j - max lw), p_j = w_0 + ... + w_j in index order, S = p_6 and u the [0, 1)
// uniform of the element's block:  k = #{ j in 0..5 : u S >= p_j }.  A missing y_t (NaN) draws k from the prior weights and keeps
// ystar_t = NaN; an observed y_t whose log y_t^2 is not finite (y_t = 0, or y_t^2 underflowing: Q20) is treated as missing and the
// series gets DLM_ST_NONFINITE.
//
// k_sv_params is one wavefront per series, lanes striding over the pairs (alpha_{t-1}, alpha_t), t = 2..T; the pair t = 1 -- which
// the reference's sums leave out (Q17) -- is kept apart and added behind the reduction in the default mode.  Every reduction is a
// lane-sequential sum over t = 2 + lane, 2 + lane + 64, ... followed by the xor butterfly (wave_sum): a fixed order, no atomics, so
// that a series' output depends on neither N nor its neighbours.  mu's sum needs the new phi and sigma's needs both: three passes
// over a row the wave has just read.  Scalar draws are made on lane 0 and broadcast; the Beta mode's six lgamma values are made
// side by side, one per lane.  The kernel is flattened: an out-of-line gamma_unit costs a call frame in scratch.
//
// Default (corrected) arithmetic, psi the prior's standard deviation, all T pairs:
//   phi | . ~ N(mean, 1 / prec) on (-1, 1):  prec = 1 / psi^2 + sum (alpha_{t-1} - mu)^2 / sigma^2,
//                                            mean = (m / psi^2 + sum (alpha_{t-1} - mu)(alpha_t - mu) / sigma^2) / prec
//       by rejection over the attempts 0, 1, ... (at most 1023: then phi stays and the series gets DLM_ST_NOT_PD)
//   mu | .  ~ N(mean, 1 / prec):  prec = 1 / psi^2 + T (1 - phi)^2 / sigma^2,  mean = (m / psi^2 + (1 - phi) / sigma^2 sum (alpha_t - phi alpha_{t-1})) / prec
//   sigma^2 | . ~ InverseGamma(shape + T / 2, scale + 1/2 sum (alpha_t - mu - phi (alpha_{t-1} - mu))^2) = scale' / Gamma(shape', 1)
//   Beta mode: phi' ~ Beta(lambda phi + tau, lambda (1 - phi) + tau), accepted against
//       log Beta(a, b)(phi) + log N(alpha_0; mu, sigma^2 / (1 - phi^2)) + sum_t log N(alpha_t; mu + phi (alpha_{t-1} - mu), sigma^2)
//       with the full Hastings ratio (terms that do not depend on phi are left out of the target: they cancel)
// literal = 1, the reference's arithmetic: `1 / sigma * sigma` = 1 where 1 / sigma^2 belongs (Q16); the T - 1
// pairs t = 2..T everywhere, but sum (alpha_t - mu)^2 over t = 1..T in phi's precision (Q17); shape + (T + 1) / 2 (Q18); an
// unrestricted Gaussian phi (Q19).
//
// Random streams: key DLM_KEY_SV, counter (series, iteration, slot): slot t for k_t (the u2 uniform of attempt 0), DLM_SV_SLOT_* for
// the scalar draws (the slot table of dlm_draws.h).  Normals are the Box-Muller cosine of the pair at attempt k (draw_normal); gamma_unit
// is Marsaglia-Tsang; the Beta proposal is BetaProposal (all dlm_draws.h).
#include "dlm_draws.h"
#include "dlm_wave.h"

namespace dlm {

// The mixture of StochasticVolatility.scala:42-44 (pi_j, m_j, v_j), j = 0..6, and what the weights need of it:
//   SV_C[j] = log pi_j - 1/2 log(2 pi v_j),  SV_H[j] = 1 / (2 v_j),  SV_LP[j] = log pi_j
//   pi = 0.0073, 0.1056, 0.00002, 0.044, 0.34, 0.2457, 0.2575
__device__ constexpr double SV_M[7] = {-11.4, -5.24, -9.84, 1.51, -0.65, 0.53, -2.36};
__device__ constexpr double SV_V[7] = {5.8, 2.61, 5.18, 0.17, 0.64, 0.34, 1.26};
__device__ constexpr double SV_C[7] = {-6.7177484228086515, -3.6467105515819496, -12.561119345750651, -3.156525757302611,
                                       -1.7746046432623928, -1.7831777019737114, -2.3912299525647125};
__device__ constexpr double SV_H[7] = {0.08620689655172414, 0.19157088122605365, 0.09652509652509653, 2.941176470588235,
                                       0.78125, 1.4705882352941175, 0.3968253968253968};
__device__ constexpr double SV_LP[7] = {-4.919880930827792, -2.248096907709976, -10.819778284410283, -3.123565645063876,
                                        -1.0788096613719298, -1.4036439994550036, -1.3567355588783463};

__global__ __launch_bounds__(256) void k_sv_mixture(SvMixArgs a) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x, total = (long long)a.N * a.T;
  if (e >= total) return;
  // (the 64-bit division is a long sequence: only the batches that need it take it)
  const int n = total <= 0xFFFFFFFFll ? (int)((unsigned)e / (unsigned)a.T) : (int)(e / a.T);
  const int t = (int)(e - (long long)n * a.T);
  const double yt = a.y[e];
  const double ly = log(yt * yt);
  bool obs = yt == yt;
  if (obs && !(fabs(ly) < __builtin_inf())) {   // Q20: log y^2 not finite
    obs = false;
    if (a.status) atomicOr(&a.status[n], DLM_ST_NONFINITE);
  }
  if (!a.alpha) {   // initialStateAr: E log eps^2 = -1.27, Var log eps^2 = pi^2 / 2
    a.ystar[e] = obs ? ly + 1.27 : __builtin_nan("");
    a.v[e] = 4.934802200544679;
    return;
  }
  const double x = a.alpha[(size_t)n * (a.T + 1) + t + 1];
  if (!(fabs(x) < __builtin_inf()) && a.status) atomicOr(&a.status[n], DLM_ST_NONFINITE);
  double lw[7], mx = -__builtin_inf();
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const double r = (ly - SV_M[j]) - x;
    lw[j] = obs ? SV_C[j] - r * r * SV_H[j] : SV_LP[j];
    mx = lw[j] > mx ? lw[j] : mx;
  }
  double p[7], c = 0.0;
#pragma unroll
  for (int j = 0; j < 7; ++j) { c = c + exp(lw[j] - mx); p[j] = c; }
  double u1, u2;
  gibbs_rand(a.rs.seed, a.rs.series_offset + (unsigned long long)n, a.rs.iteration, (unsigned)t, 0u, 0u, u1, u2, DLM_KEY_SV);
  const double us = u2 * p[6];
  int k = 0;
#pragma unroll
  for (int j = 0; j < 6; ++j) k += us >= p[j] ? 1 : 0;
  double mk = SV_M[0], vk = SV_V[0];
#pragma unroll
  for (int j = 1; j < 7; ++j) { mk = k == j ? SV_M[j] : mk; vk = k == j ? SV_V[j] : vk; }
  a.ystar[e] = obs ? ly - mk : __builtin_nan("");
  a.v[e] = vk;
  if (a.k) a.k[e] = (signed char)k;
}

__global__ __launch_bounds__(256) __attribute__((flatten)) void k_sv_params(SvParamsArgs a) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= a.N) return;   // (whole waves: the shuffles below see every lane of the wave)
  const int T = a.T;
  const dlm_sv_prior& pr = a.prior;
  const bool lit = pr.literal != 0, beta = pr.phi_update != 0;
  const unsigned long long series = a.rs.series_offset + (unsigned long long)n, seed = a.rs.seed, it = a.rs.iteration;
  const double INF = __builtin_inf();
  const double* al = a.alpha + (size_t)n * (T + 1);
  const double phi0 = a.sv_in[(size_t)n * 3], mu0 = a.sv_in[(size_t)n * 3 + 1], sig0 = a.sv_in[(size_t)n * 3 + 2];
  bool bad = !(fabs(phi0) < INF) || !(fabs(mu0) < INF) || !(sig0 > 0.0) || !(sig0 < INF) || (beta && !(phi0 > 0.0 && phi0 < 1.0));
  const double s2 = sig0 * sig0;
  const double a0 = al[0], a1 = al[1], aT = al[T];
  const double Td = (double)T;
  int st = 0, acc = 0;
  double phi = phi0;

  if (!beta) {
    // samplePhiConjugate.  Corrected: sums over (alpha_{t-1}, alpha_t), t = 1..T.  Literal: sum (alpha_t - mu)^2 over t = 1..T and the
    // cross products over t = 2..T (Q17) -- the same lane sums, another term behind them
    double S = 0.0, S2 = 0.0;
    for (int t = 2 + lane; t <= T; t += 64) {
      const double p = al[t - 1] - mu0, c = al[t] - mu0;
      S = S + p * p;
      S2 = S2 + p * c;
    }
    const double d0 = a0 - mu0, d1 = a1 - mu0, dT = aT - mu0;
    S = wave_sum(S) + (lit ? dT * dT : d0 * d0);
    S2 = wave_sum(S2) + (lit ? 0.0 : d0 * d1);
    const double psi2 = pr.phi_b * pr.phi_b;
    const double prec = lit ? 1.0 / psi2 + S : 1.0 / psi2 + S / s2;   // Q16
    const double mean = lit ? (pr.phi_a / psi2 + S2) / prec : (pr.phi_a / psi2 + S2 / s2) / prec;
    if (!(prec > 0.0) || !(prec < INF) || !(fabs(mean) < INF)) bad = true;
    if (lane == 0 && !bad) {
      const double sd = sqrt(1.0 / prec);
      if (lit) {   // Q19: unrestricted
        phi = mean + sd * draw_normal(DLM_KEY_SV, seed, series, it, DLM_SV_SLOT_PHI);
      } else {
        bool ok = false;
        for (unsigned k = 0; k < 1023u && !ok; ++k) {
          const double cand = mean + sd * draw_normal(DLM_KEY_SV, seed, series, it, DLM_SV_SLOT_PHI, k);
          if (fabs(cand) < 1.0) { phi = cand; ok = true; }
        }
        if (!ok) st |= DLM_ST_NOT_PD;
      }
    }
  } else {
    // samplePhi: the proposal needs no data and is drawn first (lanes 0, 1), then both residual sums in one pass
    BetaProposal q;
    q.draw(lane, phi0, pr.prop_lambda, pr.prop_tau, bad, DLM_KEY_SV, seed, series, it, DLM_SV_SLOT_PROP_A, DLM_SV_SLOT_PROP_B);
    const double phip = q.phip;
    double Q0 = 0.0, Q1 = 0.0;
    for (int t = 2 + lane; t <= T; t += 64) {
      const double p = al[t - 1] - mu0, c = al[t] - mu0;
      const double r0 = c - phi0 * p, r1 = c - phip * p;
      Q0 = Q0 + r0 * r0;
      Q1 = Q1 + r1 * r1;
    }
    const double d0 = a0 - mu0, d1 = a1 - mu0;
    const double f0 = d1 - phi0 * d0, f1 = d1 - phip * d0;
    Q0 = wave_sum(Q0) + (lit ? 0.0 : f0 * f0);
    Q1 = wave_sum(Q1) + (lit ? 0.0 : f1 * f1);
    q.lgammas(lane);
    if (!(fabs(Q0) < INF)) bad = true;
    if (lane == 0 && !bad && q.ok) {
      // log target without the terms free of phi: Beta(a, b) prior, the stationary density of alpha_0, the transitions
      const double o0 = 1.0 - phi0 * phi0, o1 = 1.0 - phip * phip;
      const double lt0 = (pr.phi_a - 1.0) * log(phi0) + (pr.phi_b - 1.0) * log(1.0 - phi0) + 0.5 * log(o0) - 0.5 * d0 * d0 * o0 / s2 - 0.5 * Q0 / s2;
      const double lt1 = (pr.phi_a - 1.0) * log(phip) + (pr.phi_b - 1.0) * log(1.0 - phip) + 0.5 * log(o1) - 0.5 * d0 * d0 * o1 / s2 - 0.5 * Q1 / s2;
      const double lacc = lt1 - lt0 + q.lq_back() - q.lq_fwd();
      if (draw_log_uniform(DLM_KEY_SV, seed, series, it, DLM_SV_SLOT_ACCEPT) < lacc) { acc = 1; phi = phip; }
    }
  }
  phi = __shfl(phi, 0, 64);

  // sampleMu at the new phi
  double M = 0.0;
  for (int t = 2 + lane; t <= T; t += 64) M = M + (al[t] - phi * al[t - 1]);
  M = wave_sum(M) + (lit ? 0.0 : a1 - phi * a0);
  const double pm2 = pr.mu_sd * pr.mu_sd, omp = 1.0 - phi;
  const double mprec = lit ? 1.0 / pm2 + (Td - 1.0) * omp * omp : 1.0 / pm2 + Td * omp * omp / s2;   // Q16
  const double mmean = lit ? (pr.mu_mean / pm2 + omp * M) / mprec : (pr.mu_mean / pm2 + omp / s2 * M) / mprec;
  if (!(mprec > 0.0) || !(mprec < INF) || !(fabs(mmean) < INF)) bad = true;
  double mu = mu0;
  if (lane == 0 && !bad) mu = mmean + sqrt(1.0 / mprec) * draw_normal(DLM_KEY_SV, seed, series, it, DLM_SV_SLOT_MU);
  mu = __shfl(mu, 0, 64);

  // sampleSigma at the new phi and mu
  double Q = 0.0;
  for (int t = 2 + lane; t <= T; t += 64) {
    const double r = (al[t] - mu) - phi * (al[t - 1] - mu);
    Q = Q + r * r;
  }
  const double fr = (a1 - mu) - phi * (a0 - mu);
  Q = wave_sum(Q) + (lit ? 0.0 : fr * fr);
  const double shape = pr.sigma_shape + (lit ? (Td + 1.0) * 0.5 : Td * 0.5);   // Q18
  const double scale = pr.sigma_scale + 0.5 * Q;
  if (!(scale > 0.0) || !(scale < INF)) bad = true;
  if (lane == 0) {
    double sig = __builtin_nan("");
    if (!bad) sig = sqrt(scale / gamma_unit(shape, seed, series, it, DLM_SV_SLOT_SIGMA, DLM_KEY_SV));
    double* o = a.sv_out + (size_t)n * 3;
    o[0] = bad ? __builtin_nan("") : phi;
    o[1] = bad ? __builtin_nan("") : mu;
    o[2] = sig;
    if (a.accepted) a.accepted[n] += bad ? 0 : acc;
    if (a.status) a.status[n] = bad ? DLM_ST_NONFINITE : st;
  }
}

hipError_t launch_sv_mixture(const SvMixArgs& a, hipStream_t s) {
  const long long total = (long long)a.N * a.T;
  return launch(k_sv_mixture, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
}

hipError_t launch_sv_params(const SvParamsArgs& a, hipStream_t s) {
  return launch(k_sv_params, dim3((unsigned)((a.N + 3) / 4)), dim3(256), 0, s, a);
}

}  // namespace dlm
