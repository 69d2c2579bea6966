// The parameter step of the stochastic-volatility sampler with Ornstein-Uhlenbeck log-volatility on an irregular time grid
// (StochasticVolatility.sampleOu / stepOu, StochasticVolatility.scala:343-500): three Metropolis moves against the OU transition
// likelihood, after dlm_sv_mixture_batch (dlm_sv.hip, as it is: per element, no time grid) and dlm_ou_ffbs_batch (dlm_ar1.hip).
//   alpha(t + dt) | alpha(t) ~ N(mu + e^(-phi dt) (alpha(t) - mu), sigma^2 (1 - e^(-2 phi dt)) / (2 phi)),   phi > 0 the rate
// alpha rows are [T+1] as dlm_ou_ffbs_batch writes its theta: alpha[0] and alpha[1] both sit at times[0] (the reference's first dt is
// 0), alpha[t] belongs to times[t-1]; the informative pairs are (alpha[t-1], alpha[t]), t = 2..T, with dt_t = times[t-1] - times[t-2].
// A pair with dt = 0 contributes nothing (ouLikelihood, :360-361); n = #{t : dt_t > 0}.
//
// With e_t = exp(-phi dt_t), g_t = -expm1(-2 phi dt_t) (= 1 - e_t^2; the reference's 1 - exp(..) loses digits on short gaps: this
// form in both modes) and d_t = alpha[t] - mu0, mu0 the incoming mu:
//   log p(alpha | phi, mu, sigma) = -n/2 log 2 pi - n log sigma + n/2 log(2 phi) - L(phi) / 2 - phi Q(phi, mu) / sigma^2
//   L = sum log g_t,  A = sum (d_t - e_t d_{t-1})^2 / g_t,  B = sum (d_t - e_t d_{t-1}) (1 - e_t) / g_t,  C = sum (1 - e_t)^2 / g_t
//   Q(phi, mu0 + delta) = A - 2 delta B + delta^2 C
// sigma's move needs no sum of its own and mu's needs (A, B, C) at the phi that survived, so the wave reads its row ONCE and
// accumulates (L, A, B, C) at phi and at the proposed phi' -- eight sums; the proposal needs no data and is drawn first.  Behind the
// reduction the three accept decisions are scalar work on lane 0.  (Three passes in the style of k_sv_params would read the row, and
// take its exps and logs, three times.)
//
// k_sv_ou_params is one wavefront per series, four per block; every reduction is lane-sequential over t = 2 + lane, 2 + lane + 64, ...
// followed by the xor butterfly (wave_sum): a fixed order, no atomics, a series' output depends on neither N nor its neighbours.
//
// The moves, in the reference's order (stepOu, :459-478); each accepts when log u < Delta:
//   phi'   ~ Beta(lambda phi + tau, lambda (1 - phi) + tau) as ga / (ga + gb) (a phi' that rounds to 0 or 1 is rejected); prior Beta(a, b);
//            target (a - 1) log phi + (b - 1) log(1 - phi) + n/2 log(2 phi) - L(phi) / 2 - phi A(phi) / sigma0^2
//   sigma' = sigma0 exp(delta_sigma z) at the new phi; prior InverseGamma(shape, scale) on sigma ITSELF (priorSigma.logPdf(newSigma), :407);
//            target -(shape + 1) log sigma - scale / sigma - n log sigma - phi A(phi) / sigma^2
//   mu'    = mu0 + delta_mu z at the new phi and sigma; prior Gaussian(mean, sd); target -(mu - m)^2 / (2 s^2) - phi Q(phi, mu) / sigma^2
// Default arithmetic against literal = 1, the reference's:
//   Q23  Metropolis.mAccept is plain Metropolis: the default adds lq_back - lq_fwd of the Beta proposal and log(sigma' / sigma) of the
//        log-normal walk; literal adds neither.
//   Q24  ouLikelihood has no term for the initial state, which FilterOu draws from N(mu, c0 = sigma^2): the default's sigma and mu
//        targets carry -log sigma - (alpha_0 - mu)^2 / (2 sigma^2); literal leaves it out.
//   Q22  (lambda = 0.05 where tau was meant) is the caller's choice of arguments; Q25 (sigma and mu start from the incoming values and
//        see the new phi, sigma) is the order above.
//
// Random streams: key DLM_KEY_SVOU, counter (series, iteration, slot), the seven slots below.  Normals are the Box-Muller cosine of
// attempt 0 (draw_normal), the uniforms come as their logs (draw_log_uniform), gamma_unit is Marsaglia-Tsang and the Beta proposal is
// BetaProposal, k_sv_params' own (all dlm_draws.h, with the slot table).  The kernel is flattened, as k_sv_params is.
#include "dlm_draws.h"
#include "dlm_wave.h"

namespace dlm {

__global__ __launch_bounds__(256) __attribute__((flatten)) void k_sv_ou_params(SvOuParamsArgs a) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= a.N) return;   // (whole waves: the shuffles below see every lane of the wave)
  const int T = a.T;
  const dlm_sv_ou_prior& pr = a.prior;
  const bool lit = pr.literal != 0;
  const unsigned long long series = a.rs.series_offset + (unsigned long long)n, seed = a.rs.seed, it = a.rs.iteration;
  const double INF = __builtin_inf();
  const double* al = a.alpha + (size_t)n * (T + 1);
  const double* tm = a.times;
  const double phi0 = a.sv_in[(size_t)n * 3], mu0 = a.sv_in[(size_t)n * 3 + 1], sig0 = a.sv_in[(size_t)n * 3 + 2];
  bool bad = !(phi0 > 0.0 && phi0 < 1.0) || !(fabs(mu0) < INF) || !(sig0 > 0.0) || !(sig0 < INF);

  // samplePhiOu's proposal (lanes 0, 1)
  BetaProposal q;
  q.draw(lane, phi0, pr.prop_lambda, pr.prop_tau, bad, DLM_KEY_SVOU, seed, series, it, DLM_SVOU_SLOT_PROP_A, DLM_SVOU_SLOT_PROP_B);
  const double phip = q.phip;

  // the row, once: (L, A, B, C) at phi0 and at phi'
  double L0 = 0.0, SA0 = 0.0, SB0 = 0.0, SC0 = 0.0, L1 = 0.0, SA1 = 0.0, SB1 = 0.0, SC1 = 0.0;
  int cnt = 0, tbad = 0;
  for (int t = 2 + lane; t <= T; t += 64) {
    const double dt = tm[t - 1] - tm[t - 2];
    if (!(dt >= 0.0) || !(dt < INF)) tbad = 1;
    if (dt > 0.0) {
      const double p = al[t - 1] - mu0, c = al[t] - mu0;
      const double e0 = exp(-phi0 * dt), g0 = -expm1(-2.0 * phi0 * dt), ig0 = 1.0 / g0;   // one reciprocal serves three sums
      const double e1 = exp(-phip * dt), g1 = -expm1(-2.0 * phip * dt), ig1 = 1.0 / g1;
      const double r0 = c - e0 * p, w0 = 1.0 - e0, r1 = c - e1 * p, w1 = 1.0 - e1;
      L0 = L0 + log(g0);
      SA0 = SA0 + r0 * r0 * ig0;
      SB0 = SB0 + r0 * w0 * ig0;
      SC0 = SC0 + w0 * w0 * ig0;
      L1 = L1 + log(g1);
      SA1 = SA1 + r1 * r1 * ig1;
      SB1 = SB1 + r1 * w1 * ig1;
      SC1 = SC1 + w1 * w1 * ig1;
      ++cnt;
    }
  }
  L0 = wave_sum(L0); SA0 = wave_sum(SA0); SB0 = wave_sum(SB0); SC0 = wave_sum(SC0);
  L1 = wave_sum(L1); SA1 = wave_sum(SA1); SB1 = wave_sum(SB1); SC1 = wave_sum(SC1);
  const double nd = (double)wave_sum_int(cnt);
  if (wave_sum_int(tbad) != 0) bad = true;   // the grid is the batch's: every series finds it
  if (!(fabs(L0) < INF) || !(fabs(SA0) < INF) || !(fabs(SB0) < INF) || !(fabs(SC0) < INF)) bad = true;

  // the Beta proposal's six lgamma values side by side, one per lane
  q.lgammas(lane);

  if (lane != 0) return;
  double* o = a.sv_out + (size_t)n * 3;
  if (bad) {
    o[0] = o[1] = o[2] = __builtin_nan("");
    if (a.status) a.status[n] = DLM_ST_NONFINITE;
    return;
  }
  int acc_phi = 0, acc_sig = 0, acc_mu = 0;

  // phi
  double phi = phi0, SA = SA0, SB = SB0, SC = SC0;
  if (q.ok) {
    const double s2 = sig0 * sig0;
    const double lt0 = (pr.phi_a - 1.0) * log(phi0) + (pr.phi_b - 1.0) * log(1.0 - phi0) + 0.5 * nd * log(2.0 * phi0) - 0.5 * L0 - phi0 * SA0 / s2;
    const double lt1 = (pr.phi_a - 1.0) * log(phip) + (pr.phi_b - 1.0) * log(1.0 - phip) + 0.5 * nd * log(2.0 * phip) - 0.5 * L1 - phip * SA1 / s2;
    const double lacc = lit ? lt1 - lt0 : lt1 - lt0 + q.lq_back() - q.lq_fwd();   // Q23
    if (draw_log_uniform(DLM_KEY_SVOU, seed, series, it, DLM_SVOU_SLOT_ACC_PHI) < lacc) { acc_phi = 1; phi = phip; SA = SA1; SB = SB1; SC = SC1; }
  }

  // sigma at the new phi, from sig0 (Q25)
  const double d0 = al[0] - mu0;
  double sig = sig0;
  {
    const double sigp = sig0 * exp(pr.delta_sigma * draw_normal(DLM_KEY_SVOU, seed, series, it, DLM_SVOU_SLOT_Z_SIGMA));
    if (sigp > 0.0 && sigp < INF) {
      const double ls0 = log(sig0), ls1 = log(sigp);
      double lt0 = -(pr.sigma_shape + 1.0) * ls0 - pr.sigma_scale / sig0 - nd * ls0 - phi * SA / (sig0 * sig0);
      double lt1 = -(pr.sigma_shape + 1.0) * ls1 - pr.sigma_scale / sigp - nd * ls1 - phi * SA / (sigp * sigp);
      if (!lit) {   // Q24, Q23
        lt0 = lt0 - ls0 - d0 * d0 / (2.0 * sig0 * sig0);
        lt1 = lt1 - ls1 - d0 * d0 / (2.0 * sigp * sigp);
      }
      const double lacc = lit ? lt1 - lt0 : lt1 - lt0 + log(sigp / sig0);
      if (draw_log_uniform(DLM_KEY_SVOU, seed, series, it, DLM_SVOU_SLOT_ACC_SIGMA) < lacc) { acc_sig = 1; sig = sigp; }
    }
  }

  // mu at the new phi and sigma, from mu0 (Q25)
  double mu = mu0;
  {
    const double mup = mu0 + pr.delta_mu * draw_normal(DLM_KEY_SVOU, seed, series, it, DLM_SVOU_SLOT_Z_MU);
    const double dl = mup - mu0, s2 = sig * sig, ps2 = pr.mu_sd * pr.mu_sd;
    const double Q1 = SA - 2.0 * dl * SB + dl * dl * SC;
    const double m0 = mu0 - pr.mu_mean, m1 = mup - pr.mu_mean;
    double lt0 = -(m0 * m0) / (2.0 * ps2) - phi * SA / s2;
    double lt1 = -(m1 * m1) / (2.0 * ps2) - phi * Q1 / s2;
    if (!lit) {   // Q24
      const double d1 = al[0] - mup;
      lt0 = lt0 - d0 * d0 / (2.0 * s2);
      lt1 = lt1 - d1 * d1 / (2.0 * s2);
    }
    if (draw_log_uniform(DLM_KEY_SVOU, seed, series, it, DLM_SVOU_SLOT_ACC_MU) < lt1 - lt0) { acc_mu = 1; mu = mup; }
  }

  o[0] = phi; o[1] = mu; o[2] = sig;
  int* ac = a.accepted + (size_t)n * 3;
  ac[0] += acc_phi; ac[1] += acc_sig; ac[2] += acc_mu;
  if (a.status) a.status[n] = 0;
}

hipError_t launch_sv_ou_params(const SvOuParamsArgs& a, hipStream_t s) {
  return launch(k_sv_ou_params, dim3((unsigned)((a.N + 3) / 4)), dim3(256), 0, s, a);
}

}  // namespace dlm
