// One Gibbs step of the Student-t observation DLM on the device (StudentT.step: StudentTGibbs.scala:182-212), after the FFBS
// call of its state draw.  The observation noise is the scale mixture y_t | theta_t, v_t ~ N(F_t^T theta_t, v_t),
// v_t ~ InverseGamma(nu / 2, nu s / 2), so that y_t | theta_t ~ ScaledStudentsT(nu, F_t^T theta_t, sqrt(s)).  Per series:
//   W_ii ~ InverseGamma(alpha_w + T / 2, beta_w + ss_i / 2)                    GibbsSampling.sampleSystemMatrix, Gibbs.scala:56-78
//   nu'  = Poisson(Gamma(r, nu / r)) + 1, accepted by Metropolis-Hastings      sampleNu, :141-157 (example: StudentT.scala:59-80)
//          against Poisson(lambda) x prod_obs ScaledStudentsT(nu, F^T theta_t, sqrt(s)).pdf(y_t)     ll, :65-81
//   v_t  ~ InverseGamma((nu + 1) / 2, nu s / 2 + e_t^2 / 2), e_t = y_t - F_t^T theta_t       sampleVariances, :36-54
//   s    ~ Gamma(T nu / 2 + 1, 1 / (nu / 2 sum_t 1 / v_t))                                    sampleScaleT, :89-98
// The default order is theta, W, nu | (theta, s), v | (theta, nu, s), s | (v, nu) -- nu moves with v marginalised, so v is
// redrawn behind it (a partially collapsed sampler, SURVEY/DESIGN Q15); a missing y_t draws v_t from its prior (Q13) and the
// proposal density is evaluated at to - 1, where the draw NB + 1 puts it (Q12).  DLM_OPT_STUDENTT_LITERAL runs the reference's
// arithmetic instead: v_t with the previous nu and theta_{t-1} (Q11), s with the previous nu, nu moved last (Q15), the proposal
// density at `to` (Q12), shape (nu + 1) / 2 for a missing y_t (Q13), 0.5 log(pi nu sqrt(s)) in the normaliser (Q14).
//
// One wavefront per series, lanes striding over t.  The first pass reads theta and y once and makes, per lane, the two sums of
// log1p(e^2 / (nu s)) at the current and the proposed nu (the proposal is drawn before it, on lane d) and the count of observed
// steps; the residual the variance draws need is parked in v_out[t] by the lane that will overwrite it in the second pass (the
// same thread: no barrier, and theta is not read twice).  Both reductions (these sums and sum 1 / v_t) are a lane-sequential sum
// over t = lane, lane + 64, ... followed by a xor butterfly: a fixed order, no atomics, so that a series' output does not depend
// on N or on its neighbours.  The scalar draws are made on one lane each and broadcast.  The kernel is flattened: an out-of-line
// gamma_unit costs a call frame in scratch.
//
// Random streams.  W: dlm_dinvgamma_step_batch's draw (w_draw / store_diag_draw of dlm_draws.h with p = 1: key DLM_KEY_GIBBS, component
// 1 + i), so that W_out is that call's W_out for the same statistics, seed, iteration and offset.  Everything else: key
// DLM_KEY_STUDENTT, counter (series, iteration, slot): slot t for v_t, DLM_ST_SLOT_* for the four scalar draws (the slot table of
// dlm_draws.h).  gamma_unit is Marsaglia-Tsang (dlm_draws.h); Poisson is inversion below lambda = 10 and Hormann's PTRS (1993) above.
#include "dlm_draws.h"
#include "dlm_wave.h"

namespace dlm {

// log Gamma(x) for the PTRS test: Stirling's series at x + n >= 7, recursion below (the loggam of NumPy's PTRS); lighter than lgamma
__device__ __forceinline__ double ptrs_loggam(double x) {
  if (x == 1.0 || x == 2.0) return 0.0;
  const int n = x < 7.0 ? (int)(7.0 - x) : 0;
  double x0 = x + n;
  const double x2 = (1.0 / x0) * (1.0 / x0);
  const double c[10] = {8.333333333333333e-02, -2.777777777777778e-03, 7.936507936507937e-04, -5.952380952380952e-04,
                        8.417508417508418e-04, -1.917526917526918e-03, 6.410256410256410e-03, -2.955065359477124e-02,
                        1.796443723688307e-01, -1.39243221690590e+00};
  double gl0 = c[9];
#pragma unroll
  for (int k = 8; k >= 0; --k) { gl0 *= x2; gl0 += c[k]; }
  double gl = gl0 / x0 + 0.5 * 1.8378770664093453e+00 + (x0 - 0.5) * log(x0) - x0;
  for (int k = 1; k <= n; ++k) { gl -= log(x0 - 1.0); x0 -= 1.0; }
  return gl;
}

// Poisson(lam): inversion (one uniform) for lam < 10, else PTRS (Hormann, "The transformed rejection method for generating
// Poisson random variables", 1993), two uniforms per attempt
__device__ double poisson_draw(double lam, unsigned long long seed, unsigned long long series, unsigned long long it) {
  if (!(lam > 0.0)) return 0.0;
  double u1, u2;
  if (lam < 10.0) {
    gibbs_rand(seed, series, it, DLM_ST_SLOT_POISSON, 0u, 0u, u1, u2, DLM_KEY_STUDENTT);
    double p = exp(-lam), cdf = p, k = 0.0;
    while (u2 > cdf && k < 200.0) { k += 1.0; p *= lam / k; cdf += p; }
    return k;
  }
  const double slam = sqrt(lam), loglam = log(lam);
  const double b = 0.931 + 2.53 * slam, a = -0.059 + 0.02483 * b;
  const double invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
  for (unsigned att = 0; att < 1023u; ++att) {
    gibbs_rand(seed, series, it, DLM_ST_SLOT_POISSON, att, 0u, u1, u2, DLM_KEY_STUDENTT);
    const double U = u2 - 0.5, V = u1, us = 0.5 - fabs(U);
    if (!(us > 0.0)) continue;
    const double k = floor((2.0 * a / us + b) * U + lam + 0.43);
    if (us >= 0.07 && V <= vr) return k;
    if (k < 0.0 || (us < 0.013 && V > us)) continue;
    if (log(V) + log(invalpha) - log(a / (us * us) + b) <= -lam + k * loglam - ptrs_loggam(k + 1.0)) return k;
  }
  return floor(lam);   // unreachable in practice (acceptance > 85 % per attempt)
}

__global__ __launch_bounds__(256) __attribute__((flatten)) void k_studentt_step(StudentTArgs a) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= a.N) return;   // (whole waves: the shuffles below see every lane of the wave)
  const int d = a.d, T = a.T;
  const bool lit = a.literal != 0;
  const unsigned long long series = a.rs.series_offset + (unsigned long long)n, seed = a.rs.seed, it = a.rs.iteration;
  const double s = a.scale_in[n];
  const int nu = a.nu_in[n];
  const double* th = a.theta + (size_t)n * (T + 1) * d;
  const double* yn = a.y + (size_t)n * T;
  double* vn = a.v_out + (size_t)n * T;
  bool bad = !(nu >= 1) || !(s > 0.0) || !(s < __builtin_inf());
  const double r = a.prior.prop_nu_size, dnu = (double)nu;

  // the Gamma draws that need no data, one per lane: W_ii as dlm_dinvgamma_step_batch draws it (p = 1: stats = [ssy | n | ss (d) | T])
  // for j = i < d; for j = d the proposal's lambda ~ Gamma(r, q / (1 - q)), q = nu / (r + nu) (Breeze's NegativeBinomial(r, q)
  // draws Poisson(lambda)), then nu' = Poisson(lambda) + 1
  const double* st = a.stats + (size_t)n * (d + 3);
  double* Wn = a.W_out + (size_t)n * d * d;
  double nup = 0.0;
  for (int j = lane; j <= d; j += 64) {
    const bool w = j < d;
    const double q = dnu / (r + dnu);
    const InvGammaDraw wq = w ? w_draw(st, d, 1, j, a.prior.prior_w_shape, a.prior.prior_w_scale) : InvGammaDraw{r, 0.0, DLM_ST_SLOT_PROP_GAMMA};
    const double g = bad ? __builtin_nan("") : gamma_unit(wq.shape, seed, series, it, wq.comp, w ? DLM_KEY_GIBBS : DLM_KEY_STUDENTT);
    if (w) {
      store_diag_draw(Wn, d, j, wq, g);
    } else if (!bad) {
      nup = poisson_draw(g * (q / (1.0 - q)), seed, series, it) + 1.0;
    }
  }
  nup = __shfl(nup, d & 63, 64);
  const bool prop_ok = nup >= 1.0 && nup < 1.0e9;   // a proposal beyond int32 is rejected (Poisson(lambda) prior: never accepted anyway)

  // pass 1: e_t = y_t - F_t^T theta_t (record t + 1) for the likelihood; the residual of the variance draw parked in v_out[t]
  const double sc = sqrt(s);
  const double den0 = lit ? dnu * sc * sc : dnu * s, den1 = lit ? nup * sc * sc : nup * s;
  double A0 = 0.0, A1 = 0.0;
  int nobs = 0;
  bool nonfin = false;
  for (int t = lane; t < T; t += 64) {
    const double* Ft = a.F + (a.f_stride ? (size_t)t * a.f_stride : 0);
    const double* x1 = th + (size_t)(t + 1) * d;
    double f1 = 0.0;
    for (int i = 0; i < d; ++i) f1 += Ft[i] * x1[i];
    const double yt = yn[t];
    const double e1 = yt - f1;
    double e = e1;
    if (lit) {   // Q11: y_t against theta_{t-1} (record t), F at its time (time-invariant F only)
      const double* x0 = th + (size_t)t * d;
      double f0 = 0.0;
      for (int i = 0; i < d; ++i) f0 += a.F[i] * x0[i];
      nonfin |= !(fabs(f0) < __builtin_inf());
      e = yt - f0;
    }
    nonfin |= !(fabs(f1) < __builtin_inf());
    if (yt == yt) {
      ++nobs;
      A0 += log1p(e1 * e1 / den0);
      A1 += log1p(e1 * e1 / den1);
    }
    vn[t] = e;   // NaN where y_t is missing
  }
  A0 = wave_sum(A0); A1 = wave_sum(A1);
  nobs = wave_sum_int(nobs);
  bad |= __any(nonfin) != 0;

  // Metropolis-Hastings on nu.  log measure(k) = ll(k) + log Poisson(lambda).pmf(k), ll(k) = sum over the observed steps of
  // ScaledStudentsT(k, F^T theta_t, sqrt(s)).logPdf(y_t); proposal density propP(from, to) = log NB(r, from / (r + from)).pmf(to - 1)
  // (Q12: the literal mode evaluates it at `to`).  The eleven lgamma values it needs are made side by side, one per lane.
  const double off = lit ? 0.0 : 1.0, k1 = dnu - off, k2 = nup - off;   // the NB arguments of propP(nu', nu) and propP(nu, nu')
  double garg = 1.0;
  switch (lane) {
    case 0: garg = (dnu + 1.0) * 0.5; break;  case 1: garg = dnu * 0.5; break;
    case 2: garg = (nup + 1.0) * 0.5; break;  case 3: garg = nup * 0.5; break;
    case 4: garg = dnu + 1.0; break;          case 5: garg = nup + 1.0; break;
    case 6: garg = r + k1; break;             case 7: garg = k1 + 1.0; break;
    case 8: garg = r; break;
    case 9: garg = r + k2; break;             case 10: garg = k2 + 1.0; break;
    default: break;
  }
  const double lg = lgamma(garg);
  double G[11];
#pragma unroll
  for (int j = 0; j < 11; ++j) G[j] = __shfl(lg, j, 64);
  int acc = 0, nu_v = nu;
  double ll_out = 0.0;
  if (lane == 0 && !bad) {
    const double lam = a.prior.prior_nu_rate, nobsd = (double)nobs, PI = 3.141592653589793;
    const double c0 = lit ? sc : s;   // Q14: the reference's normaliser has the scale sqrt(s) where s belongs
    const double ll0 = nobsd * (G[0] - 0.5 * log(PI * dnu * c0) - G[1]) - (dnu + 1.0) * 0.5 * A0;
    ll_out = ll0;
    if (prop_ok) {
      const double ll1 = nobsd * (G[2] - 0.5 * log(PI * nup * c0) - G[3]) - (nup + 1.0) * 0.5 * A1;
      const double lm0 = ll0 + (dnu * log(lam) - lam - G[4]), lm1 = ll1 + (nup * log(lam) - lam - G[5]);
      const double q1 = nup / (r + nup), q2 = dnu / (r + dnu);
      const double pp1 = G[6] - G[7] - G[8] + r * log(1.0 - q1) + k1 * log(q1);   // propP(nu', nu)
      const double pp2 = G[9] - G[10] - G[8] + r * log(1.0 - q2) + k2 * log(q2);  // propP(nu, nu')
      const double lacc = lm1 + pp1 - lm0 - pp2;
      if (draw_log_uniform(DLM_KEY_STUDENTT, seed, series, it, DLM_ST_SLOT_ACCEPT) < lacc) { acc = 1; ll_out = ll1; }
    }
    nu_v = (acc && !lit) ? (int)nup : nu;   // the nu of the variance and scale draws: the new one (Q15), the old one when literal
  }
  nu_v = __shfl(nu_v, 0, 64);
  const double dnv = (double)nu_v;

  // pass 2: v_t ~ InverseGamma(alpha, beta) = beta / Gamma(alpha, 1), and sum 1 / v_t; then (one more round of the same loop, on
  // lane T % 64) s ~ Gamma(T nu / 2 + 1, scale 1 / rate), rate = nu / 2 sum 1 / v_t
  double R = 0.0;
  for (int t = lane; t < T; t += 64) {
    double v = __builtin_nan("");
    if (!bad) {
      const double e = vn[t];
      const bool obs = e == e;
      const double shape = (obs || lit) ? (dnv + 1.0) * 0.5 : dnv * 0.5;   // Q13
      const double beta = dnv * s * 0.5 + (obs ? e * e * 0.5 : 0.0);
      v = beta / gamma_unit(shape, seed, series, it, (unsigned)t, DLM_KEY_STUDENTT);
      R += 1.0 / v;
    }
    vn[t] = v;
  }
  R = wave_sum(R);
  if (lane == 0) {
    double snew = __builtin_nan("");
    if (!bad) snew = gamma_unit((double)T * dnv * 0.5 + 1.0, seed, series, it, DLM_ST_SLOT_SCALE, DLM_KEY_STUDENTT) / (dnv * 0.5 * R);
    a.scale_out[n] = snew;
    a.nu_out[n] = bad ? nu : (acc ? (int)nup : nu);
    a.accepted[n] += acc;
    if (a.loglik) a.loglik[n] = bad ? __builtin_nan("") : ll_out;
    if (a.status) a.status[n] = bad ? DLM_ST_NONFINITE : 0;
  }
}

hipError_t launch_studentt_step(const StudentTArgs& a, hipStream_t s) {
  return launch(k_studentt_step, dim3((unsigned)((a.N + 3) / 4)), dim3(256), 0, s, a);
}

}  // namespace dlm
