// Particle Gibbs for a dynamic generalised linear model: one conditional-SMC sweep with ancestor sampling per series (Andrieu, Doucet &
// Holenstein 2010; Lindsten, Jordan & Schoen 2014; what ParticleGibbs.scala aims at -- DESIGN.md 2, Q67-Q70 say why its step is not restated):
// dlm_pg_batch.  k_pf's layout: ONE WAVEFRONT PER SERIES, particle i = 64 s + lane in slot s of its lane, the cloud component-major in LDS
// x[k][i] next to the weights wg[i], the row `cum` (the running sums of a search, the ancestor-sampling densities, the log-weights, the row a
// component is gathered through), the ancestors, ONE d x d factor (chol(C0) for the initial cloud, chol(W) from then on) and ref_{t+1} [d].
// Particle P - 1 is the reference particle: it is never drawn, its state is ref_t at every t, and with ancestor sampling its ancestor is
// drawn from W_{t-1,j} N(ref_{t+1}; G_t x_t,j, W dt_t).  EVERY step resamples.
//
// What the trace-back needs -- the cloud x_t [d][P] and the ancestors a_t [P] of every step -- goes to HBM as whole rows of P (64 consecutive
// doubles or ints per slot and lane row: coalesced), a.clouds [T+1][d][P] and a.ancestors [T][P] of the launch's block.  After the last step
// the wave draws k_T, fences, and walks back k_{t-1} = a_{t-1,k_t}: lane c < D carries component c of path_t, the statistics of the drawn path
// are summed on the way (t descending; products with the index ascending, the first product starting the sum).
//
// Every reduction runs in k_pf's FIXED orders (dlm_pf.hip; tests/pg_restatement.py follows them operation for operation).  No atomics, no
// dependence on N, on the neighbours or on how the host split the batch into launches.
#include "dlm_pf_common.h"

namespace dlm {
namespace {

// z ~ N(0, I_D) of (slot, particle): block q gives the components 2 q (cosine) and 2 q + 1 (sine), each Philox block drawn once
template <int D>
__device__ __forceinline__ void pg_normals(const DrawStream& rs, unsigned long long series, unsigned slot, unsigned particle, double (&z)[D]) {
#pragma unroll
  for (int q = 0; q < (D + 1) / 2; ++q) {
    double u1, u2;
    gibbs_rand(rs.seed, series, rs.iteration, slot, particle, 0u, u1, u2, DLM_KEY_PG | (unsigned)q);
    const double r = sqrt(-2.0 * log(u1)), ang = PF_2PI * u2;
    z[2 * q] = r * cos(ang);
    if (2 * q + 1 < D) z[2 * q + 1] = r * sin(ang);
  }
}

// the [0, 1) uniform of (slot, particle) in `block`
__device__ __forceinline__ double pg_uniform(const DrawStream& rs, unsigned long long series, unsigned slot, unsigned particle, unsigned block) {
  double u1, u2;
  gibbs_rand(rs.seed, series, rs.iteration, slot, particle, 0u, u1, u2, DLM_KEY_PG | block);
  return u2;
}

// ref_t (d doubles) into LDS; false when an entry is not finite
template <int D>
__device__ __forceinline__ bool pg_load_ref(const double* ref_t, double* rf, int lane) {
  double v = 0.0;
  if (lane < D) { v = ref_t[lane]; rf[lane] = v; }
  const double worst = wave_max(fabs(v) < __builtin_inf() ? 0.0 : 1.0);
  wave_sync();
  return worst == 0.0;
}

// one row of P doubles / ints of LDS to HBM
__device__ __forceinline__ void pg_store_rows(double* out, const double* x, int count, int lane) {
  for (int j = lane; j < count; j += 64) out[j] = x[j];
}

template <int D>
__global__ __launch_bounds__(64, D <= 8 ? 2 : 1) void k_pg(PgArgs a) {
  extern __shared__ double pg_lds[];
  const int nb = blockIdx.x, n = a.n_first + nb, lane = threadIdx.x, P = a.P, T = a.T;
  double* x = pg_lds;              // [D][P]
  double* wg = x + (size_t)D * P;  // [P] the normalised weights W_t,i
  double* cum = wg + P;            // [P]
  double* sl = cum + P;            // [D][D] row-major
  double* rf = sl + D * D;         // [D] ref_{t+1}
  int* anc = (int*)(rf + D);       // [P]
  const unsigned long long series = a.rs.series_offset + (unsigned long long)n;
  const double rP = 1.0 / (double)P;
  const double* y = a.y + (size_t)n * T;
  const double* ref = a.ref + (size_t)n * (T + 1) * D;
  double* clouds = a.clouds + (size_t)nb * (T + 1) * D * P;
  int* ancs = a.ancestors + (size_t)nb * T * P;
  double* stepw = a.step_weights ? a.step_weights + (size_t)n * T * P : nullptr;

  int bad = 0;
  double ll = 0.0;

  // ---- the initial cloud x_0,i = m0 + chol(C0) z with x_0,P-1 = ref_0, then chol(W) for the steps
  if (!pf_chol<D>(a.C0 + (size_t)n * a.c0_stride, sl, lane)) bad = DLM_ST_NOT_PD;
  if (!bad) {
    pf_init_cloud<D>(a.m0 + (size_t)n * a.m0_stride, sl, x, wg, rP, P, lane,
                     [&](int i, double (&z)[D]) { pg_normals<D>(a.rs, series, DLM_PG_SLOT_INIT, (unsigned)i, z); }, [](int, int) {});
    wave_sync();
    if (!pf_chol<D>(a.W + (size_t)n * a.w_stride, sl, lane)) bad = DLM_ST_NOT_PD;
  }
  if (!bad && !pg_load_ref<D>(ref, rf, lane)) bad = DLM_ST_NONFINITE;
  if (!bad) {
    if (lane < D) x[lane * P + (P - 1)] = rf[lane];
    wave_sync();
    pg_store_rows(clouds, x, D * P, lane);
  }

  if (!bad) {
    const double v = a.V[(size_t)n * a.v_stride], nu = a.obs_param ? a.obs_param[n] : 0.0;
    for (int t = 0; t < T; ++t) {
      const double yt = y[t];
      const bool missing = yt != yt;
      const double dte = a.dt ? a.dt[t] : 1.0;
      const double* G = a.G + (size_t)(a.g_index ? a.g_index[t] : 0) * (D * D);

      // -- the ancestors of the free particles: multinomial under W_{t-1}
      const double total = pf_running_sums(wg, cum, P, lane);
      wave_sync();
      pf_search(DLM_KEY_PG | DLM_PG_BLOCK_RESAMPLE, a.rs, series, (unsigned)t, cum, total, anc, P, lane);
      wave_sync();

      // -- the reference's: itself, or drawn from omega_j = W_{t-1,j} exp(q_j - max q)
      int aref = P - 1;
      if (dte != 0.0) {
        if (!pg_load_ref<D>(ref + (size_t)(t + 1) * D, rf, lane)) { bad = DLM_ST_NONFINITE; break; }
        if (a.ancestor_sampling) {
          double mx = -__builtin_inf();
          for (int i = lane; i < P; i += 64) {
            double xo[D], e[D];
#pragma unroll
            for (int c = 0; c < D; ++c) xo[c] = x[c * P + i];
            double q = 0.0;
#pragma nounroll
            for (int r = 0; r < D; ++r) {   // e = L^-1 (ref - G x), row by row
              double gx = G[r] * xo[0];
#pragma unroll
              for (int c = 1; c < D; ++c) gx = gx + G[r + c * D] * xo[c];
              double s = rf[r] - gx;
#pragma unroll
              for (int c = 0; c < D; ++c) if (c < r) s = s - sl[r * D + c] * e[c];
              s = s / sl[r * D + r];
#pragma unroll
              for (int c = 0; c < D; ++c) if (c == r) e[c] = s;
              q = q + s * s;
            }
            q = (-0.5 * q) / dte;
            cum[i] = q;
            mx = fmax(mx, q);
          }
          const double m = wave_max(mx);
          if (!(fabs(m) < __builtin_inf())) { bad = DLM_ST_NONFINITE; break; }
          for (int i = lane; i < P; i += 64) cum[i] = wg[i] * exp(cum[i] - m);
          const double tot = pf_running_sums(cum, cum, P, lane);
          if (!(tot > 0.0 && tot < __builtin_inf())) { bad = DLM_ST_NONFINITE; break; }
          wave_sync();
          aref = pf_ancestor(cum, P, pg_uniform(a.rs, series, (unsigned)t, (unsigned)(P - 1), DLM_PG_BLOCK_REF) * tot);
          wave_sync();
        }
      }
      if (lane == 63) anc[P - 1] = aref;
      wave_sync();
      for (int i = lane; i < P; i += 64) ancs[(size_t)t * P + i] = anc[i];

      pf_gather(x, D, cum, anc, P, lane);   // component by component

      // -- advance the free particles: x <- G x + sqrt(dt) L z (dt == 0: no advance, no noise); the reference moves to ref_{t+1}
      if (dte != 0.0) {
        const double sdt = sqrt(dte);
        for (int i = lane; i < P; i += 64) {
          double z[D], xo[D];
          pg_normals<D>(a.rs, series, (unsigned)t, (unsigned)i, z);
#pragma unroll
          for (int c = 0; c < D; ++c) xo[c] = x[c * P + i];
#pragma nounroll
          for (int r = 0; r < D; ++r) {
            double gx = G[r] * xo[0];
#pragma unroll
            for (int c = 1; c < D; ++c) gx = gx + G[r + c * D] * xo[c];
            double lz = sl[r * D] * z[0];
#pragma unroll
            for (int c = 1; c < D; ++c) lz = lz + sl[r * D + c] * z[c];
            x[r * P + i] = (i == P - 1) ? rf[r] : gx + sdt * lz;
          }
        }
        wave_sync();
      }
      pg_store_rows(clouds + (size_t)(t + 1) * D * P, x, D * P, lane);

      // -- the weights: every step starts from 1 / P
      if (missing) {
        for (int i = lane; i < P; i += 64) wg[i] = rP;
      } else {
        const PfObs ob = pf_obs(a.family, 0, yt, v, nu);
        const double* F = a.F + (size_t)t * a.f_stride;
        double mx = -__builtin_inf();
        for (int i = lane; i < P; i += 64) {
          double eta = F[0] * x[i];
#pragma unroll
          for (int k = 1; k < D; ++k) eta = eta + F[k] * x[k * P + i];
          const double l = pf_logdens(a.family, ob, eta);
          cum[i] = l;
          mx = fmax(mx, l);
        }
        const double m = wave_max(mx);
        if (!(fabs(m) < __builtin_inf())) { bad = DLM_ST_NONFINITE; break; }
        double part = 0.0;
        for (int i = lane; i < P; i += 64) {
          const double w = exp(cum[i] - m);
          wg[i] = w;
          part = part + w;
        }
        const double stot = wave_sum(part);
        if (!(stot > 0.0 && stot < __builtin_inf())) { bad = DLM_ST_NONFINITE; break; }
        ll = ll + (m + log(stot / (double)P));
        (void)pf_normalise(wg, stot, P, lane);
      }
      wave_sync();
      if (stepw) pg_store_rows(stepw + (size_t)t * P, wg, P, lane);
    }
  }

  // ---- the final index, then the trace-back with the statistics of the drawn path
  double* path = a.path + (size_t)n * (T + 1) * D;
  double* so = a.stats + (size_t)n * (D + 3);
  int* kout = a.path_index ? a.path_index + (size_t)n * (T + 1) : nullptr;
  if (!bad) {
    const double total = pf_running_sums(wg, cum, P, lane);
    wave_sync();
    int k = pf_ancestor(cum, P, pg_uniform(a.rs, series, DLM_PG_SLOT_INIT, 0u, DLM_PG_BLOCK_FINAL) * total);
    __threadfence();   // the rows this wave wrote are what its lanes read back
    double pn = lane < D ? clouds[((size_t)T * D + lane) * P + k] : 0.0;   // component `lane` of path_{t+1}
    if (lane < D) path[(size_t)T * D + lane] = pn;
    if (kout && lane == 0) kout[T] = k;
    double ss = 0.0, ssy = 0.0, nob = 0.0;
    for (int t = T - 1; t >= 0; --t) {
      k = min(max(ancs[(size_t)t * P + k], 0), P - 1);   // (read back from HBM: whatever it holds, it never becomes an address outside the cloud)
      const double pt = lane < D ? clouds[((size_t)t * D + lane) * P + k] : 0.0;
      if (a.family == DLM_OBS_GAUSSIAN) {
        const double yt = y[t];
        if (yt == yt) {
          const double* F = a.F + (size_t)t * a.f_stride;
          double f = F[0] * __shfl(pn, 0, 64);
#pragma unroll
          for (int c = 1; c < D; ++c) f = f + F[c] * __shfl(pn, c, 64);
          ssy = ssy + (yt - f) * (yt - f);
          nob = nob + 1.0;
        }
      }
      const double dte = a.dt ? a.dt[t] : 1.0;
      if (dte != 0.0) {
        const double* G = a.G + (size_t)(a.g_index ? a.g_index[t] : 0) * (D * D);
        const int r = lane < D ? lane : 0;
        double gx = G[r] * __shfl(pt, 0, 64);
#pragma unroll
        for (int c = 1; c < D; ++c) gx = gx + G[r + c * D] * __shfl(pt, c, 64);
        const double e = pn - gx;
        ss = ss + (e * e) / dte;
      }
      if (lane < D) path[(size_t)t * D + lane] = pt;
      if (kout && lane == 0) kout[t] = k;
      pn = pt;
    }
    if (lane < D) so[2 + lane] = ss;
    if (lane == 0) { so[0] = ssy; so[1] = nob; so[D + 2] = (double)T; }
  } else {
    ll = -__builtin_inf();
    pf_no_results(path, D, 0, T + 1, lane);
    pf_no_results(so, D + 3, 0, 1, lane);
  }
  if (lane == 0) {
    a.ll[n] = ll;
    if (a.status && bad) a.status[n] = bad;
  }
}

}  // namespace

size_t pg_lds_bytes(int d, int P) { return pf_lds_bytes(d, P) + (size_t)d * sizeof(double); }

hipError_t launch_pg(const PgArgs& a, int n_series, hipStream_t s) {
  return pick<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(a.d, [&](auto D) {
    return launch(k_pg<decltype(D)::value>, dim3((unsigned)n_series), dim3(64), pg_lds_bytes(a.d, a.P), s, a);
  });
}

}  // namespace dlm
