// The scalar draws of the Gibbs parameter steps (dlm_gibbs.hip, dlm_studentt.hip, dlm_sv.hip, dlm_sv_ou.hip, dlm_fsv.hip), each defined here ONCE:
// the Philox uniforms under a stream key, the Gamma, normal and log-uniform variates, the Beta proposal of the two stochastic-volatility
// steps, the conjugate draw of a diagonal W, and the table of counter slots (dlm_engine.hip takes its limits on T from it).
#pragma once
#include "dlm_internal.h"

namespace dlm {

// ---- the streams ----------------------------------------------------------------------------------------------------------------
// Counter (series lo, series hi, iteration, comp * 2048 + attempt * 2 + which) under the key (seed lo, seed hi ^ key): one stream per
// key, each disjoint from the FFBS / simulation normals (key (seed lo, seed hi)) and from the others.  oracle/dlm_oracle.c restates the
// GIBB stream.
//   DLM_KEY_GIBBS     dlm_dinvgamma_step_batch: comp = component of [V diagonal (p) | W diagonal (d)]; the Student-t step draws W here too
//   DLM_KEY_STUDENTT  dlm_studentt_step_batch: comp = t for the variance v_t, DLM_ST_SLOT_* for its scalar draws
//   DLM_KEY_SV        dlm_sv_mixture_batch: comp = t for the mixture indicator k_t; dlm_sv_params_batch: DLM_SV_SLOT_*
//   DLM_KEY_SVOU      dlm_sv_ou_params_batch: DLM_SVOU_SLOT_*; the OU chain's mixture call draws under DLM_KEY_SV
//   DLM_KEY_FSV       dlm_fsv_factors_batch: comp = t, attempt j for the normal of factor j at time t; dlm_fsv_loadings_batch: DLM_FSV_SLOT_*
//                     (the factor chains' volatility calls draw under DLM_KEY_SV at the series (series_offset + n) k + j)
//   DLM_KEY_DLMFSV    dlm_dlmfsv_impute_batch: comp = t; attempt j < 8 the normal of factor j, attempt 8 + i the normal of component i
constexpr unsigned DLM_KEY_GIBBS = 0x47494242u;      // "GIBB"
constexpr unsigned DLM_KEY_STUDENTT = 0x53545544u;   // "STUD"
constexpr unsigned DLM_KEY_SV = 0x5354564Fu;         // "STVO"
constexpr unsigned DLM_KEY_SVOU = 0x53564F55u;       // "SVOU"
constexpr unsigned DLM_KEY_FSV = 0x46535620u;        // "FSV "
constexpr unsigned DLM_KEY_DLMFSV = 0x444C4653u;     // "DLFS"
//   DLM_KEY_SVKNOT    dlm_sv_knots_batch: comp = s for state s <= T: which 0 the normal of the state's proposal, which 1 the acceptance
//                     uniform of the block whose first state is s
constexpr unsigned DLM_KEY_SVKNOT = 0x53564B4Eu;     // "SVKN"
//   DLM_KEY_PF        dlm_pf_batch: comp = t for the step into observation t, DLM_PF_SLOT_INIT for the initial cloud; attempt = the particle
//                     (i < 1024: the attempt field's ten bits), which = 0.  The low byte of the key is the BLOCK of that (slot, particle):
//                     block q < 8 gives the Box-Muller pair (cosine, sine) = the normals of the state components (2 q, 2 q + 1), block
//                     DLM_PF_BLOCK_RESAMPLE the [0, 1) uniform u_i of the resampling search of step t (pf_rand, dlm_pf.hip)
constexpr unsigned DLM_KEY_PF = 0x50462000u;         // "PF " and the block in the low byte
constexpr unsigned DLM_PF_BLOCK_RESAMPLE = 8u;
//                     dlm_pf_forecast_particles draws under DLM_KEY_PF too (slot slot_offset + h for step h, the blocks above for the state normals and the
//                     resampling of an observed step), and its own blocks beside them: DLM_PF_BLOCK_RESAMPLE0 the uniform of the resampling of a
//                     WEIGHTED entry cloud (slot slot_offset); DLM_PF_BLOCK_OBS the observation's first draw (u1, u2): the Box-Muller cosine of the
//                     Gaussian and Student-t families, u1 the zero-inflation uniform, u2 the inversion uniform of a small Poisson rate;
//                     DLM_PF_BLOCK_POISSON + j attempt j < DLM_PF_POISSON_ATTEMPTS of the transformed rejection of a large rate; DLM_PF_BLOCK_GAMMA_A
//                     + j and DLM_PF_BLOCK_GAMMA_B + j attempt j < DLM_PF_GAMMA_ATTEMPTS of the first and the second Gamma of a draw (`which` 0 its
//                     normal, 1 its accept uniform), j = DLM_PF_GAMMA_ATTEMPTS the boost of a shape below 1.  The attempts are BLOCKS because the
//                     counter's attempt field holds the particle (dlm_obs_draws.h)
constexpr unsigned DLM_PF_BLOCK_RESAMPLE0 = 9u, DLM_PF_BLOCK_OBS = 10u;
constexpr unsigned DLM_PF_POISSON_ATTEMPTS = 32u, DLM_PF_GAMMA_ATTEMPTS = 32u;
constexpr unsigned DLM_PF_BLOCK_POISSON = 11u;
constexpr unsigned DLM_PF_BLOCK_GAMMA_A = DLM_PF_BLOCK_POISSON + DLM_PF_POISSON_ATTEMPTS;       // 43 .. 75
constexpr unsigned DLM_PF_BLOCK_GAMMA_B = DLM_PF_BLOCK_GAMMA_A + DLM_PF_GAMMA_ATTEMPTS + 1u;     // 76 .. 108
//                     dlm_pf_resampled with DLM_RESAMPLE_METROPOLIS draws under DLM_KEY_PF too: block DLM_PF_BLOCK_MH0 + s of (slot t, particle i)
//                     gives step s < mh_steps <= DLM_PF_MAX_MH_STEPS of particle i's chain in the resampling of step t, u1 its acceptance uniform
//                     and u2 its proposal.  The stratified scheme reads the u2 of DLM_PF_BLOCK_RESAMPLE of every particle as the multinomial one
//                     does, the systematic scheme particle 0's alone
constexpr unsigned DLM_PF_BLOCK_MH0 = 128u;
constexpr int DLM_PF_MAX_MH_STEPS = 64;                                                         // 128 .. 191
//   DLM_KEY_STORVIK   dlm_storvik_batch: comp and attempt field as DLM_KEY_PF (slot t or DLM_STORVIK_SLOT_INIT, the particle).  The low byte of the
//                     key is the BLOCK: q < 8 the Box-Muller pair of the state components (2 q, 2 q + 1), DLM_STORVIK_BLOCK_RESAMPLE the resampling
//                     uniform, DLM_STORVIK_BLOCK_GAMMA + k the Gamma of component k (k < d: the variance W_kk; k = d: V).  The second byte is the
//                     ATTEMPT of that Gamma's rejection loop (the counter word has no room for it beside the particle): attempt j <
//                     DLM_STORVIK_GAMMA_ATTEMPTS, `which` 0 its normal and 1 its accept uniform; DLM_STORVIK_GAMMA_ATTEMPTS itself the boost of a shape
//                     below 1.  The second byte is 0 for every other block.
constexpr unsigned DLM_KEY_STORVIK = 0x53740000u;    // "St", then the attempt byte and the block byte
constexpr unsigned DLM_STORVIK_BLOCK_RESAMPLE = 8u, DLM_STORVIK_BLOCK_GAMMA = 9u, DLM_STORVIK_GAMMA_ATTEMPTS = 255u;
//   DLM_KEY_LW        dlm_lw_batch: comp and attempt field as DLM_KEY_PF (slot t or DLM_LW_SLOT_INIT, the particle).  The low byte of the key is the
//                     BLOCK: q < 8 the Box-Muller pair of the state components (2 q, 2 q + 1), DLM_LW_BLOCK_RESAMPLE the uniform of the second
//                     stage's resampling, DLM_LW_BLOCK_FIRST the uniform of the first (auxiliary) stage's, DLM_LW_BLOCK_PARAM + q the Box-Muller
//                     pair of the log-variances (2 q, 2 q + 1) (k < d: log W_kk; k = d: log V).  The second byte is 0.
constexpr unsigned DLM_KEY_LW = 0x4C570000u;         // "LW", a zero byte and the block byte
constexpr unsigned DLM_LW_BLOCK_RESAMPLE = 8u, DLM_LW_BLOCK_FIRST = 9u, DLM_LW_BLOCK_PARAM = 10u;
//   DLM_KEY_RB        dlm_rb_batch: comp and attempt field as DLM_KEY_PF (slot t or DLM_RB_SLOT_INIT, the particle).  The state is integrated out, so
//                     there are no state normals.  The low byte of the key is the BLOCK: DLM_RB_BLOCK_RESAMPLE the uniform of the second stage's
//                     resampling, DLM_RB_BLOCK_FIRST the uniform of the first (auxiliary) stage's, DLM_RB_BLOCK_PARAM + q the Box-Muller pair of
//                     the log-variances (2 q, 2 q + 1) (k < d: log W_kk; k = d: log V).  The second byte is 0.
constexpr unsigned DLM_KEY_RB = 0x52420000u;         // "RB", a zero byte and the block byte
constexpr unsigned DLM_RB_BLOCK_RESAMPLE = 0u, DLM_RB_BLOCK_FIRST = 1u, DLM_RB_BLOCK_PARAM = 2u;
//                     dlm_rb_state_draw draws under DLM_KEY_RB too, at the slot its caller names: DLM_RB_BLOCK_STATE + q, q < 8, the Box-Muller pair
//                     of the components (2 q, 2 q + 1) of z in x_i = m_i + chol(C_i) z (blocks no step of dlm_rb_batch uses)
constexpr unsigned DLM_RB_BLOCK_STATE = 16u;
//   DLM_KEY_FCL       dlm_pf_forecast_learned, DLM_FC_IG_SCALE only (its state normals, entry resampling and observation draws are DLM_KEY_PF's, above):
//                     comp = slot_offset, the attempt field the particle.  The low byte of the key is the BLOCK: DLM_FCL_BLOCK_GAMMA + k the Gamma of the
//                     variance of component k (k < d: W_kk; k = d: V), drawn ONCE per particle after the entry resampling.  The second byte is the ATTEMPT
//                     of that Gamma's rejection loop, as under DLM_KEY_STORVIK: attempt j < DLM_FCL_GAMMA_ATTEMPTS, `which` 0 its normal and 1 its accept
//                     uniform; DLM_FCL_GAMMA_ATTEMPTS itself the boost of a shape below 1.
constexpr unsigned DLM_KEY_FCL = 0x464C0000u;        // "FL", then the attempt byte and the block byte
constexpr unsigned DLM_FCL_BLOCK_GAMMA = 0u, DLM_FCL_GAMMA_ATTEMPTS = 255u;
//   DLM_KEY_PG        dlm_pg_batch: comp and attempt field as DLM_KEY_PF (slot t for the step into observation t or DLM_PG_SLOT_INIT, the particle).
//                     The low byte of the key is the BLOCK: q < 8 the Box-Muller pair of the state components (2 q, 2 q + 1) of a free particle,
//                     DLM_PG_BLOCK_RESAMPLE the [0, 1) uniform of a free particle's ancestor search in step t, DLM_PG_BLOCK_REF the uniform of the
//                     REFERENCE particle's ancestor (slot t, particle P - 1: ancestor sampling), DLM_PG_BLOCK_FINAL the uniform of the final index
//                     k_T (slot DLM_PG_SLOT_INIT, particle 0).  The second byte is 0.
constexpr unsigned DLM_KEY_PG = 0x50470000u;         // "PG", a zero byte and the block byte
constexpr unsigned DLM_PG_BLOCK_RESAMPLE = 8u, DLM_PG_BLOCK_REF = 9u, DLM_PG_BLOCK_FINAL = 10u;
//   DLM_KEY_SVPATH    dlm_sv_paths: comp = the step h of the path (1 .. H; DLM_SVPATH_SLOT_START = 0 the draw of a stationary start), the attempt
//                     field the path r < 1024, which = 0.  The low byte of the key is the FACTOR j < 8.  The second byte is 0.
constexpr unsigned DLM_KEY_SVPATH = 0x53500000u;     // "SP", a zero byte and the factor byte
constexpr unsigned DLM_SVPATH_SLOT_START = 0u;
constexpr int DLM_SVPATH_MAX_H = 0x1FFFFF;           // step h takes slot h <= H
constexpr int DLM_SVPATH_MAX_R = 1024;

// ---- the slots ------------------------------------------------------------------------------------------------------------------
// comp is a 21-bit field (the counter word is comp * 2048 + attempt * 2 + which).  A sampler whose per-time draws take comp = t < T
// gives its scalar draws the slots from DLM_SLOT_TOP downward, and T stays below the lowest of them: DLM_*_MAX_T is the largest T the
// entry points admit (dlm_engine.hip).
constexpr unsigned DLM_SLOT_TOP = 0x1FFFFFu;
enum : unsigned {   // dlm_studentt_step_batch, DLM_KEY_STUDENTT
  DLM_ST_SLOT_PROP_GAMMA = DLM_SLOT_TOP,        // lambda ~ Gamma(r, nu / r) of the proposal
  DLM_ST_SLOT_POISSON = DLM_SLOT_TOP - 1,       // Poisson(lambda)
  DLM_ST_SLOT_ACCEPT = DLM_SLOT_TOP - 2,        // the Metropolis-Hastings uniform
  DLM_ST_SLOT_SCALE = DLM_SLOT_TOP - 3,         // s ~ Gamma
};
enum : unsigned {   // dlm_sv_params_batch, DLM_KEY_SV (dlm_sv_mixture_batch takes the slots t)
  DLM_SV_SLOT_PHI = DLM_SLOT_TOP,               // phi ~ N (conjugate mode; attempt k of the rejection)
  DLM_SV_SLOT_MU = DLM_SLOT_TOP - 1,            // mu ~ N
  DLM_SV_SLOT_SIGMA = DLM_SLOT_TOP - 2,         // sigma^2: the Gamma of the InverseGamma
  DLM_SV_SLOT_PROP_A = DLM_SLOT_TOP - 3,        // Beta proposal: Gamma(lambda phi + tau)
  DLM_SV_SLOT_PROP_B = DLM_SLOT_TOP - 4,        //                Gamma(lambda (1 - phi) + tau)
  DLM_SV_SLOT_ACCEPT = DLM_SLOT_TOP - 5,        // the Metropolis-Hastings uniform
};
enum : unsigned {   // dlm_sv_ou_params_batch, DLM_KEY_SVOU (no per-time draws of its own: the limit is the mixture call's)
  DLM_SVOU_SLOT_PROP_A = DLM_SLOT_TOP,          // Beta proposal: Gamma(lambda phi + tau)
  DLM_SVOU_SLOT_PROP_B = DLM_SLOT_TOP - 1,      //                Gamma(lambda (1 - phi) + tau)
  DLM_SVOU_SLOT_ACC_PHI = DLM_SLOT_TOP - 2,     // phi's uniform
  DLM_SVOU_SLOT_Z_SIGMA = DLM_SLOT_TOP - 3,     // sigma's walk
  DLM_SVOU_SLOT_ACC_SIGMA = DLM_SLOT_TOP - 4,   // sigma's uniform
  DLM_SVOU_SLOT_Z_MU = DLM_SLOT_TOP - 5,        // mu's walk
  DLM_SVOU_SLOT_ACC_MU = DLM_SLOT_TOP - 6,      // mu's uniform
};
enum : unsigned {   // dlm_fsv_loadings_batch, DLM_KEY_FSV (dlm_fsv_factors_batch takes the slots t)
  DLM_FSV_SLOT_SIGMA = DLM_SLOT_TOP,            // sigma^2: the Gamma of the InverseGamma
  DLM_FSV_SLOT_ROW0 = DLM_SLOT_TOP - 1,         // row i of beta takes the slot DLM_FSV_SLOT_ROW0 - i, attempt j the normal of its entry j
  DLM_FSV_SLOT_ROW_LAST = DLM_SLOT_TOP - 64,    // i <= 63 (p <= 64)
};
enum : unsigned {   // dlm_pf_batch, DLM_KEY_PF (the steps take the slots t)
  DLM_PF_SLOT_INIT = DLM_SLOT_TOP,              // the initial cloud x_0,i = m0 + chol(C0) z
};
constexpr int DLM_ST_MAX_T = 0x1FFFFC;     // v_t takes slot t < T
constexpr int DLM_SV_MAX_T = 0x1FFFF7;     // k_t takes slot t < T; 0x1FFFF8 and 0x1FFFF9 are kept free
constexpr int DLM_SVOU_MAX_T = 0x1FFFF7;   // the chain's mixture call runs at the same T
constexpr int DLM_SVKNOT_MAX_T = 0x1FFFF6; // state s takes slot s <= T: T + 1 stays below 2^21 - 8, as the chain's parameter call asks of T
constexpr int DLM_FSV_MAX_T = 0x1FFFBF;    // the factors' normals take slot t < T
constexpr int DLM_PF_MAX_T = 0x1FFFFE;     // the step into observation t takes slot t < T
constexpr int DLM_PF_MAX_D = 16, DLM_PF_MAX_P = 1024;
static_assert(DLM_PF_SLOT_INIT > (unsigned)DLM_PF_MAX_T - 1, "the particle filter's initial cloud lies above every time slot");
static_assert(DLM_PF_MAX_P <= 1024 && (DLM_PF_MAX_D + 1) / 2 <= (int)DLM_PF_BLOCK_RESAMPLE && DLM_PF_BLOCK_RESAMPLE < 256u,
              "a particle fits the attempt field and a block the key's low byte");
static_assert(DLM_PF_BLOCK_RESAMPLE0 > DLM_PF_BLOCK_RESAMPLE && DLM_PF_BLOCK_OBS > DLM_PF_BLOCK_RESAMPLE0 && DLM_PF_BLOCK_POISSON > DLM_PF_BLOCK_OBS &&
              DLM_PF_BLOCK_GAMMA_A >= DLM_PF_BLOCK_POISSON + DLM_PF_POISSON_ATTEMPTS && DLM_PF_BLOCK_GAMMA_B > DLM_PF_BLOCK_GAMMA_A + DLM_PF_GAMMA_ATTEMPTS &&
              DLM_PF_BLOCK_GAMMA_B + DLM_PF_GAMMA_ATTEMPTS < 256u,
              "the forecast's blocks (entry resampling, the observation's first draw, the Poisson attempts, two Gammas' attempts and boosts) are distinct from the filter's and from one another and fit the key's low byte");
static_assert(DLM_PF_BLOCK_MH0 > DLM_PF_BLOCK_GAMMA_B + DLM_PF_GAMMA_ATTEMPTS && DLM_PF_BLOCK_MH0 + (unsigned)DLM_PF_MAX_MH_STEPS <= 256u,
              "the Metropolis resampling's blocks lie above every block of the filter and of the forecast and fit the key's low byte");
constexpr unsigned DLM_STORVIK_SLOT_INIT = DLM_SLOT_TOP;   // dlm_storvik_batch, DLM_KEY_STORVIK: the initial cloud (the steps take the slots t < T <= DLM_PF_MAX_T)
static_assert(DLM_STORVIK_BLOCK_GAMMA > DLM_STORVIK_BLOCK_RESAMPLE && (DLM_PF_MAX_D + 1) / 2 <= (int)DLM_STORVIK_BLOCK_RESAMPLE &&
              DLM_STORVIK_BLOCK_GAMMA + (unsigned)DLM_PF_MAX_D < 256u && DLM_STORVIK_GAMMA_ATTEMPTS < 256u,
              "the Storvik filter's blocks (the Gammas of d + 1 components included) and a Gamma's attempts fit a byte of the key each");
constexpr unsigned DLM_LW_SLOT_INIT = DLM_SLOT_TOP;   // dlm_lw_batch, DLM_KEY_LW: the initial cloud (the steps take the slots t < T <= DLM_PF_MAX_T)
static_assert(DLM_LW_SLOT_INIT > (unsigned)DLM_PF_MAX_T - 1, "the Liu-West filter's initial cloud lies above every time slot");
static_assert((DLM_PF_MAX_D + 1) / 2 <= (int)DLM_LW_BLOCK_RESAMPLE && DLM_LW_BLOCK_FIRST > DLM_LW_BLOCK_RESAMPLE && DLM_LW_BLOCK_PARAM > DLM_LW_BLOCK_FIRST &&
              DLM_LW_BLOCK_PARAM + (unsigned)(DLM_PF_MAX_D + 2) / 2 <= 256u,
              "the Liu-West filter's blocks (the pairs of d + 1 log-variances included) are distinct and fit the key's low byte");
constexpr unsigned DLM_RB_SLOT_INIT = DLM_SLOT_TOP;   // dlm_rb_batch, DLM_KEY_RB: the initial log-variances (the steps take the slots t < T <= DLM_PF_MAX_T)
static_assert(DLM_RB_SLOT_INIT > (unsigned)DLM_PF_MAX_T - 1, "the Rao-Blackwellised filter's initial log-variances lie above every time slot");
static_assert(DLM_RB_BLOCK_FIRST > DLM_RB_BLOCK_RESAMPLE && DLM_RB_BLOCK_PARAM > DLM_RB_BLOCK_FIRST &&
              DLM_RB_BLOCK_PARAM + (unsigned)(DLM_PF_MAX_D + 2) / 2 <= 256u,
              "the Rao-Blackwellised filter's blocks (the pairs of d + 1 log-variances included) are distinct and fit the key's low byte");
static_assert(DLM_RB_BLOCK_STATE >= DLM_RB_BLOCK_PARAM + (unsigned)(DLM_PF_MAX_D + 2) / 2 && DLM_RB_BLOCK_STATE + (unsigned)(DLM_PF_MAX_D + 1) / 2 <= 256u,
              "the state draw's blocks lie above the Rao-Blackwellised filter's own and fit the key's low byte");
static_assert(DLM_FCL_BLOCK_GAMMA + (unsigned)DLM_PF_MAX_D < 256u && DLM_FCL_GAMMA_ATTEMPTS < 256u && (DLM_KEY_FCL & 0xFFFFu) == 0u &&
              DLM_KEY_FCL != DLM_KEY_STORVIK && DLM_KEY_FCL != DLM_KEY_LW && DLM_KEY_FCL != DLM_KEY_RB && DLM_KEY_FCL != DLM_KEY_PG &&
              (DLM_KEY_FCL >> 16) != (DLM_KEY_PF >> 16),
              "the learned forecast's Gammas (d + 1 components) and their attempts fit a byte of the key each, under a key of their own");
constexpr unsigned DLM_PG_SLOT_INIT = DLM_SLOT_TOP;   // dlm_pg_batch, DLM_KEY_PG: the initial cloud and the final index (the steps take the slots t < T <= DLM_PF_MAX_T)
static_assert(DLM_PG_SLOT_INIT > (unsigned)DLM_PF_MAX_T - 1, "the conditional filter's initial cloud and final index lie above every time slot");
static_assert((DLM_PF_MAX_D + 1) / 2 <= (int)DLM_PG_BLOCK_RESAMPLE && DLM_PG_BLOCK_REF > DLM_PG_BLOCK_RESAMPLE && DLM_PG_BLOCK_FINAL > DLM_PG_BLOCK_REF &&
              DLM_PG_BLOCK_FINAL < 256u,
              "the conditional filter's blocks (state normals, free ancestors, the reference's ancestor, the final index) are distinct and fit the key's low byte");
static_assert((DLM_KEY_SVPATH & 0xFFFFu) == 0u && (DLM_KEY_SVPATH >> 16) != (DLM_KEY_PF >> 16) && DLM_KEY_SVPATH != DLM_KEY_STORVIK &&
              DLM_KEY_SVPATH != DLM_KEY_LW && DLM_KEY_SVPATH != DLM_KEY_RB && DLM_KEY_SVPATH != DLM_KEY_FCL && DLM_KEY_SVPATH != DLM_KEY_PG &&
              DLM_SVPATH_MAX_R <= 1024 && (unsigned)DLM_SVPATH_MAX_H <= DLM_SLOT_TOP,
              "the volatility paths draw under a key of their own; a path fits the attempt field, a factor the key's low byte, a step the slot field");
static_assert(DLM_ST_SLOT_SCALE > (unsigned)DLM_ST_MAX_T - 1, "the Student-t step's scalar slots lie above every time slot");
static_assert(DLM_SV_SLOT_ACCEPT > (unsigned)DLM_SV_MAX_T, "the SV step's scalar slots lie above every time slot");
static_assert(DLM_SVOU_SLOT_ACC_MU > (unsigned)DLM_SVOU_MAX_T, "the OU step's scalar slots lie above every time slot");
static_assert(DLM_FSV_SLOT_ROW_LAST > (unsigned)DLM_FSV_MAX_T - 1, "the loadings' slots lie above every time slot");
static_assert(DLM_FSV_MAX_T <= DLM_SV_MAX_T, "the factor chains' mixture call runs at the same T");

// ---- uniforms, normals, Gammas ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void gibbs_rand(unsigned long long seed, unsigned long long series, unsigned long long iteration,
                                           unsigned comp, unsigned attempt, unsigned which, double& u1, double& u2,
                                           unsigned key = DLM_KEY_GIBBS) {
  unsigned c[4] = {(unsigned)series, (unsigned)(series >> 32), (unsigned)iteration, comp * 2048u + attempt * 2u + which};
  philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32) ^ key);
  u1 = ((double)c[0] * 4294967296.0 + (double)c[1] + 1.0) * (1.0 / 18446744073709551616.0);   // (0, 1]
  u2 = ((double)c[2] * 4294967296.0 + (double)c[3]) * (1.0 / 18446744073709551616.0);         // [0, 1)
}

// N(0, 1) of attempt `attempt` of a scalar slot: the Box-Muller cosine of the block's pair
__device__ __forceinline__ double draw_normal(unsigned key, unsigned long long seed, unsigned long long series, unsigned long long it,
                                              unsigned slot, unsigned attempt = 0u) {
  double u1, u2;
  gibbs_rand(seed, series, it, slot, attempt, 0u, u1, u2, key);
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925286766559 * u2);
}
// log u, u the (0, 1] uniform of a scalar slot: what a Metropolis-Hastings move compares its log acceptance ratio with
__device__ __forceinline__ double draw_log_uniform(unsigned key, unsigned long long seed, unsigned long long series, unsigned long long it,
                                                   unsigned slot) {
  double u1, u2;
  gibbs_rand(seed, series, it, slot, 0u, 0u, u1, u2, key);
  return log(u1);
}

// Gamma(a, 1): Marsaglia & Tsang, "A simple method for generating gamma variables" (2000); a < 1 by the u^(1/a) boost.  Written ONCE:
// src(attempt, which, u1, u2) hands out the uniforms of attempt < n_attempts (which 0: the normal's pair, 1: the accept uniform) and of
// attempt n_attempts, the boost.
template <class Source>
__device__ __forceinline__ double gamma_unit_from(double a, unsigned n_attempts, Source&& src) {
  double boost = 1.0;
  if (a < 1.0) {
    double u1, u2;
    src(n_attempts, 0u, u1, u2);
    boost = pow(u1, 1.0 / a);
    a += 1.0;
  }
  const double dd = a - 1.0 / 3.0, cc = 1.0 / sqrt(9.0 * dd);
  for (unsigned k = 0; k < n_attempts; ++k) {
    double u1, u2, w1, w2;
    src(k, 0u, u1, u2);
    const double x = sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925286766559 * u2);
    double v = 1.0 + cc * x;
    if (v <= 0.0) continue;
    v = v * v * v;
    src(k, 1u, w1, w2);
    if (log(w1) < 0.5 * x * x + dd - dd * v + dd * log(v)) return dd * v * boost;
  }
  return dd * boost;   // unreachable in practice (acceptance > 95 % per attempt)
}
// the Gamma of a scalar slot: attempt k of the counter word, the boost at attempt 1023
__device__ inline double gamma_unit(double a, unsigned long long seed, unsigned long long series, unsigned long long iteration, unsigned comp,
                                    unsigned key = DLM_KEY_GIBBS) {
  return gamma_unit_from(a, 1023u, [&](unsigned attempt, unsigned which, double& u1, double& u2) {
    gibbs_rand(seed, series, iteration, comp, attempt, which, u1, u2, key);
  });
}

// ---- the Beta proposal of phi (samplePhi, StochasticVolatility.scala:189-202; samplePhiOu of stepOu) ------------------------------
// phi' ~ Beta(lambda phi + tau, lambda (1 - phi) + tau) as ga / (ga + gb).  Both functions are called by the WHOLE wave: the two Gammas
// are drawn on lanes 0 and 1, the six lgamma values of the Hastings ratio are made side by side on lanes 0..5, and the shuffles leave
// every lane with every member.  lq_fwd / lq_back are returned apart: the callers add them to their target in their own order.
struct BetaProposal {
  double phi0, phip;       // the current value and the proposal
  double A0, B0, A1, B1;   // the proposal's parameters at phi0 and at phip
  double G[6];             // lgamma of A0, B0, A0 + B0, A1, B1, A1 + B1
  bool ok;                 // phip lies inside (0, 1) (one that rounds to 0 or 1 is rejected)

  // `bad`: the series' input is unusable -- nothing is drawn, and the caller uses no member
  __device__ __forceinline__ void draw(int lane, double phi, double lam, double tau, bool bad, unsigned key, unsigned long long seed,
                                       unsigned long long series, unsigned long long it, unsigned slot_a, unsigned slot_b) {
    phi0 = phi;
    A0 = lam * phi0 + tau; B0 = lam * (1.0 - phi0) + tau;
    double g = 1.0;
    if (lane < 2 && !bad) g = gamma_unit(lane == 0 ? A0 : B0, seed, series, it, lane == 0 ? slot_a : slot_b, key);
    const double ga = __shfl(g, 0, 64), gb = __shfl(g, 1, 64);
    phip = ga / (ga + gb);
    ok = phip > 0.0 && phip < 1.0;
    A1 = lam * phip + tau; B1 = lam * (1.0 - phip) + tau;
  }
  __device__ __forceinline__ void lgammas(int lane) {
    double garg = 1.0;
    switch (lane) {
      case 0: garg = A0; break;  case 1: garg = B0; break;  case 2: garg = A0 + B0; break;
      case 3: garg = A1; break;  case 4: garg = B1; break;  case 5: garg = A1 + B1; break;
      default: break;
    }
    const double lg = lgamma(garg);
#pragma unroll
    for (int j = 0; j < 6; ++j) G[j] = __shfl(lg, j, 64);
  }
  __device__ __forceinline__ double lq_fwd() const {    // log q(phi' | phi)
    return G[2] - G[0] - G[1] + (A0 - 1.0) * log(phip) + (B0 - 1.0) * log(1.0 - phip);
  }
  __device__ __forceinline__ double lq_back() const {   // log q(phi | phi')
    return G[5] - G[3] - G[4] + (A1 - 1.0) * log(phi0) + (B1 - 1.0) * log(1.0 - phi0);
  }
};

// ---- the conjugate InverseGamma draw of a diagonal variance (GibbsSampling.sampleSystemMatrix, Gibbs.scala:56-78) ----------------------
// InverseGamma(shape, rate).draw = rate / Gamma(shape, 1).draw on DLM_KEY_GIBBS component comp.  The kernel draws the Gamma at its ONE
// call of gamma_unit (k_dinvgamma_step draws V there too, k_studentt_step its proposal: the lanes of a second call site would run behind
// the first's); the rest is here, so that dlm_studentt_step_batch's W_out is dlm_dinvgamma_step_batch's by construction.
struct InvGammaDraw { double shape, rate; unsigned comp; };
// W_ii of a series with the FFBS statistics st = [ssy (p) | n (p) | ss (d) | T]:  InverseGamma(aw + T / 2, bw + ss_i / 2) (the shape uses
// T), component p + i
__device__ __forceinline__ InvGammaDraw w_draw(const double* st, int d, int p, int i, double aw, double bw) {
  const int L = 2 * p + d + 1;
  return InvGammaDraw{aw + 0.5 * st[L - 1], bw + 0.5 * st[2 * p + i], (unsigned)(p + i)};
}
// column i of the dense diagonal n x n matrix M: the draw q, whose Gamma(q.shape, 1) variate is g, on the diagonal
__device__ __forceinline__ void store_diag_draw(double* M, int n, int i, const InvGammaDraw& q, double g) {
  const double val = q.rate / g;
  double* col = M + (size_t)i * n;
  for (int k = 0; k < n; ++k) col[k] = (k == i) ? val : 0.0;
}

}  // namespace dlm
