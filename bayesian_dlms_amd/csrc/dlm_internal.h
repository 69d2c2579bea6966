// Internal declarations shared by the engine's translation units (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/dlm_engine.h"

namespace dlm {

// Device-pointer view of one batched call.  All pointers are device pointers.
struct KArgs {
  int d, p, T, N;
  const double* F; long long f_stride;
  const double* G; int n_g; const int* g_index; const double* dt;
  const double* V; long long v_stride;
  const double* W; long long w_stride;
  long long v_tstride, w_tstride;   // per-time strides of V_t / W_t (0 = time-invariant)
  const double* m0; long long m0_stride;
  const double* C0; long long c0_stride;
  const double* y;     // [N][T][p]
  const double* z;     // [N][T+1][d] injected normals or nullptr
  const double* filt_in;  // [N][T+1][d+dd] (smoother / sampler input)
  double* filt;        // outputs (nullable where optional)
  double* prior;
  double* fq;
  double* smooth;
  double* theta;
  double* cond;
  double* stats;
  double* loglik;      // [N] prediction-error log-likelihood (nullable); with it, filt may be null (nothing stored)
  int* status;
  int packed;          // structured d <= 15 fast path only.  bit 0: filt / filt_in hold PACKED records (engine-internal workspace,
                       // or DLM_OPT_PACKED_SYM); bit 1: the smoothed records are written packed too (DLM_OPT_PACKED_SYM)
  const struct SparseBig* spb;   // tiled path: [2 n_g] row / column tables of a structured G, or nullptr (dense G)
  int spb_k;           // largest nonzero count per row / column over those tables (1..4)
  const struct SparseF* spf;     // structured (time-invariant) F of the tiled path: column / row tables, or nullptr
  int spf_k;           // largest nonzero count per column / row of F (1..4)
  unsigned flags;
  unsigned long long seed, series_offset;
  // Shared-covariance path (dlm_sparse16.hip): route[n] != 0 marks a series with a missing observation.  The
  // mean-only kernels set it and skip such a series; the per-series kernels launched behind them with route_take = 1 serve
  // exactly those series (and leave at once for the others).  nullptr: every series is served (the ordinary calls).
  unsigned char* route;
  int route_take;
  unsigned long long* counters;   // engine-owned [4], zeroed per call (nullable): steady (short) steps taken by the forward [0] / backward [1] kernel,
                                  // series served by the shared-covariance kernels [2], series sent to their own full recursion [3]
  const unsigned char* plain;     // structured d <= 15 path, regular grid (nullable): plain[n] = 1 -- series n misses enough observations (more than T / 256)
                                  // that its covariance recursion is not worth testing for convergence: it takes every step in full, in the
                                  // backward kernel's instantiation without the shortcut's machinery (k_count_gaps fills it from the data alone)
  const unsigned char* keep_cov;  // per-wave filter, 16 <= d <= 48 (nullable): a dlm_ffbs_batch call that keeps no records and draws against shared factors
                                  // reads only the MEANS of the series without a gap -- once such a series' covariance has settled its steady steps
                                  // store the mean alone (keep_cov[n] = 0); the series with a gap (1) write whole records for their own sampler
  double* ktab;                   // per-wave filter, with keep_cov: the steady gain K^T (16 PT rows of the LDS image) of the batch -- WRITTEN by the series
                                  // of zeros where its covariance recursion settles (with settle_step), and, when set for the batch's own filter, the
                                  // sign that its series without a gap leave at that step: k_steady_filter_w48 carries their means on from there
  int* leave_step;                // per-wave filter, with ktab set for the batch's own filter: [N] the step at which series n left k_filter_w48 (its own
                                  // convergence test; T: it never did) -- k_steady_filter_w48 carries series n on from THAT record, so that no assumption
                                  // about every series settling at the zero series' step is needed
  int stretches;                  // backward sampler: 1 = every stretch of steps starts from scratch (dlm_sampler16.hip: SF_STRETCH), set for the calls
                                  // whose parameters allow a shared-factor table -- its stretches are made side by side, and a series that computes
                                  // its own factors in such a call follows the same rule, so that the two agree bit for bit
  int* settle_step;               // the filter of the shared-factor tables' series of zeros (nullptr otherwise): the kernel stops when its covariance
                                  // recursion has settled and leaves here the last record it wrote -- every later record would repeat that covariance
};

// The arguments of a TABLE RUN: one wave that runs a per-series kernel on a series of zeros (the shared-covariance, shared-factor and
// shared RTS routes, the SVD filter's shared factors).  table_run_args is where every one of them starts: N = 1, what describes the model
// and the parameters the batch shares, and NOTHING that belongs to the call's own series -- every pointer null, every count 0.  The site
// then assigns what its run reads or writes (its zeros, its record buffers, status, ...).  Every field of KArgs stands in one of the two
// lists, so that a new field cannot be added without deciding which it is (tests/test_launch_layer_host.py holds the lists against the
// struct and against the function; site by field: profiles/r09_notes.md):
//   TABLE-RUN carried:  d p T F f_stride G n_g g_index dt V v_stride W w_stride v_tstride w_tstride C0 c0_stride spb spb_k spf spf_k flags stretches
//   TABLE-RUN per call: N m0 m0_stride y z filt_in filt prior fq smooth theta cond stats loglik status packed seed series_offset route route_take counters plain keep_cov ktab leave_step settle_step
inline KArgs table_run_args(const KArgs& a) {
  KArgs k{};
  k.N = 1;
  k.d = a.d; k.p = a.p; k.T = a.T;
  k.F = a.F; k.f_stride = a.f_stride; k.G = a.G; k.n_g = a.n_g; k.g_index = a.g_index; k.dt = a.dt;
  k.V = a.V; k.v_stride = a.v_stride; k.W = a.W; k.w_stride = a.w_stride; k.v_tstride = a.v_tstride; k.w_tstride = a.w_tstride;
  k.C0 = a.C0; k.c0_stride = a.c0_stride;
  k.spb = a.spb; k.spb_k = a.spb_k; k.spf = a.spf; k.spf_k = a.spf_k;
  k.flags = a.flags; k.stretches = a.stretches;
  return k;
}

// Packed record of the structured fast path's internal workspaces: [m (d) | lower triangle of C by rows], padded to a
// multiple of 16 B (the backward pass fetches records by 16-byte LDS-DMA pieces).
__host__ __device__ inline int packed_rec_bytes(int d) { return ((d + d * (d + 1) / 2) * 8 + 15) & ~15; }

__host__ __device__ inline int stats_len(int d, int p, unsigned flags) {
  return 2 * p + ((flags & (1u << 4)) ? d * d : d) + 1;  // DLM_OPT_STATS_OUTER
}

// The one hand-counted vector-memory wait of the LDS-DMA prefetches (dlm_sparse16.hip, dlm_sampler16.hip, dlm_svd.hip): at most
// N vector-memory operations of this wave still in flight.  N counts the loads, stores and LDS DMAs the wave issued after the
// one waited for (the DMA itself: lds_dma<NR>, dlm_wave.h).  -DDLM_DRAIN_WAITS=1 turns every such wait into vmcnt(0) and changes nothing else
// (build.build_drain_variant): tests/test_counted_waits_gpu.py compares the two builds bit for bit.  Every counted wait
// goes through here (tests/test_counted_waits_host.py checks the sources and the code objects).
#ifndef DLM_DRAIN_WAITS
#define DLM_DRAIN_WAITS 0
#endif
template <int N>
__device__ __forceinline__ void vm_wait() {
  static_assert(N >= 0 && N <= 63, "vmcnt holds 0..63");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DLM_DRAIN_WAITS ? 0 : N) : "memory");
}

// ---- launchers: from run-time values to template arguments (host only) -------------------------------------------------
// A kernel's template arguments are chosen by selection rules: pick / pick_bool hand the rule's value to a generic lambda as a
// type (std::integral_constant: V() or decltype(V)::value is a constant expression there), and only the listed values are
// instantiated.  Each rule is ONE function (with_* / pick in the kernel files); a table run that must use the per-series
// launch's very instantiation goes through the same function (below the table of variants).
template <int... Vs, class F>
inline hipError_t pick(int v, F&& f) {   // f(integral_constant<int, V>) for the listed V equal to v; no such V: hipErrorInvalidValue
  // (a LEFT fold: the compiler instantiates f for the listed values in their order, and the kernels stand in the code object in that order)
  hipError_t err = hipErrorInvalidValue;
  (void)(... || (v == Vs && ((err = f(std::integral_constant<int, Vs>{})), true)));
  return err;
}
template <class F>
inline hipError_t pick_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
// Dynamic LDS above the 64 KB a kernel gets without asking is asked for in ONE place (dlm_engine.hip; DESIGN.md 4, below the table of
// variants): lds_opt_in grants `bytes` to `fn` on the CURRENT device -- HIP keeps the attribute per device, and a process may hold engines
// on several -- once per (function, device) and amount; more than the device has: hipErrorInvalidValue.  launch calls it, nobody else.
hipError_t lds_opt_in(const void* fn, size_t bytes);
size_t lds_limit();   // LDS of one workgroup on the current device (hipDeviceAttributeMaxSharedMemoryPerBlock); 0: the runtime does not say
// Dynamic LDS that, with the kernel's static LDS, fills a CU: no other workgroup that uses LDS -- every batch kernel of this library --
// becomes resident beside it.  A table run is ONE wave whose dependent chain is what the call waits for; on a CU it shares with eight waves
// per SIMD of the batch's forward pass it queues behind their MFMAs (64 cycles of the pipe each) and LDS traffic at every link of the chain
// (measured: 1.8 ms alone, 4.5 ms beside k_filter_sp16).  One CU of 256 is what the isolation costs the batch.  0: the runtime refused
// (the run then shares its CU; nothing records that).
size_t whole_cu_lds(const void* fn);
template <class Kernel, class... Args>
inline hipError_t launch(Kernel kernel, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, const Args&... args) {
  if (lds_bytes > 64 * 1024) {
    const hipError_t err = lds_opt_in((const void*)kernel, lds_bytes);
    if (err != hipSuccess) return err;
  }
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, s, args...);
  return hipGetLastError();
}

// ---- generic wave-per-series kernels (any d <= 64, p <= 64), dlm_generic.hip ----------
size_t generic_filter_lds_bytes(int d, int p);
size_t generic_smoother_lds_bytes(int d, int p);
size_t generic_sampler_lds_bytes(int d, int p);
hipError_t launch_generic_filter(const KArgs& a, hipStream_t s);
hipError_t launch_generic_smoother(const KArgs& a, hipStream_t s);
hipError_t launch_generic_sampler(const KArgs& a, hipStream_t s);
hipError_t launch_generic_simulate(const KArgs& a, hipStream_t s);   // a.theta = x (nullable), a.smooth = y
hipError_t launch_stats_pool(const double* stats, int N, int L, double* pooled, hipStream_t s);

// ---- specialised d <= 16, p == 1 kernels on the fp64 MFMA layout, dlm_mfma16.hip ------
bool mfma16_supported(const KArgs& a);   // dense-G kernels: regular grid only
bool fast_shape(const KArgs& a);         // d <= 15, p == 1, time-invariant F
// `side` [N][T+1][2] carries (e_t/Q_t, 1/Q_t) from the forward to the backward pass (NaN = no update)
hipError_t launch_mfma16_filter(const KArgs& a, double* side, hipStream_t s);
hipError_t launch_mfma16_smoother(const KArgs& a, const double* side, hipStream_t s);

// ---- structured-G variant of the fast path (<= 4 nonzeros per row/column), dlm_sparse16.hip
struct SparseT { int K; int pad; int idx[16][4]; double val[16][4]; };
int sparse16_analyse(const double* G_host, int d, SparseT* rows, SparseT* cols);
// sparse16 kernels take tabs[2 * gi + 0] = rows of G_gi, tabs[2 * gi + 1] = columns of G_gi; K = max count
// xplus != nullptr: simulation-smoother forward pass (also writes x+ [N][T+1][d])
hipError_t launch_sparse16_filter(const KArgs& a, int K, const SparseT* rows_dev, double* side, double* xplus, hipStream_t s);
// tabs_dev[0] = rows of G, tabs_dev[1] = columns of G
hipError_t launch_sparse16_simsmooth(const KArgs& a, int K, const SparseT* tabs_dev, const double* side, const double* xplus, hipStream_t s);
// the reference-form backward sampler (a.filt_in -> theta / cond / stats), dlm_sampler16.hip; tabs_dev as above
hipError_t launch_sparse16_sampler(const KArgs& a, int K, const SparseT* tabs_dev, hipStream_t s);
hipError_t launch_small_mv_sampler(const KArgs& a, hipStream_t s);   // the same for d <= 15, p >= 2 (a.spb tables)
// RTS smoother (Smoothing.smoothStep) from filter records alone on the same register tiles; textbook or literal Q1
hipError_t launch_sparse16_rts(const KArgs& a, int K, const SparseT* tabs_dev, hipStream_t s);
hipError_t launch_small_mv_rts(const KArgs& a, hipStream_t s);
hipError_t launch_sparse16_smoother(const KArgs& a, int K, const SparseT* cols_dev, const double* side, hipStream_t s);
hipError_t launch_sparse16_count_gaps(const KArgs& a, unsigned char* plain, hipStream_t s);   // KArgs::plain of the call from its observations
// ---- shared covariance sequence: with parameters shared by the batch and no missing observation C_t, R_t, K_t,
// Q_t, P_t and S_t do not depend on the data.  ONE wave runs the covariance recursions (the per-series kernels' own code on a
// series of zeros: the same arithmetic, bit for bit) into L2-resident tables, and every series runs only its mean recursions
// against them.  A series that meets a missing observation is marked in KArgs::route and served by the per-series kernels.
struct CovTabs {
  double* ftab;   // [T+1] rows of frow bytes: [filtered record of the covariance-only run (mean slots 0): C_t | 16 doubles: R_t F (full
                  //   step) or K_t (steady step) per component, [15] = +-1/Q_t (negative: steady step)]
  double* btab;   // [T+1] rows of brow bytes: [smoothed record of the covariance-only run: S_t | 16 doubles: K_t = C_t F / V per
                  //   component, [15] = 1 where the step was a steady one | C_t record]
  double* cside;  // [T+1][2]  side records of the covariance-only forward run (0, +-1/Q_t), read by its backward run
  double* eq;     // [N][T+1]  per series: e_t / Q_t, forward -> backward
  double* mc;     // fused call: the filtered means once more, compact -- [ceil(N / 4)][T+1][4][16] (512 bytes per wave and step) --
                  //   for the backward kernel (a sequential stream instead of 112 bytes out of every 1456-byte record); nullptr: dlm_filter_batch
  double* sc;     // (unused: the smoothed means of the record-writer experiment, profiles/r03_notes.md)
  int frow, brow;
  const int* skip;   // nullable: nonzero on the device -- the tables are not wanted after all (most series of the call have a gap): the covariance-only filter returns at once
};
size_t covtabs_doubles(int d, int T);   // doubles of the table block (everything but eq)
void covtabs_carve(double* base, int d, int T, CovTabs& t);
bool shared_cov_eligible(const KArgs& a);   // regular grid, time-invariant F / V / W, V, W, C0 shared by the batch, dense records, no prior / forecast records
hipError_t launch_sparse16_cov_filter(const KArgs& a, int K, const SparseT* rows_dev, const CovTabs& tabs, hipStream_t s);
hipError_t launch_sparse16_cov_smoother(const KArgs& a, int K, const SparseT* cols_dev, const CovTabs& tabs, hipStream_t s);
hipError_t launch_sparse16_mean_filter(const KArgs& a, int K, const SparseT* rows_dev, const CovTabs& tabs, hipStream_t s);
hipError_t launch_sparse16_mean_smoother(const KArgs& a, int K, const SparseT* cols_dev, const CovTabs& tabs, hipStream_t s);

// ---- shared factors of the reference-form backward sampler, dlm_sampler16.hip: J_t, H_t and chol(H_t) depend on
// the filtered covariances alone.  With parameters shared by the batch ONE wave runs k_sampler_sp16 on the records of a series of
// zeros into a table; every series without a missing observation draws with the mean-only kernel (four series per wave), the
// others with k_sampler_sp16 as always.  Draw for draw the per-series kernel's results, bit for bit.
struct SampTabs {
  double* rows;          // [T+1] rows of 16 x 34 doubles: per component c [ J_t^T[.][c] (16) | L_t[c][.] (16) | pad (2) ]
  double* zrec;          // [T+1][d + d^2] filter records of the series of zeros
  double* zeros;         // max(T, 16) zeros: its observations and initial mean
  unsigned char* need;   // [T+1] 1: row t was written (a full step); 0: the factors of the last row above it
  int* status;           // status of the zero series' two kernels, for every series served by the tables
  double* z4;            // the normals of the call, made while the batch is filtered.  d <= 15 (k_normals4): [ceil(N / 4)][T+1][4][16], 512 bytes per step
                         //   and wave of the draw kernel; 16 <= d <= 48 (k_normals_rows): [N][T+1][d].  nullptr: injected normals (KArgs::z)
  int zstride;           // d <= 15, table kernel: bytes between the records of the series of zeros (0: d + d^2 doubles; the rows of CovTabs::ftab otherwise)
  const double* mc4;     // d <= 15, draw kernel: the filtered means come from the mean-only forward kernel's compact stream ([ceil(N / 4)][T+1][4][16],
                         //   CovTabs::mc) instead of the filter records: a dlm_ffbs_batch call that does not want the records (filt_ws == NULL)
  int marked;            // KArgs::route holds this call's gap marks already (the draw launch does not mark again)
  double* ktab;          // 16 <= d <= 48: the steady gain K^T as the zero series' filter leaves it (KArgs::ktab), for k_steady_filter_w48
  int* settle;           // index of the last record of zrec that was written (KArgs::settle_step): the records above it repeat its covariance
};
bool sampler_shared_model_ok(const KArgs& a);   // V, W, C0 shared by the batch, regular grid, time-invariant model (what KArgs::stretches follows)
bool sampler_shared_eligible(const KArgs& a);   // ... and this call can use the table (no conditional-moment records, flags)
size_t sampler_shared_ws_bytes(const KArgs& a);
void sampler_shared_carve(void* ws, const KArgs& a, SampTabs& tb);
// the tables: filter on zeros, then the sampler with its export on (both one wave; stream s)
hipError_t launch_sampler_shared_tables(const KArgs& a, int K, const SparseT* tabs_dev, const SampTabs& tb, hipStream_t s);
// the same from covariance records that exist already (crec, stride bytes apart: the forward table of the shared-covariance kernels)
hipError_t launch_sampler_shared_tables_from(const KArgs& a, int K, const SparseT* tabs_dev, SampTabs tb, const double* crec, int stride, hipStream_t s);
size_t sampler_shared_normals_bytes(const KArgs& a);
hipError_t launch_sampler_shared_normals(const KArgs& a, double* z4, hipStream_t s);   // the Philox normals of every series and step, in the draw kernel's layout
// a.route [N] is filled here (series with a missing observation), the mean-only kernel draws for the others, k_sampler_sp16 for these
hipError_t launch_sampler_shared_draw(const KArgs& a, int K, const SparseT* tabs_dev, const SampTabs& tb, hipStream_t s);

// Shared factors of the RTS smoother (Smoothing.scala:38-47, textbook or literal Q1; dlm_sampler16.hip): k_smoother_rts16 runs once, on the
// filter records of a series of zeros, into these tables; every series without a missing observation runs the mean recursion against them
// (k_mean_rts16, four series per wave), the others k_smoother_rts16 as always.  Bit for bit the per-series kernel's records.
struct RtsTabs {
  double* jrows;         // [T+1] rows of 16 x 18 doubles: per component c [ J_t^T[.][c] (16) | pad (2) ], written where need[t]
  double* srec;          // [T+1][d + d^2] smoothed records of the series of zeros: S_t behind d doubles nobody reads
  unsigned char* need;   // [T+1] 1: row t of jrows was written (a full step); 0: J of the last row above it
  int* status;           // status of the zero series' two kernels, for every series served by the tables
  const double* crec;    // the covariances exist already: records crec_stride bytes apart (the forward table of the shared-covariance kernels, CovTabs::ftab)
  int crec_stride;
  int* gaps;             // the number of series with a missing observation (launch_rts_shared_mark)
  int* skip;             // 1: more than half of the series have one -- the tables are not made, every series is routed to the per-series kernel
};
// The tables are a function of the model and of V, W, C0 alone: the engine keeps those of the last call that made them, in a workspace of
// their own, and the next call uses them when everything they were computed from is byte for byte the same.  The key is a
// copy of every byte the two one-wave kernels (k_cov_filter_sp16, k_smoother_rts16<.., true>) read; k_rts_key_check compares it with the
// call's on the engine's stream -- the words themselves, no checksum -- and k_rts_key_commit writes it behind a table run.
// What becomes of every field of KArgs in those two kernels (tests/test_rts_table_reuse_host.py holds this list against the struct, the
// key, sampler_shared_model_ok and the launchers):
//   RTS-KEY keyed:    d T flags F V W C0 G
//                     (flags: the bits of RTS_KEY_FLAGS, what the two kernels test; G: as the tables of its rows and columns, SparseT [2],
//                      and their K -- the kernels read G nowhere else)
//   RTS-KEY fixed:    p g_index dt f_stride v_stride w_stride v_tstride w_tstride c0_stride packed
//                     (one value only: sampler_shared_model_ok refuses the call otherwise)
//   RTS-KEY replaced: N y m0_stride filt_in filt smooth status stats loglik prior fq route counters theta z series_offset plain settle_step
//                     (per call: table_run_args carries none of them; launch_rts_shared_tables / cov_args / launch_cf set the table run's own
//                      where it has one)
//   RTS-KEY unread:   n_g m0 cond spb spb_k spf spf_k seed route_take keep_cov ktab leave_step stretches
//                     (n_g: without g_index only G_0 is used; m0: the covariance-only run starts from a mean of zeros; seed: simulation smoother
//                      only; route_take: behind route; the others belong to other kernels)
constexpr unsigned RTS_KEY_FLAGS = (1u << 0) | (1u << 22);   // DLM_OPT_SMOOTHER_COMPAT_Q1 (S_t), DLM_OPT_NO_STEADY (the covariance-only filter)
struct RtsKeySrc {         // the call's side of the comparison: device pointers of the call
  int d, T, K;             // K: the sparsity class, the template argument of both kernels
  unsigned flags;          // KArgs::flags & RTS_KEY_FLAGS
  const double *F, *V, *W, *C0;
  const SparseT* sp;       // [2] rows, columns of G
};
// control words of the kept tables, at the head of their workspace: [0] the zero series' status (what RtsTabs::status points at: kept with the
// tables), [8] gaps, [9] skip (RtsTabs), then
enum { RTS_CTL_HIT = 10,     // this call found its key: the kept tables serve it
       RTS_CTL_GATE = 11,    // skip | hit: what the two table kernels take for RtsTabs::skip -- they return at once
       RTS_CTL_VALID = 12,   // the workspace holds a complete set of tables and their key
       RTS_CTL_LAST = 13 };  // DLM_TABLES_* of the call (dlm_last_table_reuse)
struct RtsKeep { int* ctl; unsigned* key; };
constexpr int RTS_KEY_WORDS = 8 + 2 * (15 + 1 + 2 * 15 * 15) + 2 * (int)(sizeof(SparseT) / 4);   // at d = 15
bool rts_shared_eligible(const KArgs& a, bool textbook);   // textbook: the call asks for S = C - J (R+ - S+) J^T (the default): a larger batch is needed to pay for the tables
size_t rts_shared_ws_bytes(const KArgs& a);
void rts_shared_carve(void* ws, const KArgs& a, RtsTabs& tb, RtsKeep& keep);   // (control words and key first: where they are does not depend on T)
// behind launch_rts_shared_mark on the engine's stream: hit, gate; a miss marks the kept tables invalid before anything overwrites them.
// no_reuse (DLM_OPT_NO_TABLE_REUSE): always a miss, and nothing is kept
hipError_t launch_rts_key_check(const KArgs& a, int K, const SparseT* tabs_dev, const RtsKeep& keep, bool no_reuse, hipStream_t s);
// behind launch_rts_shared_tables on its stream: after a table run that ran, the key and "valid"
hipError_t launch_rts_key_commit(const KArgs& a, int K, const SparseT* tabs_dev, const RtsKeep& keep, bool no_reuse, hipStream_t s);
// the tables: the covariance-only filter into ctb.ftab (launch_sparse16_cov_filter), then the smoother with its export on (both one wave).
// gate: the device word for which the two kernels return at once (RTS_CTL_GATE)
hipError_t launch_rts_shared_cov(const KArgs& a, int K, const SparseT* tabs_dev, RtsTabs& tb, const CovTabs& ctb, const int* gate, hipStream_t s);
hipError_t launch_rts_shared_tables(const KArgs& a, int K, const SparseT* tabs_dev, const RtsTabs& tb, const int* gate, hipStream_t s);
hipError_t launch_rts_shared_mark(const KArgs& a, unsigned char* route, const RtsTabs& tb, hipStream_t s);   // KArgs::route of the call from its observations; tb.gaps, tb.skip
hipError_t launch_rts_shared_means(const KArgs& a, int K, const SparseT* tabs_dev, const RtsTabs& tb, bool own_rts, hipStream_t s);
// behind launch_rts_key_commit on its stream: S_t of the tables into a.smooth for every series that route leaves to them (k_rts_broadcast); the mean
// kernel of launch_rts_shared_means writes the lines that hold s_t
hipError_t launch_rts_broadcast(const KArgs& a, const unsigned char* route, const RtsTabs& tb, hipStream_t s);

// the same for 16 <= d <= 48 (dlm_wave48.hip): rows of 64 x (4 DT^2 + 16 DT) doubles, per lane [ J^T tiles | row `lane` of L ]
bool wave48_sampler_shared_model_ok(const KArgs& a);
bool wave48_sampler_shared_eligible(const KArgs& a);
size_t wave48_sampler_shared_ws_bytes(const KArgs& a);
void wave48_sampler_shared_carve(void* ws, const KArgs& a, SampTabs& tb);
hipError_t launch_wave48_sampler_shared_tables(const KArgs& a, const SampTabs& tb, hipStream_t s, hipEvent_t after_filter = nullptr);   // after_filter: recorded behind the zero series' filter (ktab, settle)
hipError_t launch_wave48_sampler_shared_draw(const KArgs& a, const SampTabs& tb, hipStream_t s);
size_t wave48_ktab_doubles(const KArgs& a);
// the steady steps of the series without a gap, from record *settle on: a = G m, e = y - F^T a, m = a + K e (the per-wave filter's steady step,
// operation for operation), the mean stored into the records' mean slots; k.keep_cov marks the series, ktab / settle come from the zero series
hipError_t launch_wave48_steady_filter(const KArgs& a, const double* ktab, const int* settle, hipStream_t s);
hipError_t launch_wave48_mark_gaps(const KArgs& a, unsigned char* route, hipStream_t s);   // route[n] = 1: series n has a missing observation component
size_t wave48_sampler_shared_normals_bytes(const KArgs& a);
hipError_t launch_wave48_sampler_shared_normals(const KArgs& a, double* z, hipStream_t s);   // rows [N][T+1][d], SampTabs::z4 of these calls

// ---- multivariate path: workgroup per series, MFMA-tiled GEMMs from LDS, dlm_tiled.hip --------
// Nonzeros of the rows (`rows`) and of the columns (`cols`) of a d x d G with at most 4 per row and column (every
// model the reference can build): the congruences G C G^T and G^T M G are then two gather passes instead of two
// dense MFMA products.  sparse48_analyse returns the largest count, or 99 if G is not that sparse.
struct SparseBig { int K; int pad; int idx[48][4]; double val[48][4]; };
int sparse48_analyse(const double* G_host, int d, SparseBig* rows, SparseBig* cols);
// The same for the observation matrix F (d x p): block models composed with |*| (Dlm.scala:197-208) have one component's
// few nonzeros in every column.  cidx/cval: nonzeros of column j (states loading on observation j); ridx/rval: nonzeros of
// row i (observations state i loads on).  sparsef_analyse returns the largest count, or 99 if F is not that sparse.
struct SparseF { int K; int pad; int cidx[32][4]; double cval[32][4]; int ridx[48][4]; double rval[48][4]; };
int sparsef_analyse(const double* F_host, int d, int p, SparseF* out);
bool tiled_supported(const KArgs& a);
// innov [N][T][p] (nullable for the filter): innovations y_t - f_t (NaN = missing) handed from the forward to the backward pass
hipError_t launch_tiled_filter(const KArgs& a, double* innov, hipStream_t s);
hipError_t launch_tiled_smoother(const KArgs& a, const double* innov, hipStream_t s);
// ---- one wavefront per series, register-resident tiles (structured G, 16 <= d <= 48), dlm_wave48.hip ----
bool wave48_small_shape(const KArgs& a);   // d <= 15 with 2 <= p <= 32: the per-wave kernels with one tile per dimension
bool wave48_small_ok(const KArgs& a);      // ... and a structured G
bool wave48_filter_supported(const KArgs& a);
hipError_t launch_wave48_filter(const KArgs& a, int K, double* innov, hipStream_t s);
bool wave48_smoother_supported(const KArgs& a);
hipError_t launch_wave48_smoother(const KArgs& a, int K, const double* innov, hipStream_t s);
bool wave48_simsmooth_supported(const KArgs& a);
hipError_t launch_wave48_simsmooth(const KArgs& a, int K, double* xplus, double* ystar, hipStream_t s);
bool wave48_sampler_supported(const KArgs& a);   // the reference-form backward sampler on register tiles (16 <= d <= 48, structured G)
hipError_t launch_wave48_sampler(const KArgs& a, hipStream_t s);
// simulation-smoother FFBS (forward SIM pass + mean-only backward pass); xplus [N][T+1][d], ystar [N][T][p]
hipError_t launch_tiled_simsmooth(const KArgs& a, double* xplus, double* ystar, hipStream_t s);

// ---- SVD filter / sampler (one-sided Jacobi in LDS), dlm_svd.hip ----------------------
bool svd_supported(const KArgs& a);      // d <= 48, p <= 32
size_t svd_filter_lds_bytes(int d, int p);
hipError_t launch_svd_filter(const KArgs& a, double* svd_rec, hipStream_t s);
hipError_t launch_svd_sampler(const KArgs& a, const double* svd_rec, hipStream_t s);
// shared factors (parameters shared by the batch, no missing observation): the decompositions once per call, a mean-only kernel per series
bool svd_shared_eligible(const KArgs& a);
size_t svd_shared_ws_doubles(const KArgs& a);
hipError_t launch_svd_filter_shared(const KArgs& a, double* svd_rec, double* ws, unsigned char* route, hipStream_t s);

// ---- one lane per series for d <= 3, p = 1 (dlm_lane.hip): filter (+ prior / forecast records, log-likelihood), RTS smoother
bool lane_supported(const KArgs& a);
hipError_t launch_lane_filter(const KArgs& a, hipStream_t s);
hipError_t launch_lane_smoother(const KArgs& a, hipStream_t s);   // a.filt_in -> a.smooth; no side buffer
hipError_t launch_lane_sampler(const KArgs& a, hipStream_t s);   // the literal backward sampler (a.filt_in -> theta / cond / stats)
hipError_t launch_lane_simsmooth(const KArgs& a, double* xplus, hipStream_t s);   // simulation-smoother FFBS + statistics (time-invariant V, W)

// ---- scalar AR(1) FFBS, one lane per series (FilterAr.scala:15-82), dlm_ar1.hip -----------------
// times != nullptr: the Ornstein-Uhlenbeck variant on that (shared, irregular) time grid (FilterOu.scala:7-79)
hipError_t launch_ar1_ffbs(int N, int T, const double* times, const double* y, const double* v, long long v_stride,
                           const double* sv, long long sv_stride, const double* z, unsigned long long seed,
                           unsigned long long series_offset, double* filt, double* theta, int* status, hipStream_t s);

// ---- the Gibbs parameter steps: where a call's draws sit in the Philox counter space (dlm_draws.h) ----
struct DrawStream { unsigned long long seed, series_offset, iteration; };   // series n draws at (seed, series_offset + n, iteration)

// ---- d-Inverse-Gamma conjugate draws on the device (Gibbs.scala:23-78), dlm_gibbs.hip --------------
hipError_t launch_dinvgamma_step(int d, int p, int N, const double* stats, double av, double bv, double aw, double bw,
                                 const DrawStream& rs, double* Vout, double* Wout, hipStream_t s);

// ---- Student-t observation DLM: one Gibbs step after the FFBS call (StudentTGibbs.scala:182-212), dlm_studentt.hip -------------
struct StudentTArgs {
  int d, T, N;
  const double* F; long long f_stride;   // F_t = F + t * f_stride (d doubles, p = 1)
  const double* y;        // [N][T]
  const double* theta;    // [N][T+1][d]
  const double* stats;    // [N][d + 3] = [ssy | n | ss (d) | T] of the FFBS call
  const double* scale_in; const int* nu_in;
  dlm_studentt_prior prior;
  int literal;            // DLM_OPT_STUDENTT_LITERAL
  DrawStream rs;
  double* v_out; double* scale_out; int* nu_out; double* W_out; int* accepted;
  double* loglik; int* status;   // nullable
};
hipError_t launch_studentt_step(const StudentTArgs& a, hipStream_t s);

// ---- AR(1) stochastic volatility: the mixture indicators before the AR(1) FFBS call and the parameter draws after it
// (StochasticVolatility.scala:112-157, :170-252, StochVolKnots.scala:25-43), dlm_sv.hip -------------
struct SvMixArgs {
  int N, T;
  const double* y;        // [N][T]
  const double* alpha;    // [N][T+1], or nullptr: the initial transform (no draw)
  DrawStream rs;
  double* ystar; double* v;   // [N][T]
  signed char* k;         // [N][T], nullable
  int* status;            // [N], nullable (zeroed by the caller)
};
struct SvParamsArgs {
  int N, T;
  const double* alpha;    // [N][T+1]
  const double* sv_in;    // [N][3] = (phi, mu, sigma_eta)
  dlm_sv_prior prior;
  DrawStream rs;
  double* sv_out;         // [N][3], may be sv_in
  int* accepted; int* status;   // nullable
};
hipError_t launch_sv_mixture(const SvMixArgs& a, hipStream_t s);
hipError_t launch_sv_params(const SvParamsArgs& a, hipStream_t s);

// ---- AR(1) stochastic volatility: the knot block sampler of the state (StochVolKnots.scala:74-176), one red-black sweep in place,
// dlm_sv_knots.hip -------------
struct SvKnotsArgs {
  int N, T, B;
  const double* y;        // [N][T]
  const int* knots;       // [B+1], shared by the batch: 0 = k_0 < ... < k_B = T + 1 (checked on the host)
  const double* sv; long long sv_stride;   // (phi, mu, sigma_eta): [N][3] with stride 3, or one triple with stride 0
  DrawStream rs;
  double* alpha;          // [N][T+1], in and out
  double* filt;           // scratch [N][T+1][2]: the blocks' filtering records
  double* prop;           // scratch [N][T+1]: ystar, then the proposal
  int* rowflag;           // scratch [N]: the flags of the rows the sweep leaves alone
  int* accepted; int* status;   // nullable
};
hipError_t launch_sv_knots(const SvKnotsArgs& a, hipStream_t s);   // the row check, the even blocks, the odd blocks

// ---- stochastic volatility with Ornstein-Uhlenbeck log-volatility on an irregular grid: the three Metropolis moves after the OU
// FFBS call (StochasticVolatility.scala:350-431, :459-478), dlm_sv_ou.hip -------------
struct SvOuParamsArgs {
  int N, T;
  const double* times;    // [T], shared by the batch
  const double* alpha;    // [N][T+1] as dlm_ou_ffbs_batch writes its theta
  const double* sv_in;    // [N][3] = (phi, mu, sigma_eta), phi the mean-reversion rate
  dlm_sv_ou_prior prior;
  DrawStream rs;
  double* sv_out;         // [N][3], may be sv_in
  int* accepted;          // [N][3]: phi, sigma, mu
  int* status;            // nullable
};
hipError_t launch_sv_ou_params(const SvOuParamsArgs& a, hipStream_t s);

// ---- factor stochastic volatility: the factor draw and the draws of sigma^2 and the loading matrix around the factor chains'
// AR(1) volatility calls (FactorSv.scala:168-186, :253-333, :516-541), dlm_fsv.hip -------------
constexpr int DLM_FSV_MAX_K = 8, DLM_FSV_MAX_P = 64;
struct FsvFactorsArgs {
  int N, T, p, k;
  const double* y;        // [N][T][p]
  const double* beta;     // [N][p][k]
  const double* v;        // [N][p]
  const double* alpha;    // [N][k][T+1], or nullptr: unit factor variances (initialiseFactors)
  int literal;
  DrawStream rs;
  double* f;              // [N][k][T]
  int* status;            // [N], nullable (zeroed by the caller)
};
struct FsvLoadingsArgs {
  int N, T, p, k;
  const double* y;        // [N][T][p]
  const double* f;        // [N][k][T]
  const double* beta_in;  // [N][p][k]
  const double* v_in;     // [N][p], nullable: what v_out keeps for a panel without an observed time
  dlm_fsv_prior prior;
  DrawStream rs;
  double* beta_out;       // [N][p][k], may be beta_in
  double* v_out;          // [N][p], may be v_in
  int* status;            // [N], nullable (zeroed by the caller)
};
hipError_t launch_fsv_factors(const FsvFactorsArgs& a, hipStream_t s);
hipError_t launch_fsv_loadings(const FsvLoadingsArgs& a, hipStream_t s);

// ---- DLM with factor stochastic-volatility noise: what joins dlm_ffbs_batch to the factor sampler above (DlmFsv.scala:173-185;
// DlmFsvSystem.calculateVariance, DlmFsvSystem.scala:126-131), dlm_dlmfsv.hip.  k and p as above, d <= 64 -------------
struct DlmFsvCenterArgs {
  int N, T, p, d;
  const double* y;        // [N][T][p]
  const double* theta;    // [N][T+1][d]
  const double* F;        // [d*p] column-major, or [T][d*p] with f_stride = d*p
  long long f_stride;
  double* r;              // [N][T][p]
  int* status;            // [N], nullable (zeroed by the caller)
};
struct DlmFsvVarianceArgs {
  int N, T, p, k;
  const double* beta;     // [N][p][k]
  const double* v;        // [N][p]
  const double* alpha;    // [N][k][T+1]
  double* V;              // [N][T][p*p]
  int* status;            // [N], nullable (zeroed by the caller)
};
struct DlmFsvImputeArgs {
  int N, T, p, k;
  const double* r_in;     // [N][T][p], NaN = missing
  const double* beta;     // [N][p][k]
  const double* v;        // [N][p]
  const double* alpha;    // [N][k][T+1]
  DrawStream rs;
  double* r_out;          // [N][T][p], may be r_in
  int* status;            // [N], nullable (zeroed by the caller)
};
struct DlmFsvSysInnovationsArgs {   // the factor process as the system noise (factorState, DlmFsvSystem.scala:109-117)
  int N, T, d;
  const double* theta;    // [N][T+1][d]
  const double* G;        // [d*d] column-major
  double* w;              // [N][T][d], not theta
  int* status;            // [N], nullable (zeroed by the caller)
};
hipError_t launch_dlmfsvsys_innovations(const DlmFsvSysInnovationsArgs& a, hipStream_t s);
hipError_t launch_dlmfsv_impute(const DlmFsvImputeArgs& a, hipStream_t s);
hipError_t launch_dlmfsv_center(const DlmFsvCenterArgs& a, hipStream_t s);
hipError_t launch_dlmfsv_variance(const DlmFsvVarianceArgs& a, hipStream_t s);

// ---- posterior-predictive forecasts of the factor stochastic-volatility models: future log-volatility paths and the summary of the
// Gaussian mixture they give per time (mean, total covariance, exact marginal quantiles), dlm_fsv_forecast.hip -------------
struct SvPathsArgs {
  int N, k, H, R;
  const double* sv;       // [N][k][3] = (phi, mu, sigma_eta)
  const double* alpha0;   // [N][k], or nullptr: a stationary start
  DrawStream rs;
  double* alpha;          // [N][R][k][H+1]
  int* status;            // [N], nullable (zeroed by the caller)
};
constexpr int DLM_MIX_MAX_P = 64, DLM_MIX_MAX_NQ = 8, DLM_MIX_MAX_C = 1 << 30;   // (C + 256 fits an int: the kernels' component loops)
constexpr int DLM_MIX_LDS_C = 4096;   // the components of a cell that k_mixture_quantiles holds in LDS; beyond it they are packed into `pack`
struct MixtureArgs {
  int N, C, H, p, nq;
  const double* f;        // component c of row n at time h: f + n f_nstride + c f_cstride + h f_tstride (p doubles), or nullptr: 0
  const double* Q;        // ... Q + n q_nstride + c q_cstride + h q_tstride (p p doubles, symmetric)
  long long f_nstride, f_cstride, f_tstride, q_nstride, q_cstride, q_tstride;
  double probs[DLM_MIX_MAX_NQ];
  int cell_first;         // k_mixture_quantiles: the launch serves the cells cell_first .. cell_first + (grid size) - 1 of the N H p
  double* pack;           // C > DLM_MIX_LDS_C: [launch's cells][C][2] = (f_ci, sqrt(2 Q_cii)), else nullptr
  double* mean;           // [N][H][p]
  double* cov;            // [N][H][p p]
  double* quant;          // [N][H][p][nq], nullable with nq = 0
  int* status;            // [N], nullable (zeroed by the caller)
};
hipError_t launch_sv_paths(const SvPathsArgs& a, hipStream_t s);
hipError_t launch_mixture_moments(const MixtureArgs& a, hipStream_t s);
hipError_t launch_mixture_quantiles(const MixtureArgs& a, int cells, hipStream_t s);

// ---- the particle filters of a DGLM, one wavefront per series: what all three kernels read and write (dlm_pf_common.h) ---------------------
// PfArgs and StorvikArgs derive from it.  LwArgs repeats the fields under the same names in the order k_lw was written with: its kernel
// holds 106 SGPRs, and where the arguments lie decides how many of them it parks in VGPRs -- every derived order that was tried moves its
// register count at some d (profiles/r23_notes.md).  The host code stages all three through one template.
struct PfCommonArgs {
  int d, T, N, P;         // P particles, a multiple of 64
  int family, n0, literal;   // DLM_OBS_*; resample when ESS < n0 (resolved: >= 0); 1: the reference's arithmetic (Q37-Q39, Q43)
  const double* F; long long f_stride;   // F_t = F + t * f_stride (d doubles, p = 1)
  const double* G; int n_g; const int* g_index; const double* dt;
  const double* V; long long v_stride;   // v = V[n * v_stride]; k_storvik reads it without learn_v only
  const double* m0; long long m0_stride;
  const double* C0; long long c0_stride;
  const double* obs_param;   // [N], nullable: nu of DLM_OBS_STUDENTT
  const double* y;        // [N][T], NaN = missing
  DrawStream rs;
  double* ll;             // [N]
  double* mean;           // [N][T][d], nullable
  double* ess;            // [N][T], nullable
  double* cloud;          // [N][d][P], nullable
  double* weights;        // [N][P], nullable
  int* status;            // [N], nullable (zeroed by the caller)
};

// ---- bootstrap particle filter (ParticleFilter.scala:38-85, Dglm.scala:46-175), dlm_pf.hip ----------------------------------------------
struct PfArgs : PfCommonArgs {
  const double* W; long long w_stride;
};
// dlm_pf_resampled: k_pf's arguments and the scheme.  DLM_RESAMPLE_MULTINOMIAL launches k_pf on the PfArgs part, any other scheme k_pf_scheme
struct PfSchemeArgs : PfArgs {
  int resample, mh_steps;   // DLM_RESAMPLE_*; the steps of a Metropolis chain, 1 .. DLM_PF_MAX_MH_STEPS (0 under the other schemes)
};
size_t pf_lds_bytes(int d, int P);   // the cloud [d][P], the weights and their running sums [2][P], chol(W) and chol(C0)
hipError_t launch_pf(const PfSchemeArgs& a, hipStream_t s);

// ---- posterior-predictive forecast of a DGLM from a cloud (Dglm.forecastParticles, Dglm.scala:305-335), dlm_pf_forecast.hip -------------
// k_pf's step plus one observation draw per particle and their order statistics.  T is the number H of forecast steps; ess is always null
struct PfForecastArgs : PfCommonArgs {
  const double* W; long long w_stride;
  int slot_offset;        // step h draws from the Philox slot slot_offset + h
  int n_ranks; int ranks[8];   // 0 <= ranks[j] < P
  const double* cloud0;   // [N][d][P], nullable: the initial cloud is drawn from (m0, C0)
  const double* weights0; // [N][P], nullable: equal weights
  double* fmean;          // [N][T]
  double* fquant;         // [N][T][n_ranks], nullable with n_ranks = 0
  double* draws;          // [N][T][P], nullable
};
hipError_t launch_pf_forecast(const PfForecastArgs& a, hipStream_t s);   // the LDS is pf_lds_bytes: the draws are sorted in the row `cum`

// ---- Storvik filter: a particle filter that learns the diagonal of W (and V, Gaussian family) online (Storvik.scala:105-159), dlm_storvik.hip ----
struct StorvikArgs : PfCommonArgs {
  int learn_v;            // 1: V is learned (Gaussian family)
  const double* prior_v; long long prior_v_stride;   // [2] = (shape, scale) at n * prior_v_stride, read with learn_v only
  const double* prior_w; long long prior_w_stride;   // [d][2] at n * prior_w_stride
  double* scale_mean;     // [N][T][d+1], nullable
  double* scales;         // [N][d+1][P], nullable
};
size_t storvik_lds_bytes(int d, int P);   // the cloud and the scales of W [2 d][P], the scale of V, the weights and their running sums [3][P], chol(C0), the ancestors
hipError_t launch_storvik(const StorvikArgs& a, hipStream_t s);

// ---- Liu-West filter: an auxiliary particle filter whose particles carry their own log-variances (LiuAndWest.scala:47-81, AuxFilter.scala), dlm_lw.hip ----
struct LwArgs {           // PfCommonArgs' fields and its own, in the order that holds k_lw's register counts (above)
  int d, T, N, P;         // P particles, a multiple of 64
  int family, n0, literal, learn_v;   // DLM_OBS_*; the second stage resamples when ESS < n0 (resolved: >= 0); 1: Q39, Q50, Q51; 1: log V is a row of psi
  double a;               // the shrinkage, 0 < a <= 1
  const double* F; long long f_stride;   // F_t = F + t * f_stride (d doubles, p = 1)
  const double* G; int n_g; const int* g_index; const double* dt;
  const double* V; long long v_stride;   // v = V[n * v_stride], read without learn_v only
  const double* m0; long long m0_stride;
  const double* C0; long long c0_stride;
  const double* prior_v; long long prior_v_stride;   // [2] = (mean, sd) of log V at n * prior_v_stride, read with learn_v only
  const double* prior_w; long long prior_w_stride;   // [d][2] = (mean, sd) of log W_kk at n * prior_w_stride
  const double* obs_param;   // [N], nullable: nu of DLM_OBS_STUDENTT
  const double* y;        // [N][T], NaN = missing
  DrawStream rs;
  double* ll;             // [N]
  double* mean;           // [N][T][d], nullable
  double* ess;            // [N][T], nullable
  double* psi_mean;       // [N][T][d+1], nullable
  double* psi_var;        // [N][T][d+1], nullable
  double* cloud;          // [N][d][P], nullable
  double* weights;        // [N][P], nullable
  double* psi;            // [N][d+1][P], nullable
  int* status;            // [N], nullable (zeroed by the caller)
};
size_t lw_lds_bytes(int d, int P);   // the cloud [d][P], the log-variances [d + 1][P], the weights and their running sums [2][P], chol(C0), h s [d + 1], the ancestors
hipError_t launch_lw(const LwArgs& a, hipStream_t s);

// ---- Rao-Blackwellised filter of a Gaussian DLM: the Liu-West filter whose particles carry the Kalman moments (m, C) of the state given their own
// log-variances in place of a drawn state (RaoBlackwellFilter.scala), dlm_rb.hip ----
struct RbArgs {           // a struct of its own: the fields the host's shared staging fills keep PfCommonArgs' names
  int d, T, N, P;         // P particles, a multiple of 64
  int family, n0, literal, learn_v;   // always DLM_OBS_GAUSSIAN; the second stage resamples when ESS < n0 (resolved: >= 0); 1: Q50, Q57, Q58; 1: log V is a row of psi
  double a;               // the shrinkage, 0 < a <= 1
  const double* F; long long f_stride;   // F_t = F + t * f_stride (d doubles, p = 1)
  const double* G; int n_g; const int* g_index; const double* dt;
  const double* V; long long v_stride;   // v = V[n * v_stride], read without learn_v only
  const double* m0; long long m0_stride;
  const double* C0; long long c0_stride;   // column-major, the lower triangle is read
  const double* prior_v; long long prior_v_stride;   // [2] = (mean, sd) of log V at n * prior_v_stride, read with learn_v only
  const double* prior_w; long long prior_w_stride;   // [d][2] = (mean, sd) of log W_kk at n * prior_w_stride
  const double* obs_param;   // always null (the shared staging's field)
  const double* y;        // [N][T], NaN = missing
  DrawStream rs;
  double* ll;             // [N]
  double* mean;           // [N][T][d], nullable
  double* cov;            // [N][T][d][d], nullable: the mixture covariance
  double* ess;            // [N][T], nullable
  double* psi_mean;       // [N][T][d+1], nullable
  double* psi_var;        // [N][T][d+1], nullable
  double* cloud;          // [N][d][P], nullable: the particles' Kalman means after the last step
  double* covs;           // [N][d(d+1)/2][P], nullable: their covariances, the lower triangle by rows
  double* weights;        // [N][P], nullable
  double* psi;            // [N][d+1][P], nullable
  int* status;            // [N], nullable (zeroed by the caller)
};
size_t rb_lds_bytes(int d, int P);   // the means [d][P], the covariances [d(d+1)/2][P], the log-variances [d + 1][P], the weights and their running sums [2][P], one slot of predicted covariances [d(d+1)/2][64], G^T F [d], the step's mean [d], h s [d + 1], the ancestors
hipError_t launch_rb(const RbArgs& a, hipStream_t s);

// ---- posterior-predictive forecast from the cloud of a LEARNING filter, whose particles carry their own variances (dlm_storvik_batch's scales,
// dlm_lw_batch's and dlm_rb_batch's psi), dlm_pf_forecast_learned.hip.  k_pf_forecast's layout and step with a diagonal state noise s_k,i and an
// observation scale v_i per particle; nothing is observed, weighted or resampled after the entry.  T is the number H of forecast steps
struct PfForecastLearnedArgs {
  int d, T, N, P;         // P particles, a multiple of 64
  int family, var_kind;   // DLM_OBS_*; DLM_FC_VAR, DLM_FC_LOGVAR or DLM_FC_IG_SCALE: what the rows of pw and pv hold
  const double* F; long long f_stride;   // F_t = F + t * f_stride (d doubles, p = 1)
  const double* G; int n_g; const int* g_index; const double* dt;
  const double* V; long long v_stride;   // v = V[n * v_stride] for every particle, read without pv only
  const double* obs_param;   // [N], nullable: nu of DLM_OBS_STUDENTT
  DrawStream rs;
  int slot_offset;        // step h draws from the Philox slot slot_offset + h
  int n_ranks; int ranks[8];   // 0 <= ranks[j] < P
  const double* cloud0;   // [N][d][P]
  const double* weights0; // [N][P], nullable: equal weights
  const double* pw;       // [N][d][P] the rows of the state variances
  const double* pv;       // [N][P], nullable: the row of the observation scale
  const double* shapes; long long shapes_stride;   // [d + 1] at n * shapes_stride, DLM_FC_IG_SCALE only (entry d is read with pv only)
  double* fmean;          // [N][T]
  double* fquant;         // [N][T][n_ranks], nullable with n_ranks = 0
  double* draws;          // [N][T][P], nullable
  double* mean;           // [N][T][d], nullable
  double* cloud;          // [N][d][P], nullable
  double* var_w;          // [N][d][P], nullable: the variances the steps used
  double* var_v;          // [N][P], nullable
  int* status;            // [N], nullable (zeroed by the caller)
};
size_t pf_forecast_learned_lds_bytes(int d, int P);   // the cloud and the standard deviations of the state noise [2 d][P], the observation scale, the weights and the row of the draws [3][P], the ancestors
hipError_t launch_pf_forecast_learned(const PfForecastLearnedArgs& a, hipStream_t s);

// ---- a state per particle from the Kalman moments dlm_rb_batch leaves: x_i = m_i + chol(C_i) z_i, dlm_pf_forecast_learned.hip ----
struct RbStateDrawArgs {
  int d, N, P;
  const double* means;    // [N][d][P]
  const double* covs;     // [N][d(d+1)/2][P], the lower triangles by rows
  DrawStream rs;
  unsigned slot;
  double* cloud;          // [N][d][P]
  int* status;            // [N], nullable (zeroed by the caller)
};
hipError_t launch_rb_state_draw(const RbStateDrawArgs& a, hipStream_t s);   // no dynamic LDS: a particle's factor lives in its thread's registers

// ---- Particle Gibbs: conditional SMC with ancestor sampling, one draw of the state path x_{0:T} | y, V, W of a DGLM (Andrieu, Doucet & Holenstein
// 2010; Lindsten, Jordan & Schoen 2014; what ParticleGibbs.scala aims at), dlm_pg.hip ----
// A struct of its own: the fields the host's shared staging fills keep PfCommonArgs' names (n0 and literal are staged and not read).  A LAUNCH serves
// the series n_first .. n_first + (grid size) - 1 of the call: every per-series array of the call is indexed by the call's n, the two workspaces
// `clouds` and `ancestors` by the launch's own block index.
struct PgArgs {
  int d, T, N, P;         // P particles, a multiple of 64; particle P - 1 is the reference
  int family, n0, literal, ancestor_sampling;
  int n_first;            // the launch's first series
  const double* F; long long f_stride;   // F_t = F + t * f_stride (d doubles, p = 1)
  const double* G; int n_g; const int* g_index; const double* dt;
  const double* V; long long v_stride;
  const double* W; long long w_stride;
  const double* m0; long long m0_stride;
  const double* C0; long long c0_stride;
  const double* obs_param;   // [N], nullable: nu of DLM_OBS_STUDENTT
  const double* y;        // [N][T], NaN = missing
  const double* ref;      // [N][T+1][d] the reference path (may be `path`: a series reads all of its own before it writes)
  DrawStream rs;
  double* ll;             // [N]
  double* mean;           // always null (the shared staging's fields)
  double* ess;
  double* cloud;
  double* weights;
  double* path;           // [N][T+1][d]
  double* stats;          // [N][d + 3] = [ssy | n | ss (d) | T]
  int* path_index;        // [N][T+1], nullable
  double* step_weights;   // [N][T][P], nullable
  double* clouds;         // [launch][T+1][d][P]: the call's output where it was asked for, else the engine's workspace
  int* ancestors;         // [launch][T][P]
  int* status;            // [N], nullable (zeroed by the caller)
};
size_t pg_lds_bytes(int d, int P);   // pf_lds_bytes plus d doubles: ref_{t+1}
hipError_t launch_pg(const PgArgs& a, int n_series, hipStream_t s);   // the series a.n_first .. a.n_first + n_series - 1

// ---- KalmanFilter.likelihood literally (transition density of the filtered means), dlm_loglik.hip ------
size_t loglik_q7_ws_bytes(const KArgs& a);
hipError_t launch_loglik_q7(const KArgs& a, const double* records, void* ws, hipStream_t s);   // a.loglik [N] <- records [N][T+1][d+dd]

// ---- when may a converged covariance recursion stop being recomputed? -------------------------------------------------
// The reference recomputes C_t, R_t, K_t, Q_t (KalmanFilter.scala:64-107) and the smoother's matrices (Smoothing.scala:31-47)
// at every step.  The kernels may stop once the recursion has converged -- but a small ONE-STEP change says little about the
// distance to the limit when the recursion contracts slowly (small W / V): what remains is the geometric tail
// delta * rho / (1 - rho).  settle_test bounds that tail.  `delta` is the largest change of an entry over one step and
// `scale` the largest entry of the matrix (both wave-uniform); tests come every `period` steps on an uninterrupted regular
// stretch (settle_reset otherwise).  With r = delta_k / delta_{k-1} (= rho^period) and 1 / (1 - rho) <= period / (1 - r):
//     settled  <=>  period * delta_k / (1 - r)  <=  DLM_SETTLE_TOL * scale,
// where r is the LARGER of the last two estimates, each taken from two consecutive tests whose changes stand clear of the
// rounding noise of the recursion's own arithmetic (`noise`, relative to scale: 32 eps for the covariance recursions; a
// change below it counts as that level and gives no new estimate).  At least three tests, r < 1.  A recursion too slow to
// be resolved above the noise floor (rho > ~0.993 per step at period 4) never settles: it is recomputed at every step like
// the reference's.  What the rule assumes: from the test on, successive changes shrink at least as fast as the larger of
// the two measured ratios (the convergence is geometric by then).  NumPy replay against the every-step recursion:
// tools/settle_replay.py (the frozen matrix stays within DLM_SETTLE_TOL * max|C| for W scaled by 1 .. 1e-6 and V = 1e4 at
// T up to 40 000; the round-2 rule -- one step's change <= 1e-13 Q -- was off by up to 6e-9 there); GPU tests of every
// kernel that freezes, in the slow regime: tests/test_settle_gpu.py.
constexpr double DLM_SETTLE_TOL = 1e-12;
// The state of the test -- the relative change at the previous test (< 0: none) and the last two estimates of rho^period
// (2: none yet) -- lives in three floats of the wave's LDS (`st`): kept in registers it cost the d <= 15 backward kernel its
// fifth wave per SIMD.  Every lane reads and writes the same values (the maxima are wave-uniform): no lane masking, and the
// LDS queue of a wave is in order.
constexpr int SETTLE_FLOATS = 4;
__device__ __forceinline__ float settle_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ void settle_reset(float* st) { st[0] = -1.f; st[1] = 2.f; st[2] = 2.f; }
// (single precision throughout -- the callers bring their maxima into float range with a power-of-two factor --: a double
// division at the point where a kernel holds the most live values costs it a dozen registers)
__device__ __forceinline__ bool settle_test(float* st, float delta, float scale, int period, float noise = 7.1e-15f) {
  const float x = delta * __builtin_amdgcn_rcpf(scale);
  float prev = st[0], rate = st[1], rate_prev = st[2];
  bool ok = false;
  if (!(x >= 0.f) || !(x < 1e30f)) { prev = -1.f; rate = 2.f; rate_prev = 2.f; }   // NaN / Inf / empty matrix: start over
  else {
    const float xe = fmaxf(x, noise);
    if (prev > 8.f * noise && x >= noise) { rate_prev = rate; rate = xe * __builtin_amdgcn_rcpf(prev); }   // a clean pair
    const float r = fmaxf(rate, rate_prev);
    ok = r < 1.f && (float)period * xe <= (float)DLM_SETTLE_TOL * (1.f - r);
    ok |= (x == 0.f && prev == 0.f);                             // a fixed point reached bit for bit
    prev = x > 0.f ? xe : 0.f;
  }
  st[0] = prev; st[1] = rate; st[2] = rate_prev;
  return __builtin_amdgcn_readfirstlane((int)ok) != 0;
}
// NaN-proof |a - b| for the maxima that feed settle_test (fmax drops a NaN operand)
__device__ __forceinline__ double settle_absdiff(double a, double b) { const double v = fabs(a - b); return v == v ? v : __builtin_inf(); }
// 2^-k for x = f * 2^k (f in [1, 2)), x a positive normal wave-uniform double: brings matrices of x's order of magnitude into float range
__device__ __forceinline__ double settle_pow2_inverse_of(double x) {
  const int e = (__builtin_amdgcn_readfirstlane(__double2hiint(x)) >> 20) & 0x7ff;
  return (e > 0 && e < 0x7fe) ? __hiloint2double((2046 - e) << 20, 0) : __builtin_nan("");   // NaN: the test starts over
}

// ---- counter-based normals (same stream as oracle_normal in oracle/dlm_oracle.c) ------
__device__ __forceinline__ void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1;
    unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

__device__ __forceinline__ double philox_normal(unsigned long long seed, unsigned long long series,
                                                unsigned t, unsigned i) {
  unsigned c[4] = {(unsigned)series, (unsigned)(series >> 32), t, i >> 1};
  philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
  double u1 = ((double)c[0] * 4294967296.0 + (double)c[1] + 1.0) * (1.0 / 18446744073709551616.0);
  double u2 = ((double)c[2] * 4294967296.0 + (double)c[3]) * (1.0 / 18446744073709551616.0);
  double r = sqrt(-2.0 * log(u1));
  double ang = 6.283185307179586476925286766559 * u2;
  return (i & 1) ? r * sin(ang) : r * cos(ang);
}

// components 2 q and 2 q + 1 of record t share one Philox block and one Box-Muller pair: both at the cost of one
__device__ __forceinline__ void philox_normal2(unsigned long long seed, unsigned long long series, unsigned t, unsigned q,
                                               double& z_even, double& z_odd) {
  unsigned c[4] = {(unsigned)series, (unsigned)(series >> 32), t, q};
  philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
  double u1 = ((double)c[0] * 4294967296.0 + (double)c[1] + 1.0) * (1.0 / 18446744073709551616.0);
  double u2 = ((double)c[2] * 4294967296.0 + (double)c[3]) * (1.0 / 18446744073709551616.0);
  double r = sqrt(-2.0 * log(u1));
  double ang = 6.283185307179586476925286766559 * u2;
  z_even = r * cos(ang); z_odd = r * sin(ang);
}

}  // namespace dlm
