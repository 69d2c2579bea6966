// C-ABI implementation (include/dlm_engine.h): argument checking, host<->device staging,
// kernel-variant dispatch, RCCL wrapper.  No torch types, no exceptions across the boundary.
#include "../../include/dlm_engine.h"
#include <cstdlib>
#include "dlm_internal.h"
#include "dlm_draws.h"

#include <rccl/rccl.h>

#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

using dlm::KArgs;

// ---- who asks for LDS (dlm_internal.h: launch).  One book for the process, guarded: an engine is single-threaded, a process may hold several.
namespace dlm {
namespace {
struct LdsEntry {
  size_t granted = 0;     // hipFuncAttributeMaxDynamicSharedMemorySize of this (function, device) so far
  long long whole = -1;   // whole_cu_lds of it (-1: not asked yet)
};
std::mutex lds_mutex;
std::map<std::pair<const void*, int>, LdsEntry> lds_book;   // (kernel, device); (nullptr, device): `granted` holds the device's limit
size_t limit_locked(int dev) {
  LdsEntry& lim = lds_book[{nullptr, dev}];
  if (!lim.granted) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) { (void)hipGetLastError(); v = 0; }
    lim.granted = v > 0 ? (size_t)v : 0;
  }
  return lim.granted;
}
hipError_t opt_in_locked(const void* fn, int dev, size_t bytes) {
  if (bytes > limit_locked(dev)) return hipErrorInvalidValue;
  LdsEntry& en = lds_book[{fn, dev}];
  if (bytes <= en.granted) return hipSuccess;
  const hipError_t err = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (err == hipSuccess) en.granted = bytes;
  return err;
}
}  // namespace
size_t lds_limit() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
  std::lock_guard<std::mutex> lock(lds_mutex);
  return limit_locked(dev);
}
hipError_t lds_opt_in(const void* fn, size_t bytes) {
  int dev = 0;
  const hipError_t err = hipGetDevice(&dev);
  if (err != hipSuccess) return err;
  std::lock_guard<std::mutex> lock(lds_mutex);
  return opt_in_locked(fn, dev, bytes);
}
size_t whole_cu_lds(const void* fn) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
  std::lock_guard<std::mutex> lock(lds_mutex);
  LdsEntry& en = lds_book[{fn, dev}];
  if (en.whole < 0) {
    en.whole = 0;
    hipFuncAttributes at;
    const size_t whole = limit_locked(dev);
    if (hipFuncGetAttributes(&at, fn) != hipSuccess) (void)hipGetLastError();
    else if (at.sharedSizeBytes < whole) {
      if (opt_in_locked(fn, dev, whole - at.sharedSizeBytes) == hipSuccess) en.whole = (long long)(whole - at.sharedSizeBytes);
      else (void)hipGetLastError();
    }
  }
  return (size_t)en.whole;
}
}  // namespace dlm

// A grow-only piece of device memory of the engine.  ensure() (below) is the one place that re-sizes one, dlm_engine_destroy the one
// that frees them: every Ws member joins the engine's list when it is constructed.
struct Workspace {
  void* p = nullptr;
  size_t bytes = 0;
  Workspace* next;
  explicit Workspace(Workspace*& list) : next(list) { list = this; }
};
template <class T>
struct Ws : Workspace {
  using Workspace::Workspace;
  operator T*() const { return (T*)p; }
};

struct dlm_engine {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;
  const char* variant = "none";
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // around the forward and backward kernels
  bool timed = false;
  // The workspaces, who lives in them during ONE call, and the streams that touch them (E: the engine's, C: cov_stream, R: rng_stream).
  // Carves depend on the call's own d, T, N alone; only rtsws means anything to the call after.
  //   arena     E C R  the staged buffers of a DLM_MEM_HOST call (Stager), 256-byte slots
  //   sp_dev    E C    [2 n_g] row table, column table of every G (structured d <= 15 path)
  //   spb_dev   E C    the same for the per-wave / tiled path (d up to 48)
  //   fws       E      filtered records nobody asked for (packed on the structured path) | behind them the workspace of the Q7 log-likelihood
  //   side      E      (e / Q, 1 / Q) per record, forward -> backward pass [N][T+1][2] | behind them CovTabs::eq [N][T+1]; the AR(1) records
  //   xplus     E      x+ of the simulation smoother [N][T+1][d] | the compact means CovTabs::mc of the mean-only kernels
  //   ystar     E      y - y+ of the simulation smoother, innovations of the tiled pass [N][T][p] | behind them the steady-step marks [N][T+1]
  //   covws     E C    one of: the shared-covariance tables (4.9) | the forward covariance table of the shared RTS route | the SVD shared factors (4.10)
  //   route     E C    one byte per series (which kernel serves it) | behind them, 64-byte aligned, KArgs::leave_step [N] (leave_of)
  //   plainbuf  E      KArgs::plain of the call (k_count_gaps): one byte per series
  //   sampws    E C    shared factors of the backward sampler (4.11): table, the zero series' records, flags
  //   zws       E R    the call's normals in the draw kernel's layout
  //   rtsws     E C    shared factors of the RTS smoother (4.13): control words, key and tables of the last call that made them -- kept
  //                    across calls, so nobody else lives here; reused where k_rts_key_check finds the call's key equal to theirs
  //   pgws      E      dlm_pg_batch without its trace outputs: the clouds [launch][T+1][d][P] | behind them the ancestors [launch][T][P] of ONE launch
  //                    (the launches of a call follow one another on the engine's stream)
  //   mixws     E      dlm_gaussian_mixture_summary with more components than a cell holds in LDS: the packed pairs [launch's cells][C][2] of ONE
  //                    launch of the quantile kernel
  Workspace* workspaces = nullptr;   // (in front of the Ws members: they link themselves in)
  Ws<void> arena{workspaces};
  Ws<dlm::SparseT> sp_dev{workspaces};
  Ws<dlm::SparseBig> spb_dev{workspaces};
  Ws<double> fws{workspaces}, side{workspaces}, xplus{workspaces}, ystar{workspaces}, covws{workspaces};
  Ws<unsigned char> route{workspaces}, plainbuf{workspaces};
  Ws<void> sampws{workspaces};
  Ws<double> zws{workspaces};
  Ws<void> rtsws{workspaces};
  Ws<void> pgws{workspaces};
  Ws<double> mixws{workspaces};
  dlm::SparseF* spf_dev = nullptr;     // tables of a structured F (tiled path), allocated once
  int sparse_k = 0;           // 0: some G is not structured (dense MFMA path, regular grids only)
  ncclComm_t comm = nullptr;
  bool has_comm = false;
  std::set<void*> buffers;     // dlm_buffer_alloc allocations still owned by the caller (released at destroy)
  hipEvent_t order_ev = nullptr;   // dlm_engine_wait_stream / dlm_stream_wait_engine
  // The structure analysis of the last call (what analyse_g left behind), reused by DLM_OPT_MODEL_UNCHANGED and -- in host
  // mode, where the tables can be compared -- whenever G and F are bit for bit the same: two stream round trips per call less.
  struct Analysis {
    bool valid = false;
    int d = 0, p = 0, n_g = 0, branch = 0;      // branch: 0 none, 1 structured d <= 15 tables, 2 per-wave / tiled tables
    long long f_stride = 0;
    unsigned generic = 0;
    int sparse_k = 0, spb_k = 0, spf_k = 0;
    bool have_spb = false, have_spf = false;
    std::vector<double> g_host, f_host;         // host-mode calls: the tables analysed
  } an;
  bool an_touched = true;
  bool rts_last = false;        // the last dlm_filter_smooth_batch call went through the tables of rtsws (dlm_last_table_reuse)
  // the auxiliary streams: the one-wave table runs of the shared-covariance / shared-factor paths overlap the
  // batch's forward kernel on cov_stream, the call's normals are made on rng_stream.  cov_ev[0] / the gate of aux_fork: a point of the engine's
  // stream; cov_ev[1] / rng_ev: the stream's tail at its join
  hipStream_t rng_stream = nullptr;
  hipEvent_t rng_ev = nullptr;
  hipStream_t cov_stream = nullptr;
  hipEvent_t cov_ev[2] = {nullptr, nullptr};
  hipEvent_t rng_gate = nullptr;  // 16 <= d <= 48, records-free shared-factor FFBS: the end of the batch's forward pass, behind which the normals start
  hipEvent_t cov_ev2 = nullptr;   // behind the zero series' filter of a shared-factor table (its steady gain and settle step)
  hipEvent_t rts_ev = nullptr;    // behind the shared RTS tables (start_rts_tables): what the backward kernels wait for; the broadcast of S_t runs on behind it
  // work of the CURRENT call is (or may be) in flight on the auxiliary streams and e->stream does not depend on it yet: set by aux_fork,
  // cleared by join_cov / join_rng / drain_all (the rules are written at aux_fork)
  bool cov_busy = false, rng_busy = false;
  // DLM_OPT_COUNT_STEPS: [4] device counters the kernels add to (KArgs::counters), read by dlm_last_counters
  unsigned long long* counters = nullptr;
  // DLM_OPT_MODEL_UNCHANGED is verified on the device: model_sum[0] = checksum of (F, G, g_index, dt) at the last fresh
  // analysis, [1] = scratch; a mismatch raises *model_bad (pinned host memory the kernel writes through model_bad_dev)
  unsigned long long* model_sum = nullptr;
  int* model_bad = nullptr;
  int* model_bad_dev = nullptr;
  bool model_sum_valid = false;
};

namespace {

int fail(dlm_engine* e, int code, const std::string& msg) {
  if (e) e->err = msg;
  return code;
}

// the options of a call: present, and opts->mem one of the two memory spaces
int check_opts(dlm_engine* e, const dlm_options* o) {
  if (!o) return fail(e, DLM_ERR_ARG, "null descriptor");
  if (o->mem != DLM_MEM_DEVICE && o->mem != DLM_MEM_HOST) return fail(e, DLM_ERR_ARG, "opts->mem");
  return DLM_OK;
}
// what the entry points ask of a prior's numbers (a NaN fails both)
bool is_finite(double x) { return x - x == 0.0; }
bool is_positive(double x) { return x > 0.0 && is_finite(x); }
// where the draws of a Gibbs parameter step sit in the Philox counter space
dlm::DrawStream draw_stream(const dlm_options* o, uint64_t iteration) { return dlm::DrawStream{o->seed, o->series_offset, iteration}; }

// the device checksum of a DLM_OPT_MODEL_UNCHANGED call did not match the model the engine analysed: its results are invalid
int promise_broken(dlm_engine* e) {
  *e->model_bad = 0;
  e->an.valid = false;
  return fail(e, DLM_ERR_ARG, "DLM_OPT_MODEL_UNCHANGED was set, but F, G or the time grid differ from the model of the previous call (device checksum): the results of this call are invalid -- drop the flag when the model changes");
}

#define HIP_TRY(e, expr)                                                                    \
  do {                                                                                      \
    hipError_t _err = (expr);                                                               \
    if (_err != hipSuccess)                                                                 \
      return fail((e), DLM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_err));   \
  } while (0)

// ---- the auxiliary streams (cov_stream: tables of the shared-covariance / shared-factor paths, raised priority; rng_stream: the
// normals of a shared-factor call) -- who waits for whom.  Two rules, kept by every entry point:
//   A. when an entry point returns -- success, error or "not eligible after all" -- e->stream depends on everything the call put on
//      the auxiliary streams (join_cov / join_rng where the call wants the result; AuxScope on every other exit path).  A caller that
//      synchronises e->stream (every call without DLM_OPT_ASYNC does, dlm_engine_sync does) has therefore waited for the auxiliary work
//      too, and the next call's work, whose auxiliary launches wait for an event recorded on e->stream, is ordered behind it.
//   B. before a workspace any of the three streams may touch is freed or resized (ensure), before the engine moves to another stream
//      and before it is destroyed, all three streams are drained on the host (drain_all).
// (Round 3 kept neither on its error paths: a return between start_sampler_tables and the hipStreamWaitEvent of the draw left kernels
// on cov_stream / rng_stream reading the staging arena and e->sampws with nothing ordered behind them, the workspace re-size paths
// synchronised e->stream alone, and dlm_engine_destroy freed buffers and destroyed streams with auxiliary work possibly in flight.)
// Fork: what e->stream holds up to `at` is visible to the auxiliary stream, which is busy from here on (every exit path joins it).
// record = false: the caller recorded `at` on e->stream already (the gates of start_sampler_normals).
int aux_fork(dlm_engine* e, hipStream_t aux, bool& busy, hipEvent_t at, bool record = true) {
  if (record) HIP_TRY(e, hipEventRecord(at, e->stream));
  busy = true;
  HIP_TRY(e, hipStreamWaitEvent(aux, at, 0));
  return DLM_OK;
}
// Join: e->stream waits for everything queued on the auxiliary stream so far.  Nothing to do when the call put nothing there.
int aux_join_one(dlm_engine* e, hipStream_t aux, bool& busy, hipEvent_t tail) {
  if (!busy) return DLM_OK;
  busy = false;   // (cleared first: a failing HIP call must not make every later exit path fail again)
  HIP_TRY(e, hipEventRecord(tail, aux));
  HIP_TRY(e, hipStreamWaitEvent(e->stream, tail, 0));
  return DLM_OK;
}
int join_cov(dlm_engine* e) { return aux_join_one(e, e->cov_stream, e->cov_busy, e->cov_ev[1]); }
int join_rng(dlm_engine* e) { return aux_join_one(e, e->rng_stream, e->rng_busy, e->rng_ev); }
int aux_join(dlm_engine* e) {
  const int rc = join_cov(e);
  return rc ? rc : join_rng(e);
}
int drain_all(dlm_engine* e) {
  e->cov_busy = e->rng_busy = false;
  if (e->cov_stream) HIP_TRY(e, hipStreamSynchronize(e->cov_stream));
  if (e->rng_stream) HIP_TRY(e, hipStreamSynchronize(e->rng_stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return DLM_OK;
}
struct AuxScope {   // rule A on every exit path of an entry point that may use the auxiliary streams
  dlm_engine* e;
  explicit AuxScope(dlm_engine* e_) : e(e_) {}
  ~AuxScope() { if (e && (e->cov_busy || e->rng_busy)) (void)aux_join(e); }
};
// Rule B in one place: `w` holds at least `need` bytes afterwards.  Grow-only; growing drains the three streams, frees, allocates anew
// (the contents are gone: *fresh tells a caller that cares); a first allocation drains nothing; a failed hipMalloc leaves `w` empty.
int ensure(dlm_engine* e, Workspace& w, size_t need, bool* fresh = nullptr) {
  if (fresh) *fresh = false;
  if (need <= w.bytes) return DLM_OK;
  if (w.p) {
    const int rc = drain_all(e);
    if (rc) return rc;
    HIP_TRY(e, hipFree(w.p));
    w.p = nullptr;
    w.bytes = 0;
  }
  HIP_TRY(e, hipMalloc(&w.p, need));
  w.bytes = need;
  if (fresh) *fresh = true;
  return DLM_OK;
}

// Collects the buffers of one call.  Device mode: pointers pass through.  Host mode: every
// buffer gets a slot in the engine's arena; inputs are copied up before the launch, outputs
// are copied back by finish().
class Stager {
 public:
  Stager(dlm_engine* e, bool host) : e_(e), host_(host) {}

  template <class T>
  void in(const T** field, const T* p, size_t count) { add((void**)field, (void*)p, count * sizeof(T), true, false); }
  template <class T>
  void out(T** field, T* p, size_t count) { add((void**)field, (void*)p, count * sizeof(T), false, true); }
  template <class T>
  void zeroed_out(T** field, T* p, size_t count) { add((void**)field, (void*)p, count * sizeof(T), false, true, true); }
  template <class T>
  void inout(T** field, T* p, size_t count) { add((void**)field, (void*)p, count * sizeof(T), true, true); }

  int commit() {
    if (host_) {
      size_t need = 0;
      for (auto& b : bufs_) if (b.user) { b.offset = need; need += (b.bytes + 255) & ~(size_t)255; }
      const int rc = ensure(e_, e_->arena, need);
      if (rc) return rc;
    }
    for (auto& b : bufs_) {
      if (!b.user) { *b.field = nullptr; continue; }
      void* dev = host_ ? (void*)((char*)e_->arena.p + b.offset) : b.user;
      b.dev = dev;
      *b.field = dev;
      if (host_ && b.is_in) HIP_TRY(e_, hipMemcpyAsync(dev, b.user, b.bytes, hipMemcpyHostToDevice, e_->stream));
      if (b.zero) HIP_TRY(e_, hipMemsetAsync(dev, 0, b.bytes, e_->stream));
    }
    return DLM_OK;
  }

  int finish(bool async) {
    if (host_) {
      for (auto& b : bufs_)
        if (b.user && b.is_out) HIP_TRY(e_, hipMemcpyAsync(b.user, b.dev, b.bytes, hipMemcpyDeviceToHost, e_->stream));
      HIP_TRY(e_, hipStreamSynchronize(e_->stream));
    } else if (!async) {
      HIP_TRY(e_, hipStreamSynchronize(e_->stream));
    }
    if ((host_ || !async) && e_->model_bad && *e_->model_bad) return promise_broken(e_);
    return DLM_OK;
  }

 private:
  struct Buf { void** field; void* user; size_t bytes; bool is_in, is_out, zero; size_t offset; void* dev; };
  void add(void** field, void* p, size_t bytes, bool is_in, bool is_out, bool zero = false) {
    bufs_.push_back(Buf{field, p, bytes, is_in, is_out, zero, 0, nullptr});
  }
  dlm_engine* e_;
  bool host_;
  std::vector<Buf> bufs_;
};

int check_common(dlm_engine* e, const dlm_model_desc* m, const dlm_params_desc* p, const dlm_options* o) {
  if (!e) return DLM_ERR_ARG;
  if (!e->an_touched) e->an.valid = false;   // the call before this one took a model but did not analyse it: DLM_OPT_MODEL_UNCHANGED speaks of ITS model
  e->an_touched = false;
  if (!m || !p || !o) return fail(e, DLM_ERR_ARG, "null descriptor");
  if (m->d < 1 || m->p < 1 || m->T < 1 || m->N < 1) return fail(e, DLM_ERR_ARG, "d, p, T, N must be >= 1 (the reference throws on empty input, KalmanFilter.scala:116-117)");
  if (!m->F || !m->G || m->n_g < 1) return fail(e, DLM_ERR_ARG, "model tables F/G missing");
  if (m->n_g > 1 && !m->g_index) return fail(e, DLM_ERR_ARG, "n_g > 1 needs g_index");
  if (m->f_stride != 0 && m->f_stride != (int64_t)m->d * m->p) return fail(e, DLM_ERR_ARG, "f_stride must be 0 or d*p");
  if (!p->V || !p->W || !p->m0 || !p->C0) return fail(e, DLM_ERR_ARG, "parameter arrays missing");
  if ((p->v_tstride != 0 && p->v_tstride != (int64_t)m->p * m->p) || (p->w_tstride != 0 && p->w_tstride != (int64_t)m->d * m->d))
    return fail(e, DLM_ERR_ARG, "v_tstride must be 0 or p*p, w_tstride 0 or d*d");
  if (o->mem != DLM_MEM_DEVICE && o->mem != DLM_MEM_HOST) return fail(e, DLM_ERR_ARG, "opts->mem");
  if (m->d > 64 || m->p > 64) return fail(e, DLM_ERR_UNSUPPORTED, "d and p are limited to 64 in this build (and by the LDS of one CU on the general kernels: see the entry point's message)");
  HIP_TRY(e, hipSetDevice(e->device));
  return DLM_OK;
}

// DLM_OPT_COUNT_STEPS: the kernels of this call count their short steps into the engine's counters
int want_counters(dlm_engine* e, KArgs& k) {
  k.counters = nullptr;
  if (!(k.flags & DLM_OPT_COUNT_STEPS)) return DLM_OK;
  if (!e->counters) HIP_TRY(e, hipMalloc((void**)&e->counters, 4 * sizeof(unsigned long long)));
  HIP_TRY(e, hipMemsetAsync(e->counters, 0, 4 * sizeof(unsigned long long), e->stream));
  k.counters = e->counters;
  return DLM_OK;
}

// model + params -> staged KArgs fields
void stage_model(Stager& st, KArgs& k, const dlm_model_desc* m, const dlm_params_desc* p, const dlm_options* o) {
  const size_t d = m->d, pp = m->p, T = m->T, N = m->N;
  k.d = m->d; k.p = m->p; k.T = m->T; k.N = m->N; k.n_g = m->n_g;
  k.f_stride = m->f_stride; k.v_stride = p->v_stride; k.w_stride = p->w_stride;
  k.v_tstride = p->v_tstride; k.w_tstride = p->w_tstride;
  k.m0_stride = p->m0_stride; k.c0_stride = p->c0_stride;
  k.flags = o->flags; k.seed = o->seed; k.series_offset = o->series_offset;
  st.in(&k.F, m->F, (m->f_stride ? T : 1) * d * pp);
  st.in(&k.G, m->G, (size_t)m->n_g * d * d);
  st.in(&k.g_index, (const int*)m->g_index, m->g_index ? T : 0);
  st.in(&k.dt, m->dt, m->dt ? T : 0);
  const size_t vblk = p->v_tstride ? (T - 1) * (size_t)p->v_tstride + pp * pp : pp * pp;   // one series' V (or V_0 .. V_{T-1})
  const size_t wblk = p->w_tstride ? (T - 1) * (size_t)p->w_tstride + d * d : d * d;
  st.in(&k.V, p->V, p->v_stride ? (N - 1) * (size_t)p->v_stride + vblk : vblk);
  st.in(&k.W, p->W, p->w_stride ? (N - 1) * (size_t)p->w_stride + wblk : wblk);
  st.in(&k.m0, p->m0, p->m0_stride ? (N - 1) * (size_t)p->m0_stride + d : d);
  st.in(&k.C0, p->C0, p->c0_stride ? (N - 1) * (size_t)p->c0_stride + d * d : d * d);
}

bool fast_shape_ok(const KArgs& k) { return !(k.flags & DLM_OPT_FORCE_GENERIC) && dlm::fast_shape(k); }
// d <= 15, p = 1 fast path: the structured kernels take any time grid, the dense-G MFMA kernels a regular one
bool use_fast(const dlm_engine* e, const KArgs& k) { return fast_shape_ok(k) && (e->sparse_k > 0 || dlm::mfma16_supported(k)); }
// d <= 5, p = 1: one lane per series (DLM_OPT_NO_LANE: A/B measurements)
bool use_lane(const KArgs& k) { return !(k.flags & (DLM_OPT_FORCE_GENERIC | DLM_OPT_NO_LANE)) && dlm::lane_supported(k); }
// the d >= 16 kernels, or -- d <= 15 with several observation components and a structured G -- the per-wave kernels
bool use_tiled(const KArgs& k) { return !(k.flags & DLM_OPT_FORCE_GENERIC) && (dlm::tiled_supported(k) || dlm::wave48_small_ok(k)); }
bool tiled_analysis_wanted(const KArgs& k) { return !(k.flags & DLM_OPT_FORCE_GENERIC) && (dlm::tiled_supported(k) || dlm::wave48_small_shape(k)); }

// Inspect every G of the table (fast-path shapes only) and upload the sparse tables when all of them are
// structured.  `G_user` is the caller's pointer (host or device according to host_mode).
int analyse_g_tiled(dlm_engine* e, KArgs& k, const double* G_user, bool host_mode) {
  const size_t dd = (size_t)k.d * k.d, ng = (size_t)k.n_g;
  std::vector<double> g(dd * ng);
  if (host_mode) memcpy(g.data(), G_user, g.size() * sizeof(double));
  else {
    HIP_TRY(e, hipMemcpyAsync(g.data(), G_user, g.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
  }
  std::vector<dlm::SparseBig> tabs(2 * ng);
  for (size_t q = 0; q < ng; ++q)
    if (dlm::sparse48_analyse(g.data() + q * dd, k.d, &tabs[2 * q], &tabs[2 * q + 1]) > 4) return DLM_OK;   // dense G
  int K = 1;
  for (auto& t : tabs) K = t.K > K ? t.K : K;
  for (auto& t : tabs) t.K = K;
  { const int rc = ensure(e, e->spb_dev, tabs.size() * sizeof(dlm::SparseBig)); if (rc) return rc; }
  HIP_TRY(e, hipMemcpyAsync(e->spb_dev, tabs.data(), tabs.size() * sizeof(dlm::SparseBig), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));  // tabs lives on this stack frame
  k.spb = e->spb_dev;
  k.spb_k = K;
  k.spf = nullptr;
  if (!k.f_stride) {   // a time-invariant F: its few nonzeros per column / row turn the products with F into gathers
    std::vector<double> f((size_t)k.d * k.p);
    HIP_TRY(e, hipMemcpyAsync(f.data(), k.F, f.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    dlm::SparseF tf;
    const int kf = dlm::sparsef_analyse(f.data(), k.d, k.p, &tf);
    if (kf <= 4) {
      if (!e->spf_dev) HIP_TRY(e, hipMalloc((void**)&e->spf_dev, sizeof(dlm::SparseF)));
      HIP_TRY(e, hipMemcpyAsync(e->spf_dev, &tf, sizeof(tf), hipMemcpyHostToDevice, e->stream));
      HIP_TRY(e, hipStreamSynchronize(e->stream));
      k.spf = e->spf_dev; k.spf_k = kf;
    }
  }
  return DLM_OK;
}

int analyse_g_fresh(dlm_engine* e, KArgs& k, const double* G_user, bool host_mode);

// 64-bit checksum of the model tables (F, G, g_index, dt) of a device-memory call: one 256-thread block, every 64-bit word
// mixed with its position (splitmix64 finaliser) and summed.  store != 0: remember it (fresh analysis); store == 0: compare with
// the remembered one and raise *bad (pinned host memory) on a mismatch -- the check behind DLM_OPT_MODEL_UNCHANGED.
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull; x ^= x >> 27; x *= 0x94d049bb133111ebull; x ^= x >> 31;
  return x;
}
__global__ __launch_bounds__(256) void k_model_checksum(const double* F, long long nF, const double* G, long long nG, const int* gi,
                                                        const double* dt, long long T, unsigned long long* sums, int store, int* bad) {
  __shared__ unsigned long long part[256];
  unsigned long long acc = 0;
  const unsigned long long* f = (const unsigned long long*)F;
  const unsigned long long* g = (const unsigned long long*)G;
  const unsigned long long* q = (const unsigned long long*)dt;
  for (long long i = threadIdx.x; i < nF; i += 256) acc += mix64(f[i] + 0x9e3779b97f4a7c15ull * (unsigned long long)(i + 1));
  for (long long i = threadIdx.x; i < nG; i += 256) acc += mix64(g[i] + 0xc2b2ae3d27d4eb4full * (unsigned long long)(i + 1));
  if (gi) for (long long i = threadIdx.x; i < T; i += 256) acc += mix64((unsigned long long)(unsigned)gi[i] + 0x165667b19e3779f9ull * (unsigned long long)(i + 1));
  if (dt) for (long long i = threadIdx.x; i < T; i += 256) acc += mix64(q[i] + 0x27d4eb2f165667c5ull * (unsigned long long)(i + 1));
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) {
    const unsigned long long v = part[0] + mix64((unsigned long long)nF) + mix64((unsigned long long)nG * 3 + (gi ? 1 : 0) + (dt ? 2 : 0)) + mix64((unsigned long long)T * 7);
    if (store) sums[0] = v;
    else if (sums[0] != v) { __threadfence_system(); *bad = 1; }
  }
}
int model_checksum(dlm_engine* e, const KArgs& k, bool store) {
  if (!e->model_sum) {
    HIP_TRY(e, hipMalloc((void**)&e->model_sum, 2 * sizeof(unsigned long long)));
    HIP_TRY(e, hipHostMalloc((void**)&e->model_bad, sizeof(int), hipHostMallocMapped));
    *e->model_bad = 0;
    HIP_TRY(e, hipHostGetDevicePointer((void**)&e->model_bad_dev, e->model_bad, 0));
  }
  const long long nF = (long long)(k.f_stride ? k.T : 1) * k.d * k.p, nG = (long long)k.n_g * k.d * k.d;
  HIP_TRY(e, dlm::launch(k_model_checksum, dim3(1), dim3(256), 0, e->stream, k.F, nF, k.G, nG, k.g_index, k.dt, (long long)k.T,
                         e->model_sum, store ? 1 : 0, e->model_bad_dev));
  return DLM_OK;
}

// analyse_g with the cache of the last call's result in front of it
int analyse_g(dlm_engine* e, KArgs& k, const double* G_user, bool host_mode) {
  dlm_engine::Analysis& an = e->an;
  e->an_touched = true;
  { const int rcc = want_counters(e, k); if (rcc) return rcc; }   // (every kernel-launching entry point of the filter family passes through here)
  const int branch = tiled_analysis_wanted(k) ? 2 : (fast_shape_ok(k) ? 1 : 0);
  const unsigned generic = k.flags & DLM_OPT_FORCE_GENERIC;
  bool same = an.valid && an.d == k.d && an.p == k.p && an.n_g == k.n_g && an.branch == branch && an.f_stride == k.f_stride &&
              an.generic == generic;
  const size_t gn = (size_t)k.d * k.d * (size_t)k.n_g, fn = (size_t)k.d * k.p;
  if (same && host_mode) {   // host pointers: compare the tables themselves (the caller's F is staged by now: compare the user's copy of G and our copy of F's source)
    same = an.g_host.size() == gn && memcmp(an.g_host.data(), G_user, gn * sizeof(double)) == 0;
    if (same && branch == 2 && !k.f_stride) same = false;   // (F of a host-mode call is only known staged: analysed afresh, it is one small copy)
  } else if (same) {
    same = (k.flags & DLM_OPT_MODEL_UNCHANGED) != 0 && e->model_sum_valid;
    // the promise is verified on the device (no host round trip: a mismatch surfaces when the call synchronises)
    if (same && !(k.flags & DLM_OPT_TRUST_MODEL_UNCHANGED)) { const int rc = model_checksum(e, k, false); if (rc) return rc; }
  }
  if (same) {
    e->sparse_k = an.sparse_k;
    k.spb = an.have_spb ? e->spb_dev : nullptr;
    k.spb_k = an.spb_k;
    k.spf = an.have_spf ? e->spf_dev : nullptr;
    k.spf_k = an.spf_k;
    return DLM_OK;
  }
  an.valid = false;
  const int rc = analyse_g_fresh(e, k, G_user, host_mode);
  if (rc) return rc;
  an.valid = true; an.d = k.d; an.p = k.p; an.n_g = k.n_g; an.branch = branch; an.f_stride = k.f_stride; an.generic = generic;
  an.sparse_k = e->sparse_k; an.spb_k = k.spb_k; an.spf_k = k.spf_k; an.have_spb = k.spb != nullptr; an.have_spf = k.spf != nullptr;
  an.g_host.clear();
  if (host_mode) an.g_host.assign(G_user, G_user + gn);
  (void)fn;
  e->model_sum_valid = false;
  if (!host_mode) { const int rc2 = model_checksum(e, k, true); if (rc2) return rc2; e->model_sum_valid = true; }   // what a later DLM_OPT_MODEL_UNCHANGED call is checked against
  return DLM_OK;
}

int analyse_g_fresh(dlm_engine* e, KArgs& k, const double* G_user, bool host_mode) {
  e->sparse_k = 0;
  k.spb = nullptr;
  if (tiled_analysis_wanted(k)) return analyse_g_tiled(e, k, G_user, host_mode);
  if (!fast_shape_ok(k)) return DLM_OK;
  const size_t dd = (size_t)k.d * k.d, ng = (size_t)k.n_g;
  std::vector<double> g(dd * ng);
  if (host_mode) memcpy(g.data(), G_user, g.size() * sizeof(double));
  else {
    HIP_TRY(e, hipMemcpyAsync(g.data(), G_user, g.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
  }
  std::vector<dlm::SparseT> tabs(2 * ng);
  int K = 1;
  for (size_t q = 0; q < ng; ++q) {
    const int kq = dlm::sparse16_analyse(g.data() + q * dd, k.d, &tabs[2 * q], &tabs[2 * q + 1]);
    if (kq > 4) return DLM_OK;
    K = kq > K ? kq : K;
  }
  { const int rc = ensure(e, e->sp_dev, tabs.size() * sizeof(dlm::SparseT)); if (rc) return rc; }
  HIP_TRY(e, hipMemcpyAsync(e->sp_dev, tabs.data(), tabs.size() * sizeof(dlm::SparseT), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));  // tabs lives on this stack frame
  e->sparse_k = K;
  return DLM_OK;
}

// HIP events around the forward (0 -> 1) and backward (1 -> 2) part of a call, read back by dlm_last_timing
int mark(dlm_engine* e, int i) {
  HIP_TRY(e, hipEventRecord(e->ev[i], e->stream));
  if (i == 2) e->timed = true;
  return DLM_OK;
}

// (e / Q, 1 / Q) per record for the per-series kernels, and behind them one double per record (e / Q) for the shared-covariance kernels
int ensure_side(dlm_engine* e, size_t N, size_t T) { return ensure(e, e->side, sizeof(double) * 3 * N * (T + 1)); }

int ensure_xplus(dlm_engine* e, const KArgs& k) { return ensure(e, e->xplus, sizeof(double) * (size_t)k.N * ((size_t)k.T + 1) * (size_t)k.d); }

int ensure_ystar(dlm_engine* e, const KArgs& k) {
  // innovations [N][T][p], then one byte per record [N][T+1]: the marks "C_t is C_{t-1}" of the per-wave forward kernel's steady steps
  return ensure(e, e->ystar, sizeof(double) * (size_t)k.N * (size_t)k.T * (size_t)k.p + (((size_t)k.N * (size_t)(k.T + 1) + 15) & ~(size_t)15));
}

// DLM_OPT_PACKED_SYM is served by the structured d <= 15, p = 1 kernels (the lane kernels step aside for it)
int packed_path(dlm_engine* e, KArgs& k) {
  k.flags |= DLM_OPT_NO_LANE;
  if (!(fast_shape_ok(k) && e->sparse_k > 0) || (k.flags & DLM_OPT_SMOOTHER_COMPAT_Q1))
    return fail(e, DLM_ERR_UNSUPPORTED, "DLM_OPT_PACKED_SYM needs the structured d <= 15, p = 1 path (time-invariant F, <= 4 nonzeros per row and column of G) without DLM_OPT_FORCE_GENERIC / DLM_OPT_SMOOTHER_COMPAT_Q1; use dense records otherwise");
  return DLM_OK;
}

// Shared covariance sequence (dlm_sparse16.hip): structured d <= 15, p = 1 path on a regular grid with V, W, C0
// shared by the batch.  One wave runs the covariance recursions into tables, every series its mean recursions against them; a
// series with a missing observation is marked by the forward mean kernel and served by the per-series kernels launched behind.
bool use_shared_cov(const dlm_engine* e, const KArgs& k) {
  return fast_shape_ok(k) && e->sparse_k > 0 && !dlm::lane_supported(k) && dlm::shared_cov_eligible(k);
}
// route: one byte per series; behind it (64-byte aligned) one int per series, the step a series left the per-wave filter at (KArgs::leave_step)
size_t route_pad(size_t N) { return (N + 63) & ~(size_t)63; }
int ensure_route(dlm_engine* e, size_t N) { return ensure(e, e->route, route_pad(N) + N * sizeof(int)); }
int* leave_of(dlm_engine* e, size_t N) { return (int*)(e->route + route_pad(N)); }   // (N: the call's, as in its ensure_route)
// Structured d <= 15 path on a regular grid: the series that miss more than T / 256 of their observations are marked (from the data
// alone: the choice does not depend on the batch) and take every step in full -- the forward kernel without its convergence test, the
// backward kernel in the instantiation without the shortcut's machinery.  With gaps nothing settles, and the machinery only costs.
int mark_plain(dlm_engine* e, KArgs& k) {
  k.plain = nullptr;
  if (!(fast_shape_ok(k) && e->sparse_k > 0) || use_lane(k) || !k.y || k.g_index || k.dt || k.f_stride || k.v_tstride || k.w_tstride ||
      (k.flags & DLM_OPT_NO_STEADY)) return DLM_OK;
  { const int rc = ensure(e, e->plainbuf, (size_t)k.N); if (rc) return rc; }
  HIP_TRY(e, dlm::launch_sparse16_count_gaps(k, e->plainbuf, e->stream));
  k.plain = e->plainbuf;
  return DLM_OK;
}
int ensure_cov_stream(dlm_engine* e) {
  if (!e->cov_stream) {
    int lo = 0, hi = 0;   // the few waves of the table kernels go first: they run beside a kernel that fills the device
    HIP_TRY(e, hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIP_TRY(e, hipStreamCreateWithPriority(&e->cov_stream, hipStreamNonBlocking, hi));
    for (auto& ev : e->cov_ev) HIP_TRY(e, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIP_TRY(e, hipEventCreateWithFlags(&e->cov_ev2, hipEventDisableTiming));
    HIP_TRY(e, hipEventCreateWithFlags(&e->rts_ev, hipEventDisableTiming));
  }
  return DLM_OK;
}
// Shared factors of the reference-form backward sampler (dlm_sampler16.hip): the tables are made on the second
// stream -- a filter and a sampler run of ONE wave on a series of zeros -- while the batch is filtered on the first.
int start_sampler_normals(dlm_engine* e, const KArgs& k, dlm::SampTabs& tb, bool big, hipEvent_t gate);
int start_sampler_tables(dlm_engine* e, const KArgs& k, dlm::SampTabs& tb, bool big, const double* crec = nullptr, int crec_stride = 0, bool defer_normals = false) {
  int rc = ensure(e, e->sampws, big ? dlm::wave48_sampler_shared_ws_bytes(k) : dlm::sampler_shared_ws_bytes(k));
  if (rc || (rc = ensure_route(e, (size_t)k.N)) || (rc = ensure_cov_stream(e))) return rc;
  if (big) dlm::wave48_sampler_shared_carve(e->sampws, k, tb); else dlm::sampler_shared_carve(e->sampws, k, tb);
  if ((rc = aux_fork(e, e->cov_stream, e->cov_busy, e->cov_ev[0]))) return rc;   // the model and the tables of G are staged
  tb.zstride = 0; tb.mc4 = nullptr; tb.marked = 0;
  if (big) HIP_TRY(e, dlm::launch_wave48_sampler_shared_tables(k, tb, e->cov_stream, e->cov_ev2));
  else if (crec) HIP_TRY(e, dlm::launch_sampler_shared_tables_from(k, e->sparse_k, e->sp_dev, tb, crec, crec_stride, e->cov_stream));   // the covariances exist already
  else HIP_TRY(e, dlm::launch_sampler_shared_tables(k, e->sparse_k, e->sp_dev, tb, e->cov_stream));
  tb.z4 = nullptr;
  if (defer_normals) return DLM_OK;   // (start_sampler_normals, behind the forward pass's launch)
  return start_sampler_normals(e, k, tb, big, e->cov_ev[0]);
}
// The normals of the call (third stream).  `gate`: an event of the engine's stream the launch waits for -- the staging of the call (the draw kernel of the
// call before has read its normals) or, 16 <= d <= 48, the END of the batch's forward pass: k_filter_w48 is one wave per SIMD and launched behind a
// kernel of forty million threads it started 0.4 ms late (the normals are wanted last, by the draw kernel; they now run beside k_steady_filter_w48).
int start_sampler_normals(dlm_engine* e, const KArgs& k, dlm::SampTabs& tb, bool big, hipEvent_t gate) {
  if (!k.z) {
    int rc = ensure(e, e->zws, big ? dlm::wave48_sampler_shared_normals_bytes(k) : dlm::sampler_shared_normals_bytes(k));
    if (rc) return rc;
    if (!e->rng_stream) {
      HIP_TRY(e, hipStreamCreateWithFlags(&e->rng_stream, hipStreamNonBlocking));
      HIP_TRY(e, hipEventCreateWithFlags(&e->rng_ev, hipEventDisableTiming));
    }
    if ((rc = aux_fork(e, e->rng_stream, e->rng_busy, gate, false))) return rc;
    if (big) HIP_TRY(e, dlm::launch_wave48_sampler_shared_normals(k, e->zws, e->rng_stream));
    else HIP_TRY(e, dlm::launch_sampler_shared_normals(k, e->zws, e->rng_stream));
    tb.z4 = e->zws;
  }
  return DLM_OK;
}
// Shared factors of the RTS smoother (dlm_sampler16.hip): the tables are made on the second stream -- a filter and a smoother run of ONE wave
// on a series of zeros -- while the batch is filtered on the first.  They live in a workspace of their own (e->rtsws) and stay there: a call
// whose key equals theirs (k_rts_key_check, on the device: the host does not know hit from miss and queues the same launches either way) finds
// the two one-wave kernels returning at once.  A re-size frees the old tables with the workspace; the new one starts invalid.
int start_rts_tables(dlm_engine* e, const KArgs& k, dlm::RtsTabs& tb) {
  bool fresh = false;
  int rc = ensure(e, e->rtsws, dlm::rts_shared_ws_bytes(k), &fresh);
  if (rc) return rc;
  if (fresh) HIP_TRY(e, hipMemsetAsync(e->rtsws, 0, 64, e->stream));   // the control words: no valid tables
  if ((rc = ensure(e, e->covws, sizeof(double) * dlm::covtabs_doubles(k.d, k.T)))) return rc;   // the forward covariance table of the shared-covariance kernels
  if ((rc = ensure_route(e, (size_t)k.N)) || (rc = ensure_cov_stream(e))) return rc;
  dlm::RtsKeep keep{};
  dlm::rts_shared_carve(e->rtsws, k, tb, keep);
  dlm::CovTabs ctb{};
  dlm::covtabs_carve(e->covws, k.d, k.T, ctb);
  const bool no_reuse = (k.flags & DLM_OPT_NO_TABLE_REUSE) != 0;
  const int* gate = keep.ctl + dlm::RTS_CTL_GATE;
  e->rts_last = true;
  HIP_TRY(e, dlm::launch_rts_shared_mark(k, e->route, tb, e->stream));                     // the series with a gap; where they are the majority, no tables (tb.skip)
  HIP_TRY(e, dlm::launch_rts_key_check(k, e->sparse_k, e->sp_dev, keep, no_reuse, e->stream));   // hit or miss; a miss marks the kept tables invalid before the kernels below overwrite them
  HIP_TRY(e, dlm::launch_rts_shared_cov(k, e->sparse_k, e->sp_dev, tb, ctb, gate, e->stream));   // the forward covariances: in front of the batch's forward pass
  if ((rc = aux_fork(e, e->cov_stream, e->cov_busy, e->cov_ev[0]))) return rc;
  HIP_TRY(e, dlm::launch_rts_shared_tables(k, e->sparse_k, e->sp_dev, tb, gate, e->cov_stream));   // J_t, S_t: beside it
  // The table run keeps a whole CU to itself (whole_cu_lds): it has to be resident before the forward pass fills every CU with its
  // workgroups, or it waits for that kernel's last wave.  The caller launches the gap count of the forward pass (mark_plain: a 30 us kernel)
  // in between on the engine's stream.
  // Behind a table run that ran: its key and "valid".  An error exit from here on leaves a complete set (every exit path joins the stream),
  // one before it leaves the set invalid.
  HIP_TRY(e, dlm::launch_rts_key_commit(k, e->sparse_k, e->sp_dev, keep, no_reuse, e->cov_stream));
  // The tables stand: the backward kernels of the call wait for this point, not for the end of the stream.  Behind it S_t goes into the smoothed
  // records of the series the tables serve (k_rts_broadcast) -- on a hit the two one-wave kernels above return at once and it runs beside the
  // forward pass, on a miss beside the backward kernels.  The call joins the stream behind those (every other exit path: AuxScope).
  HIP_TRY(e, hipEventRecord(e->rts_ev, e->cov_stream));
  HIP_TRY(e, dlm::launch_rts_broadcast(k, e->route, tb, e->cov_stream));
  return DLM_OK;
}
int ensure_shared(dlm_engine* e, const KArgs& k, dlm::CovTabs& tb, bool with_backward) {
  int rc = ensure(e, e->covws, sizeof(double) * dlm::covtabs_doubles(k.d, k.T));
  if (rc || (rc = ensure_route(e, (size_t)k.N)) || (rc = ensure_side(e, k.N, k.T)) || (rc = ensure_cov_stream(e))) return rc;
  dlm::covtabs_carve(e->covws, k.d, k.T, tb);
  tb.eq = e->side + 2 * (size_t)k.N * ((size_t)k.T + 1);
  tb.mc = tb.sc = nullptr;
  if (with_backward) {   // compact means of the mean-only kernels: 512 bytes per step and group of four series, filtered then smoothed
    const size_t one = 64 * (size_t)((k.N + 3) / 4) * ((size_t)k.T + 1);
    if ((rc = ensure(e, e->xplus, sizeof(double) * one))) return rc;
    tb.mc = e->xplus;
  }
  return DLM_OK;
}
// forward half: covariance-only run, mean kernel, then the per-series kernel for the series the mean kernel routed away.
// with_backward: the backward covariance run starts on the engine's second stream as soon as the forward tables exist and
// overlaps the forward mean kernel (it needs nothing from the data).
int run_shared_filter(dlm_engine* e, KArgs& k, dlm::CovTabs& tb, bool with_backward) {
  int rc = ensure_shared(e, k, tb, with_backward);
  if (rc) return rc;
  k.route = e->route; k.route_take = 0;
  e->variant = "sparse16";   // (the same kernel family; dlm_last_counters[2] tells the series served by the shared-covariance kernels)
  HIP_TRY(e, dlm::launch_sparse16_cov_filter(k, e->sparse_k, e->sp_dev, tb, e->stream));
  if (with_backward) {
    if ((rc = aux_fork(e, e->cov_stream, e->cov_busy, e->cov_ev[0]))) return rc;
    HIP_TRY(e, dlm::launch_sparse16_cov_smoother(k, e->sparse_k, e->sp_dev, tb, e->cov_stream));
  }
  HIP_TRY(e, dlm::launch_sparse16_mean_filter(k, e->sparse_k, e->sp_dev, tb, e->stream));
  KArgs kg = k;
  kg.route_take = 1;
  HIP_TRY(e, dlm::launch_sparse16_filter(kg, e->sparse_k, e->sp_dev, with_backward ? e->side : nullptr, nullptr, e->stream));
  return DLM_OK;
}
int run_shared_smoother(dlm_engine* e, KArgs& k, const dlm::CovTabs& tb) {
  { const int rc = join_cov(e); if (rc) return rc; }   // the S_t table
  HIP_TRY(e, dlm::launch_sparse16_mean_smoother(k, e->sparse_k, e->sp_dev, tb, e->stream));
  KArgs kg = k;
  kg.route_take = 1;
  HIP_TRY(e, dlm::launch_sparse16_smoother(kg, e->sparse_k, e->sp_dev, e->side, e->stream));
  return DLM_OK;
}

// want_side: the caller will run the fast backward pass on this filter's output
int run_filter(dlm_engine* e, const KArgs& k, bool want_side) {
  if (use_lane(k)) {
    e->variant = "lane";
    HIP_TRY(e, dlm::launch_lane_filter(k, e->stream));
  } else if (use_fast(e, k) && (!k.prior || e->sparse_k)) {   // the dense-G MFMA kernel does not write (a, R) records
    if (want_side) { int rc = ensure_side(e, k.N, k.T); if (rc) return rc; }
    double* side = want_side ? e->side : nullptr;
    if (e->sparse_k) {
      e->variant = "sparse16";
      HIP_TRY(e, dlm::launch_sparse16_filter(k, e->sparse_k, e->sp_dev, side, nullptr, e->stream));
    } else {
      e->variant = "mfma16";
      HIP_TRY(e, dlm::launch_mfma16_filter(k, side, e->stream));
    }
  } else if (use_tiled(k)) {
    e->variant = dlm::wave48_filter_supported(k) ? "wave-mfma" : "tiled-mfma";
    if (want_side) { int rc = ensure_ystar(e, k); if (rc) return rc; }
    HIP_TRY(e, dlm::launch_tiled_filter(k, want_side ? e->ystar : nullptr, e->stream));
  } else {
    e->variant = "generic";
    if (dlm::generic_filter_lds_bytes(k.d, k.p) > dlm::lds_limit())   // 3 d + 4 d^2 + 2 d p + 2 p^2 + 3 p doubles of one CU's 160 KB of LDS
      return fail(e, DLM_ERR_UNSUPPORTED, "the general filter kernel keeps a series' matrices in the LDS of one CU: this d, p needs more than its 160 KB (d = 64 fits with p <= 12, p = 64 with d <= 26)");
    HIP_TRY(e, dlm::launch_generic_filter(k, e->stream));
  }
  return DLM_OK;
}

bool fast_smoother_ok(const dlm_engine* e, const KArgs& k) { return use_fast(e, k) && !(k.flags & DLM_OPT_SMOOTHER_COMPAT_Q1); }

// have_side: the preceding run_filter(.., want_side = true) of THIS call filled e->side
int run_smoother(dlm_engine* e, const KArgs& k, bool have_side) {
  if (use_lane(k) && !(k.flags & DLM_OPT_SMOOTHER_COMPAT_Q1) && !k.packed) {
    e->variant = "lane";   // needs nothing from the forward pass: also serves dlm_smooth_batch
    HIP_TRY(e, dlm::launch_lane_smoother(k, e->stream));
  } else if (have_side && fast_smoother_ok(e, k)) {
    if (e->sparse_k) {
      e->variant = "sparse16";
      HIP_TRY(e, dlm::launch_sparse16_smoother(k, e->sparse_k, e->sp_dev, e->side, e->stream));
    } else {
      e->variant = "mfma16";
      HIP_TRY(e, dlm::launch_mfma16_smoother(k, e->side, e->stream));
    }
  } else if (have_side && use_tiled(k) && !(k.flags & DLM_OPT_SMOOTHER_COMPAT_Q1)) {
    e->variant = dlm::wave48_smoother_supported(k) ? "wave-mfma" : "tiled-mfma";   // fused call only: the information-form pass takes the innovations of the forward pass
    HIP_TRY(e, dlm::launch_tiled_smoother(k, e->ystar, e->stream));
  } else if (fast_shape_ok(k) && e->sparse_k > 0 && !(k.packed & 1)) {
    // RTS recursion on register tiles from the records alone: dlm_smooth_batch, and the literal Q1 covariance (Smoothing.scala:44)
    e->variant = "sparse16-rts";
    HIP_TRY(e, dlm::launch_sparse16_rts(k, e->sparse_k, e->sp_dev, e->stream));
  } else if (!(k.flags & DLM_OPT_FORCE_GENERIC) && dlm::wave48_small_ok(k)) {
    e->variant = "sparse16-rts";   // d <= 15 with several observation components: the same kernel on the multivariate tables
    HIP_TRY(e, dlm::launch_small_mv_rts(k, e->stream));
  } else {
    e->variant = "generic";
    if (dlm::generic_smoother_lds_bytes(k.d, k.p) > dlm::lds_limit())
      return fail(e, DLM_ERR_UNSUPPORTED, "the general RTS smoother kernel keeps six d x d matrices in the LDS of one CU: d <= 58 (structured models with d <= 48 take the per-wave kernels)");
    HIP_TRY(e, dlm::launch_generic_smoother(k, e->stream));
  }
  return DLM_OK;
}

// packed [m | lower triangle by rows] -> dense [m | C column-major]; one thread per dense element
__global__ void k_unpack_records(int d, long long count, int prec, const double* __restrict__ packed, double* __restrict__ dense) {
  const int rec = d + d * d;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count * rec) return;
  const long long r = i / rec;
  const int e = (int)(i - r * rec);
  const double* src = packed + r * prec;
  if (e < d) { dense[i] = src[e]; return; }
  const int a = (e - d) % d, b = (e - d) / d;           // element (row a, column b) of C
  const int hi = a > b ? a : b, lo = a > b ? b : a;
  dense[i] = src[d + hi * (hi + 1) / 2 + lo];
}

// ---- the three particle filters of a DGLM (dlm_pf.hip, dlm_storvik.hip, dlm_lw.hip) ----
// The checks they share, in the order every entry point makes them: the model and the descriptor's family and literal, then the filter's
// `own` (its learn_v, its shrinkage, its priors), then the data and the shapes the kernels cover.  `name`: "the ... filter" of the messages;
// reads_w: the bootstrap filter, which reads params->V and W; reads_v: params->V is read (a learning filter without learn_v)
template <class Own>
int pf_check(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params, int family, int literal, int P,
             const double* obs_param, const double* y, const double* ll, const std::string& name, bool reads_v, bool reads_w, Own&& own) {
  const int d = model->d, T = model->T, N = model->N;
  if (d < 1 || model->p < 1 || T < 1 || N < 1) return fail(e, DLM_ERR_ARG, "d, p, T, N must be >= 1");
  if (!model->F || !model->G || model->n_g < 1) return fail(e, DLM_ERR_ARG, "model tables F/G missing");
  if (model->n_g > 1 && !model->g_index) return fail(e, DLM_ERR_ARG, "n_g > 1 needs g_index");
  if (model->f_stride != 0 && model->f_stride != (int64_t)d * model->p) return fail(e, DLM_ERR_ARG, "f_stride must be 0 or d*p");
  if ((reads_w && (!params->V || !params->W)) || !params->m0 || !params->C0) return fail(e, DLM_ERR_ARG, reads_w ? "parameter arrays missing" : "parameter arrays m0/C0 missing");
  if (family < DLM_OBS_GAUSSIAN || family > DLM_OBS_BETA) return fail(e, DLM_ERR_ARG, "family: one of DLM_OBS_*");
  if (literal != 0 && literal != 1) return fail(e, DLM_ERR_ARG, "literal: 0 or 1");
  if (const int rc = own()) return rc;
  if (family == DLM_OBS_STUDENTT && !obs_param) return fail(e, DLM_ERR_ARG, "DLM_OBS_STUDENTT needs obs_param (the degrees of freedom of every series)");
  if (!y || !ll) return fail(e, DLM_ERR_ARG, "y and ll are required");
  if (model->p != 1) return fail(e, DLM_ERR_UNSUPPORTED, name + " takes a univariate observation (p = 1): every Dglm family reads y(0) and V(0,0)");
  if (d > dlm::DLM_PF_MAX_D) return fail(e, DLM_ERR_UNSUPPORTED, name + " takes d <= 16");
  if (P < 64 || P > dlm::DLM_PF_MAX_P || P % 64 != 0) return fail(e, DLM_ERR_UNSUPPORTED, "n_particles must be a multiple of 64 with 64 <= n_particles <= 1024 (one wavefront per series, whole slots of particles)");
  if (T > dlm::DLM_PF_MAX_T) return fail(e, DLM_ERR_UNSUPPORTED, "T must stay below 2^21 - 1 (the Philox counter's slot field)");
  if (reads_w && (params->v_tstride || params->w_tstride)) return fail(e, DLM_ERR_UNSUPPORTED, name + " takes time-invariant V and W (v_tstride = w_tstride = 0)");
  if (reads_v && params->v_tstride) return fail(e, DLM_ERR_UNSUPPORTED, name + " takes a time-invariant V (v_tstride = 0)");
  return DLM_OK;
}

// what the two learning filters ask of learn_v's sources and of the priors' strides
int pf_check_priors(dlm_engine* e, const dlm_params_desc* params, int d, int learn_v, const double* prior_v, int64_t prior_v_stride,
                    const double* prior_w, int64_t prior_w_stride) {
  if (learn_v ? !prior_v : !params->V) return fail(e, DLM_ERR_ARG, "learn_v = 1 needs prior_v, learn_v = 0 needs params->V");
  if (!prior_w) return fail(e, DLM_ERR_ARG, "prior_w is required");
  if ((prior_v_stride != 0 && prior_v_stride < 2) || (prior_w_stride != 0 && prior_w_stride < 2 * (int64_t)d)) return fail(e, DLM_ERR_ARG, "prior_v_stride must be 0 or >= 2, prior_w_stride 0 or >= 2 d");
  return DLM_OK;
}

// What the three kernels read and write, staged into the fields every argument struct has under PfCommonArgs' names, with its scalars and
// strides.  V: params->V, or null where the filter learns it (a null pointer stages nothing)
template <class Args>
void pf_stage(Stager& st, Args& a, const dlm_model_desc* model, const dlm_params_desc* params, int family, int literal, int n0, int P,
              const double* V, const double* obs_param, const double* y, const dlm_options* opts, uint64_t iteration, double* ll,
              double* mean, double* ess, double* cloud, double* weights, int32_t* status) {
  const size_t n = model->N, t = model->T, dd = model->d, np = P;
  st.in(&a.F, model->F, (model->f_stride ? t : 1) * dd);
  st.in(&a.G, model->G, (size_t)model->n_g * dd * dd);
  st.in(&a.g_index, (const int*)model->g_index, model->g_index ? t : 0);
  st.in(&a.dt, model->dt, model->dt ? t : 0);
  st.in(&a.V, V, params->v_stride ? (n - 1) * (size_t)params->v_stride + 1 : 1);
  st.in(&a.m0, params->m0, params->m0_stride ? (n - 1) * (size_t)params->m0_stride + dd : dd);
  st.in(&a.C0, params->C0, params->c0_stride ? (n - 1) * (size_t)params->c0_stride + dd * dd : dd * dd);
  st.in(&a.obs_param, obs_param, obs_param ? n : 0);
  st.in(&a.y, y, n * t);
  st.out(&a.ll, ll, n);
  st.out(&a.mean, mean, mean ? n * t * dd : 0);
  st.out(&a.ess, ess, ess ? n * t : 0);
  st.out(&a.cloud, cloud, cloud ? n * dd * np : 0);
  st.out(&a.weights, weights, weights ? n * np : 0);
  st.zeroed_out(&a.status, (int*)status, status ? n : 0);
  a.d = model->d; a.T = model->T; a.N = model->N; a.P = P;
  a.family = family; a.literal = literal;
  a.n0 = n0 < 0 ? P / 5 : n0;   // ParticleFilter.likelihood: floor(n / 5)
  a.f_stride = model->f_stride; a.n_g = model->n_g;
  a.v_stride = params->v_stride; a.m0_stride = params->m0_stride; a.c0_stride = params->c0_stride;
  a.rs = draw_stream(opts, iteration);
}

// the priors of a learning filter: prior_w [d][2] of every series, prior_v [2] with learn_v only
template <class Args>
void pf_stage_priors(Stager& st, Args& a, int learn_v, const double* prior_v, int64_t prior_v_stride, const double* prior_w,
                     int64_t prior_w_stride) {
  const size_t n = a.N, dd = a.d;
  st.in(&a.prior_v, learn_v ? prior_v : nullptr, prior_v_stride ? (n - 1) * (size_t)prior_v_stride + 2 : 2);
  st.in(&a.prior_w, prior_w, prior_w_stride ? (n - 1) * (size_t)prior_w_stride + 2 * dd : 2 * dd);
  a.learn_v = learn_v; a.prior_v_stride = prior_v_stride; a.prior_w_stride = prior_w_stride;
}

}  // namespace

extern "C" {

const char* dlm_version(void) { return "bayesian_dlms_amd 0.1.0 (gfx950)"; }

int dlm_engine_create(int device, dlm_engine** out) {
  if (!out) return DLM_ERR_ARG;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return DLM_ERR_HIP;
  dlm_engine* e = new dlm_engine();
  e->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete e;
    return DLM_ERR_HIP;
  }
  e->stream = e->own_stream;
  for (auto& ev : e->ev) (void)hipEventCreate(&ev);
  (void)hipEventCreateWithFlags(&e->order_ev, hipEventDisableTiming);
  *out = e;
  return DLM_OK;
}

void dlm_engine_destroy(dlm_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  (void)drain_all(e);   // rule B: nothing of a DLM_OPT_ASYNC call (or of a call that failed half-way) is in flight on any of the three streams
  if (e->has_comm) ncclCommDestroy(e->comm);
  for (Workspace* w = e->workspaces; w; w = w->next) if (w->p) (void)hipFree(w->p);
  if (e->spf_dev) (void)hipFree(e->spf_dev);
  if (e->rng_ev) (void)hipEventDestroy(e->rng_ev);
  if (e->rng_stream) (void)hipStreamDestroy(e->rng_stream);
  for (auto& ev : e->cov_ev) if (ev) (void)hipEventDestroy(ev);
  if (e->cov_ev2) (void)hipEventDestroy(e->cov_ev2);
  if (e->rts_ev) (void)hipEventDestroy(e->rts_ev);
  if (e->rng_gate) (void)hipEventDestroy(e->rng_gate);
  if (e->cov_stream) (void)hipStreamDestroy(e->cov_stream);
  if (e->counters) (void)hipFree(e->counters);
  if (e->model_sum) (void)hipFree(e->model_sum);
  if (e->model_bad) (void)hipHostFree(e->model_bad);
  for (void* b : e->buffers) (void)hipFree(b);
  if (e->order_ev) (void)hipEventDestroy(e->order_ev);
  for (auto& ev : e->ev) if (ev) (void)hipEventDestroy(ev);
  if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
  delete e;
}

const char* dlm_last_error(const dlm_engine* e) { return e ? e->err.c_str() : "null engine"; }
const char* dlm_last_variant(const dlm_engine* e) { return e ? e->variant : "none"; }

int dlm_engine_set_stream(dlm_engine* e, void* hip_stream) {
  if (!e) return DLM_ERR_ARG;
  hipStream_t next = hip_stream ? (hipStream_t)hip_stream : e->own_stream;
  if (next != e->stream) {
    // the engine's workspaces (side records, tables, staged parameters) belong to whatever runs on its stream: work still in
    // flight from DLM_OPT_ASYNC calls on the old stream is drained before anything is launched on the new one
    HIP_TRY(e, hipSetDevice(e->device));
    { const int rcd = drain_all(e); if (rcd) return rcd; }
    e->stream = next;
  }
  return DLM_OK;
}

int dlm_engine_sync(dlm_engine* e) {
  if (!e) return DLM_ERR_ARG;
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  if (e->model_bad && *e->model_bad) return promise_broken(e);   // a DLM_OPT_ASYNC call whose DLM_OPT_MODEL_UNCHANGED did not hold
  return DLM_OK;
}

int dlm_last_counters(dlm_engine* e, uint64_t out[4]) {
  if (!e || !out) return DLM_ERR_ARG;
  out[0] = out[1] = out[2] = out[3] = 0;
  if (!e->counters) return fail(e, DLM_ERR_ARG, "no call with DLM_OPT_COUNT_STEPS has been made");
  HIP_TRY(e, hipSetDevice(e->device));
  unsigned long long h[4];
  HIP_TRY(e, hipMemcpyAsync(h, e->counters, sizeof(h), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  for (int i = 0; i < 4; ++i) out[i] = h[i];
  return DLM_OK;
}

int dlm_last_table_reuse(dlm_engine* e, int32_t* out) {
  if (!e || !out) return DLM_ERR_ARG;
  *out = DLM_TABLES_NONE;
  if (!e->rts_last || !e->rtsws) return DLM_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  int h = 0;
  HIP_TRY(e, hipMemcpyAsync(&h, (const int*)e->rtsws.p + dlm::RTS_CTL_LAST, sizeof(h), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  *out = h;
  return DLM_OK;
}

int dlm_engine_wait_stream(dlm_engine* e, void* hip_stream) {
  if (!e) return DLM_ERR_ARG;
  HIP_TRY(e, hipSetDevice(e->device));
  if ((hipStream_t)hip_stream == e->stream) return DLM_OK;
  HIP_TRY(e, hipEventRecord(e->order_ev, (hipStream_t)hip_stream));
  HIP_TRY(e, hipStreamWaitEvent(e->stream, e->order_ev, 0));
  return DLM_OK;
}

int dlm_stream_wait_engine(dlm_engine* e, void* hip_stream) {
  if (!e) return DLM_ERR_ARG;
  HIP_TRY(e, hipSetDevice(e->device));
  if ((hipStream_t)hip_stream == e->stream) return DLM_OK;
  HIP_TRY(e, hipEventRecord(e->order_ev, e->stream));
  HIP_TRY(e, hipStreamWaitEvent((hipStream_t)hip_stream, e->order_ev, 0));
  return DLM_OK;
}

int dlm_buffer_alloc(dlm_engine* e, uint64_t bytes, void** dev_ptr) {
  if (!e) return DLM_ERR_ARG;
  if (!dev_ptr || bytes == 0) return fail(e, DLM_ERR_ARG, "dlm_buffer_alloc: dev_ptr and a non-zero size are required");
  *dev_ptr = nullptr;
  HIP_TRY(e, hipSetDevice(e->device));
  void* p = nullptr;
  HIP_TRY(e, hipMalloc(&p, (size_t)bytes));
  e->buffers.insert(p);
  *dev_ptr = p;
  return DLM_OK;
}

int dlm_buffer_free(dlm_engine* e, void* dev_ptr) {
  if (!e) return DLM_ERR_ARG;
  if (!dev_ptr) return DLM_OK;
  auto it = e->buffers.find(dev_ptr);
  if (it == e->buffers.end()) return fail(e, DLM_ERR_ARG, "dlm_buffer_free: not a buffer of this engine");
  HIP_TRY(e, hipSetDevice(e->device));
  HIP_TRY(e, hipStreamSynchronize(e->stream));   // no engine work may still use it
  HIP_TRY(e, hipFree(dev_ptr));
  e->buffers.erase(it);
  return DLM_OK;
}

int dlm_buffer_upload(dlm_engine* e, void* dst_dev, uint64_t dst_offset, const void* src_host, uint64_t bytes) {
  if (!e) return DLM_ERR_ARG;
  if (!dst_dev || (!src_host && bytes)) return fail(e, DLM_ERR_ARG, "dlm_buffer_upload: null pointer");
  if (!bytes) return DLM_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  HIP_TRY(e, hipMemcpyAsync((char*)dst_dev + dst_offset, src_host, (size_t)bytes, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return DLM_OK;
}

int dlm_buffer_download(dlm_engine* e, const void* src_dev, uint64_t src_offset, void* dst_host, uint64_t bytes) {
  if (!e) return DLM_ERR_ARG;
  if (!src_dev || (!dst_host && bytes)) return fail(e, DLM_ERR_ARG, "dlm_buffer_download: null pointer");
  if (!bytes) return DLM_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  HIP_TRY(e, hipMemcpyAsync(dst_host, (const char*)src_dev + src_offset, (size_t)bytes, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return DLM_OK;
}

int dlm_buffer_fill(dlm_engine* e, void* dst_dev, uint64_t dst_offset, int byte_value, uint64_t bytes) {
  if (!e) return DLM_ERR_ARG;
  if (!dst_dev) return fail(e, DLM_ERR_ARG, "dlm_buffer_fill: null pointer");
  if (!bytes) return DLM_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  HIP_TRY(e, hipMemsetAsync((char*)dst_dev + dst_offset, byte_value, (size_t)bytes, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return DLM_OK;
}

int dlm_device_mem_info(dlm_engine* e, uint64_t* free_bytes, uint64_t* total_bytes) {
  if (!e) return DLM_ERR_ARG;
  HIP_TRY(e, hipSetDevice(e->device));
  size_t f = 0, t = 0;
  HIP_TRY(e, hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = f;
  if (total_bytes) *total_bytes = t;
  return DLM_OK;
}

int dlm_last_timing(dlm_engine* e, double ms[2]) {
  if (!e || !ms) return DLM_ERR_ARG;
  if (!e->timed) return fail(e, DLM_ERR_ARG, "no forward / backward call has been timed yet");
  float f = 0.f, b = 0.f;
  HIP_TRY(e, hipEventSynchronize(e->ev[2]));
  HIP_TRY(e, hipEventElapsedTime(&f, e->ev[0], e->ev[1]));
  HIP_TRY(e, hipEventElapsedTime(&b, e->ev[1], e->ev[2]));
  ms[0] = f; ms[1] = b;
  return DLM_OK;
}

int32_t dlm_stats_len(int32_t d, int32_t p, uint32_t flags) { return dlm::stats_len(d, p, flags); }

int32_t dlm_packed_record_doubles(int32_t d) { return d < 1 ? 0 : dlm::packed_rec_bytes(d) / 8; }

int dlm_unpack_records(dlm_engine* e, int32_t d, int64_t count, const double* packed, const dlm_options* opts, double* dense) {
  if (!e) return DLM_ERR_ARG;
  if (!opts || (opts->mem != DLM_MEM_DEVICE && opts->mem != DLM_MEM_HOST)) return fail(e, DLM_ERR_ARG, "opts");
  if (d < 1 || d > 64 || count < 1 || !packed || !dense) return fail(e, DLM_ERR_ARG, "dlm_unpack_records arguments");
  HIP_TRY(e, hipSetDevice(e->device));
  const size_t prec = (size_t)dlm_packed_record_doubles(d), rec = (size_t)d + (size_t)d * d;
  const double* src = nullptr; double* dst = nullptr;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  st.in(&src, packed, (size_t)count * prec);
  st.out(&dst, dense, (size_t)count * rec);
  int rc = st.commit();
  if (rc) return rc;
  const long long total = (long long)count * (long long)rec;
  HIP_TRY(e, dlm::launch(k_unpack_records, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, e->stream, (int)d, (long long)count, (int)prec, src, dst));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_filter_batch(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params,
                     const double* y, const dlm_options* opts, double* filt, double* prior,
                     double* fq, int32_t* status) {
  int rc = check_common(e, model, params, opts);
  if (rc) return rc;
  if (!y || !filt) return fail(e, DLM_ERR_ARG, "y and filt are required");
  const size_t d = model->d, p = model->p, T = model->T, N = model->N, rec = d + d * d;
  const bool want_packed = (opts->flags & DLM_OPT_PACKED_SYM) != 0;
  if (want_packed && prior) return fail(e, DLM_ERR_UNSUPPORTED, "DLM_OPT_PACKED_SYM: prior records are not available packed");
  KArgs k{};
  Stager st(e, opts->mem == DLM_MEM_HOST);
  stage_model(st, k, model, params, opts);
  st.in(&k.y, y, N * T * p);
  st.out(&k.filt, filt, N * (T + 1) * (want_packed ? (size_t)dlm_packed_record_doubles((int)d) : rec));
  st.out(&k.prior, prior, N * (T + 1) * rec);
  st.out(&k.fq, fq, N * (T + 1) * (p + p * p));
  st.zeroed_out(&k.status, (int*)status, N);
  if ((rc = st.commit())) return rc;
  if ((rc = analyse_g(e, k, model->G, opts->mem == DLM_MEM_HOST))) return rc;
  if (want_packed) {
    if ((rc = packed_path(e, k))) return rc;
    k.packed = 1;
  }
  if ((rc = mark_plain(e, k))) return rc;
  if (use_shared_cov(e, k)) {
    dlm::CovTabs tb;
    if ((rc = run_shared_filter(e, k, tb, false))) return rc;
    return st.finish(opts->flags & DLM_OPT_ASYNC);
  }
  if ((rc = run_filter(e, k, false))) return rc;
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_simulate_batch(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params,
                       const dlm_options* opts, double* x, double* y, int32_t* status) {
  int rc = check_common(e, model, params, opts);
  if (rc) return rc;
  if (!y) return fail(e, DLM_ERR_ARG, "y is required");
  const size_t d = model->d, p = model->p, T = model->T, N = model->N;
  KArgs k{};
  Stager st(e, opts->mem == DLM_MEM_HOST);
  stage_model(st, k, model, params, opts);
  st.out(&k.theta, x, x ? N * (T + 1) * d : 0);
  st.out(&k.smooth, y, N * T * p);
  st.zeroed_out(&k.status, (int*)status, status ? N : 0);
  if ((rc = st.commit())) return rc;
  e->variant = "generic-simulate";
  HIP_TRY(e, dlm::launch_generic_simulate(k, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_dinvgamma_step_batch(dlm_engine* e, int32_t d, int32_t p, int32_t N, const double* stats, double alpha_v,
                             double beta_v, double alpha_w, double beta_w, uint64_t iteration, const dlm_options* opts,
                             double* V_out, double* W_out) {
  if (!e) return DLM_ERR_ARG;
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  if (d < 1 || p < 1 || N < 1 || !stats || !V_out || !W_out) return fail(e, DLM_ERR_ARG, "d, p, N >= 1; stats, V_out, W_out required");
  if (!(alpha_v > 0.0 && beta_v > 0.0 && alpha_w > 0.0 && beta_w > 0.0)) return fail(e, DLM_ERR_ARG, "InverseGamma priors need positive shape and scale");
  HIP_TRY(e, hipSetDevice(e->device));
  struct { const double* stats; double *V, *W; } k{};
  const size_t n = N, L = 2 * (size_t)p + d + 1;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  st.in(&k.stats, stats, n * L);
  st.out(&k.V, V_out, n * p * p);
  st.out(&k.W, W_out, n * d * d);
  if ((rc = st.commit())) return rc;
  e->variant = "dinvgamma-step";
  HIP_TRY(e, dlm::launch_dinvgamma_step(d, p, N, k.stats, alpha_v, beta_v, alpha_w, beta_w, draw_stream(opts, iteration), k.V, k.W, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_studentt_step_batch(dlm_engine* e, const dlm_model_desc* model, const double* y, const double* theta,
                            const double* stats, const dlm_studentt_prior* prior, const double* scale_in,
                            const int32_t* nu_in, uint64_t iteration, const dlm_options* opts, double* v_out,
                            double* scale_out, int32_t* nu_out, double* W_out, int32_t* accepted,
                            double* loglik, int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  if (!model || !prior) return fail(e, DLM_ERR_ARG, "null descriptor");
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  const int d = model->d, T = model->T, N = model->N;
  if (d < 1 || T < 1 || N < 1 || model->p < 1) return fail(e, DLM_ERR_ARG, "d, p, T, N must be >= 1");
  if (model->p != 1) return fail(e, DLM_ERR_UNSUPPORTED, "the Student-t step is univariate (StudentTGibbs.scala reads y(0) and v(0,0)): p must be 1");
  if (d > 64) return fail(e, DLM_ERR_UNSUPPORTED, "d is limited to 64 in this build");
  if (T > dlm::DLM_ST_MAX_T) return fail(e, DLM_ERR_UNSUPPORTED, "T must stay below 2^21 - 4 (the Philox counter's slot field)");
  if (!model->F || (model->f_stride != 0 && model->f_stride != (int64_t)d)) return fail(e, DLM_ERR_ARG, "F required; f_stride must be 0 or d");
  const bool literal = (opts->flags & DLM_OPT_STUDENTT_LITERAL) != 0;
  if (literal && model->f_stride)
    return fail(e, DLM_ERR_UNSUPPORTED, "DLM_OPT_STUDENTT_LITERAL pairs y_t with theta_{t-1} and F at ITS time (SURVEY Q11): t0 - 1 is not in a time-varying F table");
  if (!y || !theta || !stats || !scale_in || !nu_in || !v_out || !scale_out || !nu_out || !W_out || !accepted)
    return fail(e, DLM_ERR_ARG, "y, theta, stats, scale_in, nu_in, v_out, scale_out, nu_out, W_out and accepted are required");
  if (!(prior->prior_nu_rate > 0.0 && prior->prop_nu_size > 0.0 && prior->prior_w_shape > 0.0 && prior->prior_w_scale > 0.0))
    return fail(e, DLM_ERR_ARG, "the Poisson rate, the proposal size and the InverseGamma prior of W must be positive");
  HIP_TRY(e, hipSetDevice(e->device));
  dlm::StudentTArgs k{};
  const size_t n = N, t = T, dd = d;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  st.in(&k.F, model->F, (model->f_stride ? t : 1) * dd);
  st.in(&k.y, y, n * t);
  st.in(&k.theta, theta, n * (t + 1) * dd);
  st.in(&k.stats, stats, n * (dd + 3));
  st.in(&k.scale_in, scale_in, n);
  st.in(&k.nu_in, (const int*)nu_in, n);
  st.out(&k.v_out, v_out, n * t);
  st.out(&k.scale_out, scale_out, n);
  st.out(&k.nu_out, (int*)nu_out, n);
  st.out(&k.W_out, W_out, n * dd * dd);
  st.inout(&k.accepted, (int*)accepted, n);
  st.out(&k.loglik, loglik, loglik ? n : 0);
  st.zeroed_out(&k.status, (int*)status, status ? n : 0);
  if ((rc = st.commit())) return rc;
  k.d = d; k.T = T; k.N = N; k.f_stride = model->f_stride;
  k.prior = *prior;
  k.literal = literal ? 1 : 0;
  k.rs = draw_stream(opts, iteration);
  e->variant = "studentt-step";
  HIP_TRY(e, dlm::launch_studentt_step(k, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_sv_mixture_batch(dlm_engine* e, int32_t N, int32_t T, const double* y, const double* alpha, uint64_t iteration,
                         const dlm_options* opts, double* ystar, double* v, int8_t* k, int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  if (N < 1 || T < 2) return fail(e, DLM_ERR_ARG, "N >= 1 and T >= 2 (the reference's parameter draws throw on a single observation, StochasticVolatility.scala:220-222)");
  if (T > dlm::DLM_SV_MAX_T) return fail(e, DLM_ERR_ARG, "T must stay below 2^21 - 8 (the Philox counter's slot field)");
  if ((long long)N * T >= (1ll << 39)) return fail(e, DLM_ERR_ARG, "N T must stay below 2^39 (one thread per element)");
  if (!y || !ystar || !v) return fail(e, DLM_ERR_ARG, "y, ystar and v are required");
  HIP_TRY(e, hipSetDevice(e->device));
  dlm::SvMixArgs a{};
  const size_t n = N, t = T;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  st.in(&a.y, y, n * t);
  st.in(&a.alpha, alpha, alpha ? n * (t + 1) : 0);
  st.out(&a.ystar, ystar, n * t);
  st.out(&a.v, v, n * t);
  st.out(&a.k, (signed char*)k, k ? n * t : 0);
  st.zeroed_out(&a.status, (int*)status, status ? n : 0);
  if ((rc = st.commit())) return rc;
  a.N = N; a.T = T;
  a.rs = draw_stream(opts, iteration);
  e->variant = "sv-mixture";
  HIP_TRY(e, dlm::launch_sv_mixture(a, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_sv_params_batch(dlm_engine* e, int32_t N, int32_t T, const double* alpha, const double* sv_in, const dlm_sv_prior* prior,
                        uint64_t iteration, const dlm_options* opts, double* sv_out, int32_t* accepted, int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  if (!prior) return fail(e, DLM_ERR_ARG, "null descriptor");
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  if (N < 1 || T < 2) return fail(e, DLM_ERR_ARG, "N >= 1 and T >= 2 (the reference's sums throw on a single observation, StochasticVolatility.scala:220-222)");
  if (T > dlm::DLM_SV_MAX_T) return fail(e, DLM_ERR_ARG, "T must stay below 2^21 - 8 (the Philox counter's slot field)");
  if (prior->phi_update != 0 && prior->phi_update != 1) return fail(e, DLM_ERR_ARG, "phi_update: 0 (Gaussian conjugate) or 1 (Beta-proposal Metropolis-Hastings)");
  if (prior->literal != 0 && prior->literal != 1) return fail(e, DLM_ERR_ARG, "literal: 0 or 1");
  const bool beta = prior->phi_update == 1;
  if (!alpha || !sv_in || !sv_out || (beta && !accepted)) return fail(e, DLM_ERR_ARG, "alpha, sv_in and sv_out are required (and accepted with the Beta proposal)");
  if (!(is_positive(prior->mu_sd) && is_finite(prior->mu_mean))) return fail(e, DLM_ERR_ARG, "the Gaussian prior of mu needs a finite mean and a positive standard deviation");
  if (!(is_positive(prior->sigma_shape) && is_positive(prior->sigma_scale))) return fail(e, DLM_ERR_ARG, "the InverseGamma prior of sigma^2 needs a positive shape and scale");
  if (beta) {
    if (!(is_positive(prior->phi_a) && is_positive(prior->phi_b))) return fail(e, DLM_ERR_ARG, "the Beta prior of phi needs positive a and b");
    if (!(is_positive(prior->prop_lambda) && is_positive(prior->prop_tau))) return fail(e, DLM_ERR_ARG, "the Beta proposal needs positive lambda and tau");
  } else if (!(is_positive(prior->phi_b) && is_finite(prior->phi_a))) {
    return fail(e, DLM_ERR_ARG, "the Gaussian prior of phi needs a finite mean and a positive standard deviation");
  }
  HIP_TRY(e, hipSetDevice(e->device));
  dlm::SvParamsArgs a{};
  const size_t n = N, t = T;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  st.in(&a.alpha, alpha, n * (t + 1));
  st.in(&a.sv_in, sv_in, n * 3);
  st.out(&a.sv_out, sv_out, n * 3);
  st.inout(&a.accepted, (int*)accepted, accepted ? n : 0);
  st.zeroed_out(&a.status, (int*)status, status ? n : 0);
  if ((rc = st.commit())) return rc;
  a.N = N; a.T = T;
  a.prior = *prior;
  a.rs = draw_stream(opts, iteration);
  e->variant = "sv-params";
  HIP_TRY(e, dlm::launch_sv_params(a, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_sv_ou_params_batch(dlm_engine* e, int32_t N, int32_t T, const double* times, const double* alpha, const double* sv_in,
                           const dlm_sv_ou_prior* prior, uint64_t iteration, const dlm_options* opts, double* sv_out,
                           int32_t* accepted, int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  if (!prior) return fail(e, DLM_ERR_ARG, "null descriptor");
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  if (N < 1 || T < 2) return fail(e, DLM_ERR_ARG, "N >= 1 and T >= 2 (one informative pair of states at least)");
  if (T > dlm::DLM_SVOU_MAX_T) return fail(e, DLM_ERR_ARG, "T must stay below 2^21 - 8 (the Philox counter's slot field)");
  if (prior->literal != 0 && prior->literal != 1) return fail(e, DLM_ERR_ARG, "literal: 0 or 1");
  if (!times || !alpha || !sv_in || !sv_out || !accepted) return fail(e, DLM_ERR_ARG, "times, alpha, sv_in, sv_out and accepted are required");
  if (!(is_positive(prior->phi_a) && is_positive(prior->phi_b))) return fail(e, DLM_ERR_ARG, "the Beta prior of phi needs positive a and b");
  if (!(is_positive(prior->mu_sd) && is_finite(prior->mu_mean))) return fail(e, DLM_ERR_ARG, "the Gaussian prior of mu needs a finite mean and a positive standard deviation");
  if (!(is_positive(prior->sigma_shape) && is_positive(prior->sigma_scale))) return fail(e, DLM_ERR_ARG, "the InverseGamma prior of sigma needs a positive shape and scale");
  if (!(is_positive(prior->prop_lambda) && is_positive(prior->prop_tau))) return fail(e, DLM_ERR_ARG, "the Beta proposal needs positive lambda and tau");
  if (!(is_positive(prior->delta_sigma) && is_positive(prior->delta_mu))) return fail(e, DLM_ERR_ARG, "the random walks of sigma and mu need positive standard deviations");
  HIP_TRY(e, hipSetDevice(e->device));
  dlm::SvOuParamsArgs a{};
  const size_t n = N, t = T;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  st.in(&a.times, times, t);
  st.in(&a.alpha, alpha, n * (t + 1));
  st.in(&a.sv_in, sv_in, n * 3);
  st.out(&a.sv_out, sv_out, n * 3);
  st.inout(&a.accepted, (int*)accepted, n * 3);
  st.zeroed_out(&a.status, (int*)status, status ? n : 0);
  if ((rc = st.commit())) return rc;
  a.N = N; a.T = T;
  a.prior = *prior;
  a.rs = draw_stream(opts, iteration);
  e->variant = "sv-ou-params";
  HIP_TRY(e, dlm::launch_sv_ou_params(a, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_sv_knots_batch(dlm_engine* e, int32_t N, int32_t T, const double* y, const int32_t* knots, int32_t B, const double* sv,
                       int64_t sv_stride, uint64_t iteration, const dlm_options* opts, double* alpha, int32_t* accepted, int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  if (N < 1 || T < 2) return fail(e, DLM_ERR_ARG, "N >= 1 and T >= 2 (the chain's parameter draws need two observations)");
  if (T > dlm::DLM_SVKNOT_MAX_T) return fail(e, DLM_ERR_ARG, "T + 1 must stay below 2^21 - 8 (the Philox counter's slot field)");
  if (!y || !knots || !sv || !alpha) return fail(e, DLM_ERR_ARG, "y, knots, sv and alpha are required");
  if (B < 1 || B > T + 1) return fail(e, DLM_ERR_ARG, "1 <= B <= T + 1 blocks");
  if (sv_stride != 0 && sv_stride != 3) return fail(e, DLM_ERR_ARG, "sv_stride must be 0 or 3");
  HIP_TRY(e, hipSetDevice(e->device));
  // the knots bound every index of the sweep: they are read on the host before anything is launched
  std::vector<int32_t> kn((size_t)B + 1);
  if (opts->mem == DLM_MEM_HOST) {
    kn.assign(knots, knots + B + 1);
  } else {
    HIP_TRY(e, hipMemcpyAsync(kn.data(), knots, kn.size() * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
  }
  if (kn[0] != 0 || kn[B] != T + 1) return fail(e, DLM_ERR_ARG, "knots[0] must be 0 and knots[B] must be T + 1");
  for (int i = 0; i < B; ++i)
    if (kn[i + 1] <= kn[i]) return fail(e, DLM_ERR_ARG, "knots must be strictly increasing");
  dlm::SvKnotsArgs a{};
  const size_t n = N, t = T;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  st.in(&a.y, y, n * t);
  st.in(&a.knots, (const int*)knots, (size_t)B + 1);
  st.in(&a.sv, sv, sv_stride ? n * 3 : 3);
  st.inout(&a.alpha, alpha, n * (t + 1));
  st.inout(&a.accepted, (int*)accepted, accepted ? n : 0);
  st.zeroed_out(&a.status, (int*)status, status ? n : 0);
  if ((rc = st.commit())) return rc;
  // scratch: the records [N][T+1][2], the proposal [N][T+1], and one more record per series, whose first N words are the row flags
  if ((rc = ensure_side(e, n, t + 1))) return rc;
  a.filt = e->side;
  a.prop = e->side + 2 * n * (t + 1);
  a.rowflag = (int*)(e->side + 3 * n * (t + 1));
  a.N = N; a.T = T; a.B = B; a.sv_stride = sv_stride;
  a.rs = draw_stream(opts, iteration);
  e->variant = "sv-knots-lane";
  HIP_TRY(e, dlm::launch_sv_knots(a, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

// what the two factor stochastic-volatility calls ask of their shape
static int fsv_check_shape(dlm_engine* e, int32_t N, int32_t T, int32_t p, int32_t k) {
  if (N < 1 || T < 2) return fail(e, DLM_ERR_ARG, "N >= 1 and T >= 2 (the factor chains' volatility calls need two observations)");
  if (T > dlm::DLM_FSV_MAX_T) return fail(e, DLM_ERR_ARG, "T must stay below 2^21 - 64 (the Philox counter's slot field)");
  if (k < 1 || k > dlm::DLM_FSV_MAX_K || p < k || p > dlm::DLM_FSV_MAX_P) return fail(e, DLM_ERR_ARG, "1 <= k <= 8 and k <= p <= 64");
  if ((long long)N * ((T + 255) / 256) > 0x7FFFFFFFll) return fail(e, DLM_ERR_ARG, "N ceil(T / 256) must stay below 2^31 (one block per 256 times of a panel)");
  return DLM_OK;
}

int dlm_fsv_factors_batch(dlm_engine* e, int32_t N, int32_t T, int32_t p, int32_t k, const double* y, const double* beta,
                          const double* v, const double* alpha, int32_t literal, uint64_t iteration, const dlm_options* opts,
                          double* f, int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  if ((rc = fsv_check_shape(e, N, T, p, k))) return rc;
  if (literal != 0 && literal != 1) return fail(e, DLM_ERR_ARG, "literal: 0 or 1");
  if (!y || !beta || !v || !f) return fail(e, DLM_ERR_ARG, "y, beta, v and f are required");
  HIP_TRY(e, hipSetDevice(e->device));
  dlm::FsvFactorsArgs a{};
  const size_t n = N, t = T, pp = p, kk = k;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  st.in(&a.y, y, n * t * pp);
  st.in(&a.beta, beta, n * pp * kk);
  st.in(&a.v, v, n * pp);
  st.in(&a.alpha, alpha, alpha ? n * kk * (t + 1) : 0);
  st.out(&a.f, f, n * kk * t);
  st.zeroed_out(&a.status, (int*)status, status ? n : 0);
  if ((rc = st.commit())) return rc;
  a.N = N; a.T = T; a.p = p; a.k = k;
  a.literal = literal;
  a.rs = draw_stream(opts, iteration);
  e->variant = "fsv-factors";
  HIP_TRY(e, dlm::launch_fsv_factors(a, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_fsv_loadings_batch(dlm_engine* e, int32_t N, int32_t T, int32_t p, int32_t k, const double* y, const double* f,
                           const double* beta_in, const double* v_in, const dlm_fsv_prior* prior, uint64_t iteration,
                           const dlm_options* opts, double* beta_out, double* v_out, int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  if (!prior) return fail(e, DLM_ERR_ARG, "null descriptor");
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  if ((rc = fsv_check_shape(e, N, T, p, k))) return rc;
  if (prior->literal != 0 && prior->literal != 1) return fail(e, DLM_ERR_ARG, "literal: 0 or 1");
  if (!(is_positive(prior->beta_sd) && is_finite(prior->beta_mean))) return fail(e, DLM_ERR_ARG, "the Gaussian prior of beta needs a finite mean and a positive standard deviation");
  if (!(is_positive(prior->sigma_shape) && is_positive(prior->sigma_scale))) return fail(e, DLM_ERR_ARG, "the InverseGamma prior of sigma^2 needs a positive shape and scale");
  if (!y || !f || !beta_in || !beta_out || !v_out) return fail(e, DLM_ERR_ARG, "y, f, beta_in, beta_out and v_out are required");
  HIP_TRY(e, hipSetDevice(e->device));
  dlm::FsvLoadingsArgs a{};
  const size_t n = N, t = T, pp = p, kk = k;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  st.in(&a.y, y, n * t * pp);
  st.in(&a.f, f, n * kk * t);
  st.in(&a.beta_in, beta_in, n * pp * kk);
  st.in(&a.v_in, v_in, v_in ? n * pp : 0);
  st.out(&a.beta_out, beta_out, n * pp * kk);
  st.out(&a.v_out, v_out, n * pp);
  st.zeroed_out(&a.status, (int*)status, status ? n : 0);
  if ((rc = st.commit())) return rc;
  a.N = N; a.T = T; a.p = p; a.k = k;
  a.prior = *prior;
  a.rs = draw_stream(opts, iteration);
  e->variant = "fsv-loadings";
  HIP_TRY(e, dlm::launch_fsv_loadings(a, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_dlmfsv_center_batch(dlm_engine* e, const dlm_model_desc* model, const double* y, const double* theta,
                            const dlm_options* opts, double* r, int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  if (!model) return fail(e, DLM_ERR_ARG, "null descriptor");
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  const int d = model->d, p = model->p, T = model->T, N = model->N;
  if (d < 1 || p < 1 || T < 1 || N < 1) return fail(e, DLM_ERR_ARG, "d, p, T, N must be >= 1");
  if (d > 64 || p > dlm::DLM_FSV_MAX_P) return fail(e, DLM_ERR_UNSUPPORTED, "d and p are limited to 64 in this build");
  if (!model->F || (model->f_stride != 0 && model->f_stride != (int64_t)d * p)) return fail(e, DLM_ERR_ARG, "F required; f_stride must be 0 or d p");
  if ((long long)T * p > 0x7FFFF000ll) return fail(e, DLM_ERR_ARG, "T p must stay below 2^31 - 4096 (a panel's elements are indexed with an int)");
  if ((long long)N * (((long long)T * p + 255) / 256) > 0x7FFFFFFFll) return fail(e, DLM_ERR_ARG, "N ceil(T p / 256) must stay below 2^31 (the grid of the centring kernel)");
  if (!y || !theta || !r) return fail(e, DLM_ERR_ARG, "y, theta and r are required");
  HIP_TRY(e, hipSetDevice(e->device));
  dlm::DlmFsvCenterArgs a{};
  const size_t n = N, t = T, pp = p, dd = d;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  st.in(&a.F, model->F, (model->f_stride ? t : 1) * dd * pp);
  st.in(&a.y, y, n * t * pp);
  st.in(&a.theta, theta, n * (t + 1) * dd);
  st.out(&a.r, r, n * t * pp);
  st.zeroed_out(&a.status, (int*)status, status ? n : 0);
  if ((rc = st.commit())) return rc;
  a.N = N; a.T = T; a.p = p; a.d = d; a.f_stride = model->f_stride;
  e->variant = "dlmfsv-center";
  HIP_TRY(e, dlm::launch_dlmfsv_center(a, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_dlmfsv_impute_batch(dlm_engine* e, int32_t N, int32_t T, int32_t p, int32_t k, const double* r_in, const double* beta,
                            const double* v, const double* alpha, uint64_t iteration, const dlm_options* opts, double* r_out,
                            int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  if ((rc = fsv_check_shape(e, N, T, p, k))) return rc;
  if (!r_in || !beta || !v || !alpha || !r_out) return fail(e, DLM_ERR_ARG, "r_in, beta, v, alpha and r_out are required");
  HIP_TRY(e, hipSetDevice(e->device));
  dlm::DlmFsvImputeArgs a{};
  const size_t n = N, t = T, pp = p, kk = k;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  st.in(&a.r_in, r_in, n * t * pp);
  st.in(&a.beta, beta, n * pp * kk);
  st.in(&a.v, v, n * pp);
  st.in(&a.alpha, alpha, n * kk * (t + 1));
  st.out(&a.r_out, r_out, n * t * pp);
  st.zeroed_out(&a.status, (int*)status, status ? n : 0);
  if ((rc = st.commit())) return rc;
  a.N = N; a.T = T; a.p = p; a.k = k;
  a.rs = draw_stream(opts, iteration);
  e->variant = "dlmfsv-impute";
  HIP_TRY(e, dlm::launch_dlmfsv_impute(a, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_dlmfsv_variance_batch(dlm_engine* e, int32_t N, int32_t T, int32_t p, int32_t k, const double* beta, const double* v,
                              const double* alpha, const dlm_options* opts, double* V, int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  if (N < 1 || T < 1) return fail(e, DLM_ERR_ARG, "N >= 1 and T >= 1");
  if (k < 1 || k > dlm::DLM_FSV_MAX_K || p < k || p > dlm::DLM_FSV_MAX_P) return fail(e, DLM_ERR_UNSUPPORTED, "1 <= k <= 8 and k <= p <= 64");
  if ((long long)N * ((T + 63) / 64) > 0x7FFFFFFFll) return fail(e, DLM_ERR_ARG, "N ceil(T / 64) must stay below 2^31 (one block per 64 times of a panel)");
  if (!beta || !v || !alpha || !V) return fail(e, DLM_ERR_ARG, "beta, v, alpha and V are required");
  HIP_TRY(e, hipSetDevice(e->device));
  dlm::DlmFsvVarianceArgs a{};
  const size_t n = N, t = T, pp = p, kk = k;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  st.in(&a.beta, beta, n * pp * kk);
  st.in(&a.v, v, n * pp);
  st.in(&a.alpha, alpha, n * kk * (t + 1));
  st.out(&a.V, V, n * t * pp * pp);
  st.zeroed_out(&a.status, (int*)status, status ? n : 0);
  if ((rc = st.commit())) return rc;
  a.N = N; a.T = T; a.p = p; a.k = k;
  e->variant = "dlmfsv-variance";
  HIP_TRY(e, dlm::launch_dlmfsv_variance(a, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_dlmfsvsys_innovations_batch(dlm_engine* e, const dlm_model_desc* model, const double* theta, const dlm_options* opts,
                                    double* w, int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  if (!model) return fail(e, DLM_ERR_ARG, "null descriptor");
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  const int d = model->d, T = model->T, N = model->N;
  if (d < 1 || T < 1 || N < 1) return fail(e, DLM_ERR_ARG, "d, T, N must be >= 1");
  if (d > 64) return fail(e, DLM_ERR_UNSUPPORTED, "d is limited to 64 in this build");
  if (model->g_index || model->dt) return fail(e, DLM_ERR_UNSUPPORTED, "the innovations take one G on the regular unit grid (no g_index, no dt): the AR(1) volatility of the factors has no dt");
  if (!model->G || model->n_g != 1) return fail(e, DLM_ERR_ARG, "one G required (n_g = 1)");
  if ((long long)T * d > 0x7FFFF000ll) return fail(e, DLM_ERR_ARG, "T d must stay below 2^31 - 4096 (a panel's elements are indexed with an int)");
  if ((long long)N * (((long long)T * d + 255) / 256) > 0x7FFFFFFFll) return fail(e, DLM_ERR_ARG, "N ceil(T d / 256) must stay below 2^31 (the grid of the innovations kernel)");
  if (!theta || !w) return fail(e, DLM_ERR_ARG, "theta and w are required");
  if (w == theta) return fail(e, DLM_ERR_ARG, "w must not be theta");
  HIP_TRY(e, hipSetDevice(e->device));
  dlm::DlmFsvSysInnovationsArgs a{};
  const size_t n = N, t = T, dd = d;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  st.in(&a.G, model->G, dd * dd);
  st.in(&a.theta, theta, n * (t + 1) * dd);
  st.out(&a.w, w, n * t * dd);
  st.zeroed_out(&a.status, (int*)status, status ? n : 0);
  if ((rc = st.commit())) return rc;
  a.N = N; a.T = T; a.d = d;
  e->variant = "dlmfsvsys-innovations";
  HIP_TRY(e, dlm::launch_dlmfsvsys_innovations(a, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_pf_batch(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params, const dlm_pf_desc* pf,
                 const double* obs_param, const double* y, uint64_t iteration, const dlm_options* opts, double* ll,
                 double* mean, double* ess, double* cloud, double* weights, int32_t* status) {
  const dlm_resample_desc rs{DLM_RESAMPLE_MULTINOMIAL, 0};
  return dlm_pf_resampled(e, model, params, pf, &rs, obs_param, y, iteration, opts, ll, mean, ess, cloud, weights, status);
}

int dlm_pf_resampled(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params, const dlm_pf_desc* pf,
                           const dlm_resample_desc* resample, const double* obs_param, const double* y, uint64_t iteration,
                           const dlm_options* opts, double* ll, double* mean, double* ess, double* cloud, double* weights, int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  if (!model || !params || !pf || !resample) return fail(e, DLM_ERR_ARG, "null descriptor");
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  const int d = model->d, P = pf->n_particles;
  if ((rc = pf_check(e, model, params, pf->family, pf->literal, P, obs_param, y, ll, "the particle filter", true, true, [&] {
        if (resample->scheme < DLM_RESAMPLE_MULTINOMIAL || resample->scheme > DLM_RESAMPLE_METROPOLIS) return fail(e, DLM_ERR_ARG, "scheme: one of DLM_RESAMPLE_*");
        if (resample->scheme == DLM_RESAMPLE_METROPOLIS ? (resample->mh_steps < 1 || resample->mh_steps > dlm::DLM_PF_MAX_MH_STEPS) : resample->mh_steps != 0)
          return fail(e, DLM_ERR_ARG, "mh_steps: 1 .. 64 under DLM_RESAMPLE_METROPOLIS, 0 under every other scheme");
        return (int)DLM_OK;
      }))) return rc;
  HIP_TRY(e, hipSetDevice(e->device));
  const size_t lds = dlm::pf_lds_bytes(d, P), have = dlm::lds_limit();
  if (have && lds > have) return fail(e, DLM_ERR_UNSUPPORTED, "d and n_particles need more LDS than a workgroup of this device gets: (d + 2.5) n_particles + d^2 doubles");
  dlm::PfSchemeArgs a{};
  const size_t n = model->N, dd = d;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  pf_stage(st, a, model, params, pf->family, pf->literal, pf->n0, P, params->V, obs_param, y, opts, iteration, ll, mean, ess, cloud, weights, status);
  st.in(&a.W, params->W, params->w_stride ? (n - 1) * (size_t)params->w_stride + dd * dd : dd * dd);
  a.w_stride = params->w_stride;
  a.resample = resample->scheme; a.mh_steps = resample->mh_steps;
  if ((rc = st.commit())) return rc;
  e->variant = "pf-wave";
  HIP_TRY(e, dlm::launch_pf(a, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_pf_forecast_particles(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params, const dlm_pf_forecast_desc* fc,
                          const double* obs_param, const int32_t* ranks, const double* cloud0, const double* weights0, const double* y,
                          uint64_t iteration, const dlm_options* opts, double* fmean, double* fquant, double* draws, double* ll,
                          double* mean, double* cloud, double* weights, int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  if (!model || !params || !fc) return fail(e, DLM_ERR_ARG, "null descriptor");
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  const int d = model->d, P = fc->n_particles;
  if ((rc = pf_check(e, model, params, fc->family, fc->literal, P, obs_param, y, ll, "the particle forecast", true, true, [&] {
        if (fc->n_ranks < 0 || fc->n_ranks > 8) return fail(e, DLM_ERR_ARG, "n_ranks: 0 .. 8 order statistics per time");
        if (fc->n_ranks && (!ranks || !fquant)) return fail(e, DLM_ERR_ARG, "n_ranks > 0 needs ranks and fquant");
        for (int j = 0; j < fc->n_ranks; ++j)
          if (ranks[j] < 0 || ranks[j] >= P) return fail(e, DLM_ERR_ARG, "a rank must satisfy 0 <= rank < n_particles");
        if (!fmean) return fail(e, DLM_ERR_ARG, "fmean is required");
        if (weights0 && !cloud0) return fail(e, DLM_ERR_ARG, "weights0 needs cloud0");
        if (fc->slot_offset < 0) return fail(e, DLM_ERR_ARG, "slot_offset must be >= 0");
        return (int)DLM_OK;
      }))) return rc;
  if (fc->slot_offset > (int64_t)dlm::DLM_PF_MAX_T - model->T)
    return fail(e, DLM_ERR_UNSUPPORTED, "slot_offset + T must stay below 2^21 - 1 (the Philox counter's slot field)");
  HIP_TRY(e, hipSetDevice(e->device));
  const size_t lds = dlm::pf_lds_bytes(d, P), have = dlm::lds_limit();
  if (have && lds > have) return fail(e, DLM_ERR_UNSUPPORTED, "d and n_particles need more LDS than a workgroup of this device gets: (d + 2.5) n_particles + d^2 doubles");
  dlm::PfForecastArgs a{};
  const size_t n = model->N, t = model->T, dd = d, np = P;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  pf_stage(st, a, model, params, fc->family, fc->literal, P + 1, P, params->V, obs_param, y, opts, iteration, ll, mean, nullptr, cloud, weights, status);
  st.in(&a.W, params->W, params->w_stride ? (n - 1) * (size_t)params->w_stride + dd * dd : dd * dd);
  a.w_stride = params->w_stride;
  st.in(&a.cloud0, cloud0, cloud0 ? n * dd * np : 0);
  st.in(&a.weights0, weights0, weights0 ? n * np : 0);
  st.out(&a.fmean, fmean, n * t);
  st.out(&a.fquant, fc->n_ranks ? fquant : nullptr, n * t * (size_t)fc->n_ranks);
  st.out(&a.draws, draws, draws ? n * t * np : 0);
  a.slot_offset = (int)fc->slot_offset;
  a.n_ranks = fc->n_ranks;
  for (int j = 0; j < fc->n_ranks; ++j) a.ranks[j] = ranks[j];   // a host array whatever opts->mem: checked above, passed by value
  if ((rc = st.commit())) return rc;
  e->variant = "pf-forecast-wave";
  HIP_TRY(e, dlm::launch_pf_forecast(a, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_storvik_batch(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params, const dlm_storvik_desc* sv,
                      const double* prior_v, int64_t prior_v_stride, const double* prior_w, int64_t prior_w_stride,
                      const double* obs_param, const double* y, uint64_t iteration, const dlm_options* opts, double* ll, double* mean,
                      double* ess, double* scale_mean, double* cloud, double* weights, double* scales, int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  if (!model || !params || !sv) return fail(e, DLM_ERR_ARG, "null descriptor");
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  const int d = model->d, P = sv->n_particles;
  if ((rc = pf_check(e, model, params, sv->family, sv->literal, P, obs_param, y, ll, "the Storvik filter", !sv->learn_v, false, [&] {
        if (sv->learn_v != 0 && sv->learn_v != 1) return fail(e, DLM_ERR_ARG, "learn_v: 0 or 1");
        if (sv->learn_v && sv->family != DLM_OBS_GAUSSIAN) return fail(e, DLM_ERR_ARG, "learn_v = 1 needs DLM_OBS_GAUSSIAN: the InverseGamma statistic of V is conjugate for the Gaussian family only (the others learn W alone)");
        return pf_check_priors(e, params, d, sv->learn_v, prior_v, prior_v_stride, prior_w, prior_w_stride);
      }))) return rc;
  HIP_TRY(e, hipSetDevice(e->device));
  const size_t lds = dlm::storvik_lds_bytes(d, P), have = dlm::lds_limit();
  if (have && lds > have) return fail(e, DLM_ERR_UNSUPPORTED, "d and n_particles need more LDS than a workgroup of this device gets: (2 d + 3.5) n_particles + d^2 doubles");
  dlm::StorvikArgs a{};
  const size_t n = model->N, t = model->T, dd = d, np = P;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  pf_stage(st, a, model, params, sv->family, sv->literal, sv->n0, P, sv->learn_v ? nullptr : params->V, obs_param, y, opts, iteration, ll, mean, ess, cloud, weights, status);
  pf_stage_priors(st, a, sv->learn_v, prior_v, prior_v_stride, prior_w, prior_w_stride);
  st.out(&a.scale_mean, scale_mean, scale_mean ? n * t * (dd + 1) : 0);
  st.out(&a.scales, scales, scales ? n * (dd + 1) * np : 0);
  if ((rc = st.commit())) return rc;
  e->variant = "storvik-wave";
  HIP_TRY(e, dlm::launch_storvik(a, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_lw_batch(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params, const dlm_lw_desc* lw,
                 const double* prior_v, int64_t prior_v_stride, const double* prior_w, int64_t prior_w_stride,
                 const double* obs_param, const double* y, uint64_t iteration, const dlm_options* opts, double* ll, double* mean,
                 double* ess, double* psi_mean, double* psi_var, double* cloud, double* weights, double* psi, int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  if (!model || !params || !lw) return fail(e, DLM_ERR_ARG, "null descriptor");
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  const int d = model->d, P = lw->n_particles;
  if ((rc = pf_check(e, model, params, lw->family, lw->literal, P, obs_param, y, ll, "the Liu-West filter", !lw->learn_v, false, [&] {
        if (lw->learn_v != 0 && lw->learn_v != 1) return fail(e, DLM_ERR_ARG, "learn_v: 0 or 1");
        if (!(lw->a > 0.0 && lw->a <= 1.0)) return fail(e, DLM_ERR_ARG, "a: the shrinkage must satisfy 0 < a <= 1");
        if (lw->learn_v && lw->family != DLM_OBS_GAUSSIAN && lw->family != DLM_OBS_STUDENTT && lw->family != DLM_OBS_BETA)
          return fail(e, DLM_ERR_ARG, "learn_v = 1 needs DLM_OBS_GAUSSIAN, DLM_OBS_STUDENTT or DLM_OBS_BETA: the families whose v is a positive scale");
        return pf_check_priors(e, params, d, lw->learn_v, prior_v, prior_v_stride, prior_w, prior_w_stride);
      }))) return rc;
  HIP_TRY(e, hipSetDevice(e->device));
  const size_t lds = dlm::lw_lds_bytes(d, P), have = dlm::lds_limit();
  if (have && lds > have) return fail(e, DLM_ERR_UNSUPPORTED, "d and n_particles need more LDS than a workgroup of this device gets: (2 d + 3.5) n_particles + d^2 + d + 1 doubles");
  dlm::LwArgs a{};
  const size_t n = model->N, t = model->T, dd = d, np = P;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  pf_stage(st, a, model, params, lw->family, lw->literal, lw->n0, P, lw->learn_v ? nullptr : params->V, obs_param, y, opts, iteration, ll, mean, ess, cloud, weights, status);
  pf_stage_priors(st, a, lw->learn_v, prior_v, prior_v_stride, prior_w, prior_w_stride);
  st.out(&a.psi_mean, psi_mean, psi_mean ? n * t * (dd + 1) : 0);
  st.out(&a.psi_var, psi_var, psi_var ? n * t * (dd + 1) : 0);
  st.out(&a.psi, psi, psi ? n * (dd + 1) * np : 0);
  a.a = lw->a;
  if ((rc = st.commit())) return rc;
  e->variant = "lw-wave";
  HIP_TRY(e, dlm::launch_lw(a, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_rb_batch(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params, const dlm_rb_desc* rb,
                 const double* prior_v, int64_t prior_v_stride, const double* prior_w, int64_t prior_w_stride,
                 const double* y, uint64_t iteration, const dlm_options* opts, double* ll, double* mean, double* cov,
                 double* ess, double* psi_mean, double* psi_var, double* means, double* covs, double* weights, double* psi,
                 int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  if (!model || !params || !rb) return fail(e, DLM_ERR_ARG, "null descriptor");
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  const int d = model->d, P = rb->n_particles;
  if ((rc = pf_check(e, model, params, DLM_OBS_GAUSSIAN, rb->literal, P, nullptr, y, ll, "the Rao-Blackwellised filter", !rb->learn_v, false, [&] {
        if (rb->learn_v != 0 && rb->learn_v != 1) return fail(e, DLM_ERR_ARG, "learn_v: 0 or 1");
        if (!(rb->a > 0.0 && rb->a <= 1.0)) return fail(e, DLM_ERR_ARG, "a: the shrinkage must satisfy 0 < a <= 1");
        return pf_check_priors(e, params, d, rb->learn_v, prior_v, prior_v_stride, prior_w, prior_w_stride);
      }))) return rc;
  HIP_TRY(e, hipSetDevice(e->device));
  const size_t lds = dlm::rb_lds_bytes(d, P), have = dlm::lds_limit();
  if (have && lds > have) return fail(e, DLM_ERR_UNSUPPORTED, "d and n_particles need more LDS than a workgroup of this device gets: (d (d + 1) / 2 + 2 d + 3.5) n_particles + 32 d (d + 1) + 3 d + 1 doubles");
  dlm::RbArgs a{};
  const size_t n = model->N, t = model->T, dd = d, np = P;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  pf_stage(st, a, model, params, DLM_OBS_GAUSSIAN, rb->literal, rb->n0, P, rb->learn_v ? nullptr : params->V, nullptr, y, opts, iteration, ll, mean, ess, means, weights, status);
  pf_stage_priors(st, a, rb->learn_v, prior_v, prior_v_stride, prior_w, prior_w_stride);
  st.out(&a.cov, cov, cov ? n * t * dd * dd : 0);
  st.out(&a.psi_mean, psi_mean, psi_mean ? n * t * (dd + 1) : 0);
  st.out(&a.psi_var, psi_var, psi_var ? n * t * (dd + 1) : 0);
  st.out(&a.covs, covs, covs ? n * (dd * (dd + 1) / 2) * np : 0);
  st.out(&a.psi, psi, psi ? n * (dd + 1) * np : 0);
  a.a = rb->a;
  if ((rc = st.commit())) return rc;
  e->variant = "rb-wave";
  HIP_TRY(e, dlm::launch_rb(a, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_pf_forecast_learned(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params, const dlm_pf_forecast_learned_desc* fc,
                            const double* obs_param, const int32_t* ranks, const double* cloud0, const double* weights0, const double* pw,
                            const double* pv, const double* shapes, int64_t shapes_stride, uint64_t iteration, const dlm_options* opts,
                            double* fmean, double* fquant, double* draws, double* mean, double* cloud, double* var_w, double* var_v,
                            int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  if (!model || !params || !fc) return fail(e, DLM_ERR_ARG, "null descriptor");
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  const int d = model->d, T = model->T, N = model->N, P = fc->n_particles, family = fc->family;
  if (d < 1 || model->p < 1 || T < 1 || N < 1) return fail(e, DLM_ERR_ARG, "d, p, T, N must be >= 1");
  if (!model->F || !model->G || model->n_g < 1) return fail(e, DLM_ERR_ARG, "model tables F/G missing");
  if (model->n_g > 1 && !model->g_index) return fail(e, DLM_ERR_ARG, "n_g > 1 needs g_index");
  if (model->f_stride != 0 && model->f_stride != (int64_t)d * model->p) return fail(e, DLM_ERR_ARG, "f_stride must be 0 or d*p");
  if (family < DLM_OBS_GAUSSIAN || family > DLM_OBS_BETA) return fail(e, DLM_ERR_ARG, "family: one of DLM_OBS_*");
  if (fc->var_kind != DLM_FC_VAR && fc->var_kind != DLM_FC_LOGVAR && fc->var_kind != DLM_FC_IG_SCALE) return fail(e, DLM_ERR_ARG, "var_kind: one of DLM_FC_*");
  if (!cloud0 || !pw) return fail(e, DLM_ERR_ARG, "cloud0 and pw are required: the particles carry their own variances");
  if (!fmean) return fail(e, DLM_ERR_ARG, "fmean is required");
  if (fc->var_kind == DLM_FC_IG_SCALE && !shapes) return fail(e, DLM_ERR_ARG, "DLM_FC_IG_SCALE needs shapes (the InverseGamma shapes of the d + 1 components)");
  if (shapes_stride != 0 && shapes_stride < (int64_t)d + 1) return fail(e, DLM_ERR_ARG, "shapes_stride must be 0 or >= d + 1");
  if (pv && fc->var_kind != DLM_FC_VAR && (family == DLM_OBS_NEGBIN || family == DLM_OBS_ZIP))
    return fail(e, DLM_ERR_ARG, "pv of DLM_OBS_NEGBIN and DLM_OBS_ZIP is no variance (a log size, a logit): DLM_FC_VAR only");
  if (!pv && !params->V) return fail(e, DLM_ERR_ARG, "pv == NULL needs params->V");
  if (!pv && params->v_tstride) return fail(e, DLM_ERR_ARG, "the learned forecast takes a time-invariant V (v_tstride = 0)");
  if (fc->n_ranks < 0 || fc->n_ranks > 8) return fail(e, DLM_ERR_ARG, "n_ranks: 0 .. 8 order statistics per time");
  if (fc->n_ranks && (!ranks || !fquant)) return fail(e, DLM_ERR_ARG, "n_ranks > 0 needs ranks and fquant");
  for (int j = 0; j < fc->n_ranks; ++j)
    if (ranks[j] < 0 || ranks[j] >= P) return fail(e, DLM_ERR_ARG, "a rank must satisfy 0 <= rank < n_particles");
  if (fc->slot_offset < 0) return fail(e, DLM_ERR_ARG, "slot_offset must be >= 0");
  if (family == DLM_OBS_STUDENTT && !obs_param) return fail(e, DLM_ERR_ARG, "DLM_OBS_STUDENTT needs obs_param (the degrees of freedom of every series)");
  if (model->p != 1) return fail(e, DLM_ERR_UNSUPPORTED, "the learned forecast takes a univariate observation (p = 1): every Dglm family reads y(0) and V(0,0)");
  if (d > dlm::DLM_PF_MAX_D) return fail(e, DLM_ERR_UNSUPPORTED, "the learned forecast takes d <= 16");
  if (P < 64 || P > dlm::DLM_PF_MAX_P || P % 64 != 0) return fail(e, DLM_ERR_UNSUPPORTED, "n_particles must be a multiple of 64 with 64 <= n_particles <= 1024 (one wavefront per series, whole slots of particles)");
  if (T > dlm::DLM_PF_MAX_T || fc->slot_offset > (int64_t)dlm::DLM_PF_MAX_T - T)
    return fail(e, DLM_ERR_UNSUPPORTED, "slot_offset + T must stay below 2^21 - 1 (the Philox counter's slot field)");
  HIP_TRY(e, hipSetDevice(e->device));
  const size_t lds = dlm::pf_forecast_learned_lds_bytes(d, P), have = dlm::lds_limit();
  if (have && lds > have) return fail(e, DLM_ERR_UNSUPPORTED, "d and n_particles need more LDS than a workgroup of this device gets: (2 d + 3.5) n_particles doubles");
  dlm::PfForecastLearnedArgs a{};
  const size_t n = N, t = T, dd = d, np = P;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  st.in(&a.F, model->F, (model->f_stride ? t : 1) * dd);
  st.in(&a.G, model->G, (size_t)model->n_g * dd * dd);
  st.in(&a.g_index, (const int*)model->g_index, model->g_index ? t : 0);
  st.in(&a.dt, model->dt, model->dt ? t : 0);
  st.in(&a.V, pv ? nullptr : params->V, params->v_stride ? (n - 1) * (size_t)params->v_stride + 1 : 1);
  st.in(&a.obs_param, obs_param, obs_param ? n : 0);
  st.in(&a.cloud0, cloud0, n * dd * np);
  st.in(&a.weights0, weights0, weights0 ? n * np : 0);
  st.in(&a.pw, pw, n * dd * np);
  st.in(&a.pv, pv, pv ? n * np : 0);
  const bool ig = fc->var_kind == DLM_FC_IG_SCALE;
  st.in(&a.shapes, ig ? shapes : nullptr, shapes_stride ? (n - 1) * (size_t)shapes_stride + dd + 1 : dd + 1);
  st.out(&a.fmean, fmean, n * t);
  st.out(&a.fquant, fc->n_ranks ? fquant : nullptr, n * t * (size_t)fc->n_ranks);
  st.out(&a.draws, draws, draws ? n * t * np : 0);
  st.out(&a.mean, mean, mean ? n * t * dd : 0);
  st.out(&a.cloud, cloud, cloud ? n * dd * np : 0);
  st.out(&a.var_w, var_w, var_w ? n * dd * np : 0);
  st.out(&a.var_v, var_v, var_v ? n * np : 0);
  st.zeroed_out(&a.status, (int*)status, status ? n : 0);
  a.d = d; a.T = T; a.N = N; a.P = P;
  a.family = family; a.var_kind = fc->var_kind;
  a.f_stride = model->f_stride; a.n_g = model->n_g; a.v_stride = params->v_stride; a.shapes_stride = shapes_stride;
  a.rs = draw_stream(opts, iteration);
  a.slot_offset = (int)fc->slot_offset;
  a.n_ranks = fc->n_ranks;
  for (int j = 0; j < fc->n_ranks; ++j) a.ranks[j] = ranks[j];   // a host array whatever opts->mem: checked above, passed by value
  if ((rc = st.commit())) return rc;
  e->variant = "pf-forecast-learned-wave";
  HIP_TRY(e, dlm::launch_pf_forecast_learned(a, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_rb_state_draw(dlm_engine* e, int32_t d, int32_t N, int32_t P, const double* means, const double* covs, int64_t slot,
                      uint64_t iteration, const dlm_options* opts, double* cloud, int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  if (d < 1 || N < 1) return fail(e, DLM_ERR_ARG, "d, N must be >= 1");
  if (!means || !covs || !cloud) return fail(e, DLM_ERR_ARG, "means, covs and cloud are required");
  if (slot < 0 || slot > (int64_t)dlm::DLM_SLOT_TOP) return fail(e, DLM_ERR_ARG, "slot must satisfy 0 <= slot <= 2^21 - 1 (the Philox counter's slot field)");
  if (d > dlm::DLM_PF_MAX_D) return fail(e, DLM_ERR_UNSUPPORTED, "the state draw takes d <= 16");
  if (P < 64 || P > dlm::DLM_PF_MAX_P || P % 64 != 0) return fail(e, DLM_ERR_UNSUPPORTED, "n_particles must be a multiple of 64 with 64 <= n_particles <= 1024 (one wavefront per series, whole slots of particles)");
  HIP_TRY(e, hipSetDevice(e->device));
  dlm::RbStateDrawArgs a{};
  const size_t n = N, dd = d, np = P;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  st.in(&a.means, means, n * dd * np);
  st.in(&a.covs, covs, n * (dd * (dd + 1) / 2) * np);
  st.out(&a.cloud, cloud, n * dd * np);
  st.zeroed_out(&a.status, (int*)status, status ? n : 0);
  a.d = d; a.N = N; a.P = P;
  a.rs = draw_stream(opts, iteration);
  a.slot = (unsigned)slot;
  if ((rc = st.commit())) return rc;
  e->variant = "rb-state-draw";
  HIP_TRY(e, dlm::launch_rb_state_draw(a, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_sv_paths(dlm_engine* e, int32_t N, int32_t k, int32_t H, int32_t R, const double* sv, const double* alpha0, uint64_t iteration,
                 const dlm_options* opts, double* alpha, int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  if (N < 1 || H < 1) return fail(e, DLM_ERR_ARG, "N >= 1 and H >= 1");
  if (H > dlm::DLM_SVPATH_MAX_H) return fail(e, DLM_ERR_ARG, "H must stay at or below 2^21 - 1 (the Philox counter's slot field)");
  if (k < 1 || k > dlm::DLM_FSV_MAX_K) return fail(e, DLM_ERR_UNSUPPORTED, "1 <= k <= 8");
  if (R < 64 || R > dlm::DLM_SVPATH_MAX_R || R % 64 != 0) return fail(e, DLM_ERR_UNSUPPORTED, "n_paths must be a multiple of 64 with 64 <= n_paths <= 1024 (one lane per path, the path in the counter's attempt field)");
  if ((long long)N * (R / 64) > 0x7FFFFFFFll) return fail(e, DLM_ERR_ARG, "N n_paths / 64 must stay below 2^31 (one block per 64 paths of a row)");
  if (!sv || !alpha) return fail(e, DLM_ERR_ARG, "sv and alpha are required");
  HIP_TRY(e, hipSetDevice(e->device));
  dlm::SvPathsArgs a{};
  const size_t n = N, kk = k, h = H, r = R;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  st.in(&a.sv, sv, n * kk * 3);
  st.in(&a.alpha0, alpha0, alpha0 ? n * kk : 0);
  st.out(&a.alpha, alpha, n * r * kk * (h + 1));
  st.zeroed_out(&a.status, (int*)status, status ? n : 0);
  if ((rc = st.commit())) return rc;
  a.N = N; a.k = k; a.H = H; a.R = R;
  a.rs = draw_stream(opts, iteration);
  e->variant = "sv-paths";
  HIP_TRY(e, dlm::launch_sv_paths(a, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_gaussian_mixture_summary(dlm_engine* e, const dlm_mixture_desc* mx, const double* f, const double* Q, const double* probs,
                                 const dlm_options* opts, double* mean, double* cov, double* quant, int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  if (!mx) return fail(e, DLM_ERR_ARG, "null descriptor");
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  const int N = mx->N, C = mx->C, H = mx->H, p = mx->p, nq = mx->nq;
  if (N < 1 || C < 1 || H < 1 || p < 1) return fail(e, DLM_ERR_ARG, "N, C, H, p must be >= 1");
  if (p > dlm::DLM_MIX_MAX_P) return fail(e, DLM_ERR_UNSUPPORTED, "p is limited to 64");
  if (C > dlm::DLM_MIX_MAX_C) return fail(e, DLM_ERR_ARG, "C must stay at or below 2^30 (the kernels index a row's components with an int)");
  if (nq < 0 || nq > dlm::DLM_MIX_MAX_NQ) return fail(e, DLM_ERR_ARG, "0 <= nq <= 8 quantiles per cell");
  if (nq > 0 && (!probs || !quant)) return fail(e, DLM_ERR_ARG, "probs and quant are required with nq > 0");
  for (int j = 0; j < nq; ++j)
    if (!(probs[j] > 0.0 && probs[j] < 1.0)) return fail(e, DLM_ERR_ARG, "every prob must lie inside (0, 1)");
  if (!Q || !mean || !cov) return fail(e, DLM_ERR_ARG, "Q, mean and cov are required");
  const int64_t strides[6] = {mx->f_nstride, mx->f_cstride, mx->f_tstride, mx->q_nstride, mx->q_cstride, mx->q_tstride};
  for (int j = f ? 0 : 3; j < 6; ++j)
    if (strides[j] < 0) return fail(e, DLM_ERR_ARG, "the strides must not be negative");
  if ((long long)N * H * p > 0x7FFFFFFFll) return fail(e, DLM_ERR_ARG, "N H p must stay below 2^31 (one block per cell)");
  HIP_TRY(e, hipSetDevice(e->device));
  dlm::MixtureArgs a{};
  const size_t n = N, c = C, h = H, pp = p;
  // what the strides reach: the last component of the last row at the last time, and its p (p p) doubles
  const size_t f_extent = (n - 1) * (size_t)mx->f_nstride + (c - 1) * (size_t)mx->f_cstride + (h - 1) * (size_t)mx->f_tstride + pp;
  const size_t q_extent = (n - 1) * (size_t)mx->q_nstride + (c - 1) * (size_t)mx->q_cstride + (h - 1) * (size_t)mx->q_tstride + pp * pp;
  // host memory, f and Q inside one buffer (the fq records): one staged range serves both
  const bool one_range = opts->mem == DLM_MEM_HOST && f && Q >= f && (size_t)(Q - f) < f_extent;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  if (one_range) {
    st.in(&a.f, f, std::max(f_extent, (size_t)(Q - f) + q_extent));
  } else {
    st.in(&a.f, f, f ? f_extent : 0);
    st.in(&a.Q, Q, q_extent);
  }
  st.out(&a.mean, mean, n * h * pp);
  st.out(&a.cov, cov, n * h * pp * pp);
  st.out(&a.quant, quant, nq ? n * h * pp * (size_t)nq : 0);
  st.zeroed_out(&a.status, (int*)status, status ? n : 0);
  if ((rc = st.commit())) return rc;
  if (one_range) a.Q = a.f + (Q - f);
  a.N = N; a.C = C; a.H = H; a.p = p; a.nq = nq;
  a.f_nstride = mx->f_nstride; a.f_cstride = mx->f_cstride; a.f_tstride = mx->f_tstride;
  a.q_nstride = mx->q_nstride; a.q_cstride = mx->q_cstride; a.q_tstride = mx->q_tstride;
  for (int j = 0; j < nq; ++j) a.probs[j] = probs[j];   // a host array whatever opts->mem: checked above, passed by value
  e->variant = "mixture-summary";
  HIP_TRY(e, dlm::launch_mixture_moments(a, e->stream));
  if (nq > 0) {
    // beyond DLM_MIX_LDS_C components a cell's pairs live in the engine's workspace: launches of whole cells under the cap
    const size_t cells = n * h * pp, per_cell = c * 2 * sizeof(double);
    size_t chunk = cells;
    if (C > dlm::DLM_MIX_LDS_C) {
      chunk = std::max<size_t>(1, std::min<size_t>(cells, (size_t)DLM_MIXTURE_WORKSPACE_CAP / per_cell));
      if ((rc = ensure(e, e->mixws, chunk * per_cell))) return rc;
      a.pack = e->mixws;
    }
    for (size_t first = 0; first < cells; first += chunk) {
      a.cell_first = (int)first;
      HIP_TRY(e, dlm::launch_mixture_quantiles(a, (int)std::min(chunk, cells - first), e->stream));
    }
  }
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_pg_batch(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params, const dlm_pg_desc* pg,
                 const double* obs_param, const double* y, const double* ref, uint64_t iteration, const dlm_options* opts,
                 double* ll, double* path, double* stats, int32_t* path_index, double* clouds, int32_t* ancestors,
                 double* step_weights, int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  if (!model || !params || !pg) return fail(e, DLM_ERR_ARG, "null descriptor");
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  const int d = model->d, P = pg->n_particles;
  if ((rc = pf_check(e, model, params, pg->family, 0, P, obs_param, y, ll, "particle Gibbs", true, true, [&] {
        if (pg->ancestor_sampling != 0 && pg->ancestor_sampling != 1) return fail(e, DLM_ERR_ARG, "ancestor_sampling: 0 or 1");
        if (pg->workspace_cap < 0) return fail(e, DLM_ERR_ARG, "workspace_cap: bytes, or 0 for DLM_PG_WORKSPACE_CAP");
        if (!ref || !path || !stats) return fail(e, DLM_ERR_ARG, "ref, path and stats are required");
        if ((clouds == nullptr) != (ancestors == nullptr)) return fail(e, DLM_ERR_ARG, "clouds and ancestors are given together or not at all");
        return (int)DLM_OK;
      }))) return rc;
  HIP_TRY(e, hipSetDevice(e->device));
  const size_t lds = dlm::pg_lds_bytes(d, P), have = dlm::lds_limit();
  if (have && lds > have) return fail(e, DLM_ERR_UNSUPPORTED, "d and n_particles need more LDS than a workgroup of this device gets: (d + 2.5) n_particles + d^2 + d doubles");
  dlm::PgArgs a{};
  const size_t n = model->N, t = model->T, dd = d, np = P;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  pf_stage(st, a, model, params, pg->family, 0, 0, P, params->V, obs_param, y, opts, iteration, ll, nullptr, nullptr, nullptr, nullptr, status);
  st.in(&a.W, params->W, params->w_stride ? (n - 1) * (size_t)params->w_stride + dd * dd : dd * dd);
  a.w_stride = params->w_stride;
  a.ancestor_sampling = pg->ancestor_sampling;
  st.in(&a.ref, ref, n * (t + 1) * dd);
  st.out(&a.path, path, n * (t + 1) * dd);
  st.out(&a.stats, stats, n * (dd + 3));
  st.out(&a.path_index, (int*)path_index, path_index ? n * (t + 1) : 0);
  st.out(&a.clouds, clouds, clouds ? n * (t + 1) * dd * np : 0);
  st.out(&a.ancestors, (int*)ancestors, ancestors ? n * t * np : 0);
  st.out(&a.step_weights, step_weights, step_weights ? n * t * np : 0);
  if ((rc = st.commit())) return rc;
  // the clouds and ancestors of every step: the caller's arrays, or the engine's workspace in launches of whole series under the cap
  const size_t cloud_doubles = (t + 1) * dd * np, anc_ints = t * np;
  const size_t per_series = cloud_doubles * sizeof(double) + anc_ints * sizeof(int);
  size_t chunk = n;
  if (!clouds) {
    const size_t cap = pg->workspace_cap ? (size_t)pg->workspace_cap : (size_t)DLM_PG_WORKSPACE_CAP;
    chunk = std::max<size_t>(1, std::min<size_t>(n, cap / per_series));
    if ((rc = ensure(e, e->pgws, chunk * per_series))) return rc;
    a.clouds = (double*)e->pgws.p;
    a.ancestors = (int*)(a.clouds + chunk * cloud_doubles);
  }
  e->variant = "pg-wave";
  for (size_t first = 0; first < n; first += chunk) {
    a.n_first = (int)first;
    HIP_TRY(e, dlm::launch_pg(a, (int)std::min(chunk, n - first), e->stream));
  }
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

static int ar1_common(dlm_engine* e, int32_t N, int32_t T, const double* times, bool ou, const double* y, const double* v,
                      int64_t v_stride, const double* sv, int64_t sv_stride, const double* z, const dlm_options* opts,
                      double* filt, double* theta, int32_t* status);

int dlm_ar1_ffbs_batch(dlm_engine* e, int32_t N, int32_t T, const double* y, const double* v, int64_t v_stride,
                       const double* sv, int64_t sv_stride, const double* z, const dlm_options* opts,
                       double* filt, double* theta, int32_t* status) {
  return ar1_common(e, N, T, nullptr, false, y, v, v_stride, sv, sv_stride, z, opts, filt, theta, status);
}

int dlm_ou_ffbs_batch(dlm_engine* e, int32_t N, int32_t T, const double* times, const double* y, const double* v,
                      int64_t v_stride, const double* sv, int64_t sv_stride, const double* z, const dlm_options* opts,
                      double* filt, double* theta, int32_t* status) {
  if (e && !times) return fail(e, DLM_ERR_ARG, "times are required");
  return ar1_common(e, N, T, times, true, y, v, v_stride, sv, sv_stride, z, opts, filt, theta, status);
}

static int ar1_common(dlm_engine* e, int32_t N, int32_t T, const double* times, bool ou, const double* y, const double* v,
                      int64_t v_stride, const double* sv, int64_t sv_stride, const double* z, const dlm_options* opts,
                      double* filt, double* theta, int32_t* status) {
  if (!e) return DLM_ERR_ARG;
  int rc;
  if ((rc = check_opts(e, opts))) return rc;
  if (N < 1 || T < 1) return fail(e, DLM_ERR_ARG, "N and T must be >= 1 (the reference throws on empty input, FilterAr.scala:40)");
  if (!y || !v || !sv) return fail(e, DLM_ERR_ARG, "y, v and sv are required");
  if (!filt && !theta) return fail(e, DLM_ERR_ARG, "nothing to compute: filt and theta are both NULL");
  if ((v_stride != 0 && v_stride != T) || (sv_stride != 0 && sv_stride != 3)) return fail(e, DLM_ERR_ARG, "v_stride must be 0 or T, sv_stride 0 or 3");
  HIP_TRY(e, hipSetDevice(e->device));
  struct { const double *times, *y, *v, *sv, *z; double *filt, *theta; int* status; } k{};
  const size_t n = N, t = T;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  st.in(&k.times, times, ou ? t : 0);
  st.in(&k.y, y, n * t);
  st.in(&k.v, v, v_stride ? n * t : t);
  st.in(&k.sv, sv, sv_stride ? n * 3 : 3);
  st.in(&k.z, z, z ? n * (t + 1) : 0);
  st.out(&k.filt, filt, filt ? n * (t + 1) * 2 : 0);
  st.out(&k.theta, theta, theta ? n * (t + 1) : 0);
  st.zeroed_out(&k.status, (int*)status, status ? n : 0);
  if ((rc = st.commit())) return rc;
  double* fws = k.filt;
  if (!fws) {   // the backward sampler reads the filter records: engine scratch when the caller does not want them
    if ((rc = ensure_side(e, n, t))) return rc;
    fws = e->side;
  }
  e->variant = ou ? "ou-lane" : "ar1-lane";
  HIP_TRY(e, dlm::launch_ar1_ffbs(N, T, k.times, k.y, k.v, v_stride, k.sv, sv_stride, k.z, opts->seed, opts->series_offset, fws,
                                  k.theta, k.status, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_loglik_batch(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params,
                     const double* y, const dlm_options* opts, double* loglik, int32_t* status) {
  int rc = check_common(e, model, params, opts);
  if (rc) return rc;
  if (!y || !loglik) return fail(e, DLM_ERR_ARG, "y and loglik are required");
  const size_t p = model->p, T = model->T, N = model->N;
  KArgs k{};
  Stager st(e, opts->mem == DLM_MEM_HOST);
  stage_model(st, k, model, params, opts);
  st.in(&k.y, y, N * T * p);
  st.out(&k.loglik, loglik, N);
  st.zeroed_out(&k.status, (int*)status, N);
  if ((rc = st.commit())) return rc;
  if ((rc = analyse_g(e, k, model->G, opts->mem == DLM_MEM_HOST))) return rc;
  if (opts->flags & DLM_OPT_LOGLIK_LITERAL_Q7) {
    // KalmanFilter.likelihood as written (KalmanFilter.scala:299-306): filter into a workspace, then the transition density of
    // the filtered means (dlm_loglik.hip)
    if (params->w_tstride) return fail(e, DLM_ERR_UNSUPPORTED, "DLM_OPT_LOGLIK_LITERAL_Q7 takes a time-invariant W (KalmanFilter.likelihood is given p.w)");
    const size_t d = model->d, rec = d + d * d;
    const size_t recs = N * (T + 1) * rec * sizeof(double), wsb = dlm::loglik_q7_ws_bytes(k);
    if ((rc = ensure(e, e->fws, recs + wsb))) return rc;
    double* ll_out = k.loglik;
    k.filt = e->fws; k.loglik = nullptr;
    if ((rc = run_filter(e, k, false))) return rc;
    k.loglik = ll_out;
    HIP_TRY(e, dlm::launch_loglik_q7(k, e->fws, (char*)e->fws.p + recs, e->stream));
    return st.finish(opts->flags & DLM_OPT_ASYNC);
  }
  if ((rc = run_filter(e, k, false))) return rc;   // k.filt == nullptr: the forward kernels store nothing
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_smooth_batch(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params,
                     const double* filt, const dlm_options* opts, double* smooth, int32_t* status) {
  int rc = check_common(e, model, params, opts);
  if (rc) return rc;
  if (!filt || !smooth) return fail(e, DLM_ERR_ARG, "filt and smooth are required");
  if (opts->flags & DLM_OPT_PACKED_SYM) return fail(e, DLM_ERR_UNSUPPORTED, "DLM_OPT_PACKED_SYM: packed records are read by the fused call only (dlm_filter_smooth_batch); dlm_smooth_batch takes dense records (dlm_unpack_records)");
  const size_t d = model->d, T = model->T, N = model->N, rec = d + d * d;
  KArgs k{};
  Stager st(e, opts->mem == DLM_MEM_HOST);
  stage_model(st, k, model, params, opts);
  st.in(&k.filt_in, filt, N * (T + 1) * rec);
  st.out(&k.smooth, smooth, N * (T + 1) * rec);
  st.zeroed_out(&k.status, (int*)status, N);
  if ((rc = st.commit())) return rc;
  if ((rc = analyse_g(e, k, model->G, opts->mem == DLM_MEM_HOST))) return rc;   // structure tables for the register-tile RTS kernel
  if ((rc = mark(e, 0)) || (rc = mark(e, 1))) return rc;
  if ((rc = run_smoother(e, k, false))) return rc;
  if ((rc = mark(e, 2))) return rc;
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_filter_smooth_batch(dlm_engine* e, const dlm_model_desc* model,
                            const dlm_params_desc* params, const double* y,
                            const dlm_options* opts, double* filt, double* smooth,
                            int32_t* status) {
  int rc = check_common(e, model, params, opts);
  if (rc) return rc;
  if (!y || !smooth) return fail(e, DLM_ERR_ARG, "y and smooth are required");
  e->rts_last = false;
  AuxScope aux(e);   // (the shared-covariance path runs its backward covariance table on the second stream)
  const size_t d = model->d, p = model->p, T = model->T, N = model->N, rec = d + d * d;
  KArgs k{};
  Stager st(e, opts->mem == DLM_MEM_HOST);
  stage_model(st, k, model, params, opts);
  const bool want_packed = (opts->flags & DLM_OPT_PACKED_SYM) != 0;
  const size_t orec = want_packed ? (size_t)dlm_packed_record_doubles((int)d) : rec;
  st.in(&k.y, y, N * T * p);
  st.out(&k.filt, filt, filt ? N * (T + 1) * orec : 0);
  st.out(&k.smooth, smooth, N * (T + 1) * orec);
  st.zeroed_out(&k.status, (int*)status, N);
  if ((rc = st.commit())) return rc;
  if ((rc = analyse_g(e, k, model->G, opts->mem == DLM_MEM_HOST))) return rc;
  if (want_packed && (rc = packed_path(e, k))) return rc;
  bool fused_fast = fast_smoother_ok(e, k) || use_tiled(k);
  if (want_packed) k.packed = 3;   // filtered and smoothed records both leave packed
  // Structured d <= 15 path, V, W, C0 shared by the batch: J_t, S_t of the RTS recursion once per call, every series its mean recursion
  // (k_smoother_rts16 with its export on + k_mean_rts16).  Literal Q1: from 2048 series; textbook: from 6144 series (a caller
  // that does not take the filtered records gets them written to the engine's workspace, dense: the mean kernel reads their first 128 bytes).
  const bool q1 = (k.flags & DLM_OPT_SMOOTHER_COMPAT_Q1) != 0;
  const bool rts_shared = fast_shape_ok(k) && e->sparse_k > 0 && !use_lane(k) && !k.packed && !(k.flags & DLM_OPT_SHARED_COV) &&
                          (q1 ? !fused_fast : fast_smoother_ok(e, k)) && dlm::rts_shared_eligible(k, !q1) &&
                          ((uintptr_t)k.smooth & 15) == 0;   // (the two writers of a smoothed record split it by 16-byte pieces and 128-byte lines)
  // (textbook: the series with a missing observation keep the information-form kernel, k_smoother_sp16, and the forward pass its side records for
  //  them -- the RTS kernel per series is five times slower; literal Q1 has only that kernel)
  if (!filt) {   // smoothed moments only: the filtered records stay in an engine workspace, packed on the structured path
    k.packed |= (fast_smoother_ok(e, k) && e->sparse_k > 0 && !use_lane(k) && !rts_shared) ? 1 : 0;
    if ((rc = ensure(e, e->fws, (k.packed & 1) ? N * (T + 1) * (size_t)dlm::packed_rec_bytes((int)d) : N * (T + 1) * rec * sizeof(double)))) return rc;
    k.filt = e->fws;
  }
  if ((rc = mark(e, 0))) return rc;
  dlm::RtsTabs rtb{};
  if (rts_shared && (rc = start_rts_tables(e, k, rtb))) return rc;
  if (rts_shared && (k.flags & DLM_OPT_TEST_FAIL_AFTER_TABLES))   // test hook: an error exit with the second stream busy
    return fail(e, DLM_ERR_UNSUPPORTED, "DLM_OPT_TEST_FAIL_AFTER_TABLES");
  if ((rc = mark_plain(e, k))) return rc;
  if (filt && fast_smoother_ok(e, k) && use_shared_cov(e, k)) {
    dlm::CovTabs tb;
    if ((rc = run_shared_filter(e, k, tb, true))) return rc;
    if ((rc = mark(e, 1))) return rc;
    k.filt_in = k.filt;
    if ((rc = run_shared_smoother(e, k, tb))) return rc;
    if ((rc = mark(e, 2))) return rc;
    return st.finish(opts->flags & DLM_OPT_ASYNC);
  }
  if ((rc = run_filter(e, k, fused_fast))) return rc;
  if (rts_shared) HIP_TRY(e, hipStreamWaitEvent(e->stream, e->rts_ev, 0));   // the tables (in front of the timing mark: the backward time is the mean kernel's and what the broadcast of S_t has left)
  if ((rc = mark(e, 1))) return rc;
  k.filt_in = k.filt;
  if (rts_shared) {
    k.route = e->route; k.route_take = 0;
    e->variant = "sparse16-rts-shared";
    HIP_TRY(e, dlm::launch_rts_shared_means(k, e->sparse_k, e->sp_dev, rtb, q1, e->stream));
    if (!q1) {
      KArgs kg = k;
      kg.route_take = 1;
      HIP_TRY(e, dlm::launch_sparse16_smoother(kg, e->sparse_k, e->sp_dev, e->side, e->stream));
    }
  } else if ((rc = run_smoother(e, k, fused_fast))) return rc;
  if (rts_shared && (rc = join_cov(e))) return rc;   // the broadcast of S_t
  if ((rc = mark(e, 2))) return rc;
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

// ---- the forward halves of dlm_ffbs_batch, one route each (sampler_common chooses).  The three simulation smoothers (Durbin-Koopman) are
// the whole call: forward and backward pass, both timing marks.
static int simsmooth_lane(dlm_engine* e, KArgs& k) {
  int rc = ensure_xplus(e, k);
  if (rc) return rc;
  e->variant = "lane-simsmooth";
  HIP_TRY(e, dlm::launch_lane_simsmooth(k, e->xplus, e->stream));
  return (rc = mark(e, 1)) ? rc : mark(e, 2);
}
static int simsmooth_sparse16(dlm_engine* e, KArgs& k) {   // the structured d <= 15 path
  int rc;
  if ((rc = ensure_side(e, k.N, k.T)) || (rc = ensure_xplus(e, k))) return rc;
  e->variant = "sparse16-simsmooth";
  HIP_TRY(e, dlm::launch_sparse16_filter(k, e->sparse_k, e->sp_dev, e->side, e->xplus, e->stream));
  if ((rc = mark(e, 1))) return rc;
  k.filt_in = k.filt;
  HIP_TRY(e, dlm::launch_sparse16_simsmooth(k, e->sparse_k, e->sp_dev, e->side, e->xplus, e->stream));
  return mark(e, 2);
}
static int simsmooth_tiled(dlm_engine* e, KArgs& k) {      // per-wave / tiled kernels
  int rc;
  if (k.w_tstride) {   // a W_t stream (DlmFsvSystem.ffbs): the per-wave kernels, whose simulation prologue factors W_t at every step -- at any batch size
    k.flags |= DLM_OPT_FORCE_WAVE;
    if (!dlm::wave48_simsmooth_supported(k))
      return fail(e, DLM_ERR_UNSUPPORTED, "a W_t stream with DLM_OPT_FFBS_SIMSMOOTH needs a structured G (at most four nonzeros per row and column); the reference-form sampler takes any model");
  }
  if ((rc = ensure_xplus(e, k)) || (rc = ensure_ystar(e, k))) return rc;
  e->variant = dlm::wave48_simsmooth_supported(k) ? "wave-simsmooth" : "tiled-simsmooth";
  HIP_TRY(e, dlm::launch_tiled_simsmooth(k, e->xplus, e->ystar, e->stream));
  return (rc = mark(e, 1)) ? rc : mark(e, 2);
}
// No records AND shared factors (d <= 15): nothing of the filtered covariances is needed per series -- the draw kernel reads the
// means, the table is made from the covariance recursion alone.  So the forward pass is section 4.9's: one wave's covariance
// recursion into a table, a mean-only kernel per series (compact means, 128 instead of 1456 bytes per series-step at d = 13);
// the table of factors is made from that covariance table while the mean kernel runs; a series with a missing observation is
// marked by the mean kernel and runs its own filter and sampler on the workspace.
static int forward_shared_means(dlm_engine* e, KArgs& k, dlm::SampTabs& stb) {
  int rc;
  dlm::CovTabs ctb;
  if ((rc = ensure_shared(e, k, ctb, true))) return rc;
  k.route = e->route; k.route_take = 0; k.filt = nullptr;
  HIP_TRY(e, dlm::launch_sparse16_cov_filter(k, e->sparse_k, e->sp_dev, ctb, e->stream));
  if ((rc = start_sampler_tables(e, k, stb, false, ctb.ftab, ctb.frow))) return rc;
  if (k.flags & DLM_OPT_TEST_FAIL_AFTER_TABLES) return fail(e, DLM_ERR_UNSUPPORTED, "DLM_OPT_TEST_FAIL_AFTER_TABLES");
  HIP_TRY(e, dlm::launch_sparse16_mean_filter(k, e->sparse_k, e->sp_dev, ctb, e->stream));
  stb.mc4 = ctb.mc;
  KArgs kg = k;
  kg.route_take = 1; kg.filt = e->fws;
  HIP_TRY(e, dlm::launch_sparse16_filter(kg, e->sparse_k, e->sp_dev, nullptr, nullptr, e->stream));
  k.filt_in = e->fws;
  return DLM_OK;
}
// Every other call: run_filter, with the tables (and normals) of a shared-factor draw started in front of it.  norec_big: 16 <= d <= 48,
// shared factors and no records wanted.
static int forward_records(dlm_engine* e, KArgs& k, dlm::SampTabs& stb, bool shared_factors, bool shared_big, bool norec_big) {
  int rc;
  // (norec_big: the normals start behind the forward pass: 8.64 -> 8.26 ms per C4 Gibbs iteration on one box)
  if ((shared_factors || shared_big) && (rc = start_sampler_tables(e, k, stb, shared_big, nullptr, 0, norec_big))) return rc;
  if ((shared_factors || shared_big) && (k.flags & DLM_OPT_TEST_FAIL_AFTER_TABLES))   // test hook: an error exit with the auxiliary streams busy
    return fail(e, DLM_ERR_UNSUPPORTED, "DLM_OPT_TEST_FAIL_AFTER_TABLES");
  if (norec_big) {
    // the draw kernel reads only the means of the series without a gap, so those series' steady steps store the mean alone
    // (KArgs::keep_cov; the first, full steps still write what the convergence test re-reads)
    HIP_TRY(e, dlm::launch_wave48_mark_gaps(k, e->route, e->stream));
    k.keep_cov = e->route;
    k.ktab = stb.ktab;     // ... and they leave the filter where the recursion settles: k_steady_filter_w48 carries their means on
    k.leave_step = leave_of(e, (size_t)k.N);
    HIP_TRY(e, hipMemsetD32Async((hipDeviceptr_t)k.leave_step, k.T, (size_t)k.N, e->stream));   // T: the series ran the whole filter
    stb.marked = 1;
  }
  if ((rc = run_filter(e, k, false))) return rc;
  if (norec_big) {
    if (!e->rng_gate) HIP_TRY(e, hipEventCreateWithFlags(&e->rng_gate, hipEventDisableTiming));
    HIP_TRY(e, hipEventRecord(e->rng_gate, e->stream));
    if ((rc = start_sampler_normals(e, k, stb, true, e->rng_gate))) return rc;
    HIP_TRY(e, hipStreamWaitEvent(e->stream, e->cov_ev2, 0));   // the zero series' filter: the steady gain and the step it settled at
    HIP_TRY(e, dlm::launch_wave48_steady_filter(k, stb.ktab, stb.settle, e->stream));
  }
  k.keep_cov = nullptr; k.ktab = nullptr; k.leave_step = nullptr;
  k.filt_in = k.filt;
  return DLM_OK;
}

static int sampler_common(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params,
                          const double* y, const double* z, const dlm_options* opts,
                          const double* filt_in, double* filt_ws, double* theta, double* cond,
                          double* stats, int32_t* status, bool forward) {
  int rc = check_common(e, model, params, opts);
  if (rc) return rc;
  AuxScope aux(e);                            // rule A of the auxiliary streams on every exit path below
  const bool norec = forward && !filt_ws;     // dlm_ffbs_batch that does not want the filter records
  if (forward && !y) return fail(e, DLM_ERR_ARG, "y is required");
  if (!forward && !filt_in) return fail(e, DLM_ERR_ARG, "filter records are required");
  if (stats && !y) return fail(e, DLM_ERR_ARG, "sufficient statistics need y");
  const size_t d = model->d, p = model->p, T = model->T, N = model->N, rec = d + d * d;
  KArgs k{};
  Stager st(e, opts->mem == DLM_MEM_HOST);
  stage_model(st, k, model, params, opts);
  const bool simflag = forward && (opts->flags & DLM_OPT_FFBS_SIMSMOOTH) && !cond;
  const bool eig = (opts->flags & DLM_OPT_DRAW_EIG) != 0;   // the reference's eigen-factor for the draw: the general kernel's backward pass (any forward kernel)
  if (eig && simflag) return fail(e, DLM_ERR_ARG, "DLM_OPT_DRAW_EIG selects the factor of the reference-form backward sampler; the simulation smoother (DLM_OPT_FFBS_SIMSMOOTH) factors nothing per step");
  bool shared_factors = false, shared_big = false;
  dlm::SampTabs stb{};
  // On the structured d <= 15, p = 1 path a V_t stream is a scalar per step (the Student-t DLM, StudentTGibbs.scala:100-136) and a W_t
  // stream (DlmFsvSystem.scala:137-208 feeds one W per step) a 13-pivot Cholesky factor per step; elsewhere they would need the
  // factorisation of a p x p / 48 x 48 matrix per step: the reference-form sampler serves those callers
  if (simflag && params->v_tstride && !(model->p == 1 && model->d <= 15))
    return fail(e, DLM_ERR_UNSUPPORTED, "the simulation smoother takes a V_t stream only on the structured d <= 15, p = 1 path (drop DLM_OPT_FFBS_SIMSMOOTH otherwise)");
  st.in(&k.y, y, y ? N * T * p : 0);
  st.in(&k.z, z, z ? N * (T + 1) * (simflag ? d + p : d) : 0);
  if (forward && !norec) st.out(&k.filt, filt_ws, N * (T + 1) * rec);
  else if (!forward) st.in(&k.filt_in, filt_in, N * (T + 1) * rec);
  st.out(&k.theta, theta, N * (T + 1) * d);
  st.out(&k.cond, cond, N * (T + 1) * rec);
  st.out(&k.stats, stats, N * (size_t)dlm_stats_len(model->d, model->p, opts->flags));
  st.zeroed_out(&k.status, (int*)status, N);
  if ((rc = st.commit())) return rc;
  // the stretches of the reference-form sampler (KArgs::stretches): wherever a shared-factor table is possible for these parameters,
  // whether or not this call uses one -- a series' draws do not depend on the route it takes
  k.stretches = (dlm::sampler_shared_model_ok(k) || dlm::wave48_sampler_shared_model_ok(k)) ? 1 : 0;
  if (norec) {   // the records of the forward pass are nobody's output: an engine workspace
    if ((rc = ensure(e, e->fws, N * (T + 1) * rec * sizeof(double)))) return rc;
    k.filt = e->fws;
  }
  if (forward) {
    if ((rc = analyse_g(e, k, model->G, opts->mem == DLM_MEM_HOST))) return rc;
    if ((rc = mark(e, 0))) return rc;
    if (simflag) {
      int (*sim)(dlm_engine*, KArgs&) = nullptr;
      if (use_lane(k) && !k.v_tstride && !k.w_tstride) sim = simsmooth_lane;
      else if (e->sparse_k) sim = simsmooth_sparse16;
      else if (k.v_tstride || (k.w_tstride && !use_tiled(k)))
        return fail(e, DLM_ERR_UNSUPPORTED, "a V_t / W_t stream with DLM_OPT_FFBS_SIMSMOOTH needs a structured G (this one is dense); V_t also p = 1");
      else if (use_tiled(k)) sim = simsmooth_tiled;
      else if (z) return fail(e, DLM_ERR_UNSUPPORTED, "injected normals with DLM_OPT_FFBS_SIMSMOOTH need a fast path (structured d <= 15 or 16 <= d <= 48)");
      if (sim) return (rc = sim(e, k)) ? rc : st.finish(opts->flags & DLM_OPT_ASYNC);   // (otherwise: the reference-form sampler below)
    }
    shared_factors = !simflag && !eig && !use_lane(k) && fast_shape_ok(k) && e->sparse_k > 0 && dlm::sampler_shared_eligible(k);
    shared_big = !simflag && !eig && !shared_factors && use_tiled(k) && dlm::wave48_sampler_shared_eligible(k);   // 16 <= d <= 48 on the per-wave kernels
    rc = norec && shared_factors ? forward_shared_means(e, k, stb) : forward_records(e, k, stb, shared_factors, shared_big, norec && shared_big);
    if (rc) return rc;
  }
  if (!forward && ((rc = analyse_g(e, k, model->G, opts->mem == DLM_MEM_HOST)) || (rc = mark(e, 0)))) return rc;   // the structure tables of G
  if ((rc = mark(e, 1))) return rc;
  auto done = [&]() { const int r = mark(e, 2); return r ? r : st.finish(opts->flags & DLM_OPT_ASYNC); };
  if (eig) {
    if (dlm::generic_sampler_lds_bytes(k.d, k.p) > dlm::lds_limit())
      return fail(e, DLM_ERR_UNSUPPORTED, "DLM_OPT_DRAW_EIG runs on the general backward sampler kernel: d <= 53");
    e->variant = "generic-eig";
    HIP_TRY(e, dlm::launch_generic_sampler(k, e->stream));
    return done();
  }
  if (use_lane(k)) {
    e->variant = "lane-sampler";
    HIP_TRY(e, dlm::launch_lane_sampler(k, e->stream));
    return done();
  }
  if (shared_factors) {
    // V, W, C0 shared by the batch on a regular grid: J_t, H_t and the factors once per call (the table of the second stream), the
    // series draw against it; a series with a missing observation computes its own as always
    e->variant = "sparse16-sampler-shared";
    if ((rc = aux_join(e))) return rc;   // the tables, and the normals where the call makes them
    k.route = e->route;
    HIP_TRY(e, dlm::launch_sampler_shared_draw(k, e->sparse_k, e->sp_dev, stb, e->stream));
    return done();
  }
  if (fast_shape_ok(k) && e->sparse_k > 0 && !(k.flags & DLM_OPT_NO_SAMPLER16)) {
    e->variant = "sparse16-sampler";
    HIP_TRY(e, dlm::launch_sparse16_sampler(k, e->sparse_k, e->sp_dev, e->stream));
    return done();
  }
  if (!(k.flags & (DLM_OPT_FORCE_GENERIC | DLM_OPT_NO_SAMPLER16)) && dlm::wave48_small_ok(k)) {
    e->variant = "sparse16-sampler";
    HIP_TRY(e, dlm::launch_small_mv_sampler(k, e->stream));
    return done();
  }
  if (shared_big) {
    e->variant = "wave-sampler-shared";
    if ((rc = aux_join(e))) return rc;   // the tables, and the normals where the call makes them
    k.route = e->route;
    HIP_TRY(e, dlm::launch_wave48_sampler_shared_draw(k, stb, e->stream));
    return done();
  }
  if (!(k.flags & (DLM_OPT_FORCE_GENERIC | DLM_OPT_NO_SAMPLER16)) && dlm::wave48_sampler_supported(k)) {
    e->variant = "wave-sampler";
    HIP_TRY(e, dlm::launch_wave48_sampler(k, e->stream));
    return done();
  }
  e->variant = "generic";
  if (dlm::generic_sampler_lds_bytes(k.d, k.p) > dlm::lds_limit())
    return fail(e, DLM_ERR_UNSUPPORTED, "the general backward sampler kernel keeps seven d x d matrices in the LDS of one CU: d <= 53 (structured models with d <= 48 take the per-wave kernels)");
  HIP_TRY(e, dlm::launch_generic_sampler(k, e->stream));
  return done();
}

int dlm_ffbs_batch(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params,
                   const double* y, const double* z, const dlm_options* opts, double* filt_ws,
                   double* theta, double* cond, double* stats, int32_t* status) {
  return sampler_common(e, model, params, y, z, opts, nullptr, filt_ws, theta, cond, stats, status, true);
}

int dlm_backward_sample_batch(dlm_engine* e, const dlm_model_desc* model,
                              const dlm_params_desc* params, const double* y, const double* filt,
                              const double* z, const dlm_options* opts, double* theta,
                              double* cond, double* stats, int32_t* status) {
  return sampler_common(e, model, params, y, z, opts, filt, nullptr, theta, cond, stats, status, false);
}

int dlm_svd_filter_batch(dlm_engine* e, const dlm_model_desc* model,
                         const dlm_params_desc* params, const double* y,
                         const dlm_options* opts, double* svd_rec, int32_t* status) {
  int rc = check_common(e, model, params, opts);
  if (rc) return rc;
  if (!y || !svd_rec) return fail(e, DLM_ERR_ARG, "y and svd_rec are required");
  if (model->d > 48 || model->p > 32) return fail(e, DLM_ERR_UNSUPPORTED, "the SVD (square-root) filter takes d <= 48, p <= 32 in this build");
  const size_t d = model->d, p = model->p, T = model->T, N = model->N, srec = 2 * d + d * d;
  KArgs k{};
  Stager st(e, opts->mem == DLM_MEM_HOST);
  stage_model(st, k, model, params, opts);
  double* rec_dev = nullptr;
  st.in(&k.y, y, N * T * p);
  st.out(&rec_dev, svd_rec, N * (T + 1) * srec);
  st.zeroed_out(&k.status, (int*)status, N);
  if ((rc = st.commit())) return rc;
  e->variant = "svd-jacobi";
  if ((rc = want_counters(e, k))) return rc;
  if ((rc = mark(e, 0))) return rc;
  if (dlm::svd_shared_eligible(k)) {
    // parameters shared by the batch: the decompositions once per call (one wave), a mean-only kernel per series; a series with a
    // missing observation runs k_svd_filter as always
    if ((rc = ensure_route(e, (size_t)k.N))) return rc;
    if ((rc = ensure(e, e->covws, sizeof(double) * dlm::svd_shared_ws_doubles(k)))) return rc;
    HIP_TRY(e, dlm::launch_svd_filter_shared(k, rec_dev, e->covws, e->route, e->stream));
  } else HIP_TRY(e, dlm::launch_svd_filter(k, rec_dev, e->stream));
  if ((rc = mark(e, 1)) || (rc = mark(e, 2))) return rc;
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_svd_ffbs_batch(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params,
                       const double* y, const double* z, const dlm_options* opts,
                       double* svd_ws, double* theta, double* stats, int32_t* status) {
  int rc = check_common(e, model, params, opts);
  if (rc) return rc;
  if (!y || !svd_ws) return fail(e, DLM_ERR_ARG, "y and svd_ws are required");
  if (model->d > 48 || model->p > 32) return fail(e, DLM_ERR_UNSUPPORTED, "the SVD (square-root) sampler takes d <= 48, p <= 32 in this build");
  const size_t d = model->d, p = model->p, T = model->T, N = model->N, srec = 2 * d + d * d;
  KArgs k{};
  Stager st(e, opts->mem == DLM_MEM_HOST);
  stage_model(st, k, model, params, opts);
  double* rec_dev = nullptr;
  st.in(&k.y, y, N * T * p);
  st.in(&k.z, z, z ? N * (T + 1) * d : 0);
  st.out(&rec_dev, svd_ws, N * (T + 1) * srec);
  st.out(&k.theta, theta, N * (T + 1) * d);
  st.out(&k.stats, stats, N * (size_t)dlm_stats_len(model->d, model->p, opts->flags));
  st.zeroed_out(&k.status, (int*)status, N);
  if ((rc = st.commit())) return rc;
  e->variant = "svd-jacobi";
  if ((rc = want_counters(e, k))) return rc;
  if ((rc = mark(e, 0))) return rc;
  HIP_TRY(e, dlm::launch_svd_filter(k, rec_dev, e->stream));
  if ((rc = mark(e, 1))) return rc;
  HIP_TRY(e, dlm::launch_svd_sampler(k, rec_dev, e->stream));
  if ((rc = mark(e, 2))) return rc;
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_stats_pool(dlm_engine* e, const double* stats, int32_t N, int32_t L, double* pooled,
                   const dlm_options* opts) {
  if (!e) return DLM_ERR_ARG;
  if (!stats || !pooled || !opts || N < 1 || L < 1) return fail(e, DLM_ERR_ARG, "dlm_stats_pool arguments");
  HIP_TRY(e, hipSetDevice(e->device));
  const double* s_dev = nullptr; double* p_dev = nullptr;
  Stager st(e, opts->mem == DLM_MEM_HOST);
  st.in(&s_dev, stats, (size_t)N * L);
  st.out(&p_dev, pooled, (size_t)L);
  int rc = st.commit();
  if (rc) return rc;
  HIP_TRY(e, dlm::launch_stats_pool(s_dev, N, L, p_dev, e->stream));
  return st.finish(opts->flags & DLM_OPT_ASYNC);
}

int dlm_comm_unique_id(uint8_t id[DLM_COMM_ID_BYTES]) {
  static_assert(sizeof(ncclUniqueId) <= DLM_COMM_ID_BYTES, "id buffer too small");
  ncclUniqueId u;
  if (ncclGetUniqueId(&u) != ncclSuccess) return DLM_ERR_RCCL;
  memset(id, 0, DLM_COMM_ID_BYTES);
  memcpy(id, &u, sizeof(u));
  return DLM_OK;
}

int dlm_comm_init_rank(dlm_engine* e, int32_t nranks, int32_t rank, const uint8_t id[DLM_COMM_ID_BYTES]) {
  if (!e || !id || nranks < 1 || rank < 0 || rank >= nranks) return DLM_ERR_ARG;
  HIP_TRY(e, hipSetDevice(e->device));
  ncclUniqueId u;
  memcpy(&u, id, sizeof(u));
  ncclResult_t r = ncclCommInitRank(&e->comm, nranks, u, rank);
  if (r != ncclSuccess) return fail(e, DLM_ERR_RCCL, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
  e->has_comm = true;
  return DLM_OK;
}

int dlm_gibbs_suffstats_allreduce(dlm_engine* e, double* stats_dev, int64_t count) {
  if (!e || !stats_dev || count < 1) return DLM_ERR_ARG;
  if (!e->has_comm) return fail(e, DLM_ERR_RCCL, "no communicator: call dlm_comm_init_rank first");
  HIP_TRY(e, hipSetDevice(e->device));
  ncclResult_t r = ncclAllReduce(stats_dev, stats_dev, (size_t)count, ncclDouble, ncclSum, e->comm, e->stream);
  if (r != ncclSuccess) return fail(e, DLM_ERR_RCCL, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return DLM_OK;
}

}  // extern "C"
