// Microbenchmark 3: the traffic of a shared RTS route that writes S_t by a reads-free broadcast beside the forward pass, without its
// arithmetic.  C2's buffers: 10 000 series x 1001 records of 1456 B (d = 13), filtered and smoothed; one table of 1001 rows.
//   a     the broadcast writer alone: a wave loads bytes [128, 1456) of R adjacent table rows into registers once, then loops over its
//         share of the series and stores them into records (n, t .. t + R - 1): no load and no wait in the loop.
//         R = 1, 3, 6 | stores default / nt | 1, 2, 4 waves per SIMD | the four waves of a block on adjacent rows or on the same rows
//         of different series | every 16-byte piece, or only those of lines that no record head shares ("lines")
//   b     (a) on a second stream beside the replica of the forward pass's stores (fwd)
//   c     the heads-only backward replica (heads): per wave of four series and step one DMA of the four filtered heads eight steps
//         ahead, one 128-byte piece of the table row, a J row on 386 of 1000 steps, one store of the four 128-byte heads
//         -- and the same with whole lines: the store writes the one or two 128-byte lines each head lies in, the table DMA brings what fills them
//   d     today's k_mean_rts16 traffic (mean_io2's "scattered means + row per wave, stores nt") and fwd alone
// Every figure: min / max over REPS timed launches after one warm-up, so that the run-to-run range is in the same table.
// The last two lines price the new call, (b) + (c), against today's, (d)'s sum, for the split at line boundaries and for the split at byte 128
// of the record: "go" where the gain is more than five times the largest min-max range among the figures compared.
//   hipcc --offload-arch=gfx950 -O3 rts_broadcast.hip -o rts_broadcast ;  ./rts_broadcast [a] [b] [c] [d]   (no argument: all four)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <unistd.h>
typedef unsigned u4 __attribute__((ext_vector_type(4)));
typedef unsigned u2 __attribute__((ext_vector_type(2)));
typedef int i4 __attribute__((ext_vector_type(4)));
constexpr int REC = 182, RECB = REC * 8, HEAD = 128, NPC = (RECB - HEAD) / 16;   // 83 pieces of S_t behind the head
constexpr int RJ_ROWB = 16 * 18 * 8, NJ16 = 13 * 9;                              // a J row as dlm_sampler16.hip lays it out, and its pieces that travel
constexpr int OOB = 0x7ffffff0;
constexpr int REPS = 6;
__device__ __forceinline__ i4 rsrc_words(const void* p, unsigned bytes) {
  const unsigned long long a = (unsigned long long)p;
  i4 r = {__builtin_amdgcn_readfirstlane((int)(unsigned)a), __builtin_amdgcn_readfirstlane((int)(unsigned)((a >> 32) & 0xffffu)), __builtin_amdgcn_readfirstlane((int)bytes), 0x00020000};
  return r;
}
template <int N> __device__ __forceinline__ void vm_wait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void dma(const i4& rs, unsigned lds_addr, int voff, int soff, bool on) {
  lds_addr = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_addr);
  soff = __builtin_amdgcn_readfirstlane(soff);
  if (on) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lds_addr), "v"(voff), "s"(rs), "s"(soff) : "memory");
}
__device__ __forceinline__ unsigned lds_addr_of(const void* p) { return (unsigned)(size_t)(__attribute__((address_space(3))) const char*)p; }

// ---- a: the broadcast writer.  Wave w of the grid: row group w % nrg (rows R rg .. R rg + R - 1), series chunk w / nrg (ADJ: the waves
// of a block write adjacent rows of the same series) or row group w / nch, chunk w % nch (the waves of a block write the same rows).
template <int R, int AUX, bool ADJ, bool LINES>
__global__ __launch_bounds__(256) void k_bcast(double* out, const double* __restrict__ tab, int T, int N, int nch) {
  constexpr int NI = (R * NPC + 63) / 64;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  const int nrg = (T + R) / R;
  if (w >= nrg * nch) return;
  const int rg = ADJ ? w % nrg : w / nch, ch = ADJ ? w / nrg : w % nch;
  const int per = (N + nch - 1) / nch, nb = ch * per, ne = nb + per < N ? nb + per : N;
  const int t0 = rg * R;
  const size_t sbytes = (size_t)(T + 1) * RECB;
  u4 pc[NI];
  int voff[NI];
#pragma unroll
  for (int k = 0; k < NI; ++k) {
    const int q = 64 * k + lane, row = q / NPC, pp = q - row * NPC;
    const bool on = row < R && t0 + row <= T;
    voff[k] = on ? row * RECB + HEAD + pp * 16 : OOB;
    pc[k] = on ? *(const u4*)((const char*)tab + (size_t)(t0 + row) * RECB + HEAD + pp * 16) : u4{0, 0, 0, 0};
  }
  for (int n = nb; n < ne; ++n) {
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((char*)out + (size_t)n * sbytes, 0, (int)sbytes, 0x00020000);
    const int ph = (int)(((size_t)n * sbytes + (size_t)t0 * RECB) & 127);   // (the allocation starts on a line)
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      int vo = voff[k];
      if (LINES && vo != OOB) {   // keep a piece only where its whole line lies behind the head of its record and in front of the next record
        const int row = vo / RECB, line = (ph + vo) & ~127;
        if (line < ph + row * RECB + HEAD || line + 128 > ph + (row + 1) * RECB) vo = OOB;
      }
      __builtin_amdgcn_raw_buffer_store_b128(pc[k], r, vo, t0 * RECB, AUX);
    }
  }
}

// ---- the forward pass's stores: one series per wave, four waves per block, per step four 8-byte stores per lane at filter_body's
// offsets (lane 16 g + c: element (4 r + g, c) of C_t, lanes c == 15: m[4 r + g]), a 512-byte load of y every 64 steps.
__global__ __launch_bounds__(256) void k_fwd(double* filt, const double* __restrict__ y, int T, int N) {
  extern __shared__ double pad[];
  const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15, d = 13;
  const int n = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (n >= N) return;
  const size_t sbytes = (size_t)(T + 1) * RECB;
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((char*)filt + (size_t)n * sbytes, 0, (int)sbytes, 0x00020000);
  int offA[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { const int i = 4 * q + g; offA[q] = (i < d && c < d) ? (d + i * d + c) * 8 : ((i < d && c == 15) ? i * 8 : OOB); }
  double v = 1.0 + lane, yk = 0.0;
  if (threadIdx.x == 0) pad[0] = v;
#pragma unroll
  for (int q = 0; q < 4; ++q) __builtin_amdgcn_raw_buffer_store_b64(u2{(unsigned)__double2loint(v), (unsigned)__double2hiint(v)}, r, offA[q], 0, 0);
  for (int t = 0; t < T; ++t) {
    if ((t & 63) == 0) yk = t + lane < T ? y[(size_t)n * T + t + lane] : 0.0;
    v += __shfl(yk, t & 63) * 1e-9 + 1e-3;
    const int so = (t + 1) * RECB;
#pragma unroll
    for (int q = 0; q < 4; ++q) __builtin_amdgcn_raw_buffer_store_b64(u2{(unsigned)__double2loint(v), (unsigned)__double2hiint(v)}, r, offA[q], so, 0);
  }
}

// ---- c: the heads-only backward pass.  A step issues, in this order: the request for the means (eight steps ahead), for a J row (two
// steps ahead, when there is one), for the head of the table row (two steps ahead), its one store.  Younger than the request for the
// head of row t: that step's store, then step t + 1's means, J row (when it exists), head and store.
__device__ __forceinline__ bool need_j(int t) { return t >= 0 && (t * 386) % 1000 < 386; }
// WL (whole lines): the store writes, per series, the one or two 128-byte lines that the head of record t lies in, clipped to the series' own
// records -- 64 lanes x 16 bytes -- and the table DMA brings what fills them: the first 256 bytes of row t and the last 128 of row t - 1.
template <int AUX, bool WL>
__global__ __launch_bounds__(64, 3) void k_heads(double* out, const double* tab, const double* jrows, const double* filt, int T, int N) {
  __shared__ __attribute__((aligned(16))) double lds[8 * 64 + 2 * (RJ_ROWB / 8) + 2 * 48];
  const int lane = threadIdx.x, n0 = 4 * blockIdx.x;
  if (n0 >= N) return;
  const int nser = N - n0 < 4 ? N - n0 : 4;
  const size_t sbytes = (size_t)(T + 1) * RECB;
  const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc((char*)out + (size_t)n0 * sbytes, 0, (int)(nser * sbytes), 0x00020000);
  const i4 rmean = rsrc_words((const char*)filt + (size_t)n0 * sbytes, (unsigned)(nser * sbytes));
  const i4 rtab = rsrc_words(tab, (unsigned)sbytes), rjt = rsrc_words(jrows, (unsigned)((size_t)(T + 1) * RJ_ROWB));
  const unsigned mring = lds_addr_of(lds), jring = mring + 8 * 512, tring = jring + 2 * RJ_ROWB;
  const int mvoff = (lane < 32 && (lane >> 3) < nser) ? (int)((size_t)(lane >> 3) * sbytes) + (lane & 7) * 16 : OOB;
  auto req_j = [&](int t) { dma(rjt, jring + (t & 1) * RJ_ROWB, lane * 16, t * RJ_ROWB, true); dma(rjt, jring + (t & 1) * RJ_ROWB + 1024, lane * 16 + 1024, t * RJ_ROWB, lane + 64 < NJ16); };
  const int P0 = (int)(((size_t)n0 * sbytes) & 127);   // (the allocation starts on a line)
  const int jw = lane >> 4, qw = lane & 15;
  auto req_t = [&](int t) {
    if (WL) dma(rtab, tring + (t & 1) * 384, lane < 16 ? RECB + lane * 16 : RECB - 128 + (lane - 16) * 16, (t > 0 ? t - 1 : 0) * RECB, lane < 24);
    else dma(rtab, tring + (t & 1) * 128, lane * 16, t * RECB, lane < 8);
  };
  auto req_m = [&](int t) { dma(rmean, mring + (t & 7) * 512, mvoff, (t > 0 ? t : 0) * RECB, lane < 32); };
  auto put = [&](int t, double v) { __builtin_amdgcn_raw_buffer_store_b128(u4{(unsigned)__double2loint(v), (unsigned)__double2hiint(v), (unsigned)t, (unsigned)lane}, rout, mvoff, t * RECB, AUX); };
  auto put_lines = [&](int t, double v) {
    const long long rel = (long long)jw * (long long)sbytes + (long long)t * RECB;
    const int ph = (int)((P0 + rel) & 127);
    const long long x = rel - ph + 16 * qw;
    const bool on = jw < nser && 16 * qw < (ph ? 256 : 128) && x >= (long long)jw * (long long)sbytes && x < (long long)(jw + 1) * (long long)sbytes;
    const int off = 16 * qw - ph;                  // of the piece inside record t: < 0 the tail of row t - 1, < 128 the head, else row t
    v += lds[8 * 64 + 2 * (RJ_ROWB / 8) + (t & 1) * 48 + (off < 0 ? 32 + (128 + off) / 8 : off / 8)] * 1e-9;
    __builtin_amdgcn_raw_buffer_store_b128(u4{(unsigned)__double2loint(v), (unsigned)__double2hiint(v), (unsigned)t, (unsigned)lane}, rout, on ? (int)x : OOB, 0, AUX);
  };
  for (int k = 0; k < 8; ++k) req_m(T - k);
  req_t(T); req_t(T - 1 > 0 ? T - 1 : 0);
  if (need_j(T - 1)) req_j(T - 1);
  vm_wait<0>();
  double v = 1.0 + lane;
  req_m(T - 8);
  if (need_j(T - 2)) req_j(T - 2);
  req_t(T - 2 > 0 ? T - 2 : 0);
  if (WL) put_lines(T, v); else put(T, v);
  for (int t = T - 1; t >= 0; --t) {
    if (need_j(t - 1)) vm_wait<6>(); else vm_wait<4>();
    v += lds[(t & 7) * 64 + (lane & 31)] * 1e-9 + lds[8 * 64 + 2 * (RJ_ROWB / 8) + (t & 1) * (WL ? 48 : 16) + (lane & 15)] * 1e-9;
    if (need_j(t)) v += lds[8 * 64 + (t & 1) * (RJ_ROWB / 8) + lane] * 1e-9;
    req_m(t - 8);
    if (need_j(t - 2)) req_j(t - 2);
    req_t(t - 2 > 0 ? t - 2 : 0);
    if (WL) put_lines(t, v); else put(t, v);
    v += 1e-3;
  }
  vm_wait<0>();
}

// ---- d: today's k_mean_rts16 traffic, as mean_io2.hip's k_io<1, 1, AUX, 1>
template <int AUX>
__global__ __launch_bounds__(64) void k_today(double* out, const double* tab, const double* filt, int T, int N) {
  __shared__ __attribute__((aligned(16))) double lds[2 * 256 + 8 * 64];
  const int lane = threadIdx.x, n0 = 4 * blockIdx.x;
  if (n0 >= N) return;
  const int nser = N - n0 < 4 ? N - n0 : 4, npc = REC / 2;
  const size_t sbytes = (size_t)(T + 1) * RECB;
  const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc((char*)out + (size_t)n0 * sbytes, 0, (int)(nser * sbytes), 0x00020000);
  const i4 rtab = rsrc_words(tab, (unsigned)sbytes), rmean = rsrc_words((const char*)filt + (size_t)n0 * sbytes, (unsigned)(nser * sbytes));
  const unsigned ldst = lds_addr_of(lds), ldsm = ldst + 2 * 2048;
  int pdst[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) { const int q = 64 * k + lane, sj = q / npc, pp = q - sj * npc; pdst[k] = sj < nser ? (int)((size_t)sj * sbytes) + pp * 16 : OOB; }
  const int mvoff = (lane < 32 && (lane >> 3) < nser) ? (int)((size_t)(lane >> 3) * sbytes) + (lane & 7) * 16 : OOB;
  double v = 1.0 + lane;
  for (int s = 0; s <= T; ++s) {
    const int t = T - s;
    dma(rmean, ldsm + (s & 7) * 512, mvoff, t * RECB, lane < 32);
    dma(rtab, ldst + (s & 1) * 2048, lane * 16, t * RECB, true);
    dma(rtab, ldst + (s & 1) * 2048 + 1024, lane * 16 + 1024, t * RECB, lane + 64 < npc);
    vm_wait<9 + 6>();
    v += lds[(s & 1) * 256 + lane] * 1e-9 + lds[2 * 256 + (s & 7) * 64 + lane] * 1e-9;
#pragma unroll
    for (int k = 0; k < 6; ++k) __builtin_amdgcn_raw_buffer_store_b128(u4{(unsigned)__double2loint(v), (unsigned)__double2hiint(v), (unsigned)k, (unsigned)lane}, rout, pdst[k], t * RECB, AUX);
    v += 1e-3;
  }
  vm_wait<0>();
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
struct Fig { float lo, hi; };
int main(int argc, char** argv) {
  const int N = 10000, T = 1000;
  const size_t sbytes = (size_t)(T + 1) * RECB, bytes = (size_t)N * sbytes;
  auto want = [&](const char* s) { if (argc < 2) return true; for (int i = 1; i < argc; ++i) if (!strcmp(argv[i], s)) return true; return false; };
  double *out, *filt, *tab, *jrows, *y;
  CK(hipMalloc(&out, bytes)); CK(hipMalloc(&filt, bytes)); CK(hipMalloc(&tab, sbytes)); CK(hipMalloc(&jrows, (size_t)(T + 1) * RJ_ROWB)); CK(hipMalloc(&y, (size_t)N * T * 8));
  CK(hipMemset(filt, 0, bytes)); CK(hipMemset(tab, 0, sbytes)); CK(hipMemset(jrows, 0, (size_t)(T + 1) * RJ_ROWB)); CK(hipMemset(y, 0, (size_t)N * T * 8));
  hipStream_t s1, s2; CK(hipStreamCreate(&s1)); CK(hipStreamCreate(&s2));
  hipEvent_t e0, e1, e2; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1)); CK(hipEventCreate(&e2));
  // one launch on s1 (and one on s2 where given), timed from the common start to the end of both
  auto run = [&](const char* name, auto on1, auto on2, bool two) -> Fig {
    Fig f = {1e30f, 0.f};
    for (int rep = 0; rep <= REPS; ++rep) {
      (void)hipEventRecord(e0, s1);
      if (two) { (void)hipStreamWaitEvent(s2, e0, 0); on2(); (void)hipEventRecord(e2, s2); }
      on1();
      if (two) (void)hipStreamWaitEvent(s1, e2, 0);
      (void)hipEventRecord(e1, s1);
      if (hipEventSynchronize(e1) != hipSuccess) { printf("%s: failed\n", name); fflush(stdout); _exit(2); }
      float ms; (void)hipEventElapsedTime(&ms, e0, e1);
      if (rep) { if (ms < f.lo) f.lo = ms; if (ms > f.hi) f.hi = ms; }
    }
    printf("%-72s min %.3f  max %.3f ms\n", name, f.lo, f.hi); fflush(stdout);
    return f;
  };
  auto none = [] {};
  auto fwd = [&](hipStream_t s) { hipLaunchKernelGGL(k_fwd, dim3((N + 3) / 4), dim3(256), 32 * 1024, s, filt, (const double*)y, T, N); };
  char name[160];
  Fig best_a = {1e30f, 0.f}, best_b = {1e30f, 0.f}, best_bl = {1e30f, 0.f};
  auto bcast = [&](auto kern, int R, int aux, bool adj, bool lines, int wps) {
    const int nrg = (T + R) / R, waves = 1024 * wps, nch = (waves + nrg - 1) / nrg, blocks = (nrg * nch + 3) / 4;
    auto go = [&](hipStream_t s) { hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, s, out, (const double*)tab, T, N, nch); };
    snprintf(name, sizeof name, "R %d %s %s %s %d waves/SIMD", R, aux ? "nt     " : "default", adj ? "adjacent rows" : "same rows    ", lines ? "lines " : "pieces", wps);
    if (want("a")) { char nm[200]; snprintf(nm, sizeof nm, "a  %s", name); const Fig f = run(nm, [&] { go(s1); }, none, false); if (!lines && f.lo < best_a.lo) best_a = f; }
    if (want("b")) { char nm[200]; snprintf(nm, sizeof nm, "b  fwd + %s", name); const Fig f = run(nm, [&] { fwd(s1); }, [&] { go(s2); }, true); if (!lines && f.lo < best_b.lo) best_b = f; if (lines && f.lo < best_bl.lo) best_bl = f; }
  };
#define B4(R, AUX, WPS) bcast(k_bcast<R, AUX, true, false>, R, AUX, true, false, WPS); bcast(k_bcast<R, AUX, false, false>, R, AUX, false, false, WPS); \
                        bcast(k_bcast<R, AUX, true, true>, R, AUX, true, true, WPS);
#define B3(R, AUX) B4(R, AUX, 1) B4(R, AUX, 2) B4(R, AUX, 4)
  if (want("a") || want("b")) { B3(1, 0) B3(1, 2) B3(3, 0) B3(3, 2) B3(6, 0) B3(6, 2) }
  Fig c = {0, 0}, cl = {0, 0}, dt = {0, 0}, df = {0, 0};
  if (want("c")) {
    c = run("c  heads, stores nt", [&] { hipLaunchKernelGGL((k_heads<2, false>), dim3((N + 3) / 4), dim3(64), 0, s1, out, (const double*)tab, (const double*)jrows, (const double*)filt, T, N); }, none, false);
    const Fig c0 = run("c  heads, stores default", [&] { hipLaunchKernelGGL((k_heads<0, false>), dim3((N + 3) / 4), dim3(64), 0, s1, out, (const double*)tab, (const double*)jrows, (const double*)filt, T, N); }, none, false);
    if (c0.lo < c.lo) c = c0;
    cl = run("c  heads, whole lines, stores nt", [&] { hipLaunchKernelGGL((k_heads<2, true>), dim3((N + 3) / 4), dim3(64), 0, s1, out, (const double*)tab, (const double*)jrows, (const double*)filt, T, N); }, none, false);
    const Fig c1 = run("c  heads, whole lines, stores default", [&] { hipLaunchKernelGGL((k_heads<0, true>), dim3((N + 3) / 4), dim3(64), 0, s1, out, (const double*)tab, (const double*)jrows, (const double*)filt, T, N); }, none, false);
    if (c1.lo < cl.lo) cl = c1;
  }
  if (want("d")) {
    dt = run("d  today's backward traffic (means + row per wave, stores nt)", [&] { hipLaunchKernelGGL(k_today<2>, dim3((N + 3) / 4), dim3(64), 0, s1, out, (const double*)tab, (const double*)filt, T, N); }, none, false);
    df = run("d  fwd alone", [&] { fwd(s1); }, none, false);
  }
  if (argc < 2) {
    const float rl = fmaxf(fmaxf(best_bl.hi - best_bl.lo, cl.hi - cl.lo), fmaxf(dt.hi - dt.lo, df.hi - df.lo)), gl = dt.lo + df.lo - best_bl.lo - cl.lo;
    printf("split at line boundaries: new call b + c = %.3f ms | gain %.3f ms | largest range %.3f ms -> %s\n", best_bl.lo + cl.lo, gl, rl, gl > 5.f * rl ? "go" : "no-go");
    const float range = fmaxf(fmaxf(best_b.hi - best_b.lo, c.hi - c.lo), fmaxf(dt.hi - dt.lo, df.hi - df.lo));
    printf("split at byte 128 of the record: best a %.3f ms | new call b + c = %.3f ms | today's call d = %.3f ms | gain %.3f ms | largest range %.3f ms -> %s\n", best_a.lo, best_b.lo + c.lo,
           dt.lo + df.lo, dt.lo + df.lo - best_b.lo - c.lo, range, dt.lo + df.lo - best_b.lo - c.lo > 5.f * range ? "go" : "no-go");
  }
  return 0;
}
