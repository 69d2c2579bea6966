// Wave-level device primitives of the kernel files: the small functions that wrap one hardware instruction (or a fixed handful),
// each defined here ONCE, with the rule the hand-written pipelines rest on stated next to it.  Device code only: included by the
// kernel files, not by dlm_engine.hip.  tests/test_device_primitives_host.py keeps the kernel files from growing copies again.
//
// Lane naming throughout: lane = 16 g + c (g = 0..3 the 16-lane row, c = 0..15 the lane of the row); in the fp64 MFMA accumulator
// layout register r of a tile holds element (4 r + g, c).
#pragma once
#include "dlm_internal.h"

namespace dlm {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));
typedef unsigned u2 __attribute__((ext_vector_type(2)));
typedef unsigned u4 __attribute__((ext_vector_type(4)));
typedef int i4 __attribute__((ext_vector_type(4)));

// ---- LDS hand-off between lanes of ONE wavefront -------------------------------------------------------------------------
// The LDS queue is in order per wave, so only the compiler has to be kept from reordering: no s_barrier, and none of the
// vmcnt(0) a __syncthreads() fence would add after the record stores.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- cross-lane moves, sums and picks --------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {   // one DPP move of both words (CTRL: quad_perm, row_ror, row_half_mirror, ...)
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);   // bound_ctrl: no "old" value to set up
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
template <int N>
__device__ __forceinline__ double row_ror(double v) { return dpp_mov<0x120 + N>(v); }   // rotate within a 16-lane row
// sum over the 16 lanes of a row (over c); every lane of the row gets the sum
__device__ __forceinline__ double row_sum(double v) {
  v += row_ror<8>(v); v += row_ror<4>(v); v += row_ror<2>(v); v += row_ror<1>(v);
  return v;
}
// sum over lanes c, c+16, c+32, c+48 (over g) with the gfx950 permlane swaps; all get the sum
__device__ __forceinline__ double sum_g(double v) {
  unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
  u2 l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  u2 h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  v = __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
  lo = (unsigned)__double2loint(v); hi = (unsigned)__double2hiint(v);
  l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  return __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
}
// max over the 64 lanes; every lane gets it (the steady-state tests: every fourth step at most)
__device__ __forceinline__ double wave_max(double v) {
  v = fmax(v, row_ror<8>(v)); v = fmax(v, row_ror<4>(v)); v = fmax(v, row_ror<2>(v)); v = fmax(v, row_ror<1>(v));
  unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
  u2 l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  u2 h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  v = fmax(__hiloint2double((int)h[0], (int)l[0]), __hiloint2double((int)h[1], (int)l[1]));
  lo = (unsigned)__double2loint(v); hi = (unsigned)__double2hiint(v);
  l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  return fmax(__hiloint2double((int)h[0], (int)l[0]), __hiloint2double((int)h[1], (int)l[1]));
}
// sum over the 64 lanes by the xor butterfly (partner 32, 16, ..., 1): a fixed order, every lane gets the sum.  The reductions of the
// one-wave-per-series Gibbs steps (dlm_studentt.hip, dlm_sv.hip), whose NumPy restatements follow this order
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
// two float maxima at the price of one 64-bit reduction: a rides in the low, b in the high word through the same shuffles
__device__ __forceinline__ void wave_max2f(float& a, float& b) {
#define DLM_MAX2F_ROW(N) { a = fmaxf(a, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a), 0x120 + N, 0xf, 0xf, true))); \
                           b = fmaxf(b, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(b), 0x120 + N, 0xf, 0xf, true))); }
  DLM_MAX2F_ROW(8) DLM_MAX2F_ROW(4) DLM_MAX2F_ROW(2) DLM_MAX2F_ROW(1)
#undef DLM_MAX2F_ROW
  u2 l = __builtin_amdgcn_permlane16_swap((unsigned)__float_as_int(a), (unsigned)__float_as_int(a), false, false);
  u2 h = __builtin_amdgcn_permlane16_swap((unsigned)__float_as_int(b), (unsigned)__float_as_int(b), false, false);
  a = fmaxf(__int_as_float((int)l[0]), __int_as_float((int)l[1])); b = fmaxf(__int_as_float((int)h[0]), __int_as_float((int)h[1]));
  l = __builtin_amdgcn_permlane32_swap((unsigned)__float_as_int(a), (unsigned)__float_as_int(a), false, false);
  h = __builtin_amdgcn_permlane32_swap((unsigned)__float_as_int(b), (unsigned)__float_as_int(b), false, false);
  a = fmaxf(__int_as_float((int)l[0]), __int_as_float((int)l[1])); b = fmaxf(__int_as_float((int)h[0]), __int_as_float((int)h[1]));
}
// registers (x: rows 4 r + g, y: rows 4 (r + 1) + g)  ->  (lo, hi) = rows (base, base + 1), base = 4 (r + (g & 1)) + (g & 2):
// v_permlane16_swap of registers r and r + 1 leaves a lane with two ADJACENT rows of one of them
__device__ __forceinline__ void pair_rows(double x, double y, double& lo, double& hi) {
  const u2 l = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
  const u2 h = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
  lo = __hiloint2double((int)h[0], (int)l[0]);
  hi = __hiloint2double((int)h[1], (int)l[1]);
}
// the value of lane `src` (wave-uniform) for every lane, by v_readlane: an SGPR pair, no LDS round trip
__device__ __forceinline__ double readlane_d(double v, int src) {
  const int lo = __builtin_amdgcn_readlane((int)__double2loint(v), src);
  const int hi = __builtin_amdgcn_readlane((int)__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}
// the value of lane src (0..15, wave-uniform) of this lane's 16-lane row
__device__ __forceinline__ double row_pick(double v, int lane, int src) {
  const int a_ = ((lane & 48) + src) << 2;
  const int lo = __builtin_amdgcn_ds_bpermute(a_, __double2loint(v)), hi = __builtin_amdgcn_ds_bpermute(a_, __double2hiint(v));
  return __hiloint2double(hi, lo);
}
// ... of the row's lane 0.  row_pick(v, lane, 0) in value, kept as its own function: written through row_pick the compiler shares the
// address arithmetic with the row_pick calls beside it and the mean kernels of dlm_sparse16.hip come out three instructions shorter --
// other code than the one that was measured and compared bit for bit.
__device__ __forceinline__ double row_lane0(double v, int lane) {
  const int a = (lane & 48) << 2;
  const int lo = __builtin_amdgcn_ds_bpermute(a, __double2loint(v)), hi = __builtin_amdgcn_ds_bpermute(a, __double2hiint(v));
  return __hiloint2double(hi, lo);
}

// 1/x from v_rcp_f64 and two Newton steps (about 1 ulp): 5 VALU instructions instead of the 11 of the IEEE
// division expansion.  The forward pass is bound by VALU issue, and every lane computes this scalar.
__device__ __forceinline__ double fast_rcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  r = fma(fma(-x, r, 1.0), r, r);
  return r;
}

// X^T Y of two single tiles.  One dependent chain of four: two chains of two were measured slower (profiles/r01_pmc_notes.md).
__device__ __forceinline__ d4 mmT(const d4& x, const d4& y) {
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x[0], y[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x[1], y[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x[2], y[2], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x[3], y[3], acc, 0, 0, 0);
  return acc;
}

// ---- record I/O through raw buffer instructions ------------------------------------------------------------------------------
// Padded lanes carry an out-of-range offset (OOB), for which the hardware returns 0 on loads and drops stores: no exec-mask
// branches, and a FIXED number of instructions per lane -- which is what lets the compiler (and vm_wait<N>, by hand) count the
// vector-memory operations between a prefetch and its use.  A zero-sized resource drops every store.  Vector-memory operations of
// a wave retire in order.
constexpr int OOB = 0x7ffffff0;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t mk_rsrc(const void* p, size_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ double bld(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
  const u2 v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
  return __hiloint2double((int)v[1], (int)v[0]);
}
// the same load with glc: the re-read of a record this launch stored (dlm_wave48.hip's steady-state tests)
__device__ __forceinline__ double bld_glc(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
  const u2 v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 1);
  return __hiloint2double((int)v[1], (int)v[0]);
}
__device__ __forceinline__ void bst(__amdgpu_buffer_rsrc_t r, int voff, int soff, double x) {
  const u2 v = {(unsigned)__double2loint(x), (unsigned)__double2hiint(x)};
  __builtin_amdgcn_raw_buffer_store_b64(v, r, voff, soff, 0);
}
// 16 bytes per lane.  One wave per SIMD can keep at most 63 vector-memory operations in flight: with 8 bytes per lane a step's
// record stores are all the bandwidth a wave can ask for.  AUX: the cache policy of the store (0: default; 2: nt).
__device__ __forceinline__ d2 bld128(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
  const u4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
  d2 o = {__hiloint2double((int)v[1], (int)v[0]), __hiloint2double((int)v[3], (int)v[2])};
  return o;
}
template <int AUX = 0>
__device__ __forceinline__ void bst128(__amdgpu_buffer_rsrc_t r, int voff, int soff, double x, double y) {
  const u4 v = {(unsigned)__double2loint(x), (unsigned)__double2hiint(x), (unsigned)__double2loint(y), (unsigned)__double2hiint(y)};
  __builtin_amdgcn_raw_buffer_store_b128(v, r, voff, soff, AUX);
}
template <int AUX = 0>
__device__ __forceinline__ void bst128(__amdgpu_buffer_rsrc_t r, int voff, int soff, d2 x) { bst128<AUX>(r, voff, soff, x[0], x[1]); }

// ---- prefetch by LDS DMA -------------------------------------------------------------------------------------------------------
// `buffer_load_dwordx4 ... lds` copies 16 B per lane straight from HBM into LDS: no VGPRs are held while the load is in flight, so
// a wave can keep several records in flight (the loaded HBM latency is of the order of one step) without giving up occupancy.
// The instruction is issued from inline assembly on purpose: the compiler's wait-count insertion treats an LDS-DMA it knows about
// as aliasing every later LDS read and waits vmcnt(0) -- which would also wait for the just-issued record stores.  The waits are
// placed by hand instead (vm_wait<N>, dlm_internal.h); vector-memory operations of a wave retire in order, and N counts the loads,
// stores and DMAs the wave issued after the one waited for.
__device__ __forceinline__ i4 rsrc_words(const void* p, unsigned bytes) {   // the descriptor as four wave-uniform words (an asm "s" operand)
  const unsigned long long a = (unsigned long long)p;
  i4 r = {__builtin_amdgcn_readfirstlane((int)(unsigned)a), __builtin_amdgcn_readfirstlane((int)(unsigned)((a >> 32) & 0xffffu)),
          __builtin_amdgcn_readfirstlane((int)bytes), 0x00020000};
  return r;
}
__device__ __forceinline__ unsigned lds_addr_of(const void* p) {
  return (unsigned)(size_t)(__attribute__((address_space(3))) const char*)p;
}
// ONE DMA instruction: 16 bytes per active lane from byte voff + soff of the buffer to LDS address lds_addr + 16 lane; lds_addr and soff
// wave-uniform (readfirstlane'd by the caller).  For the callers whose lanes do not read 16 lane bytes apart (the means of four series).
__device__ __forceinline__ void lds_dma_issue(const i4& rs, unsigned lds_addr, int voff, int soff) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lds_addr), "v"(voff), "s"(rs), "s"(soff) : "memory");
}
// n16 <= 64 NR pieces of 16 bytes from byte offset soff of the buffer to LDS byte address lds_addr.  NR = ceil(n16 / 64): every
// instruction has lanes to serve, so the wave issues NR vector-memory operations whatever the exec mask -- vm_wait<N> counts them.
// (The offsets are written out: as an asm operand of one statement they cost a -DDLM_STAMP kernel of dlm_sparse16.hip its register allocation.)
template <int NR>
__device__ __forceinline__ void lds_dma(const i4& rs, unsigned lds_addr, int soff, int lane, int n16) {
  static_assert(NR >= 1 && NR <= 4, "at most 256 pieces");
  const int voff = lane * 16;
  lds_addr = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_addr);   // wave-uniform by construction
  soff = __builtin_amdgcn_readfirstlane(soff);
  if (lane < n16) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lds_addr), "v"(voff), "s"(rs), "s"(soff) : "memory");
  if constexpr (NR > 1) if (lane + 64 < n16) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen offset:1024 lds" ::"s"(lds_addr), "v"(voff), "s"(rs), "s"(soff) : "memory");
  if constexpr (NR > 2) if (lane + 128 < n16) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen offset:2048 lds" ::"s"(lds_addr), "v"(voff), "s"(rs), "s"(soff) : "memory");
  if constexpr (NR > 3) if (lane + 192 < n16) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen offset:3072 lds" ::"s"(lds_addr), "v"(voff), "s"(rs), "s"(soff) : "memory");
}

// ---- hand-issued LDS reads and their waits --------------------------------------------------------------------------------------
// LDS reads issued from inline assembly as single ds_read_b64 / ds_read_b128: the compiler would pair 64-bit reads into
// ds_read2_b64, which runs at half the LDS rate (8 LDS cycles per KiB against 4 for two ds_read_b64; MI355X_MICROARCH LDS table).
// The compiler does not count these reads: lds_fence / lds_wait wait for them (lgkmcnt(0)) and also tie the loaded registers to
// the wait, so that no use of them can be scheduled ahead of it.
template <int OFF>
__device__ __forceinline__ double lds_read64(unsigned addr) {
  double v;
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
template <int OFF = 0>
__device__ __forceinline__ d2 lds_read128(unsigned addr) {
  d2 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
__device__ __forceinline__ void lds_fence(d4& a) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a)::"memory"); }
__device__ __forceinline__ void lds_fence(d4& a, d4& b) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b)::"memory"); }
__device__ __forceinline__ void lds_wait(d2& a) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a)::"memory"); }
__device__ __forceinline__ void lds_wait(d2& a, d2& b, d2& c) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c)::"memory"); }
__device__ __forceinline__ void lds_wait(d2& a, d2& b, double& c) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c)::"memory"); }
__device__ __forceinline__ void lds_wait(d4& a, d4& b, d2& c, d2& e, double& f) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(e), "+v"(f)::"memory");
}
template <int NP>   // (an asm statement takes no pack: a ladder over the piece counts in use)
__device__ __forceinline__ void lds_wait(d2 (&pc)[NP]) {
  static_assert(NP == 2 || NP == 4 || NP == 6 || NP == 8, "pieces");
  if constexpr (NP == 2) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(pc[0]), "+v"(pc[1])::"memory");
  else if constexpr (NP == 4) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(pc[0]), "+v"(pc[1]), "+v"(pc[2]), "+v"(pc[3])::"memory");
  else if constexpr (NP == 6) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(pc[0]), "+v"(pc[1]), "+v"(pc[2]), "+v"(pc[3]), "+v"(pc[4]), "+v"(pc[5])::"memory");
  else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(pc[0]), "+v"(pc[1]), "+v"(pc[2]), "+v"(pc[3]), "+v"(pc[4]), "+v"(pc[5]), "+v"(pc[6]), "+v"(pc[7])::"memory");
}

// ---- diagnostic builds only (-DDLM_STAMP): the shader clock, for the phase stamps of a step (never in the shipped build) ----
// stamp(): scheduling barriers on both sides, so that no instruction of a neighbouring phase crosses it (dlm_sparse16.hip).  The stamps of
// dlm_tiled.hip and dlm_svd.hip sit behind workgroup barriers or around calls and never had them: stamp_loose() keeps their objects as they were.
#ifdef DLM_STAMP
__device__ __forceinline__ unsigned long long stamp() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
__device__ __forceinline__ unsigned long long stamp_loose() {
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
#endif

}  // namespace dlm
