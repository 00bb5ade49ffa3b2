// Device primitives of the 16-point-wave kernels (fenerf_siren_f16w.hip: f16x3 forward; fenerf_siren_bwd16w.hip: bf16 backward chain):
// eight waves of a workgroup share one weight stream through an LDS ring filled by LDS-DMA, and every load of the stream loop sits in
// one in-order queue waited for with counted vmcnt.  What is here has ONE meaning in both kernels; the stream state (WStream,
// ws_issue, ws_step), the MFMA steps and the wait-count schedules differ between them and live in their files.
#pragma once
#include <hip/hip_runtime.h>

#include "fenerf_lane.h"
#include "fenerf_layout.h"

// The shipped defaults of two switches that A/B builds override (make EXTRA=-D...)
#ifndef FENERF_WAVE_HALF_COPIES
#define FENERF_WAVE_HALF_COPIES 1     // 0: the wave half (DMA at the top of a chunk step / half a step later) as a run-time flag inside the stream loop (rounds 2-5)
#endif
#ifndef FENERF_ST_POLICY
#define FENERF_ST_POLICY "nt"         // cache policy of the fire-and-forget tape / d(theta) stores (profiles/r06_store_policy_ab.txt)
#endif
// macros, hence outside the namespace: the exact-fp32 MFMA of the head products, and a compiler-only barrier between LDS phases
#define MFMA32W(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
#define LDS_FENCE() asm volatile("" ::: "memory")

namespace fenerf {
namespace wave16 {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int CH = FENERF_CH;        // stream entries (KiB) per chunk = one A operand per wave
constexpr int DPF = FENERF_DPF;      // chunks in flight ahead of the chunk being consumed
constexpr int NSLOT = FENERF_NSLOT;  // LDS ring slots; every stage is a whole number of ring revolutions (packer)
constexpr int NWAVE = 8;
static_assert(CH == NWAVE, "one 1-KiB A operand per wave and chunk");
static_assert(NSLOT >= DPF + 2, "a slot is refilled two barriers after its last reader issued its reads");

__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(size_t)(const __attribute__((address_space(3))) char*)p;
}
// An opaque copy of a lane-derived value.  LICM hoists lane-only address arithmetic out of the tile loop, where it stays live
// through every layer (58 such registers at first count) until the allocator spills it INTO the stream loop -- and scratch
// traffic there would break the counted vmcnt waits.  Deriving addresses from a fresh opaque copy at each use site keeps
// them local.
__device__ __forceinline__ int opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}
// a wave-uniform pointer the compiler computed with vector instructions (64-bit multiplies) -> SGPRs, for "s" asm operands
template <class T>
__device__ __forceinline__ T* uniform_ptr(T* p) {
  const unsigned long long v = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return reinterpret_cast<T*>(((unsigned long long)hi << 32) | lo);
}
// wait until at most N of this wave's vector-memory operations are outstanding
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit field");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// LDS-DMA of one KiB: lane i's 16 bytes at g_uniform + voff  ->  lds_uniform + 16 i  (saddr form: one VGPR of address instead of
// two).  Inline asm on purpose: with the builtin hipcc tracks the DMA as a pending LDS write and drains the queue (vmcnt(0)) before
// every ring read.  The s_nop is the wait state between the write of M0 and the DMA that reads it.
__device__ __forceinline__ void glds_1k_s(const void* g_uniform, unsigned voff, unsigned lds_uniform) {
  asm volatile(
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %0, %1"
      :
      : "v"(voff), "s"(g_uniform), "s"(lds_uniform)
      : "memory");
}
// Fire-and-forget 16-byte stores, uniform base in SGPRs + one VGPR of lane offset: stores are not loads -- they only make the counted
// vmcnt waits stricter.  The s_nop is the hazard slot the compiler would insert behind a store of more than 8 bytes whose data
// registers the next VALU instruction overwrites -- it does not look inside an asm.
__device__ __forceinline__ void st_f4_nt(const void* g_uniform, unsigned voff, const f32x4& v) {
  asm volatile("global_store_dwordx4 %0, %1, %2 " FENERF_ST_POLICY "\n\ts_nop 1" : : "v"(voff), "v"(v), "s"(g_uniform) : "memory");
}
__device__ __forceinline__ void st_u4_nt(const void* g_uniform, unsigned voff, const u32x4& v) {
  asm volatile("global_store_dwordx4 %0, %1, %2 " FENERF_ST_POLICY "\n\ts_nop 1" : : "v"(voff), "v"(v), "s"(g_uniform) : "memory");
}

// A operands of one k32-step (both row tiles).  Ring slot layout = operand index (spl * 2 + rt) * 2 + hl, 1 KiB each; ring_lane = ring
// slot 0 + lane * 16.  Linear ds_read_b128, conflict-free.
struct AK { float4 hi[2], lo[2]; };
__device__ __forceinline__ void ring_read_lo(AK& a, const char* ring_lane, int slot, int spl) {
  const float4* p = reinterpret_cast<const float4*>(ring_lane + slot * (CH * 1024) + spl * 4096);
  a.lo[0] = p[1 * 64]; a.lo[1] = p[3 * 64];
}
__device__ __forceinline__ void ring_read_hi(AK& a, const char* ring_lane, int slot, int spl) {
  const float4* p = reinterpret_cast<const float4*>(ring_lane + slot * (CH * 1024) + spl * 4096);
  a.hi[0] = p[0 * 64]; a.hi[1] = p[2 * 64];
}

}  // namespace wave16
}  // namespace fenerf
