// Pipeline primitives shared by the GEMM and attention kernels: LDS-DMA, counted waits and raw barriers, one definition each.
//
// The software-pipelined K loops keep several stages of global -> LDS copies in flight ACROSS workgroup barriers.  The compiler's own
// bookkeeping cannot express that, so these few lines are inline assembly ON PURPOSE:
//   * the LDS-DMA (global_load_lds_dwordx4) is issued where the compiler cannot see it.  It then neither tracks these loads in its
//     vmcnt bookkeeping nor knows that LDS is written behind its back, and so inserts no conservative `s_waitcnt vmcnt(0)` in front of
//     later LDS reads (it does after the builtin form -- for ds_read_b64_tr_b16 always -- which collapses the prefetch distance);
//   * completion is tracked by hand: wait_vmcnt<N>() = "at most N vector-memory operations of this wave still outstanding", followed by a
//     raw s_barrier.  vmcnt counts STORES as well as loads on gfx9; loads complete in order among themselves, so the wait still implies
//     that every load older than the N youngest operations has landed, whatever the stores do -- it is merely conservative while
//     stores are in flight.  The only waits inside a K loop are the counted ones placed by hand, never 0 in steady state.
#pragma once
#include "common.hpp"

#define LDS_PART_BYTES 16384   // one part of the 256-row GEMM schedules: 128 tile rows x 128 bytes (gemm8*.hip) / 64 tokens x 256 bytes (TN)

// compiler-only fence: no memory access is moved across it, no instruction is emitted
__device__ __forceinline__ void cfence() { asm volatile("" ::: "memory"); }

// Raw SECTION barrier of the phase schedules: s_barrier with no wait of any kind (no vmcnt drain as in __syncthreads()).  The
// sched_barrier pair is what keeps MFMA out of the load sections: nothing (MFMA, ds_read, DMA issue) may be scheduled across a section
// boundary.
__device__ __forceinline__ void section_barrier() {
  cfence();
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  cfence();
}
// The attention kernels' barrier is a DIFFERENT one: it first waits for this wave's own LDS reads of the previous tile (lgkmcnt(0),
// visible to the compiler) and has no sched_barrier pair -- those kernels have no hand-placed sections to protect.
__device__ __forceinline__ void lgkm_barrier() {
  cfence();
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0) only
  __builtin_amdgcn_s_barrier();
  cfence();
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// LDS byte address of a __shared__ pointer (the value m0 takes)
__device__ __forceinline__ unsigned lds_addr(const char* p) {
  return (unsigned)(size_t)(__attribute__((address_space(3))) const char*)p;
}

// 16 bytes per lane, global -> LDS, asynchronous.  lds_base must be wave-uniform: the hardware adds lane * 16 (the destination image is
// lane-linear, so any swizzle is applied to the per-lane SOURCE address).  Two addressing forms:
__device__ __forceinline__ void dma16_v(const void* gsrc, unsigned lds_base) {   // 64-bit per-lane address
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds_base), "v"(gsrc) : "memory");
}
// wave-uniform 64-bit base in SGPRs + 32-bit per-lane byte offset: no 64-bit vector address arithmetic (v_mad_u64_u32 / v_lshl_add_u64)
// per instruction and one address VGPR per operand -- the GEMM load sections and the attention kernels are bound by instruction issue.
// (a non-temporal hint on the streaming operand was measured in round 5: +1.4 / +2.8 ms per step, profiles/r05_gemm_nt.md)
__device__ __forceinline__ void dma16_sv(const void* sbase, unsigned voff, unsigned lds_base) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds_base), "v"(voff), "s"(sbase) : "memory");
}
