// Wave-tile machinery of the 256-row schedules (gemm8.hip, gemm8p.hip, gemm4w.hip; of it gemm8_tn.hip uses the tail waits), one
// definition each: the part image (128-byte rows, 16-byte chunk c of row r at chunk c ^ (r & 7)) as the DMA writes and the fragment reads
// address it, the row-group bases of an interior tile, the 16 MFMAs of an accumulator quadrant, the tail wait ladder.
#pragma once
#include "gemm_common.hpp"

// Per-thread byte offsets of a part's chunks: thread `tid` moves row r0 = tid >> 3 (and rows a fixed distance further) at the chunk
// column swizzled by the row.  B_INTERLEAVED (8-wave kernels): B parts interleave the four wave columns' 32-row halves.
template <bool B_INTERLEAVED = true>
__device__ __forceinline__ void part_voff(int tid, int64_t lda, int64_t ldb, unsigned& voff_a, unsigned& voff_b) {
  const int r0 = tid >> 3, cpos = tid & 7;
  const int c = cpos ^ (r0 & 7);
  const int rb = B_INTERLEAVED ? (r0 >> 5) * 64 + (r0 & 31) : r0;
  voff_a = (unsigned)((r0 * lda + c * 8) * 2);
  voff_b = (unsigned)((rb * ldb + c * 8) * 2);
}

// Interior 256 x 256 tiles (every row exists): a part's two chunks per thread are rows r0 and r0 + 64 of the part at the same swizzled
// chunk column, so their addresses are a WAVE-UNIFORM base per (operand, sub-part, j) -- held in SGPRs -- plus part_voff's 32-bit
// per-thread offset (+ 128 bytes per K-tile).  That removes the 64-bit VALU address arithmetic from every load section.
// RowGroupOrigin derives a base where it is used (a handful of SALU instructions); RowGroupBases keeps all eight.
struct RowGroupOrigin {
  const char *a0, *b0;   // byte pointers of the tile's first A / B row at k = 0
  int64_t lda2, ldb2;    // row strides in bytes
  __device__ __forceinline__ const char* a(int mq, int j) const { return a0 + (int64_t)(j * 128 + mq * 64) * lda2; }   // A rows m0 + j*128 + mq*64
  __device__ __forceinline__ const char* b(int nq, int j) const { return b0 + (int64_t)(j * 128 + nq * 32) * ldb2; }   // B rows n0 + j*128 + nq*32
};
struct RowGroupBases {
  const char* pa[2][2];   // [mq][j]
  const char* pb[2][2];   // [nq][j]
  __device__ __forceinline__ const char* a(int mq, int j) const { return pa[mq][j]; }
  __device__ __forceinline__ const char* b(int nq, int j) const { return pb[nq][j]; }
};
__device__ __forceinline__ void make_row_group_bases(RowGroupBases& r, const char* a0, const char* b0, int64_t lda2, int64_t ldb2) {
  const RowGroupOrigin o = {a0, b0, lda2, ldb2};
#pragma unroll
  for (int sub = 0; sub < 2; sub++)
#pragma unroll
    for (int j = 0; j < 2; j++) {
      r.pa[sub][j] = o.a(sub, j);
      r.pb[sub][j] = o.b(sub, j);
    }
}

// byte offset of 16-byte chunk c of part row pr
__device__ __forceinline__ int part_chunk_off(int pr, int c) { return pr * 128 + ((c ^ (pr & 7)) * 16); }
// Per-lane fragment byte offsets inside a part, [fragment][k-step], of wave (wm, wn) of the 2 x 4 grid: A fragments = rows wm*64 + i*16
// + frow of an A part, B fragments = rows wn*32 + j*16 + frow of a B part, 16-byte chunk ks*4 + fg.
__device__ __forceinline__ void frag_offsets(int (&a_off)[4][2], int (&b_off)[2][2], int wm, int wn, int frow, int fg) {
#pragma unroll
  for (int ks = 0; ks < 2; ks++) {
    const int c = ks * 4 + fg;
#pragma unroll
    for (int i = 0; i < 4; i++) a_off[i][ks] = part_chunk_off(wm * 64 + i * 16 + frow, c);
#pragma unroll
    for (int j = 0; j < 2; j++) b_off[j][ks] = part_chunk_off(wn * 32 + j * 16 + frow, c);
  }
}
// an A set (4 x 2 fragments) / a B set (2 x 2) from the part image at `slot`
__device__ __forceinline__ void frag_read_a(bf16x8_t (&ra)[4][2], const char* slot, const int (&a_off)[4][2]) {
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int ks = 0; ks < 2; ks++) ra[i][ks] = *(const bf16x8_t*)(slot + a_off[i][ks]);
}
__device__ __forceinline__ void frag_read_b(bf16x8_t (&rb)[2][2], const char* slot, const int (&b_off)[2][2]) {
#pragma unroll
  for (int j = 0; j < 2; j++)
#pragma unroll
    for (int ks = 0; ks < 2; ks++) rb[j][ks] = *(const bf16x8_t*)(slot + b_off[j][ks]);
}

// The 16 MFMAs of accumulator quadrant (QI, QJ) of the 128 x 64 wave tile x K = 64, operands swapped (D = Bfrag x Afrag)
template <int QI, int QJ>
__device__ __forceinline__ void quad_mma(f32x4_t (&acc)[8][4], const bf16x8_t (&rb)[2][2], const bf16x8_t (&ra)[4][2]) {
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int ks = 0; ks < 2; ks++)
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
        acc[4 * QI + i][2 * QJ + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rb[j][ks], ra[i][ks], acc[4 * QI + i][2 * QJ + j], 0, 0, 0);
  __builtin_amdgcn_s_setprio(0);
}

// Tail of a K loop: the part that must have landed has `n` younger parts (DMA_PER_PART instructions per thread each, at most MAX of
// them) behind it, which may stay in flight
template <int DMA_PER_PART, int MAX = 2>
__device__ __forceinline__ void wait_younger_parts(int n) {
  if (MAX >= 3 && n >= 3) wait_vmcnt<3 * DMA_PER_PART>();
  else if (n >= 2) wait_vmcnt<2 * DMA_PER_PART>();
  else if (n == 1) wait_vmcnt<DMA_PER_PART>();
  else wait_vmcnt<0>();
}

// gemm_dbg bit 0 (no output traffic): one store that never happens keeps the accumulators alive
__device__ __forceinline__ void acc_sink(const GemmArgs& p, const f32x4_t (&acc)[8][4]) {
  if (acc[0][0][0] == 12345.678f && acc[7][3][3] == 0.5f) *(float*)p.C = acc[3][2][1];
}
