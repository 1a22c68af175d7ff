// 8-phase bf16 MFMA GEMM for gfx950: C[M,N] = A[M,K] * B[N,K]^T, 256x256 tile, 8 waves (2 x 4), BK = 64.
//
// Schedule (two K-tiles = 8 phases per loop trip; all numbers per workgroup):
//   * A K-tile is staged as four 16 KB PARTS: B0, B1, A1 and (for the NEXT K-tile) A0, where A(mq) holds the 64
//     rows of m-fragments 4mq..4mq+3 of BOTH wave rows and B(nq) the 32 rows of n-fragments 2nq,2nq+1 of all four
//     wave columns.  Part q lives in LDS slot q % 8 (8 x 16 KB = 128 KB = two K-tiles).
//   * Phase q has a LOAD section L(q): ds_read_b128 the fragments of part q into one of four register sets
//     (RB0 | RB1 | RA1 | RA0-of-next-tile: 4 or 8 reads), issue the LDS-DMA of part q+4 (2 x global_load_lds_dwordx4
//     per thread), s_waitcnt vmcnt(6) so that part q+1 has landed while parts q+2..q+4 stay in flight ACROSS the
//     barrier; and a COMPUTE section C(q): 16 MFMA 16x16x32 (one quadrant of the wave's 128x64 tile x K=64) under
//     s_setprio 1.  Sections are separated by raw s_barrier (no vmcnt drain).
//   * Waves 0-3 and waves 4-7 (one of each per SIMD) run ONE barrier interval apart, so on every SIMD the LDS/DMA
//     section of one wave overlaps the MFMA section of the other.
// Hazards: part q is read only after a barrier that follows every thread's vmcnt for it (end of L(q-1)); its slot is
// re-filled by part q+8 issued in L(q+4), >= 7 barrier intervals after the last read.
// Shared with gemm8p.hip / gemm4w.hip (gemm_tile.hpp): part image offsets, fragment reads, quadrant MFMAs, row-group bases, tail waits;
// with every one-tile kernel (gemm_common.hpp): K range of a work unit, launcher preamble, epilogues.  Its own: the tile decode and the
// fragment-offset loops (profiles/gemm_bodies_refactor.md: the shared forms cost this kernel 1 - 2 %).
#include "gemm_tile.hpp"
#include "internal.hpp"

#define P8_BM 256
#define P8_BN 256
#define P8_BK 64

// Interior tiles (all 256 x 256 rows exist): wave-uniform row-group bases, fixed for the whole K loop, + one per-thread offset per operand
struct PartBase8 {
  RowGroupBases rg;
  unsigned voff_a, voff_b;
};

// issue the LDS-DMA of part q (q = -1 .. 4*nk-1) into slot (q+8) % 8
template <bool EDGE>
__device__ __forceinline__ void issue_part(const GemmArgs& p, const PartBase8& pb, int q, int64_t m0, int64_t n0, int kt0,
                                           char* smem, int tid, int wave_u) {
  // q = 4t+0 -> B0(t), 4t+1 -> B1(t), 4t+2 -> A1(t), 4t+3 -> A0(t+1);  q = -1 -> A0(0).  With qq = q + 1:
  // qq = 4T + kind, kind 0 = A0(T), 1 = B0(T), 2 = B1(T), 3 = A1(T)
  const int qq = q + 1;
  const int kind = qq & 3;
  const int t = qq >> 2;
  const unsigned slot = lds_addr(smem) + ((q + 8) & 7) * LDS_PART_BYTES;
  const bool isA = (kind == 0) || (kind == 3);
  const int sub = (kind == 0) ? 0 : (kind == 3 ? 1 : kind - 1);  // mq for A parts, nq for B parts
  if constexpr (!EDGE) {
    const unsigned koff = (unsigned)t * (P8_BK * 2);   // bytes along K
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const unsigned dst = slot + (j * 512 + wave_u * 64) * 16;
      if (isA) dma16_sv(pb.rg.a(sub, j), pb.voff_a + koff, dst);
      else dma16_sv(pb.rg.b(sub, j), pb.voff_b + koff, dst);
    }
    return;
  }
  const int64_t k0 = (int64_t)(kt0 + t) * P8_BK;
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int c16 = j * 512 + tid;            // 16-byte chunk index inside the part (linear LDS image)
    const int pr = c16 >> 3, cpos = c16 & 7;  // part row, chunk position
    const int c = cpos ^ (pr & 7);            // source-side XOR swizzle (the DMA destination is lane-linear)
    const bf16_t* src;
    if (isA) {
      int64_t gr = m0 + (pr >> 6) * 128 + sub * 64 + (pr & 63);
      gr = gr < p.M ? gr : p.M - 1;
      src = p.A + gr * p.lda + k0 + c * 8;
    } else {
      int64_t gr = n0 + (pr >> 5) * 64 + sub * 32 + (pr & 31);
      gr = gr < p.N ? gr : p.N - 1;
      src = p.B + gr * p.ldb + k0 + c * 8;
    }
    dma16_v(src, slot + (j * 512 + wave_u * 64) * 16);
  }
}

// One workgroup's tile.  EDGE: the tile sticks out of the matrix (per-chunk clamped 64-bit addressing); interior tiles use
// the SGPR-base form.  Two instantiations of the same schedule; the kernel picks one per workgroup (uniform branch).
template <int EPI, bool EDGE>
__device__ __forceinline__ void gemm8_body(const GemmArgs& p, char* smem, int tm, int tn, int slice) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave_u >> 2, wn = wave_u & 3;
  const bool late_group = wave_u >= 4;        // waves 4-7 run one barrier interval behind waves 0-3
  const int frow = lane & 15, fg = lane >> 4;

  const int64_t m0 = (int64_t)tm * P8_BM, n0 = (int64_t)tn * P8_BN;
  int kt0, nk;   // this workgroup's K-tile range (split-K for wgrads)
  unit_k_range<P8_BK>(p, slice, kt0, nk);
  const int last_part = 4 * nk - 2;   // parts: -1 (A0 of tile 0), then per tile B0, B1, A1 and A0 of the next tile
  PartBase8 pb;
  if constexpr (!EDGE) {
    part_voff(tid, p.lda, p.ldb, pb.voff_a, pb.voff_b);
    make_row_group_bases(pb.rg, (const char*)(p.A + m0 * p.lda + (int64_t)kt0 * P8_BK), (const char*)(p.B + n0 * p.ldb + (int64_t)kt0 * P8_BK),
                         p.lda * 2, p.ldb * 2);
  }

  f32x4_t acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  bf16x8_t ra0[4][2], ra1[4][2], rb0[2][2], rb1[2][2];  // [fragment][k-step]

  // per-lane fragment byte offsets inside a part (frag_offsets' loops written out: the call moves this kernel's register allocation)
  int a_off[4][2], b_off[2][2];
#pragma unroll
  for (int ks = 0; ks < 2; ks++) {
    const int c = ks * 4 + fg;
#pragma unroll
    for (int i = 0; i < 4; i++) a_off[i][ks] = part_chunk_off(wm * 64 + i * 16 + frow, c);
#pragma unroll
    for (int j = 0; j < 2; j++) b_off[j][ks] = part_chunk_off(wn * 32 + j * 16 + frow, c);
  }

  // ---- prologue: parts -1 (A0 of tile 0), 0, 1, 2 in flight; part -1 landed for everyone
  issue_part<EDGE>(p, pb, -1, m0, n0, kt0, smem, tid, wave_u);
#pragma unroll
  for (int q = 0; q < 3; q++)
    if (q <= last_part) issue_part<EDGE>(p, pb, q, m0, n0, kt0, smem, tid, wave_u);
  if (last_part >= 2) wait_vmcnt<6>();
  else wait_vmcnt<0>();
  section_barrier();
  if (late_group) section_barrier();
  // L(-1): A0 fragments of tile 0; issue part 3; part 0 must have landed before the next barrier
  frag_read_a(ra0, smem + 7 * LDS_PART_BYTES, a_off);   // slot (-1 + 8) % 8
  if (3 <= last_part) issue_part<EDGE>(p, pb, 3, m0, n0, kt0, smem, tid, wave_u);
  if (3 <= last_part) wait_vmcnt<6>();
  else wait_vmcnt<0>();
  section_barrier();
  section_barrier();

  for (int t = 0; t < nk; t++) {
#pragma unroll
    for (int ph = 0; ph < 4; ph++) {
      const int q = 4 * t + ph;
      const char* slot = smem + (q & 7) * LDS_PART_BYTES;
      // ---------------- L(q)
#ifdef VJ_GEMM8_SKIP_READS   // timing experiment (A/B build `python -m jepa_amd.build skipreads -DVJ_GEMM8_SKIP_READS`): after the
      if (t > 0) {          // first K-tile the fragment reads are skipped -- WRONG results, same MFMA operands forever -- which
      } else                // bounds what moving the LDS reads out of the load sections could buy
#endif
      if (ph == 0) frag_read_b(rb0, slot, b_off);
      else if (ph == 1) frag_read_b(rb1, slot, b_off);
      else if (ph == 2) frag_read_a(ra1, slot, a_off);
      else if (t + 1 < nk) frag_read_a(ra0, slot, a_off);
      if (q + 4 <= last_part) {
        issue_part<EDGE>(p, pb, q + 4, m0, n0, kt0, smem, tid, wave_u);
        wait_vmcnt<6>();                              // part q+1 landed; q+2..q+4 in flight
      } else {
        wait_younger_parts<2>(last_part - (q + 1));   // tail: fewer younger parts behind part q+1
      }
      section_barrier();
      // ---------------- C(q): one quadrant x K = 64
      if (ph == 0) quad_mma<0, 0>(acc, rb0, ra0);
      else if (ph == 1) quad_mma<0, 1>(acc, rb1, ra0);
      else if (ph == 2) quad_mma<1, 1>(acc, rb1, ra1);
      else quad_mma<1, 0>(acc, rb0, ra1);
      section_barrier();
    }
  }
  if (!late_group) section_barrier();   // the early group matches the late group's extra barrier
  if (p.dbg & 1) {   // diagnostics: no output traffic (keeps the accumulators alive through one predicated store)
    acc_sink(p, acc);
    return;
  }
  // every wave is past its last LDS read and every DMA has landed: the ring is free, 16 KB of it per wave.
  // The lane id is re-derived here (mbcnt) so that nothing epilogue-only stays live across the K loop (256 VGPRs).
  const int elane = lane_id();
  const int efrow = elane & 15, efg = elane >> 4;
  if (!(p.dbg & 2) && gemm_epilogue_try_staged<EPI, 8, false>(p, acc, m0 + wm * 128, n0 + wn * 64, efrow, efg, elane,
                                                    smem + wave_u * 16384))
    return;
  gemm_epilogue<EPI, 8, 4, /*INTERIOR_VARIANT=*/(EPI == EPI_F32), false>(p, acc, m0 + wm * 128, n0 + wn * 64, efrow, efg, slice);
}

template <int EPI>
__global__ __launch_bounds__(512) void gemm_nt_8phase_kernel(GemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ntile = p.tiles_m * p.tiles_n;
  const int logical_all = xcd_logical(blockIdx.x, ntile * p.splitk);
  const int slice = logical_all / ntile;
  int tm, tn;
  tile_of(logical_all - slice * ntile, p.tiles_m, p.tiles_n, tm, tn);
#ifdef VJ_GEMM8_VADDR_ONLY   // A/B build: every tile on the per-chunk 64-bit addressing
  const bool interior = false;
#else
  const bool interior = ((int64_t)(tm + 1) * P8_BM <= p.M) && ((int64_t)(tn + 1) * P8_BN <= p.N);   // workgroup-uniform
#endif
  if (interior) gemm8_body<EPI, false>(p, smem, tm, tn, slice);
  else gemm8_body<EPI, true>(p, smem, tm, tn, slice);
}

template <int EPI>
static int launch8(const GemmArgs& a, void* ws, int64_t ws_bytes, hipStream_t stream) {
  constexpr int smem = 8 * LDS_PART_BYTES;
  set_max_dynamic_lds<gemm_nt_8phase_kernel<EPI>>(smem);
  GemmArgs b = a;   // wgrad: one workgroup per CU needs >= ~256 of them; >= 8 K-tiles per slice
  plan_tiles(b, P8_BM, P8_BN, P8_BK, 256, 1.45, EPI == EPI_F32 ? ws : nullptr, ws_bytes);
  hipLaunchKernelGGL(gemm_nt_8phase_kernel<EPI>, dim3(b.tiles_m * b.tiles_n * b.splitk), dim3(512), smem, stream, b);
  VJ_LAUNCH_CHECK("vj_gemm_bf16_nt(8-phase)");
  return vj_splitk_reduce(b, stream);
}

// entry used by gemm.hip's dispatcher (pipeline 3); requires K % 64 == 0
int vj_gemm_launch_8phase(const GemmArgs& a, int epilogue, void* ws, int64_t ws_bytes, hipStream_t stream) {
  return with_epilogue(epilogue, ws, ws_bytes, [&](auto epi, void* w, int64_t wb) { return launch8<decltype(epi)::value>(a, w, wb, stream); });
}
