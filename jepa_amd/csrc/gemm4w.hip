// Two-workgroups-per-CU bf16 MFMA GEMM for gfx950: C[M,N] = A[M,K] * B[N,K]^T, 256x128 tile, 4 waves (2 x 2), BK = 64.
//
// Why a second schedule next to gemm8.hip: the 8-wave 256x256 kernel owns a whole CU (8 x 256 VGPRs, 128 KB LDS), so
// the ~6.7 us a tile spends outside its K loop (first-DMA latency, epilogue stores) is time the CU's matrix pipes sit
// idle: 22 % of a K = 1024 tile, 43 % of a K = 384 one (profiles/r02_gemm_shapes_vitl16.md).  Here a workgroup is ONE
// wave per SIMD with the same 128x64 wave tile and the same phase structure, and TWO workgroups share a CU (2 x 80 KB
// LDS, 2 x 4 x 256 VGPRs): they are not synchronised with each other, so one workgroup's prologue / epilogue and
// LDS-load sections run under the other's MFMA sections -- the role the second wave group plays inside gemm8.hip -- and
// the tile grid is twice as fine (wave quantisation of the N = 1024 shapes).
//
// Schedule (4 phases per K-tile, one barrier per phase; all numbers per workgroup):
//   * a K-tile is staged as three 16 KB PARTS: B (128 n-rows: the 4 n-fragments of both wave columns), A1 (m-fragments
//     4..7 of both wave rows) and, for the NEXT K-tile, A0 (m-fragments 0..3).  Part p lives in slot (p + 5) % 5 of a
//     5 x 16 KB ring; parts are issued three ahead (one K-tile) and waited for with counted vmcnt (4 DMA instructions
//     per thread and part), never 0 inside the loop.
//   * phase 0: read rb0 (n-fragments 0,1) from B, issue part +3        | 16 MFMA  acc[0..3][0..1] += rb0 x ra0
//     phase 1: read rb1 (n-fragments 2,3) from B, wait for A1          | 16 MFMA  acc[0..3][2..3] += rb1 x ra0
//     phase 2: read ra1 from A1, issue part +3, wait for A0(next)      | 16 MFMA  acc[4..7][2..3] += rb1 x ra1
//     phase 3: read ra0(next) from A0, issue part +3, wait for B(next) | 16 MFMA  acc[4..7][0..1] += rb0 x ra1
// Hazards: a part is read only after a barrier that follows every thread's counted wait for it; a slot is re-filled at
// least two barriers after the section that read it last (see the slot arithmetic next to issue_part4).
// Shared with gemm8.hip / gemm8p.hip (gemm_tile.hpp): per-thread part offsets, quadrant MFMAs, tail waits; with every one-tile kernel
// (gemm_common.hpp): work-unit decode, launcher preamble, epilogues.  Its own: twelve row-group bases, fragments as two bases + immediates.
#include "gemm_tile.hpp"
#include "internal.hpp"
#include <type_traits>
#include <cstdlib>

#define W4_BM 256
#define W4_BN 128
#define W4_BK 64
#define W4_SLOTS 5

// part index p: -1 = A0(0);  3T = B(T), 3T+1 = A1(T), 3T+2 = A0(T+1).  Slot (p+5) % 5: part p+5 overwrites part p, and
// part p+5 is issued in the section that reads part p+2 -- part p was read three sections (>= 2 barriers) earlier.
// A part is 128 rows x 128 bytes = 1024 16-byte chunks; thread `tid` moves chunks tid, tid+256, tid+512, tid+768, i.e.
// rows r0, r0+32, r0+64, r0+96 (r0 = tid >> 3) at the same (swizzled) chunk column.  Interior tiles address them as
// WAVE-UNIFORM row-group base (SGPR pair, fixed for the whole K loop) + one 32-bit per-thread byte offset
// (row r0, swizzled chunk, + 128 bytes per K-tile): the saddr form of global_load_lds_dwordx4 (dma16_sv, lds_pipe.hpp).  No
// 64-bit VALU address arithmetic and two address VGPRs in total.
struct PartBase {
  const char* a[8];   // A0 chunks j = 0..3 (wave row j >> 1, rows +32 (j & 1)), then the same for A1 (+64 rows)
  const char* b[4];   // B chunks j = 0..3 (rows +32 j)
};

// interior tiles: all 256 x 128 rows exist.  kind 0: A0, 1: B, 2: A1.  voff already includes the K-tile's 128 bytes.
template <int KIND>
__device__ __forceinline__ void issue_fast(const PartBase& s, unsigned voff, unsigned lds_slot, int wave_u) {
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const char* base = KIND == 1 ? s.b[j] : s.a[(KIND == 2 ? 4 : 0) + j];
    dma16_sv(base, voff, lds_slot + j * 4096 + wave_u * 1024);   // chunk (j * 256 + wave * 64 + lane) * 16 bytes
  }
}

// edge tiles: rows beyond M / N re-read the last valid row (their products land in rows / columns that are never stored)
__device__ __forceinline__ void issue_edge(const GemmArgs& p, int kind, int tile, int64_t m0, int64_t n0, int kt0,
                                           char* slot, int tid, int wave_u) {
  const int64_t k0 = (int64_t)(kt0 + tile) * W4_BK;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int c16 = j * 256 + tid;            // 16-byte chunk index inside the part (linear LDS image)
    const int pr = c16 >> 3, cpos = c16 & 7;  // part row (0..127), chunk position
    const int c = cpos ^ (pr & 7);            // source-side XOR swizzle (the DMA destination is lane-linear)
    const bf16_t* src;
    if (kind != 1) {
      int64_t gr = m0 + (pr >> 6) * 128 + (kind == 2 ? 64 : 0) + (pr & 63);
      gr = gr < p.M ? gr : p.M - 1;
      src = p.A + gr * p.lda + k0 + c * 8;
    } else {
      int64_t gr = n0 + pr;                   // wave column (pr >> 6) * 64 + fragment row (pr & 63)
      gr = gr < p.N ? gr : p.N - 1;
      src = p.B + gr * p.ldb + k0 + c * 8;
    }
    char* dst = slot + (j * 256 + wave_u * 64) * 16;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
  }
}

// fragments first .. first + N - 1 of a part: fragment i sits 16 rows = 2048 bytes behind fragment 0 with the same swizzle key, so the two
// per-lane bases of fragment 0 (one per k-step) + immediates cover all of them
template <int N>
__device__ __forceinline__ void read_frags(bf16x8_t (&r)[N][2], const char* slot, const int (&base)[2], int first) {
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int ks = 0; ks < 2; ks++) r[i][ks] = *(const bf16x8_t*)(slot + base[ks] + (first + i) * 2048);
}

// K loop of one workgroup.  EDGE: the tile sticks out of the matrix (clamped per-chunk addressing); otherwise one base
// pointer per operand.  The steady state (all three look-ahead parts exist) is straight-line: unconditional issues and a
// constant vmcnt(8); the last two K-tiles run the same phases with existence checks and shrinking wait counts.
template <bool EDGE>
__device__ __forceinline__ void k_loop_4w(const GemmArgs& p, char* smem, f32x4_t (&acc)[8][4], int64_t m0, int64_t n0,
                                          int kt0, int nk, int tid, int wave_u, int wm, int wn, int frow, int fg) {
  const int last_part = 3 * nk - 2;   // A1 of the last K-tile
  bf16x8_t ra0[4][2], ra1[4][2], rb0[2][2], rb1[2][2];  // [fragment][k-step]
  // per-lane fragment byte offsets inside a part (128-byte rows, chunks swizzled by row & 7): fragment i of a wave sits
  // 16 rows = 2048 bytes further with the same swizzle key, so two bases per operand + immediates cover all of them
  int a_base[2], b_base[2];
#pragma unroll
  for (int ks = 0; ks < 2; ks++) {
    const int c = ks * 4 + fg;
    a_base[ks] = part_chunk_off(wm * 64 + frow, c);
    b_base[ks] = part_chunk_off(wn * 64 + frow, c);
  }
  PartBase src;
  unsigned voff_a = 0, voff_b = 0;
  if constexpr (!EDGE) {
    part_voff<false>(tid, p.lda, p.ldb, voff_a, voff_b);   // rows r0 + 32 j share r0 & 7
    const char* a0 = (const char*)(p.A + m0 * p.lda + (int64_t)kt0 * W4_BK);
    const char* b0 = (const char*)(p.B + n0 * p.ldb + (int64_t)kt0 * W4_BK);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      src.a[j] = a0 + ((j >> 1) * 128 + (j & 1) * 32) * p.lda * 2;
      src.a[4 + j] = a0 + ((j >> 1) * 128 + (j & 1) * 32 + 64) * p.lda * 2;
      src.b[j] = b0 + (j * 32) * p.ldb * 2;
    }
  }
  const unsigned lds0 = lds_addr(smem);
  // kind: 0 A0, 1 B, 2 A1 ; tile = its K-tile ; sl = its ring slot
  auto issue = [&](auto kind_tag, int tile, int sl) {
    constexpr int KIND = decltype(kind_tag)::value;
    if constexpr (EDGE) issue_edge(p, KIND, tile, m0, n0, kt0, smem + sl * LDS_PART_BYTES, tid, wave_u);
    else issue_fast<KIND>(src, (KIND == 1 ? voff_b : voff_a) + (unsigned)tile * 128u, lds0 + sl * LDS_PART_BYTES, wave_u);
  };
  using K0 = std::integral_constant<int, 0>;
  using K1 = std::integral_constant<int, 1>;
  using K2 = std::integral_constant<int, 2>;
  int issued = -2;   // highest part index issued so far (only consulted by the tail iterations)
  auto issue_if = [&](int q, auto kind_tag, int tile, int sl) {
    if (q <= last_part) {
      issue(kind_tag, tile, sl);
      issued = q;
    }
  };
  auto wait_for = [&](int q) {   // this thread's share of part q has landed; younger parts stay in flight
    if (q <= last_part) wait_younger_parts<4>(issued - q);
  };

  // ---- prologue: A0(0) -> slot 4, B(0) -> 0, A1(0) -> 1 in flight; A0(0) and B(0) landed for everyone; A0(1) -> slot 2
  issue_if(-1, K0{}, 0, 4);
  issue_if(0, K1{}, 0, 0);
  issue_if(1, K2{}, 0, 1);
  wait_for(0);
  section_barrier();
  {
    read_frags(ra0, smem + 4 * LDS_PART_BYTES, a_base, 0);
    issue_if(2, K0{}, 1, 2);
  }

  int s0 = 0;   // ring slot of part 3t (B(t)); parts 3t+1 .. 3t+5 follow cyclically
  auto slot_of = [&](int d) {   // slot of part 3t + d, d = 0..5
    int s = s0 + d;
    return s >= 2 * W4_SLOTS ? s - 2 * W4_SLOTS : (s >= W4_SLOTS ? s - W4_SLOTS : s);
  };
  auto k_tile = [&](int t, auto tail_tag) {
    constexpr bool TAIL = decltype(tail_tag)::value;
    const int pb = 3 * t;
    // ---------------- phase 0: rb0 <- B(t); part +3 = B(t+1)
    {
      read_frags(rb0, smem + s0 * LDS_PART_BYTES, b_base, 0);
      if constexpr (TAIL) issue_if(pb + 3, K1{}, t + 1, slot_of(3));
      else issue(K1{}, t + 1, slot_of(3));
      section_barrier();
      quad_mma<0, 0>(acc, rb0, ra0);
    }
    // ---------------- phase 1: rb1 <- B(t); A1(t) must land
    {
      read_frags(rb1, smem + s0 * LDS_PART_BYTES, b_base, 2);
      if constexpr (TAIL) wait_for(pb + 1);
      else wait_younger_parts<4>(2);
      section_barrier();
      quad_mma<0, 1>(acc, rb1, ra0);
    }
    // ---------------- phase 2: ra1 <- A1(t); part +3 = A1(t+1); A0(t+1) must land
    {
      read_frags(ra1, smem + slot_of(1) * LDS_PART_BYTES, a_base, 0);
      if constexpr (TAIL) {
        issue_if(pb + 4, K2{}, t + 1, slot_of(4));
        wait_for(pb + 2);
      } else {
        issue(K2{}, t + 1, slot_of(4));
        wait_younger_parts<4>(2);
      }
      section_barrier();
      quad_mma<1, 1>(acc, rb1, ra1);
    }
    // ---------------- phase 3: ra0 <- A0(t+1); part +3 = A0(t+2); B(t+1) must land
    {
      if (!TAIL || t + 1 < nk) read_frags(ra0, smem + slot_of(2) * LDS_PART_BYTES, a_base, 0);
      if constexpr (TAIL) {
        issue_if(pb + 5, K0{}, t + 2, slot_of(5));
        wait_for(pb + 3);
      } else {
        issue(K0{}, t + 2, slot_of(5));
        wait_younger_parts<4>(2);
      }
      section_barrier();
      quad_mma<1, 0>(acc, rb0, ra1);
    }
    s0 = slot_of(3);
  };
  int t = 0;
  for (; t < nk - 2; t++) k_tile(t, std::false_type{});
  if (nk >= 3) issued = 3 * nk - 4;   // what the steady state left in flight: parts up to 3(nk-3)+5
  for (; t < nk; t++) k_tile(t, std::true_type{});
  wait_vmcnt<0>();
  section_barrier();   // every wave is past its last LDS read and every DMA has landed: the ring is free, 16 KB of it per wave
}

template <int EPI>
__global__ __launch_bounds__(256, 2) void gemm_nt_4w_kernel(GemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave_u >> 1, wn = wave_u & 1;
  const int frow = lane & 15, fg = lane >> 4;

  const GemmUnit u = gemm_unit<W4_BM, W4_BN, W4_BK>(p);
  const int64_t m0 = u.m0, n0 = u.n0;
  const bool interior = (m0 + W4_BM <= p.M) && (n0 + W4_BN <= p.N);   // workgroup-uniform

  f32x4_t acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  if (interior) k_loop_4w<false>(p, smem, acc, m0, n0, u.kt0, u.nk, tid, wave_u, wm, wn, frow, fg);
  else k_loop_4w<true>(p, smem, acc, m0, n0, u.kt0, u.nk, tid, wave_u, wm, wn, frow, fg);
  if (p.dbg & 1) {
    acc_sink(p, acc);
    return;
  }
  const int elane = lane_id();
  const int efrow = elane & 15, efg = elane >> 4;
  if (!(p.dbg & 2) && gemm_epilogue_try_staged<EPI, 8, false>(p, acc, m0 + wm * 128, n0 + wn * 64, efrow, efg, elane,
                                                              smem + wave_u * 16384))
    return;
  gemm_epilogue<EPI, 8, 4, /*INTERIOR_VARIANT=*/(EPI == EPI_F32), false>(p, acc, m0 + wm * 128, n0 + wn * 64, efrow, efg, u.slice);
}

// (A persistent form of this kernel -- two workgroups per CU walking tile lists -- was built in round 5: bit-identical, slower on every
//  shape and policy, profiles/r05_gemm_4wp.md.)

template <int EPI>
static int launch4w(const GemmArgs& a, void* ws, int64_t ws_bytes, hipStream_t stream) {
  constexpr int smem = W4_SLOTS * LDS_PART_BYTES;
  set_max_dynamic_lds<gemm_nt_4w_kernel<EPI>>(smem);
  static const bool occ_dbg = [] {
    if (getenv("VJ_GEMM_DBG_OCC")) {
      int n = -1;
      hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)gemm_nt_4w_kernel<EPI>, 256, smem);
      fprintf(stderr, "[vj] gemm_nt_4w_kernel<%d>: %d workgroups per CU (query rc %d, %d B dynamic LDS)\n", EPI, n, (int)e, smem);
    }
    return true;
  }();
  (void)occ_dbg;
  GemmArgs b = a;   // wgrad: 512 workgroup slots per round, K-tile time of a half-size tile
  plan_tiles(b, W4_BM, W4_BN, W4_BK, 512, 1.45, EPI == EPI_F32 ? ws : nullptr, ws_bytes);
  hipLaunchKernelGGL(gemm_nt_4w_kernel<EPI>, dim3(b.tiles_m * b.tiles_n * b.splitk), dim3(256), smem, stream, b);
  VJ_LAUNCH_CHECK("vj_gemm_bf16_nt(4-wave)");
  return vj_splitk_reduce(b, stream);
}

int vj_gemm_launch_4w(const GemmArgs& a, int epilogue, void* ws, int64_t ws_bytes, hipStream_t stream) {
  return with_epilogue(epilogue, ws, ws_bytes, [&](auto epi, void* w, int64_t wb) { return launch4w<decltype(epi)::value>(a, w, wb, stream); });
}
