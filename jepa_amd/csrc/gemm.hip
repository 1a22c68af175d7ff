// bf16 MFMA GEMM for gfx950:  C[M,N] = A[M,K] * B[N,K]^T   (both operands K-contiguous, fp32 accumulate)
//
// This one core serves every Linear of the V-JEPA step (reference: nn.Linear call sites modules.py:31-34,63,76;
// predictor.py:194,237; Conv3d patch embed patch_embed.py:56 after tubelet packing):
//   fwd    Y  = X  * W^T            A = X  [M,K],      B = W   [N,K]
//   dgrad  dX = dY * W              A = dY [M,N],      B = W^T [K,N]   (bf16 transposed weight shadow)
//   wgrad  dW = dY^T * X            A = dY^T [N,Mpad], B = X^T [K,Mpad] -> fp32 straight into the grad arena
//
// Structure: 128x128 block tile, 4 waves (2x2), each wave 64x64 = 4x4 MFMA 16x16x32 tiles; K-tile 64 (32 as a
// fallback when K % 64 != 0); two LDS buffers; ONE barrier per K-tile; tile t+1 is staged while tile t is
// multiplied.  Staging is LDS-DMA (global_load_lds_dwordx4: no VGPR round trip) with the XOR swizzle applied on the
// per-lane SOURCE address (the DMA destination is lane-linear).  The MFMA is issued with swapped operands (D = Bfrag x Afrag) so each lane owns four
// CONSECUTIVE output columns: 8-byte bf16 / 16-byte fp32 epilogue accesses for C, bias, residual and aux.
// Workgroup ids are remapped so every XCD (private L2) works on a contiguous band of tiles.  Shared with the other GEMM files
// (gemm_common.hpp): xcd_logical / tile_of / unit_k_range, called one by one as in gemm8.hip (gemm_unit, which wraps them, reorders this
// kernel's prologue: profiles/gemm_bodies_refactor.md), the launcher preamble and the epilogues.
#include "gemm_common.hpp"
#include "internal.hpp"
#include "options.hpp"
#include <cstdlib>

// tile configurations: <BM, BN, WM, WN> = block tile and wave grid; each wave owns (BM/WM) x (BN/WN)
//   128x128, 2x2 waves (64x64 per wave)  : 64 KB LDS, 2 workgroups / CU -- small / skinny problems
//   256x256, 2x4 waves (128x64 per wave) : 128 KB LDS, 1 workgroup / CU, 2 waves / SIMD -- 2x the L2->LDS reuse
//   256x128, 2x2 waves (128x64 per wave) : BK32 x 3 stages = 72 KB, 2 INDEPENDENT workgroups / CU: one workgroup's
//                                          prologue / epilogue overlaps the other's K loop (short-K shapes)

// 16-byte-chunk XOR swizzle of a tile row (rows are BK*2 bytes): makes every ds_read_b128 lane group of a fragment
// read hit 16 distinct 16-byte slots of the 256-byte bank row.  BK=64 (8 chunks/row): chunk ^= row&7.
// BK=32 (4 chunks/row, 4 rows per bank row): chunk ^= (4 - ((row>>2)&3)) & 3.
template <int BK>
__device__ __forceinline__ int swz_of(int row) {
  return BK == 64 ? (row & 7) : ((4 - ((row >> 2) & 3)) & 3);
}

// ---- staging: one 128 x BK bf16 operand tile -> LDS (lane-linear image, source-side swizzle) ----
template <int BK, int ROWS, int NT>
__device__ __forceinline__ void stage_issue(const bf16_t* __restrict__ G, int64_t ld, int64_t row0, int64_t rows,
                                            int64_t k0, char* lds_tile, int tid, int wave_u) {
  constexpr int CPR = BK / 8;                  // 16-byte chunks per tile row
  constexpr int NIT = (ROWS * CPR) / NT;       // chunks per thread
#pragma unroll
  for (int j = 0; j < NIT; j++) {
    const int q = j * NT + tid;
    const int row = q / CPR, cpos = q % CPR;
    const int c = cpos ^ swz_of<BK>(row);
    int64_t gr = row0 + row;
    gr = gr < rows ? gr : rows - 1;            // clamp: tail rows are never stored
    const bf16_t* src = G + gr * ld + k0 + c * 8;
    char* dst = lds_tile + (j * NT + wave_u * 64) * 16;  // wave-uniform base; HW adds lane*16
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
  }
}

// NS = LDS ring depth.  NS == 2 is the classic double buffer (stage t+1 while multiplying t, drain before the
// barrier).  NS > 2 keeps NS-2 stages of LDS-DMA in flight ACROSS the per-K-tile barrier with a counted
// s_waitcnt vmcnt (never 0 in steady state) and a raw s_barrier, which is what hides HBM/L2 latency when the
// K loop is short (K = 1024 / 384 in this model).
template <int BK, int NS, int EPI, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(WM * WN * 64, (WM * WN == 4 ? 2 : 1)) void gemm_nt_kernel(GemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NT = WM * WN * 64;
  constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE_BYTES = A_BYTES + B_BYTES;
  constexpr int CPR = BK / 8;
  constexpr int NIT_A = (BM * CPR) / NT, NIT_B = (BN * CPR) / NT;
  constexpr int FM = BM / WM / 16, FN = BN / WN / 16;   // 16x16 MFMA tiles per wave
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave_u / WN, wn = wave_u % WN;

  // ---- XCD-aware, grouped tile mapping (bijective for any grid size) ----
  const int ntile = p.tiles_m * p.tiles_n;
  const int logical_all = xcd_logical(blockIdx.x, ntile * p.splitk);
  const int slice = logical_all / ntile;
  int tm, tn;
  tile_of(logical_all - slice * ntile, p.tiles_m, p.tiles_n, tm, tn);
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;

  f32x4_t acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; i++)
#pragma unroll
    for (int j = 0; j < FN; j++) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  int kt0, nkt;   // this workgroup's K-tile range (split-K for wgrads)
  unit_k_range<BK>(p, slice, kt0, nkt);

  // fragment read offsets (bytes inside a tile), constant across K-tiles
  const int frow = lane & 15, fg = lane >> 4;
  int a_off[FM][BK / 32], b_off[FN][BK / 32];
#pragma unroll
  for (int ks = 0; ks < BK / 32; ks++) {
    const int c = ks * 4 + fg;
#pragma unroll
    for (int i = 0; i < FM; i++) {
      const int r_ = wm * (FM * 16) + i * 16 + frow;
      a_off[i][ks] = r_ * (BK * 2) + ((c ^ swz_of<BK>(r_)) * 16);
    }
#pragma unroll
    for (int j = 0; j < FN; j++) {
      const int r_ = wn * (FN * 16) + j * 16 + frow;
      b_off[j][ks] = r_ * (BK * 2) + ((c ^ swz_of<BK>(r_)) * 16);
    }
  }

  constexpr int LOADS = NIT_A + NIT_B;  // LDS-DMA instructions per thread per stage
  // prologue: put the first NS-1 stages in flight
#pragma unroll
  for (int st = 0; st < NS - 1; st++) {
    if (st < nkt) {
      char* slot = smem + st * STAGE_BYTES;
      stage_issue<BK, BM, NT>(p.A, p.lda, m0, p.M, (int64_t)(kt0 + st) * BK, slot, tid, wave_u);
      stage_issue<BK, BN, NT>(p.B, p.ldb, n0, p.N, (int64_t)(kt0 + st) * BK, slot + A_BYTES, tid, wave_u);
    }
  }

  for (int it = 0; it < nkt; it++) {
    char* cur = smem + (it % NS) * STAGE_BYTES;
    char* nxt = smem + ((it + NS - 1) % NS) * STAGE_BYTES;
    // stage `it` must have landed; in steady state NS-2 younger stages stay in flight
    if (it + NS - 2 <= nkt - 1) wait_vmcnt<(NS - 2) * LOADS>();
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();  // every wave's DMA for stage `it` landed; every wave finished reading stage it-1
    if (it + NS - 1 < nkt) {
      stage_issue<BK, BM, NT>(p.A, p.lda, m0, p.M, (int64_t)(kt0 + it + NS - 1) * BK, nxt, tid, wave_u);
      stage_issue<BK, BN, NT>(p.B, p.ldb, n0, p.N, (int64_t)(kt0 + it + NS - 1) * BK, nxt + A_BYTES, tid, wave_u);
    }
#pragma unroll
    for (int ks = 0; ks < BK / 32; ks++) {
      bf16x8_t af[FM], bfr[FN];
#pragma unroll
      for (int j = 0; j < FN; j++) bfr[j] = *(const bf16x8_t*)(cur + A_BYTES + b_off[j][ks]);
#pragma unroll
      for (int i = 0; i < FM; i++) af[i] = *(const bf16x8_t*)(cur + a_off[i][ks]);
#pragma unroll
      for (int i = 0; i < FM; i++)
#pragma unroll
        for (int j = 0; j < FN; j++)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
    }
  }

  gemm_epilogue<EPI, FM, FN>(p, acc, m0 + wm * (FM * 16), n0 + wn * (FN * 16), frow, fg, slice);
}

// out[m][n] = alpha * sum_s ws[s][m][n] + beta * out[m][n]   (deterministic split-K combine)
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float4* __restrict__ ws, float* __restrict__ out,
                                                            int64_t M, int64_t N, int64_t ldc, int S, float alpha,
                                                            float beta) {
  const int64_t n4 = M * N / 4, nq = N / 4;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n4; q += (int64_t)gridDim.x * 256) {
    float4 acc = ws[q];
    for (int s = 1; s < S; s++) {
      const float4 v = ws[(int64_t)s * n4 + q];
      acc.x += v.x;
      acc.y += v.y;
      acc.z += v.z;
      acc.w += v.w;
    }
    const int64_t m = q / nq, n = (q - m * nq) * 4;
    float* cp = out + m * ldc + n;
    float4 o = make_float4(acc.x * alpha, acc.y * alpha, acc.z * alpha, acc.w * alpha);
    if (beta != 0.f) {
      const float4 c0 = *(const float4*)cp;
      o.x += beta * c0.x;
      o.y += beta * c0.y;
      o.z += beta * c0.z;
      o.w += beta * c0.w;
    }
    *(float4*)cp = o;
  }
}

// the split-K tail of every launcher (declared in gemm_common.hpp)
void vj_splitk_finish_plan(int nk, int& splitk, int& ktiles_per) {
  ktiles_per = (nk + splitk - 1) / splitk;
  splitk = (nk + ktiles_per - 1) / ktiles_per;   // no empty slices
}
int vj_splitk_reduce(const GemmArgs& b, hipStream_t stream) {
  if (b.splitk <= 1) return 0;
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(flat_grid(b.M * b.N / 4, 256 * 8)), dim3(256), 0, stream, (const float4*)b.ws,
                     (float*)b.C, b.M, b.N, b.ldc, b.splitk, b.alpha, b.beta);
  VJ_LAUNCH_CHECK("vj_gemm_bf16(split-K reduce)");
  return 0;
}

template <int BK, int NS, int EPI, int BM, int BN, int WM, int WN>
static int launch_gemm(const GemmArgs& a, void* ws, int64_t ws_bytes, hipStream_t stream) {
  constexpr int smem = NS * (BM + BN) * BK * 2;
  set_max_dynamic_lds<gemm_nt_kernel<BK, NS, EPI, BM, BN, WM, WN>>(smem);
  // wgrad: fill the chip (>= 2 waves of workgroups); each slice keeps >= 8 K-tiles of work.  Concurrent workgroups per round: 2 per CU for
  // the 4-wave tiles, 1 per CU for 256x256; K-tile time scales with the tile area and BK
  const int slots = (BM * BN >= 256 * 256) ? 256 : 512;
  const double us_kt = 1.45 * ((double)BM * BN * BK) / (256.0 * 256.0 * 64.0) * (slots == 512 ? 2.6 : 1.3);
  GemmArgs b = a;
  plan_tiles(b, BM, BN, BK, slots, us_kt, EPI == EPI_F32 ? ws : nullptr, ws_bytes);
  const int nblk = b.tiles_m * b.tiles_n * b.splitk;
  hipLaunchKernelGGL((gemm_nt_kernel<BK, NS, EPI, BM, BN, WM, WN>), dim3(nblk), dim3(WM * WN * 64), smem, stream,
                     b);
  VJ_LAUNCH_CHECK("vj_gemm_bf16_nt");
  return vj_splitk_reduce(b, stream);
}

// flags: bits 4-5 = tile config (0 auto, 1 = 128x128, 2 = 256x256); bits 6-7 = pipeline (0 auto, 1 = BK64 double buffer, 2 = BK32 4-stage
//        ring with counted vmcnt, 3 = 256x256 staggered 8-phase schedule, gemm8.hip / gemm8p.hip); bit 8 = the 4-wave 256x128 kernel with two
//        workgroups per CU (gemm4w.hip: single-stream inference).  (Register-staged operands, a 256x128 BK32 ring and a persistent form of
//        the 4-wave kernel existed through round 5; all measured slower in the step: profiles/r03_abab_switches.md, r05_gemm_4wp.md.)
//        The launchers behind the selection (gemm8.hip, gemm4w.hip, gemm8p.hip) are declared in internal.hpp.

extern "C" int64_t vj_gemm_colsum_rows(int64_t M) { return 2 * cdiv64(M, 256); }   // rows of colpart: (row tile, wave row) slots

// vj_gemm_bf16_nt_dgelu_colsum's request: column sums of the output into colpart[rows][N] IF the persistent kernel takes the problem
struct ColsumReq {
  float* colpart;
  int64_t rows;
  int* fused;   // out: 1 when the sums were written
};

// the automatic selection hands a problem to the 256x256 8-phase kernels (gemm8p.hip / gemm8.hip) from this many 256x256 tiles on
constexpr int64_t AUTO_256_MIN_TILES = 90, AUTO_256_MIN_TILES_WGRAD = 40;

template <int EPI>
static int dispatch_gemm(GemmArgs a, int flags, void* ws, int64_t ws_bytes, hipStream_t stream, const ColsumReq* cs) {   // (a, flags: by value, edited below)
  int cfg = (flags >> 4) & 3;
  int pipe = (flags >> 6) & 3;
  const bool is_wgrad = (EPI == EPI_F32 && ws != nullptr);
  bool auto_256 = false;
  if (a.lnf_rs != nullptr) flags &= ~0x100;   // the 4-wave kernel carries no folded-LayerNorm epilogue
  // bit 8: the 4-wave 256x128 kernel with two workgroups per CU (gemm4w.hip)
  if ((flags & 0x100) && a.K % 64 == 0) return vj_gemm_launch_4w(a, EPI, ws, ws_bytes, stream);
  if (pipe == 0 && cfg == 0) {
    // measured on the ViT-L step shapes (tools/gemm_bench.py): the staggered 8-phase 256x256 kernel wins on every
    // forward / dgrad shape with >= ~90 tiles; split-K wgrads (few tiles, long K) stay on 128x128 with 2 workgroups
    // per CU.  The 4-wave 256x128 kernel with two workgroups per CU (gemm4w.hip) is FASTER in isolation on most step
    // shapes (+35 % on the K = N = 1024 projection, +32 % predictor qkv, +17 % patch embed / context qkv: the tile-fixed
    // costs hide under the co-resident workgroup) and makes a single-stream step 1.9 % faster, but the training step
    // runs two HIP streams, where the other stream's kernels already fill the 8-phase kernel's idle CUs, and half-CU
    // workgroups then share CUs with attention / LayerNorm workgroups at half of their tuned occupancy: same-box A/B
    // 87.0 ms (8-phase) vs 90.0 ms (4-wave) per step, for every selection policy tried.  So it is opt-in: flags bit 8 or
    // VJ_GEMM_4W=1 (all forward / dgrad GEMMs), meant for single-stream use (inference, profiling).
    const int64_t t4w = cdiv64(a.M, 256) * cdiv64(a.N, 128);
    const int use_4w = a.lnf_rs != nullptr ? 0 : vj_opt(VJ_OPT_GEMM_4W);
    if (use_4w == 1 && !is_wgrad && a.K % 64 == 0 && t4w >= 64) return vj_gemm_launch_4w(a, EPI, ws, ws_bytes, stream);
    const int64_t t256 = cdiv64(a.M, 256) * cdiv64(a.N, 256);
    // (qkv/fc1/fc2 wgrads: 8-phase + split-K, 0.97-1.08 vs 0.78-0.96 PF)
    auto_256 = a.K % 64 == 0 && t256 >= (is_wgrad ? AUTO_256_MIN_TILES_WGRAD : AUTO_256_MIN_TILES);
    if (auto_256) pipe = 3;
  }
  if (cfg == 0) cfg = 1;
  if (pipe == 0) pipe = 1;       // BK64 double buffer (beats the BK32 ring on every step shape)
  if (a.K % 64 != 0) pipe = 2;   // K % 32 only fits the BK32 pipeline
  if (pipe == 3 && a.K % 64 == 0) {
    // persistent variant (gemm8p.hip): one workgroup per CU walks its tiles, next tile's operands prefetched under the
    // current tile, epilogue stores drained under the next K loop; bit-identical outputs.  Run-time option "gemm_persist".
    if (EPI != EPI_F32 && vj_opt(VJ_OPT_GEMM_PERSIST) != 0 && !(a.dbg & 2)) {
      // fused column sums: only where the automatic selection itself picked this kernel (no flags, no 4-wave or diagnostic option)
      if (EPI == EPI_DGELU && cs != nullptr && cs->colpart != nullptr && auto_256 && flags == 0 && vj_opt(VJ_OPT_GEMM_4W) == 0 && a.dbg == 0) {
        VJ_CHECK_ARG(cs->rows >= vj_gemm_colsum_rows(a.M), "vj_gemm_bf16_nt_dgelu_colsum: colpart has %ld rows, needs %ld", (long)cs->rows,
                     (long)vj_gemm_colsum_rows(a.M));
        a.colpart = cs->colpart;
        const int rc = vj_gemm_launch_8phase_persist(a, EPI, stream);
        if (rc != VJ_PERSIST_NA) {
          *cs->fused = (rc == 0);
          return rc;
        }
        a.colpart = nullptr;   // declined (aliasing operands, N % 8, a misaligned colpart): the plain GEMM, the caller sums C itself
      }
      const int rc = vj_gemm_launch_8phase_persist(a, EPI, stream);
      if (rc != VJ_PERSIST_NA) return rc;
    }
    if (a.lnf_rs == nullptr) return vj_gemm_launch_8phase(a, EPI, ws, ws_bytes, stream);
    pipe = 1;   // folded LayerNorm: only the persistent kernel and the generic kernels below carry that epilogue
    if (cfg == 1 && a.M >= 256 && a.N >= 256) cfg = 2;
  }
  if (pipe == 3) pipe = 1;
  if (pipe == 1)
    return cfg == 2 ? launch_gemm<64, 2, EPI, 256, 256, 2, 4>(a, ws, ws_bytes, stream)
                    : launch_gemm<64, 2, EPI, 128, 128, 2, 2>(a, ws, ws_bytes, stream);
  return cfg == 2 ? launch_gemm<32, 4, EPI, 256, 256, 2, 4>(a, ws, ws_bytes, stream)
                  : launch_gemm<32, 4, EPI, 128, 128, 2, 2>(a, ws, ws_bytes, stream);
}

static int gemm_entry(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M,
                      int64_t N, int64_t K, const float* bias, const void* residual, int64_t ldr, const void* aux_in,
                      void* aux_out, int64_t ldaux, int epilogue, float alpha, float beta, int flags, void* ws,
                      int64_t ws_bytes, hipStream_t stream, const float* lnf_rs = nullptr, const float* lnf_c = nullptr,
                      const ColsumReq* cs = nullptr) {
  VJ_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "vj_gemm_bf16_nt: negative dim");
  if (M == 0 || N == 0) return 0;
  VJ_CHECK_ARG(K > 0 && K % 32 == 0, "vj_gemm_bf16_nt: K=%ld must be a positive multiple of 32 (pad the operands)", (long)K);
  VJ_CHECK_ARG(N % 4 == 0, "vj_gemm_bf16_nt: N=%ld must be a multiple of 4", (long)N);
  VJ_CHECK_ARG(lda % 8 == 0 && ldb % 8 == 0 && lda >= K && ldb >= K,
               "vj_gemm_bf16_nt: lda/ldb must be multiples of 8 and >= K (lda=%ld ldb=%ld K=%ld)", (long)lda,
               (long)ldb, (long)K);
  VJ_CHECK_ARG(((uintptr_t)A % 16 == 0) && ((uintptr_t)B % 16 == 0), "vj_gemm_bf16_nt: A/B must be 16-byte aligned");
  VJ_CHECK_ARG(ldc % 4 == 0 && ldc >= N, "vj_gemm_bf16_nt: ldc=%ld must be a multiple of 4 and >= N", (long)ldc);
  float qscale = 0.f;
  if (epilogue == EPI_QKV_API) {   // qkv projection whose q third carries alpha (= scale * log2 e): bf16 epilogue + column scale
    VJ_CHECK_ARG(N % 12 == 0 && residual == nullptr && alpha != 0.f, "vj_gemm_bf16_nt: epilogue 4 needs N %% 12 == 0, no residual, alpha != 0");
    qscale = alpha;
    epilogue = EPI_BF16;
  }
  VJ_CHECK_ARG(epilogue >= EPI_BF16 && epilogue <= EPI_F32, "vj_gemm_bf16_nt: unknown epilogue %d", epilogue);
  VJ_CHECK_ARG((uintptr_t)C % (epilogue == EPI_F32 ? 16 : 8) == 0, "vj_gemm_bf16_nt: C misaligned");
  if (epilogue == EPI_DGELU) VJ_CHECK_ARG(aux_in != nullptr && ldaux % 4 == 0, "vj_gemm_bf16_nt: EPI_DGELU needs aux_in");
  if (residual) VJ_CHECK_ARG(epilogue == EPI_BF16 && ldr % 4 == 0, "vj_gemm_bf16_nt: residual only with EPI_BF16");
  GemmArgs a;
  a.A = (const bf16_t*)A; a.B = (const bf16_t*)B; a.C = C; a.bias = bias; a.res = (const bf16_t*)residual;
  a.aux_in = (const bf16_t*)aux_in; a.aux_out = (bf16_t*)aux_out;
  a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldb = ldb; a.ldc = ldc; a.ldr = ldr; a.ldaux = ldaux;
  a.alpha = alpha; a.beta = beta;
  a.dbg = vj_opt(VJ_OPT_GEMM_DBG);
  a.lnf_rs = lnf_rs;
  a.lnf_c = lnf_c;
  a.qscale = qscale;
  a.qcols = qscale != 0.f ? N / 3 : 0;
  return with_epilogue(epilogue, ws, ws_bytes, [&](auto epi, void* w, int64_t wb) {
    return dispatch_gemm<decltype(epi)::value>(a, flags, w, wb, stream, cs);
  });
}

extern "C" int vj_gemm_bf16_nt(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                               int64_t M, int64_t N, int64_t K, const float* bias, const void* residual, int64_t ldr,
                               const void* aux_in, void* aux_out, int64_t ldaux, int epilogue, float alpha,
                               float beta, int flags, hipStream_t stream) {
  return gemm_entry(A, lda, B, ldb, C, ldc, M, N, K, bias, residual, ldr, aux_in, aux_out, ldaux, epilogue, alpha, beta,
                    flags, nullptr, 0, stream);
}

// LayerNorm folded into the Linear that consumes it (round 5): C = LayerNorm(X) W^T + b computed from the RAW rows X as
//   C[m,n] = rstd_m * (sum_k X[m,k] Wf[n,k] - mean_m * c[n]) + bf[n],   Wf = bf16(W diag(gamma)), c[n] = sum_k Wf[n,k], bf = b + W beta
// (vj_ln_fold_weights prepares Wf / c / bf, vj_ln_rowstats the rows' {rstd, -mean * rstd}): the LayerNorm output is never written or
// re-read, and the activation is rounded to bf16 once less than on the unfused path.  epilogue: 0 (bf16), 1 (GELU, no saved
// derivative) or 4 (bf16 with the first N/3 columns times alpha: the q third of a qkv projection).  Replaces: norm1 -> attn.qkv and
// norm2 -> mlp.fc1 of a Block whose backward never runs (the EMA target encoder, frozen-encoder inference): modules.py:115,119.
extern "C" int vj_gemm_bf16_nt_lnfold(const void* X, int64_t ldx, const void* Wf, int64_t ldw, void* C, int64_t ldc, int64_t M,
                                      int64_t N, int64_t K, const float* bias_f, const float* rowstats, const float* colsum_w,
                                      int epilogue, float alpha, int flags, hipStream_t stream) {
  VJ_CHECK_ARG(bias_f != nullptr && rowstats != nullptr && colsum_w != nullptr, "vj_gemm_bf16_nt_lnfold: bias_f / rowstats / colsum_w must be given");
  VJ_CHECK_ARG(epilogue == EPI_BF16 || epilogue == EPI_GELU || epilogue == EPI_QKV_API, "vj_gemm_bf16_nt_lnfold: epilogue %d (0, 1 or 4)", epilogue);
  VJ_CHECK_ARG(((uintptr_t)rowstats % 8 == 0) && ((uintptr_t)colsum_w % 16 == 0) && ((uintptr_t)bias_f % 16 == 0),
               "vj_gemm_bf16_nt_lnfold: rowstats / colsum_w / bias_f misaligned");
  return gemm_entry(X, ldx, Wf, ldw, C, ldc, M, N, K, bias_f, nullptr, 0, nullptr, nullptr, 0, epilogue, alpha, 0.0f, flags, nullptr, 0,
                    stream, rowstats, colsum_w);
}

// fc2 dgrad with the bias gradient of fc1 fused: C = (A B^T) * aux_in (EPI_DGELU) and, when the persistent 256x256 kernel
// takes the problem, colpart[2 * cdiv(M,256)][N] = per-(row tile, wave row) fp32 column sums of C before the bf16 rounding
// (*fused = 1; reduce them with vj_reduce_segments).  Otherwise the plain GEMM runs and *fused = 0 (the caller sums C itself).
// C is bit-identical to vj_gemm_bf16_nt's either way.  Replaces: autograd of Mlp.fc1's bias (modules.py:31-34).
extern "C" int vj_gemm_bf16_nt_dgelu_colsum(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                                            int64_t M, int64_t N, int64_t K, const void* aux_in, int64_t ldaux,
                                            float* colpart, int64_t colpart_rows, int flags, int* fused,
                                            hipStream_t stream) {
  VJ_CHECK_ARG(fused != nullptr, "vj_gemm_bf16_nt_dgelu_colsum: null `fused`");
  *fused = 0;
  const ColsumReq cs = {colpart, colpart_rows, fused};
  return gemm_entry(A, lda, B, ldb, C, ldc, M, N, K, nullptr, nullptr, 0, aux_in, nullptr, ldaux, EPI_DGELU, 1.0f, 0.0f, flags,
                    nullptr, 0, stream, nullptr, nullptr, &cs);
}

// wgrad form: C (fp32) = alpha * A B^T + beta * C with the long K (= tokens) dimension split across workgroups
// when the [M,N] tile grid alone cannot fill 256 CUs; partials are combined deterministically from `ws`.
extern "C" int vj_gemm_bf16_nt_splitk(const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t ldc,
                                      int64_t M, int64_t N, int64_t K, float alpha, float beta, int flags, void* ws,
                                      int64_t ws_bytes, hipStream_t stream) {
  VJ_CHECK_ARG(ws != nullptr && ws_bytes >= M * N * 4, "vj_gemm_bf16_nt_splitk: workspace must hold at least M*N fp32");
  return gemm_entry(A, lda, B, ldb, C, ldc, M, N, K, nullptr, nullptr, 0, nullptr, nullptr, 0, EPI_F32, alpha, beta,
                    flags, ws, ws_bytes, stream);
}
