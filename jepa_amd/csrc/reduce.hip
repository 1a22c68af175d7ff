// bf16 transposes (the K-contiguous wgrad operands dY^T and X^T, the W^T dgrad shadows) and deterministic column sums
// (bias and mask-token gradients; the one reduction that ends a block's backward).
#include "common.hpp"
#include "internal.hpp"
#include "../../include/vjepa_hip.h"

// ---------------------------------------------------------------------------------------------
// One 64x64 tile of a transpose through LDS: in [M,N] (ld_in) -> out [N, Mpad], out[n, m>=M] = 0, 256 threads.
// transpose_load: each thread loads two 16-byte chunks of the tile at (m0, n0) into tile[64][66], then the barrier.
// transpose_store: each thread stores two packed 16-byte chunks of the transposed tile.  What a kernel does with the loaded tile
// between the two (the fused column sum of transpose_bf16_kernel) is written in that kernel.
// transpose_load returns a reference to a function-local __shared__ tile; it is __forceinline__, so the tile belongs to the kernel
// that calls it (8448 bytes of LDS each) and must be called once per kernel.
// ---------------------------------------------------------------------------------------------
typedef bf16_t TransposeTile[64][66];
__device__ __forceinline__ TransposeTile& transpose_load(const bf16_t* __restrict__ in, int64_t M, int64_t N, int64_t ld_in,
                                                         int64_t m0, int64_t n0) {
  __shared__ TransposeTile tile;
  const int t = threadIdx.x;
  // load: 64 rows x 8 chunks of 8 bf16
#pragma unroll
  for (int it = 0; it < 2; it++) {
    const int q = t + it * 256;
    const int r = q >> 3, c = (q & 7) * 8;
    u32x4_t v = {0, 0, 0, 0};
    if (m0 + r < M && n0 + c < N) v = *(const u32x4_t*)(in + (m0 + r) * ld_in + n0 + c);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      *(uint32_t*)&tile[r][c + 2 * i] = v[i];
    }
  }
  __syncthreads();
  return tile;
}
__device__ __forceinline__ void transpose_store(const TransposeTile& tile, bf16_t* __restrict__ out, int64_t N, int64_t Mpad,
                                                int64_t m0, int64_t n0) {
  const int t = threadIdx.x;
#pragma unroll
  for (int it = 0; it < 2; it++) {
    const int q = t + it * 256;
    const int n = q >> 3, mc = (q & 7) * 8;
    if (n0 + n < N && m0 + mc < Mpad) {
      u32x4_t o;
#pragma unroll
      for (int i = 0; i < 4; i++)
        o[i] = (uint32_t)tile[mc + 2 * i][n] | ((uint32_t)tile[mc + 2 * i + 1][n] << 16);
      *(u32x4_t*)(out + (n0 + n) * Mpad + m0 + mc) = o;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// transpose_bf16: in [M,N] (ld_in) -> out [N, Mpad], out[n, m>=M] = 0.  64x64 tiles through LDS.
// Feeds the K-contiguous ("NT") MFMA GEMM with the wgrad operands dY^T and X^T.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void transpose_bf16_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out,
                                                             int64_t M, int64_t N, int64_t ld_in, int64_t Mpad,
                                                             float* __restrict__ part) {
  const int64_t m0 = (int64_t)blockIdx.x * 64, n0 = (int64_t)blockIdx.y * 64;
  const int t = threadIdx.x;
  const TransposeTile& tile = transpose_load(in, M, N, ld_in, m0, n0);
  if (part != nullptr && t < 64 && n0 + t < N) {  // fused bias-gradient partial: column sums of this 64-row tile
    float sum = 0.f;
#pragma unroll 16
    for (int r = 0; r < 64; r++) sum += bf2f(tile[r][t]);
    part[(int64_t)blockIdx.x * N + n0 + t] = sum;
  }
  transpose_store(tile, out, N, Mpad, m0, n0);
}

extern "C" int vj_transpose_bf16(const void* in, void* out, int64_t M, int64_t N, int64_t ld_in, int64_t Mpad,
                                 hipStream_t stream) {
  VJ_CHECK_ARG(N % 8 == 0 && ld_in % 8 == 0 && Mpad % 8 == 0 && Mpad >= M,
               "vj_transpose_bf16: need N,ld_in,Mpad multiples of 8 and Mpad>=M (M=%ld N=%ld ld=%ld Mpad=%ld)",
               (long)M, (long)N, (long)ld_in, (long)Mpad);
  if (N == 0 || Mpad == 0) return 0;
  dim3 grid((unsigned)cdiv64(Mpad, 64), (unsigned)cdiv64(N, 64));
  hipLaunchKernelGGL(transpose_bf16_kernel, grid, dim3(256), 0, stream, (const bf16_t*)in, (bf16_t*)out, M, N, ld_in,
                     Mpad, (float*)nullptr);
  VJ_LAUNCH_CHECK("vj_transpose_bf16");
  return 0;
}

// transpose + bias gradient in one pass over dY: out = in^T (zero padded), colsum[n] = alpha*sum_m in[m][n] + beta*colsum[n]
extern "C" int64_t vj_transpose_colsum_ws_bytes(int64_t M, int64_t N) { return cdiv64(((M + 63) / 64) * 64, 64) * N * 4; }

extern "C" int vj_transpose_colsum_bf16(const void* in, void* out, int64_t M, int64_t N, int64_t ld_in, int64_t Mpad,
                                        float* colsum, float alpha, float beta, void* ws, int64_t ws_bytes,
                                        hipStream_t stream) {
  VJ_CHECK_ARG(N % 8 == 0 && ld_in % 8 == 0 && Mpad % 8 == 0 && Mpad >= M, "vj_transpose_colsum_bf16: bad dims");
  const int64_t mt = cdiv64(Mpad, 64);
  VJ_CHECK_ARG(ws_bytes >= mt * N * 4, "vj_transpose_colsum_bf16: workspace too small");
  if (N == 0 || Mpad == 0) return 0;
  dim3 grid((unsigned)mt, (unsigned)cdiv64(N, 64));
  hipLaunchKernelGGL(transpose_bf16_kernel, grid, dim3(256), 0, stream, (const bf16_t*)in, (bf16_t*)out, M, N, ld_in,
                     Mpad, (float*)ws);
  VJ_LAUNCH_CHECK("vj_transpose_colsum_bf16");
  return vj_reduce_partials((const float*)ws, colsum, mt, N, alpha, beta, stream);
}

// ---------------------------------------------------------------------------------------------
// transpose_multi: ONE launch that transposes many bf16 matrices (the W^T dgrad shadows of every Linear, refreshed
// once per optimizer step).  desc[t] = {src, dst, M, N, ld_in, Mpad}; blocks[b] = {tensor, tile_m, tile_n, 0}.
// ---------------------------------------------------------------------------------------------
struct TransposeDesc {
  const bf16_t* src;
  bf16_t* dst;
  int64_t M, N, ld_in, Mpad;
};

__global__ __launch_bounds__(256) void transpose_multi_kernel(const TransposeDesc* __restrict__ desc,
                                                              const int4* __restrict__ blocks) {
  const int4 bi = blocks[blockIdx.x];
  const TransposeDesc d = desc[bi.x];
  const int64_t m0 = (int64_t)bi.y * 64, n0 = (int64_t)bi.z * 64;
  transpose_store(transpose_load(d.src, d.M, d.N, d.ld_in, m0, n0), d.dst, d.N, d.Mpad, m0, n0);
}

// desc: device array of 6 x int64 per tensor {src, dst, M, N, ld_in, Mpad}; blocks: device int32[4*n_blocks]
extern "C" int vj_transpose_multi(const void* desc, const void* blocks, int64_t n_blocks, hipStream_t stream) {
  if (n_blocks == 0) return 0;
  VJ_CHECK_ARG(n_blocks < (1ll << 31), "vj_transpose_multi: too many blocks");
  hipLaunchKernelGGL(transpose_multi_kernel, dim3((unsigned)n_blocks), dim3(256), 0, stream,
                     (const TransposeDesc*)desc, (const int4*)blocks);
  VJ_LAUNCH_CHECK("vj_transpose_multi");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// colsum_bf16: partial[p][n] = sum over the p-th row chunk of in[m][n] (rows m in [row_lo,row_hi) of
// each group of `group` rows -- used both for plain bias grads (group = M) and for the mask-token grad,
// which sums only the target rows j >= Ke of every [Ke+Kp]-row sample).  Deterministic two-stage sum.
// ---------------------------------------------------------------------------------------------
#define VJ_COLSUM_PARTS 256   // maximum number of row chunks (workspace sizing); the launcher picks 33 .. 256 (vj_colsum_bf16)
__global__ __launch_bounds__(256) void colsum_bf16_kernel(const bf16_t* __restrict__ in, float* __restrict__ part,
                                                          int64_t M, int64_t N, int64_t ld, int64_t group,
                                                          int64_t row_lo, int64_t row_hi, int parts) {
  __shared__ float red[8][256];
  const int cg = threadIdx.x & 31, rl = threadIdx.x >> 5;  // 32 column groups of 8, 8 row lanes
  const int64_t n = (int64_t)blockIdx.x * 256 + cg * 8;
  const int64_t p = blockIdx.y;
  const int64_t rows_per = cdiv64(M, parts);
  const int64_t mbeg = p * rows_per, mend = (mbeg + rows_per < M) ? mbeg + rows_per : M;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (n < N) {
    for (int64_t m = mbeg + rl; m < mend; m += 8) {
      const int64_t j = m % group;
      if (j < row_lo || j >= row_hi) continue;
      const u32x4_t v = *(const u32x4_t*)(in + m * ld + n);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        acc[2 * i] += bf_lo(v[i]);
        acc[2 * i + 1] += bf_hi(v[i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 8; i++) red[rl][cg * 8 + i] = acc[i];
  __syncthreads();
  const int c = threadIdx.x;
  const int64_t nn = (int64_t)blockIdx.x * 256 + c;
  if (nn < N) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 8; r++) s += red[r][c];
    part[p * N + nn] = s;
  }
}

// out[n] = alpha * sum_p part[p*stride + n] + (beta != 0 ? beta * out[n] : 0)
// one workgroup per 64 columns, 8 partial-lanes of 64 threads each (coalesced 256-B row reads, 8 in flight),
// then a fixed-order LDS combine -> deterministic.  The N columns may be split into up to three segments of `seg`
// columns with their own outputs (several reductions over one partial matrix in ONE launch: LayerNorm's
// dgamma | dbeta | column sum of dx); seg must be a multiple of 64.
struct ReduceOuts {
  float* o[3];
};
// The per-column reduction both kernels below run on column n of part[P][stride] (a workgroup owns 64 consecutive columns): 8 partial
// lanes sum rows pl, pl + 8, ... in order, then a fixed-order LDS combine and alpha.  True in the one thread that holds the result t.
__device__ __forceinline__ bool reduce_column(const float* __restrict__ part, int64_t P, int64_t N, int64_t stride, int64_t n,
                                              float alpha, float& t) {
  __shared__ float red[8][64];
  const int c = threadIdx.x & 63, pl = threadIdx.x >> 6;
  float s = 0.f;
  if (n < N) {
#pragma unroll 8
    for (int64_t p = pl; p < P; p += 8) s += part[p * stride + n];
  }
  red[pl][c] = s;
  __syncthreads();
  if (pl != 0 || n >= N) return false;
  t = red[0][c];
#pragma unroll
  for (int i = 1; i < 8; i++) t += red[i][c];
  t *= alpha;
  return true;
}
// *o = t + beta * *o, the old value read only when beta != 0
__device__ __forceinline__ void reduce_store(float* o, float t, float beta) {
  if (beta != 0.f) t += beta * *o;
  *o = t;
}
__global__ __launch_bounds__(512) void reduce_partials_kernel(const float* __restrict__ part, ReduceOuts outs, int64_t seg,
                                                              int64_t P, int64_t N, int64_t stride, float alpha,
                                                              float beta) {
  const int64_t n = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
  float t;
  if (!reduce_column(part, P, N, stride, n, alpha, t)) return;
  const int64_t sg = n / seg;                       // workgroup-uniform (seg % 64 == 0)
  reduce_store((sg == 0 ? outs.o[0] : (sg == 1 ? outs.o[1] : outs.o[2])) + (n - sg * seg), t, beta);
}

int vj_reduce_partials_strided(const float* part, float* out, int64_t P, int64_t N, int64_t stride, float alpha,
                               float beta, hipStream_t stream) {
  if (N == 0) return 0;
  ReduceOuts outs = {{out, nullptr, nullptr}};
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)cdiv64(N, 64)), dim3(512), 0, stream, part, outs,
                     (int64_t)(cdiv64(N, 64) * 64), P, N, stride, alpha, beta);
  VJ_LAUNCH_CHECK("vj_reduce_partials");
  return 0;
}

// part[p][k*D : (k+1)*D] -> outs[k], k < nseg <= 3, in one launch (D % 64 == 0; otherwise one launch per output)
int vj_reduce_partials_multi(const float* part, float* const* outs, int nseg, int64_t P, int64_t D, float alpha, float beta,
                             hipStream_t stream) {
  if (D == 0 || nseg == 0) return 0;
  if (D % 64 != 0) {
    for (int k = 0; k < nseg; k++) {
      int rc = vj_reduce_partials_strided(part + k * D, outs[k], P, D, (int64_t)nseg * D, alpha, beta, stream);
      if (rc) return rc;
    }
    return 0;
  }
  ReduceOuts ro = {{outs[0], nseg > 1 ? outs[1] : nullptr, nseg > 2 ? outs[2] : nullptr}};
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)cdiv64(nseg * D, 64)), dim3(512), 0, stream, part, ro, D, P,
                     (int64_t)nseg * D, (int64_t)nseg * D, alpha, beta);
  VJ_LAUNCH_CHECK("vj_reduce_partials(multi)");
  return 0;
}

extern "C" int vj_reduce_partials(const float* part, float* out, int64_t P, int64_t N, float alpha, float beta,
                                  hipStream_t stream) {
  return vj_reduce_partials_strided(part, out, P, N, N, alpha, beta, stream);
}

// Several independent partial reductions in ONE launch: segment s computes out_s[n] = alpha * sum_p part_s[p * stride_s + n]
// (+ beta * out_s[n]), n < N_s.  Same per-column arithmetic and summation order as reduce_partials_kernel (8 partial lanes,
// fixed-order combine), so a reduction gives the same bits whether it runs alone or as a segment here.  The backward of a
// transformer block ends with one such launch (LayerNorm dgamma | dbeta | proj / fc2 bias sums of both norms + the qkv and fc1
// bias partials of the producing kernels) instead of six reduction / column-sum launches.
#define VJ_REDUCE_MAX_SEGS 16
struct ReduceSegs {
  const float* part[VJ_REDUCE_MAX_SEGS];
  float* out[VJ_REDUCE_MAX_SEGS];
  int64_t P[VJ_REDUCE_MAX_SEGS], N[VJ_REDUCE_MAX_SEGS], stride[VJ_REDUCE_MAX_SEGS];
  int blk_end[VJ_REDUCE_MAX_SEGS];   // exclusive prefix sums of the segments' workgroup counts (cdiv(N, 64) each)
  int n;
};
__global__ __launch_bounds__(512) void reduce_segments_kernel(ReduceSegs rs, float alpha, float beta) {
  int sg = 0;
  while (sg + 1 < rs.n && (int)blockIdx.x >= rs.blk_end[sg]) sg++;      // workgroup-uniform
  const int blk0 = sg == 0 ? 0 : rs.blk_end[sg - 1];
  const int64_t n = (int64_t)((int)blockIdx.x - blk0) * 64 + (threadIdx.x & 63);
  float t;
  if (reduce_column(rs.part[sg], rs.P[sg], rs.N[sg], rs.stride[sg], n, alpha, t)) reduce_store(rs.out[sg] + n, t, beta);
}

extern "C" int vj_reduce_segments(const vj_reduce_seg_t* segs, int64_t n_segs, float alpha, float beta, hipStream_t stream) {
  VJ_CHECK_ARG(segs != nullptr && n_segs >= 0 && n_segs <= VJ_REDUCE_MAX_SEGS, "vj_reduce_segments: 0..%d segments", VJ_REDUCE_MAX_SEGS);
  ReduceSegs rs;
  int nb = 0, k = 0;
  for (int64_t i = 0; i < n_segs; i++) {
    const vj_reduce_seg_t& sg = segs[i];
    VJ_CHECK_ARG(sg.P >= 0 && sg.N >= 0 && sg.stride >= sg.N, "vj_reduce_segments: segment %ld has bad dims", (long)i);
    if (sg.N == 0) continue;
    VJ_CHECK_ARG(sg.out != nullptr && (sg.part != nullptr || sg.P == 0), "vj_reduce_segments: segment %ld has null pointers", (long)i);
    rs.part[k] = sg.part;
    rs.out[k] = sg.out;
    rs.P[k] = sg.P;
    rs.N[k] = sg.N;
    rs.stride[k] = sg.stride;
    nb += (int)cdiv64(sg.N, 64);
    rs.blk_end[k] = nb;
    k++;
  }
  if (k == 0) return 0;
  rs.n = k;
  hipLaunchKernelGGL(reduce_segments_kernel, dim3((unsigned)nb), dim3(512), 0, stream, rs, alpha, beta);
  VJ_LAUNCH_CHECK("vj_reduce_segments");
  return 0;
}

extern "C" int64_t vj_colsum_ws_bytes(int64_t N) { return (int64_t)VJ_COLSUM_PARTS * N * 4; }

extern "C" int vj_colsum_bf16(const void* in, int64_t M, int64_t N, int64_t ld, int64_t group, int64_t row_lo,
                              int64_t row_hi, float* out, float alpha, float beta, void* ws, int64_t ws_bytes,
                              hipStream_t stream) {
  VJ_CHECK_ARG(N % 8 == 0 && ld % 8 == 0, "vj_colsum_bf16: N and ld must be multiples of 8");
  VJ_CHECK_ARG(ws_bytes >= vj_colsum_ws_bytes(N), "vj_colsum_bf16: workspace too small (%ld < %ld)", (long)ws_bytes,
               (long)vj_colsum_ws_bytes(N));
  if (N == 0) return 0;
  if (group <= 0) group = (M > 0 ? M : 1);
  // row chunks: enough workgroups (>= ~2048, 8 per CU) to keep HBM busy when N is narrow (N = 1024: 4 column groups), halved
  // while a chunk would hold fewer than 64 rows (8 per row lane).  The count starts in 64 .. 256; the halving stops once it is at
  // or below 64, so it ends in 64 .. 256 for N <= 2048 (the start there is 256) and can end below 64 for wider N, where
  // the start is no power of two: N = 3072 and M < 5440 gives 171 -> 85 -> 42, N = 2056 and M < 7296 gives 228 -> 114 -> 57.  Never
  // below 33.  The chunk count only changes the (fixed, deterministic) summation order
  const int64_t gx = cdiv64(N, 256);
  int64_t parts = cdiv64(2048, gx);
  if (parts < 64) parts = 64;
  if (parts > VJ_COLSUM_PARTS) parts = VJ_COLSUM_PARTS;
  while (parts > 64 && M / parts < 64) parts /= 2;
  dim3 grid((unsigned)gx, (unsigned)parts);
  hipLaunchKernelGGL(colsum_bf16_kernel, grid, dim3(256), 0, stream, (const bf16_t*)in, (float*)ws, M, N, ld, group,
                     row_lo, row_hi, (int)parts);
  VJ_LAUNCH_CHECK("vj_colsum_bf16");
  return vj_reduce_partials((const float*)ws, out, parts, N, alpha, beta, stream);
}
