// Soft-max DOWN THE KEY AXIS for a bank of attentive probes that share one frozen forward pass
// (src/models/attentive_pooler.py AttentiveClassifierBank; include/vjepa_hip.h "bank of attentive probes").
//
// With one query token shared by the batch, the scores of every (probe, head) are one column of S = x_hat U^T, fp32 [B, N, C]
// with C = probes * heads (padded): the soft-max of CrossAttention.forward (modules.py:150-153) runs over the N keys of each
// (sample, column).  A thread owns 4 adjacent columns (one float4 per key row, so a wave reads 256 contiguous bytes of a row) and
// the keys are split into POOL_CHUNK-key chunks:
//   stage 1  per (sample, chunk, 64 columns): running maximum m and sum l of exp(s - m) of the chunk -> ws
//   stage 2  per (sample, column): the chunks merged in ASCENDING chunk order -> lse = M + log L
//   stage 3  A = bf16(exp(s - lse))
// No atomics anywhere: the order of every sum is fixed by the shape, so two runs give the same bits.
#include "common.hpp"

#define POOL_CHUNK 256     // keys per stage-1 workgroup
#define POOL_COLS 64       // columns per workgroup: 16 threads x 4
#define POOL_ROWS 16       // key rows a workgroup reads at once: 256 threads / 16

__global__ __launch_bounds__(256) void pool_softmax_partial_kernel(const float* __restrict__ S, float* __restrict__ ws_m,
                                                                   float* __restrict__ ws_l, int64_t N, int64_t C) {
  __shared__ float sm[POOL_ROWS][POOL_COLS], sl[POOL_ROWS][POOL_COLS];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int64_t c0 = (int64_t)blockIdx.x * POOL_COLS + tx * 4;
  const int64_t chunk = blockIdx.y, b = blockIdx.z, n0 = chunk * POOL_CHUNK;
  const bool col_ok = c0 < C;   // C % 4 == 0: the four columns of a thread are inside together
  float4 v[POOL_CHUNK / POOL_ROWS];
  float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, l[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < POOL_CHUNK / POOL_ROWS; i++) {
    const int64_t n = n0 + ty + i * POOL_ROWS;
    if (col_ok && n < N) {
      v[i] = *(const float4*)(S + (b * N + n) * C + c0);
      m[0] = fmaxf(m[0], v[i].x); m[1] = fmaxf(m[1], v[i].y); m[2] = fmaxf(m[2], v[i].z); m[3] = fmaxf(m[3], v[i].w);
    }
  }
#pragma unroll
  for (int i = 0; i < POOL_CHUNK / POOL_ROWS; i++) {
    const int64_t n = n0 + ty + i * POOL_ROWS;
    if (col_ok && n < N) {   // m is finite here: this thread has read at least row n
      l[0] += expf(v[i].x - m[0]); l[1] += expf(v[i].y - m[1]); l[2] += expf(v[i].z - m[2]); l[3] += expf(v[i].w - m[3]);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {
    sm[ty][tx * 4 + j] = m[j];
    sl[ty][tx * 4 + j] = l[j];
  }
  __syncthreads();
  if (threadIdx.x < POOL_COLS) {
    const int64_t c = (int64_t)blockIdx.x * POOL_COLS + threadIdx.x;
    if (c < C) {
      float M = sm[0][threadIdx.x];   // row n0 exists (n0 < N by the grid): finite
#pragma unroll
      for (int r = 1; r < POOL_ROWS; r++) M = fmaxf(M, sm[r][threadIdx.x]);
      float L = 0.f;
#pragma unroll
      for (int r = 0; r < POOL_ROWS; r++) {   // a key row past N left (m, l) = (-inf, 0): contributes exactly 0
        const float lr = sl[r][threadIdx.x];
        if (lr > 0.f) L += lr * expf(sm[r][threadIdx.x] - M);
      }
      const int64_t o = (b * gridDim.y + chunk) * C + c;
      ws_m[o] = M;
      ws_l[o] = L;
    }
  }
}

__global__ __launch_bounds__(256) void pool_softmax_merge_kernel(const float* __restrict__ ws_m, const float* __restrict__ ws_l,
                                                                 float* __restrict__ lse, int64_t B, int64_t C, int64_t n_chunks) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B * C) return;
  const int64_t b = i / C, c = i % C;
  const float* pm = ws_m + b * n_chunks * C + c;
  const float* pl = ws_l + b * n_chunks * C + c;
  float M = pm[0];
  for (int64_t k = 1; k < n_chunks; k++) M = fmaxf(M, pm[k * C]);
  float L = 0.f;
  for (int64_t k = 0; k < n_chunks; k++) L += pl[k * C] * expf(pm[k * C] - M);   // ascending chunk order
  lse[i] = M + logf(L);   // L >= 1: the chunk that holds the maximum contributes exp(0)
}

__global__ __launch_bounds__(256) void pool_softmax_write_kernel(const float* __restrict__ S, const float* __restrict__ lse,
                                                                 bf16_t* __restrict__ A, int64_t N, int64_t C) {
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int64_t c0 = (int64_t)blockIdx.x * POOL_COLS + tx * 4;
  const int64_t b = blockIdx.z, n0 = (int64_t)blockIdx.y * POOL_CHUNK;
  if (c0 >= C) return;
  const float4 e = *(const float4*)(lse + b * C + c0);
#pragma unroll 4
  for (int i = 0; i < POOL_CHUNK / POOL_ROWS; i++) {
    const int64_t n = n0 + ty + i * POOL_ROWS;
    if (n < N) {
      const int64_t o = (b * N + n) * C + c0;
      const float4 s = *(const float4*)(S + o);
      *(u32x2_t*)(A + o) = pack4_bf16(expf(s.x - e.x), expf(s.y - e.y), expf(s.z - e.z), expf(s.w - e.w));
    }
  }
}

// dS = A (dA - delta): the soft-max backward down the key axis, delta[b, c] = sum_n A dA given by the caller
__global__ __launch_bounds__(256) void pool_softmax_bwd_kernel(const bf16_t* __restrict__ A, const float* __restrict__ dA,
                                                               const float* __restrict__ delta, bf16_t* __restrict__ dS, int64_t N,
                                                               int64_t C) {
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int64_t c0 = (int64_t)blockIdx.x * POOL_COLS + tx * 4;
  const int64_t b = blockIdx.z, n0 = (int64_t)blockIdx.y * POOL_CHUNK;
  if (c0 >= C) return;
  const float4 d = *(const float4*)(delta + b * C + c0);
#pragma unroll 4
  for (int i = 0; i < POOL_CHUNK / POOL_ROWS; i++) {
    const int64_t n = n0 + ty + i * POOL_ROWS;
    if (n < N) {
      const int64_t o = (b * N + n) * C + c0;
      const u32x2_t a = *(const u32x2_t*)(A + o);
      const float4 g = *(const float4*)(dA + o);
      *(u32x2_t*)(dS + o) = pack4_bf16(bf2f((bf16_t)(a[0] & 0xffffu)) * (g.x - d.x), bf2f((bf16_t)(a[0] >> 16)) * (g.y - d.y),
                                       bf2f((bf16_t)(a[1] & 0xffffu)) * (g.z - d.z), bf2f((bf16_t)(a[1] >> 16)) * (g.w - d.w));
    }
  }
}

static inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// shared by the three entry points: the grid's y / z extents are chunk and sample counts
static int pool_check_dims(const char* who, int64_t B, int64_t N, int64_t C) {
  VJ_CHECK_ARG(B > 0 && N > 0 && C > 0, "%s: B, N and C must be positive (got %lld, %lld, %lld)", who, (long long)B, (long long)N,
               (long long)C);
  VJ_CHECK_ARG(C % 4 == 0, "%s: C = %lld must be a multiple of 4 (pad the columns with zero rows of U)", who, (long long)C);
  VJ_CHECK_ARG(B <= 65535 && cdiv64(N, POOL_CHUNK) <= 65535 && C <= (1 << 24),
               "%s: B <= 65535, N <= 65535 * %d and C <= 2^24 (got %lld, %lld, %lld)", who, POOL_CHUNK, (long long)B, (long long)N,
               (long long)C);
  return 0;
}

extern "C" int64_t vj_pool_softmax_chunk_keys(void) { return POOL_CHUNK; }

extern "C" int64_t vj_pool_softmax_fwd_ws_bytes(int64_t B, int64_t N, int64_t C) {
  if (pool_check_dims("vj_pool_softmax_fwd_ws_bytes", B, N, C) != 0) return -1;
  return 2 * B * cdiv64(N, POOL_CHUNK) * C * (int64_t)sizeof(float);
}

extern "C" int vj_pool_softmax_fwd(const float* S, void* A_bf16, float* lse, int64_t B, int64_t N, int64_t C, void* ws,
                                   int64_t ws_bytes, hipStream_t stream) {
  if (pool_check_dims("vj_pool_softmax_fwd", B, N, C) != 0) return -1;
  VJ_CHECK_ARG(S != nullptr && A_bf16 != nullptr && lse != nullptr && ws != nullptr, "vj_pool_softmax_fwd: null S, A, lse or ws");
  VJ_CHECK_ARG(aligned_to(S, 16) && aligned_to(lse, 16) && aligned_to(ws, 16) && aligned_to(A_bf16, 8),
               "vj_pool_softmax_fwd: S, lse and ws must be 16-byte aligned, A 8-byte aligned");
  const int64_t n_chunks = cdiv64(N, POOL_CHUNK), need = 2 * B * n_chunks * C * (int64_t)sizeof(float);
  VJ_CHECK_ARG(ws_bytes >= need, "vj_pool_softmax_fwd: workspace of %lld bytes, %lld needed (vj_pool_softmax_fwd_ws_bytes)",
               (long long)ws_bytes, (long long)need);
  float* ws_m = (float*)ws;
  float* ws_l = ws_m + B * n_chunks * C;
  const dim3 grid((unsigned)cdiv64(C, POOL_COLS), (unsigned)n_chunks, (unsigned)B);
  hipLaunchKernelGGL(pool_softmax_partial_kernel, grid, dim3(256), 0, stream, S, ws_m, ws_l, N, C);
  VJ_LAUNCH_CHECK("vj_pool_softmax_fwd (partials)");
  hipLaunchKernelGGL(pool_softmax_merge_kernel, dim3((unsigned)cdiv64(B * C, 256)), dim3(256), 0, stream, ws_m, ws_l, lse, B, C,
                     n_chunks);
  VJ_LAUNCH_CHECK("vj_pool_softmax_fwd (merge)");
  hipLaunchKernelGGL(pool_softmax_write_kernel, grid, dim3(256), 0, stream, S, lse, (bf16_t*)A_bf16, N, C);
  VJ_LAUNCH_CHECK("vj_pool_softmax_fwd (write)");
  return 0;
}

extern "C" int vj_pool_softmax_bwd(const void* A_bf16, const float* dA, const float* delta, void* dS_bf16, int64_t B, int64_t N,
                                   int64_t C, hipStream_t stream) {
  if (pool_check_dims("vj_pool_softmax_bwd", B, N, C) != 0) return -1;
  VJ_CHECK_ARG(A_bf16 != nullptr && dA != nullptr && delta != nullptr && dS_bf16 != nullptr,
               "vj_pool_softmax_bwd: null A, dA, delta or dS");
  VJ_CHECK_ARG(aligned_to(dA, 16) && aligned_to(delta, 16) && aligned_to(A_bf16, 8) && aligned_to(dS_bf16, 8),
               "vj_pool_softmax_bwd: dA and delta must be 16-byte aligned, A and dS 8-byte aligned");
  const dim3 grid((unsigned)cdiv64(C, POOL_COLS), (unsigned)cdiv64(N, POOL_CHUNK), (unsigned)B);
  hipLaunchKernelGGL(pool_softmax_bwd_kernel, grid, dim3(256), 0, stream, (const bf16_t*)A_bf16, dA, delta, (bf16_t*)dS_bf16, N, C);
  VJ_LAUNCH_CHECK("vj_pool_softmax_bwd");
  return 0;
}
