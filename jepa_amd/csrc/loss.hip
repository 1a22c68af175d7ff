// The latent L_p loss of the V-JEPA step and its variance regulariser, each with its gradient.
//
// Reference behaviour restated (never copied):
//   loss_fn: mean(|z-h|^p)/p averaged over masks         app/vjepa/train.py:440-446
//   reg_fn : sqrt(var_tokens(z)+1e-4)                    app/vjepa/train.py:448-449,458
#include "common.hpp"

// ---------------------------------------------------------------------------------------------
// latent_loss: sum |z-h|^p / p over all elements (z bf16, h fp32), deterministic two-stage reduction,
// optionally writing dz = sign(z-h)*|z-h|^(p-1) * gscale (bf16) in the same pass.
// part[blk] holds the block sums; finish kernel folds them:  out[slot] = scale * sum.
// Non-finite d follows autograd of the reference expression: an infinite d gives +-gscale (p == 1) or +-inf; a NaN d gives 0
// for p == 1 (sgn(NaN) = 0) and NaN otherwise, so that the gradient-norm guard of the optimizer sees it.
// ---------------------------------------------------------------------------------------------
#define LOSS_BLOCKS 512
__global__ __launch_bounds__(256) void latent_loss_kernel(const bf16_t* __restrict__ z, const float* __restrict__ h,
                                                          bf16_t* __restrict__ dz, float* __restrict__ part,
                                                          int64_t n8, float p, float gscale) {
  __shared__ float red[1][4];
  float acc = 0.f;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n8; q += (int64_t)gridDim.x * 256) {
    float zv[8];
    load8(z + q * 8, zv);
    const float4 h0 = *(const float4*)(h + q * 8);
    const float4 h1 = *(const float4*)(h + q * 8 + 4);
    const float hv[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
    float g[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float d = zv[j] - hv[j];
      const float a = fabsf(d);
      if (p == 1.0f) {
        acc += a;
        g[j] = (d > 0.f) ? gscale : ((d < 0.f) ? -gscale : 0.f);
      } else {
        acc += __powf(a, p) / p;
        const float m = (a > 0.f) ? __powf(a, p - 1.0f) : 0.f;
        // a NaN d takes neither comparison and is passed on, as autograd does for p != 1 (p == 1: sgn(NaN) is 0 there too)
        g[j] = (d > 0.f) ? m * gscale : ((d <= 0.f) ? -m * gscale : d);
      }
    }
    if (dz) store8(dz + q * 8, g);
  }
  block4_stage(red, {acc});
  if (threadIdx.x == 0) part[blockIdx.x] = block4_total(red[0]);
}

__global__ void scalar_finish_kernel(const float* __restrict__ part, int n, float scale, float* __restrict__ out,
                                     int accumulate) {
  __shared__ float red[1][4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += part[i];
  block4_stage(red, {s});
  if (threadIdx.x == 0) {
    const float v = block4_total(red[0]) * scale;
    *out = accumulate ? (*out + v) : v;
  }
}

extern "C" int64_t vj_latent_loss_ws_bytes(void) { return LOSS_BLOCKS * 4; }

// loss_out (device scalar) = [accumulate ? loss_out : 0] + out_scale * sum(|z-h|^p / p)
extern "C" int vj_latent_loss(const void* z_bf16, const float* h, void* dz_bf16, int64_t numel, float p,
                              float gscale, float out_scale, int accumulate, float* loss_out, void* ws,
                              int64_t ws_bytes, hipStream_t stream) {
  VJ_CHECK_ARG(numel % 8 == 0, "vj_latent_loss: numel=%ld must be a multiple of 8", (long)numel);
  VJ_CHECK_ARG(ws_bytes >= vj_latent_loss_ws_bytes(), "vj_latent_loss: workspace too small");
  VJ_CHECK_ARG(p > 0.f, "vj_latent_loss: loss_exp must be > 0");
  if (numel == 0) return 0;
  hipLaunchKernelGGL(latent_loss_kernel, dim3(LOSS_BLOCKS), dim3(256), 0, stream, (const bf16_t*)z_bf16, h,
                     (bf16_t*)dz_bf16, (float*)ws, numel / 8, p, gscale);
  VJ_LAUNCH_CHECK("vj_latent_loss");
  hipLaunchKernelGGL(scalar_finish_kernel, dim3(1), dim3(256), 0, stream, (const float*)ws, LOSS_BLOCKS, out_scale,
                     loss_out, accumulate);
  VJ_LAUNCH_CHECK("vj_latent_loss(finish)");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// token_pstd: pstd[b,d] (+)= sqrt(unbiased_var_k z[b,k,d] + 1e-4)   (reg_fn, train.py:448-449)
// one block per (b, 256-column slab); two-pass over the K rows for accuracy.
// ---------------------------------------------------------------------------------------------
// one workgroup per (b, 64-column slab): 4 waves split the K rows, each lane owns one column pair... 8 columns per
// thread (16-byte loads), shifted single-pass sums (shift = first row) combined across the 8 row-lanes in LDS.
__global__ __launch_bounds__(256) void token_pstd_kernel(const bf16_t* __restrict__ z, float* __restrict__ pstd,
                                                         float* __restrict__ stats, int64_t K, int D,
                                                         int accumulate) {
  __shared__ float red[2][32][65];
  const int64_t b = blockIdx.y;
  const int cg = threadIdx.x & 7, rl = threadIdx.x >> 3;       // 8 column groups of 8, 32 row lanes
  const int d0 = blockIdx.x * 64 + cg * 8;
  const bf16_t* zp = z + b * K * D;
  float s[8], q[8], sh[8];
#pragma unroll
  for (int j = 0; j < 8; j++) s[j] = q[j] = sh[j] = 0.f;
  if (d0 < D) {
    load8(zp + d0, sh);                                         // shift by row 0: well-conditioned single pass
    for (int64_t k = rl; k < K; k += 32) {
      float v[8];
      load8(zp + k * D + d0, v);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float t = v[j] - sh[j];
        s[j] += t;
        q[j] += t * t;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; j++) {
    red[0][rl][cg * 8 + j] = s[j];
    red[1][rl][cg * 8 + j] = q[j];
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int c = threadIdx.x, d = blockIdx.x * 64 + c;
    if (d < D) {
      float ss = 0.f, qq = 0.f;
      for (int r = 0; r < 32; r++) {
        ss += red[0][r][c];
        qq += red[1][r][c];
      }
      const float var = (qq - ss * ss / (float)K) / (float)(K - 1);   // unbiased, shift-invariant
      const float v = sqrtf(fmaxf(var, 0.f) + 1e-4f);
      float* o = pstd + b * D + d;
      *o = accumulate ? (*o + v) : v;
      if (stats) {   // per-(b,d) token mean and sqrt(var + eps) of THIS mask, for reg_grad
        stats[(b * D + d) * 2] = bf2f(zp[d]) + ss / (float)K;
        stats[(b * D + d) * 2 + 1] = v;
      }
    }
  }
}

// reg = mean(relu(1 - pstd_sum / n_masks))
__global__ __launch_bounds__(256) void reg_finish_kernel(const float* __restrict__ pstd, int64_t n, float inv_masks,
                                                         float* __restrict__ out) {
  __shared__ float red[1][4];
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += 256) s += fmaxf(0.f, 1.0f - pstd[i] * inv_masks);
  block4_stage(red, {s});
  if (threadIdx.x == 0) *out = block4_total(red[0]) / (float)n;
}

extern "C" int vj_token_pstd(const void* z_bf16, float* pstd, float* stats, int64_t B, int64_t K, int64_t D,
                             int accumulate, hipStream_t stream) {
  VJ_CHECK_ARG(K >= 2, "vj_token_pstd: need at least 2 tokens for an unbiased variance (K=%ld)", (long)K);
  if (B * D == 0) return 0;
  VJ_CHECK_ARG(D % 8 == 0, "vj_token_pstd: D must be a multiple of 8");
  hipLaunchKernelGGL(token_pstd_kernel, dim3((unsigned)cdiv64(D, 64), (unsigned)B), dim3(256), 0, stream,
                     (const bf16_t*)z_bf16, pstd, stats, K, (int)D, accumulate);
  VJ_LAUNCH_CHECK("vj_token_pstd");
  return 0;
}

extern "C" int vj_reg_finish(const float* pstd_sum, int64_t n, int64_t n_masks, float* out, hipStream_t stream) {
  hipLaunchKernelGGL(reg_finish_kernel, dim3(1), dim3(256), 0, stream, pstd_sum, n, 1.0f / (float)n_masks, out);
  VJ_LAUNCH_CHECK("vj_reg_finish");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// reg_grad: dz[b,k,d] += coef * d/dz mean_{b,d} relu(1 - pstd_avg[b,d]),  pstd_avg = pstd_sum / n_masks
//   = -coef / (B*D*n_masks) * 1[pstd_avg < 1] * (z - mean) / ((K-1) * sqrt(var + eps))       (train.py:448-459)
// dz holds the latent-loss gradient in units of 1/gscale (see vj_latent_loss); `coef` is pre-divided accordingly.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void reg_grad_kernel(const bf16_t* __restrict__ z, const float* __restrict__ pstd_sum,
                                                       const float* __restrict__ stats, bf16_t* __restrict__ dz,
                                                       int64_t B, int64_t K, int D, float inv_masks, float coef) {
  const int64_t n8 = B * K * D / 8;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n8; q += (int64_t)gridDim.x * 256) {
    const int64_t e = q * 8;
    const int d0 = (int)(e % D);
    const int64_t b = e / ((int64_t)K * D);
    float zv[8], gv[8];
    load8(z + e, zv);
    load8(dz + e, gv);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int64_t bd = b * D + d0 + j;
      const float active = (pstd_sum[bd] * inv_masks < 1.0f) ? 1.0f : 0.f;
      gv[j] -= coef * active * (zv[j] - stats[bd * 2]) / ((float)(K - 1) * stats[bd * 2 + 1]);
    }
    store8(dz + e, gv);
  }
}

extern "C" int vj_reg_grad(const void* z_bf16, const float* pstd_sum, const float* stats, void* dz_bf16, int64_t B,
                           int64_t K, int64_t D, int64_t n_masks, float coef, hipStream_t stream) {
  VJ_CHECK_ARG(D % 8 == 0 && K >= 2, "vj_reg_grad: need D %% 8 == 0 and K >= 2");
  if (B * K * D == 0) return 0;
  hipLaunchKernelGGL(reg_grad_kernel, dim3(flat_grid(B * K * D / 8, 256 * 8)), dim3(256), 0, stream, (const bf16_t*)z_bf16, pstd_sum, stats,
                     (bf16_t*)dz_bf16, B, K, (int)D, 1.0f / (float)n_masks, coef);
  VJ_LAUNCH_CHECK("vj_reg_grad");
  return 0;
}
