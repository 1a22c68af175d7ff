// Stochastic depth (drop path) at the two residual adds of a transformer block, one wave per token row: the per-sample scaled
// residual add of the forward and the per-sample scaling of the branch's output gradient of the backward.  Both stream their rows
// once in 16-byte chunks; a dropped sample's branch rows are never read.
//
// Reference behaviour restated (never copied): the ViT lineage's drop_path(x, p, training) = x / keep * floor(keep + U[0,1)) per
// sample, applied to a block's attention and MLP branches before their residual adds.  The V-JEPA reference itself builds its blocks
// without it (src/models/utils/modules.py:114-120); the fine-tuning eval is where this package uses it.
#include "common.hpp"
#include "../../include/vjepa_hip.h"

// ---------------------------------------------------------------------------------------------
// drop_path_add: y[r,:] = bf16(fmaf(s[b], y[r,:], x[r,:])) for the S rows r of sample b; s[b] == 0: y[r,:] = x[r,:] verbatim, y unread.
// The fused multiply-add is written out (the file is built with -ffp-contract=fast, which would fuse it anyway): the product is
// never rounded on its own, so the result is the exact x + s*y rounded to fp32 and then to bf16.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void drop_path_add_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
                                                            const float* __restrict__ scale, int64_t rows, int64_t S, int D) {
  const int lane = wave_lane();
  const int64_t wave = wave_row(), nw = wave_row_step();
  for (int64_t r = wave; r < rows; r += nw) {
    const float s = scale[r / S];   // (the same address in every lane: one read per row)
    const bf16_t* xp = x + r * D;
    bf16_t* yp = y + r * D;
    if (s == 0.0f) {
      for (int c = lane * 8; c < D; c += 512) *(u32x4_t*)(yp + c) = *(const u32x4_t*)(xp + c);
    } else {
      for (int c = lane * 8; c < D; c += 512) {
        const u32x4_t xv = *(const u32x4_t*)(xp + c);
        u32x4_t yv = *(const u32x4_t*)(yp + c);
#pragma unroll
        for (int i = 0; i < 4; i++) yv[i] = pack_bf2(fmaf(s, bf_lo(yv[i]), bf_lo(xv[i])), fmaf(s, bf_hi(yv[i]), bf_hi(xv[i])));
        *(u32x4_t*)(yp + c) = yv;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// drop_path_scale: out[r,:] = bf16(s[b] * dx[r,:]) (fp32 product, one rounding to bf16); s[b] == 0: out[r,:] = +0, dx unread.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void drop_path_scale_kernel(const bf16_t* __restrict__ dx, bf16_t* __restrict__ out,
                                                              const float* __restrict__ scale, int64_t rows, int64_t S, int D) {
  const int lane = wave_lane();
  const int64_t wave = wave_row(), nw = wave_row_step();
  for (int64_t r = wave; r < rows; r += nw) {
    const float s = scale[r / S];
    const bf16_t* dp = dx + r * D;
    bf16_t* op = out + r * D;
    if (s == 0.0f) {
      for (int c = lane * 8; c < D; c += 512) *(u32x4_t*)(op + c) = (u32x4_t){0u, 0u, 0u, 0u};
    } else {
      for (int c = lane * 8; c < D; c += 512) {
        u32x4_t v = *(const u32x4_t*)(dp + c);
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = pack_bf2(s * bf_lo(v[i]), s * bf_hi(v[i]));
        *(u32x4_t*)(op + c) = v;
      }
    }
  }
}

// the argument checks of both entry points: everything is refused on the host, before any HIP call
static int drop_path_check(const char* who, const void* a, const void* b, const float* scale, int64_t B, int64_t S, int64_t D,
                           int64_t* rows) {
  VJ_CHECK_ARG(B >= 0 && S >= 0 && D > 0, "%s: bad dims B=%ld S=%ld D=%ld", who, (long)B, (long)S, (long)D);
  VJ_CHECK_ARG(D % 8 == 0 && D <= (int64_t)1 << 30, "%s: D=%ld must be a multiple of 8 (and at most 2^30)", who, (long)D);
  VJ_CHECK_ARG(S == 0 || B <= INT64_MAX / S, "%s: B*S overflows", who);
  *rows = B * S;
  if (*rows == 0) return 0;
  VJ_CHECK_ARG(a != nullptr && b != nullptr && scale != nullptr, "%s: null pointer", who);
  VJ_CHECK_ARG(a != b, "%s: the two row buffers must be distinct", who);
  VJ_CHECK_ARG(((uintptr_t)a | (uintptr_t)b) % 16 == 0 && (uintptr_t)scale % 4 == 0, "%s: row buffers must be 16-byte aligned", who);
  return 0;
}

extern "C" int vj_drop_path_add(const void* x_bf16, void* y_bf16, const float* scale, int64_t B, int64_t S, int64_t D,
                                hipStream_t stream) {
  int64_t rows = 0;
  if (int rc = drop_path_check("vj_drop_path_add", x_bf16, y_bf16, scale, B, S, D, &rows)) return rc;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(drop_path_add_kernel, dim3(rows_grid(rows)), dim3(256), 0, stream, (const bf16_t*)x_bf16, (bf16_t*)y_bf16,
                     scale, rows, S, (int)D);
  VJ_LAUNCH_CHECK("vj_drop_path_add");
  return 0;
}

extern "C" int vj_drop_path_scale(const void* dx_bf16, void* out_bf16, const float* scale, int64_t B, int64_t S, int64_t D,
                                  hipStream_t stream) {
  int64_t rows = 0;
  if (int rc = drop_path_check("vj_drop_path_scale", dx_bf16, out_bf16, scale, B, S, D, &rows)) return rc;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(drop_path_scale_kernel, dim3(rows_grid(rows)), dim3(256), 0, stream, (const bf16_t*)dx_bf16,
                     (bf16_t*)out_bf16, scale, rows, S, (int)D);
  VJ_LAUNCH_CHECK("vj_drop_path_scale");
  return 0;
}
