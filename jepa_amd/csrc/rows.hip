// Row-granular HBM-bound kernels of the V-JEPA step: bit-exact mask gather/scatter of token rows,
// tubelet packing of fp32 clips into bf16 patch rows, positional-embedding add, predictor token
// assembly, bf16 transposes (wgrad operands) and column sums (bias grads).
//
// Reference behaviour restated (never copied):
//   apply_masks                      src/masks/utils.py:11-23      (gather of kept token rows)
//   PatchEmbed3D token/K ordering    src/models/utils/patch_embed.py:31-57
//   x += pos_embed                   src/models/vision_transformer.py:172-174
//   predictor token assembly         src/models/predictor.py:194-221
#include "common.hpp"
#include "internal.hpp"
#include "../../include/vjepa_hip.h"

// ---------------------------------------------------------------------------------------------
// gather_rows: dst[b,k,:] = src[b*src_bstride + idx[b,k], :]   (payload moved verbatim -> bit exact)
// one wave per row, 16 B per lane per trip (row_bytes % 16 == 0) or 4 B per lane (row_bytes % 4 == 0)
// ---------------------------------------------------------------------------------------------
template <typename VEC>
__global__ __launch_bounds__(256) void gather_rows_kernel(const char* __restrict__ src, char* __restrict__ dst,
                                                          const int64_t* __restrict__ idx, int64_t rows, int64_t K,
                                                          int64_t row_bytes, int64_t src_bstride_rows) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  const int64_t nvec = row_bytes / (int64_t)sizeof(VEC);
  for (int64_t r = wave; r < rows; r += nw) {
    const int64_t b = r / K;
    const int64_t s = b * src_bstride_rows + idx[r];
    const VEC* sp = (const VEC*)(src + s * row_bytes);
    VEC* dp = (VEC*)(dst + r * row_bytes);
    for (int64_t v = lane; v < nvec; v += 64) dp[v] = sp[v];
  }
}

// scatter_rows: dst[b, idx[b,k], :] = src[b,k,:]  (dst pre-zeroed; indices unique per b as produced by
// the collator, multiblock3d.py:185-186) -- backward of gather_rows.
template <typename VEC>
__global__ __launch_bounds__(256) void scatter_rows_kernel(const char* __restrict__ src, char* __restrict__ dst,
                                                           const int64_t* __restrict__ idx, int64_t rows, int64_t K,
                                                           int64_t row_bytes, int64_t N) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  const int64_t nvec = row_bytes / (int64_t)sizeof(VEC);
  for (int64_t r = wave; r < rows; r += nw) {
    const int64_t b = r / K;
    const int64_t d = b * N + idx[r];
    const VEC* sp = (const VEC*)(src + r * row_bytes);
    VEC* dp = (VEC*)(dst + d * row_bytes);
    for (int64_t v = lane; v < nvec; v += 64) dp[v] = sp[v];
  }
}

static inline int rows_grid(int64_t rows) {
  int64_t g = cdiv64(rows, 4);
  if (g > 256 * 16) g = 256 * 16;
  if (g < 1) g = 1;
  return (int)g;
}

extern "C" int vj_gather_rows(const void* src, void* dst, const int64_t* idx, int64_t B, int64_t K, int64_t row_bytes,
                              int64_t src_batch_stride_rows, hipStream_t stream) {
  VJ_CHECK_ARG(B >= 0 && K >= 0 && row_bytes > 0, "vj_gather_rows: bad dims B=%ld K=%ld row_bytes=%ld", (long)B,
               (long)K, (long)row_bytes);
  VJ_CHECK_ARG(row_bytes % 4 == 0, "vj_gather_rows: row_bytes=%ld must be a multiple of 4", (long)row_bytes);
  const int64_t rows = B * K;
  if (rows == 0) return 0;
  const bool v16 = (row_bytes % 16 == 0) && (((uintptr_t)src | (uintptr_t)dst) % 16 == 0);
  if (v16)
    hipLaunchKernelGGL(gather_rows_kernel<u32x4_t>, dim3(rows_grid(rows)), dim3(256), 0, stream, (const char*)src,
                       (char*)dst, idx, rows, K, row_bytes, src_batch_stride_rows);
  else
    hipLaunchKernelGGL(gather_rows_kernel<uint32_t>, dim3(rows_grid(rows)), dim3(256), 0, stream, (const char*)src,
                       (char*)dst, idx, rows, K, row_bytes, src_batch_stride_rows);
  VJ_LAUNCH_CHECK("vj_gather_rows");
  return 0;
}

extern "C" int vj_scatter_rows(const void* src, void* dst, const int64_t* idx, int64_t B, int64_t N, int64_t K,
                               int64_t row_bytes, hipStream_t stream) {
  VJ_CHECK_ARG(B >= 0 && K >= 0 && N >= 0 && row_bytes > 0, "vj_scatter_rows: bad dims");
  VJ_CHECK_ARG(row_bytes % 4 == 0, "vj_scatter_rows: row_bytes=%ld must be a multiple of 4", (long)row_bytes);
  if (B * N == 0) return 0;
  hipError_t e = hipMemsetAsync(dst, 0, (size_t)(B * N * row_bytes), stream);
  if (e != hipSuccess) {
    vj_set_error("vj_scatter_rows: memset failed: %s", hipGetErrorString(e));
    return (int)e;
  }
  const int64_t rows = B * K;
  if (rows == 0) return 0;
  const bool v16 = (row_bytes % 16 == 0) && (((uintptr_t)src | (uintptr_t)dst) % 16 == 0);
  if (v16)
    hipLaunchKernelGGL(scatter_rows_kernel<u32x4_t>, dim3(rows_grid(rows)), dim3(256), 0, stream, (const char*)src,
                       (char*)dst, idx, rows, K, row_bytes, N);
  else
    hipLaunchKernelGGL(scatter_rows_kernel<uint32_t>, dim3(rows_grid(rows)), dim3(256), 0, stream, (const char*)src,
                       (char*)dst, idx, rows, K, row_bytes, N);
  VJ_LAUNCH_CHECK("vj_scatter_rows");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// tubelet_pack: fp32 clips [B,C,T,H,W] -> bf16 patch rows [B,K,C*tub*p*p]; row k of clip b is token
// n = idx ? idx[b,k] : k, n -> (t',h',w') row-major (flatten(2).transpose(1,2), patch_embed.py:56),
// element order (c,dt,dh,dw) = Conv3d weight order [D,C,tub,p,p].  8 pixels per thread.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tubelet_pack_kernel(const float* __restrict__ clips, bf16_t* __restrict__ out,
                                                           const int64_t* __restrict__ idx, int64_t B, int C, int T,
                                                           int H, int W, int tub, int p, int64_t K) {
  const int gh = H / p, gw = W / p;
  const int kdim = C * tub * p * p;
  const int cpr = kdim / 8;  // 16-byte output chunks per row
  const int64_t total = B * K * cpr;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
    const int64_t row = q / cpr;
    const int e = (int)(q - row * cpr) * 8;
    const int64_t b = row / K;
    const int64_t n = idx ? idx[row] : (row - b * K);
    const int wq = (int)(n % gw), hq = (int)((n / gw) % gh), tq = (int)(n / ((int64_t)gw * gh));
    const int dw = e % p, dh = (e / p) % p, dt = (e / (p * p)) % tub, c = e / (p * p * tub);
    const float* s = clips + ((((b * C + c) * T + (tq * tub + dt)) * H + (hq * p + dh)) * (int64_t)W + wq * p + dw);
    const float4 lo = *(const float4*)s;
    const float4 hi = *(const float4*)(s + 4);
    u32x4_t o;
    o[0] = pack_bf2(lo.x, lo.y);
    o[1] = pack_bf2(lo.z, lo.w);
    o[2] = pack_bf2(hi.x, hi.y);
    o[3] = pack_bf2(hi.z, hi.w);
    *(u32x4_t*)(out + row * kdim + e) = o;
  }
}

extern "C" int vj_tubelet_pack(const float* clips, void* out_bf16, const int64_t* idx, int64_t B, int64_t C,
                               int64_t T, int64_t H, int64_t W, int64_t tubelet, int64_t patch, int64_t K,
                               hipStream_t stream) {
  VJ_CHECK_ARG(patch % 8 == 0 && W % 4 == 0, "vj_tubelet_pack: patch (%ld) must be a multiple of 8 and W%%4==0",
               (long)patch);
  VJ_CHECK_ARG(T % tubelet == 0 && H % patch == 0 && W % patch == 0, "vj_tubelet_pack: clip not divisible into tubelets");
  if (B * K == 0) return 0;
  const int64_t total = B * K * (C * tubelet * patch * patch / 8);
  int64_t g = cdiv64(total, 256);
  if (g > 256 * 32) g = 256 * 32;
  hipLaunchKernelGGL(tubelet_pack_kernel, dim3((int)g), dim3(256), 0, stream, clips, (bf16_t*)out_bf16, idx, B,
                     (int)C, (int)T, (int)H, (int)W, (int)tubelet, (int)patch, K);
  VJ_LAUNCH_CHECK("vj_tubelet_pack");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// clip_transform: decoded uint8 frames -> model-ready fp32 clips [B,3,T,S,S]: per-frame crop box (i,j,h,w), bilinear resize
// of the crop to S x S (F.interpolate(mode='bilinear', align_corners=False)), horizontal flip of the whole clip, then
// (x - mean) / std with mean / std in 0..255 units.  Source clip b is [T,Hs,Ws,3] (interleaved RGB) at byte `off` of one flat
// buffer; desc[b] = {off, Hs, Ws, flip}.  Per axis: scale = (float)h / S, c = max(fma(scale, dst + 0.5, -0.5), 0) -- the FUSED
// form is the one that reproduces the CPU reference (a separately rounded product moves a coordinate near 1000 by one ulp,
// 1.3e-4 after a 255-step) --, i0 = min((int)c, h - 1), i1 = min(i0 + 1, h - 1), weights 1 - l and l with l = c - i0; rows are
// blended last: wy0 * (wx0 * p00 + wx1 * p01) + wy1 * (wx0 * p10 + wx1 * p11).  A flipped clip takes output column x from
// S - 1 - x.  One thread per 4 consecutive output pixels of one (b,t,y): three 16-byte stores, one per channel plane; source
// bytes come through the cache (neighbouring outputs share them).  Every source row / column is clamped into the frame and a
// clip whose extent does not lie inside the buffer is written as zeros, whatever the descriptor says: nothing outside
// [frames, frames + frames_bytes) is ever read.
// ---------------------------------------------------------------------------------------------
struct ClipAxis {
  int i0, i1;
  float w0, w1;
};

__device__ __forceinline__ ClipAxis clip_axis(int dst, float scale, int org, int len, int lim) {
  const float c = fmaxf(fmaf(scale, (float)dst + 0.5f, -0.5f), 0.f);
  int i0 = (int)c;
  if (i0 > len - 1) i0 = len - 1;
  const int i1 = i0 + 1 < len ? i0 + 1 : len - 1;
  const float l = fminf(fmaxf(c - (float)i0, 0.f), 1.f);
  ClipAxis a;
  a.i0 = min(max(org + i0, 0), lim - 1);
  a.i1 = min(max(org + i1, 0), lim - 1);
  a.w0 = 1.f - l;
  a.w1 = l;
  return a;
}

struct ClipNorm {
  float mean[3], std[3];
};

__global__ __launch_bounds__(256) void clip_transform_kernel(const uint8_t* __restrict__ frames, int64_t frames_bytes,
                                                             const int64_t* __restrict__ desc,
                                                             const int4* __restrict__ boxes, float* __restrict__ out,
                                                             int64_t B, int T, int S, ClipNorm nm) {
  const uint32_t qpr = (uint32_t)S / 4;  // 16-byte output chunks per row
  const uint32_t total = (uint32_t)B * T * S * qpr;   // < 2^31 (checked by the launcher): 32-bit index arithmetic
  const int64_t plane = (int64_t)T * S * S;
  for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < total; q += gridDim.x * 256u) {
    const uint32_t r = q / qpr;   // (b,t,y)
    const int xq = (int)(q - r * qpr) * 4;
    const uint32_t bt = r / (uint32_t)S;
    const int y = (int)(r - bt * (uint32_t)S);
    const int64_t b = bt / (uint32_t)T;
    const int t = (int)(bt - (uint32_t)b * (uint32_t)T);
    const int64_t off = desc[b * 4 + 0], Hs = desc[b * 4 + 1], Ws = desc[b * 4 + 2];
    const bool flip = desc[b * 4 + 3] != 0;
    const int4 box = boxes[bt];  // (i, j, h, w)
    float* o = out + ((b * 3 * T + t) * S + y) * (int64_t)S + xq;
    float4 res[3];
    const bool ok = off >= 0 && Hs > 0 && Ws > 0 && Hs < (1 << 20) && Ws < (1 << 20) && box.z > 0 && box.w > 0 &&
                    off <= frames_bytes && (int64_t)T * Hs * Ws * 3 <= frames_bytes - off;
    if (ok) {
      const uint8_t* f = frames + off + (int64_t)t * Hs * Ws * 3;
      const ClipAxis ay = clip_axis(y, (float)box.z / (float)S, box.x, box.z, (int)Hs);
      const uint8_t* r0 = f + (int64_t)ay.i0 * Ws * 3;
      const uint8_t* r1 = f + (int64_t)ay.i1 * Ws * 3;
      const float sx = (float)box.w / (float)S;
      float v[3][4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int x = flip ? S - 1 - (xq + k) : xq + k;
        const ClipAxis ax = clip_axis(x, sx, box.y, box.w, (int)Ws);
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const float p00 = (float)r0[ax.i0 * 3 + c], p01 = (float)r0[ax.i1 * 3 + c];
          const float p10 = (float)r1[ax.i0 * 3 + c], p11 = (float)r1[ax.i1 * 3 + c];
          const float top = ax.w0 * p00 + ax.w1 * p01, bot = ax.w0 * p10 + ax.w1 * p11;
          v[c][k] = (ay.w0 * top + ay.w1 * bot - nm.mean[c]) / nm.std[c];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; c++) res[c] = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
    } else {
#pragma unroll
      for (int c = 0; c < 3; c++) res[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) *(float4*)(o + c * plane) = res[c];
  }
}

extern "C" int vj_clip_transform(const uint8_t* frames, int64_t frames_bytes, const int64_t* desc, const int32_t* boxes,
                                 float* out, int64_t B, int64_t T, int64_t S, float mean_r, float mean_g, float mean_b,
                                 float std_r, float std_g, float std_b, hipStream_t stream) {
  VJ_CHECK_ARG(B >= 0 && T > 0 && S > 0 && frames_bytes >= 0 && T < (1 << 20) && S < (1 << 20),
               "vj_clip_transform: bad dims B=%ld T=%ld S=%ld frames_bytes=%ld", (long)B, (long)T, (long)S, (long)frames_bytes);
  VJ_CHECK_ARG(S % 4 == 0, "vj_clip_transform: S=%ld must be a multiple of 4", (long)S);
  VJ_CHECK_ARG(std_r != 0.f && std_g != 0.f && std_b != 0.f, "vj_clip_transform: std must be non-zero");
  if (B == 0) return 0;
  VJ_CHECK_ARG(frames != nullptr && desc != nullptr && boxes != nullptr && out != nullptr, "vj_clip_transform: null pointer");
  VJ_CHECK_ARG(((uintptr_t)out % 16 == 0) && ((uintptr_t)boxes % 16 == 0), "vj_clip_transform: out and boxes must be 16-byte aligned");
  const int64_t total = B * T * S * (S / 4);
  VJ_CHECK_ARG(B < (1ll << 31) && total < (1ll << 31), "vj_clip_transform: batch too large (B=%ld)", (long)B);
  int64_t g = cdiv64(total, 256);
  if (g > 256 * 32) g = 256 * 32;
  ClipNorm nm = {{mean_r, mean_g, mean_b}, {std_r, std_g, std_b}};
  hipLaunchKernelGGL(clip_transform_kernel, dim3((int)g), dim3(256), 0, stream, frames, frames_bytes, desc, (const int4*)boxes,
                     out, B, (int)T, (int)S, nm);
  VJ_LAUNCH_CHECK("vj_clip_transform");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// add_pos: x[b,k,:] (bf16) += pos[idx ? idx[b,k] : k, :] (fp32), fp32 add, one rounding.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void add_pos_kernel(bf16_t* __restrict__ x, const float* __restrict__ pos,
                                                      const int64_t* __restrict__ idx, int64_t rows, int64_t K,
                                                      int D) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t r = wave; r < rows; r += nw) {
    const int64_t n = idx ? idx[r] : (r % K);
    bf16_t* xp = x + r * D;
    const float* pp = pos + n * D;
    for (int c = lane * 8; c < D; c += 512) {
      u32x4_t v = *(u32x4_t*)(xp + c);
      const float4 p0 = *(const float4*)(pp + c);
      const float4 p1 = *(const float4*)(pp + c + 4);
      v[0] = pack_bf2(bf_lo(v[0]) + p0.x, bf_hi(v[0]) + p0.y);
      v[1] = pack_bf2(bf_lo(v[1]) + p0.z, bf_hi(v[1]) + p0.w);
      v[2] = pack_bf2(bf_lo(v[2]) + p1.x, bf_hi(v[2]) + p1.y);
      v[3] = pack_bf2(bf_lo(v[3]) + p1.z, bf_hi(v[3]) + p1.w);
      *(u32x4_t*)(xp + c) = v;
    }
  }
}

extern "C" int vj_add_pos(void* x_bf16, const float* pos, const int64_t* idx, int64_t B, int64_t K, int64_t D,
                          hipStream_t stream) {
  VJ_CHECK_ARG(D % 8 == 0, "vj_add_pos: D=%ld must be a multiple of 8", (long)D);
  const int64_t rows = B * K;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(add_pos_kernel, dim3(rows_grid(rows)), dim3(256), 0, stream, (bf16_t*)x_bf16, pos, idx, rows, K,
                     (int)D);
  VJ_LAUNCH_CHECK("vj_add_pos");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// image_pack: fp32 still images [B,C,H,W] -> bf16 patch rows [B,K,C*tub*p*p] of the clip that repeats the image along
// time (input.unsqueeze(2).repeat(1,1,T,1,1), evals/image_classification_frozen/eval.py:452-455).  All tubelets of one
// spatial cell of that clip are the same row, so only the gh*gw distinct ones are packed (idx == NULL: K = gh*gw, row k
// is cell k).  With idx, row k of image b is cell idx[b,k] % (gh*gw): an index into the (t,h,w) grid of the repeated clip
// names the same pixels as its spatial part.  Element order (c,dt,dh,dw) as tubelet_pack; every pixel is read ONCE and
// its bf16 rounding is written to the `tub` dt slices.  Same fp32 -> bf16 rounding of the same pixels as tubelet_pack on
// the repeated clip: the rows are bit-identical to that kernel's.  8 pixels per thread.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void image_pack_kernel(const float* __restrict__ images, bf16_t* __restrict__ out,
                                                         const int64_t* __restrict__ idx, int64_t B, int C, int H, int W,
                                                         int tub, int p, int64_t K) {
  const int gh = H / p, gw = W / p;
  const int kdim = C * tub * p * p;
  const int cpr = C * p * p / 8;  // 16-byte input chunks per row (one dt slice)
  const int64_t cells = (int64_t)gh * gw;
  const int64_t total = B * K * cpr;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
    const int64_t row = q / cpr;
    const int e = (int)(q - row * cpr) * 8;   // offset inside the (c,dh,dw) slice
    const int64_t b = row / K;
    const int64_t n = (idx ? idx[row] : (row - b * K)) % cells;
    const int wq = (int)(n % gw), hq = (int)(n / gw);
    const int dw = e % p, dh = (e / p) % p, c = e / (p * p);
    const float* s = images + (((b * C + c) * H + (hq * p + dh)) * (int64_t)W + wq * p + dw);
    const float4 lo = *(const float4*)s;
    const float4 hi = *(const float4*)(s + 4);
    u32x4_t o;
    o[0] = pack_bf2(lo.x, lo.y);
    o[1] = pack_bf2(lo.z, lo.w);
    o[2] = pack_bf2(hi.x, hi.y);
    o[3] = pack_bf2(hi.z, hi.w);
    bf16_t* d = out + row * kdim + ((int64_t)c * tub * p + dh) * p + dw;
    for (int dt = 0; dt < tub; dt++) *(u32x4_t*)(d + (int64_t)dt * p * p) = o;
  }
}

extern "C" int vj_image_pack(const float* images, void* out_bf16, const int64_t* idx, int64_t B, int64_t C, int64_t H,
                             int64_t W, int64_t tubelet, int64_t patch, int64_t K, hipStream_t stream) {
  VJ_CHECK_ARG(B >= 0 && K >= 0 && C > 0 && H > 0 && W > 0 && tubelet > 0 && patch > 0,
               "vj_image_pack: bad dims B=%ld K=%ld C=%ld H=%ld W=%ld tubelet=%ld patch=%ld", (long)B, (long)K, (long)C,
               (long)H, (long)W, (long)tubelet, (long)patch);
  VJ_CHECK_ARG(patch % 8 == 0, "vj_image_pack: patch (%ld) must be a multiple of 8", (long)patch);
  VJ_CHECK_ARG(H % patch == 0 && W % patch == 0, "vj_image_pack: image %ldx%ld not divisible into tubelets of patch %ld",
               (long)H, (long)W, (long)patch);
  VJ_CHECK_ARG(idx != nullptr || K == (H / patch) * (W / patch), "vj_image_pack: K=%ld must be gh*gw=%ld without idx", (long)K,
               (long)((H / patch) * (W / patch)));
  VJ_CHECK_ARG(C * tubelet * patch * patch < (1ll << 31), "vj_image_pack: row too long");
  if (B * K == 0) return 0;
  const int64_t total = B * K * (C * patch * patch / 8);
  int64_t g = cdiv64(total, 256);
  if (g > 256 * 32) g = 256 * 32;
  hipLaunchKernelGGL(image_pack_kernel, dim3((int)g), dim3(256), 0, stream, images, (bf16_t*)out_bf16, idx, B, (int)C, (int)H,
                     (int)W, (int)tubelet, (int)patch, K);
  VJ_LAUNCH_CHECK("vj_image_pack");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// add_pos_bcast: out[b, t*S + s, :] = bf16(float(y[b,s,:]) + pos[t*S + s, :]), t < Gt.  y = patch embedding of the S
// distinct tubelets of a still image; the Gt temporal slices of the repeated clip share it and differ only in their
// position rows.  The add is add_pos_kernel's (fp32, one rounding), so out equals add_pos on the Gt-fold repeated rows
// bit for bit.  One wave per (b,s): y is read once, Gt position rows are read and Gt output rows written.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void add_pos_bcast_kernel(const bf16_t* __restrict__ y, const float* __restrict__ pos,
                                                            bf16_t* __restrict__ out, int64_t rows, int64_t S, int64_t Gt,
                                                            int D) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t r = wave; r < rows; r += nw) {
    const int64_t b = r / S, s = r - b * S;
    const bf16_t* yp = y + r * D;
    for (int c = lane * 8; c < D; c += 512) {
      const u32x4_t v = *(const u32x4_t*)(yp + c);
      for (int64_t t = 0; t < Gt; t++) {
        const float* pp = pos + (t * S + s) * D + c;
        const float4 p0 = *(const float4*)pp;
        const float4 p1 = *(const float4*)(pp + 4);
        u32x4_t o;
        o[0] = pack_bf2(bf_lo(v[0]) + p0.x, bf_hi(v[0]) + p0.y);
        o[1] = pack_bf2(bf_lo(v[1]) + p0.z, bf_hi(v[1]) + p0.w);
        o[2] = pack_bf2(bf_lo(v[2]) + p1.x, bf_hi(v[2]) + p1.y);
        o[3] = pack_bf2(bf_lo(v[3]) + p1.z, bf_hi(v[3]) + p1.w);
        *(u32x4_t*)(out + ((b * Gt + t) * S + s) * D + c) = o;
      }
    }
  }
}

extern "C" int vj_add_pos_bcast(const void* y_bf16, const float* pos, void* out_bf16, int64_t B, int64_t S, int64_t Gt,
                                int64_t D, hipStream_t stream) {
  VJ_CHECK_ARG(B >= 0 && S >= 0 && Gt >= 0 && D > 0, "vj_add_pos_bcast: bad dims B=%ld S=%ld Gt=%ld D=%ld", (long)B, (long)S,
               (long)Gt, (long)D);
  VJ_CHECK_ARG(D % 8 == 0, "vj_add_pos_bcast: D=%ld must be a multiple of 8", (long)D);
  const int64_t rows = B * S;
  if (rows * Gt == 0) return 0;
  hipLaunchKernelGGL(add_pos_bcast_kernel, dim3(rows_grid(rows)), dim3(256), 0, stream, (const bf16_t*)y_bf16, pos,
                     (bf16_t*)out_bf16, rows, S, Gt, (int)D);
  VJ_LAUNCH_CHECK("vj_add_pos_bcast");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// pos_interp3d: fp32 table [Nt,Nh,Nw,D] -> [To,Ho,Wo,D], the trilinear F.interpolate(scale_factor=(st,sh,sw)) of
// interpolate_pos_encoding (src/models/vision_transformer.py:197-228) on the channels-last view it permutes to and from.
// align_corners=False with the scale factor GIVEN: per axis src = (dst + 0.5) * r - 0.5 clamped below at 0, with
// r = float(1 / scale) (not in/out); i0 = int(src), i1 = i0 + (i0 < in - 1), weights src - i0 and 1 - (src - i0).  The
// products and differences of the coordinate are kept unfused so they round as the plain expression does.  One thread
// per 4 output floats; the 8 corner rows are 16-byte loads.
// ---------------------------------------------------------------------------------------------
struct InterpAxis {
  int i0, i1;
  float w0, w1;
};

__device__ __forceinline__ InterpAxis interp_axis(int dst, float r, int in) {
  float src = __fsub_rn(__fmul_rn(r, (float)dst + 0.5f), 0.5f);
  if (src < 0.f) src = 0.f;
  int i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  float l = src - (float)i0;
  l = l < 0.f ? 0.f : (l > 1.f ? 1.f : l);
  InterpAxis a;
  a.i0 = i0;
  a.i1 = i0 + (i0 < in - 1 ? 1 : 0);
  a.w1 = l;
  a.w0 = 1.f - l;
  return a;
}

__global__ __launch_bounds__(256) void pos_interp3d_kernel(const float* __restrict__ in, float* __restrict__ out, int Nt,
                                                           int Nh, int Nw, int D, float rt, float rh, float rw, int To,
                                                           int Ho, int Wo) {
  const int dv = D / 4;
  const int64_t total = (int64_t)To * Ho * Wo * dv;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
    const int64_t cell = q / dv;
    const int c = (int)(q - cell * dv) * 4;
    const int w = (int)(cell % Wo), h = (int)((cell / Wo) % Ho), t = (int)(cell / ((int64_t)Wo * Ho));
    const InterpAxis at = interp_axis(t, rt, Nt), ah = interp_axis(h, rh, Nh), aw = interp_axis(w, rw, Nw);
    float4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int ti = (k & 4) ? at.i1 : at.i0, hi = (k & 2) ? ah.i1 : ah.i0, wi = (k & 1) ? aw.i1 : aw.i0;
      const float wt = ((k & 4) ? at.w1 : at.w0) * ((k & 2) ? ah.w1 : ah.w0) * ((k & 1) ? aw.w1 : aw.w0);
      const float4 v = *(const float4*)(in + (((int64_t)ti * Nh + hi) * Nw + wi) * D + c);
      acc.x += wt * v.x;
      acc.y += wt * v.y;
      acc.z += wt * v.z;
      acc.w += wt * v.w;
    }
    *(float4*)(out + cell * D + c) = acc;
  }
}

extern "C" int vj_pos_interp3d(const float* table, float* out, int64_t Nt, int64_t Nh, int64_t Nw, int64_t D, double scale_t,
                               double scale_h, double scale_w, int64_t To, int64_t Ho, int64_t Wo, hipStream_t stream) {
  VJ_CHECK_ARG(Nt > 0 && Nh > 0 && Nw > 0 && D > 0 && Nt < (1 << 20) && Nh < (1 << 20) && Nw < (1 << 20),
               "vj_pos_interp3d: bad table dims %ldx%ldx%ldx%ld", (long)Nt, (long)Nh, (long)Nw, (long)D);
  VJ_CHECK_ARG(D % 4 == 0, "vj_pos_interp3d: D=%ld must be a multiple of 4", (long)D);
  VJ_CHECK_ARG(scale_t > 0.0 && scale_h > 0.0 && scale_w > 0.0, "vj_pos_interp3d: scale factors must be positive");
  VJ_CHECK_ARG(To > 0 && Ho > 0 && Wo > 0 && To < (1 << 20) && Ho < (1 << 20) && Wo < (1 << 20),
               "vj_pos_interp3d: non-positive output grid %ldx%ldx%ld", (long)To, (long)Ho, (long)Wo);
  // F.interpolate's output extent for a given scale factor: floor(in * scale) in double
  VJ_CHECK_ARG(To == (int64_t)floor((double)Nt * scale_t) && Ho == (int64_t)floor((double)Nh * scale_h) &&
                   Wo == (int64_t)floor((double)Nw * scale_w),
               "vj_pos_interp3d: output grid %ldx%ldx%ld is not floor(in * scale)", (long)To, (long)Ho, (long)Wo);
  const int64_t total = To * Ho * Wo * (D / 4);
  int64_t g = cdiv64(total, 256);
  if (g > 256 * 32) g = 256 * 32;
  hipLaunchKernelGGL(pos_interp3d_kernel, dim3((int)g), dim3(256), 0, stream, table, out, (int)Nt, (int)Nh, (int)Nw, (int)D,
                     (float)(1.0 / scale_t), (float)(1.0 / scale_h), (float)(1.0 / scale_w), (int)To, (int)Ho, (int)Wo);
  VJ_LAUNCH_CHECK("vj_pos_interp3d");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// pos_interp2d_bicubic: fp32 table [Nh,Nw,D] -> [Ho,Wo,D], the bicubic F.interpolate(scale_factor=s) of the image branch of
// interpolate_pos_encoding (src/models/vision_transformer.py:230-246) on the channels-last view it permutes to and from.
// align_corners=False with the scale factor GIVEN: per axis src = (dst + 0.5) * r - 0.5 with r = float(1 / scale), NOT
// clamped at zero (only the linear modes clamp); i = floor(src), t = src - i; the four taps i-1 .. i+2 are clamped into
// [0, in-1] and weighted by the cubic convolution with A = -0.75:
//   w0 = ((A(t+1) - 5A)(t+1) + 8A)(t+1) - 4A,  w1 = ((A+2)t - (A+3))t^2 + 1,  w2 = w1(1-t),  w3 = w0(1-t).
// Rows are blended last, each an fp32 sum of its four columns.  One thread per 4 output floats; the 16 taps are 16-byte loads.
// ---------------------------------------------------------------------------------------------
struct CubicAxis {
  int i[4];
  float w[4];
};

__device__ __forceinline__ float cubic_near(float x) {   // |x| <= 1
  const float A = -0.75f;
  return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
}

__device__ __forceinline__ float cubic_far(float x) {   // 1 < |x| < 2
  const float A = -0.75f;
  return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
}

__device__ __forceinline__ CubicAxis cubic_axis(int dst, float r, int in) {
  const float src = __fsub_rn(__fmul_rn(r, (float)dst + 0.5f), 0.5f);
  int i0 = (int)floorf(src);
  if (i0 > in - 1) i0 = in - 1;
  float t = src - (float)i0;
  t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
  CubicAxis a;
#pragma unroll
  for (int k = 0; k < 4; k++) a.i[k] = min(max(i0 - 1 + k, 0), in - 1);
  a.w[0] = cubic_far(t + 1.f);
  a.w[1] = cubic_near(t);
  a.w[2] = cubic_near(1.f - t);
  a.w[3] = cubic_far((1.f - t) + 1.f);
  return a;
}

__global__ __launch_bounds__(256) void pos_interp2d_bicubic_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                   int Nh, int Nw, int D, float r, int Ho, int Wo) {
  const int dv = D / 4;
  const int64_t total = (int64_t)Ho * Wo * dv;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
    const int64_t cell = q / dv;
    const int c = (int)(q - cell * dv) * 4;
    const int w = (int)(cell % Wo), h = (int)(cell / Wo);
    const CubicAxis ah = cubic_axis(h, r, Nh), aw = cubic_axis(w, r, Nw);
    float4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float* row = in + (int64_t)ah.i[j] * Nw * D + c;
      float4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const float4 v = *(const float4*)(row + (int64_t)aw.i[k] * D);
        s.x += aw.w[k] * v.x;
        s.y += aw.w[k] * v.y;
        s.z += aw.w[k] * v.z;
        s.w += aw.w[k] * v.w;
      }
      acc.x += ah.w[j] * s.x;
      acc.y += ah.w[j] * s.y;
      acc.z += ah.w[j] * s.z;
      acc.w += ah.w[j] * s.w;
    }
    *(float4*)(out + cell * D + c) = acc;
  }
}

extern "C" int vj_pos_interp2d_bicubic(const float* table, float* out, int64_t Nh, int64_t Nw, int64_t D, double scale,
                                       int64_t Ho, int64_t Wo, hipStream_t stream) {
  VJ_CHECK_ARG(Nh > 0 && Nw > 0 && D > 0 && Nh < (1 << 20) && Nw < (1 << 20), "vj_pos_interp2d_bicubic: bad table dims %ldx%ldx%ld",
               (long)Nh, (long)Nw, (long)D);
  VJ_CHECK_ARG(D % 4 == 0, "vj_pos_interp2d_bicubic: D=%ld must be a multiple of 4", (long)D);
  VJ_CHECK_ARG(scale > 0.0, "vj_pos_interp2d_bicubic: the scale factor must be positive");
  VJ_CHECK_ARG(Ho > 0 && Wo > 0 && Ho < (1 << 20) && Wo < (1 << 20), "vj_pos_interp2d_bicubic: non-positive output grid %ldx%ld",
               (long)Ho, (long)Wo);
  // F.interpolate's output extent for a given scale factor: floor(in * scale) in double
  VJ_CHECK_ARG(Ho == (int64_t)floor((double)Nh * scale) && Wo == (int64_t)floor((double)Nw * scale),
               "vj_pos_interp2d_bicubic: output grid %ldx%ld is not floor(in * scale)", (long)Ho, (long)Wo);
  VJ_CHECK_ARG(table != nullptr && out != nullptr, "vj_pos_interp2d_bicubic: null pointer");
  VJ_CHECK_ARG(((uintptr_t)table | (uintptr_t)out) % 16 == 0, "vj_pos_interp2d_bicubic: table and out must be 16-byte aligned");
  const int64_t total = Ho * Wo * (D / 4);
  int64_t g = cdiv64(total, 256);
  if (g > 256 * 32) g = 256 * 32;
  hipLaunchKernelGGL(pos_interp2d_bicubic_kernel, dim3((int)g), dim3(256), 0, stream, table, out, (int)Nh, (int)Nw, (int)D,
                     (float)(1.0 / scale), (int)Ho, (int)Wo);
  VJ_LAUNCH_CHECK("vj_pos_interp2d_bicubic");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// add_pos_frames: x[b, f*N + n, :] (bf16) += pos[idx[b,f], :] (fp32), the temporal position embedding of FrameAggregation
// (evals/video_classification_frozen/utils.py:74-80): every token of frame f of sample b takes the table row of that frame's
// index.  add_pos_kernel's add (fp32, one rounding).  One wave per token row; idx values were validated on the host and are
// clamped into [0, max_frames) here all the same, so no row outside the table is ever read.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void add_pos_frames_kernel(bf16_t* __restrict__ x, const float* __restrict__ pos,
                                                             const int64_t* __restrict__ idx, int64_t rows, int64_t N, int D,
                                                             int64_t max_frames) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t r = wave; r < rows; r += nw) {
    int64_t n = idx[r / N];   // rows = B*F*N, idx is [B,F]: row r belongs to frame r / N
    n = n < 0 ? 0 : (n > max_frames - 1 ? max_frames - 1 : n);
    bf16_t* xp = x + r * D;
    const float* pp = pos + n * D;
    for (int c = lane * 8; c < D; c += 512) {
      u32x4_t v = *(u32x4_t*)(xp + c);
      const float4 p0 = *(const float4*)(pp + c);
      const float4 p1 = *(const float4*)(pp + c + 4);
      v[0] = pack_bf2(bf_lo(v[0]) + p0.x, bf_hi(v[0]) + p0.y);
      v[1] = pack_bf2(bf_lo(v[1]) + p0.z, bf_hi(v[1]) + p0.w);
      v[2] = pack_bf2(bf_lo(v[2]) + p1.x, bf_hi(v[2]) + p1.y);
      v[3] = pack_bf2(bf_lo(v[3]) + p1.z, bf_hi(v[3]) + p1.w);
      *(u32x4_t*)(xp + c) = v;
    }
  }
}

extern "C" int vj_add_pos_frames(void* x_bf16, const float* pos, const int64_t* idx, int64_t B, int64_t F, int64_t N, int64_t D,
                                 int64_t max_frames, hipStream_t stream) {
  VJ_CHECK_ARG(B >= 0 && F >= 0 && N >= 0 && D > 0 && max_frames > 0, "vj_add_pos_frames: bad dims B=%ld F=%ld N=%ld D=%ld max_frames=%ld",
               (long)B, (long)F, (long)N, (long)D, (long)max_frames);
  VJ_CHECK_ARG(D % 8 == 0, "vj_add_pos_frames: D=%ld must be a multiple of 8", (long)D);
  const int64_t rows = B * F * N;
  if (rows == 0) return 0;
  VJ_CHECK_ARG(x_bf16 != nullptr && pos != nullptr && idx != nullptr, "vj_add_pos_frames: null pointer");
  VJ_CHECK_ARG(((uintptr_t)x_bf16 | (uintptr_t)pos) % 16 == 0, "vj_add_pos_frames: x and pos must be 16-byte aligned");
  hipLaunchKernelGGL(add_pos_frames_kernel, dim3(rows_grid(rows)), dim3(256), 0, stream, (bf16_t*)x_bf16, pos, idx, rows, N,
                     (int)D, max_frames);
  VJ_LAUNCH_CHECK("vj_add_pos_frames");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// pred_assemble_fwd: out[b, j, :] = j < Ke ? e[b,j,:] + pos[idx_e[b,j]] : tok[:] + pos[idx_p[b,j-Ke]]
//   e  = predictor_embed(z)   bf16 [B,Ke,Dp]     (predictor.py:194-200)
//   tok = mask_tokens[i]      fp32 [Dp]          (predictor.py:207-217)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pred_assemble_kernel(const bf16_t* __restrict__ e, const float* __restrict__ tok,
                                                            const float* __restrict__ pos,
                                                            const int64_t* __restrict__ idx_e,
                                                            const int64_t* __restrict__ idx_p,
                                                            bf16_t* __restrict__ out, int64_t B, int64_t Ke,
                                                            int64_t Kp, int D) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  const int64_t S = Ke + Kp;
  for (int64_t r = wave; r < B * S; r += nw) {
    const int64_t b = r / S, j = r - b * S;
    const bool ctx = j < Ke;
    const int64_t n = ctx ? idx_e[b * Ke + j] : idx_p[b * Kp + (j - Ke)];
    const float* pp = pos + n * D;
    const bf16_t* ep = e + (b * Ke + j) * D;
    bf16_t* op = out + r * D;
    for (int c = lane * 8; c < D; c += 512) {
      float v[8];
      if (ctx) {
        const u32x4_t w = *(const u32x4_t*)(ep + c);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          v[2 * i] = bf_lo(w[i]);
          v[2 * i + 1] = bf_hi(w[i]);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = tok[c + i];
      }
      u32x4_t o;
#pragma unroll
      for (int i = 0; i < 4; i++) o[i] = pack_bf2(v[2 * i] + pp[c + 2 * i], v[2 * i + 1] + pp[c + 2 * i + 1]);
      *(u32x4_t*)(op + c) = o;
    }
  }
}

extern "C" int vj_pred_assemble_fwd(const void* e_bf16, const float* mask_token, const float* pos,
                                    const int64_t* idx_e, const int64_t* idx_p, void* out_bf16, int64_t B,
                                    int64_t Ke, int64_t Kp, int64_t D, hipStream_t stream) {
  VJ_CHECK_ARG(D % 8 == 0, "vj_pred_assemble_fwd: D=%ld must be a multiple of 8", (long)D);
  const int64_t rows = B * (Ke + Kp);
  if (rows == 0) return 0;
  hipLaunchKernelGGL(pred_assemble_kernel, dim3(rows_grid(rows)), dim3(256), 0, stream, (const bf16_t*)e_bf16,
                     mask_token, pos, idx_e, idx_p, (bf16_t*)out_bf16, B, Ke, Kp, (int)D);
  VJ_LAUNCH_CHECK("vj_pred_assemble_fwd");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// transpose_bf16: in [M,N] (ld_in) -> out [N, Mpad], out[n, m>=M] = 0.  64x64 tiles through LDS.
// Feeds the K-contiguous ("NT") MFMA GEMM with the wgrad operands dY^T and X^T.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void transpose_bf16_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out,
                                                             int64_t M, int64_t N, int64_t ld_in, int64_t Mpad,
                                                             float* __restrict__ part) {
  __shared__ bf16_t tile[64][66];
  const int64_t m0 = (int64_t)blockIdx.x * 64, n0 = (int64_t)blockIdx.y * 64;
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
  if (part != nullptr && t < 64 && n0 + t < N) {  // fused bias-gradient partial: column sums of this 64-row tile
    float sum = 0.f;
#pragma unroll 16
    for (int r = 0; r < 64; r++) sum += bf2f(tile[r][t]);
    part[(int64_t)blockIdx.x * N + n0 + t] = sum;
  }
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
// colsum_bf16: partial[p][n] = sum over the p-th row chunk of in[m][n] (rows m in [row_lo,row_hi) of
// each group of `group` rows -- used both for plain bias grads (group = M) and for the mask-token grad,
// which sums only the target rows j >= Ke of every [Ke+Kp]-row sample).  Deterministic two-stage sum.
// ---------------------------------------------------------------------------------------------
#define VJ_COLSUM_PARTS 256   // maximum number of row chunks (workspace sizing); the launcher picks 64 .. 256
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
__global__ __launch_bounds__(512) void reduce_partials_kernel(const float* __restrict__ part, ReduceOuts outs, int64_t seg,
                                                              int64_t P, int64_t N, int64_t stride, float alpha,
                                                              float beta) {
  __shared__ float red[8][64];
  const int c = threadIdx.x & 63, pl = threadIdx.x >> 6;
  const int64_t n = (int64_t)blockIdx.x * 64 + c;
  float s = 0.f;
  if (n < N) {
#pragma unroll 8
    for (int64_t p = pl; p < P; p += 8) s += part[p * stride + n];
  }
  red[pl][c] = s;
  __syncthreads();
  if (pl == 0 && n < N) {
    float t = red[0][c];
#pragma unroll
    for (int i = 1; i < 8; i++) t += red[i][c];
    t *= alpha;
    const int64_t sg = n / seg;                       // workgroup-uniform (seg % 64 == 0)
    float* o = (sg == 0 ? outs.o[0] : (sg == 1 ? outs.o[1] : outs.o[2])) + (n - sg * seg);
    if (beta != 0.f) t += beta * *o;
    *o = t;
  }
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
  __shared__ float red[8][64];
  int sg = 0;
  while (sg + 1 < rs.n && (int)blockIdx.x >= rs.blk_end[sg]) sg++;      // workgroup-uniform
  const int blk0 = sg == 0 ? 0 : rs.blk_end[sg - 1];
  const float* part = rs.part[sg];
  const int64_t P = rs.P[sg], N = rs.N[sg], stride = rs.stride[sg];
  const int c = threadIdx.x & 63, pl = threadIdx.x >> 6;
  const int64_t n = (int64_t)((int)blockIdx.x - blk0) * 64 + c;
  float s = 0.f;
  if (n < N) {
#pragma unroll 8
    for (int64_t p = pl; p < P; p += 8) s += part[p * stride + n];
  }
  red[pl][c] = s;
  __syncthreads();
  if (pl == 0 && n < N) {
    float t = red[0][c];
#pragma unroll
    for (int i = 1; i < 8; i++) t += red[i][c];
    t *= alpha;
    float* o = rs.out[sg] + n;
    if (beta != 0.f) t += beta * *o;
    *o = t;
  }
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
  // row chunks: enough workgroups (>= ~2048, 8 per CU) to keep HBM busy when N is narrow (N = 1024: 4 column groups), at
  // least 8 rows per row lane and chunk; the chunk count only changes the (fixed, deterministic) summation order
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

// ---------------------------------------------------------------------------------------------
// copy_rows_strided: dst[b, dst_off + j, :] = src[b, src_off + j, :] for j < n  (bf16 rows; used to split the
// predictor stream into its context rows (grad of predictor_embed) and to slice target rows).  src == nullptr: the
// destination rows are ZEROED (the context rows of the predictor trunk's output gradient: no ATen fill on the step).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void copy_rows_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst,
                                                        int64_t B, int64_t src_rows, int64_t src_off,
                                                        int64_t dst_rows, int64_t dst_off, int64_t n, int D) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t r = wave; r < B * n; r += nw) {
    const int64_t b = r / n, j = r - b * n;
    u32x4_t* dp = (u32x4_t*)(dst + (b * dst_rows + dst_off + j) * D);
    if (src != nullptr) {   // (kernel argument: uniform)
      const u32x4_t* sp = (const u32x4_t*)(src + (b * src_rows + src_off + j) * D);
      for (int c = lane; c < D / 8; c += 64) dp[c] = sp[c];
    } else {
      for (int c = lane; c < D / 8; c += 64) dp[c] = (u32x4_t){0u, 0u, 0u, 0u};
    }
  }
}

extern "C" int vj_copy_rows(const void* src, void* dst, int64_t B, int64_t src_rows, int64_t src_off,
                            int64_t dst_rows, int64_t dst_off, int64_t n, int64_t D, hipStream_t stream) {
  VJ_CHECK_ARG(D % 8 == 0, "vj_copy_rows: D must be a multiple of 8");
  VJ_CHECK_ARG((src == nullptr || src_off + n <= src_rows) && dst_off + n <= dst_rows, "vj_copy_rows: slice out of range");
  if (B * n == 0) return 0;
  hipLaunchKernelGGL(copy_rows_kernel, dim3(rows_grid(B * n)), dim3(256), 0, stream, (const bf16_t*)src,
                     (bf16_t*)dst, B, src_rows, src_off, dst_rows, dst_off, n, (int)D);
  VJ_LAUNCH_CHECK("vj_copy_rows");
  return 0;
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
  __shared__ bf16_t tile[64][66];
  const int4 bi = blocks[blockIdx.x];
  const TransposeDesc d = desc[bi.x];
  const int64_t m0 = (int64_t)bi.y * 64, n0 = (int64_t)bi.z * 64;
  const int t = threadIdx.x;
#pragma unroll
  for (int it = 0; it < 2; it++) {
    const int q = t + it * 256;
    const int r = q >> 3, c = (q & 7) * 8;
    u32x4_t v = {0, 0, 0, 0};
    if (m0 + r < d.M && n0 + c < d.N) v = *(const u32x4_t*)(d.src + (m0 + r) * d.ld_in + n0 + c);
#pragma unroll
    for (int i = 0; i < 4; i++) *(uint32_t*)&tile[r][c + 2 * i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 2; it++) {
    const int q = t + it * 256;
    const int n = q >> 3, mc = (q & 7) * 8;
    if (n0 + n < d.N && m0 + mc < d.Mpad) {
      u32x4_t o;
#pragma unroll
      for (int i = 0; i < 4; i++)
        o[i] = (uint32_t)tile[mc + 2 * i][n] | ((uint32_t)tile[mc + 2 * i + 1][n] << 16);
      *(u32x4_t*)(d.dst + (n0 + n) * d.Mpad + m0 + mc) = o;
    }
  }
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
