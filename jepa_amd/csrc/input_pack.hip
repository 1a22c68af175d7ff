// Pixels to model input: tubelet packing of fp32 clips (and of still images repeated along time) into bf16 patch rows, and the
// device-side clip augmentation that turns decoded uint8 frames into model-ready fp32 clips.
//
// Reference behaviour restated (never copied):
//   PatchEmbed3D token/K ordering    src/models/utils/patch_embed.py:31-57
//   still image -> repeated clip     evals/image_classification_frozen/eval.py:452-455
//   VideoTransform.__call__          app/vjepa/transforms.py:86-115,138-153
//   eval VideoTransform / EvalVideoTransform   evals/video_classification_frozen/utils.py:251-283,303-323,326-343
//   RandomErasing._erase_cube        src/datasets/utils/video/randerase.py:116-156
#include "common.hpp"
#include "../../include/vjepa_hip.h"

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
    *(u32x4_t*)(out + row * kdim + e) = pack8_bf16(*(const float4*)s, *(const float4*)(s + 4));
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
  hipLaunchKernelGGL(tubelet_pack_kernel, dim3(flat_grid(total, 256 * 32)), dim3(256), 0, stream, clips, (bf16_t*)out_bf16, idx, B,
                     (int)C, (int)T, (int)H, (int)W, (int)tubelet, (int)patch, K);
  VJ_LAUNCH_CHECK("vj_tubelet_pack");
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
    const u32x4_t o = pack8_bf16(*(const float4*)s, *(const float4*)(s + 4));
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
  hipLaunchKernelGGL(image_pack_kernel, dim3(flat_grid(total, 256 * 32)), dim3(256), 0, stream, images, (bf16_t*)out_bf16, idx, B, (int)C, (int)H,
                     (int)W, (int)tubelet, (int)patch, K);
  VJ_LAUNCH_CHECK("vj_image_pack");
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
//
// PRE is the normalise-first form of the frozen eval (evals/video_classification_frozen/utils.py:256-274: ToTensor / 255, then
// tensor_normalize, then random_resized_crop; EvalVideoTransform: ClipToTensor / 255, then Normalize): every source byte u of
// channel c becomes n = (float(u) / 255 - mean_c) / std_c -- three separately rounded fp32 operations, mean / std in 0..1 units --
// and the taps are blended with the same arithmetic; nothing follows the blend.  n depends on (u, c) alone, so a block computes the
// 768 values once into LDS and a tap is a table read.  A box with h == w == S has scale 1: the fused coordinate is the integer dst,
// the weights are exactly 1 and 0, and the output is the tap itself, bit for bit (the validation views: crops without a resize).
// ---------------------------------------------------------------------------------------------
// ClipAxis (here), InterpAxis and CubicAxis (pos_interp.hip) look alike and stay three: each encodes the rounding of the code it
// reproduces -- a FUSED coordinate for the CPU reference of the clip transform, unfused products for F.interpolate's linear modes,
// and no clamp at zero for bicubic.
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

template <bool PRE>
__global__ __launch_bounds__(256) void clip_transform_kernel(const uint8_t* __restrict__ frames, int64_t frames_bytes,
                                                             const int64_t* __restrict__ desc,
                                                             const int4* __restrict__ boxes, float* __restrict__ out,
                                                             int64_t B, int T, int S, ClipNorm nm) {
  [[maybe_unused]] const float* lut = nullptr;
  if constexpr (PRE) {
    __shared__ float norm_lut[3][256];
#pragma unroll
    for (int c = 0; c < 3; c++) norm_lut[c][threadIdx.x] = ((float)threadIdx.x / 255.f - nm.mean[c]) / nm.std[c];
    __syncthreads();
    lut = &norm_lut[0][0];
  }
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
          float p00, p01, p10, p11;
          if constexpr (PRE) {
            p00 = lut[c * 256 + r0[ax.i0 * 3 + c]], p01 = lut[c * 256 + r0[ax.i1 * 3 + c]];
            p10 = lut[c * 256 + r1[ax.i0 * 3 + c]], p11 = lut[c * 256 + r1[ax.i1 * 3 + c]];
          } else {
            p00 = (float)r0[ax.i0 * 3 + c], p01 = (float)r0[ax.i1 * 3 + c];
            p10 = (float)r1[ax.i0 * 3 + c], p11 = (float)r1[ax.i1 * 3 + c];
          }
          const float top = ax.w0 * p00 + ax.w1 * p01, bot = ax.w0 * p10 + ax.w1 * p11;
          if constexpr (PRE) v[c][k] = ay.w0 * top + ay.w1 * bot;
          else v[c][k] = (ay.w0 * top + ay.w1 * bot - nm.mean[c]) / nm.std[c];
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

template <bool PRE>
static int clip_transform_launch(const char* what, const uint8_t* frames, int64_t frames_bytes, const int64_t* desc,
                                 const int32_t* boxes, float* out, int64_t B, int64_t T, int64_t S, const ClipNorm& nm,
                                 hipStream_t stream) {
  VJ_CHECK_ARG(B >= 0 && T > 0 && S > 0 && frames_bytes >= 0 && T < (1 << 20) && S < (1 << 20),
               "%s: bad dims B=%ld T=%ld S=%ld frames_bytes=%ld", what, (long)B, (long)T, (long)S, (long)frames_bytes);
  VJ_CHECK_ARG(S % 4 == 0, "%s: S=%ld must be a multiple of 4", what, (long)S);
  VJ_CHECK_ARG(nm.std[0] != 0.f && nm.std[1] != 0.f && nm.std[2] != 0.f, "%s: std must be non-zero", what);
  if (B == 0) return 0;
  VJ_CHECK_ARG(frames != nullptr && desc != nullptr && boxes != nullptr && out != nullptr, "%s: null pointer", what);
  VJ_CHECK_ARG(((uintptr_t)out % 16 == 0) && ((uintptr_t)boxes % 16 == 0), "%s: out and boxes must be 16-byte aligned", what);
  const int64_t total = B * T * S * (S / 4);
  VJ_CHECK_ARG(B < (1ll << 31) && total < (1ll << 31), "%s: batch too large (B=%ld)", what, (long)B);
  hipLaunchKernelGGL(clip_transform_kernel<PRE>, dim3(flat_grid(total, 256 * 32)), dim3(256), 0, stream, frames, frames_bytes, desc,
                     (const int4*)boxes, out, B, (int)T, (int)S, nm);
  VJ_LAUNCH_CHECK(what);
  return 0;
}

extern "C" int vj_clip_transform(const uint8_t* frames, int64_t frames_bytes, const int64_t* desc, const int32_t* boxes,
                                 float* out, int64_t B, int64_t T, int64_t S, float mean_r, float mean_g, float mean_b,
                                 float std_r, float std_g, float std_b, hipStream_t stream) {
  const ClipNorm nm = {{mean_r, mean_g, mean_b}, {std_r, std_g, std_b}};
  return clip_transform_launch<false>("vj_clip_transform", frames, frames_bytes, desc, boxes, out, B, T, S, nm, stream);
}

extern "C" int vj_clip_transform_pre(const uint8_t* frames, int64_t frames_bytes, const int64_t* desc, const int32_t* boxes,
                                     float* out, int64_t B, int64_t T, int64_t S, float mean_r, float mean_g, float mean_b,
                                     float std_r, float std_g, float std_b, hipStream_t stream) {
  const ClipNorm nm = {{mean_r, mean_g, mean_b}, {std_r, std_g, std_b}};
  return clip_transform_launch<true>("vj_clip_transform_pre", frames, frames_bytes, desc, boxes, out, B, T, S, nm, stream);
}

// ---------------------------------------------------------------------------------------------
// clip_erase: RandomErasing in cube mode (randerase.py:116-156: one box per clip, fresh N(0,1) values for every frame, written
// after flip and normalisation) as a copy: clips[b,c,t,top+y,left+x] = noise[noise_off[b] + ((t*3+c)*h+y)*w+x] for the box
// ebox[b] = (top, left, h, w); h == 0: the clip is not erased.  The values are a DRAW, made on the host in the reference's order
// and shipped as [T,3,h,w] per erased clip.  Block row b walks the 3*T*h*w values of clip b, consecutive threads on consecutive
// noise elements and (within a box row) consecutive pixels.  A clip whose box leaves S x S or whose block leaves
// [0, noise_elems) is skipped whole: nothing outside either buffer is read or written.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clip_erase_kernel(float* __restrict__ clips, const int4* __restrict__ ebox,
                                                         const float* __restrict__ noise, int64_t noise_elems,
                                                         const int64_t* __restrict__ noise_off, int T, int S) {
  const int64_t b = blockIdx.y;
  const int4 e = ebox[b];  // (top, left, h, w)
  if (e.z <= 0 || e.w <= 0 || e.x < 0 || e.y < 0 || e.z > S - e.x || e.w > S - e.y) return;
  const int64_t off = noise_off[b];
  const uint32_t n = (uint32_t)T * 3u * (uint32_t)e.z * (uint32_t)e.w;   // <= 3*T*S*S < 2^31 (checked by the launcher)
  if (off < 0 || off > noise_elems || (int64_t)n > noise_elems - off) return;
  const uint32_t h = (uint32_t)e.z, w = (uint32_t)e.w;
  float* base = clips + b * 3 * T * (int64_t)S * S + (int64_t)e.x * S + e.y;
  for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < n; q += gridDim.x * 256u) {
    const uint32_t r = q / w, x = q - r * w;
    const uint32_t tc = r / h, y = r - tc * h;
    const uint32_t t = tc / 3u, c = tc - t * 3u;
    base[((int64_t)c * T + t) * S * S + (int64_t)y * S + x] = noise[off + q];
  }
}

extern "C" int vj_clip_erase(float* clips, const int32_t* ebox, const float* noise, int64_t noise_elems, const int64_t* noise_off,
                             int64_t B, int64_t T, int64_t S, hipStream_t stream) {
  VJ_CHECK_ARG(B >= 0 && T > 0 && S > 0 && noise_elems >= 0 && B < 65536 && 3 * T * S * S < (1ll << 31) && T < (1 << 20) && S < (1 << 20),
               "vj_clip_erase: bad dims B=%ld T=%ld S=%ld noise_elems=%ld", (long)B, (long)T, (long)S, (long)noise_elems);
  if (B == 0 || noise_elems == 0) return 0;   // no clip of the batch is erased: nothing is launched
  VJ_CHECK_ARG(clips != nullptr && ebox != nullptr && noise != nullptr && noise_off != nullptr, "vj_clip_erase: null pointer");
  VJ_CHECK_ARG((uintptr_t)ebox % 16 == 0, "vj_clip_erase: ebox must be 16-byte aligned");
  const int64_t widest = 3 * T * S * S;
  hipLaunchKernelGGL(clip_erase_kernel, dim3(flat_grid(widest, 256), (unsigned)B), dim3(256), 0, stream, clips, (const int4*)ebox,
                     noise, noise_elems, noise_off, (int)T, (int)S);
  VJ_LAUNCH_CHECK("vj_clip_erase");
  return 0;
}
