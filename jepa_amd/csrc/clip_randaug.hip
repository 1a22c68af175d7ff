// RandAugment on decoded uint8 frames, in place in the flat frame buffer that vj_clip_transform[_pre] reads next.
//
// Reference behaviour restated (never copied):
//   RandAugment / AugmentOp and the operations      src/datasets/utils/video/randaugment.py:51-179,324-369,449-465
//   where the eval applies it (before everything)   evals/video_classification_frozen/utils.py:233-237,256-259
// and, behind those, PIL's own arithmetic on 8-bit RGB images: ImageOps.autocontrast / equalize / invert / posterize / solarize,
// Image.point, ImageEnhance (Image.blend against a degenerate image), ImageFilter.SMOOTH, and Image.transform(AFFINE, BICUBIC)
// with a fill colour.  The draws stay on the host (jepa_amd/app/vjepa/randaugment.py); this file is the pixel work, byte for byte:
// the results are compared with np.array_equal against PIL's.
//
// THIS FILE IS BUILT WITH FLOATING-POINT CONTRACTION OFF (jepa_amd/build.py EXTRA_FLAGS): PIL's x86-64 build rounds every product
// and every sum on its own, and a fused multiply-add moves a value across a truncation boundary.  Geometry is fp64, blend and
// filter are fp32, statistics are integers.
//
// A plan is ops int32 [B,L] / args double [B,L,6]; layer l+1 reads layer l's output, so layers are launched one after the other,
// each reading one copy of the frame buffer and writing the other (frames and the workspace's copy take turns; a clip without an
// operation in a layer is copied through), and an odd number of layers ends with one copy back.  Per layer:
//   randaug_table_kernel   one workgroup per (clip, frame): for the operations that map the bytes of a channel on their own, the
//                          [3][256] table of that frame -- after a 256-bin histogram per channel (AutoContrast, Equalize) or the
//                          sum of the luma (Contrast), both exact integers accumulated with LDS atomics
//   randaug_apply_kernel   table lookup and Color, four pixels per thread; Sharpness and the affine family, one pixel per lane in
//                          tiles of 16 x 4
// Every index is clamped into its frame, and a clip whose extent does not lie inside the buffer on a 16-byte boundary is skipped
// by every kernel: nothing outside [frames, frames + frames_bytes), the same range of the copy, and the tables is touched.
//
// The colour the affine family writes where the source has no pixel is an argument of the one kernel body: vj_clip_randaug passes
// the reference's video _FILL (128, 128, 128), vj_clip_randaug_fill what its caller gives -- the image evals pass timm's
// round(255 * mean) = (124, 116, 104) for the AutoAugment policy of   evals/image_classification_frozen/eval.py:392-403.
#include "common.hpp"
#include "../../include/vjepa_hip.h"

namespace {

enum RaOp : int {
  RA_NONE = 0, RA_AUTO_CONTRAST, RA_EQUALIZE, RA_INVERT, RA_ROTATE, RA_POSTERIZE, RA_SOLARIZE, RA_SOLARIZE_ADD, RA_COLOR,
  RA_CONTRAST, RA_BRIGHTNESS, RA_SHARPNESS, RA_SHEAR_X, RA_SHEAR_Y, RA_TRANSLATE_X, RA_TRANSLATE_Y
};
constexpr int RA_ARGS = 6;
constexpr int RA_TABLE_BYTES = 3 * 256;
constexpr int RA_MAX_SIDE = 1 << 15;

__device__ __forceinline__ bool ra_is_table(int op) {
  return op == RA_AUTO_CONTRAST || op == RA_EQUALIZE || op == RA_INVERT || op == RA_POSTERIZE || op == RA_SOLARIZE ||
         op == RA_SOLARIZE_ADD || op == RA_CONTRAST || op == RA_BRIGHTNESS;
}

// descriptor row b -> (off, H, W); false: the clip is skipped
__device__ __forceinline__ bool ra_clip(const int64_t* __restrict__ desc, int64_t b, int T, int64_t frames_bytes, int64_t& off,
                                        int& H, int& W) {
  off = desc[b * 4 + 0];
  const int64_t Hs = desc[b * 4 + 1], Ws = desc[b * 4 + 2];
  if (off < 0 || (off & 15) != 0 || off > frames_bytes || Hs <= 0 || Ws <= 0 || Hs >= RA_MAX_SIDE || Ws >= RA_MAX_SIDE) return false;
  H = (int)Hs, W = (int)Ws;
  return (int64_t)T * Hs * Ws * 3 <= frames_bytes - off;
}

__device__ __forceinline__ int ra_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

__device__ __forceinline__ int ra_clip8(float v) { return v <= 0.f ? 0 : v >= 255.f ? 255 : (int)v; }

// ImageEnhance: Image.blend(degenerate, image, factor) = d + f * (i - d), every step an fp32 rounding
__device__ __forceinline__ int ra_blend(int d, int i, float f, bool convex) {
  const float df = (float)d;
  const float prod = f * ((float)i - df);
  const float t = df + prod;
  return convex ? (int)t : ra_clip8(t);
}

__device__ __forceinline__ double ra_cubic(double v1, double v2, double v3, double v4, double d) {
  const double p1 = v2;
  const double p2 = -v1 + v3;
  const double p3 = 2 * (v1 - v2) + v3 - v4;
  const double p4 = -v1 + v2 - v3 + v4;
  return p1 + d * (p2 + d * (p3 + d * p4));
}

// the same cubic across four bytes of a row: its coefficients are integers below 2^11 whichever way they are computed, so they are
// made in int32 and converted, and only the Horner steps are fp64 operations -- the values are those of ra_cubic on the doubles
__device__ __forceinline__ double ra_cubic_bytes(int v1, int v2, int v3, int v4, double d) {
  const double p1 = (double)v2;
  const double p2 = (double)(-v1 + v3);
  const double p3 = (double)(2 * (v1 - v2) + v3 - v4);
  const double p4 = (double)(-v1 + v2 - v3 + v4);
  return p1 + d * (p2 + d * (p3 + d * p4));
}

// ---------------------------------------------------------------------------------------------
// tables[(b*T + t)][3][256] for the table operations of one layer
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void randaug_table_kernel(const uint8_t* __restrict__ src, int64_t frames_bytes,
                                                            const int64_t* __restrict__ desc, const int32_t* __restrict__ ops,
                                                            const double* __restrict__ args, int L, int layer, int T,
                                                            uint8_t* __restrict__ tables) {
  const int64_t bt = blockIdx.x;
  const int64_t b = bt / T;
  const int t = (int)(bt - b * T);
  const int op = ops[b * L + layer];
  if (!ra_is_table(op)) return;
  int64_t off;
  int H, W;
  if (!ra_clip(desc, b, T, frames_bytes, off, H, W)) return;
  const double arg = args[(b * L + layer) * RA_ARGS];
  const uint32_t HW = (uint32_t)H * (uint32_t)W, n = HW * 3u;
  const uint8_t* f = src + off + (int64_t)t * n;
  const uint32_t tid = threadIdx.x;

  __shared__ uint32_t hist[3][256];
  __shared__ unsigned long long luma_sum;
  __shared__ int lo_s[3], hi_s[3], bins_s[3];

  if (op == RA_AUTO_CONTRAST || op == RA_EQUALIZE) {
    for (uint32_t i = tid; i < 768u; i += 512u) (&hist[0][0])[i] = 0u;
    __syncthreads();
    uint32_t head = (uint32_t)((4u - ((uintptr_t)f & 3u)) & 3u);
    if (head > n) head = n;
    const uint32_t nd = (n - head) / 4u;
    if (tid < head) atomicAdd(&hist[tid % 3u][f[tid]], 1u);
    const uint32_t* fw = (const uint32_t*)(f + head);
    for (uint32_t j = tid; j < nd; j += 512u) {
      const uint32_t v = fw[j];
      uint32_t c = (head + 4u * j) % 3u;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        atomicAdd(&hist[c][(v >> (8 * k)) & 255u], 1u);
        c = c == 2u ? 0u : c + 1u;
      }
    }
    const uint32_t i = head + 4u * nd + tid;
    if (i < n) atomicAdd(&hist[i % 3u][f[i]], 1u);
    __syncthreads();
    if (tid < 3) {
      int lo = 256, hi = -1, bins = 0;
      for (int k = 0; k < 256; k++)
        if (hist[tid][k]) {
          if (lo == 256) lo = k;
          hi = k;
          bins++;
        }
      lo_s[tid] = lo, hi_s[tid] = hi, bins_s[tid] = bins;
    }
    __syncthreads();
  } else if (op == RA_CONTRAST) {
    if (tid == 0) luma_sum = 0ull;
    __syncthreads();
    uint32_t acc = 0;   // at most 2^30 / 512 pixels of at most 255 each per thread
    for (uint32_t p = tid; p < HW; p += 512u) acc += (uint32_t)ra_luma(f[p * 3u], f[p * 3u + 1u], f[p * 3u + 2u]);
    atomicAdd(&luma_sum, (unsigned long long)acc);
    __syncthreads();
  }
  if (tid >= 256u) return;

  const int i = (int)tid;
  uint8_t* tab = tables + bt * RA_TABLE_BYTES;
  if (op == RA_AUTO_CONTRAST || op == RA_EQUALIZE) {
#pragma unroll 1
    for (int c = 0; c < 3; c++) {
      int e = i;
      const int lo = lo_s[c], hi = hi_s[c];
      if (op == RA_AUTO_CONTRAST) {
        if (hi > lo) {
          const double scale = 255.0 / (double)(hi - lo);
          const double offset = -(double)lo * scale;
          const double prod = (double)i * scale;
          const int v = (int)(prod + offset);
          e = v < 0 ? 0 : v > 255 ? 255 : v;
        }
      } else if (bins_s[c] > 1) {
        const uint32_t step = (HW - hist[c][hi]) / 255u;
        if (step) {
          uint32_t acc = step / 2u;
          for (int k = 0; k < i; k++) acc += hist[c][k];
          const uint32_t v = acc / step;
          e = v > 255u ? 255 : (int)v;
        }
      }
      tab[c * 256 + i] = (uint8_t)e;
    }
    return;
  }
  int e = i;
  const int ia = (int)arg;
  if (op == RA_INVERT) {
    e = 255 - i;
  } else if (op == RA_POSTERIZE) {
    const int bits = ia < 0 ? 0 : ia > 8 ? 8 : ia;
    e = i & ~((1 << (8 - bits)) - 1);
  } else if (op == RA_SOLARIZE) {
    e = i < ia ? i : 255 - i;
  } else if (op == RA_SOLARIZE_ADD) {
    const int s = i + (ia < 0 ? 0 : ia > 255 ? 255 : ia);
    e = i < 128 ? (s > 255 ? 255 : s) : i;
  } else {
    const float fct = (float)arg;
    const bool convex = fct >= 0.f && fct <= 1.f;
    int d = 0;
    if (op == RA_CONTRAST) {
      const double mean = (double)luma_sum / (double)HW;
      d = (int)(mean + 0.5);
    }
    e = ra_blend(d, i, fct, convex);
  }
  tab[i] = tab[256 + i] = tab[512 + i] = (uint8_t)e;
}

// ---------------------------------------------------------------------------------------------
// one layer: dst clip = operation(src clip).  ops == nullptr: every clip is copied (the copy back)
// ---------------------------------------------------------------------------------------------
// One output pixel of the affine family.  s: the clip (16-byte aligned), frame: byte offset of the frame in it, clip_bytes: its
// length.  Where the four columns of a row are four different pixels -- everywhere but at the left and right edge -- they are twelve
// consecutive bytes, read as the four aligned words around them (never past the clip's end) instead of twelve byte loads.
typedef uint32_t ra_u32x4_t __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ uint32_t ra_affine_pixel(const uint8_t* __restrict__ s, uint32_t frame, uint32_t clip_bytes, int H, int W,
                                                    int x, int y, const double* a, uint32_t fill) {
  const double xc = (double)x + 0.5, yc = (double)y + 0.5;
  const double xa = a[0] * xc, xb = a[1] * yc;
  const double ya = a[3] * xc, yb = a[4] * yc;
  double xin = (xa + xb) + a[2];
  double yin = (ya + yb) + a[5];
  if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) return fill;
  xin -= 0.5, yin -= 0.5;
  const double xf = floor(xin), yf = floor(yin);
  const double dx = xin - xf, dy = yin - yf;
  const int x0 = (int)xf - 1, y0 = (int)yf - 1;
  const bool inner = x0 >= 0 && x0 + 3 < W;
  int col[4];
#pragma unroll
  for (int k = 0; k < 4; k++) col[k] = min(max(x0 + k, 0), W - 1) * 3;
  double v[3][4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int yy = y0 + k;
    if (k == 0 || (yy >= 0 && yy < H)) {
      const uint32_t row = frame + (uint32_t)min(max(yy, 0), H - 1) * (uint32_t)W * 3u;
      const uint32_t at = row + (uint32_t)col[0];
      if (inner && (at & ~3u) + 16u <= clip_bytes) {
        const ra_u32x4_t q = *(const ra_u32x4_t*)(s + (at & ~3u));
        const uint32_t sh = (at & 3u) * 8u;
        const uint32_t w0 = (uint32_t)((((uint64_t)q.y << 32) | q.x) >> sh), w1 = (uint32_t)((((uint64_t)q.z << 32) | q.y) >> sh),
                       w2 = (uint32_t)((((uint64_t)q.w << 32) | q.z) >> sh);
        // bytes 0..11 = (column 0: r g b) (column 1: r g b) ...
        v[0][k] = ra_cubic_bytes(w0 & 255u, (w0 >> 24) & 255u, (w1 >> 16) & 255u, (w2 >> 8) & 255u, dx);
        v[1][k] = ra_cubic_bytes((w0 >> 8) & 255u, w1 & 255u, (w1 >> 24) & 255u, (w2 >> 16) & 255u, dx);
        v[2][k] = ra_cubic_bytes((w0 >> 16) & 255u, (w1 >> 8) & 255u, w2 & 255u, (w2 >> 24) & 255u, dx);
      } else {
        const uint8_t* r = s + row;
#pragma unroll
        for (int c = 0; c < 3; c++) v[c][k] = ra_cubic_bytes(r[col[0] + c], r[col[1] + c], r[col[2] + c], r[col[3] + c], dx);
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; c++) v[c][k] = v[c][k - 1];
    }
  }
  uint32_t px = 0;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const double o = ra_cubic(v[c][0], v[c][1], v[c][2], v[c][3], dy);
    const uint32_t u = o <= 0.0 ? 0u : o >= 255.0 ? 255u : (uint32_t)(int)o;
    px |= u << (8 * c);
  }
  return px;
}

// One output pixel of Sharpness; the arguments of ra_affine_pixel.  The three taps of a row are nine consecutive bytes, read as the
// aligned words around them where those end inside the clip.
__device__ __forceinline__ uint32_t ra_sharp_pixel(const uint8_t* __restrict__ s, uint32_t frame, uint32_t clip_bytes, int H, int W,
                                                   int x, int y, float fct, bool convex) {
  const uint32_t at = frame + ((uint32_t)y * (uint32_t)W + (uint32_t)x) * 3u;
  const uint8_t* p = s + at;
  if (x == 0 || y == 0 || x == W - 1 || y == H - 1)     // the smoothing filter copies the border, and blending a value with itself keeps it
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
  const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
  const uint32_t rs = (uint32_t)W * 3u;
  // PIL's 3x3 filter: 0.5, then the three taps of a row summed among themselves and added, row after row, the row below first
  float ss[3] = {0.5f, 0.5f, 0.5f};
  int centre[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const uint32_t left = at + rs - (uint32_t)k * rs - 3u;      // rows y + 1, y, y - 1
    const float kc = k == 1 ? k5 : k1;
    uint32_t w0, w1, w2;
    if ((left & ~3u) + 16u <= clip_bytes) {
      const ra_u32x4_t q = *(const ra_u32x4_t*)(s + (left & ~3u));
      const uint32_t sh = (left & 3u) * 8u;
      w0 = (uint32_t)((((uint64_t)q.y << 32) | q.x) >> sh), w1 = (uint32_t)((((uint64_t)q.z << 32) | q.y) >> sh);
      w2 = (uint32_t)((((uint64_t)q.w << 32) | q.z) >> sh);
    } else {
      const uint8_t* r = s + left;
      w0 = (uint32_t)r[0] | ((uint32_t)r[1] << 8) | ((uint32_t)r[2] << 16) | ((uint32_t)r[3] << 24);
      w1 = (uint32_t)r[4] | ((uint32_t)r[5] << 8) | ((uint32_t)r[6] << 16) | ((uint32_t)r[7] << 24);
      w2 = r[8];
    }
    const uint32_t l[3] = {w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u};
    const uint32_t m[3] = {w0 >> 24, w1 & 255u, (w1 >> 8) & 255u};
    const uint32_t r3[3] = {(w1 >> 16) & 255u, w1 >> 24, w2 & 255u};
#pragma unroll
    for (int c = 0; c < 3; c++) {
      ss[c] += ((float)l[c] * k1 + (float)m[c] * kc) + (float)r3[c] * k1;
      if (k == 1) centre[c] = (int)m[c];
    }
  }
  uint32_t px = 0;
#pragma unroll
  for (int c = 0; c < 3; c++) px |= (uint32_t)ra_blend(ra_clip8(ss[c]), centre[c], fct, convex) << (8 * c);
  return px;
}

__global__ __launch_bounds__(256) void randaug_apply_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                            int64_t frames_bytes, const int64_t* __restrict__ desc,
                                                            const int32_t* __restrict__ ops, const double* __restrict__ args,
                                                            int L, int layer, int T, const uint8_t* __restrict__ tables,
                                                            uint32_t fill) {
  const int64_t b = blockIdx.y;
  int64_t off;
  int H, W;
  if (!ra_clip(desc, b, T, frames_bytes, off, H, W)) return;
  int op = ops ? ops[b * L + layer] : RA_NONE;
  if (op < RA_NONE || op > RA_TRANSLATE_Y) op = RA_NONE;
  const uint32_t HW = (uint32_t)H * (uint32_t)W, npix = (uint32_t)T * HW;   // 3 * npix <= frames_bytes < 2^31
  const uint8_t* s = src + off;
  uint8_t* d = dst + off;
  const uint32_t tid = blockIdx.x * 256u + threadIdx.x, stride = gridDim.x * 256u;

  if (op == RA_NONE) {
    const uint32_t nbytes = npix * 3u, nv = nbytes / 16u;
    for (uint32_t q = tid; q < nv; q += stride) ((u32x4_t*)d)[q] = ((const u32x4_t*)s)[q];
    const uint32_t i = nv * 16u + tid;
    if (i < nbytes) d[i] = s[i];
    return;
  }

  double a[RA_ARGS];
#pragma unroll
  for (int k = 0; k < RA_ARGS; k++) a[k] = args[(b * L + layer) * RA_ARGS + k];
  const float fct = (float)a[0];
  const bool convex = fct >= 0.f && fct <= 1.f;
  if (!ra_is_table(op) && op != RA_COLOR) {
    // Sharpness and the affine family read a neighbourhood: a wave takes a tile of 16 x 4 pixels, one pixel per lane, so that one
    // load instruction of the wave stays within a few rows of the source whichever way the frame is turned
    const uint32_t tx = ((uint32_t)W + 15u) / 16u, per_frame = tx * (((uint32_t)H + 3u) / 4u);
    const uint32_t ntiles = (uint32_t)T * per_frame;   // <= T * H * W
    const int lx = (int)(threadIdx.x & 15u), ly = (int)((threadIdx.x >> 4) & 3u);
    for (uint32_t u = tid >> 6; u < ntiles; u += stride >> 6) {
      const uint32_t t = u / per_frame, r = u - t * per_frame;
      const int x = (int)(r % tx) * 16 + lx, y = (int)(r / tx) * 4 + ly;
      if (x >= W || y >= H) continue;
      const uint32_t px = op == RA_SHARPNESS ? ra_sharp_pixel(s, t * HW * 3u, npix * 3u, H, W, x, y, fct, convex)
                                             : ra_affine_pixel(s, t * HW * 3u, npix * 3u, H, W, x, y, a, fill);
      uint8_t* o = d + (int64_t)t * HW * 3 + ((int64_t)y * W + x) * 3;
      o[0] = (uint8_t)px, o[1] = (uint8_t)(px >> 8), o[2] = (uint8_t)(px >> 16);
    }
    return;
  }

  // the operations that look at one pixel: four pixels, twelve bytes, per thread
  const uint8_t* tab0 = tables + b * T * RA_TABLE_BYTES;
  const uint32_t nchunk = (npix + 3u) / 4u;
  for (uint32_t q = tid; q < nchunk; q += stride) {
    const uint32_t p0 = q * 4u;
    const uint32_t cnt = npix - p0 < 4u ? npix - p0 : 4u;
    uint64_t lo = 0, hi = 0;   // pixels 0,1 and 2,3 of the chunk, 24 bits each
#pragma unroll 1
    for (uint32_t k = 0; k < cnt; k++) {
      const uint32_t p = p0 + k;
      const uint32_t t = p / HW, rem = p - t * HW;
      const uint8_t* u = s + (int64_t)t * HW * 3 + rem * 3u;
      uint32_t px;
      if (op != RA_COLOR) {
        const uint8_t* tab = tab0 + t * RA_TABLE_BYTES;
        px = (uint32_t)tab[u[0]] | ((uint32_t)tab[256 + u[1]] << 8) | ((uint32_t)tab[512 + u[2]] << 16);
      } else {
        const int r = u[0], g = u[1], bl = u[2];
        const int lum = ra_luma(r, g, bl);
        px = (uint32_t)ra_blend(lum, r, fct, convex) | ((uint32_t)ra_blend(lum, g, fct, convex) << 8) |
             ((uint32_t)ra_blend(lum, bl, fct, convex) << 16);
      }
      if (k < 2u) lo |= (uint64_t)px << (24u * k);
      else hi |= (uint64_t)px << (24u * (k - 2u));
    }
    const uint32_t w0 = (uint32_t)lo, w1 = (uint32_t)(lo >> 32) | ((uint32_t)hi << 16), w2 = (uint32_t)(hi >> 16);
    if (cnt == 4u) {
      uint32_t* o = (uint32_t*)(d + (int64_t)q * 12);
      o[0] = w0, o[1] = w1, o[2] = w2;
    } else {
      uint8_t* o = d + (int64_t)q * 12;
      for (uint32_t j = 0; j < cnt * 3u; j++) o[j] = (uint8_t)((j < 4u ? w0 >> (8u * j) : j < 8u ? w1 >> (8u * (j - 4u)) : w2 >> (8u * (j - 8u))) & 255u);
    }
  }
}

inline int64_t ra_align(int64_t v) { return (v + 255) / 256 * 256; }

}  // namespace

extern "C" int64_t vj_clip_randaug_ws_bytes(int64_t frames_bytes, int64_t B, int64_t T) {
  if (frames_bytes < 0 || B < 0 || T < 0) return -1;
  return ra_align(frames_bytes) + ra_align(B * T * RA_TABLE_BYTES);
}

// fill: the colour the affine family writes where the source has no pixel, packed as a pixel is (r | g << 8 | b << 16)
static int ra_run(uint8_t* frames, int64_t frames_bytes, const int64_t* desc, int64_t B, int64_t T, const int32_t* ops,
                  const double* args, int64_t L, void* ws, int64_t ws_bytes, uint32_t fill, hipStream_t stream) {
  VJ_CHECK_ARG(B >= 0 && B < 65536 && T > 0 && T < (1 << 20) && frames_bytes >= 0 && frames_bytes < (1ll << 31),
               "vj_clip_randaug: bad dims B=%ld T=%ld frames_bytes=%ld", (long)B, (long)T, (long)frames_bytes);
  VJ_CHECK_ARG(L >= 0 && L <= 8, "vj_clip_randaug: L=%ld layers, at most 8", (long)L);
  VJ_CHECK_ARG(B * T < (1ll << 31) / RA_TABLE_BYTES, "vj_clip_randaug: batch too large (B=%ld T=%ld)", (long)B, (long)T);
  if (B == 0 || L == 0 || frames_bytes == 0) return 0;
  VJ_CHECK_ARG(frames != nullptr && desc != nullptr && ops != nullptr && args != nullptr && ws != nullptr,
               "vj_clip_randaug: null pointer");
  VJ_CHECK_ARG((uintptr_t)frames % 16 == 0 && (uintptr_t)ws % 16 == 0 && (uintptr_t)args % 8 == 0,
               "vj_clip_randaug: frames and ws must be 16-byte aligned, args 8-byte aligned");
  VJ_CHECK_ARG(ws_bytes >= vj_clip_randaug_ws_bytes(frames_bytes, B, T), "vj_clip_randaug: workspace of %ld bytes, %ld needed",
               (long)ws_bytes, (long)vj_clip_randaug_ws_bytes(frames_bytes, B, T));
  uint8_t* copy = (uint8_t*)ws;
  uint8_t* tables = copy + ra_align(frames_bytes);
  int64_t gx = cdiv64(cdiv64(frames_bytes, 12), 256 * B);
  gx = gx < 1 ? 1 : gx > 2048 ? 2048 : gx;
  const dim3 grid((unsigned)gx, (unsigned)B);
  uint8_t* src = frames;
  uint8_t* dst = copy;
  for (int layer = 0; layer < (int)L; layer++) {
    hipLaunchKernelGGL(randaug_table_kernel, dim3((unsigned)(B * T)), dim3(512), 0, stream, src, frames_bytes, desc, ops, args, (int)L,
                       layer, (int)T, tables);
    hipLaunchKernelGGL(randaug_apply_kernel, grid, dim3(256), 0, stream, src, dst, frames_bytes, desc, ops, args, (int)L, layer, (int)T,
                       tables, fill);
    uint8_t* swap = src;
    src = dst, dst = swap;
  }
  if (src != frames)
    hipLaunchKernelGGL(randaug_apply_kernel, grid, dim3(256), 0, stream, src, frames, frames_bytes, desc, (const int32_t*)nullptr, args,
                       (int)L, 0, (int)T, tables, fill);
  VJ_LAUNCH_CHECK("vj_clip_randaug");
  return 0;
}

extern "C" int vj_clip_randaug(uint8_t* frames, int64_t frames_bytes, const int64_t* desc, int64_t B, int64_t T,
                               const int32_t* ops, const double* args, int64_t L, void* ws, int64_t ws_bytes, hipStream_t stream) {
  return ra_run(frames, frames_bytes, desc, B, T, ops, args, L, ws, ws_bytes, 0x808080u, stream);   // the reference's video _FILL
}

extern "C" int vj_clip_randaug_fill(uint8_t* frames, int64_t frames_bytes, const int64_t* desc, int64_t B, int64_t T,
                                    const int32_t* ops, const double* args, int64_t L, void* ws, int64_t ws_bytes, int fill_r,
                                    int fill_g, int fill_b, hipStream_t stream) {
  VJ_CHECK_ARG(fill_r >= 0 && fill_r <= 255 && fill_g >= 0 && fill_g <= 255 && fill_b >= 0 && fill_b <= 255,
               "vj_clip_randaug_fill: fill colour (%d, %d, %d), bytes are taken", fill_r, fill_g, fill_b);
  return ra_run(frames, frames_bytes, desc, B, T, ops, args, L, ws, ws_bytes,
                (uint32_t)fill_r | ((uint32_t)fill_g << 8) | ((uint32_t)fill_b << 16), stream);
}
