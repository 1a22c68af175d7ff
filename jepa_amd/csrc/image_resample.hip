// PIL's antialiased two-pass resample on decoded uint8 images: crop box -> OH x OW -> an S x S window of it, byte for byte what
// Image.crop(box).resize((OW, OH), BILINEAR | BICUBIC) gives on 8-bit RGB.  The input edge of the image evals:
//   reference's loader factory (timm create_transform / torchvision Resize + CenterCrop)   evals/image_classification_frozen/eval.py:379-423
// Behaviour restated, never copied.  The draws stay on the host (jepa_amd/evals/image_classification_frozen/transforms.py); the output
// is a buffer of one-frame S x S clips that vj_clip_transform_pre reads next (ToTensor + Normalize + flip).
//
// The arithmetic, per axis with source extent n (the crop's) and resize extent m, everything fp64:
//   scale = n / m;  fs = max(scale, 1);  support = filter_support * fs                      (bilinear 1, bicubic 2 with a = -0.5)
//   output index x:  center = (x + 0.5) * scale;  lo = max(int(center - support + 0.5), 0);  hi = min(int(center + support + 0.5), n)
//   tap t in [lo, hi):  w_t = f((t - center + 0.5) / fs), summed in ascending order; divided by the sum when that is not zero;
//   coefficient = int(0.5 + w * 2^22) for w >= 0, int(-0.5 + w * 2^22) below (truncation)
// A pass accumulates 2^21 + sum pixel * coefficient in int32, shifts right by 22 arithmetically and clamps to 0..255.  The
// horizontal pass runs first and its uint8 result is what the vertical pass reads: that rounding and clamping are part of the bytes.
//
// THIS FILE IS BUILT WITH FLOATING-POINT CONTRACTION OFF (jepa_amd/build.py EXTRA_FLAGS), as clip_randaug.hip is: a fused
// multiply-add in the filter or the centre moves a coefficient across its truncation.
//
// Three launches:
//   resample_coeff_kernel   one thread per (image, axis, window index): bounds (lo, count) and the int32 coefficients of its taps
//   resample_h_kernel       one thread per (needed source row, window column): uint8 intermediate [B, rows, S, 3]
//   resample_v_kernel       one thread per four bytes of an output row (S % 4 == 0; the vertical pass does not mix channels)
// Tap loops are bounded at run time by the table's counts, which are clamped to the capacities the workspace was sized for
// (taps_x, taps_y, rows: maxima over the batch, computed by the caller from the geometry it validated).  Every kernel re-derives
// from desc / geom whether the image lies inside the buffer, the box inside the image, the window inside the resize and the needs
// inside the capacities; an image that fails is written as zeros, and every source index is clamped into the crop, so nothing
// outside [frames, frames + frames_bytes), the workspace and the output is touched whatever the tables say.  The frame buffer is
// only read: the padding between images stays as it is.
//
// The second half of the file is the same resample for clips (vj_clip_resample): whole frames, one table per clip, rows of any
// length.  The table entry (rs_axis_entry) and the bodies of the two passes (rs_hpixel, rs_vword) are shared by both halves.
#include "common.hpp"
#include "../../include/vjepa_hip.h"

namespace {

constexpr int RS_BILINEAR = 0, RS_BICUBIC = 1;
constexpr int RS_PRECISION_BITS = 22;        // 32 - 8 - 2
constexpr int RS_MAX_SIDE = 1 << 15;

struct RsImage {
  const uint8_t* src;   // the image's first byte
  int Ws;               // its row length in pixels
  int i, j, h, w;       // crop box
  int OH, OW, wy, wx;   // resize extent and the window's corner
};

__host__ __device__ __forceinline__ double rs_support(int filter) { return filter == RS_BICUBIC ? 2.0 : 1.0; }

// taps one output index of an axis can have at most: int(ceil(support)) * 2 + 1
__host__ __device__ __forceinline__ int rs_ksize(int n, int m, int filter) {
  const double scale = (double)n / (double)m;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = rs_support(filter) * fs;
  return (int)ceil(support) * 2 + 1;
}

// descriptor and geometry row b -> the image; false: the image is written as zeros
__device__ __forceinline__ bool rs_image(const uint8_t* __restrict__ frames, int64_t frames_bytes, const int64_t* __restrict__ desc,
                                         const int32_t* __restrict__ geom, int64_t b, int S, int filter, int taps_x, int taps_y,
                                         RsImage& im) {
  const int64_t off = desc[b * 4 + 0], Hs = desc[b * 4 + 1], Ws = desc[b * 4 + 2];
  if (off < 0 || (off & 15) != 0 || off > frames_bytes || Hs <= 0 || Ws <= 0 || Hs >= RS_MAX_SIDE || Ws >= RS_MAX_SIDE) return false;
  if (Hs * Ws * 3 > frames_bytes - off) return false;
  const int32_t* g = geom + b * 8;
  im.i = g[0], im.j = g[1], im.h = g[2], im.w = g[3], im.OH = g[4], im.OW = g[5], im.wy = g[6], im.wx = g[7];
  if (im.i < 0 || im.j < 0 || im.h <= 0 || im.w <= 0 || (int64_t)im.i + im.h > Hs || (int64_t)im.j + im.w > Ws) return false;
  if (im.OH <= 0 || im.OW <= 0 || im.OH >= RS_MAX_SIDE || im.OW >= RS_MAX_SIDE) return false;
  if (im.wy < 0 || im.wx < 0 || (int64_t)im.wy + S > im.OH || (int64_t)im.wx + S > im.OW) return false;
  if (rs_ksize(im.w, im.OW, filter) > taps_x || rs_ksize(im.h, im.OH, filter) > taps_y) return false;
  im.src = frames + off;
  im.Ws = (int)Ws;
  return true;
}

__device__ __forceinline__ double rs_filter(double u, int filter) {
  if (u < 0.0) u = -u;
  if (filter == RS_BICUBIC) {
    const double a = -0.5;
    if (u < 1.0) return ((a + 2.0) * u - (a + 3.0)) * u * u + 1.0;
    if (u < 2.0) return (((u - 5.0) * u + 8.0) * u - 4.0) * a;
    return 0.0;
  }
  return u < 1.0 ? 1.0 - u : 0.0;
}

// The shifted value is made opaque before the clamp.  Left to itself hipcc fuses shift, clamp and the packing of two results into
// v_ashr_pk_u8_i32, which writes the low 16 bits of its destination only, and then ORs that register -- its upper half still the old
// accumulator -- into the packed word as if it had been zero-extended: bytes 2 and 3 of every word came out wrong on the device.
__device__ __forceinline__ int rs_clip8(int acc) {
  int v = acc >> RS_PRECISION_BITS;
  asm("" : "+v"(v));
  return v < 0 ? 0 : v > 255 ? 255 : v;
}

// Bounds (lo, count) and the 22-bit coefficients of output index xo of an axis that takes n source samples to m: the table entry of
// the image kernels and of the clip kernels alike.
__device__ __forceinline__ void rs_axis_entry(int n, int m, int xo, int filter, int cap, int32_t* __restrict__ k,
                                              int32_t* __restrict__ bd) {
  const double scale = (double)n / (double)m;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = rs_support(filter) * fs;
  const double center = ((double)xo + 0.5) * scale;
  int lo = (int)(center - support + 0.5);
  if (lo < 0) lo = 0;
  int hi = (int)(center + support + 0.5);
  if (hi > n) hi = n;
  // what follows cannot happen for a geometry that passed rs_image / rs_clip; the clamps keep the passes inside the crop and the tables
  if (lo > n - 1) lo = n - 1;
  int cnt = hi - lo;
  if (cnt < 0) cnt = 0;
  if (cnt > cap) cnt = cap;
  double ww = 0.0;
  for (int t = 0; t < cnt; t++) ww += rs_filter(((double)(t + lo) - center + 0.5) / fs, filter);
  for (int t = 0; t < cnt; t++) {
    double w = rs_filter(((double)(t + lo) - center + 0.5) / fs, filter);
    if (ww != 0.0) w = w / ww;
    const double scaled = w * (double)(1 << RS_PRECISION_BITS);
    k[t] = w < 0.0 ? (int)(-0.5 + scaled) : (int)(0.5 + scaled);
  }
  bd[0] = lo, bd[1] = cnt;
}

// One pixel of the horizontal pass: cnt taps of interleaved RGB at p.
__device__ __forceinline__ void rs_hpixel(const uint8_t* __restrict__ p, const int32_t* __restrict__ k, int cnt,
                                          uint8_t* __restrict__ o) {
  int a0 = 1 << (RS_PRECISION_BITS - 1), a1 = a0, a2 = a0;
  for (int t = 0; t < cnt; t++) {
    const int c = k[t];
    a0 += p[3 * t + 0] * c;
    a1 += p[3 * t + 1] * c;
    a2 += p[3 * t + 2] * c;
  }
  o[0] = (uint8_t)rs_clip8(a0);
  o[1] = (uint8_t)rs_clip8(a1);
  o[2] = (uint8_t)rs_clip8(a2);
}

// Four bytes of a row of the vertical pass (it does not mix channels): word(t) is the four intermediate bytes under tap t.
template <class Word>
__device__ __forceinline__ uint32_t rs_vword(Word word, const int32_t* __restrict__ k, int cnt) {
  int a0 = 1 << (RS_PRECISION_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
  for (int t = 0; t < cnt; t++) {
    const int c = k[t];
    const uint32_t v = word(t);
    a0 += (int)(v & 255u) * c;
    a1 += (int)((v >> 8) & 255u) * c;
    a2 += (int)((v >> 16) & 255u) * c;
    a3 += (int)(v >> 24) * c;
  }
  return (uint32_t)rs_clip8(a0) | ((uint32_t)rs_clip8(a1) << 8) | ((uint32_t)rs_clip8(a2) << 16) | ((uint32_t)rs_clip8(a3) << 24);
}

// Workspace: bounds int32 [B][2][S][2] = (lo, count), axis 0 = x; coefficients int32 [B][S][taps_x] then [B][S][taps_y]; then the
// intermediate uint8 [B][rows][S][3].  Every part starts on a 256-byte boundary.
inline int64_t rs_align(int64_t v) { return (v + 255) / 256 * 256; }
inline int64_t rs_bounds_bytes(int64_t B, int64_t S) { return rs_align(B * 2 * S * 2 * 4); }
inline int64_t rs_coeff_bytes(int64_t B, int64_t S, int64_t taps) { return rs_align(B * S * taps * 4); }
inline int64_t rs_tmp_bytes(int64_t B, int64_t S, int64_t rows) { return rs_align(B * rows * S * 3); }

// ---------------------------------------------------------------------------------------------
// bounds and coefficients of (image, axis, window index)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void resample_coeff_kernel(const uint8_t* __restrict__ frames, int64_t frames_bytes,
                                                             const int64_t* __restrict__ desc, const int32_t* __restrict__ geom,
                                                             int S, int filter, int taps_x, int taps_y, int32_t* __restrict__ bounds,
                                                             int32_t* __restrict__ coeff_x, int32_t* __restrict__ coeff_y) {
  const int64_t b = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2 * S) return;
  const int axis = idx / S, x = idx - axis * S;
  int32_t* bd = bounds + ((b * 2 + axis) * S + x) * 2;
  RsImage im;
  if (!rs_image(frames, frames_bytes, desc, geom, b, S, filter, taps_x, taps_y, im)) {
    bd[0] = 0, bd[1] = 0;
    return;
  }
  const int n = axis == 0 ? im.w : im.h, m = axis == 0 ? im.OW : im.OH;
  const int xo = (axis == 0 ? im.wx : im.wy) + x;          // index in the resized image
  const int cap = axis == 0 ? taps_x : taps_y;
  int32_t* k = axis == 0 ? coeff_x + (b * S + x) * taps_x : coeff_y + (b * S + x) * taps_y;

  rs_axis_entry(n, m, xo, filter, cap, k, bd);
}

// first source row (relative to the crop) that the window's vertical taps read, and how many rows they span
__device__ __forceinline__ void rs_rows(const int32_t* __restrict__ bounds, int64_t b, int S, int h, int& row0, int& nrows) {
  const int32_t* by = bounds + (b * 2 + 1) * S * 2;
  row0 = by[0];
  nrows = by[(S - 1) * 2] + by[(S - 1) * 2 + 1] - row0;
  if (row0 < 0) row0 = 0;
  if (row0 > h) row0 = h;
  if (nrows < 0) nrows = 0;
  if (nrows > h - row0) nrows = h - row0;
}

// ---------------------------------------------------------------------------------------------
// horizontal pass: tmp[b][r][x][c], r < nrows of image b
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void resample_h_kernel(const uint8_t* __restrict__ frames, int64_t frames_bytes,
                                                         const int64_t* __restrict__ desc, const int32_t* __restrict__ geom, int S,
                                                         int filter, int taps_x, int taps_y, int rows,
                                                         const int32_t* __restrict__ bounds, const int32_t* __restrict__ coeff_x,
                                                         uint8_t* __restrict__ tmp) {
  const int64_t b = blockIdx.y;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)rows * S) return;
  const int r = (int)(idx / S), x = (int)(idx - (int64_t)r * S);
  RsImage im;
  if (!rs_image(frames, frames_bytes, desc, geom, b, S, filter, taps_x, taps_y, im)) return;
  int row0, nrows;
  rs_rows(bounds, b, S, im.h, row0, nrows);
  if (r >= nrows) return;
  const int32_t* bd = bounds + ((b * 2 + 0) * S + x) * 2;
  int lo = bd[0], cnt = bd[1];
  lo = lo < 0 ? 0 : lo > im.w - 1 ? im.w - 1 : lo;
  cnt = cnt < 0 ? 0 : cnt > taps_x ? taps_x : cnt;
  if (cnt > im.w - lo) cnt = im.w - lo;
  const int32_t* k = coeff_x + (b * S + x) * taps_x;
  const uint8_t* p = im.src + ((int64_t)(im.i + row0 + r) * im.Ws + im.j + lo) * 3;
  rs_hpixel(p, k, cnt, tmp + (((int64_t)b * rows + r) * S + x) * 3);
}

// ---------------------------------------------------------------------------------------------
// vertical pass: out[b][y][x][c], four bytes of a row per thread
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void resample_v_kernel(const uint8_t* __restrict__ frames, int64_t frames_bytes,
                                                         const int64_t* __restrict__ desc, const int32_t* __restrict__ geom, int S,
                                                         int filter, int taps_x, int taps_y, int rows,
                                                         const int32_t* __restrict__ bounds, const int32_t* __restrict__ coeff_y,
                                                         const uint8_t* __restrict__ tmp, uint8_t* __restrict__ out) {
  const int64_t b = blockIdx.y;
  const int words = S * 3 / 4;                                  // S % 4 == 0
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)S * words) return;
  const int y = (int)(idx / words), q = (int)(idx - (int64_t)y * words);
  uint32_t* o = (uint32_t*)(out + (((int64_t)b * S + y) * S) * 3) + q;
  RsImage im;
  if (!rs_image(frames, frames_bytes, desc, geom, b, S, filter, taps_x, taps_y, im)) {
    *o = 0u;
    return;
  }
  int row0, nrows;
  rs_rows(bounds, b, S, im.h, row0, nrows);
  if (nrows > rows) {                                           // the intermediate was sized for fewer rows than this image needs
    *o = 0u;
    return;
  }
  const int32_t* bd = bounds + ((b * 2 + 1) * S + y) * 2;
  int lo = bd[0] - row0, cnt = bd[1];
  lo = lo < 0 ? 0 : lo;
  cnt = cnt < 0 ? 0 : cnt > taps_y ? taps_y : cnt;
  if (cnt > nrows - lo) cnt = nrows - lo;                       // negative: no tap
  const int32_t* k = coeff_y + (b * S + y) * taps_y;
  const uint32_t* p = (const uint32_t*)(tmp + (((int64_t)b * rows + lo) * S) * 3) + q;
  *o = rs_vword([&](int t) { return p[(int64_t)t * words]; }, k, cnt);
}

// =============================================================================================
// Clips: Image.resize((OW, OH)) of every frame of a clip, whole frames, into a second frame buffer
// =============================================================================================
// The validation transforms of the video evals resize every frame to the reference's short side and crop their views from the
// result (evals/video_classification_frozen/utils.py:217-223, 297-321).  A clip differs from the images above in three ways: the
// output is the whole OH x OW rectangle, the T frames of a clip share one table entry per (axis, output index), and the row length
// OW * 3 is arbitrary -- only the clip starts on a 16-byte boundary.  The table entry and the two pass bodies are the ones above.
//
// Workspace: bounds int32 [B][ow][2] and [B][oh][2]; coefficients int32 [B][ow][taps_x] and [B][oh][taps_y]; the intermediate
// uint8 [B][T][rows][pitch] with pitch = ow * 3 rounded up to four, plus four: a row starts on a word, and the word after a row's
// last one can be read.  oh, ow, rows are capacities like the taps: maxima over the batch of OH, OW and the source height.
struct RsClipArgs {
  const uint8_t* frames;
  int64_t frames_bytes;
  const int64_t* desc;
  const int32_t* rgeom;
  const int64_t* desc_out;
  uint8_t* out;
  int64_t out_bytes;
  int T, filter, oh, ow, taps_x, taps_y, rows, pitch;
  int32_t *bounds_x, *bounds_y, *coeff_x, *coeff_y;
  uint8_t* tmp;
};

struct RsClip {
  const uint8_t* src;   // the first byte of the clip's first frame
  uint8_t* dst;         // the first byte of the resized clip
  int Hs, Ws, OH, OW;
};

inline int64_t rs_clip_pitch(int64_t ow) { return (ow * 3 + 3) / 4 * 4 + 4; }

// The bytes of `out` that row b of desc_out names, cut at the end of `out`: [out + off, out + off + n).  n == 0: the row names nothing
// that may be written.  This is all a clip that fails rs_clip is allowed to touch (it is zeroed).
__device__ __forceinline__ int64_t rs_clip_range(const RsClipArgs& a, int64_t b, int64_t& off) {
  off = a.desc_out[b * 4 + 0];
  const int64_t OH = a.desc_out[b * 4 + 1], OW = a.desc_out[b * 4 + 2];
  if (off < 0 || (off & 15) != 0 || off >= a.out_bytes || OH <= 0 || OW <= 0 || OH >= RS_MAX_SIDE || OW >= RS_MAX_SIDE) return 0;
  const int64_t n = (int64_t)a.T * OH * OW * 3, room = a.out_bytes - off;
  return n < room ? n : room;
}

// rows b of desc, rgeom and desc_out -> the clip; false: the clip is written as zeros
__device__ __forceinline__ bool rs_clip(const RsClipArgs& a, int64_t b, RsClip& c) {
  const int64_t off = a.desc[b * 4 + 0], Hs = a.desc[b * 4 + 1], Ws = a.desc[b * 4 + 2];
  if (off < 0 || (off & 15) != 0 || off > a.frames_bytes || Hs <= 0 || Ws <= 0 || Hs >= RS_MAX_SIDE || Ws >= RS_MAX_SIDE) return false;
  if ((int64_t)a.T * Hs * Ws * 3 > a.frames_bytes - off) return false;
  const int64_t OH = a.rgeom[b * 2 + 0], OW = a.rgeom[b * 2 + 1];
  if (OH <= 0 || OW <= 0 || OH >= RS_MAX_SIDE || OW >= RS_MAX_SIDE) return false;
  if (OH > a.oh || OW > a.ow || Hs > a.rows) return false;
  const int64_t doff = a.desc_out[b * 4 + 0];
  if (a.desc_out[b * 4 + 1] != OH || a.desc_out[b * 4 + 2] != OW) return false;
  if (doff < 0 || (doff & 15) != 0 || doff > a.out_bytes || (int64_t)a.T * OH * OW * 3 > a.out_bytes - doff) return false;
  if (rs_ksize((int)Ws, (int)OW, a.filter) > a.taps_x || rs_ksize((int)Hs, (int)OH, a.filter) > a.taps_y) return false;
  c.src = a.frames + off;
  c.dst = a.out + doff;
  c.Hs = (int)Hs, c.Ws = (int)Ws, c.OH = (int)OH, c.OW = (int)OW;
  return true;
}

// ---------------------------------------------------------------------------------------------
// bounds and coefficients of (clip, axis, output index): once per clip, read by all its frames
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clip_resample_coeff_kernel(RsClipArgs a) {
  const int64_t b = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.ow + a.oh) return;
  const int axis = idx < a.ow ? 0 : 1, x = axis == 0 ? idx : idx - a.ow;
  int32_t* bd = axis == 0 ? a.bounds_x + (b * a.ow + x) * 2 : a.bounds_y + (b * a.oh + x) * 2;
  RsClip c = {};
  const bool ok = rs_clip(a, b, c);
  const int n = axis == 0 ? c.Ws : c.Hs, m = axis == 0 ? c.OW : c.OH;
  if (!ok || x >= m) {                                          // entries past the clip's own extent are never read
    bd[0] = 0, bd[1] = 0;
    return;
  }
  int32_t* k = axis == 0 ? a.coeff_x + (b * a.ow + x) * a.taps_x : a.coeff_y + (b * a.oh + x) * a.taps_y;
  rs_axis_entry(n, m, x, a.filter, axis == 0 ? a.taps_x : a.taps_y, k, bd);
}

// ---------------------------------------------------------------------------------------------
// horizontal pass: tmp[b][t][r][x][c] for every source row r of frame t
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clip_resample_h_kernel(RsClipArgs a) {
  const int64_t b = blockIdx.z;
  const int t = blockIdx.y;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  RsClip c;
  if (!rs_clip(a, b, c)) return;
  if (idx >= (int64_t)c.Hs * c.OW) return;                      // Hs <= rows and OW <= ow: the grid covers it
  const int r = (int)(idx / c.OW), x = (int)(idx - (int64_t)r * c.OW);
  const int32_t* bd = a.bounds_x + (b * a.ow + x) * 2;
  int lo = bd[0], cnt = bd[1];
  lo = lo < 0 ? 0 : lo > c.Ws - 1 ? c.Ws - 1 : lo;
  cnt = cnt < 0 ? 0 : cnt > a.taps_x ? a.taps_x : cnt;
  if (cnt > c.Ws - lo) cnt = c.Ws - lo;
  const int32_t* k = a.coeff_x + (b * a.ow + x) * a.taps_x;
  const uint8_t* p = c.src + (((int64_t)t * c.Hs + r) * c.Ws + lo) * 3;
  rs_hpixel(p, k, cnt, a.tmp + ((b * a.T + t) * a.rows + r) * a.pitch + x * 3);
}

// ---------------------------------------------------------------------------------------------
// vertical pass: out[t][y][x][c] of the clip.  A row of OW * 3 bytes starts anywhere; it is cut into the bytes in front of its first
// word boundary (thread 0 of the row), its aligned words (one thread each, one 4-byte store) and the bytes behind the last whole
// word.  The intermediate is read in aligned words too: the four bytes under an output word are shifted out of two of them.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clip_resample_v_kernel(RsClipArgs a) {
  const int64_t b = blockIdx.z;
  const int t = blockIdx.y;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  RsClip c;
  if (!rs_clip(a, b, c)) {
    // zeros over what desc_out names inside `out`, by all threads the clip has, in words (the range starts on a 16-byte boundary)
    int64_t off;
    const int64_t n = rs_clip_range(a, b, off);
    const int64_t G = (int64_t)gridDim.x * gridDim.y * 256, g = ((int64_t)t * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
    uint8_t* d = a.out + off;
    for (int64_t i = g * 4; i < n; i += G * 4) {
      if (i + 4 <= n) {
        *(uint32_t*)(d + i) = 0u;
      } else {
        for (int64_t j = i; j < n; j++) d[j] = 0;
      }
    }
    return;
  }
  const int L = c.OW * 3, nq = 2 + L / 4;                       // nq <= 2 + ow * 3 / 4, OH <= oh: the grid covers it
  if (idx >= (int64_t)c.OH * nq) return;
  const int y = (int)(idx / nq), q = (int)(idx - (int64_t)y * nq);
  const int64_t row = ((int64_t)t * c.OH + y) * L;              // the clip starts on a 16-byte boundary
  int head = (int)((4 - (row & 3)) & 3);
  if (head > L) head = L;
  const int x0 = q == 0 ? 0 : head + 4 * (q - 1);
  const int x1 = q == 0 ? head : (x0 + 4 < L ? x0 + 4 : L);
  if (x0 >= x1) return;
  const int32_t* bd = a.bounds_y + (b * a.oh + y) * 2;
  int lo = bd[0], cnt = bd[1];
  lo = lo < 0 ? 0 : lo > c.Hs - 1 ? c.Hs - 1 : lo;
  cnt = cnt < 0 ? 0 : cnt > a.taps_y ? a.taps_y : cnt;
  if (cnt > c.Hs - lo) cnt = c.Hs - lo;
  const int32_t* k = a.coeff_y + (b * a.oh + y) * a.taps_y;
  const uint32_t* p = (const uint32_t*)(a.tmp + ((b * a.T + t) * a.rows + lo) * a.pitch) + (x0 >> 2);
  const int words = a.pitch / 4, shift = (x0 & 3) * 8;
  const uint32_t v = rs_vword(
      [&](int tap) {
        const uint32_t* w = p + (int64_t)tap * words;
        return (uint32_t)((((uint64_t)w[1] << 32) | w[0]) >> shift);
      },
      k, cnt);
  uint8_t* o = c.dst + row + x0;
  if (x1 - x0 == 4) {
    *(uint32_t*)o = v;                                          // q >= 1: row + head is a multiple of four
  } else {
    for (int i = 0; i < x1 - x0; i++) o[i] = (uint8_t)(v >> (8 * i));
  }
}

}  // namespace

static bool rs_clip_caps_ok(int64_t B, int64_t T, int64_t oh, int64_t ow, int64_t taps_x, int64_t taps_y, int64_t rows) {
  return B >= 0 && B < 65536 && T > 0 && T < 65536 && oh > 0 && oh < RS_MAX_SIDE && ow > 0 && ow < RS_MAX_SIDE && taps_x > 0 &&
         taps_y > 0 && taps_x <= 2 * RS_MAX_SIDE && taps_y <= 2 * RS_MAX_SIDE && rows > 0 && rows < RS_MAX_SIDE;
}

extern "C" int64_t vj_clip_resample_ws_bytes(int64_t B, int64_t T, int64_t oh, int64_t ow, int64_t taps_x, int64_t taps_y,
                                             int64_t rows) {
  if (!rs_clip_caps_ok(B, T, oh, ow, taps_x, taps_y, rows)) return -1;
  return rs_align(B * ow * 8) + rs_align(B * oh * 8) + rs_align(B * ow * taps_x * 4) + rs_align(B * oh * taps_y * 4) +
         rs_align(B * T * rows * rs_clip_pitch(ow));
}

extern "C" int vj_clip_resample(const uint8_t* frames, int64_t frames_bytes, const int64_t* desc, const int32_t* rgeom, uint8_t* out,
                                int64_t out_bytes, const int64_t* desc_out, int64_t B, int64_t T, int filter, int64_t oh, int64_t ow,
                                int64_t taps_x, int64_t taps_y, int64_t rows, void* ws, int64_t ws_bytes, hipStream_t stream) {
  VJ_CHECK_ARG(frames_bytes >= 0 && frames_bytes < (1ll << 40) && out_bytes >= 0 && out_bytes < (1ll << 40),
               "vj_clip_resample: bad sizes frames_bytes=%ld out_bytes=%ld", (long)frames_bytes, (long)out_bytes);
  VJ_CHECK_ARG(filter == RS_BILINEAR || filter == RS_BICUBIC, "vj_clip_resample: filter=%d (0 bilinear, 1 bicubic)", filter);
  VJ_CHECK_ARG(rs_clip_caps_ok(B, T, oh, ow, taps_x, taps_y, rows),
               "vj_clip_resample: bad dims or capacities B=%ld T=%ld oh=%ld ow=%ld taps_x=%ld taps_y=%ld rows=%ld", (long)B, (long)T,
               (long)oh, (long)ow, (long)taps_x, (long)taps_y, (long)rows);
  if (B == 0) return 0;
  const int64_t need = vj_clip_resample_ws_bytes(B, T, oh, ow, taps_x, taps_y, rows);
  VJ_CHECK_ARG(need < (1ll << 40), "vj_clip_resample: workspace of %ld bytes", (long)need);
  VJ_CHECK_ARG(frames != nullptr && desc != nullptr && rgeom != nullptr && out != nullptr && desc_out != nullptr && ws != nullptr,
               "vj_clip_resample: null pointer");
  VJ_CHECK_ARG((uintptr_t)frames % 16 == 0 && (uintptr_t)ws % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)rgeom % 4 == 0 &&
                   (uintptr_t)desc % 8 == 0 && (uintptr_t)desc_out % 8 == 0,
               "vj_clip_resample: frames, out and ws must be 16-byte aligned, desc and desc_out 8-byte, rgeom 4-byte");
  VJ_CHECK_ARG(ws_bytes >= need, "vj_clip_resample: workspace of %ld bytes, %ld needed", (long)ws_bytes, (long)need);
  RsClipArgs a;
  a.frames = frames, a.frames_bytes = frames_bytes, a.desc = desc, a.rgeom = rgeom, a.desc_out = desc_out;
  a.out = out, a.out_bytes = out_bytes;
  a.T = (int)T, a.filter = filter, a.oh = (int)oh, a.ow = (int)ow, a.taps_x = (int)taps_x, a.taps_y = (int)taps_y;
  a.rows = (int)rows, a.pitch = (int)rs_clip_pitch(ow);
  uint8_t* p = (uint8_t*)ws;
  a.bounds_x = (int32_t*)p, p += rs_align(B * ow * 8);
  a.bounds_y = (int32_t*)p, p += rs_align(B * oh * 8);
  a.coeff_x = (int32_t*)p, p += rs_align(B * ow * taps_x * 4);
  a.coeff_y = (int32_t*)p, p += rs_align(B * oh * taps_y * 4);
  a.tmp = p;
  const int64_t nq = 2 + ow * 3 / 4;
  hipLaunchKernelGGL(clip_resample_coeff_kernel, dim3((unsigned)cdiv64(oh + ow, 256), (unsigned)B), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(clip_resample_h_kernel, dim3((unsigned)cdiv64(rows * ow, 256), (unsigned)T, (unsigned)B), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(clip_resample_v_kernel, dim3((unsigned)cdiv64(oh * nq, 256), (unsigned)T, (unsigned)B), dim3(256), 0, stream, a);
  VJ_LAUNCH_CHECK("vj_clip_resample");
  return 0;
}

extern "C" int64_t vj_image_resample_ws_bytes(int64_t B, int64_t S, int64_t taps_x, int64_t taps_y, int64_t rows) {
  if (B < 0 || B >= 65536 || S <= 0 || S >= RS_MAX_SIDE || taps_x <= 0 || taps_y <= 0 || rows <= 0 || taps_x > 2 * RS_MAX_SIDE ||
      taps_y > 2 * RS_MAX_SIDE || rows >= RS_MAX_SIDE)
    return -1;
  return rs_bounds_bytes(B, S) + rs_coeff_bytes(B, S, taps_x) + rs_coeff_bytes(B, S, taps_y) + rs_tmp_bytes(B, S, rows);
}

extern "C" int vj_image_resample(const uint8_t* frames, int64_t frames_bytes, const int64_t* desc, const int32_t* geom, uint8_t* out,
                                 int64_t B, int64_t S, int filter, int64_t taps_x, int64_t taps_y, int64_t rows, void* ws,
                                 int64_t ws_bytes, hipStream_t stream) {
  VJ_CHECK_ARG(B >= 0 && B < 65536 && S > 0 && S < RS_MAX_SIDE && frames_bytes >= 0 && frames_bytes < (1ll << 40),
               "vj_image_resample: bad dims B=%ld S=%ld frames_bytes=%ld", (long)B, (long)S, (long)frames_bytes);
  VJ_CHECK_ARG(S % 4 == 0, "vj_image_resample: S=%ld must be a multiple of 4", (long)S);
  VJ_CHECK_ARG(filter == RS_BILINEAR || filter == RS_BICUBIC, "vj_image_resample: filter=%d (0 bilinear, 1 bicubic)", filter);
  VJ_CHECK_ARG(taps_x > 0 && taps_y > 0 && rows > 0 && taps_x <= 2 * RS_MAX_SIDE && taps_y <= 2 * RS_MAX_SIDE && rows < RS_MAX_SIDE,
               "vj_image_resample: bad capacities taps_x=%ld taps_y=%ld rows=%ld", (long)taps_x, (long)taps_y, (long)rows);
  if (B == 0) return 0;
  const int64_t need = vj_image_resample_ws_bytes(B, S, taps_x, taps_y, rows);
  VJ_CHECK_ARG(need < (1ll << 40), "vj_image_resample: workspace of %ld bytes", (long)need);
  VJ_CHECK_ARG(frames != nullptr && desc != nullptr && geom != nullptr && out != nullptr && ws != nullptr,
               "vj_image_resample: null pointer");
  VJ_CHECK_ARG((uintptr_t)frames % 16 == 0 && (uintptr_t)ws % 16 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)geom % 4 == 0 &&
                   (uintptr_t)desc % 8 == 0,
               "vj_image_resample: frames and ws must be 16-byte aligned, desc 8-byte, out and geom 4-byte");
  VJ_CHECK_ARG(ws_bytes >= need, "vj_image_resample: workspace of %ld bytes, %ld needed", (long)ws_bytes, (long)need);
  int32_t* bounds = (int32_t*)ws;
  int32_t* coeff_x = (int32_t*)((uint8_t*)ws + rs_bounds_bytes(B, S));
  int32_t* coeff_y = (int32_t*)((uint8_t*)coeff_x + rs_coeff_bytes(B, S, taps_x));
  uint8_t* tmp = (uint8_t*)coeff_y + rs_coeff_bytes(B, S, taps_y);
  const int s = (int)S, tx = (int)taps_x, ty = (int)taps_y, nr = (int)rows;
  hipLaunchKernelGGL(resample_coeff_kernel, dim3((unsigned)cdiv64(2 * S, 256), (unsigned)B), dim3(256), 0, stream, frames, frames_bytes,
                     desc, geom, s, filter, tx, ty, bounds, coeff_x, coeff_y);
  hipLaunchKernelGGL(resample_h_kernel, dim3((unsigned)cdiv64(rows * S, 256), (unsigned)B), dim3(256), 0, stream, frames, frames_bytes,
                     desc, geom, s, filter, tx, ty, nr, bounds, coeff_x, tmp);
  hipLaunchKernelGGL(resample_v_kernel, dim3((unsigned)cdiv64(S * (S * 3 / 4), 256), (unsigned)B), dim3(256), 0, stream, frames,
                     frames_bytes, desc, geom, s, filter, tx, ty, nr, bounds, coeff_y, tmp, out);
  VJ_LAUNCH_CHECK("vj_image_resample");
  return 0;
}
