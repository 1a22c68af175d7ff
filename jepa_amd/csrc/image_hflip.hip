// Horizontal flip, in place, of the flagged images of the uint8 [B,S,S,3] buffer vj_image_resample writes: what
// torchvision's RandomHorizontalFlip (PIL Image.transpose(FLIP_LEFT_RIGHT)) does to the S x S crop BEFORE timm's AutoAugment sees
// it   evals/image_classification_frozen/eval.py:392-403 (RandomResizedCrop -> RandomHorizontalFlip -> AutoAugment -> ToTensor -> ...)
// Behaviour restated, never copied.  Without a plan the flip stays where it was, on the fp32 side (vj_clip_transform_pre).
//
// S % 4 == 0, so an image is a multiple of 48 bytes (it starts on a 16-byte boundary of a 16-byte aligned buffer) and a row is
// S / 4 whole groups of four pixels, twelve bytes, three aligned words.  One thread owns group g of a row and its mirror group
// S/4 - 1 - g: it reads both as three words each, reverses the pixel order of each in registers (the bytes of a pixel keep their
// order) and writes each where the other was.  Both groups are read before either is written and no other thread touches them, so
// the pass is in place without a second copy; the middle group of an odd S / 4 is its own mirror and is read and written once.
// Adjacent lanes hold adjacent groups on both sides, so both loads and both stores of a wave are runs of consecutive bytes.
// Nothing outside [buf, buf + B*S*S*3) is addressed, and an unflagged image is left after one read of its flag.
#include "common.hpp"
#include "../../include/vjepa_hip.h"

namespace {

typedef uint32_t hf_u32x3_t __attribute__((ext_vector_type(3), aligned(4)));

// twelve bytes (p0 p1 p2 p3, three bytes each) -> (p3 p2 p1 p0)
__device__ __forceinline__ hf_u32x3_t hf_reverse(hf_u32x3_t w) {
  hf_u32x3_t o;
  o.x = (w.z >> 8) | ((w.y & 0x00ff0000u) << 8);
  o.y = (w.y >> 24) | ((w.z & 0xffu) << 8) | ((w.x >> 24) << 16) | (w.y << 24);
  o.z = ((w.y >> 8) & 0xffu) | (w.x << 8);
  return o;
}

__global__ __launch_bounds__(256) void image_hflip_kernel(uint8_t* __restrict__ buf, const int64_t* __restrict__ flags, int S) {
  const int64_t b = blockIdx.y;
  if (flags[b * 4 + 3] == 0) return;
  const uint32_t G = (uint32_t)S / 4u, half = (G + 1u) / 2u;       // groups of a row, and those a thread owns
  const uint32_t u = blockIdx.x * 256u + threadIdx.x;              // < S * half <= S * S, below 2^31 / 3
  if (u >= (uint32_t)S * half) return;
  const uint32_t y = u / half, g = u - y * half, m = G - 1u - g;   // g <= m
  uint8_t* row = buf + ((int64_t)b * S + y) * ((int64_t)S * 3);
  hf_u32x3_t* left = (hf_u32x3_t*)(row + (int64_t)g * 12);
  hf_u32x3_t* right = (hf_u32x3_t*)(row + (int64_t)m * 12);
  const hf_u32x3_t l = *left;
  if (g == m) {
    *left = hf_reverse(l);
    return;
  }
  const hf_u32x3_t r = *right;
  *left = hf_reverse(r);
  *right = hf_reverse(l);
}

}  // namespace

extern "C" int vj_image_hflip(uint8_t* buf, const int64_t* flags, int64_t B, int64_t S, int64_t flagged, hipStream_t stream) {
  VJ_CHECK_ARG(B >= 0 && B < 65536 && S > 0 && S < (1 << 15), "vj_image_hflip: bad dims B=%ld S=%ld", (long)B, (long)S);
  VJ_CHECK_ARG(S % 4 == 0, "vj_image_hflip: S=%ld must be a multiple of 4", (long)S);
  VJ_CHECK_ARG(B * S * S * 3 < (1ll << 31), "vj_image_hflip: buffer of %ld bytes, below 2^31 are taken", (long)(B * S * S * 3));
  VJ_CHECK_ARG(flagged >= 0 && flagged <= B, "vj_image_hflip: flagged=%ld of B=%ld images", (long)flagged, (long)B);
  if (B == 0 || flagged == 0) return 0;
  VJ_CHECK_ARG(buf != nullptr && flags != nullptr, "vj_image_hflip: null pointer");
  VJ_CHECK_ARG((uintptr_t)buf % 16 == 0 && (uintptr_t)flags % 8 == 0, "vj_image_hflip: buf must be 16-byte aligned, flags 8-byte");
  const int64_t per_image = S * ((S / 4 + 1) / 2);
  hipLaunchKernelGGL(image_hflip_kernel, dim3((unsigned)cdiv64(per_image, 256), (unsigned)B), dim3(256), 0, stream, buf, flags, (int)S);
  VJ_LAUNCH_CHECK("vj_image_hflip");
  return 0;
}
