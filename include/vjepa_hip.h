/*
 * vjepa_hip.h -- C ABI of libvjepa_hip.so: the MI355X (gfx950 / CDNA4) kernels of the V-JEPA pretraining step.
 *
 * The reference (facebookresearch/jepa) has no FFI layer: its device work is the ATen operator stream issued by
 * app/vjepa/train.py:414-498 through the modules of src/models.  This header is the boundary a maintainer would bind instead of
 * those ATen calls (see INTEGRATION.md for the ctypes stub).  Each entry point names the reference call site it
 * replaces.  Conventions:
 *   - every function returns 0 on success, a negative value for an argument error, or a positive hipError_t;
 *     vj_last_error() returns a thread-local description.  No C++ exception crosses this boundary.
 *   - all pointers are DEVICE pointers owned by the caller (borrowed for the duration of the launch);
 *     the library never allocates, frees or retains them.  Workspaces are passed in (vj_*_ws_bytes()).
 *   - every launch goes to the explicit hipStream_t (last argument); entry points are re-entrant.
 *   - "bf16" buffers are raw bfloat16 bits (uint16_t); indices are int64 as produced by the reference collator
 *     (src/masks/multiblock3d.py:155-203).
 *   - no torch types appear here; PyTorch is only the allocator/stream provider on the host side.
 */
#ifndef VJEPA_HIP_H
#define VJEPA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* vj_stream_t; /* == hipStream_t */

int vj_abi_version(void);
const char* vj_last_error(void);

/* ---- token-row movement (bit-exact) -------------------------------------------------------------------------
 * apply_masks: torch.gather(x, 1, idx[..., None].repeat(1,1,D))            src/masks/utils.py:11-23
 * dst[b,k,:] = src[b*src_batch_stride_rows + idx[b,k], :]; rows are row_bytes wide (multiple of 4).
 * src_batch_stride_rows = N for a [B,N,D] source, 0 to broadcast a [1,N,D] table (predictor.py:199,214). */
int vj_gather_rows(const void* src, void* dst, const int64_t* idx, int64_t B, int64_t K, int64_t row_bytes,
                   int64_t src_batch_stride_rows, vj_stream_t stream);
/* backward of the gather (aten::gather_backward -> scatter_add_ into zeros; indices unique per sample):
 * dst[B,N,row] is zero-filled, then dst[b, idx[b,k], :] = src[b,k,:]. */
int vj_scatter_rows(const void* src, void* dst, const int64_t* idx, int64_t B, int64_t N, int64_t K,
                    int64_t row_bytes, vj_stream_t stream);
/* bf16 row-slice copy: dst[b, dst_off+j, :] = src[b, src_off+j, :], j < n  (x[:, N_ctxt:], predictor.py:236);
 * src == NULL zero-fills those destination rows instead (autograd's zero gradient of the rows x[:, :N_ctxt] that the slice drops) */
int vj_copy_rows(const void* src, void* dst, int64_t B, int64_t src_rows, int64_t src_off, int64_t dst_rows,
                 int64_t dst_off, int64_t n, int64_t D, vj_stream_t stream);

/* ---- tubelet PatchEmbed3D front end -------------------------------------------------------------------------
 * Conv3d(3->D, k=s=(tub,p,p)) + flatten(2).transpose(1,2)                  src/models/utils/patch_embed.py:31-57
 * is a GEMM over non-overlapping tubelets; this packs fp32 clips [B,C,T,H,W] into its bf16 A operand
 * [B,K,C*tub*p*p] (element order c,dt,dh,dw = Conv3d weight order).  idx (nullable, [B,K]) fuses the context
 * mask gather (only kept tubelets are packed); NULL packs all K = N tokens in (t,h,w) order. */
int vj_tubelet_pack(const float* clips, void* out_bf16, const int64_t* idx, int64_t B, int64_t C, int64_t T,
                    int64_t H, int64_t W, int64_t tubelet, int64_t patch, int64_t K, vj_stream_t stream);
/* x += pos_embed (vision_transformer.py:172-174); with idx: x[b,k] += pos[idx[b,k]] (gather fused). */
int vj_add_pos(void* x_bf16, const float* pos, const int64_t* idx, int64_t B, int64_t K, int64_t D,
               vj_stream_t stream);

/* ---- device-side clip augmentation: decoded uint8 frames -> model-ready fp32 clips -----------------------------
 * VideoTransform.__call__ / _tensor_normalize_inplace                       app/vjepa/transforms.py:86-115,138-153
 * random_resized_crop[_with_shift] / horizontal_flip        src/datasets/utils/video/transforms.py:160-192,545-622
 * The random draws stay on the host (jepa_amd/app/vjepa/transforms.py); this is the pixel work: per-frame crop box, bilinear
 * resize to S x S (align_corners=False, fused source coordinate), flip(-1) of the clip, (x - mean) / std.
 *   frames  flat uint8 buffer of frames_bytes bytes holding clip after clip, each [T,Hs,Ws,3] interleaved RGB
 *   desc    int64 [B,4] = (byte offset of the clip in frames, Hs, Ws, flip flag)
 *   boxes   int32 [B,T,4] = (i, j, h, w): top, left, height, width of each frame's crop; 16-byte aligned
 *   out     fp32 [B,3,T,S,S] (what vj_tubelet_pack takes), S % 4 == 0
 *   mean_*, std_* in 0..255 units (the reference multiplies its ImageNet constants by 255).
 * Callers validate desc / boxes on the host before copying them (RawClipBatch.validate); the kernel itself clamps every source
 * row and column into the frame and writes zeros for a clip whose extent leaves the buffer.  B == 0 launches nothing. */
int vj_clip_transform(const uint8_t* frames, int64_t frames_bytes, const int64_t* desc, const int32_t* boxes, float* out,
                      int64_t B, int64_t T, int64_t S, float mean_r, float mean_g, float mean_b, float std_r, float std_g,
                      float std_b, vj_stream_t stream);
/* The normalise-first form the frozen video eval needs:        evals/video_classification_frozen/utils.py:256-274,298-301,326-343
 * (ToTensor / 255 -> tensor_normalize -> random_resized_crop; EvalVideoTransform and eval_transform: ClipToTensor / 255 -> Normalize).
 * Same arguments, tables and limits as vj_clip_transform, but mean_*, std_* are in 0..1 units and every source byte u of channel c
 * becomes n = (float(u) / 255 - mean_c) / std_c (three separately rounded fp32 operations) BEFORE the taps are blended; nothing is
 * done after the blend.  A box with h == w == S is a crop without a resize: its output is n of the addressed pixel, bit for bit.
 * Several rows of desc may name the same byte offset (the spatial views of one segment share one copy of their frames). */
int vj_clip_transform_pre(const uint8_t* frames, int64_t frames_bytes, const int64_t* desc, const int32_t* boxes, float* out,
                          int64_t B, int64_t T, int64_t S, float mean_r, float mean_g, float mean_b, float std_r, float std_g,
                          float std_b, vj_stream_t stream);
/* RandomErasing(mode='pixel', max_count=1, cube=True)._erase_cube         src/datasets/utils/video/randerase.py:116-156
 * as the reference applies it after flip and normalisation (app/vjepa/transforms.py:110-113, eval utils.py:278-281).  The box and
 * the N(0,1) values are draws and stay on the host; this is the copy:
 *   clips[b,c,t,top+y,left+x] = noise[noise_off[b] + ((t*3+c)*h+y)*w+x],   y < h, x < w
 *   clips      fp32 [B,3,T,S,S], written in place (the output of vj_clip_transform[_pre])
 *   ebox       int32 [B,4] = (top, left, h, w); h == 0: clip b is not erased; 16-byte aligned
 *   noise      fp32 [noise_elems]: per erased clip one [T,3,h,w] block starting at noise_off[b] (int64 [B])
 * Bit-exact.  Callers validate the tables on the host (RawClipBatch.validate); the kernel skips a clip whose box leaves S x S or
 * whose block leaves [0, noise_elems), so nothing outside either buffer is touched.  B == 0 or noise_elems == 0 (no clip of the
 * batch is erased) launches nothing.  B < 65536, 3*T*S*S < 2^31. */
int vj_clip_erase(float* clips, const int32_t* ebox, const float* noise, int64_t noise_elems, const int64_t* noise_off, int64_t B,
                  int64_t T, int64_t S, vj_stream_t stream);
/* RandAugment on the decoded uint8 frames, before everything else        evals/video_classification_frozen/utils.py:233-237,256-259
 * RandAugment.__call__ / AugmentOp.__call__ and the 15 operations         src/datasets/utils/video/randaugment.py:51-179,324-369,449-465
 * (PIL behind them: ImageOps, ImageEnhance, ImageFilter.SMOOTH, Image.transform(AFFINE, BICUBIC, fillcolor=(128,128,128))).
 * The draws stay on the host (jepa_amd/app/vjepa/randaugment.py: which operations, whether each runs, magnitudes, signs, and the
 * affine coefficients); this is the pixel work, in place, byte for byte what PIL gives.
 *   frames  the flat buffer of vj_clip_transform (clip b: [T,Hs,Ws,3] interleaved RGB); 16-byte aligned, frames_bytes < 2^31
 *   desc    int64 [B,4] = (byte offset, Hs, Ws, unused), the table vj_clip_transform takes; offsets are multiples of 16
 *   ops     int32 [B,L], L <= 8: operation code of clip b in layer l, applied in order (layer l+1 reads layer l's output):
 *           0 nothing, 1 AutoContrast, 2 Equalize, 3 Invert, 4 Rotate, 5 Posterize, 6 Solarize, 7 SolarizeAdd, 8 Color, 9 Contrast,
 *           10 Brightness, 11 Sharpness, 12 ShearX, 13 ShearY, 14 TranslateXRel, 15 TranslateYRel
 *   args    double [B,L,6]: the six affine coefficients (4, 12..15), else in [0] the factor (8..11), the bits kept (5), the
 *           threshold (6) or the addend (7)
 *   ws      workspace of vj_clip_randaug_ws_bytes(frames_bytes, B, T) bytes, 16-byte aligned: a second copy of the frame buffer
 *           (layers read one copy and write the other) and one [3][256] byte table per (clip, frame)
 * Two launches per layer and one more when L is odd; callers drop the layers in which no clip has an operation before they upload
 * the tables.  A clip whose row is all zeros, the padding between clips, and a clip whose extent leaves the buffer are not
 * changed by one byte.  An augmented clip must not share its bytes with another row.  B == 0 or L == 0 launches nothing. */
int vj_clip_randaug(uint8_t* frames, int64_t frames_bytes, const int64_t* desc, int64_t B, int64_t T, const int32_t* ops,
                    const double* args, int64_t L, void* ws, int64_t ws_bytes, vj_stream_t stream);
int64_t vj_clip_randaug_ws_bytes(int64_t frames_bytes, int64_t B, int64_t T);
/* vj_clip_randaug with the fill colour of the affine family (Rotate, ShearX/Y, TranslateX/YRel) as an argument: the colour PIL's
 * Image.transform / Image.rotate write where the source has no pixel.  timm's AutoAugment / RandAugment for images fill with the
 * dataset mean, img_mean = tuple(min(255, round(255 * m)) for m in mean) = (124, 116, 104) for the ImageNet mean (timm
 * transforms_factory.py, the aa_params of create_transform -> auto_augment_transform, which the image evals' training transform is:
 * evals/image_classification_frozen/eval.py:392-403); the reference's video RandAugment fills with (128, 128, 128)
 * (src/datasets/utils/video/randaugment.py _FILL), which is what vj_clip_randaug passes here.  One kernel body serves both.
 *   fill_r, fill_g, fill_b   the colour as three bytes, each passed as an int in 0..255 (anything else is an error)
 * Every other argument, limit and guarantee is vj_clip_randaug's, the workspace that of vj_clip_randaug_ws_bytes.  The operations
 * outside the affine family do not read the colour. */
int vj_clip_randaug_fill(uint8_t* frames, int64_t frames_bytes, const int64_t* desc, int64_t B, int64_t T, const int32_t* ops,
                         const double* args, int64_t L, void* ws, int64_t ws_bytes, int fill_r, int fill_g, int fill_b,
                         vj_stream_t stream);
/* The input edge of the image evals: random-resized crop (bicubic) of training, Resize (bilinear, short side) + CenterCrop of
 * validation                                                                 evals/image_classification_frozen/eval.py:379-423
 * as PIL does them on 8-bit RGB: Image.crop(box).resize((OW, OH), filter), an antialiased two-pass resample whose support widens
 * with the reduction ratio, with 22-bit integer coefficients and a uint8 intermediate between the horizontal (first) and the
 * vertical pass.  Byte for byte what PIL gives; csrc/image_resample.hip states the arithmetic.  The draws stay on the host
 * (jepa_amd/evals/image_classification_frozen/transforms.py).
 *   frames  the flat buffer of vj_clip_transform holding image after image, each [Hs,Ws,3] interleaved RGB; 16-byte aligned; only read
 *   desc    int64 [B,4] = (byte offset, Hs, Ws, unused); offsets are multiples of 16
 *   geom    int32 [B,8] = (i, j, h, w, OH, OW, wy, wx): the crop box top i, left j, height h, width w is resampled to OH x OW, and
 *           the S x S window of that result whose corner is (wy, wx) is written -- only the window is computed.  Training: OH = OW = S,
 *           window (0, 0); validation: the box is the image, (OH, OW) the short-side size, the window the centre crop
 *   out     uint8 [B,S,S,3], S % 4 == 0: a buffer of one-frame clips with Hs = Ws = S at offsets b*S*S*3, which vj_clip_transform_pre
 *           (and vj_clip_randaug[_fill], vj_image_hflip) takes
 *   filter  0 bilinear (support 1), 1 bicubic (a = -0.5, support 2)
 *   taps_x, taps_y, rows   capacities of the workspace, maxima over the batch: taps an output index can have per axis,
 *           int(ceil(support * max(n / m, 1))) * 2 + 1, and source rows the window's vertical taps span.  Tap loops are bounded at
 *           run time; there is no compile-time cap on the reduction ratio
 *   ws      workspace of vj_image_resample_ws_bytes(B, S, taps_x, taps_y, rows) bytes, 16-byte aligned: bounds and coefficient
 *           tables and the intermediate
 * Three launches.  Callers validate desc and geom on the host before copying them (RawImageBatch.validate); the kernels clamp every
 * source index into the crop and write zeros for an image that leaves the buffer, whose box leaves the image, whose window leaves
 * OH x OW or that needs more than the capacities.  B == 0 launches nothing.  B < 65536, sides below 32768. */
int vj_image_resample(const uint8_t* frames, int64_t frames_bytes, const int64_t* desc, const int32_t* geom, uint8_t* out, int64_t B,
                      int64_t S, int filter, int64_t taps_x, int64_t taps_y, int64_t rows, void* ws, int64_t ws_bytes,
                      vj_stream_t stream);
int64_t vj_image_resample_ws_bytes(int64_t B, int64_t S, int64_t taps_x, int64_t taps_y, int64_t rows);
/* The short-side Resize of the video evals' validation transforms    evals/video_classification_frozen/utils.py:217-223, 297-321
 * on frames that are PIL images (src/datasets/utils/video/functional.py:52-67): Image.resize((OW, OH), filter) of every frame of
 * every clip, whole frames, byte for byte, with the arithmetic of vj_image_resample (the table entry and the two pass bodies are
 * shared).  Bounds and coefficients are computed once per (clip, axis, output index) and read by all T frames.  The reference's
 * numpy frames go through cv2.INTER_LINEAR, which is not antialiased; that arithmetic is not implemented.
 *   frames, desc   exactly what vj_clip_transform_pre takes: clip b is [T,Hs,Ws,3] at desc[b] = (byte offset, Hs, Ws, flag); only read
 *   rgeom     int32 [B,2] = (OH, OW); a clip with (OH, OW) == (Hs, Ws) comes out as a copy
 *   out       flat uint8 buffer of out_bytes bytes, 16-byte aligned
 *   desc_out  int64 [B,4] = (byte offset of the resized clip in out, a multiple of 16; OH; OW; the flag carried over), built and
 *             validated by the caller on the host.  Clip b is written dense, [T,OH,OW,3]: out with desc_out is a frame buffer for
 *             vj_clip_transform_pre, vj_clip_randaug and the box tables.  OW * 3 need not be a multiple of anything: the vertical
 *             pass stores aligned words and single bytes at the row edges, and writes no byte outside
 *             [offset, offset + T*OH*OW*3) of its clip -- padding between clips keeps its bytes
 *   filter    0 bilinear, 1 bicubic
 *   oh, ow, taps_x, taps_y, rows   capacities of the workspace, maxima over the batch: OH, OW, the taps per axis as for
 *             vj_image_resample, and the source height Hs
 *   ws        workspace of vj_clip_resample_ws_bytes(B, T, oh, ow, taps_x, taps_y, rows) bytes, 16-byte aligned
 * Three launches.  Every kernel re-derives validity from the tables: a clip whose source leaves frames, whose destination leaves
 * out, whose desc_out disagrees with rgeom or that needs more than the capacities is written as zeros over the part of out its
 * desc_out row names; source indices are clamped; nothing outside frames, ws and the clip's own output range is touched.
 * B == 0 launches nothing.  B, T < 65536, sides below 32768. */
int vj_clip_resample(const uint8_t* frames, int64_t frames_bytes, const int64_t* desc, const int32_t* rgeom, uint8_t* out,
                     int64_t out_bytes, const int64_t* desc_out, int64_t B, int64_t T, int filter, int64_t oh, int64_t ow,
                     int64_t taps_x, int64_t taps_y, int64_t rows, void* ws, int64_t ws_bytes, vj_stream_t stream);
int64_t vj_clip_resample_ws_bytes(int64_t B, int64_t T, int64_t oh, int64_t ow, int64_t taps_x, int64_t taps_y, int64_t rows);
/* RandomHorizontalFlip of the S x S crop on the uint8 side, in place: PIL's Image.transpose(FLIP_LEFT_RIGHT), which timm's training
 * pipeline applies BEFORE its AutoAugment policy (RandomResizedCrop -> RandomHorizontalFlip -> AutoAugment -> ToTensor -> Normalize ->
 * RandomErasing; evals/image_classification_frozen/eval.py:392-403), so a batch that carries a policy plan is mirrored here and
 * vj_clip_transform_pre then gets a zero flip column.  out[b, y, x, :] = in[b, y, S-1-x, :] for every flagged image b.
 *   buf      uint8 [B,S,S,3], the output buffer of vj_image_resample; 16-byte aligned, S % 4 == 0, B*S*S*3 < 2^31
 *   flags    int64 [B,4]: column 3 is the flip flag of image b (the descriptor table vj_clip_transform_pre takes); 8-byte aligned
 *   flagged  how many images are flagged, as the host knows them (0 <= flagged <= B): only 0 is acted upon, it launches nothing
 * Words are moved, never single bytes: a thread swaps a group of four pixels with its mirror group and permutes their bytes in
 * registers.  An unflagged image, and anything outside [buf, buf + B*S*S*3), is not touched by one byte.  B == 0 launches nothing.
 * Bit-exact. */
int vj_image_hflip(uint8_t* buf, const int64_t* flags, int64_t B, int64_t S, int64_t flagged, vj_stream_t stream);

/* ---- still-image front end of the video encoder and position-table interpolation ------------------------------
 * input.unsqueeze(2).repeat(1, 1, frames_per_clip, 1, 1) + patch_embed    evals/image_classification_frozen/eval.py:452-455
 * fp32 images [B,C,H,W] -> the bf16 A operand [B,K,C*tub*p*p] of the patch-embed GEMM for the gh*gw DISTINCT tubelets of
 * the repeated clip (element order c,dt,dh,dw; each pixel read once, written to the `tubelet` dt slices).  idx (nullable,
 * [B,K]): row k of image b is cell idx[b,k] % (gh*gw), so both spatial indices and indices into the (t,h,w) grid of the
 * repeated clip are accepted; NULL packs K = gh*gw cells in (h,w) order.  Rows are bit-identical to vj_tubelet_pack's on
 * the materialised clip. */
int vj_image_pack(const float* images, void* out_bf16, const int64_t* idx, int64_t B, int64_t C, int64_t H, int64_t W,
                  int64_t tubelet, int64_t patch, int64_t K, vj_stream_t stream);
/* x += pos_embed (vision_transformer.py:172-174) for the repeated clip of a still image: y bf16 [B,S,D] holds the patch
 * embedding of the S = gh*gw distinct tubelets, pos fp32 [Gt*S,D], out bf16 [B,Gt*S,D]:
 * out[b, t*S+s, :] = bf16(float(y[b,s,:]) + pos[t*S+s, :]).  Same fp32 add and single rounding as vj_add_pos. */
int vj_add_pos_bcast(const void* y_bf16, const float* pos, void* out_bf16, int64_t B, int64_t S, int64_t Gt, int64_t D,
                     vj_stream_t stream);
/* The adjoint of vj_add_pos_bcast (the backward of the still-image front end; the position table is a constant): the gradient of
 * the S distinct patch embeddings is the sum of the gradients of the Gt temporal slices.  dx bf16 [B,Gt*S,D] -> dy bf16 [B,S,D]:
 * dy[b,s,:] = bf16( sum_{t<Gt} float(dx[b, t*S+s, :]) ), accumulated in fp32 from slice 0 in ascending t with plain adds (a fixed
 * order: the result is reproducible bit for bit) and rounded once; Gt == 1 copies the bits.  D % 8 == 0, dx and dy 16-byte
 * aligned and distinct.  B*S*Gt == 0 launches nothing. */
int vj_slice_sum(const void* dx_bf16, void* dy_bf16, int64_t B, int64_t S, int64_t Gt, int64_t D, vj_stream_t stream);
/* nn.functional.interpolate(pos_embed [1,D,Nt,Nh,Nw], scale_factor=(T/N_t, H/N_h, W/N_w), mode='trilinear')
 *                                                                         src/models/vision_transformer.py:221-227
 * on the token-major table: fp32 [Nt,Nh,Nw,D] -> [To,Ho,Wo,D].  align_corners=False with the scale factors given (the
 * source coordinate uses float(1/scale), not in/out); To,Ho,Wo must equal floor(in * scale) computed in double. */
int vj_pos_interp3d(const float* table, float* out, int64_t Nt, int64_t Nh, int64_t Nw, int64_t D, double scale_t,
                    double scale_h, double scale_w, int64_t To, int64_t Ho, int64_t Wo, vj_stream_t stream);

/* ---- image (num_frames = 1) encoders ---------------------------------------------------------------------------
 * The 2-D PatchEmbed (Conv2d, src/models/utils/patch_embed.py:11-28) is vj_tubelet_pack on the image viewed as [B,C,1,H,W]
 * with tubelet = 1, the patch-embed GEMM with K = C*p*p and vj_add_pos.
 * nn.functional.interpolate(pos_embed [1,D,Nh,Nw], scale_factor=sqrt(npatch / N), mode='bicubic')
 *                                                                         src/models/vision_transformer.py:238-245
 * on the token-major table: fp32 [Nh,Nw,D] -> [Ho,Wo,D].  align_corners=False with the scale factor given: the source
 * coordinate (dst + 0.5) * float(1/scale) - 0.5 is not clamped at zero, the four taps per axis are clamped into the table
 * and weighted by the cubic convolution with A = -0.75, fp32 accumulation.  Ho, Wo must equal floor(in * scale) computed in
 * double; table and out 16-byte aligned, D % 4 == 0. */
int vj_pos_interp2d_bicubic(const float* table, float* out, int64_t Nh, int64_t Nw, int64_t D, double scale, int64_t Ho,
                            int64_t Wo, vj_stream_t stream);
/* FrameAggregation's temporal position embedding: o += pos_embed[clip_indices] repeated over the N tokens of each frame
 *                                                                         evals/video_classification_frozen/utils.py:74-80
 * x bf16 [B, F*N, D], pos fp32 [max_frames, D], idx int64 [B,F] (the segments' clip_indices concatenated along time):
 * x[b, f*N+n, :] = bf16(float(x[b, f*N+n, :]) + pos[idx[b,f], :]).  Same fp32 add and single rounding as vj_add_pos.  The
 * caller validates 0 <= idx < max_frames on the host before copying idx; the kernel clamps it all the same.  D % 8 == 0; x and pos 16-byte aligned. */
int vj_add_pos_frames(void* x_bf16, const float* pos, const int64_t* idx, int64_t B, int64_t F, int64_t N, int64_t D,
                      int64_t max_frames, vj_stream_t stream);

/* ---- stochastic depth (drop path) of encoder fine-tuning ------------------------------------------------------
 * The ViT lineage's `x = x + drop_path(branch(x))` at the two residual adds of a block, drop_path(v) = v * floor(keep + u) / keep
 * with one u ~ U[0,1) per sample; the V-JEPA reference builds its blocks without it (src/models/utils/modules.py:114-120) and
 * releases no fine-tuning loop.  These two replace the ATen broadcast multiply + add of that expression and the multiply autograd
 * runs for it in the backward; the caller computes the per-sample scales s[b] (0 or 1 / keep) on the device.
 * y <- bf16( fmaf(s[b], y, x) ) for the rows of sample b (rows b*S .. b*S+S-1); where s[b] == 0 the row becomes the bits of x and
 * y is NOT read (it may hold anything, NaN included).  x, y bf16 [B*S, D], s fp32 [B] on the device.  D % 8 == 0; x and y distinct,
 * 16-byte aligned.  B * S == 0 launches nothing; every argument is checked on the host before any HIP call. */
int vj_drop_path_add(const void* x_bf16, void* y_bf16, const float* scale, int64_t B, int64_t S, int64_t D, vj_stream_t stream);
/* out <- bf16( s[b] * dx ) (fp32 product, one rounding to bf16); where s[b] == 0 the row is +0 and dx is NOT read.  The scaled
 * copy is the dY of the branch's last Linear (proj / fc2): its dgrad, weight gradient and bias gradient all read it.  Same shapes
 * and conditions as vj_drop_path_add. */
int vj_drop_path_scale(const void* dx_bf16, void* out_bf16, const float* scale, int64_t B, int64_t S, int64_t D, vj_stream_t stream);

/* ---- mixup / cutmix / label smoothing of encoder fine-tuning ----------------------------------------------------
 * The ViT lineage's batch-mode mixup and cutmix (x = lam * x + (1 - lam) * x.flip(0); x[..., y0:y1, x0:x1] = x.flip(0)[..., y0:y1,
 * x0:x1]) and its soft-target cross-entropy; the V-JEPA reference has neither (its probes train on hard labels,
 * evals/video_classification_frozen/eval.py:309) and releases no fine-tuning loop.  The draws stay on the host (jepa_amd/evals/mix.py).
 * vj_clip_mix replaces the ATen flip / multiply / add / slice-assign of those expressions without a second copy of the batch:
 *   x    fp32 [B,P,H,W] (P = 3*T planes of a clip), mixed IN PLACE: sample i with sample B-1-i, both directions by one thread per
 *        16-byte chunk of the pair; the middle sample of an odd B, and B == 1, keep their bits
 *   lam  fp32 [B], box int32 [B,4] = (y0, y1, x0, x1) per sample (batch mode gives a pair equal rows; the kernel does not assume it)
 * per element of sample i: inside box_i the bits of x_j; outside it with lam_i == 1 the bits of x_i (not written; a pair with lam == 1
 * and empty boxes on both sides is not read); otherwise fmaf(lam_i, x_i, (1 - lam_i) * x_j) in fp32 (1 - lam_i and the product are
 * rounded on their own).  W % 4 == 0, x 16-byte aligned, P*H*W < 2^33; callers validate 0 <= y0 <= y1 <= H, 0 <= x0 <= x1 <= W on the
 * host before they copy the table (the kernel only compares against it: no box makes it leave x).  Every argument is checked on the
 * host before any HIP call. */
int vj_clip_mix(float* x, const float* lam, const int32_t* box, int64_t B, int64_t P, int64_t H, int64_t W, vj_stream_t stream);
/* sum(-t * log_softmax(z), dim=-1) per row for the target t_c = eps / C + (1 - eps) * (lam * [c == a] + (1 - lam) * [c == b]), which
 * is never materialised: loss[r] = lse - (1 - eps) * (lam * z_a + (1 - lam) * z_b) - (eps / C) * sum_c z_c, dlogits[r,:] = softmax(z) - t
 * (d loss[r] / d z; a == b gives the one column the whole 1 - eps), probs (nullable) = softmax(z).  One wave per row, three passes
 * (maximum; sum exp(z - max) and sum z in fp32; the outputs).  logits fp32 [R,C] with row stride ld >= C; label_a, label_b int32 [R];
 * lam fp32 [R]; loss fp32 [R]; dlogits, probs fp32 [R,C] contiguous.  0 <= smoothing < 1, C >= 1.  Callers validate the labels on the
 * host (the kernel clamps them into [0, C) all the same).  eps = 0, lam = 1 is nn.CrossEntropyLoss(reduction='none'). */
int vj_soft_ce(const float* logits, int64_t ld, const int32_t* label_a, const int32_t* label_b, const float* lam, float smoothing,
               int64_t R, int64_t C, float* loss, float* dlogits, float* probs, vj_stream_t stream);

/* ---- LayerNorm ----------------------------------------------------------------------------------------------
 * nn.LayerNorm(eps=1e-6) (modules.py:97,106,115,119; vision_transformer.py:193; predictor.py:233).
 * bf16 in/out, fp32 statistics; mean/rstd (nullable pair) are saved for the backward. */
int vj_layernorm_fwd(const void* x_bf16, const float* gamma, const float* beta, void* y_bf16, float* mean,
                     float* rstd, int64_t rows, int64_t D, float eps, vj_stream_t stream);
int64_t vj_layernorm_bwd_ws_bytes(int64_t D);
/* dx = LN'(dy) [+ dres]; dgamma/dbeta = alpha*sum + beta_acc*old (fp32, into the gradient arena). */
int vj_layernorm_bwd(const void* dy_bf16, const void* x_bf16, const float* gamma, const float* mean,
                     const float* rstd, const void* dres_bf16, void* dx_bf16, float* dgamma, float* dbeta,
                     float alpha, float beta_acc, int64_t rows, int64_t D, void* ws, int64_t ws_bytes,
                     vj_stream_t stream);

/* the same, plus dxsum[D] (nullable) = alpha * column sums of dx + beta_acc * old: in a Block, dx of norm2's backward is the dY
 * of attn.proj and dx of norm1's backward the dY of the previous block's mlp.fc2, so autograd's bias gradients of those two
 * Linears (sum over tokens of dY, modules.py:34,76) come out of this pass instead of a separate read of dY. */
int vj_layernorm_bwd_colsum(const void* dy_bf16, const void* x_bf16, const float* gamma, const float* mean,
                            const float* rstd, const void* dres_bf16, void* dx_bf16, float* dgamma, float* dbeta,
                            float* dxsum, float alpha, float beta_acc, int64_t rows, int64_t D, void* ws,
                            int64_t ws_bytes, vj_stream_t stream);

/* ---- bf16 MFMA GEMM  C[M,N] = A[M,K] * B[N,K]^T (+ fused epilogue) ------------------------------------------
 * nn.Linear fwd/bwd (modules.py:31-34,63,76; predictor.py:194,237) and the Conv3d GEMM (patch_embed.py:56).
 * epilogue: 0 bf16 out = acc [+bias] [+residual]      (qkv / proj+residual / fc2+residual / dgrads)
 *           1 bf16 out = gelu(u), u = bf16(acc+bias); aux_out(nullable) = bf16(gelu'(u))   (fc1 + nn.GELU, modules.py:31-32;
 *             the derivative is saved INSTEAD of the pre-activation: it shares the erfc evaluation of the forward and is
 *             the only thing the backward needs from u)
 *           2 bf16 out = acc * aux_in, aux_in = what epilogue 1 saved   (fc2 dgrad fused with the GELU backward)
 *           3 fp32 out = alpha*acc + beta*C            (wgrad straight into the fp32 gradient arena)
 *           4 bf16 out = (acc + bias) * (n < N/3 ? alpha : 1)   (the qkv projection of Attention, modules.py:63, whose q part carries
 *             the soft-max scale alpha = head_dim^-0.5 * log2(e) with ONE rounding; the attention entry points are then called with
 *             a NEGATIVE scale = "q is pre-scaled"; N % 12 == 0, no residual)
 * K % 32 == 0, N % 4 == 0, lda/ldb % 8 == 0.  flags bits 4-8: kernel selection (0 = automatic).  The GELU epilogues (1) evaluate
 * Phi(-|x|) as exp2 of a degree-6 polynomial: 5 of the 24 222 bf16 inputs in (-5, 2^127) round differently from the correctly
 * rounded bf16 erf-GELU of nn.GELU() (tests/test_gelu_poly.py). */
int vj_gemm_bf16_nt(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M,
                    int64_t N, int64_t K, const float* bias, const void* residual, int64_t ldr, const void* aux_in,
                    void* aux_out, int64_t ldaux, int epilogue, float alpha, float beta, int flags,
                    vj_stream_t stream);
/* fc2 dgrad (epilogue 2) that also produces the bias gradient of fc1 (autograd of Mlp.fc1's bias, modules.py:31-34: the sum
 * over tokens of the dY this GEMM writes): when the persistent 256 x 256 kernel takes the problem, colpart
 * [vj_gemm_colsum_rows(M)][N] receives fp32 column sums of C (before the bf16 rounding) per (row tile, wave row) and *fused = 1;
 * otherwise the plain GEMM runs and *fused = 0 (sum C with vj_colsum_bf16).  C is bit-identical to vj_gemm_bf16_nt's. */
int64_t vj_gemm_colsum_rows(int64_t M);
int vj_gemm_bf16_nt_dgelu_colsum(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M,
                                 int64_t N, int64_t K, const void* aux_in, int64_t ldaux, float* colpart,
                                 int64_t colpart_rows, int flags, int* fused, vj_stream_t stream);
/* wgrad form of the same GEMM: C (fp32) = alpha*A*B^T + beta*C where K (= tokens) is long and the [M,N] tile grid
 * alone cannot fill 256 CUs: K is split across workgroups, partials combined deterministically from ws
 * (ws_bytes >= M*N*4; more workspace allows more slices). */
int vj_gemm_bf16_nt_splitk(const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t ldc, int64_t M,
                           int64_t N, int64_t K, float alpha, float beta, int flags, void* ws, int64_t ws_bytes,
                           vj_stream_t stream);
/* weight gradient WITHOUT operand transposes (autograd of nn.Linear, modules.py:31-34,63,76):
 *   dW[N1,N2] (fp32) = alpha * dY[T,N1]^T * X[T,N2] + beta * dW,   T = tokens (any positive count; the last 64-token
 * tile is completed with zero rows inside the kernel).  Both operands are read row-major as the backward pass left
 * them; N1 % 8 == 0, N2 % 8 == 0, ldy/ldx % 8 == 0 and < 2^24, 16-byte aligned bases; split-K over the tokens as
 * above (ws_bytes >= N1*N2*4). */
int vj_gemm_bf16_tn_splitk(const void* dY, int64_t ldy, const void* X, int64_t ldx, float* dW, int64_t ldw, int64_t T,
                           int64_t N1, int64_t N2, float alpha, float beta, void* ws, int64_t ws_bytes,
                           vj_stream_t stream);
/* The weight gradients of n <= 4 Linear layers over the SAME T tokens in ONE launch -- a transformer block's qkv, proj,
 * fc1, fc2 (the four nn.Linear backward nodes of Block.forward, modules.py:31-34,63,76).  Per problem the contract of
 * vj_gemm_bf16_tn_splitk; one split factor for the group; ws_bytes >= 4 * sum N1*N2 (more allows split-K). */
typedef struct vj_tn_problem {
  const void* dY; int64_t ldy; /* [T, N1] bf16 */
  const void* X;  int64_t ldx; /* [T, N2] bf16 */
  float* dW;      int64_t ldw; /* [N1, N2] fp32 */
  int64_t N1, N2;
} vj_tn_problem_t;
int vj_gemm_bf16_tn_grouped(const vj_tn_problem_t* problems, int64_t n, int64_t T, float alpha, float beta, void* ws,
                            int64_t ws_bytes, vj_stream_t stream);
/* out[N, Mpad] = in[M,N]^T (zero padded): the wgrad operands dY^T, X^T; weight shadows W^T for dgrad. */
int vj_transpose_bf16(const void* in, void* out, int64_t M, int64_t N, int64_t ld_in, int64_t Mpad,
                      vj_stream_t stream);
/* one launch for many transposes (all W^T dgrad shadows after an optimizer step): desc = device array of
 * {src, dst, M, N, ld_in, Mpad} (6 x int64 per tensor), blocks = device int32[4*n_blocks] {tensor, tile_m, tile_n, 0} */
int vj_transpose_multi(const void* desc, const void* blocks, int64_t n_blocks, vj_stream_t stream);
/* transpose + bias gradient in ONE pass over dY: colsum[n] = alpha*sum_m in[m][n] + beta*colsum[n] */
int64_t vj_transpose_colsum_ws_bytes(int64_t M, int64_t N);
int vj_transpose_colsum_bf16(const void* in, void* out, int64_t M, int64_t N, int64_t ld_in, int64_t Mpad,
                             float* colsum, float alpha, float beta, void* ws, int64_t ws_bytes, vj_stream_t stream);
/* bias / mask-token gradients: out[n] = alpha * sum_{m: row_lo <= m % group < row_hi} in[m][n] + beta*out[n] */
int64_t vj_colsum_ws_bytes(int64_t N);
int vj_colsum_bf16(const void* in, int64_t M, int64_t N, int64_t ld, int64_t group, int64_t row_lo, int64_t row_hi,
                   float* out, float alpha, float beta, void* ws, int64_t ws_bytes, vj_stream_t stream);
int vj_reduce_partials(const float* part, float* out, int64_t P, int64_t N, float alpha, float beta,
                       vj_stream_t stream);
/* n <= 16 such reductions in ONE launch: out_s[n] = alpha * sum_p part_s[p*stride_s + n] + beta * out_s[n]; same summation
 * order (hence the same bits) as vj_reduce_partials.  The backward of a Block ends with one of these: LayerNorm dgamma / dbeta,
 * the proj / fc2 bias sums (modules.py:34,76) and the qkv / fc1 bias partials of the kernels that produce their dY. */
typedef struct vj_reduce_seg {
  const float* part; /* [P, stride] fp32 partials */
  float* out;        /* [N] */
  int64_t P, N, stride;
} vj_reduce_seg_t;
int vj_reduce_segments(const vj_reduce_seg_t* segs, int64_t n_segs, float alpha, float beta, vj_stream_t stream);

/* ---- attention ----------------------------------------------------------------------------------------------
 * F.scaled_dot_product_attention(q,k,v) (modules.py:66-69): dense, non-causal, scale = head_dim^-0.5.
 * qkv: packed qkv-Linear output [B,S,3,H,hd] (modules.py:63 before the permute); o: [B,S,H*hd];
 * lse2: [B,H,S] fp32 log2-sum-exp saved for the backward (nullable in inference).  hd % 8 == 0, hd <= 128. */
/* scale > 0: the kernels fold scale*log2(e) into the stationary operand of the score product themselves (one more bf16 rounding
 * of q / k); scale < 0: the caller's qkv GEMM already stored q * |scale| * log2(e) (epilogue 4 above) -- same for the backward. */
int vj_attn_fwd(const void* qkv, void* o, float* lse2, int64_t B, int64_t S, int64_t H, int64_t hd, float scale,
                vj_stream_t stream);
/* The same for n_segs <= 4 segments of ONE token-major activation in one launch -- the rows of the masks of a V-JEPA batch
 * are concatenated (MultiMaskWrapper loops over them, src/models/utils/multimask.py:17-27): qkv [M, 3*H*hd], o [M, H*hd],
 * lse2 [H*M] with segment i's block [B_i, H, S_i] at offset H*row0_i.  The short segment's workgroups fill the tail of the
 * long one instead of paying their own launch. */
typedef struct vj_seg {
  int64_t row0; /* first token row of the segment */
  int64_t B, S; /* rows row0 .. row0 + B*S are B sequences of S tokens */
} vj_seg_t;
int vj_attn_fwd_segs(const void* qkv, void* o, float* lse2, const vj_seg_t* segs, int64_t n_segs, int64_t H, int64_t hd,
                     float scale, vj_stream_t stream);
int64_t vj_attn_bwd_ws_bytes(int64_t B, int64_t S, int64_t H);   /* the two-kernel form's delta [B,H,S] only: prefer the next one */
/* workspace bytes of vj_attn_bwd / vj_attn_bwd_segs / vj_attn_bwd_colsum for a segment list: delta = rowsum(dO . O) of the softmax
 * backward (autograd of modules.py:66-69), 4*H bytes per token row up to the last row of the list */
int64_t vj_attn_bwd_segs_ws_bytes(const vj_seg_t* segs, int64_t n_segs, int64_t H, int64_t hd);
/* dqkv [B,S,3,H,hd] <- (dout [B,S,H*hd], saved qkv, o, lse2) */
int vj_attn_bwd(const void* qkv, const void* o, const void* dout, const float* lse2, void* dqkv, int64_t B,
                int64_t S, int64_t H, int64_t hd, float scale, void* ws, int64_t ws_bytes, vj_stream_t stream);
/* the same, plus the column sums of dqkv over this [B,S] segment as fp32 partials -- the qkv bias gradient (autograd of
 * Attention.qkv's bias, modules.py:63) from the kernels that produce dqkv instead of a second pass over it:
 * colq [rows_q][H*hd] (dQ kernel: one row per (sample, 128-query block)), colkv [rows_kv][2*H*hd] (dK/dV kernel: one row per
 * (sample, key block)); row counts from vj_attn_bwd_colsum_rows (they depend on the head-dim class); every element is
 * written; dqkv is bit-identical to vj_attn_bwd's.  Reduce with vj_reduce_segments. */
int vj_attn_bwd_colsum_rows(int64_t B, int64_t S, int64_t hd, int64_t* rows_q, int64_t* rows_kv);
int vj_attn_bwd_colsum(const void* qkv, const void* o, const void* dout, const float* lse2, void* dqkv, int64_t B,
                       int64_t S, int64_t H, int64_t hd, float scale, void* ws, int64_t ws_bytes, float* colq,
                       float* colkv, vj_stream_t stream);
/* backward over n_segs <= 4 segments in one launch pair (dQ, then dK/dV); ws >= 4*H*M bytes; colq / colkv (both or neither,
 * nullable): the column partials, segment after segment in list order */
int vj_attn_bwd_segs(const void* qkv, const void* o, const void* dout, const float* lse2, void* dqkv, const vj_seg_t* segs,
                     int64_t n_segs, int64_t H, int64_t hd, float scale, void* ws, int64_t ws_bytes, float* colq,
                     float* colkv, vj_stream_t stream);

/* ---- cross-attention of a few learned queries against frozen-encoder tokens (attentive probe, row f4 widened) ------
 * CrossAttention.forward (src/models/utils/modules.py:140-157) as used by CrossAttentionBlock (modules.py:177-181) inside
 * AttentivePooler / AttentiveClassifier (src/models/attentive_pooler.py:96-136; num_queries = 1 there).
 * q: [B or 1, NQ, H*hd] bf16 (q_bstride = elements between samples, 0 when every sample shares the projected query);
 * kv: packed kv-Linear output [B,N,2,H,hd] (modules.py:145 before the permute); resid (nullable): [NQ, H*hd] bf16 added to
 * the result (the block's q + xattn(...)); out: [B,NQ,H*hd] bf16; lse2: [B,H,NQ] fp32 (nullable in inference).
 * Matrix-vector work, HBM-bound: 4*N*hd bytes per (sample, head, query) forward, 12*N*hd backward.  The reference's
 * `proj` Linear of CrossAttention is never applied (modules.py:156-157) and is not applied here. */
int vj_xattn_fwd(const void* q, int64_t q_bstride, const void* kv, const void* resid, void* out, float* lse2, int64_t B,
                 int64_t NQ, int64_t N, int64_t H, int64_t hd, float scale, vj_stream_t stream);
/* dq [B,H*hd] bf16 (per sample; the caller sums over the batch when the query is shared), dkv [B,N,2,H,hd] bf16
 * <- (dy [B,1,H*hd] bf16, saved q, kv, lse2).  NQ must be 1. */
int vj_xattn_bwd(const void* q, int64_t q_bstride, const void* kv, const void* dy, const float* lse2, void* dq, void* dkv,
                 int64_t B, int64_t NQ, int64_t N, int64_t H, int64_t hd, float scale, vj_stream_t stream);
/* The two calls above keep every score of a (sample, head) in LDS and refuse more keys than that holds (forward N <= 38 264,
 * backward N <= 19 132).  The _ws forms take the same arguments plus a workspace and have no key limit: within those limits they
 * run the same kernels (same bits, ws_bytes 0); above them, split-key kernels (fixed 2048-key chunks, fp32 partials in ws merged in
 * ascending chunk order, no atomics: deterministic).  vj_xattn_ws_bytes(backward = 0 / 1) is the workspace size (0 when none is
 * needed, < 0 for bad dimensions).  Split backward: 10*N*hd + 16*N bytes per (sample, head). */
int64_t vj_xattn_ws_bytes(int64_t B, int64_t NQ, int64_t N, int64_t H, int64_t hd, int backward);
int vj_xattn_fwd_ws(const void* q, int64_t q_bstride, const void* kv, const void* resid, void* out, float* lse2, int64_t B,
                    int64_t NQ, int64_t N, int64_t H, int64_t hd, float scale, void* ws, int64_t ws_bytes, vj_stream_t stream);
int vj_xattn_bwd_ws(const void* q, int64_t q_bstride, const void* kv, const void* dy, const float* lse2, void* dq, void* dkv,
                    int64_t B, int64_t NQ, int64_t N, int64_t H, int64_t hd, float scale, void* ws, int64_t ws_bytes,
                    vj_stream_t stream);

/* ---- predictor token assembly (predictor.py:194-221) --------------------------------------------------------
 * out[b, j<Ke] = embed[b,j] + pos[idx_e[b,j]];  out[b, Ke+j] = mask_token + pos[idx_p[b,j]] */
int vj_pred_assemble_fwd(const void* e_bf16, const float* mask_token, const float* pos, const int64_t* idx_e,
                         const int64_t* idx_p, void* out_bf16, int64_t B, int64_t Ke, int64_t Kp, int64_t D,
                         vj_stream_t stream);

/* ---- targets and loss (app/vjepa/train.py:419-459) ----------------------------------------------------------
 * h[b,k,:] = F.layer_norm( norm(x)[b, idx[b,k], :] ), fp32 out: final encoder LayerNorm (eps_norm), the
 * affine-free F.layer_norm (eps_ln = 1e-5, train.py:426) and apply_masks fused over the predicted rows only. */
int vj_target_rows(const void* x_bf16, const float* gamma, const float* beta, const int64_t* idx, float* h,
                   int64_t B, int64_t N, int64_t K, int64_t D, float eps_norm, float eps_ln, vj_stream_t stream);
/* loss_out (+)= out_scale * sum(|z-h|^p / p); dz (nullable) = sign(z-h)|z-h|^(p-1) * gscale  (train.py:440-446) */
int64_t vj_latent_loss_ws_bytes(void);
int vj_latent_loss(const void* z_bf16, const float* h, void* dz_bf16, int64_t numel, float p, float gscale,
                   float out_scale, int accumulate, float* loss_out, void* ws, int64_t ws_bytes,
                   vj_stream_t stream);
/* reg_fn (train.py:448-449,458): pstd[b,d] (+)= sqrt(var_k z[b,k,d] + 1e-4); reg = mean(relu(1 - pstd/n_masks)) */
int vj_token_pstd(const void* z_bf16, float* pstd, float* stats /* nullable [B,D,2] = {mean, sqrt(var+eps)} */,
                  int64_t B, int64_t K, int64_t D, int accumulate, vj_stream_t stream);
/* backward of the regulariser: dz -= coef * 1[pstd_sum/n_masks < 1] * (z - mean) / ((K-1) * sqrt(var+eps)) */
int vj_reg_grad(const void* z_bf16, const float* pstd_sum, const float* stats, void* dz_bf16, int64_t B, int64_t K,
                int64_t D, int64_t n_masks, float coef, vj_stream_t stream);
int vj_reg_finish(const float* pstd_sum, int64_t n, int64_t n_masks, float* out, vj_stream_t stream);

/* ---- parameter update over flat fp32 arenas (train.py:461-487; app/vjepa/utils.py:156-210) -------------------
 * torch.optim.AdamW step (decoupled wd, bias correction from `step`), EMA of the target encoder
 * (param_k = m*param_k + (1-m)*param_q, train.py:486-487) and the bf16 re-cast of both weight sets, one pass.
 * p_bf16 / tgt / tgt_bf16 are nullable; gscale pre-multiplies the gradient (clip coefficient). n % 4 == 0. */
int vj_adamw_ema(float* p, const float* g, float* exp_avg, float* exp_avg_sq, void* p_bf16, float* tgt,
                 void* tgt_bf16, int64_t n, float lr, float wd, float beta1, float beta2, float eps, int64_t step,
                 float gscale, float ema, vj_stream_t stream);
/* Device-guarded form of the same update: nothing between backward and update needs the host.
 *   gstat = [sumsq_enc, nonfinite_enc, sumsq_pred, nonfinite_pred] (device; two vj_sqnorm_f32 results);
 *   any non-finite gradient -> AdamW is skipped for every range (GradScaler.step, train.py:471; utils.py:209) while the
 *   EMA still runs; clip > 0 applies torch.nn.utils.clip_grad_norm_'s coefficient min(1, clip/(norm+1e-6)) with
 *   norm = sqrt(gstat[2*sel]) * norm_scale (train.py:468-470); the Adam step count t is the device float *step_dev,
 *   advanced by vj_step_advance only when the step is not skipped. */
int vj_step_advance(const float* gstat, float* step_dev, vj_stream_t stream);
int vj_adamw_ema_guarded(float* p, const float* g, float* exp_avg, float* exp_avg_sq, void* p_bf16, float* tgt,
                         void* tgt_bf16, int64_t n, float lr, float wd, float beta1, float beta2, float eps, float gscale,
                         float ema, const float* gstat, int sel, float clip, float norm_scale, const float* step_dev,
                         vj_stream_t stream);
/* Logging statistics without per-tensor host syncs (grad_logger / adamw_logger, src/utils/logging.py:91-118;
 * train.py:476-481): desc = device int64 [n_tensors][2] {element offset (multiple of 4), numel} into the flat arenas;
 * out = device fp32 [n_tensors][vj_grad_stats_chunks()][3] partial sums of {g^2, |exp_avg|, |exp_avg_sq|}
 * (M1 = M2 = NULL: gradients only).  One launch; evaluated by the caller only when a log line is due. */
int64_t vj_grad_stats_chunks(void);
int vj_grad_stats_multi(const float* G, const float* M1, const float* M2, const int64_t* desc, int64_t n_tensors,
                        float* out, vj_stream_t stream);
int vj_ema_update(float* tgt, const float* src, void* tgt_bf16, int64_t n, float m, vj_stream_t stream);
int vj_cast_f32_to_bf16(const float* src, void* dst_bf16, int64_t n, vj_stream_t stream);
/* out2[0] (+)= sum g^2, out2[1] (+)= count of non-finite values  (clip_grad_norm_, GradScaler inf check) */
int64_t vj_sqnorm_ws_bytes(void);
int vj_sqnorm_f32(const float* g, int64_t n, float* out2, int accumulate, void* ws, int64_t ws_bytes,
                  vj_stream_t stream);

/* ---- whole-trunk launch chains (host-side sequencing only; no arithmetic of their own) ------------------------
 * N transformer blocks, forward or backward, enqueued by ONE call: Block.forward / Attention.forward / MLP.forward
 * (src/models/utils/modules.py:30-36,61-78,114-120) as the loops of VisionTransformer.forward
 * (src/models/vision_transformer.py:181-184) and VisionTransformerPredictor.forward (src/models/predictor.py:231-232)
 * run them, and the autograd graph that loss.backward() (app/vjepa/train.py:461-464) walks over them.
 * Token rows of several equal-length sequence groups (one per mask) are concatenated along M; `segs` describes them
 * (attention is launched per segment, everything else over all M rows).
 * All buffers are borrowed; workspaces are caller-allocated, 256-byte aligned, sized by the *_ws_bytes queries. */
typedef struct vj_linear {
  const void* w;    /* bf16 [n_out, k_in]                                   (forward operand)              */
  const float* b;   /* fp32 [n_out] or NULL                                                                  */
  const void* wT;   /* bf16 [k_in, ldwT >= n_out] transposed shadow          (dgrad operand; NULL = fwd only) */
  int64_t ldwT;
  float* gw;        /* fp32 [n_out, k_in] weight-gradient view               (NULL = fwd only)                */
  float* gb;        /* fp32 [n_out] bias-gradient view or NULL                                               */
  int64_t n_out, k_in;
} vj_linear_t;
typedef struct vj_norm {
  const float* g;
  const float* b;
  float* gg; /* gradient views, NULL = fwd only */
  float* gb;
} vj_norm_t;
typedef struct vj_block {
  vj_norm_t norm1;
  vj_linear_t qkv, proj;
  vj_norm_t norm2;
  vj_linear_t fc1, fc2;
} vj_block_t;
/* (vj_seg_t: declared with the attention entry points above) */
typedef void (*vj_layer_cb_t)(void* user, int layer);

/* save != 0: every block keeps what its backward needs (16*D bf16 per token: x, LN1 out, qkv, o, x1, LN2 out,
 * pre-GELU u, GELU out + row statistics + softmax lse) in `ws`; save == 0: one such set is reused by all blocks. */
int64_t vj_blocks_fwd_ws_bytes(int64_t M, int64_t D, int64_t Dh, int64_t heads, int64_t n_blocks, int save);
/* x_out [M,D] bf16 = blocks[n-1](...blocks[0](x_in)) ; x_in must stay valid until the backward has run.
 * gemm_flags: kernel selection for the four Linear GEMMs of every block, as in vj_gemm_bf16_nt (0 = automatic;
 * 0x100 = the two-workgroups-per-CU kernel, the better choice when this stream has the GPU to itself: inference).
 * The fields of gemm_flags: the selection, and the first block it applies to (earlier blocks take the automatic choice). */
enum {
  VJ_GEMM_FLAGS_SEL_MASK = 0xffff, /* low 16 bits: kernel selection of vj_gemm_bf16_nt (0: option "gemm_fwd_flags") */
  VJ_GEMM_FLAGS_FROM_SHIFT = 16,   /* bits 16-23: first block the selection applies to */
  VJ_GEMM_FLAGS_FROM_MASK = 0xff
};
int vj_blocks_fwd(const vj_block_t* blocks, int64_t n_blocks, const void* x_in, void* x_out, int64_t M, int64_t D,
                  int64_t heads, const vj_seg_t* segs, int64_t n_segs, float ln_eps, int save, int gemm_flags, void* ws,
                  int64_t ws_bytes, vj_stream_t stream);
/* The same trunk for blocks that never run backward (the EMA target encoder of train.py:419-429, frozen-encoder inference) with both
 * LayerNorms of every block FOLDED into the Linear that consumes them (modules.py:115,119 -> 63 / 31): a statistics pass reads the
 * residual stream (vj_ln_rowstats), the qkv / fc1 GEMM reads it too and applies rstd_m * (acc - mean_m * c_n) + b'_n in its epilogue
 * (vj_gemm_bf16_nt_lnfold) -- the LayerNorm output is never written or re-read.  folds[i]: block i's folded weights, prepared by
 * vj_ln_fold_weights from the fp32 weights once per optimizer step.  Workspace: vj_blocks_fwd_ws_bytes(..., save = 0). */
typedef struct vj_lnfold {
  const void* w_qkv;    /* bf16 [3D, D] = bf16(W_qkv * diag(norm1.weight)) */
  const float* c_qkv;   /* [3D]  row sums of w_qkv */
  const float* b_qkv;   /* [3D]  qkv.bias + W_qkv norm1.bias */
  const void* w_fc1;    /* bf16 [Dh, D] = bf16(W_fc1 * diag(norm2.weight)) */
  const float* c_fc1;   /* [Dh] */
  const float* b_fc1;   /* [Dh]  fc1.bias + W_fc1 norm2.bias */
} vj_lnfold_t;
int vj_blocks_fwd_lnfold(const vj_block_t* blocks, const vj_lnfold_t* folds, int64_t n_blocks, const void* x_in, void* x_out,
                         int64_t M, int64_t D, int64_t heads, const vj_seg_t* segs, int64_t n_segs, float ln_eps, int gemm_flags,
                         void* ws, int64_t ws_bytes, vj_stream_t stream);
/* the pieces (also usable alone): rowstats[m] = {rstd_m, -mean_m * rstd_m} of bf16 rows (fp32, two passes in registers, biased
 * variance + eps: nn.LayerNorm's statistics); folded weights Wf = bf16(W diag(gamma)), cvec[n] = sum_k Wf[n,k], bf = b + W beta;
 * C = LayerNorm(X) W^T + b from the raw rows X (epilogue 0 bf16, 1 GELU, 4 bf16 with the first N/3 columns times alpha) */
int vj_ln_rowstats(const void* x_bf16, float* rowstats, int64_t rows, int64_t D, float eps, vj_stream_t stream);
int vj_ln_fold_weights(const float* W, const float* b, const float* gamma, const float* beta, void* Wf_bf16, float* cvec, float* bf,
                       int64_t N, int64_t K, vj_stream_t stream);
int vj_gemm_bf16_nt_lnfold(const void* X, int64_t ldx, const void* Wf, int64_t ldw, void* C, int64_t ldc, int64_t M, int64_t N,
                           int64_t K, const float* bias_f, const float* rowstats, const float* colsum_w, int epilogue, float alpha,
                           int flags, vj_stream_t stream);
int64_t vj_blocks_bwd_ws_bytes(int64_t M, int64_t D, int64_t Dh, int64_t heads);
/* dx_out [M,D] bf16 = d loss / d x_in given dout = d loss / d x_out; parameter gradients are written as
 * alpha * grad + beta_acc * old into the fp32 views of `blocks` (beta_acc = 1 accumulates micro-batches).
 * The dgrad chain runs on `stream`; weight / bias gradients (and the operand transposes feeding them) run on `side`
 * (NULL = same stream), ordered by events; on return `side` may still hold pending work -- make the consumer of the
 * gradients wait on it.  on_layer_done(user, l) (nullable) is called from the enqueueing thread as soon as block l's
 * backward has been enqueued on both streams (gradient-bucket launch hook, DDP equivalent of train.py:295-297).
 * flags bit0: transpose-free weight gradients (vj_gemm_bf16_tn_splitk; with option "wgrad_group" the four of a block
 * in one vj_gemm_bf16_tn_grouped launch once the block's last dY exists).
 * flags bit1: the caller already wrote the LAST block's fc2 bias gradient (the column sums of dout; it comes out of the
 * LayerNorm backward that produced dout, vj_layernorm_bwd_colsum) -- with the transpose-free route only.
 * flags bits 2-3: bit 3 set = "bit 2 tells whether the forward stored q pre-scaled by scale*log2(e)" (what vj_blocks_fwd does under
 * option "attn_softmax" = 2 when D % 4 == 0); callers record the convention at forward time and pass it here, so that an option change
 * between a forward and its backward cannot make the backward read the saved qkv with the wrong convention.  Bit 3 clear: the option is
 * read again at backward time (only right if it did not change).
 * With the transpose-free route and option "bias_fuse" (default) the bias gradients of qkv and fc1 come from column partials of
 * the kernels that produce dqkv / du (vj_attn_bwd_colsum, vj_gemm_bf16_nt_dgelu_colsum) and every partial reduction of a block
 * (both LayerNorms', those two) is ONE vj_reduce_segments launch at the end of the block. */
enum {
  VJ_BWD_FORCE_TN = 1,           /* flags bit0 */
  VJ_BWD_LAST_FC2_BIAS_DONE = 2, /* flags bit1 */
  VJ_BWD_Q_PRESCALED = 4,        /* flags bit2: read only with bit3 */
  VJ_BWD_Q_PRESCALED_VALID = 8   /* flags bit3 */
};
int vj_blocks_bwd(const vj_block_t* blocks, int64_t n_blocks, const void* x_in, const void* dout, void* dx_out, int64_t M,
                  int64_t D, int64_t heads, const vj_seg_t* segs, int64_t n_segs, float alpha, float beta_acc,
                  const void* save_ws, int64_t save_ws_bytes, void* tmp_ws, int64_t tmp_ws_bytes, int flags,
                  vj_stream_t stream, vj_stream_t side, vj_layer_cb_t on_layer_done, void* user);

/* ---- per-launch timing of the chains' GEMM / attention launches (HIP events on the launch stream) -------------
 * vj_prof_enable(1) starts recording; vj_prof_collect synchronises and sums per family (0 GEMM, 1 attention forward,
 * 2 attention backward): ms[3], flop[3], launches[3]; csv_path (nullable) receives one line per launch. */
int vj_prof_enable(int on);
int vj_prof_collect(double* ms, double* flop, int64_t* launches, const char* csv_path);

/* ---- gradient collective over RCCL / xGMI -------------------------------------------------------------------
 * DistributedDataParallel's gradient averaging (app/vjepa/train.py:295-297; src/utils/distributed.py:18-47) for hosts
 * without torch.distributed: one process per GPU, SUM all-reduce of slices ("buckets") of the flat fp32 gradient arena
 * on a communication stream the caller orders against the backward with events (the mean is folded into the fused
 * AdamW kernel's gscale = 1/world, see vj_adamw_ema_guarded).  librccl.so is dlopen()ed on first use (the copy already
 * mapped by the process, e.g. PyTorch's, is reused).  Rank 0 calls vj_comm_unique_id and ships the
 * vj_comm_unique_id_bytes() = 128 bytes to the other ranks out of band; every rank then calls vj_comm_init on its own
 * current HIP device.  The Python engine (jepa_amd/engine/dp.py) keeps using torch.distributed's RCCL backend by
 * default -- same library, same collectives -- so that it shares the launcher's process group. */
typedef struct vj_comm_opaque* vj_comm_t;
int64_t vj_comm_unique_id_bytes(void);
int vj_comm_unique_id(void* id_out);
int vj_comm_init(vj_comm_t* comm_out, int rank, int world, const void* id);
int vj_comm_allreduce_bucket(vj_comm_t comm, float* grad, int64_t count, vj_stream_t stream);   /* in place, SUM */
int vj_comm_broadcast(vj_comm_t comm, float* buf, int64_t count, int root, vj_stream_t stream);  /* parameter sync */
int vj_comm_destroy(vj_comm_t comm);

/* ---- run-time tuning switches ------------------------------------------------------------------------------
 * Named integer options that choose between kernels computing the same result (A/B measurements interleaved in one
 * process, tools/abab.py): "gemm_fwd_flags", "gemm_dgrad_flags", "gemm_4w", "gemm_persist", "wgrad_tn",
 * "wgrad_group", "gemm_dbg", "attn_softmax", "bias_fuse", "gemm_raster", "ws_guard", "gemm_epi_pre" (twelve; meaning, default
 * and accepted values of each: jepa_amd/csrc/options.hpp / options.cpp; forms that were measured and removed live as patches
 * under lab/patches/).  Initial value: environment variable VJ_<NAME IN UPPER CASE>, else
 * the built-in default.  Unknown names are an argument error.  The reference has no counterpart (it has no kernels). */
int vj_set_option(const char* name, int value);
int vj_get_option(const char* name, int* value);

/* Diagnostics (tests only).  With option "ws_guard" = 1 every member of the two chain workspaces (saved activations, backward
 * temporaries, column partials, split-K partials) is followed by a 256-byte gap that vj_blocks_fwd / vj_blocks_bwd fill with a byte
 * pattern before their first kernel; vj_ws_guard_check synchronises the device and reports how many distinct gaps were poisoned
 * since the last call and how many of them no longer hold the pattern (a write past the end of a workspace member).  No reference
 * counterpart. */
int vj_ws_guard_check(int64_t* n_checked, int64_t* n_bad);

/* ---- bank of attentive probes on one frozen forward pass (AttentiveClassifierBank) -----------------------------
 * P probes with ONE query token each, shared by the batch: the scores of every (probe, head) are one column of
 * S = x_hat U^T (fp32 [B, N, C], C = P * heads padded to a multiple of 4 with zero rows of U), so neither K nor V of
 * CrossAttention.forward (src/models/utils/modules.py:145-148) is materialised.
 * vj_pool_softmax_fwd replaces `F.scaled_dot_product_attention`'s soft-max over the keys (modules.py:150-153) for all columns
 * at once: A = bf16(softmax over n of S[b, n, c]), lse[b, c] = log sum_n exp S (fp32).  The column maximum is subtracted
 * before the exponential (finite S never gives a NaN; an all-zero padded column gives the uniform distribution).  Keys are
 * split into vj_pool_softmax_chunk_keys() chunks whose partial (max, sum) pairs go through ws and are merged in ascending chunk
 * order: no atomics, run-to-run bitwise equal.  ws_bytes >= vj_pool_softmax_fwd_ws_bytes(B, N, C) (< 0 for bad dimensions).
 * vj_pool_softmax_bwd replaces the soft-max backward autograd runs there: dS = bf16(A * (dA - delta[b, c])), dA fp32
 * [B, N, C], delta fp32 [B, C] = sum_n A dA (the caller has it as dZ . Z).
 * C % 4 == 0, B <= 65535, N <= 65535 chunks; fp32 buffers 16-byte aligned, bf16 buffers 8-byte aligned; every argument is
 * checked on the host before any launch. */
int64_t vj_pool_softmax_chunk_keys(void);
int64_t vj_pool_softmax_fwd_ws_bytes(int64_t B, int64_t N, int64_t C);
int vj_pool_softmax_fwd(const float* S, void* A_bf16, float* lse, int64_t B, int64_t N, int64_t C, void* ws, int64_t ws_bytes,
                        vj_stream_t stream);
int vj_pool_softmax_bwd(const void* A_bf16, const float* dA, const float* delta, void* dS_bf16, int64_t B, int64_t N, int64_t C,
                        vj_stream_t stream);

/* ---- hardware probes (tests / profiles only) ---------------------------------------------------------------- */
int vj_probe_tr16(uint32_t* out256, int addr_scale, vj_stream_t stream);
int vj_probe_copy(const void* src, void* dst, int64_t bytes, vj_stream_t stream);
/* LDS read throughput of a CU, 8 waves x iters x 8 back-to-back reads: mode 0 ds_read_b128, 1 ds_read_b64_tr_b16 (the TN
 * GEMM's fragment addressing), 2 ds_read_b64; out[wg*8 + wave] = clock64 cycles (100 MHz timer ticks on gfx9) */
int vj_probe_lds_bw(long long* out, int mode, int iters, int n_wgs, vj_stream_t stream);
/* one wave idling for `ticks` periods of the 100 MHz timer: two of them on two streams take one spin time iff the streams are
 * mapped to different hardware queues (used once per process to pick independent side / update / communication streams) */
int vj_probe_spin(int64_t ticks, vj_stream_t stream);
/* the same kernel leaving {start, end} of its spin on the chip-wide 100 MHz timer in stamps[0..1] (device memory): two of them on two
 * streams overlap ON THE DEVICE'S CLOCK iff the streams sit on different hardware queues; no host timing involved (what
 * engine/layers.py streams_concurrent uses since round 6).  No reference counterpart. */
int vj_probe_spin_stamped(int64_t ticks, int64_t* stamps, vj_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VJEPA_HIP_H */
