"""Clip and frame aggregation of the frozen video-classification eval (evals/video_classification_frozen/utils.py:22-159).

ClipAggregation keeps the reference's constructor, attributes and forward contract: the input is a list over segments of lists
over views of [B,C,T,H,W] clips; the output is a list over views of [B, S*N, D] (attend_across_segments) or a list over views of
lists over segments of [B, N, D].  The frozen encoder runs on every clip in the reference's order (segment-major, then view, then
sample) and the per-view concatenation is written by the bit-exact row copy (vj_copy_rows) straight into one bf16 buffer per
view.

`make_transforms`, `VideoTransform` and `EvalVideoTransform` (utils.py:162-323) keep the reference's names, signatures and DRAWS and
do no pixel work: they take decoded uint8 [T,H,W,3] frames and return a `RawClip` (app/vjepa/transforms.py) in the eval's
normalise-first form -- the frames as they came, the crop boxes of every view, the flip, the RandomErasing box and noise -- and
`engine.input.EvalPrefetcher` makes the fp32 views on the device (vj_clip_transform_pre, vj_clip_erase).  RandAugment is opt-in
behind the attribute `VideoTransform.rand_augment` (a `RandAugmentDraw` of app/vjepa/randaugment.py: the plan is drawn first, as
the reference augments first, and vj_clip_randaug carries it out on the uint8 frames on the device).  The short-side resize of the
two validation forms is opt-in too, behind the attribute `device_resize` of both (default False: frames must arrive with that short
side, and anything else raises): the RawClip then names the size the reference's Resize would give, vj_clip_resample makes it on
the device as PIL's antialiased Image.resize(BILINEAR) does -- what the reference applies to PIL frames
(src/datasets/utils/video/functional.py:52-67) --, and the boxes refer to the resized frames.  The reference's decord frames are
numpy arrays and go through cv2.INTER_LINEAR instead, which is not antialiased; that arithmetic is not implemented.  Out of scope,
raising: `auto_augment=True` in the constructors (PIL RandAugment on the CPU).  The decord loader behind the transforms is not part
of this package; src/datasets/frame_folder.py reads videos stored as frames.
"""
import numpy as np
import torch
import torch.nn as nn

from ...app.vjepa.transforms import RawClip, draw_erase
from ...app.vjepa.transforms import VideoTransform as _PretrainVideoTransform
from ...hip import ops
from ...src.models.utils.pos_embs import get_1d_sincos_pos_embed
from ..frozen import chunked_call, max_clips_per_call, widest_activation


class FrameAggregation(nn.Module):
    """Process each frame independently and concatenate all tokens (utils.py:23-83), for this package's image (num_frames=1)
    VisionTransformer.  Like the reference it always returns the concatenated layout: a list over views of [B, S*T*N, D].

    The reference's [B*T,C,H,W] permuted copy of the frames is never made: the image encoder packs the patch rows straight from
    the [B,C,T,H,W] clips (VisionTransformer.forward_frames), several clips per trunk call, each call small enough that its widest
    activation stays below 2^31 elements (max_tokens_per_call token rows), and the segments are written into the per-view output
    by the bit-exact row copy (vj_copy_rows).  The temporal position embedding is one in-place pass per view (vj_add_pos_frames)."""

    def __init__(self, model, max_frames=10000, use_pos_embed=False, attend_across_segments=False):
        from ...src.models.vision_transformer import VisionTransformer
        if not isinstance(model, VisionTransformer) or model.is_video:
            raise NotImplementedError("FrameAggregation drives the frames entry of this package's image (num_frames=1) "
                                      "VisionTransformer (forward_frames); other encoders are not supported")
        super().__init__()
        self.model = model
        self.embed_dim = embed_dim = model.embed_dim
        self.num_heads = model.num_heads
        self.attend_across_segments = attend_across_segments
        # 1D-temporal pos-embedding
        self.pos_embed = None
        if use_pos_embed:
            self.pos_embed = nn.Parameter(torch.zeros(1, max_frames, embed_dim), requires_grad=False)
            sincos = get_1d_sincos_pos_embed(embed_dim, max_frames)
            self.pos_embed.data.copy_(torch.from_numpy(sincos).float().unsqueeze(0))
        # encoder call size in token rows: fc1's output of one call stays below 2^31 elements
        self.max_tokens_per_call = max_clips_per_call(widest_activation(model), 1)

    def _pieces(self, x, frames_per_call):
        """(clips [b,C,t,H,W], view, first sample, first frame of the output) in the reference's order, none above frames_per_call
        frames: whole (segment, view) tensors where they fit, else runs of samples, else runs of frames of one sample.  Segments
        follow one another along time, each with its own length, as the reference's torch.cat(x, dim=2) lays them out."""
        first = 0
        for xi in x:
            for j, c in enumerate(xi):
                B, T = c.shape[0], c.shape[2]
                if frames_per_call >= T:
                    step = frames_per_call // T
                    for b0 in range(0, B, step):
                        yield c[b0:b0 + step], j, b0, first
                else:
                    for b0 in range(B):
                        for t0 in range(0, T, frames_per_call):
                            yield c[b0:b0 + 1, :, t0:t0 + frames_per_call], j, b0, first + t0
            first += xi[0].shape[2]

    def forward(self, x, clip_indices=None):
        num_views_per_clip = len(x[0])
        # what the reference's two torch.cat calls require: views of one shape, segments that differ in length only
        frame = lambda c: (c.dim(),) + tuple(c.shape[:2] + c.shape[3:])      # noqa: E731
        if x[0][0].dim() != 5 or any(len(xi) != num_views_per_clip or any(c.shape != xi[0].shape for c in xi)
                                     or frame(xi[0]) != frame(x[0][0]) for xi in x):
            raise ValueError(f"FrameAggregation: segments of {num_views_per_clip} views of [B,C,T,H,W] clips that differ in T "
                             f"only are expected, got {[[tuple(c.shape) for c in xi] for xi in x]}")
        B, C, _, H, W = x[0][0].shape
        p = self.model.patch_size
        N, D = (H // p) * (W // p), self.embed_dim
        F = sum(xi[0].shape[2] for xi in x)
        device = x[0][0].device
        idx = None
        if (self.pos_embed is not None) and (clip_indices is not None):
            idx = torch.cat([ci.reshape(B, -1) for ci in clip_indices], dim=1).to(torch.int64)   # [B, S*T], shared by all views
            lo, hi = (int(v) for v in torch.stack([idx.min(), idx.max()]).tolist()) if idx.numel() else (0, 0)
            if idx.shape[1] != F or lo < 0 or hi >= self.pos_embed.shape[1]:
                raise ValueError(f"FrameAggregation: clip_indices {tuple(idx.shape)} in [{lo}, {hi}] do not index {F} frames of a "
                                 f"temporal table of {self.pos_embed.shape[1]} rows")
            idx = idx.to(device).contiguous()
        outs = [torch.empty((B, F * N, D), dtype=torch.bfloat16, device=device) for _ in range(num_views_per_clip)]
        cap = max(1, self.max_tokens_per_call // max(N, 1))     # frames per encoder call
        call, frames = [], 0

        def flush():
            feats = self.model.forward_frames([c for c, _, _, _ in call])
            for (c, j, b0, f0), f in zip(call, feats):
                n = c.shape[2] * N
                ops.copy_rows(f, outs[j][b0:b0 + c.shape[0]], c.shape[0], n, 0, F * N, f0 * N, n, D)

        for piece in self._pieces(x, cap):
            n = piece[0].shape[0] * piece[0].shape[2]
            if call and frames + n > cap:
                flush()
                call, frames = [], 0
            call.append(piece)
            frames += n
        if call:
            flush()
        if idx is not None:
            pos = self.pos_embed.detach()[0].to(device=device, dtype=torch.float32).contiguous()
            for o in outs:
                ops.add_pos_frames(o, pos, idx, N)
        return outs


class _PlaceSegments(torch.autograd.Function):
    """ClipAggregation's concatenated form as an autograd node: bf16 features f [S*V*B, N, D] of ONE encoder call (clip
    i*V*B + j*B + b is segment i of view j of sample b) -> V tensors [B, S*N, D], by the row copy the frozen path places them
    with (vj_copy_rows).  The backward is the inverse copy: no torch.cat copies of the features either way."""

    @staticmethod
    def forward(ctx, f, S, V, B):
        N, D = f.shape[1], f.shape[2]
        outs = [torch.empty((B, S * N, D), dtype=f.dtype, device=f.device) for _ in range(V)]
        for i in range(S):
            for j in range(V):
                c = (i * V + j) * B
                ops.copy_rows(f[c:c + B], outs[j], B, N, 0, S * N, i * N, N, D)
        ctx.dims = (S, V, B, N, D)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *douts):
        S, V, B, N, D = ctx.dims
        ref = next(d for d in douts if d is not None)
        df = torch.empty((S * V * B, N, D), dtype=ref.dtype, device=ref.device)
        for j, d in enumerate(douts):
            d = None if d is None else d.contiguous()
            for i in range(S):
                c = (i * V + j) * B
                if d is None:       # a view no loss reads
                    df[c:c + B].zero_()
                else:
                    ops.copy_rows(d, df[c:c + B], B, S * N, i * N, N, 0, N, D)
        return df, None, None, None


class ClipAggregation(nn.Module):
    """Process each clip independently and concatenate all tokens (utils.py:84-159).  With a trainable encoder and gradients
    enabled (fine-tuning) the clips of a batch go through ONE encoder call, whose output stays on the autograd graph."""

    def __init__(self, model, tubelet_size=2, max_frames=10000, use_pos_embed=False, attend_across_segments=False):
        super().__init__()
        self.model = model
        self.tubelet_size = tubelet_size
        self.embed_dim = model.embed_dim
        self.num_heads = model.num_heads
        self.attend_across_segments = attend_across_segments
        if use_pos_embed:
            raise NotImplementedError("ClipAggregation(use_pos_embed=True): the temporal position embedding is not "
                                      "implemented; no shipped eval config sets it (eval.py:172-176)")
        self.pos_embed = None
        # encoder call size: fc1's output of one call stays below 2^31 elements (91 clips for ViT-H/16 at 384)
        self.max_clips_per_call = max_clips_per_call(widest_activation(model), model.num_patches)

    def _bf16(self, x):
        f = self.model(x)
        return f if f.dtype == torch.bfloat16 else f.to(torch.bfloat16)

    def forward(self, x, clip_indices=None):
        num_clips = len(x)
        num_views_per_clip = len(x[0])
        B = x[0][0].shape[0]
        eff_B = B * num_views_per_clip
        # all spatial and temporal views along the batch dimension, in the reference's order
        x = torch.cat([torch.cat(xi, dim=0) for xi in x], dim=0)
        needs_grad = getattr(self.model, "_needs_grad", None)
        if needs_grad is not None and needs_grad():
            return self._forward_with_grad(x, num_clips, num_views_per_clip, B)
        if not self.attend_across_segments:
            f = chunked_call(self._bf16, x, self.max_clips_per_call)
            return [[f[i * eff_B + j * B:i * eff_B + (j + 1) * B] for i in range(num_clips)] for j in range(num_views_per_clip)]
        # bf16 [m, N, D] of each encoder call of at most max_clips_per_call clips, with its first clip
        feats = [(c0, self._bf16(x[c0:c0 + self.max_clips_per_call])) for c0 in range(0, x.shape[0], self.max_clips_per_call)]
        N, D = feats[0][1].shape[1], feats[0][1].shape[2]
        # segment i of view j of sample b is clip i*eff_B + j*B + b; its tokens go to rows [i*N, (i+1)*N) of sample b of view j
        outs = [torch.empty((B, num_clips * N, D), dtype=torch.bfloat16, device=feats[0][1].device)
                for _ in range(num_views_per_clip)]
        for c0, f in feats:
            k, m = 0, f.shape[0]
            while k < m:   # runs of consecutive clips of one (segment, view)
                g = c0 + k
                i, j, b = g // eff_B, (g % eff_B) // B, g % B
                n = min(B - b, m - k)
                ops.copy_rows(f[k:k + n], outs[j][b:b + n], n, N, 0, num_clips * N, i * N, N, D)
                k += n
        return outs


    def _forward_with_grad(self, x, num_clips, num_views_per_clip, B):
        """The same outputs with a backward recorded: one encoder call for all clips (a second call would overwrite the gradient
        slots the first one's backward writes), slices of it or, concatenated, _PlaceSegments."""
        if x.shape[0] > self.max_clips_per_call:
            raise ValueError(f"ClipAggregation: {x.shape[0]} clips with gradients enabled need one encoder call, and one call takes "
                             f"at most max_clips_per_call = {self.max_clips_per_call} clips (fc1's output stays below 2^31 "
                             "elements); use a smaller batch or fewer segments")
        f = self._bf16(x)
        eff_B = B * num_views_per_clip
        if not self.attend_across_segments:
            return [[f[i * eff_B + j * B:i * eff_B + (j + 1) * B] for i in range(num_clips)] for j in range(num_views_per_clip)]
        return list(_PlaceSegments.apply(f, num_clips, num_views_per_clip, B))


def make_transforms(
    training=True,
    random_horizontal_flip=True,
    random_resize_aspect_ratio=(3/4, 4/3),
    random_resize_scale=(0.3, 1.0),
    reprob=0.0,
    auto_augment=False,
    motion_shift=False,
    crop_size=224,
    num_views_per_clip=1,
    normalize=((0.485, 0.456, 0.406),
               (0.229, 0.224, 0.225))
):
    if not training and num_views_per_clip > 1:
        return EvalVideoTransform(num_views_per_clip=num_views_per_clip, short_side_size=crop_size, normalize=normalize)
    return VideoTransform(
        training=training, random_horizontal_flip=random_horizontal_flip, random_resize_aspect_ratio=random_resize_aspect_ratio,
        random_resize_scale=random_resize_scale, reprob=reprob, auto_augment=auto_augment, motion_shift=motion_shift,
        crop_size=crop_size, normalize=normalize)


def _uint8_frames(buffer, who):
    frames = torch.as_tensor(np.asarray(buffer) if isinstance(buffer, (list, tuple)) else buffer)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError(f"{who}: expected a uint8 [T,H,W,3] buffer, got {frames.dtype} {tuple(frames.shape)}")
    return frames.contiguous()


def _normalize_constants(normalize):
    """mean and std as the fp32 values the reference holds (torch.tensor(normalize), 0..1 units), as Python floats."""
    t = torch.tensor(normalize, dtype=torch.float32)
    return tuple(t[0].tolist()), tuple(t[1].tolist())


def _resize_sizes(H, W, size):
    """(OH, OW) the reference's short-side Resize leaves (src/datasets/utils/video/functional.py:74-81): the short side becomes
    `size`, the long one int(size * long / short); None when the short side already is `size` (functional.py:55-58 returns the
    frames as they are)."""
    if min(H, W) == size:
        return None
    return (int(size * H / W), size) if W < H else (size, int(size * W / H))


def _require_short_side(H, W, want, who):
    if min(H, W) != want:
        raise ValueError(f"{who}: frames of {H}x{W} do not have the short side {want} that the reference's Resize would leave; the "
                         "bilinear short-side resize is the loader's job (it is not done on the device), so hand in frames whose "
                         f"short side is {want}")


class VideoTransform(object):
    """The reference's eval VideoTransform (utils.py:199-283) as draws.  training=True: the random-resized-crop box (or two, with
    motion shift), the flip and the RandomErasing box and noise, in the reference's order on the global generators; the device
    normalises every source pixel first and resizes after.  training=False: the centre crop of frames whose short side already is
    int(crop_size * 256 / 224).  Either way the call returns one `RawClip` (one view) that holds the frames untouched, where the
    reference returns a list with one finished fp32 view."""

    def __init__(
        self,
        training=True,
        random_horizontal_flip=True,
        random_resize_aspect_ratio=(3/4, 4/3),
        random_resize_scale=(0.3, 1.0),
        reprob=0.0,
        auto_augment=False,
        motion_shift=False,
        crop_size=224,
        normalize=((0.485, 0.456, 0.406),
                   (0.229, 0.224, 0.225))
    ):
        if auto_augment:
            raise NotImplementedError("auto_augment=True: RandAugment runs through PIL on the CPU and is not the crop / flip / "
                                      "normalise / erase arithmetic the device kernels implement")
        self.training = training
        self.short_side_size = int(crop_size * 256 / 224)
        self.random_horizontal_flip = random_horizontal_flip
        self.random_resize_aspect_ratio = random_resize_aspect_ratio
        self.random_resize_scale = random_resize_scale
        self.auto_augment = auto_augment
        self.motion_shift = motion_shift
        self.crop_size = crop_size
        self.reprob = reprob
        # None, or a randaugment.RandAugmentDraw: training calls then draw a RandAugment plan first and attach it to the RawClip
        # (the reference's auto_augment=True is RandAugmentDraw('rand-m7-n4-mstd0.5-inc1'), utils.py:233-237); set after
        # construction, the constructor keeps the reference's signature
        self.rand_augment = None
        # False: validation frames must come with the short side the reference's Resize leaves.  True (set after construction, as
        # rand_augment is): frames of any size are resized to it on the device, as PIL's bilinear Image.resize does it
        self.device_resize = False
        self.mean, self.std = _normalize_constants(normalize)
        # box(es) and flip are drawn exactly as in pretraining (the same functions of src/datasets/utils/video/transforms.py)
        self._spatial = _PretrainVideoTransform(
            random_horizontal_flip=random_horizontal_flip, random_resize_aspect_ratio=random_resize_aspect_ratio,
            random_resize_scale=random_resize_scale, motion_shift=motion_shift, crop_size=crop_size, normalize=normalize)

    def __call__(self, buffer):
        frames = _uint8_frames(buffer, "VideoTransform")
        T, H, W, _ = frames.shape
        S = self.crop_size
        if not self.training:
            resize = _resize_sizes(H, W, self.short_side_size) if self.device_resize else None
            if resize is None:
                _require_short_side(H, W, self.short_side_size, "VideoTransform(training=False)")
            else:
                H, W = resize           # the centre crop is taken from the resized frames
            x1 = int(round((W - S) / 2.))
            y1 = int(round((H - S) / 2.))
            boxes = torch.tensor([y1, x1, S, S], dtype=torch.int32).repeat(1, T, 1)
            return RawClip(frames, boxes, False, S, self.mean, self.std, pre=True, resize=resize)
        aug_ops = aug_args = None
        if self.rand_augment is not None:
            # the reference augments first (utils.py:258-259), so these draws come before the crop, flip and erase draws
            aug_ops, aug_args = self.rand_augment.draw(H, W)
        boxes, flip = self._spatial.draw(T, H, W)
        ebox, noise = ((0, 0, 0, 0), None)
        if self.reprob > 0:
            ebox, noise = draw_erase(self.reprob, T, S, S)
        return RawClip(frames, boxes, flip, S, self.mean, self.std, pre=True, ebox=ebox, noise=noise, aug_ops=aug_ops,
                       aug_args=aug_args)


class EvalVideoTransform(object):
    """The reference's multi-view validation transform (utils.py:286-323) as boxes: `num_views_per_clip` crops of side
    `short_side_size` along the long side of frames whose short side already is `short_side_size`, starting at multiples of
    spatial_step = (max(H, W) - side) // (views - 1).  Returns ONE `RawClip` whose box table is [V,T,4], where the reference returns
    a list of V finished views: the views share the frames, which cross to the device once."""

    def __init__(
        self,
        num_views_per_clip=1,
        short_side_size=224,
        normalize=((0.485, 0.456, 0.406),
                   (0.229, 0.224, 0.225))
    ):
        if num_views_per_clip < 2:
            raise ValueError("EvalVideoTransform: the reference divides by num_views_per_clip - 1; one view is VideoTransform(training=False)")
        self.views_per_clip = num_views_per_clip
        self.short_side_size = short_side_size
        self.device_resize = False      # as VideoTransform.device_resize
        self.mean, self.std = _normalize_constants(normalize)

    def view_starts(self, H, W):
        spatial_step = (max(H, W) - self.short_side_size) // (self.views_per_clip - 1)
        return [i * spatial_step for i in range(self.views_per_clip)]

    def __call__(self, buffer):
        frames = _uint8_frames(buffer, "EvalVideoTransform")
        T, H, W, _ = frames.shape
        S = self.short_side_size
        resize = _resize_sizes(H, W, S) if self.device_resize else None
        if resize is None:
            _require_short_side(H, W, S, "EvalVideoTransform")
        else:
            H, W = resize               # the views are cut from the resized frames, which they share
        rows = [[start, 0, S, S] if H > W else [0, start, S, S] for start in self.view_starts(H, W)]
        boxes = torch.tensor(rows, dtype=torch.int32)[:, None, :].repeat(1, T, 1)
        return RawClip(frames, boxes, False, S, self.mean, self.std, pre=True, resize=resize)
