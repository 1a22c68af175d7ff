"""Host half of the image evals' input edge: the reference's image transforms (evals/image_classification_frozen/eval.py:379-423) as
DRAWS.  The reference's pipeline is PIL arithmetic on uint8:

    training     timm create_transform: random-resized crop (scale (0.08, 1.0), ratio (3/4, 4/3), bicubic) to S x S, horizontal flip
                 (0.5), ToTensor, Normalize, RandomErasing (re_prob 0.25, pixel mode)
    validation   Resize(int(S * 256 / 224)) (bilinear, short side), CenterCrop(S), ToTensor, Normalize

`make_transforms(training, resolution, ...)` returns a transform that does no pixel work: it takes a decoded uint8 [H,W,3] image and
returns a `RawImage` -- the image as it came, its geometry row (i, j, h, w, OH, OW, wy, wx), the flip, the RandomErasing box and
noise.  `default_collate` packs a list of them into a `RawImageBatch` (one flat uint8 buffer + descriptor and geometry tables,
validated; the packing and the erase tables are those of app/vjepa/transforms.py's RawClipBatch), and engine.input.ImagePrefetcher
ships the bytes and runs vj_image_resample (PIL's antialiased two-pass resample, byte for byte), vj_clip_transform_pre (ToTensor +
Normalize + flip) and vj_clip_erase on its copy stream.

The crop box comes from app/vjepa/transforms.py's `_draw_box` and the erase box from its `draw_erase`, on the global generators
(Python `random`, `np.random`, torch).  The semantics are the reference's (timm / torchvision); the random STREAM is this package's
own: stream parity with timm / torchvision draws is not claimed.  The pixel arithmetic, given a box, is pinned byte for byte.

The reference's training pipeline also applies timm's `auto_augment='original'` policy between the flip and ToTensor.  It is an
extension key here, off by default (`data.auto_augment`: null, 'original' or a `rand-...` string; one parser,
app/vjepa/randaugment.auto_augment_draw).  With it, `ImageTransform.draw` draws box, flip, PLAN at (S, S), erase -- the reference
pipeline's order --, RawImage / RawImageBatch carry the plan tables (`aug_ops` int32 [B,8], `aug_args` float64 [B,8,6], None when no
image has a plan), and the prefetcher, after the resample, mirrors the flagged images on the uint8 side (vj_image_hflip: timm
augments the already flipped crop), runs the plan on the [B,S,S,3] buffer as one-frame clips with timm's fill colour
round(255 * mean) = (124, 116, 104) (vj_clip_randaug_fill), and hands vj_clip_transform_pre a zero flip column.  The policy table
was not checked against a timm install, and stream parity with timm's draws is not claimed, as for the box and erase draws; given a
plan, the pixels are PIL's byte for byte (tests/golden/image_autoaug_micro.npz, made with the reference's own operation functions).
Out of scope: timm's other policies ('originalr', 'v0', 'v0r', '3a', 'augmix-*', '-mstd' suffixes), JPEG decoding on the device,
non-RGB sources beyond `convert('RGB')`.
"""
import math

import numpy as np
import torch
from torch.utils.data._utils.collate import default_collate_fn_map

from ...app.vjepa.randaugment import MIN_SIDE, NUM_ARGS, auto_augment_draw
from ...app.vjepa.transforms import (_draw_box, buffer_offsets, check_aug_tables, check_constants, check_erase, check_erase_tables,
                                     check_extents, collate_aug, collate_erase, draw_erase, pack_buffers)

BILINEAR, BICUBIC = 0, 1          # the filter codes of vj_image_resample
MAX_SIDE = 1 << 15                # sides the kernel takes (exclusive)


def make_transforms(training=True, resolution=224, random_resize_scale=(0.08, 1.0), random_resize_aspect_ratio=(3 / 4, 4 / 3),
                    random_horizontal_flip=0.5, reprob=0.25,
                    normalize=((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)), auto_augment=None):
    return ImageTransform(training=training, resolution=resolution, random_resize_scale=random_resize_scale,
                          random_resize_aspect_ratio=random_resize_aspect_ratio, random_horizontal_flip=random_horizontal_flip,
                          reprob=reprob, normalize=normalize, auto_augment=auto_augment)


def fill_colour(mean):
    """timm's fill colour of the affine operations: tuple(min(255, round(255 * m)) for m in mean) -- (124, 116, 104) for ImageNet."""
    return tuple(min(255, round(255 * m)) for m in mean)


def short_side_size(H, W, R):
    """(OH, OW) of torchvision's Resize(R) on an H x W image: the short side becomes R, the long side int(R * long / short)."""
    if H <= W:
        return R, int(R * W / H)
    return int(R * H / W), R


def center_window(OH, OW, S):
    """(wy, wx) of CenterCrop(S) on an OH x OW image, with Python's round (round(58.5) == 58)."""
    return int(round((OH - S) / 2.0)), int(round((OW - S) / 2.0))


def _filter_support(filt):
    return 2.0 if filt == BICUBIC else 1.0


def axis_taps(n, m, filt):
    """Taps one output index can have when n pixels are resampled to m: int(ceil(support * max(n / m, 1))) * 2 + 1."""
    return int(math.ceil(_filter_support(filt) * max(n / m, 1.0))) * 2 + 1


def axis_span(n, m, filt, first, count):
    """(first source index, number of source indices) that outputs first .. first + count - 1 of the axis read."""
    scale = n / m
    support = _filter_support(filt) * max(scale, 1.0)
    lo = max(int((first + 0.5) * scale - support + 0.5), 0)
    hi = min(int((first + count - 0.5) * scale + support + 0.5), n)
    return lo, hi - lo


class RawImage:
    """One undecorated image on its way to the device: uint8 [H,W,3], its geometry (i, j, h, w, OH, OW, wy, wx), the flip flag, the
    output side, the filter code, mean / std (0..1 units) and the RandomErasing draw (`ebox` = (top, left, h, w), `noise` fp32
    [1,3,h,w]; h == 0 / None: not erased).  `aug_ops` int32 [8] / `aug_args` float64 [8,6]: the AutoAugment / RandAugment plan of
    the flipped S x S crop (randaugment.AutoAugmentDraw.draw; None: none)."""
    __slots__ = ("image", "geom", "flip", "crop_size", "filter", "mean", "std", "ebox", "noise", "aug_ops", "aug_args")

    def __init__(self, image, geom, flip, crop_size, filter, mean, std, ebox=(0, 0, 0, 0), noise=None, aug_ops=None, aug_args=None):
        self.image, self.geom, self.flip = image, tuple(int(v) for v in geom), bool(flip)
        self.crop_size, self.filter, self.mean, self.std = int(crop_size), int(filter), tuple(mean), tuple(std)
        self.ebox, self.noise = tuple(int(v) for v in ebox), noise
        if (aug_ops is None) != (aug_args is None):
            raise ValueError("RawImage: aug_ops and aug_args come together")
        self.aug_ops = None if aug_ops is None else torch.as_tensor(aug_ops, dtype=torch.int32).reshape(-1)
        self.aug_args = None if aug_args is None else torch.as_tensor(aug_args, dtype=torch.float64).reshape(-1, NUM_ARGS)


class RawImageBatch:
    """A collated list of RawImages, all CPU tensors:
        frames     uint8 [nbytes]   image after image, each [Hs,Ws,3], each starting on a 16-byte boundary
        desc       int64 [B,4]      (byte offset, Hs, Ws, flip)
        geom       int32 [B,8]      (i, j, h, w, OH, OW, wy, wx)
        ebox / noise / noise_off    the erase tables of RawClipBatch, one frame per image
        aug_ops    int32 [B,8]      plan of the flipped S x S crop, operation codes layer by layer (None: no image has a plan)
        aug_args   float64 [B,8,6]  their arguments (app/vjepa/randaugment.py)
    with the output side, the filter code and mean / std (0..1 units: the normalise-first form of vj_clip_transform_pre)."""

    def __init__(self, frames, desc, geom, crop_size, filter, mean, std, ebox=None, noise=None, noise_off=None, aug_ops=None,
                 aug_args=None):
        self.frames, self.desc, self.geom = frames, desc, geom
        self.aug_ops, self.aug_args = aug_ops, aug_args
        self.crop_size, self.filter, self.mean, self.std = int(crop_size), int(filter), tuple(mean), tuple(std)
        B = desc.shape[0]
        self.ebox = torch.zeros((B, 4), dtype=torch.int32) if ebox is None else ebox
        self.noise = torch.zeros(0, dtype=torch.float32) if noise is None else noise
        self.noise_off = torch.zeros(B, dtype=torch.int64) if noise_off is None else noise_off

    def __len__(self):
        return self.desc.shape[0]

    @property
    def erased(self):
        return self.noise.numel() > 0 and bool((self.ebox[:, 2] > 0).any())

    @property
    def augmented(self):
        """Whether any image carries an operation (decided on the host: otherwise no upload, no launch, and the late flip)."""
        return self.aug_ops is not None and bool((self.aug_ops != 0).any())

    def validate(self):
        """Refuse, on the host, anything that would send the kernels outside an image, its resize or a buffer."""
        who = "RawImageBatch"
        f, d, g = self.frames, self.desc, self.geom
        if f.dtype != torch.uint8 or f.dim() != 1 or d.dtype != torch.int64 or d.dim() != 2 or d.shape[1] != 4 \
                or g.dtype != torch.int32 or tuple(g.shape) != (d.shape[0], 8):
            raise ValueError(f"{who}: malformed tables frames {tuple(f.shape)} {f.dtype}, desc {tuple(d.shape)} {d.dtype}, geom "
                             f"{tuple(g.shape)} {g.dtype}")
        check_erase_tables(who, self.ebox, self.noise, self.noise_off, d.shape[0])
        check_constants(who, self.crop_size, self.mean, self.std)
        if self.filter not in (BILINEAR, BICUBIC):
            raise ValueError(f"{who}: filter={self.filter} (0 bilinear, 1 bicubic)")
        if check_aug_tables(who, self.aug_ops, self.aug_args, d.shape[0]) and self.augmented:
            S = self.crop_size
            if S < MIN_SIDE:
                raise ValueError(f"{who}: augmented images of side {S}, below {MIN_SIDE}")
            if d.shape[0] * S * S * 3 >= 1 << 31:
                raise ValueError(f"{who}: {d.shape[0]} augmented images of {S}x{S} are {d.shape[0] * S * S * 3} bytes, below 2^31 "
                                 "are taken")
        if d.shape[0] == 0:
            return self
        check_extents(who, f, d, 1, what="image")
        Hs, Ws, S = d[:, 1], d[:, 2], self.crop_size
        if bool((Hs >= MAX_SIDE).any()) or bool((Ws >= MAX_SIDE).any()):
            raise ValueError(f"{who}: an image side of {int(torch.maximum(Hs, Ws).max())} pixels, below {MAX_SIDE} are taken")
        g64 = g.to(torch.int64)
        i, j, h, w, OH, OW, wy, wx = (g64[:, k] for k in range(8))
        bad = (i < 0) | (h <= 0) | (i + h > Hs) | (j < 0) | (w <= 0) | (j + w > Ws)
        if bool(bad.any()):
            b = int(bad.nonzero()[0])
            raise ValueError(f"{who}: box {g[b, :4].tolist()} of image {b} leaves its {int(Hs[b])}x{int(Ws[b])} image")
        bad = (OH <= 0) | (OW <= 0) | (OH >= MAX_SIDE) | (OW >= MAX_SIDE) | (wy < 0) | (wx < 0) | (wy + S > OH) | (wx + S > OW)
        if bool(bad.any()):
            b = int(bad.nonzero()[0])
            raise ValueError(f"{who}: the {S}x{S} window at {g[b, 6:].tolist()} of image {b} leaves its resize to "
                             f"{int(OH[b])}x{int(OW[b])}")
        check_erase(who, self.ebox, self.noise, self.noise_off, 1, S, what="image")
        return self

    def capacities(self):
        """(taps_x, taps_y, rows) of vj_image_resample for this batch: per axis the most taps an output index has, and the most
        source rows the window's vertical taps span.  (1, 1, 1) for an empty batch."""
        tx = ty = rows = 1
        for i, j, h, w, OH, OW, wy, wx in self.geom.tolist():
            tx, ty = max(tx, axis_taps(w, OW, self.filter)), max(ty, axis_taps(h, OH, self.filter))
            rows = max(rows, axis_span(h, OH, self.filter, wy, self.crop_size)[1])
        return tx, ty, rows

    def resampled_tables(self):
        """(desc int64 [B,4], boxes int32 [B,1,4]) that read the resampled uint8 [B,S,S,3] buffer as one-frame clips: offsets
        b*S*S*3 (multiples of 16), Hs = Ws = S, this batch's flip flags, identity boxes (0, 0, S, S)."""
        B, S = len(self), self.crop_size
        desc = torch.stack([torch.arange(B, dtype=torch.int64) * (S * S * 3), torch.full((B,), S, dtype=torch.int64),
                            torch.full((B,), S, dtype=torch.int64), self.desc[:, 3]], dim=1).contiguous()
        boxes = torch.tensor([0, 0, S, S], dtype=torch.int32).repeat(B, 1, 1)
        return desc, boxes

    def image(self, b):
        """The uint8 [Hs,Ws,3] image of row b (a view of the flat buffer)."""
        off, Hs, Ws = (int(v) for v in self.desc[b, :3])
        return self.frames[off:off + Hs * Ws * 3].view(Hs, Ws, 3)

    def pin_memory(self):
        self.frames, self.desc, self.geom = self.frames.pin_memory(), self.desc.pin_memory(), self.geom.pin_memory()
        self.ebox, self.noise_off = self.ebox.pin_memory(), self.noise_off.pin_memory()
        self.noise = self.noise.pin_memory() if self.noise.numel() else self.noise
        if self.aug_ops is not None:
            self.aug_ops, self.aug_args = self.aug_ops.pin_memory(), self.aug_args.pin_memory()
        return self


def collate_raw_images(batch, *, collate_fn_map=None):
    """default_collate of a list of RawImage -> one validated RawImageBatch (nothing is copied when the tables are refused)."""
    first = batch[0]
    for c in batch:
        if (c.crop_size, c.filter, c.mean, c.std) != (first.crop_size, first.filter, first.mean, first.std):
            raise ValueError("collate: images of one batch must come from one transform (crop size, filter, mean / std)")
        if c.image.dtype != torch.uint8 or c.image.dim() != 3 or c.image.shape[-1] != 3:
            raise ValueError(f"collate: expected uint8 [H,W,3] images, got {c.image.dtype} {tuple(c.image.shape)}")
    # the tables first, over a buffer that has the extent and no bytes yet: a refused batch copies nothing
    offs, total = buffer_offsets([c.image.numel() for c in batch])
    desc =torch.tensor([[off, c.image.shape[0], c.image.shape[1], int(c.flip)] for c, off in zip(batch, offs)],
                        dtype=torch.int64).reshape(len(batch), 4)
    geom = torch.tensor([c.geom for c in batch], dtype=torch.int32).reshape(len(batch), 8)
    ebox, noise, noise_off = collate_erase(batch)
    aug_ops, aug_args = collate_aug(batch)
    out = RawImageBatch(_extent_only(total), desc, geom, first.crop_size, first.filter, first.mean, first.std, ebox=ebox,
                        noise=noise, noise_off=noise_off, aug_ops=aug_ops, aug_args=aug_args).validate()
    out.frames, _ = pack_buffers([c.image for c in batch])
    return out


def _extent_only(nbytes):
    """A uint8 [nbytes] tensor that takes no memory (one zero byte, stride 0): what validate needs of the buffer is its length."""
    return torch.zeros(1, dtype=torch.uint8).expand(nbytes) if nbytes else torch.zeros(0, dtype=torch.uint8)


default_collate_fn_map[RawImage] = collate_raw_images


class ImageTransform(object):
    """The reference's two image transforms as draws (module docstring).  training=True: the random-resized-crop box, the flip and
    the RandomErasing box and noise, in that order; the device resamples the box to S x S with the bicubic filter.  training=False:
    no draw; the whole image is resampled to the short-side size with the bilinear filter and the centre window is taken.
    auto_augment (None, 'original' or a `rand-...` string: randaugment.auto_augment_draw): training also draws the policy's plan for
    the flipped S x S crop, between the flip and the erase box; validation never draws."""

    def __init__(self, training=True, resolution=224, random_resize_scale=(0.08, 1.0), random_resize_aspect_ratio=(3 / 4, 4 / 3),
                 random_horizontal_flip=0.5, reprob=0.25, normalize=((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
                 auto_augment=None):
        if resolution <= 0 or resolution % 4 != 0:
            raise ValueError(f"resolution={resolution} must be a positive multiple of 4 (16-byte output stores)")
        self.training, self.crop_size = training, int(resolution)
        self.random_resize_scale, self.random_resize_aspect_ratio = random_resize_scale, random_resize_aspect_ratio
        self.random_horizontal_flip, self.reprob = float(random_horizontal_flip), float(reprob)
        self.resize_size = int(resolution * 256 / 224)
        self.filter = BICUBIC if training else BILINEAR
        t = torch.tensor(normalize, dtype=torch.float32)          # the fp32 values the reference's Normalize holds
        self.mean, self.std = tuple(t[0].tolist()), tuple(t[1].tolist())
        plan_draw = auto_augment_draw(auto_augment)               # parsed either way: a bad value raises for validation too
        self.auto_augment = plan_draw if training else None       # validation never draws

    def draw(self, H, W):
        """(geometry row, flip, erase box, noise, plan) for one H x W image; plan: (ops, args) or None."""
        S = self.crop_size
        if not self.training:
            OH, OW = short_side_size(H, W, self.resize_size)
            wy, wx = center_window(OH, OW, S)
            return (0, 0, H, W, OH, OW, wy, wx), False, (0, 0, 0, 0), None, None
        i, j, h, w = _draw_box(self.random_resize_scale, self.random_resize_aspect_ratio, H, W)
        flip = bool(np.random.uniform() < self.random_horizontal_flip) if self.random_horizontal_flip > 0 else False
        plan = None if self.auto_augment is None else self.auto_augment.draw(S, S)
        ebox, noise = (0, 0, 0, 0), None
        if self.reprob > 0:
            ebox, noise = draw_erase(self.reprob, num_frames=1, img_h=S, img_w=S)
        return (i, j, h, w, S, S, 0, 0), flip, ebox, noise, plan

    def __call__(self, image):
        img = torch.as_tensor(np.asarray(image))
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[-1] != 3:
            raise ValueError(f"ImageTransform: expected a uint8 [H,W,3] image, got {img.dtype} {tuple(img.shape)}")
        geom, flip, ebox, noise, plan = self.draw(img.shape[0], img.shape[1])
        aug_ops, aug_args = (None, None) if plan is None else plan
        return RawImage(img.contiguous(), geom, flip, self.crop_size, self.filter, self.mean, self.std, ebox=ebox, noise=noise,
                        aug_ops=aug_ops, aug_args=aug_args)
