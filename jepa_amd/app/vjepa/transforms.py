"""Host half of the clip augmentation, with the reference's names (app/vjepa/transforms.py:15-115).

The reference's `VideoTransform` draws a random-resized-crop box (or two, with motion shift) and a flip on the CPU and then
does the pixel work there too: fp32 conversion, bilinear resize, mirror, normalisation.  Here `VideoTransform.__call__` keeps
the DRAWS -- the same calls, in the same order, on the same global generators (Python `random`, `np.random`), so the
augmentation stream of a seeded run is the reference's bit for bit -- and does no pixel work: it returns a `RawClip` (the uint8
frames as they came, an int32 [T,4] box table, the flip flag).  `default_collate` packs a list of them into a `RawClipBatch`
(one flat uint8 buffer + descriptor and box tables, validated), the mask collators pass it through untouched, and
`engine.input.DevicePrefetcher` ships the uint8 bytes and runs `vj_clip_transform` on its copy stream.

Supported: the transform of the three pretrain configs -- auto_augment false, reprob 0, random horizontal flip, random resize
scale / aspect ratio, crop size, motion_shift false and true.  `auto_augment=True` (PIL RandAugment) and `reprob > 0`
(RandomErasing) raise NotImplementedError.
"""
import math
import random

import numpy as np
import torch
from torch.utils.data._utils.collate import default_collate_fn_map

ALIGN = 16   # every clip of a RawClipBatch starts on a 16-byte boundary of the flat buffer


def make_transforms(
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
    return VideoTransform(
        random_horizontal_flip=random_horizontal_flip, random_resize_aspect_ratio=random_resize_aspect_ratio,
        random_resize_scale=random_resize_scale, reprob=reprob, auto_augment=auto_augment, motion_shift=motion_shift,
        crop_size=crop_size, normalize=normalize)


def _draw_box(scale, ratio, height, width, num_repeat=10):
    """One crop box (i, j, h, w) drawn as the reference draws it (src/datasets/utils/video/transforms.py:503-542 with its
    defaults log_scale=True, switch_hw=False): per try two `random.uniform`, one `np.random.uniform` (consumed although the
    swap it guards is off) and, on success, two `random.randint`; after ten failures the central crop at the nearest ratio."""
    area = height * width
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    for _ in range(num_repeat):
        target_area = random.uniform(*scale) * area
        aspect_ratio = math.exp(random.uniform(*log_ratio))
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        np.random.uniform()
        if 0 < w <= width and 0 < h <= height:
            i = random.randint(0, height - h)
            j = random.randint(0, width - w)
            return i, j, h, w
    in_ratio = float(width) / float(height)
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


class RawClip:
    """One undecorated clip on its way to the device: uint8 frames [T,H,W,3], int32 boxes [T,4] = (i, j, h, w), the flip flag,
    and the constants of the transform that drew them (output side, mean and std in 0..255 units)."""
    __slots__ = ("frames", "boxes", "flip", "crop_size", "mean", "std")

    def __init__(self, frames, boxes, flip, crop_size, mean, std):
        self.frames, self.boxes, self.flip = frames, boxes, bool(flip)
        self.crop_size, self.mean, self.std = int(crop_size), tuple(mean), tuple(std)


class RawClipBatch:
    """A collated list of RawClips, all CPU tensors:
        frames  uint8 [nbytes]   clip after clip, each [T,Hs,Ws,3], each starting on a 16-byte boundary
        desc    int64 [B,4]      (byte offset, Hs, Ws, flip)
        boxes   int32 [B,T,4]    (i, j, h, w) per frame
    """

    def __init__(self, frames, desc, boxes, crop_size, mean, std):
        self.frames, self.desc, self.boxes = frames, desc, boxes
        self.crop_size, self.mean, self.std = int(crop_size), tuple(mean), tuple(std)

    def __len__(self):
        return self.desc.shape[0]

    @property
    def num_frames(self):
        return self.boxes.shape[1]

    def validate(self):
        """Refuse, on the host, anything that would send the kernel outside a frame or the buffer."""
        f, d, bx = self.frames, self.desc, self.boxes
        if f.dtype != torch.uint8 or f.dim() != 1 or d.dtype != torch.int64 or d.dim() != 2 or d.shape[1] != 4 \
                or bx.dtype != torch.int32 or bx.dim() != 3 or bx.shape[2] != 4 or bx.shape[0] != d.shape[0]:
            raise ValueError(f"RawClipBatch: malformed tables frames {tuple(f.shape)} {f.dtype}, desc {tuple(d.shape)} "
                             f"{d.dtype}, boxes {tuple(bx.shape)} {bx.dtype}")
        if self.crop_size <= 0 or self.crop_size % 4 != 0:
            raise ValueError(f"RawClipBatch: crop_size={self.crop_size} must be a positive multiple of 4")
        if len(self.mean) != 3 or len(self.std) != 3 or any(s == 0 for s in self.std):
            raise ValueError("RawClipBatch: mean / std need three values each and a non-zero std")
        if d.shape[0] == 0:
            return self
        T = bx.shape[1]
        off, Hs, Ws = d[:, 0], d[:, 1], d[:, 2]
        if T <= 0 or bool((Hs <= 0).any()) or bool((Ws <= 0).any()):
            raise ValueError("RawClipBatch: empty clip")
        if bool((off < 0).any()) or bool((off % ALIGN != 0).any()) or bool((off + T * Hs * Ws * 3 > f.numel()).any()):
            raise ValueError("RawClipBatch: a clip does not lie inside the frame buffer on a 16-byte boundary")
        b64 = bx.to(torch.int64)
        i, j, h, w = b64[..., 0], b64[..., 1], b64[..., 2], b64[..., 3]
        bad = (i < 0) | (h <= 0) | (i + h > Hs[:, None]) | (j < 0) | (w <= 0) | (j + w > Ws[:, None])
        if bool(bad.any()):
            b, t = (int(v) for v in bad.nonzero()[0])
            raise ValueError(f"RawClipBatch: box {bx[b, t].tolist()} of clip {b} frame {t} leaves its {int(Hs[b])}x{int(Ws[b])} frame")
        return self

    def clip_frames(self, b):
        """The uint8 [T,Hs,Ws,3] frames of clip b (a view of the flat buffer)."""
        off, Hs, Ws = (int(v) for v in self.desc[b, :3])
        T = self.num_frames
        return self.frames[off:off + T * Hs * Ws * 3].view(T, Hs, Ws, 3)

    def pin_memory(self):
        self.frames, self.desc, self.boxes = self.frames.pin_memory(), self.desc.pin_memory(), self.boxes.pin_memory()
        return self

    def to(self, device):
        """(frames, desc, boxes) on `device` -- the arguments of jepa_amd.hip.ops.clip_transform."""
        return self.frames.to(device), self.desc.to(device), self.boxes.to(device)


def collate_raw_clips(batch, *, collate_fn_map=None):
    """default_collate of a list of RawClip -> one validated RawClipBatch."""
    first = batch[0]
    T = first.boxes.shape[0]
    offs, total = [], 0
    for c in batch:
        if c.frames.shape[0] != T or c.boxes.shape != (T, 4):
            raise ValueError("collate: clips of one batch must have the same number of frames")
        if (c.crop_size, c.mean, c.std) != (first.crop_size, first.mean, first.std):
            raise ValueError("collate: clips of one batch must come from one transform")
        offs.append(total)
        total += -(-c.frames.numel() // ALIGN) * ALIGN
    flat = torch.zeros(total, dtype=torch.uint8)
    for c, off in zip(batch, offs):
        n = c.frames.numel()
        flat[off:off + n] = c.frames.reshape(-1)
    desc = torch.tensor([[off, c.frames.shape[1], c.frames.shape[2], int(c.flip)] for c, off in zip(batch, offs)],
                        dtype=torch.int64).reshape(len(batch), 4)
    boxes = torch.stack([c.boxes for c in batch])
    return RawClipBatch(flat, desc, boxes, first.crop_size, first.mean, first.std).validate()


default_collate_fn_map[RawClip] = collate_raw_clips


class VideoTransform(object):

    def __init__(
        self,
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
                                      "normalise arithmetic the device kernel implements (no shipped pretrain config uses it)")
        if reprob > 0:
            raise NotImplementedError("reprob > 0: RandomErasing is not implemented on the device (every shipped pretrain "
                                      "config sets reprob: 0.0)")
        if crop_size <= 0 or crop_size % 4 != 0:
            raise ValueError(f"crop_size={crop_size} must be a positive multiple of 4 (16-byte output stores)")
        self.random_horizontal_flip = random_horizontal_flip
        self.random_resize_aspect_ratio = random_resize_aspect_ratio
        self.random_resize_scale = random_resize_scale
        self.auto_augment = auto_augment
        self.motion_shift = motion_shift
        self.crop_size = crop_size
        self.reprob = reprob
        # the reference keeps fp32 tensors scaled into uint8 space (transforms.py:61-66): the same fp32 values, as floats
        self.mean = tuple((torch.tensor(normalize[0], dtype=torch.float32) * 255.).tolist())
        self.std = tuple((torch.tensor(normalize[1], dtype=torch.float32) * 255.).tolist())

    def draw(self, num_frames, height, width):
        """(int32 boxes [T,4], flip) for one clip of `num_frames` height x width frames; consumes the global generators exactly
        as the reference's __call__ does (transforms.py:99-107)."""
        scale, ratio = self.random_resize_scale, self.random_resize_aspect_ratio
        first = _draw_box(scale, ratio, height, width)
        if self.motion_shift:
            # one box for the first frame, one for the last, fp32 linspace in between, truncated (transforms.py:603-608)
            last = _draw_box(scale, ratio, height, width)
            cols = [[int(v) for v in torch.linspace(a, b, steps=num_frames).tolist()] for a, b in zip(first, last)]
            boxes = torch.tensor(cols, dtype=torch.int32).t().contiguous()
        else:
            boxes = torch.tensor(first, dtype=torch.int32).repeat(num_frames, 1)
        flip = False
        if self.random_horizontal_flip:
            flip = bool(np.random.uniform() < 0.5)
        return boxes, flip

    def __call__(self, buffer):
        frames = torch.as_tensor(buffer)
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError(f"VideoTransform: expected a uint8 [T,H,W,3] buffer, got {frames.dtype} {tuple(frames.shape)}")
        T, H, W, _ = frames.shape
        boxes, flip = self.draw(T, H, W)
        return RawClip(frames.contiguous(), boxes, flip, self.crop_size, self.mean, self.std)
