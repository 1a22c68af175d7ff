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
(RandomErasing) raise NotImplementedError here.  The RandomErasing draw itself (`draw_erase`) and the tables that carry it to
`vj_clip_erase` live in this module; the frozen eval's transforms (evals/video_classification_frozen/utils.py), which set
reprob 0.25, use them, together with the normalise-first flag and per-clip view boxes of `RawClip` / `RawClipBatch`.  Those two
also carry the optional RandAugment plan of a clip (drawn by randaugment.RandAugmentDraw, carried out by `vj_clip_randaug`), which
the eval's training transform attaches behind its `rand_augment` attribute.
"""
import math
import random

import numpy as np
import torch
from torch.utils.data._utils.collate import default_collate_fn_map

from .randaugment import MAX_LAYERS, MIN_SIDE, NUM_ARGS, NUM_OPS

ALIGN = 16   # every clip of a RawClipBatch starts on a 16-byte boundary of the flat buffer
MAX_SIDE = 1 << 15   # sides of a resize stay below it (csrc/image_resample.hip)


def resample_taps(n, m, filter_support=1.0):
    """Taps an output index of PIL's antialiased resample can have on an axis that takes n samples to m (the capacity
    vj_clip_resample's tables are sized by): int(ceil(support * max(n / m, 1))) * 2 + 1, bilinear support 1."""
    return int(math.ceil(filter_support * max(n / m, 1.0))) * 2 + 1


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


def draw_erase(probability, num_frames, img_h, img_w, min_area=0.02, max_area=1 / 3, min_aspect=0.3):
    """RandomErasing(probability, mode='pixel', max_count=1, num_splits=1, cube=True) as DRAWS only, with the reference's calls in
    the reference's order on the global generators (src/datasets/utils/video/randerase.py:116-156): `random.random()`; up to 100
    tries of two `random.uniform`; the strict `w < img_w and h < img_h` test; two `random.randint`; then one
    `torch.empty((3, h, w)).normal_()` per frame.  Returns ((top, left, h, w), noise fp32 [T,3,h,w]) or ((0, 0, 0, 0), None) when
    the clip is not erased (the first draw, or 100 boxes that do not fit)."""
    if random.random() > probability:
        return (0, 0, 0, 0), None
    area = img_h * img_w
    log_aspect = (math.log(min_aspect), math.log(1 / min_aspect))
    for _ in range(100):
        target_area = random.uniform(min_area, max_area) * area / 1
        aspect_ratio = math.exp(random.uniform(*log_aspect))
        h = int(round(math.sqrt(target_area * aspect_ratio)))
        w = int(round(math.sqrt(target_area / aspect_ratio)))
        if w < img_w and h < img_h:
            top = random.randint(0, img_h - h)
            left = random.randint(0, img_w - w)
            noise = torch.stack([torch.empty((3, h, w), dtype=torch.float32).normal_() for _ in range(num_frames)])
            return (top, left, h, w), noise
    return (0, 0, 0, 0), None


class RawClip:
    """One undecorated clip on its way to the device: uint8 frames [T,H,W,3], int32 boxes [T,4] = (i, j, h, w) -- or [V,T,4], one
    table per spatial view of the same frames --, the flip flag, and the constants of the transform that drew them (output side,
    mean and std).  `pre` selects the frozen eval's normalise-first arithmetic (mean / std in 0..1 units; otherwise 0..255).
    `ebox` = (top, left, h, w) and `noise` fp32 [T,3,h,w] are the RandomErasing draw of the clip (h == 0 / None: not erased).
    `aug_ops` int32 [8] and `aug_args` float64 [8,6] are its RandAugment plan (randaugment.RandAugmentDraw.draw; None: none), which
    the device carries out on the uint8 frames before anything else.  `resize` = (OH, OW) (None: none) has the device bring every
    frame to OH x OW first, as PIL's antialiased bilinear Image.resize does (vj_clip_resample); the boxes then refer to the resized
    frames."""
    __slots__ = ("frames", "boxes", "flip", "crop_size", "mean", "std", "pre", "ebox", "noise", "aug_ops", "aug_args", "resize")

    def __init__(self, frames, boxes, flip, crop_size, mean, std, pre=False, ebox=(0, 0, 0, 0), noise=None, aug_ops=None,
                 aug_args=None, resize=None):
        self.resize = None if resize is None else (int(resize[0]), int(resize[1]))
        self.frames, self.boxes, self.flip = frames, boxes, bool(flip)
        self.crop_size, self.mean, self.std = int(crop_size), tuple(mean), tuple(std)
        self.pre, self.ebox, self.noise = bool(pre), tuple(int(v) for v in ebox), noise
        if (aug_ops is None) != (aug_args is None):
            raise ValueError("RawClip: aug_ops and aug_args come together")
        self.aug_ops = None if aug_ops is None else torch.as_tensor(aug_ops, dtype=torch.int32).reshape(-1)
        self.aug_args = None if aug_args is None else torch.as_tensor(aug_args, dtype=torch.float64).reshape(-1, NUM_ARGS)

    @property
    def num_views(self):
        return self.boxes.shape[0] if self.boxes.dim() == 3 else 1


def buffer_offsets(sizes):
    """(byte offsets, total bytes) of buffers of `sizes` bytes laid out one after the other, each on a 16-byte boundary."""
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += -(-n // ALIGN) * ALIGN
    return offs, total


def pack_buffers(tensors):
    """uint8 tensors -> (one flat uint8 buffer that holds them one after the other, each on a 16-byte boundary, their byte offsets):
    the packing of RawClipBatch and of the image evals' RawImageBatch."""
    offs, total = buffer_offsets([t.numel() for t in tensors])
    flat = torch.zeros(total, dtype=torch.uint8)
    for t, off in zip(tensors, offs):
        n = t.numel()
        flat[off:off + n] = t.reshape(-1)
    return flat, offs


def collate_erase(rows):
    """(ebox int32 [R,4], noise fp32 [n], noise_off int64 [R]) of rows that carry `.ebox` and `.noise` (None: not erased)."""
    ebox = torch.tensor([c.ebox if c.noise is not None else (0, 0, 0, 0) for c in rows], dtype=torch.int32).reshape(len(rows), 4)
    noise_off, blocks, n = [], [], 0
    for c in rows:
        noise_off.append(n if c.noise is not None else 0)
        if c.noise is not None:
            blocks.append(c.noise.to(torch.float32).reshape(-1))
            n += blocks[-1].numel()
    noise = torch.cat(blocks) if blocks else torch.zeros(0, dtype=torch.float32)
    return ebox, noise, torch.tensor(noise_off, dtype=torch.int64)


def check_erase_tables(who, eb, nz, no, R):
    if eb.dtype != torch.int32 or tuple(eb.shape) != (R, 4) or nz.dtype != torch.float32 or nz.dim() != 1 \
            or no.dtype != torch.int64 or tuple(no.shape) != (R,):
        raise ValueError(f"{who}: malformed erase tables ebox {tuple(eb.shape)} {eb.dtype}, noise {tuple(nz.shape)} "
                         f"{nz.dtype}, noise_off {tuple(no.shape)} {no.dtype}")


def check_constants(who, crop_size, mean, std):
    if crop_size <= 0 or crop_size % 4 != 0:
        raise ValueError(f"{who}: crop_size={crop_size} must be a positive multiple of 4")
    if len(mean) != 3 or len(std) != 3 or any(s == 0 for s in std):
        raise ValueError(f"{who}: mean / std need three values each and a non-zero std")


def check_extents(who, f, d, T, what="clip"):
    """Every row of desc names T frames of Hs x Ws x 3 bytes that lie inside the flat buffer f on a 16-byte boundary."""
    off, Hs, Ws = d[:, 0], d[:, 1], d[:, 2]
    if T <= 0 or bool((Hs <= 0).any()) or bool((Ws <= 0).any()):
        raise ValueError(f"{who}: empty {what}")
    if bool((off < 0).any()) or bool((off % ALIGN != 0).any()) or bool((off + T * Hs * Ws * 3 > f.numel()).any()):
        raise ValueError(f"{who}: a {what} does not lie inside the frame buffer on a 16-byte boundary")


def check_erase(who, eb, nz, no, T, S, what="clip"):
    """Every erase box lies inside its S x S output and its [T,3,h,w] noise block inside the noise buffer."""
    e64 = eb.to(torch.int64)
    top, left, eh, ew = e64[:, 0], e64[:, 1], e64[:, 2], e64[:, 3]
    on = eh != 0
    bad = on & ((top < 0) | (left < 0) | (eh < 0) | (ew <= 0) | (top + eh > S) | (left + ew > S))
    if bool(bad.any()):
        b = int(bad.nonzero()[0])
        raise ValueError(f"{who}: erase box {eb[b].tolist()} of {what} {b} leaves its {S}x{S} {what}")
    bad = on & ((no < 0) | (no + T * 3 * eh * ew > nz.numel()))
    if bool(bad.any()):
        b = int(bad.nonzero()[0])
        raise ValueError(f"{who}: the noise block of {what} {b} ({T}x3x{int(eh[b])}x{int(ew[b])} values at {int(no[b])}) "
                         f"leaves the noise buffer of {nz.numel()} values")


def check_aug_tables(who, ao, aa, R):
    """The RandAugment / AutoAugment plan tables of R rows (None, None: no plan, returns False): int32 [R,8] codes in range and
    float64 [R,8,6] finite arguments."""
    if (ao is None) != (aa is None):
        raise ValueError(f"{who}: aug_ops and aug_args come together")
    if ao is None:
        return False
    if ao.dtype != torch.int32 or tuple(ao.shape) != (R, MAX_LAYERS) or aa.dtype != torch.float64 \
            or tuple(aa.shape) != (R, MAX_LAYERS, NUM_ARGS):
        raise ValueError(f"{who}: malformed RandAugment tables aug_ops {tuple(ao.shape)} {ao.dtype}, aug_args "
                         f"{tuple(aa.shape)} {aa.dtype}")
    if bool(((ao < 0) | (ao > NUM_OPS)).any()):
        raise ValueError(f"{who}: unknown RandAugment operation code in {ao[((ao < 0) | (ao > NUM_OPS)).any(1)][0].tolist()}")
    if not bool(torch.isfinite(aa).all()):
        raise ValueError(f"{who}: non-finite RandAugment argument")
    return True


def collate_aug(rows):
    """(aug_ops int32 [R,8], aug_args float64 [R,8,6]) of rows that carry `.aug_ops` / `.aug_args` (None: no plan, the row stays
    zero: no work), or (None, None) when no row has a plan."""
    if not any(c.aug_ops is not None for c in rows):
        return None, None
    aug_ops = torch.zeros((len(rows), MAX_LAYERS), dtype=torch.int32)
    aug_args = torch.zeros((len(rows), MAX_LAYERS, NUM_ARGS), dtype=torch.float64)
    for r, c in enumerate(rows):
        if c.aug_ops is not None:
            if tuple(c.aug_ops.shape) != (MAX_LAYERS,) or tuple(c.aug_args.shape) != (MAX_LAYERS, NUM_ARGS):
                raise ValueError(f"collate: a RandAugment plan is int32 [{MAX_LAYERS}] / float64 [{MAX_LAYERS},{NUM_ARGS}]")
            aug_ops[r], aug_args[r] = c.aug_ops, c.aug_args
    return aug_ops, aug_args


class RawClipBatch:
    """A collated list of RawClips, all CPU tensors:
        frames     uint8 [nbytes]   clip after clip, each [T,Hs,Ws,3], each starting on a 16-byte boundary, each ONCE
        desc       int64 [R,4]      (byte offset, Hs, Ws, flip)
        boxes      int32 [R,T,4]    (i, j, h, w) per frame
        ebox       int32 [R,4]      (top, left, h, w) of the erased box; h == 0: none
        noise      fp32 [n]         per erased row one [T,3,h,w] block
        noise_off  int64 [R]        where the row's block starts in `noise`
        aug_ops    int32 [R,8]      RandAugment operation codes, layer by layer; 0: nothing (None: no row has a plan)
        aug_args   float64 [R,8,6]  their arguments (randaugment.py)
        rgeom      int32 [R,2]      (OH, OW) the frames of the row are resized to before the boxes apply; a row that is not resized
                                    has its source size (None: no row is resized, nothing about the batch changes)
    R = num_views * B rows, view-major: rows [v*B, (v+1)*B) are view v of the B clips, and the rows of one clip share its byte
    offset.  `pre`: the normalise-first form (mean / std in 0..1 units)."""

    def __init__(self, frames, desc, boxes, crop_size, mean, std, pre=False, num_views=1, ebox=None, noise=None, noise_off=None,
                 aug_ops=None, aug_args=None, rgeom=None):
        self.frames, self.desc, self.boxes, self.rgeom = frames, desc, boxes, rgeom
        self.aug_ops, self.aug_args = aug_ops, aug_args
        self.crop_size, self.mean, self.std = int(crop_size), tuple(mean), tuple(std)
        self.pre, self.num_views = bool(pre), int(num_views)
        R = desc.shape[0]
        self.ebox = torch.zeros((R, 4), dtype=torch.int32) if ebox is None else ebox
        self.noise = torch.zeros(0, dtype=torch.float32) if noise is None else noise
        self.noise_off = torch.zeros(R, dtype=torch.int64) if noise_off is None else noise_off

    def __len__(self):
        return self.desc.shape[0]

    @property
    def num_frames(self):
        return self.boxes.shape[1]

    @property
    def erased(self):
        """Whether any row of the batch carries an erase box (decided on the host: no launch otherwise)."""
        return self.noise.numel() > 0 and bool((self.ebox[:, 2] > 0).any())

    @property
    def augmented(self):
        """Whether any row of the batch carries a RandAugment operation (decided on the host: no upload and no launch otherwise)."""
        return self.aug_ops is not None and bool((self.aug_ops != 0).any())

    @property
    def resized(self):
        """Whether any row of the batch is resized on the device (decided on the host: no buffer and no launch otherwise)."""
        return self.rgeom is not None and bool((self.rgeom.to(torch.int64) != self.desc[:, 1:3]).any())

    def _validate_rgeom(self):
        """The extents the boxes refer to, int64 [R] each: the resized ones where the batch carries a resize table."""
        d, rg = self.desc, self.rgeom
        if rg is None:
            return d[:, 1], d[:, 2]
        if rg.dtype != torch.int32 or tuple(rg.shape) != (d.shape[0], 2):
            raise ValueError(f"RawClipBatch: malformed resize table rgeom {tuple(rg.shape)} {rg.dtype}")
        bad = ((rg <= 0) | (rg >= MAX_SIDE)).any(1)
        if bool(bad.any()):
            b = int(bad.nonzero()[0])
            raise ValueError(f"RawClipBatch: resize {rg[b].tolist()} of clip {b} is not positive and below {MAX_SIDE}")
        if self.aug_ops is not None and self.resized:
            raise ValueError("RawClipBatch: a batch carries RandAugment plans or a resize, not both (no transform draws both)")
        B = d.shape[0] // self.num_views
        if bool((rg.reshape(self.num_views, B, 2) != rg[:B]).any()):
            raise ValueError("RawClipBatch: the views of a clip share its frames and therefore its resize")
        return rg[:, 0].to(torch.int64), rg[:, 1].to(torch.int64)

    def resample_plan(self, filter_support=1.0):
        """What vj_clip_resample needs for this (validated) batch: (rgeom int32 [B,2] of the B clips, desc_out int64 [R,4] that reads
        the resized buffer -- every clip dense at a 16-byte boundary, once, its views sharing it --, the buffer's size in bytes,
        caps = (oh, ow, taps_x, taps_y, rows))."""
        R, T = len(self), self.num_frames
        B = R // self.num_views
        rg = self.rgeom[:B]
        offs, total = buffer_offsets([T * OH * OW * 3 for OH, OW in rg.tolist()])
        desc_out = torch.stack([torch.tensor(offs, dtype=torch.int64).reshape(B), rg[:, 0].to(torch.int64), rg[:, 1].to(torch.int64),
                                self.desc[:B, 3]], dim=1).repeat(self.num_views, 1).contiguous()
        desc_out[:, 3] = self.desc[:, 3]
        oh = ow = tx = ty = rows = 1
        for (_, Hs, Ws, _), (OH, OW) in zip(self.desc[:B].tolist(), rg.tolist()):
            oh, ow, rows = max(oh, OH), max(ow, OW), max(rows, Hs)
            tx, ty = max(tx, resample_taps(Ws, OW, filter_support)), max(ty, resample_taps(Hs, OH, filter_support))
        return rg.contiguous(), desc_out, total, (oh, ow, tx, ty, rows)

    def _validate_aug(self):
        ao, aa, d = self.aug_ops, self.aug_args, self.desc
        if not check_aug_tables("RawClipBatch", ao, aa, d.shape[0]):
            return
        on = (ao != 0).any(1)
        small = on & ((d[:, 1] < MIN_SIDE) | (d[:, 2] < MIN_SIDE))
        if bool(small.any()):
            b = int(small.nonzero()[0])
            raise ValueError(f"RawClipBatch: augmented clip {b} of {int(d[b, 1])}x{int(d[b, 2])} has a side below {MIN_SIDE}")
        offs = d[:, 0].tolist()
        for b in on.nonzero().reshape(-1).tolist():
            if offs.count(offs[b]) > 1:
                raise ValueError(f"RawClipBatch: augmented clip {b} shares its byte offset {offs[b]} with another row (the pass is "
                                 "in place)")

    def validate(self):
        """Refuse, on the host, anything that would send the kernels outside a frame, a clip or a buffer."""
        f, d, bx = self.frames, self.desc, self.boxes
        if f.dtype != torch.uint8 or f.dim() != 1 or d.dtype != torch.int64 or d.dim() != 2 or d.shape[1] != 4 \
                or bx.dtype != torch.int32 or bx.dim() != 3 or bx.shape[2] != 4 or bx.shape[0] != d.shape[0]:
            raise ValueError(f"RawClipBatch: malformed tables frames {tuple(f.shape)} {f.dtype}, desc {tuple(d.shape)} "
                             f"{d.dtype}, boxes {tuple(bx.shape)} {bx.dtype}")
        eb, nz, no = self.ebox, self.noise, self.noise_off
        check_erase_tables("RawClipBatch", eb, nz, no, d.shape[0])
        check_constants("RawClipBatch", self.crop_size, self.mean, self.std)
        if self.num_views <= 0 or d.shape[0] % self.num_views != 0:
            raise ValueError(f"RawClipBatch: {d.shape[0]} rows are not {self.num_views} views of a whole number of clips")
        if d.shape[0] == 0:
            return self
        T = bx.shape[1]
        check_extents("RawClipBatch", f, d, T)
        Hs, Ws = self._validate_rgeom()             # what the boxes must stay inside
        b64 = bx.to(torch.int64)
        i, j, h, w = b64[..., 0], b64[..., 1], b64[..., 2], b64[..., 3]
        bad = (i < 0) | (h <= 0) | (i + h > Hs[:, None]) | (j < 0) | (w <= 0) | (j + w > Ws[:, None])
        if bool(bad.any()):
            b, t = (int(v) for v in bad.nonzero()[0])
            raise ValueError(f"RawClipBatch: box {bx[b, t].tolist()} of clip {b} frame {t} leaves its {int(Hs[b])}x{int(Ws[b])} frame")
        check_erase("RawClipBatch", eb, nz, no, T, self.crop_size)
        self._validate_aug()
        return self

    def clip_frames(self, b):
        """The uint8 [T,Hs,Ws,3] frames of row b (a view of the flat buffer)."""
        off, Hs, Ws = (int(v) for v in self.desc[b, :3])
        T = self.num_frames
        return self.frames[off:off + T * Hs * Ws * 3].view(T, Hs, Ws, 3)

    def pin_memory(self):
        self.frames, self.desc, self.boxes = self.frames.pin_memory(), self.desc.pin_memory(), self.boxes.pin_memory()
        self.ebox, self.noise_off = self.ebox.pin_memory(), self.noise_off.pin_memory()
        self.noise = self.noise.pin_memory() if self.noise.numel() else self.noise
        if self.aug_ops is not None:
            self.aug_ops, self.aug_args = self.aug_ops.pin_memory(), self.aug_args.pin_memory()
        if self.rgeom is not None:
            self.rgeom = self.rgeom.pin_memory()
        return self

    def to(self, device):
        """(frames, desc, boxes) on `device` -- the arguments of jepa_amd.hip.ops.clip_transform."""
        return self.frames.to(device), self.desc.to(device), self.boxes.to(device)


def collate_raw_clips(batch, *, collate_fn_map=None):
    """default_collate of a list of RawClip -> one validated RawClipBatch.  Clips that carry V views each give V * B rows,
    view-major, over ONE copy of every clip's frames."""
    first = batch[0]
    T, V = first.frames.shape[0], first.num_views
    for c in batch:
        if c.frames.shape[0] != T or tuple(c.boxes.shape[-2:]) != (T, 4) or c.num_views != V:
            raise ValueError("collate: clips of one batch must have the same number of frames and views")
        if (c.crop_size, c.mean, c.std, c.pre) != (first.crop_size, first.mean, first.std, first.pre):
            raise ValueError("collate: clips of one batch must come from one transform (crop size, mean / std, normalise-first flag)")
    flat, offs = pack_buffers([c.frames for c in batch])
    rows = [(c, off, v) for v in range(V) for c, off in zip(batch, offs)]
    desc = torch.tensor([[off, c.frames.shape[1], c.frames.shape[2], int(c.flip)] for c, off, _ in rows],
                        dtype=torch.int64).reshape(len(rows), 4)
    boxes = torch.stack([c.boxes.reshape(V, T, 4)[v] for c, _, v in rows])
    ebox, noise, noise_off = collate_erase([c for c, _, _ in rows])
    aug_ops, aug_args = collate_aug([c for c, _, _ in rows])
    rgeom = None
    if any(c.resize is not None for c in batch):
        rgeom = torch.tensor([c.resize if c.resize is not None else tuple(c.frames.shape[1:3]) for c, _, _ in rows],
                             dtype=torch.int32).reshape(len(rows), 2)
    return RawClipBatch(flat, desc, boxes, first.crop_size, first.mean, first.std, pre=first.pre, num_views=V, ebox=ebox,
                        noise=noise, noise_off=noise_off, aug_ops=aug_ops,
                        aug_args=aug_args, rgeom=rgeom).validate()


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
