"""Tensor-level wrappers over the C ABI (include/vjepa_hip.h).

Every function takes CUDA(HIP) torch tensors and enqueues the kernel on `torch.cuda.current_stream()` (or the `stream=` handle
given).  PyTorch is only the allocator and stream provider here; no torch operator computes anything on this path.

What is checked, and where:
  * everywhere: the device.  `_ptr` (and `_addr`, for the two descriptor arrays built from raw addresses) is the only way a tensor
    becomes a pointer, and it refuses a tensor that is not on the GPU with ValueError -- a host address never reaches a kernel.
  * per wrapper, before anything is allocated, queried or launched: dtype (TypeError), contiguity and shapes (ValueError) of the
    arguments the wrapper names in its `_req` / `_dev` lines.  The per-block wrappers (layernorm_*, gemm_nt, attn_*, colsum,
    gemm_wgrad_tn*, add_pos) check their leading operands only: the Python chain issues them about a thousand times per iteration.
Every kernel goes through `_launch`, which raises HipKernelError naming the symbol it called.
"""
import ctypes
import math

import torch

from .lib import VjReduceSeg, VjSeg, check, load_library

BF16 = torch.bfloat16
F32 = torch.float32
I64 = torch.int64
I32 = torch.int32

EPI_BF16, EPI_GELU, EPI_DGELU, EPI_F32 = 0, 1, 2, 3
EPI_QKV = 4   # EPI_BF16 whose first N/3 output columns (the q part of a qkv projection) are multiplied by alpha before the rounding

_raw_stream = torch._C._cuda_getCurrentRawStream   # C accessor: ~20x cheaper than torch.cuda.current_stream()
_dev_index = None


def _device():
    global _dev_index
    if _dev_index is None:
        _dev_index = torch.cuda.current_device()   # one process per GPU: the device never changes afterwards
    return _dev_index


def _stream(stream=None):
    return ctypes.c_void_p(_raw_stream(_device()) if stream is None else stream)


_NOT_ON_GPU = "must live on the GPU (jepa_amd has no CPU compute path)"


def _ptr(t):
    """Tensor -> device pointer (None -> NULL): the only tensor-to-pointer spelling; a host tensor is refused."""
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError(f"tensor {tuple(t.shape)} {t.dtype}: {_NOT_ON_GPU}")
    return ctypes.c_void_p(t.data_ptr())


def _addr(t, name):
    """_ptr's sibling for descriptor arrays that hold raw addresses: the device address as an int."""
    if not t.is_cuda:
        raise ValueError(f"{name}: {_NOT_ON_GPU}")
    return t.data_ptr()


def _dev(t, dtype, name):
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{name}: {_NOT_ON_GPU}")
    return t


def _req(t, dtype, name):
    if not _dev(t, dtype, name).is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


def _opt(t, dtype, name):
    """_req of a nullable argument: checked only when given."""
    return t if t is None else _req(t, dtype, name)


def _rows2d(t, dtype, name):
    """_dev + the layout the GEMMs read: 2-D, unit inner stride (the row stride may exceed the width)."""
    if _dev(t, dtype, name).dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: must be 2-D with unit inner stride, got {tuple(t.shape)} with strides {t.stride()}")
    return t


def _launch(name, *args, stream=None, timer=None):
    """Enqueue the library's `name`(*args, stream handle) and raise through check() under that same name.  timer = (family, work):
    while KERNEL_TIMERS is set, the call goes between two HIP events on the current stream, kept under `family` with the
    launch's `work` (FLOP)."""
    fn = getattr(load_library(), name)
    s = _stream(stream)
    if timer is None or KERNEL_TIMERS is None:
        return check(fn(*args, s), name)
    family, work = timer
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    KERNEL_TIMERS.setdefault(family, []).append((e0, e1, work))
    e0.record()
    check(fn(*args, s), name)
    e1.record()


def _query(name, *args):
    """A host-side query of the library (workspace sizes, row counts): launches nothing."""
    return getattr(load_library(), name)(*args)


def grow_only(bufs, key, nbytes, grown, device):
    """bufs[key]: a device buffer (uint8) of at least nbytes, allocated with grown(nbytes) bytes when it is missing or too small --
    the one body of Scratch and engine.chain.Workspace.  A buffer is only replaced after a device-wide synchronise, so no
    enqueued kernel can still be using the old allocation, which is dropped before the new one is made."""
    buf = bufs.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            torch.cuda.synchronize(device)
            bufs[key] = buf = None
        buf = bufs[key] = torch.empty(grown(nbytes), dtype=torch.uint8, device=device)
    return buf


class Scratch:
    """Per-(device, tag, STREAM) scratch workspace for kernels that need partial-sum buffers.  The step runs kernels
    on two streams at once (dgrad chain / weight gradients), so two launches of the same kernel family may be in
    flight together: each stream gets its own buffer, of exactly the largest size asked for so far (1 MiB at least)."""

    _bufs = {}

    @classmethod
    def get(cls, nbytes, device, tag="default", stream=None):
        dev = _device()
        key = (dev, tag, _raw_stream(dev) if stream is None else stream)
        return grow_only(cls._bufs, key, nbytes, _scratch_bytes, device)


def _scratch_bytes(nbytes):
    return max(int(nbytes), 1 << 20)


# ---------------------------------------------------------------- rows
def gather_rows(src, idx, out=None, stream=None):
    """out[b,k,:] = src[b, idx[b,k], :]; src [B,N,D] or a broadcast table [1,N,D] / [N,D].  Bit-exact."""
    idx = _req(idx, I64, "idx")
    B, K = idx.shape
    if not src.is_contiguous():
        raise ValueError("src must be contiguous")
    D = src.shape[-1]
    if src.dim() == 2 or (src.shape[0] == 1 and B > 1):
        bstride = 0  # broadcast table (pos-embed)
    elif src.dim() == 3 and src.shape[0] == B:
        bstride = src.shape[1]
    else:
        raise ValueError(f"gather_rows: batch mismatch src {tuple(src.shape)} idx {tuple(idx.shape)}")
    if out is None:
        out = torch.empty((B, K, D), dtype=src.dtype, device=src.device)
    _launch("vj_gather_rows", _ptr(src), _ptr(out), _ptr(idx), B, K, D * src.element_size(), bstride, stream=stream)
    return out


def scatter_rows(src, idx, N, stream=None):
    """zeros[B,N,D] with out[b, idx[b,k], :] = src[b,k,:] (backward of gather_rows)."""
    idx = _req(idx, I64, "idx")
    B, K = idx.shape
    D = src.shape[-1]
    out = torch.empty((B, N, D), dtype=src.dtype, device=src.device)
    _launch("vj_scatter_rows", _ptr(src.contiguous()), _ptr(out), _ptr(idx), B, N, K, D * src.element_size(), stream=stream)
    return out


def copy_rows(src, dst, B, src_rows, src_off, dst_rows, dst_off, n, D, stream=None):
    """dst[b, dst_off+j, :] = src[b, src_off+j, :], j < n, on bf16 rows of D elements; src None zero-fills those rows."""
    _opt(src, BF16, "src")
    _req(dst, BF16, "dst")
    _launch("vj_copy_rows", _ptr(src), _ptr(dst), B, src_rows, src_off, dst_rows, dst_off, n, D, stream=stream)
    return dst


def tubelet_pack(clips, tubelet, patch, idx=None, out=None, stream=None):
    clips = _req(clips, F32, "clips")
    B, C, T, H, W = clips.shape
    N = (T // tubelet) * (H // patch) * (W // patch)
    K = N if idx is None else idx.shape[1]
    kdim = C * tubelet * patch * patch
    if out is None:
        out = torch.empty((B * K, kdim), dtype=BF16, device=clips.device)
    _launch("vj_tubelet_pack", _ptr(clips), _ptr(out), _ptr(idx), B, C, T, H, W, tubelet, patch, K, stream=stream)
    return out


def add_pos(x, pos, B, K, idx=None, stream=None):
    """x [B*K, D] bf16 += pos[(idx or arange)[b,k]] (fp32 table [N,D])."""
    _req(x, BF16, "x")
    _req(pos, F32, "pos")
    _launch("vj_add_pos", _ptr(x), _ptr(pos), _ptr(idx), B, K, x.shape[-1], stream=stream)
    return x


def image_pack(images, tubelet, patch, idx=None, out=None, stream=None):
    """fp32 images [B,C,H,W] -> bf16 [B*K, C*tubelet*patch*patch]: the patch rows of the clip that repeats each image along time,
    one per spatial cell (K = gh*gw) or per idx entry (taken modulo gh*gw).  Bit-identical to tubelet_pack of that clip."""
    images = _req(images, F32, "images")
    _opt(idx, I64, "idx")
    if images.dim() != 4:
        raise ValueError(f"image_pack: expected [B,C,H,W], got {tuple(images.shape)}")
    B, C, H, W = images.shape
    K = (H // patch) * (W // patch) if idx is None else idx.shape[1]
    kdim = C * tubelet * patch * patch
    if out is None:
        out = torch.empty((B * K, kdim), dtype=BF16, device=images.device)
    _launch("vj_image_pack", _ptr(images), _ptr(out), _ptr(idx), B, C, H, W, tubelet, patch, K, stream=stream)
    return out


def clip_transform(frames, desc, boxes, S, mean, std, out=None, stream=None, pre=False):
    """Decoded uint8 frames -> fp32 clips [B,3,T,S,S]: per-frame crop + bilinear resize to S x S, clip flip, (x - mean) / std.
    frames: flat uint8 buffer of [T,Hs,Ws,3] clips; desc int64 [B,4] = (byte offset, Hs, Ws, flip); boxes int32 [B,T,4] =
    (i, j, h, w); mean / std: three floats each in 0..255 units.  The tables must have been validated on the host
    (jepa_amd.app.vjepa.transforms.RawClipBatch.validate) before they were copied to the device.
    pre=True is the frozen eval's normalise-first form (vj_clip_transform_pre): every source pixel becomes (u / 255 - mean) / std
    with mean / std in 0..1 units before the blend, and a box of side S is a bit-exact crop."""
    _req(frames, torch.uint8, "frames")
    _req(desc, I64, "desc")
    _req(boxes, torch.int32, "boxes")
    _opt(out, F32, "out")
    if frames.dim() != 1 or desc.dim() != 2 or desc.shape[1] != 4 or boxes.dim() != 3 or boxes.shape[2] != 4 \
            or boxes.shape[0] != desc.shape[0]:
        raise ValueError(f"clip_transform: frames {tuple(frames.shape)} / desc {tuple(desc.shape)} / boxes {tuple(boxes.shape)}: "
                         "expected [nbytes], [B,4], [B,T,4]")
    B, T = boxes.shape[0], boxes.shape[1]
    mean, std = [float(m) for m in mean], [float(v) for v in std]
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("clip_transform: mean and std take three values each")
    if out is None:
        out = torch.empty((B, 3, T, S, S), dtype=F32, device=frames.device)
    elif tuple(out.shape) != (B, 3, T, S, S):
        raise ValueError(f"clip_transform: out {tuple(out.shape)} is not {(B, 3, T, S, S)}")
    _launch("vj_clip_transform_pre" if pre else "vj_clip_transform", _ptr(frames), frames.numel(), _ptr(desc), _ptr(boxes), _ptr(out),
            B, T, S, *mean, *std, stream=stream)
    return out


def clip_erase(clips, ebox, noise, noise_off, stream=None):
    """RandomErasing in cube mode, in place: clips[b,c,t,top+y,left+x] = noise[noise_off[b] + ((t*3+c)*h+y)*w+x] for
    ebox[b] = (top, left, h, w) (h == 0: clip b stays as it is).  clips fp32 [B,3,T,S,S]; ebox int32 [B,4]; noise fp32 [n];
    noise_off int64 [B].  Bit-exact; an empty noise buffer (no clip of the batch is erased) launches nothing."""
    _req(clips, F32, "clips")
    _req(ebox, torch.int32, "ebox")
    _req(noise, F32, "noise")
    _req(noise_off, I64, "noise_off")
    if clips.dim() != 5 or clips.shape[1] != 3 or clips.shape[3] != clips.shape[4] or tuple(ebox.shape) != (clips.shape[0], 4) \
            or noise.dim() != 1 or tuple(noise_off.shape) != (clips.shape[0],):
        raise ValueError(f"clip_erase: clips {tuple(clips.shape)} / ebox {tuple(ebox.shape)} / noise {tuple(noise.shape)} / noise_off "
                         f"{tuple(noise_off.shape)}: expected [B,3,T,S,S], [B,4], [n], [B]")
    B, _, T, S, _ = clips.shape
    _launch("vj_clip_erase", _ptr(clips), _ptr(ebox), _ptr(noise), noise.numel(), _ptr(noise_off), B, T, S, stream=stream)
    return clips


def clip_randaug_ws_bytes(frames_bytes, B, T):
    """Bytes of workspace clip_randaug needs for a frame buffer of frames_bytes bytes holding B rows of T frames."""
    return int(_query("vj_clip_randaug_ws_bytes", int(frames_bytes), int(B), int(T)))


def clip_randaug(frames, desc, T, aug_ops, aug_args, stream=None, ws=None, fill=None):
    """RandAugment in place on the uint8 frames of a flat clip buffer (the arguments `frames`, `desc` of clip_transform; T frames
    per clip): aug_ops int32 [B,L] and aug_args float64 [B,L,6], L <= 8, are the plans drawn by
    jepa_amd.app.vjepa.randaugment.RandAugmentDraw, one layer per column, applied in order; callers drop the columns in which no
    clip has an operation (every column costs two launches) and validate the tables on the host (RawClipBatch.validate).  Byte
    for byte what the reference's PIL path gives.  ws: a uint8 device buffer of at least clip_randaug_ws_bytes(...) bytes
    (default: this stream's scratch buffer).  fill: None (vj_clip_randaug: the affine family fills with the reference's video
    colour (128, 128, 128)), or three bytes (r, g, b) (vj_clip_randaug_fill: timm's image policies fill with the dataset mean,
    (124, 116, 104))."""
    if fill is not None:
        fill = tuple(fill)
        if len(fill) != 3 or any(int(c) != c or not 0 <= c <= 255 for c in fill):
            raise ValueError(f"clip_randaug: fill={fill} is not three bytes (r, g, b)")
        fill = tuple(int(c) for c in fill)
    _req(frames, torch.uint8, "frames")
    _req(desc, I64, "desc")
    _req(aug_ops, torch.int32, "aug_ops")
    _req(aug_args, torch.float64, "aug_args")
    _opt(ws, torch.uint8, "ws")
    if frames.dim() != 1 or desc.dim() != 2 or desc.shape[1] != 4 or aug_ops.dim() != 2 or aug_ops.shape[0] != desc.shape[0] \
            or tuple(aug_args.shape) != (aug_ops.shape[0], aug_ops.shape[1], 6) or aug_ops.shape[1] > 8:
        raise ValueError(f"clip_randaug: frames {tuple(frames.shape)} / desc {tuple(desc.shape)} / aug_ops {tuple(aug_ops.shape)} / "
                         f"aug_args {tuple(aug_args.shape)}: expected [nbytes], [B,4], [B,L], [B,L,6] with L <= 8")
    if int(T) <= 0:
        raise ValueError(f"clip_randaug: T={T} frames per clip")
    B, L = aug_ops.shape
    need = clip_randaug_ws_bytes(frames.numel(), B, T)
    if ws is None:
        ws = Scratch.get(need, frames.device, tag="clip_randaug", stream=stream)
    elif ws.numel() < need:
        raise ValueError(f"clip_randaug: ws of {ws.numel()} bytes, {need} needed")
    _launch("vj_clip_randaug" if fill is None else "vj_clip_randaug_fill", _ptr(frames), frames.numel(), _ptr(desc), B, int(T),
            _ptr(aug_ops), _ptr(aug_args), L, _ptr(ws), ws.numel(), *(fill or ()), stream=stream)
    return frames


BILINEAR, BICUBIC = 0, 1   # filter codes of ImageResample


class ImageResample:
    """vj_image_resample: PIL's antialiased resample of decoded uint8 images, the first kernel of the image evals' input edge.  A
    namespace like Scratch: `ImageResample.run(...)` launches, `ImageResample.ws_bytes(...)` sizes its workspace."""

    @staticmethod
    def ws_bytes(B, S, taps_x, taps_y, rows):
        """Bytes of workspace `run` needs for B images at output side S with those capacities."""
        need = int(_query("vj_image_resample_ws_bytes", int(B), int(S), int(taps_x), int(taps_y), int(rows)))
        if need < 0:
            raise ValueError(f"ImageResample.ws_bytes: bad dims B={B} S={S} taps_x={taps_x} taps_y={taps_y} rows={rows}")
        return need

    @staticmethod
    def run(frames, desc, geom, S, filter, taps_x, taps_y, rows, out=None, stream=None, ws=None):
        """frames / desc as clip_transform takes them (image b: [Hs,Ws,3]); geom int32 [B,8] = (i, j, h, w, OH, OW, wy, wx): crop box ->
        OH x OW -> the S x S window at (wy, wx) -> out uint8 [B,S,S,3], byte for byte Image.crop(box).resize((OW, OH), filter).
        filter: BILINEAR or BICUBIC.  taps_x, taps_y, rows: the capacities of the batch (RawImageBatch.capacities); the tables must
        have been validated on the host (RawImageBatch.validate).  ws: a uint8 device buffer of at least ws_bytes(...) bytes
        (default: this stream's scratch buffer)."""
        _req(frames, torch.uint8, "frames")
        _req(desc, I64, "desc")
        _req(geom, torch.int32, "geom")
        _opt(out, torch.uint8, "out")
        _opt(ws, torch.uint8, "ws")
        if frames.dim() != 1 or desc.dim() != 2 or desc.shape[1] != 4 or tuple(geom.shape) != (desc.shape[0], 8):
            raise ValueError(f"ImageResample: frames {tuple(frames.shape)} / desc {tuple(desc.shape)} / geom {tuple(geom.shape)}: "
                             "expected [nbytes], [B,4], [B,8]")
        B, S = desc.shape[0], int(S)
        if S <= 0 or S % 4 != 0:
            raise ValueError(f"ImageResample: S={S} must be a positive multiple of 4")
        if out is None:
            out = torch.empty((B, S, S, 3), dtype=torch.uint8, device=frames.device)
        elif tuple(out.shape) != (B, S, S, 3):
            raise ValueError(f"ImageResample: out {tuple(out.shape)} is not {(B, S, S, 3)}")
        if B == 0:
            return out
        need = ImageResample.ws_bytes(B, S, taps_x, taps_y, rows)
        if ws is None:
            ws = Scratch.get(need, frames.device, tag="image_resample", stream=stream)
        elif ws.numel() < need:
            raise ValueError(f"ImageResample: ws of {ws.numel()} bytes, {need} needed")
        _launch("vj_image_resample", _ptr(frames), frames.numel(), _ptr(desc), _ptr(geom), _ptr(out), B, S, int(filter), int(taps_x),
                int(taps_y), int(rows), _ptr(ws), ws.numel(), stream=stream)
        return out


class _ClipResample:
    """`ops.clip_resample(...)`: vj_clip_resample, the short-side Resize of the video evals' validation transforms on the device, with
    `ops.clip_resample.ws_bytes(...)` sizing its workspace.  A callable object like image_hflip below, for the same reason."""

    @staticmethod
    def ws_bytes(B, T, caps):
        """Bytes of workspace a call needs for B clips of T frames with the capacities caps = (oh, ow, taps_x, taps_y, rows)."""
        need = int(_query("vj_clip_resample_ws_bytes", int(B), int(T), *(int(c) for c in caps)))
        if need < 0:
            raise ValueError(f"clip_resample.ws_bytes: bad dims B={B} T={T} (oh, ow, taps_x, taps_y, rows)={tuple(caps)}")
        return need

    @staticmethod
    def __call__(frames, desc, rgeom, T, filter, caps, out, desc_out, stream=None, ws=None):
        """vj_clip_resample: PIL's Image.resize((OW, OH), filter) of every frame of every clip, byte for byte, into a second frame buffer.
        frames / desc as clip_transform takes them (clip b: [T,Hs,Ws,3]); rgeom int32 [B,2] = (OH, OW); out: a flat uint8 buffer;
        desc_out int64 [B,4] = (byte offset in out, a multiple of 16; OH; OW; the flag): clip b is written as [T,OH,OW,3] there and no
        other byte of out changes, so (out, desc_out) is what clip_transform / clip_randaug take next.  filter: BILINEAR or BICUBIC.
        caps = (oh, ow, taps_x, taps_y, rows): the capacities of the batch, maxima of OH, OW, the taps per axis and the source height
        (RawClipBatch.resample_plan gives them with rgeom and desc_out, validated on the host).  ws: a uint8 device buffer of at least
        ws_bytes(...) bytes (default: this stream's scratch buffer).  B == 0 launches nothing."""
        _req(frames, torch.uint8, "frames")
        _req(desc, I64, "desc")
        _req(rgeom, torch.int32, "rgeom")
        _req(out, torch.uint8, "out")
        _req(desc_out, I64, "desc_out")
        _opt(ws, torch.uint8, "ws")
        B = desc.shape[0]
        if frames.dim() != 1 or out.dim() != 1 or desc.dim() != 2 or desc.shape[1] != 4 or tuple(rgeom.shape) != (B, 2) \
                or tuple(desc_out.shape) != (B, 4):
            raise ValueError(f"clip_resample: frames {tuple(frames.shape)} / desc {tuple(desc.shape)} / rgeom {tuple(rgeom.shape)} / out "
                             f"{tuple(out.shape)} / desc_out {tuple(desc_out.shape)}: expected [nbytes], [B,4], [B,2], [nbytes], [B,4]")
        if int(T) <= 0:
            raise ValueError(f"clip_resample: T={T} frames per clip")
        if int(filter) not in (BILINEAR, BICUBIC):
            raise ValueError(f"clip_resample: filter={filter} (BILINEAR or BICUBIC)")
        if len(caps) != 5:
            raise ValueError(f"clip_resample: caps={caps} is not (oh, ow, taps_x, taps_y, rows)")
        if B == 0:
            return out
        need = _ClipResample.ws_bytes(B, T, caps)
        if ws is None:
            ws = Scratch.get(need, frames.device, tag="clip_resample", stream=stream)
        elif ws.numel() < need:
            raise ValueError(f"clip_resample: ws of {ws.numel()} bytes, {need} needed")
        _launch("vj_clip_resample", _ptr(frames), frames.numel(), _ptr(desc), _ptr(rgeom), _ptr(out), out.numel(), _ptr(desc_out), B, int(T),
                int(filter), *(int(c) for c in caps), _ptr(ws), ws.numel(), stream=stream)
        return out


clip_resample = _ClipResample()


class _ImageHflip:
    """`ops.image_hflip(images, desc, flips, stream=None)`: vj_image_hflip on the buffer ImageResample.run writes.  A callable object
    beside that namespace, not a module-level function: the public functions of this module are the per-kernel wrappers of the
    training step and the evals' compute path, which tests/test_ops_host.py tabulates row by row."""

    @staticmethod
    def __call__(images, desc, flips, stream=None):
        """Mirror, in place, the flagged images of a uint8 [B,S,S,3] buffer (ImageResample.run's output, S % 4 == 0): what PIL's
        transpose(FLIP_LEFT_RIGHT) gives, on the uint8 side, where timm flips before its AutoAugment policy.  desc: the device int64
        [B,4] table whose column 3 holds the flags (RawImageBatch.resampled_tables); flips: the same flags on the HOST (B values) --
        a batch without a flagged image, or without an image, launches nothing."""
        _dev(images, torch.uint8, "images")
        _req(desc, I64, "desc")
        if images.dim() != 4 or images.shape[1] != images.shape[2] or images.shape[3] != 3 or tuple(desc.shape) != (images.shape[0], 4):
            raise ValueError(f"image_hflip: images {tuple(images.shape)} / desc {tuple(desc.shape)}: expected [B,S,S,3], [B,4]")
        B, S = images.shape[0], images.shape[1]
        flips = [bool(f) for f in (flips.tolist() if torch.is_tensor(flips) else flips)]
        if len(flips) != B:
            raise ValueError(f"image_hflip: {len(flips)} host flags for {B} images")
        if S % 4 != 0:
            raise ValueError(f"image_hflip: S={S} must be a positive multiple of 4")
        if B * S * S * 3 >= 1 << 31:
            raise ValueError(f"image_hflip: a buffer of {B * S * S * 3} bytes, below 2^31 are taken")
        _req(images, torch.uint8, "images")
        flagged = sum(flips)
        if B == 0 or flagged == 0:
            return images
        _launch("vj_image_hflip", _ptr(images), _ptr(desc), B, S, flagged, stream=stream)
        return images


image_hflip = _ImageHflip()


def add_pos_bcast(y, pos, B, S, Gt, out=None, stream=None):
    """out[b, t*S+s] = bf16(y[b,s] + pos[t*S+s]), t < Gt; y bf16 [B*S, D], pos fp32 [Gt*S, D] -> bf16 [B*Gt*S, D]."""
    _req(y, BF16, "y")
    _req(pos, F32, "pos")
    D = y.shape[-1]
    if y.numel() != B * S * D or pos.numel() != Gt * S * D:
        raise ValueError(f"add_pos_bcast: y {tuple(y.shape)} / pos {tuple(pos.shape)} do not match B={B} S={S} Gt={Gt}")
    if out is None:
        out = torch.empty((B * Gt * S, D), dtype=BF16, device=y.device)
    _launch("vj_add_pos_bcast", _ptr(y), _ptr(pos), _ptr(out), B, S, Gt, D, stream=stream)
    return out


def slice_sum(dx, B, S, Gt, out=None, stream=None):
    """out[b, s] = bf16(sum_{t<Gt} dx[b, t*S+s]) in fp32, slice 0 first and then ascending t, one rounding; dx bf16 [B*Gt*S, D] ->
    bf16 [B*S, D].  The adjoint of add_pos_bcast: the gradient of a still image's S distinct patch embeddings."""
    _req(dx, BF16, "dx")
    _opt(out, BF16, "out")
    D = dx.shape[-1]
    if dx.numel() != B * Gt * S * D or (out is not None and out.numel() != B * S * D):
        raise ValueError(f"slice_sum: dx {tuple(dx.shape)} / out {None if out is None else tuple(out.shape)} do not match B={B} S={S} "
                         f"Gt={Gt}")
    if out is None:
        out = torch.empty((B * S, D), dtype=BF16, device=dx.device)
    _launch("vj_slice_sum", _ptr(dx), _ptr(out), B, S, Gt, D, stream=stream)
    return out


def pos_interp3d(table, scale_factor, stream=None):
    """Trilinear F.interpolate(scale_factor=..., align_corners=False) of an fp32 position table [Nt,Nh,Nw,D] along its three grid
    axes -> [floor(Nt*st), floor(Nh*sh), floor(Nw*sw), D]."""
    _req(table, F32, "table")
    Nt, Nh, Nw, D = table.shape
    st, sh, sw = (float(s) for s in scale_factor)
    To, Ho, Wo = (int(math.floor(float(n) * s)) for n, s in ((Nt, st), (Nh, sh), (Nw, sw)))
    out = torch.empty((max(To, 0), max(Ho, 0), max(Wo, 0), D), dtype=F32, device=table.device)
    _launch("vj_pos_interp3d", _ptr(table), _ptr(out), Nt, Nh, Nw, D, st, sh, sw, To, Ho, Wo, stream=stream)
    return out


def pos_interp2d_bicubic(table, scale_factor, stream=None):
    """Bicubic F.interpolate(scale_factor=s, align_corners=False) of an fp32 position table [Nh,Nw,D] along its two grid axes ->
    [floor(Nh*s), floor(Nw*s), D]."""
    _req(table, F32, "table")
    Nh, Nw, D = table.shape
    s = float(scale_factor)
    Ho, Wo = (int(math.floor(float(n) * s)) for n in (Nh, Nw))
    out = torch.empty((max(Ho, 0), max(Wo, 0), D), dtype=F32, device=table.device)
    _launch("vj_pos_interp2d_bicubic", _ptr(table), _ptr(out), Nh, Nw, D, s, Ho, Wo, stream=stream)
    return out


def add_pos_frames(x, pos, idx, N, stream=None):
    """x bf16 [B, F*N, D] += pos[idx[b,f]] on the N token rows of frame f (fp32 table [max_frames, D], idx int64 [B,F] already
    validated against the table on the host); in place."""
    _req(x, BF16, "x")
    _req(pos, F32, "pos")
    _req(idx, I64, "idx")
    B, F = idx.shape
    D = x.shape[-1]
    if x.numel() != B * F * N * D or pos.dim() != 2 or pos.shape[1] != D:
        raise ValueError(f"add_pos_frames: x {tuple(x.shape)} / pos {tuple(pos.shape)} do not match idx {tuple(idx.shape)}, N={N}")
    _launch("vj_add_pos_frames", _ptr(x), _ptr(pos), _ptr(idx), B, F, N, D, pos.shape[0], stream=stream)
    return x


# ---------------------------------------------------------------- stochastic depth
def _drop_path_args(what, a, b, scale, B, S):
    """The checks of both drop-path kernels: bf16 rows a (and b, when it exists already) [B*S, D], fp32 scale [B] -> D."""
    _req(a, BF16, what + ": rows")
    _opt(b, BF16, what + ": rows")
    _req(scale, F32, what + ": scale")
    D = a.shape[-1]
    if a.numel() != B * S * D or (b is not None and b.shape != a.shape) or scale.numel() != B:
        raise ValueError(f"{what}: rows {tuple(a.shape)} / {None if b is None else tuple(b.shape)} and scale {tuple(scale.shape)} "
                         f"do not match B={B} S={S}")
    return D


def drop_path_add(x, y, scale, B, S, stream=None):
    """y [B*S, D] bf16 <- bf16(x + scale[b] * y) on the S rows of sample b, in place (one fp32 fused multiply-add, one rounding);
    where scale[b] == 0 the rows become x's bits and y is not read.  scale fp32 [B]."""
    D = _drop_path_args("drop_path_add", x, y, scale, B, S)
    _launch("vj_drop_path_add", _ptr(x), _ptr(y), _ptr(scale), B, S, D, stream=stream)
    return y


def drop_path_scale(dx, scale, B, S, out=None, stream=None):
    """bf16(scale[b] * dx) on the S rows of sample b -> out (new unless given); where scale[b] == 0 the rows are +0 and dx is not
    read.  dx bf16 [B*S, D], scale fp32 [B]."""
    D = _drop_path_args("drop_path_scale", dx, out, scale, B, S)
    if out is None:
        out = torch.empty_like(dx)
    _launch("vj_drop_path_scale", _ptr(dx), _ptr(out), _ptr(scale), B, S, D, stream=stream)
    return out


# ---------------------------------------------------------------- mixup / cutmix / soft-target cross-entropy
def _host_table(t, dtype, name):
    t = torch.as_tensor(t)
    if t.is_cuda:
        raise ValueError(f"{name}: a host table is expected here (it is validated on the host and then uploaded)")
    return t.to(dtype).contiguous()


def _checked(t, name, helper):
    """The record a device table carries from the helper that validated its host copy before uploading it."""
    mark = getattr(t, "_vj_checked", None)
    if mark is None:
        raise ValueError(f"{name}: not a table uploaded by ops.{helper} (the kernels trust these tables: they are validated on the host "
                         "before the upload, never read back)")
    return mark


def mix_tables(lam, box, H, W, device):
    """The two per-sample tables of clip_mix, validated on the host and uploaded: lam [B] -> fp32, box [B,4] = (y0, y1, x0, x1) ->
    int32 with 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W in every row.  Returns the device tensors (lam, box)."""
    lam, box = _host_table(lam, F32, "lam"), _host_table(box, I32, "box")
    if lam.dim() != 1 or tuple(box.shape) != (lam.shape[0], 4):
        raise ValueError(f"mix_tables: lam {tuple(lam.shape)} / box {tuple(box.shape)}: expected [B], [B,4]")
    if not bool(torch.isfinite(lam).all()):
        raise ValueError("mix_tables: lam must be finite")
    y0, y1, x0, x1 = box.unbind(1)
    if not bool(((0 <= y0) & (y0 <= y1) & (y1 <= H) & (0 <= x0) & (x0 <= x1) & (x1 <= W)).all()):
        raise ValueError(f"mix_tables: every box needs 0 <= y0 <= y1 <= {H} and 0 <= x0 <= x1 <= {W}, got {box.tolist()}")
    lam_d, box_d = lam.to(device, non_blocking=True), box.to(device, non_blocking=True)
    box_d._vj_checked = (int(H), int(W))
    return lam_d, box_d


def clip_mix(x, lam, box, stream=None):
    """Mixup / cutmix of a batch with its flipped self, in place (vj_clip_mix): x fp32 [B, ..., H, W]; sample i is mixed with sample
    B-1-i under lam[i] and box[i] = (y0, y1, x0, x1): inside the box the partner's bits, outside it with lam == 1 its own bits, else
    fmaf(lam, x_i, (1 - lam) * x_j).  lam fp32 [B], box int32 [B,4]: the device tables of mix_tables for this H, W."""
    _req(x, F32, "x")
    _req(lam, F32, "lam")
    _req(box, I32, "box")
    if x.dim() < 3:
        raise ValueError(f"clip_mix: x {tuple(x.shape)}: expected [B, ..., H, W]")
    B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    if tuple(lam.shape) != (B,) or tuple(box.shape) != (B, 4):
        raise ValueError(f"clip_mix: lam {tuple(lam.shape)} / box {tuple(box.shape)} do not match x {tuple(x.shape)}: expected [B], [B,4]")
    if _checked(box, "clip_mix: box", "mix_tables") != (H, W):
        raise ValueError(f"clip_mix: box was validated for {box._vj_checked}, x has H, W = {(H, W)}")
    P = math.prod(x.shape[1:-2])
    _launch("vj_clip_mix", _ptr(x), _ptr(lam), _ptr(box), B, P, H, W, stream=stream)
    return x


def soft_ce_tables(label_a, label_b, lam, C, device):
    """The three per-row tables of soft_ce, validated on the host and uploaded: label_a, label_b [R] -> int32 in [0, C), lam [R] ->
    fp32.  Returns the device tensors (label_a, label_b, lam)."""
    a, b, lam = _host_table(label_a, I32, "label_a"), _host_table(label_b, I32, "label_b"), _host_table(lam, F32, "lam")
    if a.dim() != 1 or b.shape != a.shape or lam.shape != a.shape:
        raise ValueError(f"soft_ce_tables: label_a {tuple(a.shape)} / label_b {tuple(b.shape)} / lam {tuple(lam.shape)}: expected [R] each")
    if not bool(((0 <= a) & (a < C) & (0 <= b) & (b < C)).all()):
        raise ValueError(f"soft_ce_tables: labels must lie in [0, {C}), got {a.tolist()} / {b.tolist()}")
    if not bool(torch.isfinite(lam).all()):
        raise ValueError("soft_ce_tables: lam must be finite")
    out = tuple(t.to(device, non_blocking=True) for t in (a, b, lam))
    out[0]._vj_checked = out[1]._vj_checked = int(C)
    return out


def soft_ce(logits, label_a, label_b, lam, smoothing, probs=False, stream=None):
    """Soft-target cross-entropy per row (vj_soft_ce) for the target eps / C + (1 - eps) * (lam * onehot(a) + (1 - lam) * onehot(b)):
    logits fp32 [R,C] (rows may be strided) -> (loss [R], dlogits [R,C] = softmax - target, the soft-max [R,C] or None).
    label_a, label_b int32 [R], lam fp32 [R]: the device tables of soft_ce_tables for this C."""
    for t, dt, name in ((logits, F32, "logits"), (label_a, I32, "label_a"), (label_b, I32, "label_b"), (lam, F32, "lam")):
        _dev(t, dt, name)
    if logits.dim() != 2 or logits.shape[1] < 1 or (logits.shape[0] > 1 and logits.stride(0) < logits.shape[1]) or logits.stride(1) != 1:
        raise ValueError(f"soft_ce: logits {tuple(logits.shape)} with strides {logits.stride()}: expected [R,C], C >= 1, unit column stride")
    R, C = logits.shape
    for t, name in ((label_a, "label_a"), (label_b, "label_b"), (lam, "lam")):
        if tuple(t.shape) != (R,) or not t.is_contiguous():
            raise ValueError(f"soft_ce: {name} {tuple(t.shape)}: expected a contiguous [{R}]")
    for t, name in ((label_a, "label_a"), (label_b, "label_b")):
        if _checked(t, "soft_ce: " + name, "soft_ce_tables") != C:
            raise ValueError(f"soft_ce: {name} was validated for {t._vj_checked} classes, logits have {C}")
    smoothing = float(smoothing)
    if not 0.0 <= smoothing < 1.0:
        raise ValueError(f"soft_ce: smoothing={smoothing} must lie in [0, 1)")
    loss = torch.empty((R,), dtype=F32, device=logits.device)
    dlogits = torch.empty((R, C), dtype=F32, device=logits.device)
    p = torch.empty((R, C), dtype=F32, device=logits.device) if probs else None
    ld = logits.stride(0) if R > 1 else max(logits.stride(0), C)
    _launch("vj_soft_ce", _ptr(logits), ld, _ptr(label_a), _ptr(label_b), _ptr(lam), smoothing, R, C, _ptr(loss), _ptr(dlogits), _ptr(p),
            stream=stream)
    return loss, dlogits, p


# ---------------------------------------------------------------- layernorm
def layernorm_fwd(x, gamma, beta, eps, save_stats=True, out=None, stream=None):
    _req(x, BF16, "x")
    rows, D = x.numel() // x.shape[-1], x.shape[-1]
    y = torch.empty_like(x) if out is None else out
    mean = rstd = None
    if save_stats:
        mean = torch.empty(rows, dtype=F32, device=x.device)
        rstd = torch.empty(rows, dtype=F32, device=x.device)
    _launch("vj_layernorm_fwd", _ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(mean), _ptr(rstd), rows, D, eps, stream=stream)
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta, dres=None, alpha=1.0, accumulate=False, dxsum=None,
                  stream=None):
    """dxsum (optional fp32 [D]): also alpha * column sums of the returned dx (+ old when accumulating) -- the bias
    gradient of the Linear whose dY this dx is (include/vjepa_hip.h: vj_layernorm_bwd_colsum)."""
    _req(dy, BF16, "dy")
    rows, D = x.numel() // x.shape[-1], x.shape[-1]
    dx = torch.empty_like(x)
    nws = _query("vj_layernorm_bwd_ws_bytes", D)
    ws = Scratch.get(nws, x.device, "ln", stream=stream)
    _launch("vj_layernorm_bwd_colsum", _ptr(dy), _ptr(x), _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(dres), _ptr(dx), _ptr(dgamma),
            _ptr(dbeta), _ptr(dxsum), alpha, 1.0 if accumulate else 0.0, rows, D, _ptr(ws), nws, stream=stream)
    return dx


# ---------------------------------------------------------------- gemm
GEMM_FLAGS = 0  # default kernel-selection flags of vj_gemm_bf16_nt (0 = automatic; gemm.hip dispatch_gemm)
KERNEL_TIMERS = None  # bench.py sets this to a dict: name -> list of (start_event, end_event, work) on the launch stream


def gemm_nt(A, B, out=None, bias=None, residual=None, aux_in=None, aux_out=None, epilogue=EPI_BF16, alpha=1.0,
            beta=0.0, M=None, K=None, flags=None, stream=None):
    """C[M,N] = A[M,K] @ B[N,K]^T with a fused epilogue.  A,B bf16 2-D (row stride may exceed K)."""
    _rows2d(A, BF16, "gemm_nt: A")
    _rows2d(B, BF16, "gemm_nt: B")
    M = A.shape[0] if M is None else M
    K = A.shape[1] if K is None else K
    N = B.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=F32 if epilogue == EPI_F32 else BF16, device=A.device)
    aux = aux_in if aux_in is not None else aux_out
    _launch("vj_gemm_bf16_nt", _ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(out), out.stride(0), M, N, K,
            _ptr(bias), _ptr(residual), 0 if residual is None else residual.stride(0),
            _ptr(aux_in), _ptr(aux_out), 0 if aux is None else aux.stride(0), epilogue, alpha, beta,
            GEMM_FLAGS if flags is None else flags, stream=stream, timer=("gemm_nt", 2.0 * M * N * K))
    return out


def ln_rowstats(x, eps, out=None, stream=None):
    """rowstats[m] = {rstd_m, -mean_m * rstd_m} (fp32 [M, 2]) of the bf16 rows x [M, D]: the statistics pass of a LayerNorm that is
    folded into the GEMM consuming it (vj_ln_rowstats)."""
    _req(x, BF16, "x")
    M, D = x.shape
    rs = torch.empty((M, 2), dtype=F32, device=x.device) if out is None else out
    _launch("vj_ln_rowstats", _ptr(x), _ptr(rs), M, D, eps, stream=stream)
    return rs


def ln_fold_weights(W, b, gamma, beta, Wf=None, cvec=None, bf=None, stream=None):
    """Wf = bf16(W * gamma) [N, K], cvec[n] = sum_k Wf[n, k], bf = b + W beta (vj_ln_fold_weights); W fp32 [N, K] contiguous."""
    for t, nm in ((W, "W"), (gamma, "gamma"), (beta, "beta")):
        _req(t, F32, "ln_fold_weights: " + nm)
    N, K = W.shape
    Wf = torch.empty((N, K), dtype=BF16, device=W.device) if Wf is None else Wf
    cvec = torch.empty((N,), dtype=F32, device=W.device) if cvec is None else cvec
    bf = torch.empty((N,), dtype=F32, device=W.device) if bf is None else bf
    _launch("vj_ln_fold_weights", _ptr(W), _ptr(b), _ptr(gamma), _ptr(beta), _ptr(Wf), _ptr(cvec), _ptr(bf), N, K, stream=stream)
    return Wf, cvec, bf


def gemm_nt_lnfold(X, Wf, bf, rowstats, cvec, out=None, epilogue=EPI_BF16, alpha=1.0, flags=None, stream=None):
    """out = LayerNorm(X) W^T + b from the RAW bf16 rows X [M, K] (vj_gemm_bf16_nt_lnfold): Wf / cvec / bf from ln_fold_weights,
    rowstats from ln_rowstats; epilogue EPI_BF16, EPI_GELU or EPI_QKV (first N/3 columns times alpha)."""
    _rows2d(X, BF16, "gemm_nt_lnfold: X")
    _rows2d(Wf, BF16, "gemm_nt_lnfold: Wf")
    M, K = X.shape
    N = Wf.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=BF16, device=X.device)
    _launch("vj_gemm_bf16_nt_lnfold", _ptr(X), X.stride(0), _ptr(Wf), Wf.stride(0), _ptr(out), out.stride(0), M, N, K, _ptr(bf),
            _ptr(rowstats), _ptr(cvec), epilogue, alpha, GEMM_FLAGS if flags is None else flags, stream=stream)
    return out


WGRAD_WS_BYTES = 96 << 20
GROUP_WS_BYTES = 192 << 20   # the grouped launch's workspace, same size as the C chain's (same split factor -> same bits)


def gemm_wgrad(dyT, xT, out, alpha=1.0, beta=0.0, flags=None, stream=None):
    """out[N_out, K_in] (fp32) = alpha * dyT[N_out, Tp] @ xT[K_in, Tp]^T + beta*out, split-K over the tokens (row strides may
    exceed the widths)."""
    _rows2d(dyT, BF16, "dyT")
    _rows2d(xT, BF16, "xT")
    _rows2d(out, F32, "out")
    M, K = dyT.shape
    N = xT.shape[0]
    ws = Scratch.get(WGRAD_WS_BYTES, dyT.device, "wgrad", stream=stream)
    _launch("vj_gemm_bf16_nt_splitk", _ptr(dyT), dyT.stride(0), _ptr(xT), xT.stride(0), _ptr(out), out.stride(0), M, N, K, alpha, beta,
            GEMM_FLAGS if flags is None else flags, _ptr(ws), WGRAD_WS_BYTES, stream=stream, timer=("gemm_nt", 2.0 * M * N * K))
    return out


def gemm_wgrad_tn_grouped(problems, alpha=1.0, beta=0.0, stream=None):
    """problems: [(dy [T, N1] bf16, x [T, N2] bf16, out [N1, N2] fp32), ...] (at most 4, same T): every out = alpha *
    dy^T @ x + beta * out in ONE launch (vj_gemm_bf16_tn_grouped)."""
    T = problems[0][0].shape[0]
    flat = []
    for dy, x, out in problems:
        _req(dy, BF16, "dy")
        _req(x, BF16, "x")
        assert dy.shape[0] == T and x.shape[0] == T and out.shape == (dy.shape[1], x.shape[1]) and out.dtype == F32
        flat += [_addr(dy, "dy"), dy.stride(0), _addr(x, "x"), x.stride(0), _addr(out, "out"), out.stride(0), dy.shape[1], x.shape[1]]
    arr = (ctypes.c_int64 * len(flat))(*[int(v) for v in flat])
    ws = Scratch.get(GROUP_WS_BYTES, problems[0][0].device, "wgrad_group", stream=stream)
    _launch("vj_gemm_bf16_tn_grouped", ctypes.addressof(arr), len(problems), T, alpha, beta, _ptr(ws), GROUP_WS_BYTES, stream=stream,
            timer=("gemm_nt", sum(2.0 * T * dy.shape[1] * x.shape[1] for dy, x, _ in problems)))


def gemm_wgrad_tn(dy, x, out, alpha=1.0, beta=0.0, stream=None):
    """out[N_out, K_in] (fp32) = alpha * dy[T, N_out]^T @ x[T, K_in] + beta*out: no operand transposes, split-K over T."""
    _req(dy, BF16, "dy")
    _req(x, BF16, "x")
    T, N1 = dy.shape
    N2 = x.shape[1]
    ws = Scratch.get(WGRAD_WS_BYTES, dy.device, "wgrad", stream=stream)
    _launch("vj_gemm_bf16_tn_splitk", _ptr(dy), dy.stride(0), _ptr(x), x.stride(0), _ptr(out), out.stride(0), T, N1, N2, alpha, beta,
            _ptr(ws), WGRAD_WS_BYTES, stream=stream, timer=("gemm_nt", 2.0 * T * N1 * N2))
    return out


def transpose_colsum(x, colsum_out, alpha=1.0, accumulate=False, stream=None):
    """x [M,N] bf16 -> x^T [N, pad64(M)] and colsum_out[n] = alpha*sum_m x[m,n] (+ old) in one pass."""
    _req(x, BF16, "x")
    M, N = x.shape
    Mp = pad64(M)
    out = torch.empty((N, Mp), dtype=BF16, device=x.device)
    nws = _query("vj_transpose_colsum_ws_bytes", M, N)
    ws = Scratch.get(nws, x.device, "tcolsum", stream=stream)
    _launch("vj_transpose_colsum_bf16", _ptr(x), _ptr(out), M, N, x.stride(0), Mp, _ptr(colsum_out), alpha,
            1.0 if accumulate else 0.0, _ptr(ws), nws, stream=stream)
    return out


def pad64(m):
    return (m + 63) // 64 * 64


def transpose(x, M=None, out=None, stream=None):
    """x [M,N] bf16 -> [N, pad64(M)] (zero padded): K-contiguous wgrad operand."""
    _req(x, BF16, "x")
    M = x.shape[0] if M is None else M
    N = x.shape[1]
    Mp = pad64(M)
    if out is None:
        out = torch.empty((N, Mp), dtype=BF16, device=x.device)
    _launch("vj_transpose_bf16", _ptr(x), _ptr(out), M, N, x.stride(0), Mp, stream=stream)
    return out


def transpose_multi(desc, blocks, n_blocks, stream=None):
    """One launch for many transposes: desc int64 [6 * n_tensors] = {src, dst, M, N, ld_in, Mpad}, blocks int32 [4 * n_blocks]."""
    _req(desc, I64, "desc")
    _req(blocks, I32, "blocks")
    _launch("vj_transpose_multi", _ptr(desc), _ptr(blocks), n_blocks, stream=stream)


def colsum(x, out, M=None, alpha=1.0, accumulate=False, group=0, row_lo=0, row_hi=None, stream=None):
    """out[n] (fp32) = alpha * sum_m x[m,n] (+ out); optional per-sample row window for the mask-token grad."""
    _req(x, BF16, "x")
    M = x.shape[0] if M is None else M
    N = x.shape[1]
    nws = _query("vj_colsum_ws_bytes", N)
    ws = Scratch.get(nws, x.device, "colsum", stream=stream)
    if group <= 0:
        group, row_lo, row_hi = max(M, 1), 0, max(M, 1)
    _launch("vj_colsum_bf16", _ptr(x), M, N, x.stride(0), group, row_lo, row_hi, _ptr(out), alpha, 1.0 if accumulate else 0.0,
            _ptr(ws), nws, stream=stream)
    return out


# ---------------------------------------------------------------- attention
def attn_fwd(qkv, B, S, H, hd, scale, save_lse=True, out=None, stream=None):
    """qkv [B*S, 3*H*hd] bf16 (packed [B,S,3,H,hd]) -> o [B*S, H*hd], lse2 [B,H,S]."""
    _req(qkv, BF16, "qkv")
    o = torch.empty((B * S, H * hd), dtype=BF16, device=qkv.device) if out is None else out
    lse = torch.empty((B, H, S), dtype=F32, device=qkv.device) if save_lse else None
    _launch("vj_attn_fwd", _ptr(qkv), _ptr(o), _ptr(lse), B, S, H, hd, scale, stream=stream,
            timer=("attn_fwd", 4.0 * B * H * S * S * hd))
    return o, lse


def seg_array(segs):
    """ctypes array of vj_seg_t over segments given as (row0, B, S) tuples or as objects with those fields (engine.layers.Seg)."""
    arr = (VjSeg * len(segs))()
    for i, s in enumerate(segs):
        arr[i] = VjSeg(*s) if isinstance(s, tuple) else VjSeg(s.row0, s.B, s.S)
    return arr


_seg_array = seg_array


def _attn_bwd_bufs(qkv, segs, H, hd, colsum, stream):
    """What an attention backward over `segs` needs next to its operands: (seg_arr, ws, nws, colq, colkv) -- the stream's "attn"
    scratch and, with colsum, the fp32 column partials of dqkv, the segments' rows one after the other."""
    seg_arr = seg_array(segs)
    nws = _query("vj_attn_bwd_segs_ws_bytes", seg_arr, len(segs), H, hd)
    ws = Scratch.get(nws, qkv.device, "attn", stream=stream)
    colq = colkv = None
    if colsum:
        rq_t = rkv_t = 0
        rq, rkv = ctypes.c_int64(0), ctypes.c_int64(0)
        for sg in seg_arr:
            check(_query("vj_attn_bwd_colsum_rows", sg.B, sg.S, hd, ctypes.byref(rq), ctypes.byref(rkv)), "vj_attn_bwd_colsum_rows")
            rq_t, rkv_t = rq_t + (rq.value if sg.B * sg.S else 0), rkv_t + (rkv.value if sg.B * sg.S else 0)
        colq = torch.empty((rq_t, H * hd), dtype=F32, device=qkv.device)
        colkv = torch.empty((rkv_t, 2 * H * hd), dtype=F32, device=qkv.device)
    return seg_arr, ws, nws, colq, colkv


def attn_bwd(qkv, o, dout, lse, B, S, H, hd, scale, out=None, stream=None):
    _req(dout, BF16, "dout")
    dqkv = torch.empty_like(qkv) if out is None else out
    _, ws, nws, _, _ = _attn_bwd_bufs(qkv, [(0, B, S)], H, hd, False, stream)
    _launch("vj_attn_bwd", _ptr(qkv), _ptr(o), _ptr(dout), _ptr(lse), _ptr(dqkv), B, S, H, hd, scale, _ptr(ws), nws, stream=stream,
            timer=("attn_bwd", 8.0 * B * H * S * S * hd))
    return dqkv


def attn_fwd_segs(qkv, segs, H, hd, scale, save_lse=True, stream=None):
    """Attention over several [B_i, S_i] segments of one activation in ONE launch (vj_attn_fwd_segs).  qkv [M, 3*H*hd] bf16;
    segs: list of (row0, B, S) -> o [M, H*hd], lse2 flat [H*M] (segment i: [B_i, H, S_i] at H*row0_i)."""
    _req(qkv, BF16, "qkv")
    M = qkv.shape[0]
    o = torch.empty((M, H * hd), dtype=BF16, device=qkv.device)
    lse = torch.empty((H * M,), dtype=F32, device=qkv.device) if save_lse else None
    _launch("vj_attn_fwd_segs", _ptr(qkv), _ptr(o), _ptr(lse), seg_array(segs), len(segs), H, hd, scale, stream=stream)
    return o, lse


def attn_bwd_segs(qkv, o, dout, lse, segs, H, hd, scale, colsum=False, stream=None):
    """Backward of attn_fwd_segs in one launch pair (vj_attn_bwd_segs) -> dqkv [, colq, colkv: the segments' column partials one
    after the other]."""
    _req(dout, BF16, "dout")
    dqkv = torch.empty_like(qkv)
    seg_arr, ws, nws, colq, colkv = _attn_bwd_bufs(qkv, segs, H, hd, colsum, stream)
    _launch("vj_attn_bwd_segs", _ptr(qkv), _ptr(o), _ptr(dout), _ptr(lse), _ptr(dqkv), seg_arr, len(segs), H, hd, scale, _ptr(ws), nws,
            _ptr(colq), _ptr(colkv), stream=stream)
    return (dqkv, colq, colkv) if colsum else dqkv


def attn_bwd_colsum(qkv, o, dout, lse, B, S, H, hd, scale, out=None, stream=None):
    """attn_bwd + fp32 column partials of dqkv over this segment (vj_attn_bwd_colsum): returns (dqkv, colq [rows_q, H*hd],
    colkv [rows_kv, 2*H*hd]); the qkv bias gradient is colq.sum(0) | colkv.sum(0) (reduce_segments on the product path)."""
    _req(dout, BF16, "dout")
    dqkv = torch.empty_like(qkv) if out is None else out
    _, ws, nws, colq, colkv = _attn_bwd_bufs(qkv, [(0, B, S)], H, hd, True, stream)
    _launch("vj_attn_bwd_colsum", _ptr(qkv), _ptr(o), _ptr(dout), _ptr(lse), _ptr(dqkv), B, S, H, hd, scale, _ptr(ws), nws,
            _ptr(colq), _ptr(colkv), stream=stream)
    return dqkv, colq, colkv


def gemm_dgelu_colsum(dy, wT, aux_in, stream=None):
    """fc2 dgrad with fc1's bias-gradient partials (vj_gemm_bf16_nt_dgelu_colsum): returns (du bf16 [M, N], colpart fp32
    [rows, N] or None when the fused kernel did not take the problem -- du is the plain GEMM's either way)."""
    _req(dy, BF16, "dy")
    M, K = dy.shape
    N = wT.shape[0]
    du = torch.empty((M, N), dtype=BF16, device=dy.device)
    rows = _query("vj_gemm_colsum_rows", M)
    colpart = torch.empty((rows, N), dtype=F32, device=dy.device)
    fused = ctypes.c_int(0)
    _launch("vj_gemm_bf16_nt_dgelu_colsum", _ptr(dy), dy.stride(0), _ptr(wT), wT.stride(0), _ptr(du), N, M, N, K, _ptr(aux_in),
            aux_in.stride(0), _ptr(colpart), rows, 0, ctypes.byref(fused), stream=stream)
    return du, (colpart if fused.value else None)


def reduce_segments(segs, alpha=1.0, accumulate=False, stream=None):
    """segs: list of (part fp32 [P, stride] (a 2-D tensor or a column slice of one), out fp32 [N]) -> out = alpha * column sums
    (+ old when accumulating), all in ONE launch (vj_reduce_segments)."""
    arr = (VjReduceSeg * len(segs))()
    for i, (part, out) in enumerate(segs):
        _rows2d(part, F32, "reduce_segments: part")
        _dev(out, F32, "reduce_segments: out")
        arr[i] = VjReduceSeg(_addr(part, "part"), _addr(out, "out"), part.shape[0], out.numel(), part.stride(0))
    _launch("vj_reduce_segments", arr, len(segs), alpha, 1.0 if accumulate else 0.0, stream=stream)


# ---------------------------------------------------------------- predictor / loss
def _xattn_ws(B, NQ, N, H, hd, backward, device, stream):
    """Workspace of vj_xattn_{fwd,bwd}_ws from the caching allocator: (None, 0) while N fits the single-workgroup kernels."""
    nbytes = _query("vj_xattn_ws_bytes", B, NQ, N, H, hd, int(backward))
    if nbytes < 0:
        raise ValueError(f"xattn: unsupported dims B={B} NQ={NQ} N={N} H={H} head_dim={hd}")
    if nbytes == 0:
        return None, 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    if stream is not None:   # allocated on the current stream, used on another: keep it alive until that stream gets past it
        ws.record_stream(torch.cuda.ExternalStream(stream, device=device))
    return ws, nbytes


def xattn_fwd(q, kv, B, NQ, N, H, hd, scale, resid=None, shared_q=True, save_lse=True, stream=None):
    """Few-query cross-attention (vj_xattn_fwd_ws, any N): q [NQ, D] (shared_q) or [B, NQ, D], kv [B*N, 2*D] packed -> out [B*NQ, D]
    bf16, lse2 [B, H, NQ] fp32 (None when not saved)."""
    D = H * hd
    _req(q, torch.bfloat16, "q"); _req(kv, torch.bfloat16, "kv")
    out = torch.empty((B * NQ, D), dtype=torch.bfloat16, device=kv.device)
    lse = torch.empty((B, H, NQ), dtype=torch.float32, device=kv.device) if save_lse else None
    ws, nws = _xattn_ws(B, NQ, N, H, hd, False, kv.device, stream)
    _launch("vj_xattn_fwd_ws", _ptr(q), 0 if shared_q else NQ * D, _ptr(kv), _ptr(resid), _ptr(out), _ptr(lse), B, NQ, N, H, hd,
            float(scale), _ptr(ws), nws, stream=stream)
    return out, lse


def xattn_bwd(q, kv, dy, lse, B, N, H, hd, scale, shared_q=True, stream=None):
    """Backward of xattn_fwd for one query per sample (vj_xattn_bwd_ws, any N): returns dq [B, D] bf16 (per sample) and
    dkv [B*N, 2*D] bf16."""
    D = H * hd
    _req(q, torch.bfloat16, "q"); _req(kv, torch.bfloat16, "kv"); _req(dy, torch.bfloat16, "dy")
    dq = torch.empty((B, D), dtype=torch.bfloat16, device=kv.device)
    dkv = torch.empty_like(kv)
    ws, nws = _xattn_ws(B, 1, N, H, hd, True, kv.device, stream)
    _launch("vj_xattn_bwd_ws", _ptr(q), 0 if shared_q else D, _ptr(kv), _ptr(dy), _ptr(lse), _ptr(dq), _ptr(dkv), B, 1, N, H, hd,
            float(scale), _ptr(ws), nws, stream=stream)
    return dq, dkv


def pool_softmax_fwd(S, stream=None):
    """Soft-max down the key axis of S fp32 [B, N, C] (vj_pool_softmax_fwd) -> A bf16 [B, N, C], lse fp32 [B, C]."""
    _req(S, F32, "S")
    if S.dim() != 3:
        raise ValueError(f"pool_softmax_fwd: expected [B, N, C], got {tuple(S.shape)}")
    B, N, C = S.shape
    nws = _query("vj_pool_softmax_fwd_ws_bytes", B, N, C)
    if nws < 0:
        check(-1, "vj_pool_softmax_fwd_ws_bytes")
    A = torch.empty((B, N, C), dtype=BF16, device=S.device)
    lse = torch.empty((B, C), dtype=F32, device=S.device)
    ws = Scratch.get(nws, S.device, "pool_softmax", stream=stream)
    _launch("vj_pool_softmax_fwd", _ptr(S), _ptr(A), _ptr(lse), B, N, C, _ptr(ws), nws, stream=stream)
    return A, lse


def pool_softmax_bwd(A, dA, delta, stream=None):
    """dS bf16 [B, N, C] = A * (dA - delta[b, c]) (vj_pool_softmax_bwd); A bf16, dA fp32 [B, N, C], delta fp32 [B, C]."""
    _req(A, BF16, "A"); _req(dA, F32, "dA"); _req(delta, F32, "delta")
    if A.dim() != 3 or dA.shape != A.shape or tuple(delta.shape) != (A.shape[0], A.shape[2]):
        raise ValueError(f"pool_softmax_bwd: A {tuple(A.shape)} / dA {tuple(dA.shape)} / delta {tuple(delta.shape)} do not match")
    B, N, C = A.shape
    dS = torch.empty_like(A)
    _launch("vj_pool_softmax_bwd", _ptr(A), _ptr(dA), _ptr(delta), _ptr(dS), B, N, C, stream=stream)
    return dS


def pred_assemble(e, mask_token, pos, idx_e, idx_p, out=None, stream=None):
    _req(e, BF16, "e")
    B, Ke = idx_e.shape
    Kp = idx_p.shape[1]
    D = e.shape[-1]
    if out is None:
        out = torch.empty((B * (Ke + Kp), D), dtype=BF16, device=e.device)
    _launch("vj_pred_assemble_fwd", _ptr(e), _ptr(mask_token), _ptr(pos), _ptr(idx_e), _ptr(idx_p), _ptr(out), B, Ke, Kp, D,
            stream=stream)
    return out


def target_rows(x, gamma, beta, idx, B, N, eps_norm, eps_ln=1e-5, out=None, stream=None):
    _req(x, BF16, "x")
    idx = _req(idx, I64, "idx")
    K = idx.shape[1]
    D = x.shape[-1]
    h = torch.empty((B, K, D), dtype=F32, device=x.device) if out is None else out
    _launch("vj_target_rows", _ptr(x), _ptr(gamma), _ptr(beta), _ptr(idx), _ptr(h), B, N, K, D, eps_norm, eps_ln, stream=stream)
    return h


def latent_loss(z, h, loss_out, p=1.0, out_scale=1.0, accumulate=False, dz=None, gscale=0.0, stream=None):
    """loss_out[0] (+)= out_scale * sum(|z - h|^p / p); dz (optional bf16, z's shape) = sign(z - h) |z - h|^(p-1) * gscale."""
    _req(z, BF16, "z")
    _req(h, F32, "h")
    _req(loss_out, F32, "loss_out")
    _opt(dz, BF16, "dz")
    nws = _query("vj_latent_loss_ws_bytes")
    ws = Scratch.get(nws, z.device, "loss", stream=stream)
    _launch("vj_latent_loss", _ptr(z), _ptr(h), _ptr(dz), z.numel(), p, gscale, out_scale, int(accumulate), _ptr(loss_out), _ptr(ws), nws,
            stream=stream)
    return loss_out


def token_pstd(z, pstd, B, K, D, accumulate, stats=None, stream=None):
    """pstd[b,d] (fp32) (+)= sqrt(var_k z[b,k,d] + 1e-4) of bf16 z [B,K,D]; stats (optional fp32 [B,D,2]) = {mean, sqrt(var + eps)}."""
    _req(z, BF16, "z")
    _req(pstd, F32, "pstd")
    _opt(stats, F32, "stats")
    _launch("vj_token_pstd", _ptr(z), _ptr(pstd), _ptr(stats), B, K, D, int(accumulate), stream=stream)


def reg_grad(z, pstd_sum, stats, dz, B, K, D, n_masks, coef, stream=None):
    """Backward of the variance regulariser into bf16 dz, in place, from bf16 z and the fp32 pstd_sum / stats of token_pstd."""
    _req(z, BF16, "z")
    _req(pstd_sum, F32, "pstd_sum")
    _req(stats, F32, "stats")
    _req(dz, BF16, "dz")
    _launch("vj_reg_grad", _ptr(z), _ptr(pstd_sum), _ptr(stats), _ptr(dz), B, K, D, n_masks, coef, stream=stream)


def reg_finish(pstd, n_masks, out, stream=None):
    """out[0] = mean(relu(1 - pstd / n_masks)); pstd, out fp32."""
    _req(pstd, F32, "pstd")
    _req(out, F32, "out")
    _launch("vj_reg_finish", _ptr(pstd), pstd.numel(), n_masks, _ptr(out), stream=stream)


# ---------------------------------------------------------------- optimizer
def _adam_args(p, g, m, v, p_bf16, tgt, tgt_bf16):
    """The arena slices of both AdamW forms: fp32 p, g, exp_avg, exp_avg_sq; nullable bf16 shadow, fp32 EMA target and its shadow."""
    for t, name in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _req(t, F32, name)
    _opt(p_bf16, BF16, "p_bf16")
    _opt(tgt, F32, "tgt")
    _opt(tgt_bf16, BF16, "tgt_bf16")


def adamw_ema(p, g, m, v, p_bf16, tgt, tgt_bf16, lr, wd, beta1, beta2, eps, step, gscale, ema, stream=None):
    _adam_args(p, g, m, v, p_bf16, tgt, tgt_bf16)
    _launch("vj_adamw_ema", _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(p_bf16), _ptr(tgt), _ptr(tgt_bf16), p.numel(), lr, wd, beta1,
            beta2, eps, step, gscale, ema, stream=stream)


def step_advance(gstat, step_dev, stream=None):
    _req(gstat, F32, "gstat")
    _req(step_dev, F32, "step_dev")
    _launch("vj_step_advance", _ptr(gstat), _ptr(step_dev), stream=stream)


def adamw_ema_guarded(p, g, m, v, p_bf16, tgt, tgt_bf16, lr, wd, beta1, beta2, eps, gscale, ema, gstat, sel, clip,
                      norm_scale, step_dev, stream=None):
    """AdamW + EMA + bf16 re-casts with the skip-on-non-finite flag, the clip coefficient and the step count read on
    the device (include/vjepa_hip.h: vj_adamw_ema_guarded)."""
    _adam_args(p, g, m, v, p_bf16, tgt, tgt_bf16)
    _req(gstat, F32, "gstat")
    _req(step_dev, F32, "step_dev")
    _launch("vj_adamw_ema_guarded", _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(p_bf16), _ptr(tgt), _ptr(tgt_bf16), p.numel(), lr, wd,
            beta1, beta2, eps, gscale, ema, _ptr(gstat), sel, clip, norm_scale, _ptr(step_dev), stream=stream)


def grad_stats_multi(G, M1, M2, desc, n_tensors, stream=None):
    """One launch over the arenas -> fp32 [n_tensors, 3] = per-tensor {sum g^2, sum |exp_avg|, sum |exp_avg_sq|}
    (device tensor; reading it is the only host sync)."""
    _req(G, F32, "G")
    _opt(M1, F32, "M1")
    _opt(M2, F32, "M2")
    _req(desc, I64, "desc")
    nch = _query("vj_grad_stats_chunks")
    out = torch.empty((n_tensors, nch, 3), dtype=F32, device=G.device)
    _launch("vj_grad_stats_multi", _ptr(G), _ptr(M1), _ptr(M2), _ptr(desc), n_tensors, _ptr(out), stream=stream)
    return out.sum(dim=1)


def ema_update(tgt, src, tgt_bf16, m, stream=None):
    _req(tgt, F32, "tgt")
    _req(src, F32, "src")
    _opt(tgt_bf16, BF16, "tgt_bf16")
    _launch("vj_ema_update", _ptr(tgt), _ptr(src), _ptr(tgt_bf16), tgt.numel(), m, stream=stream)


def cast_bf16(src, dst, stream=None):
    _req(src, F32, "src")
    _req(dst, BF16, "dst")
    _launch("vj_cast_f32_to_bf16", _ptr(src), _ptr(dst), src.numel(), stream=stream)
    return dst


def sqnorm(g, out2, accumulate=False, stream=None):
    """out2[0] (+)= sum g^2, out2[1] (+)= count of non-finite values; g, out2 fp32."""
    _req(g, F32, "g")
    _req(out2, F32, "out2")
    nws = _query("vj_sqnorm_ws_bytes")
    ws = Scratch.get(nws, g.device, "sqnorm", stream=stream)
    _launch("vj_sqnorm_f32", _ptr(g), g.numel(), _ptr(out2), int(accumulate), _ptr(ws), nws, stream=stream)
    return out2
