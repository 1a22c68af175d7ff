"""Shared by test_randaug_host.py and test_randaug_gpu.py: the fixture of the reference's RandAugment
(tests/golden/randaug_micro.npz, tools/make_golden_randaug.py) and a numpy restatement of the arithmetic of vj_clip_randaug
(csrc/clip_randaug.hip): fp64 for the geometry, fp32 for blend and filter, every operation rounded on its own."""
import os
import random

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_fixture = None

F32 = np.float32


def fixture():
    global _fixture
    if _fixture is None:
        z = np.load(os.path.join(GOLDEN, "randaug_micro.npz"))
        _fixture = {k: z[k] for k in z.files}
    return _fixture


def names():
    return [str(n) for n in fixture()["names"]]


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


# ---------------------------------------------------------------- the arithmetic, per frame [H,W,3] uint8
def _blend(d, i, f):
    """ImageEnhance: d + f * (i - d) in fp32, each step rounded; truncated for 0 <= f <= 1, clipped and truncated otherwise."""
    f = F32(f)
    d = np.asarray(d).astype(F32)
    t = (d + (f * (np.asarray(i).astype(F32) - d)).astype(F32)).astype(F32)
    if not (F32(0) <= f <= F32(1)):
        t = np.where(t <= 0, F32(0), np.where(t >= 255, F32(255), t))
    return t.astype(np.int64).astype(np.uint8)


def luma(frame):
    r, g, b = (frame[..., c].astype(np.int64) for c in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16).astype(np.uint8)


def table(code, arg, frame):
    """[3,256] uint8 table of an operation that maps the bytes of a channel on their own."""
    i = np.arange(256, dtype=np.int64)
    if code == 3:
        one = 255 - i
    elif code == 5:
        one = i & ~(2 ** (8 - int(arg)) - 1)
    elif code == 6:
        one = np.where(i < int(arg), i, 255 - i)
    elif code == 7:
        one = np.where(i < 128, np.minimum(255, i + int(arg)), i)
    elif code == 10:
        one = _blend(np.zeros(256), i, arg)
    elif code == 9:
        lum = luma(frame).astype(np.int64)
        mean = int(float(int(lum.sum())) / float(lum.size) + 0.5)
        one = _blend(np.full(256, mean), i, arg)
    else:
        out = np.zeros((3, 256), dtype=np.uint8)
        for c in range(3):
            h = np.bincount(frame[..., c].reshape(-1), minlength=256).astype(np.int64)
            nz = np.nonzero(h)[0]
            lut = i.copy()
            if code == 1:
                lo, hi = int(nz[0]), int(nz[-1])
                if hi > lo:
                    scale = 255.0 / (hi - lo)
                    offset = -lo * scale
                    lut = np.clip((i.astype(np.float64) * scale + offset).astype(np.int64), 0, 255)
            else:
                step = (int(h.sum()) - int(h[nz[-1]])) // 255 if len(nz) > 1 else 0
                if step:
                    n = step // 2
                    for k in range(256):
                        lut[k] = min(255, n // step)
                        n += int(h[k])
            out[c] = lut
        return out
    return np.broadcast_to(one.astype(np.uint8), (3, 256))


def sharpen(frame, f):
    H, W, _ = frame.shape
    k = [F32(v) / F32(13) for v in (1, 1, 1, 1, 5, 1, 1, 1, 1)]
    x = frame.astype(F32)
    acc = np.full((H - 2, W - 2, 3), F32(0.5))
    for r in range(3):
        row = np.zeros_like(acc)
        for c in range(3):
            term = (x[r:H - 2 + r, c:W - 2 + c] * k[r * 3 + c]).astype(F32)
            row = term if c == 0 else (row + term).astype(F32)
        acc = (acc + row).astype(F32)
    smooth = frame.copy()
    smooth[1:-1, 1:-1] = np.clip(acc.astype(np.int64), 0, 255).astype(np.uint8)
    return _blend(smooth, frame, f)


def _cubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def affine(frame, a):
    H, W, _ = frame.shape
    out = np.full_like(frame, 128)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64) + 0.5, np.arange(W, dtype=np.float64) + 0.5, indexing="ij")
    xin = (a[0] * xs + a[1] * ys) + a[2]
    yin = (a[3] * xs + a[4] * ys) + a[5]
    inside = ~((xin < 0) | (xin >= W) | (yin < 0) | (yin >= H))
    xin, yin = xin - 0.5, yin - 0.5
    x0, y0 = np.floor(xin), np.floor(yin)
    dx, dy = xin - x0, yin - y0
    x0, y0 = x0.astype(np.int64) - 1, y0.astype(np.int64) - 1
    src = frame.astype(np.float64)
    cols = [np.clip(x0 + k, 0, W - 1) for k in range(4)]
    rows, prev = [], None
    for k in range(4):
        y = y0 + k
        ok = (y >= 0) & (y < H)
        yc = np.clip(y, 0, H - 1)
        v = _cubic(*(src[yc, cx] for cx in cols), dx[..., None])
        if k > 0:
            v = np.where(ok[..., None], v, prev)
        rows.append(v)
        prev = v
    v = _cubic(*rows, dy[..., None])
    px = np.where(v <= 0, 0, np.where(v >= 255, 255, np.floor(np.clip(v, 0, 255)))).astype(np.uint8)
    out[inside] = px[inside]
    return out


def apply_op(frame, code, args):
    code = int(code)
    if code == 0:
        return frame
    if code in (1, 2, 3, 5, 6, 7, 9, 10):
        lut = table(code, args[0], frame)
        return np.stack([lut[c][frame[..., c]] for c in range(3)], axis=-1)
    if code == 8:
        return _blend(luma(frame)[..., None], frame, args[0])
    if code == 11:
        return sharpen(frame, args[0])
    return affine(frame, [float(v) for v in args])


def restate(frames, ops, args):
    """uint8 [T,H,W,3] frames through the plan (ops [L], args [L,6]), layer after layer, frame by frame."""
    out = np.array(frames, copy=True)
    for code, a in zip(ops, args):
        out = np.stack([apply_op(f, code, a) for f in out])
    return out
