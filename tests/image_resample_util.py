"""The numpy oracle of vj_image_resample: PIL's antialiased two-pass resample of 8-bit RGB, restated from its specification (fp64
coefficients truncated to 22-bit integers, horizontal pass first, uint8 intermediate), and the reference chain behind it (ToTensor,
Normalize, flip, RandomErasing) in fp32 torch operations.  Shared by tests/test_image_resample_host.py (oracle against the fixture
and against PIL), tests/test_image_resample_gpu.py and tools/make_golden_image_resample.py."""
import os

import numpy as np
import torch

BILINEAR, BICUBIC = 0, 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_resample_micro.npz")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _filter(u, filt):
    u = abs(u)
    if filt == BICUBIC:
        a = -0.5
        if u < 1.0:
            return ((a + 2.0) * u - (a + 3.0)) * u * u + 1.0
        if u < 2.0:
            return (((u - 5.0) * u + 8.0) * u - 4.0) * a
        return 0.0
    return 1.0 - u if u < 1.0 else 0.0


def coefficients(n, m, filt, first=0, count=None):
    """[(lo, int32 coefficients)] of output indices first .. first + count - 1 of an axis resampled from n to m pixels."""
    scale = n / m
    fs = max(scale, 1.0)
    support = (2.0 if filt == BICUBIC else 1.0) * fs
    out = []
    for x in range(first, first + (m - first if count is None else count)):
        center = (x + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n)
        w = [_filter((t - center + 0.5) / fs, filt) for t in range(lo, hi)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        out.append((lo, np.array([int(-0.5 + v * 4194304.0) if v < 0 else int(0.5 + v * 4194304.0) for v in w], dtype=np.int64)))
    return out


def _pass(src, table):
    """One pass along axis 1 of src uint8 [R, n, C] -> uint8 [R, len(table), C]."""
    out = np.empty((src.shape[0], len(table), src.shape[2]), dtype=np.uint8)
    s = src.astype(np.int64)
    for x, (lo, k) in enumerate(table):
        acc = (1 << 21) + (s[:, lo:lo + len(k), :] * k[None, :, None]).sum(1)
        acc = ((acc + (1 << 31)) % (1 << 32)) - (1 << 31)          # the int32 accumulator
        out[:, x, :] = np.clip(acc >> 22, 0, 255)
    return out


def resample_window(image, geom, S, filt):
    """image uint8 [H,W,3], geom = (i, j, h, w, OH, OW, wy, wx) -> uint8 [S,S,3]: the S x S window at (wy, wx) of the crop box
    resampled to OH x OW.  Only the window and the source rows it needs are computed; the bytes are those of the whole resize."""
    i, j, h, w, OH, OW, wy, wx = (int(v) for v in geom)
    crop = np.ascontiguousarray(image[i:i + h, j:j + w])
    ty = coefficients(h, OH, filt, wy, S)
    row0 = ty[0][0]
    rows = ty[-1][0] + len(ty[-1][1]) - row0
    tmp = _pass(crop[row0:row0 + rows], coefficients(w, OW, filt, wx, S))                   # horizontal first
    out = _pass(tmp.transpose(1, 0, 2), [(lo - row0, k) for lo, k in ty])                    # vertical on its uint8 result
    return np.ascontiguousarray(out.transpose(1, 0, 2))


def resample(image, OH, OW, filt):
    """The whole resize of image to OH x OW (for comparison with Image.resize)."""
    H, W = image.shape[:2]
    tmp = _pass(image, coefficients(W, OW, filt))
    return np.ascontiguousarray(_pass(tmp.transpose(1, 0, 2), coefficients(H, OH, filt)).transpose(1, 0, 2))


def reference_chain(window, flip, ebox=(0, 0, 0, 0), noise=None, mean=MEAN, std=STD):
    """What the reference's transforms make of the resampled uint8 [S,S,3] window: horizontal flip, ToTensor (/ 255), Normalize
    ((x - mean) / std on fp32 tensors), RandomErasing in pixel mode (the box is overwritten with the drawn noise) -> fp32 [3,S,S]."""
    u = torch.from_numpy(np.ascontiguousarray(window[:, ::-1] if flip else window))
    x = u.permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    m = torch.tensor(mean, dtype=torch.float32)[:, None, None]
    s = torch.tensor(std, dtype=torch.float32)[:, None, None]
    x = x.sub(m).div(s)
    top, left, eh, ew = (int(v) for v in ebox)
    if eh > 0 and noise is not None:
        x[:, top:top + eh, left:left + ew] = torch.as_tensor(noise, dtype=torch.float32).reshape(3, eh, ew)
    return x


def pack(images, align=16):
    """(flat uint8 buffer, byte offsets) of images laid out one after the other on 16-byte boundaries; the padding is 0xA5 so that a
    kernel that writes into it is seen."""
    offs, total = [], 0
    for im in images:
        offs.append(total)
        total += -(-im.size // align) * align
    flat = np.full(total, 0xA5, dtype=np.uint8)
    for im, off in zip(images, offs):
        flat[off:off + im.size] = im.reshape(-1)
    return flat, offs


def load_cases(z):
    """The fixture's cases: [(name, image uint8 [H,W,3], geom int32 [8], S, filter, expected uint8 [S,S,3])]."""
    cases = []
    for n in range(int(z["num_cases"])):
        cases.append((str(z["names"][n]), z[f"src_{int(z['src_index'][n])}"], z["geom"][n], int(z["S"][n]), int(z["filter"][n]),
                      z[f"want_{n}"]))
    return cases
