"""Inputs of tests/golden/image_eval_micro.npz, regenerated from the recorded seeds on the CPU (imported, never collected).  The
layout and order are those of tools/make_golden_image_eval.py; the fixture's sha256 values pin them."""
import hashlib

import numpy as np
import torch


def _check(sha256, *tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().numpy().tobytes())
    assert np.array_equal(np.frombuffer(h.digest(), dtype=np.uint8), np.asarray(sha256)), "image_eval_micro inputs do not regenerate"


def micro_images(z):
    """(train [iters, B, 3, H, W], train labels [iters, B], val [B, 3, H, W], val labels [B])."""
    B, C, iters, T, crop = (int(x) for x in z["dims"])
    g = torch.Generator().manual_seed(int(z["image_seed"]))
    train = torch.randn(iters, B, 3, crop, crop, generator=g)
    train_labels = torch.randint(0, C, (iters, B), generator=g)
    val = torch.randn(B, 3, crop, crop, generator=g)
    val_labels = torch.randint(0, C, (B,), generator=g)
    _check(z["images_sha256"], train, train_labels, val, val_labels)
    return train, train_labels, val, val_labels


def off_native_clips(z, size, keep=40):
    """(clips [B, 3, T, H, W], mask [B, keep] sorted int64 token indices) of the off-native size `size` = (T, H, W)."""
    B = int(z["dims"][0])
    t, h, w = size
    g = torch.Generator().manual_seed(int(z["off_seed"]) + t * 1_000_000 + h * 1_000 + w)
    clips = torch.randn(B, 3, t, h, w, generator=g)
    n = (t // 2) * (h // 16) * (w // 16)
    mask = torch.stack([torch.randperm(n, generator=g)[:min(keep, n)].sort().values for _ in range(B)])
    _check(z[f"off_sha256/{t}x{h}x{w}"], clips, mask)
    return clips, mask
