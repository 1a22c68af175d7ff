"""Clips of tests/golden/eval_micro.npz, regenerated from the recorded seed on the CPU (imported, never collected).  The layout and
order are those of tools/make_golden_eval.py; the fixture's sha256 pins them."""
import hashlib

import numpy as np
import torch


def micro_clips(seed, S, V, B, C, iters, T, crop, sha256=None):
    """(train [iters, S, 1, B, 3, T, H, W], train labels [iters, B], val [S, V, B, 3, T, H, W], val labels [B]) -- checked against
    the recorded sha256 when one is given."""
    g = torch.Generator().manual_seed(seed)
    train = torch.randn(iters, S, 1, B, 3, T, crop, crop, generator=g)
    train_labels = torch.randint(0, C, (iters, B), generator=g)
    val = torch.randn(S, V, B, 3, T, crop, crop, generator=g)
    val_labels = torch.randint(0, C, (B,), generator=g)
    if sha256 is not None:
        h = hashlib.sha256()
        for t in (train, train_labels, val, val_labels):
            h.update(t.contiguous().numpy().tobytes())
        assert np.array_equal(np.frombuffer(h.digest(), dtype=np.uint8), np.asarray(sha256)), "eval_micro clips do not regenerate"
    return train, train_labels, val, val_labels
