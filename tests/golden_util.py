"""Shared helpers for the parity tests: load the golden fixtures generated from the real reference
(oracle/make_golden.py, oracle/make_golden_reference.py) and build oracle / HIP-path states from them."""
import hashlib
import os
import random

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

MICRO = dict(embed_dim=64, depth=2, heads=2, pred_dim=32, pred_depth=2, num_mask_tokens=2, crop=64, frames=8,
             patch=16, tubelet=2, num_patches=4 * 4 * 4)
MICRO_MASKS = [
    dict(aspect_ratio=(0.75, 1.5), num_blocks=2, spatial_scale=(0.15, 0.15), temporal_scale=(1.0, 1.0),
         max_temporal_keep=1.0, max_keep=None),
    dict(aspect_ratio=(0.75, 1.5), num_blocks=1, spatial_scale=(0.5, 0.5), temporal_scale=(0.5, 1.0),
         max_temporal_keep=1.0, max_keep=None),
]
HP = dict(loss_exp=1.0, reg_coeff=0.0, ipe=10, ipe_scale=1.25, epochs=4, warmup=1, start_lr=2e-4, lr=6.25e-4,
          final_lr=1e-6, wd=0.04, final_wd=0.4, ema=(0.998, 1.0), betas=(0.9, 0.999), eps=1e-8)


def load_micro():
    return np.load(os.path.join(GOLDEN, "micro_step.npz"))


def load_tables():
    return np.load(os.path.join(GOLDEN, "host_tables.npz"))


def load_reference_api():
    """What the reference's own model factory, collators and checkpoint loaders produced (oracle/make_golden_reference.py)."""
    return np.load(os.path.join(GOLDEN, "reference_api.npz"))


def tensor_digest(*tensors):
    """sha256 over dtype, shape and raw bytes of each tensor: equal digests = bit-identical tensors."""
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().cpu().contiguous()
        h.update(f"{t.dtype}{tuple(t.shape)}".encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def tensor_fingerprint(t, n_samples=64):
    """float64 [numel, sum, sum of squares, n_samples values at evenly spaced flat indices (NaN-padded)]: pins a float
    tensor across hosts, whose CPU kernels may differ from the recording host's in the last bit."""
    x = t.detach().cpu().reshape(-1).double()
    fp = np.full(3 + n_samples, np.nan)
    fp[:3] = x.numel(), float(x.sum()), float((x * x).sum())
    if x.numel():
        idx = torch.linspace(0, x.numel() - 1, min(n_samples, x.numel())).long()
        fp[3:3 + len(idx)] = x[idx].numpy()
    return fp


def fingerprint_matches(fp, ref, rtol=1e-5):
    """Same tensor up to last-bit differences of the host's float kernels; a different draw, a different tensor or a
    misplaced one differs by its own scale."""
    n, s, ss = ref[:3]
    if fp[0] != n:
        return False
    rms = np.sqrt(ss / max(n, 1))
    a, b = fp[3:], ref[3:]
    return (np.isnan(a) == np.isnan(b)).all() and abs(fp[1] - s) <= rtol * np.sqrt(n * ss) + 1e-12 and \
        abs(fp[2] - ss) <= rtol * ss + 1e-12 and bool((np.abs(a - b)[~np.isnan(b)] <= rtol * (np.abs(b[~np.isnan(b)]) + rms) + 1e-12).all())


def collator_trials():
    """The random collator configurations of the live-reference comparison, drawn in a fixed order from Random(7):
    (multiblock trials [(kwargs, batch, [(seed, step_after), x3])], random-tube trials [(kwargs, seed)])."""
    rnd = random.Random(7)
    mb = []
    for _ in range(40):
        crop = rnd.choice([64, 128, 224, 384])
        frames = rnd.choice([8, 16])
        n_masks = rnd.choice([1, 2, 3])
        cfgs = []
        for _ in range(n_masks):
            lo = rnd.choice([0.15, 0.2, 0.5, 0.7])
            cfgs.append(dict(aspect_ratio=rnd.choice([(0.75, 1.5), (0.3, 3.0)]), num_blocks=rnd.choice([1, 2, 4, 8]),
                             spatial_scale=(lo, rnd.choice([lo, min(0.9, lo + 0.2)])),
                             temporal_scale=rnd.choice([(1.0, 1.0), (0.5, 1.0), (0.25, 0.75)]),
                             max_temporal_keep=rnd.choice([1.0, 0.5]), max_keep=rnd.choice([None, None, 64])))
        kw = dict(cfgs_mask=cfgs, crop_size=crop, num_frames=frames, patch_size=16, tubelet_size=2)
        B = rnd.choice([1, 2, 5, 24])
        its = []
        for _ in range(3):
            seed = rnd.randrange(1 << 30)
            its.append((seed, rnd.random() < 0.3))   # step_after: the resume path replays the counter (train.py:322-326)
        mb.append((kw, B, its))
    tube = []
    for _ in range(10):
        ratio = rnd.choice([0.5, 0.75, 0.9])
        kw = dict(cfgs_mask=[dict(ratio=ratio)], crop_size=224, num_frames=16, patch_size=16, tubelet_size=2)
        tube.append((kw, rnd.randrange(1 << 30)))
    return mb, tube


def collator_digests(multiblock_cls, tube_cls):
    """Run collator_trials() through the given MaskCollator classes: one tensor_digest per draw, in draw order."""
    mb, tube = collator_trials()
    mb_dig, tube_dig = [], []
    for kw, B, its in mb:
        coll = multiblock_cls(**kw)
        for seed, step_after in its:
            torch.manual_seed(seed)
            _, me, mp = coll([(torch.zeros(1), 0) for _ in range(B)])
            mb_dig.append(tensor_digest(*me, *mp))
            if step_after:
                coll.step()
    for kw, seed in tube:
        coll = tube_cls(**kw)
        torch.manual_seed(seed)
        np.random.seed(seed % (1 << 31))
        _, me, mp = coll([(torch.zeros(1), 0) for _ in range(4)])
        tube_dig.append(tensor_digest(*me, *mp))
    return mb_dig, tube_dig


def micro_weights(z):
    enc = {k[len("w0/enc/"):]: torch.from_numpy(z[k]).clone() for k in z.files if k.startswith("w0/enc/")}
    pred = {k[len("w0/pred/"):]: torch.from_numpy(z[k]).clone() for k in z.files if k.startswith("w0/pred/")}
    return enc, pred


def step_inputs(z, s, n_masks=2):
    clips = torch.from_numpy(z[f"s{s}/clips"])
    me = [torch.from_numpy(z[f"s{s}/masks_enc{i}"]) for i in range(n_masks)]
    mp = [torch.from_numpy(z[f"s{s}/masks_pred{i}"]) for i in range(n_masks)]
    return clips, me, mp


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / (b.norm() + 1e-300))
