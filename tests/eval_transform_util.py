"""Shared by test_eval_transform_host.py and test_eval_transform_gpu.py: the fixture of the reference's frozen-eval transforms
(tests/golden/eval_transform_micro.npz, tools/make_golden_eval_transform.py), the RawClip of each of its cases, and a float32 numpy
restatement of the arithmetic of vj_clip_transform_pre + vj_clip_erase."""
import os
import random

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NORMALIZE = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
# The bound on |device - reference| of the normalise-first transform: outputs stay below 2.65 in magnitude ((1 - 0.406) / 0.225 = 2.64),
# so one fp32 rounding is at most half an ulp of [2, 4): 2^-23 = 1.2e-7; about six roundings separate two orderings of the blend
# (w0x*p00 + w1x*p01, the same below, the row blend; fused or not): 7e-7, and 2e-6 leaves room for the weights' own rounding.
# A source coordinate computed unfused moves a result by more than 1e-4, fifty times the bound.
BOUND = 2e-6

_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        z = np.load(os.path.join(GOLDEN, "eval_transform_micro.npz"))
        _fixture = {k: z[k] for k in z.files}
    return _fixture


def names(kind):
    return [str(n) for n in fixture()[f"{kind}_names"]]


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def train_clip(name):
    """The RawClip that the eval's training transform draws for a train_* case from the case's seed."""
    from jepa_amd.evals.video_classification_frozen.utils import make_transforms
    z = fixture()
    seed_all(int(z[f"{name}/seed"]))
    tf = make_transforms(training=True, reprob=float(z[f"{name}/reprob"]), motion_shift=bool(z[f"{name}/shift"]),
                         crop_size=int(z[f"{name}/side"]))
    return tf(z[f"{name}/frames"])


def centre_clip(name):
    from jepa_amd.evals.video_classification_frozen.utils import make_transforms
    z = fixture()
    return make_transforms(training=False, crop_size=int(z[f"{name}/side"]))(z[f"{name}/frames"])


def views_clip(name):
    from jepa_amd.evals.video_classification_frozen.utils import make_transforms
    z = fixture()
    return make_transforms(training=False, crop_size=int(z[f"{name}/side"]), num_views_per_clip=int(z[f"{name}/views"]))(z[f"{name}/frames"])


def all_cases():
    """(name, RawClip, reference fp32 [V,3,T,S,S]) of every fixture case."""
    z = fixture()
    out = [(n, train_clip(n), z[f"{n}/ref"][None]) for n in names("train")]
    out += [(n, centre_clip(n), z[f"{n}/ref"][None]) for n in names("centre")]
    out += [(n, views_clip(n), z[f"{n}/ref"]) for n in names("views")]
    return out


def normalised_plain(frames, mean, std):
    """CPU torch (u / 255 - m) / s of uint8 [T,H,W,3] frames -> fp32 [3,T,H,W]: three separately rounded fp32 operations."""
    x = torch.as_tensor(frames).permute(3, 0, 1, 2).to(torch.float32) / 255.0
    m = torch.tensor(mean, dtype=torch.float32).view(3, 1, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(3, 1, 1, 1)
    return (x - m) / s


def _axis(n_out, length, org, lim):
    """ClipAxis of csrc/input_pack.hip for every destination index of one axis, in float32: fused source coordinate, taps, weights."""
    scale = np.float32(length) / np.float32(n_out)
    dst = np.arange(n_out, dtype=np.float64)
    c = np.maximum((np.float64(scale) * (dst + 0.5) - 0.5).astype(np.float32), np.float32(0))   # exact in float64, rounded once: the fma
    i0 = np.minimum(c.astype(np.int64), length - 1)
    i1 = np.minimum(i0 + 1, length - 1)
    lam = np.clip(c - i0.astype(np.float32), np.float32(0), np.float32(1)).astype(np.float32)
    return (np.clip(org + i0, 0, lim - 1), np.clip(org + i1, 0, lim - 1), (np.float32(1) - lam).astype(np.float32), lam)


def restate(clip):
    """float32 numpy restatement of vj_clip_transform_pre followed by vj_clip_erase on one RawClip -> [V,3,T,S,S]."""
    frames = np.asarray(clip.frames)
    T, H, W, _ = frames.shape
    S = clip.crop_size
    mean, std = np.array(clip.mean, dtype=np.float32), np.array(clip.std, dtype=np.float32)
    lut = ((np.arange(256, dtype=np.float32)[None, :] / np.float32(255) - mean[:, None]) / std[:, None]).astype(np.float32)   # [3,256]
    boxes = clip.boxes.numpy().reshape(-1, T, 4)
    out = np.zeros((boxes.shape[0], 3, T, S, S), dtype=np.float32)
    for v in range(boxes.shape[0]):
        for t in range(T):
            i, j, h, w = (int(x) for x in boxes[v, t])
            y0, y1, wy0, wy1 = _axis(S, h, i, H)
            x0, x1, wx0, wx1 = _axis(S, w, j, W)
            if clip.flip:
                x0, x1, wx0, wx1 = x0[::-1], x1[::-1], wx0[::-1], wx1[::-1]
            for c in range(3):
                n = lut[c][frames[t, :, :, c]]
                top = wx0[None, :] * n[y0][:, x0] + wx1[None, :] * n[y0][:, x1]
                bot = wx0[None, :] * n[y1][:, x0] + wx1[None, :] * n[y1][:, x1]
                out[v, c, t] = wy0[:, None] * top + wy1[:, None] * bot
        assert out.dtype == np.float32
    top, left, eh, ew = clip.ebox
    if eh > 0 and clip.noise is not None:
        out[0, :, :, top:top + eh, left:left + ew] = clip.noise.numpy().transpose(1, 0, 2, 3)
    return out
