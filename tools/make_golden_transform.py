#!/usr/bin/env python
"""Generate tests/golden/transform_micro.npz from the reference's clip augmentation, on the CPU.

    JEPA_REFERENCE=/path/to/jepa python tools/make_golden_transform.py

app/vjepa/transforms.py imports torchvision, so VideoTransform and _tensor_normalize_inplace are taken out of it with `ast`, and
_get_param_spatial_crop, random_resized_crop, random_resized_crop_with_shift and horizontal_flip out of
src/datasets/utils/video/transforms.py, with stubs for create_random_augment and RandomErasing (both unused with
auto_augment false and reprob 0).  One CPU thread, so that a second run reproduces the file bit for bit.

Per case (T = 4; output side 32, one case at 64): the seed given to `random` and `np.random`, the uint8 frames, the reference
output fp32 [3,T,S,S] of VideoTransform.__call__, the per-frame boxes (i, j, h, w) and the flip.  The reference does not return
its boxes: they are read back by running the same spatial function under the same seed on a COORDINATE image (channel 0 = row
index, channel 1 = column index) while F.interpolate is watched -- the crop handed to it carries (i, j) in its first pixel and
(h, w) in its shape; the flip is whether horizontal_flip returned a new tensor.  Both runs must leave `random` and `np.random`
in the same state.  The cases cover, and the script asserts that they cover: a flipped and an unflipped clip, a motion-shift
clip, a source smaller than the output side, a non-square source, and a source whose ten draws all fail (central-crop fallback).

Also a sequence of 240 consecutive draws from one seeding over a list of source sizes (motion shift on every third), with the
next draw of each generator after it.
"""
import ast
import math
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("JEPA_REFERENCE", "")
OUT = os.path.join(ROOT, "tests", "golden", "transform_micro.npz")

T = 4
FRAME_SEED = 77
# name, (H, W), output side, motion_shift, wanted flip (None: any), wants the fallback
CASES = (
    ("flipped", (48, 64), 32, False, True, False),
    ("unflipped", (48, 64), 32, False, False, False),
    ("shift", (40, 56), 32, True, None, False),
    ("upsampled", (20, 24), 32, False, None, False),
    ("fallback", (25, 100), 32, False, None, True),
    ("side64", (72, 96), 64, True, None, False),
)
SEQ_SIZES = ((100, 400), (240, 320), (256, 340), (720, 1280), (20, 24), (400, 100), (360, 360))
SEQ_LEN, SEQ_SEED = 240, 4242


def _reference_defs(rel_path, names, ns):
    src = open(os.path.join(REF, rel_path)).read()
    body = [n for n in ast.parse(src).body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert sorted(n.name for n in body) == sorted(names), (rel_path, names)
    exec(compile(ast.Module(body=body, type_ignores=[]), rel_path, "exec"), ns)
    return [ns[n] for n in names]


class _CountingRandom:
    """np.random as the reference sees it: the real generator, with the calls to uniform() counted (ten per failed box)."""
    calls = 0

    @staticmethod
    def uniform(*a, **k):
        _CountingRandom.calls += 1
        return np.random.uniform(*a, **k)


class _NP:
    random = _CountingRandom


def frames_for(name, hw):
    g = torch.Generator().manual_seed(FRAME_SEED + sum(ord(c) for c in name))
    return torch.randint(0, 256, (T, hw[0], hw[1], 3), generator=g, dtype=torch.uint8).numpy()


_coord_cache = {}


def coord_image(hw):
    if hw not in _coord_cache:
        img = torch.zeros(3, T, hw[0], hw[1])
        img[0] = torch.arange(hw[0], dtype=torch.float32)[None, :, None]
        img[1] = torch.arange(hw[1], dtype=torch.float32)[None, None, :]
        _coord_cache.clear()
        _coord_cache[hw] = img
    return _coord_cache[hw]


def main():
    if not REF or not os.path.isfile(os.path.join(REF, "app", "vjepa", "transforms.py")):
        raise SystemExit("set JEPA_REFERENCE to the root of a facebookresearch/jepa checkout")
    torch.set_num_threads(1)
    import types
    vns = dict(torch=torch, np=_NP, math=math, random=random)
    names = ["_get_param_spatial_crop", "random_resized_crop", "random_resized_crop_with_shift", "horizontal_flip"]
    _reference_defs("src/datasets/utils/video/transforms.py", names, vns)
    video_transforms = types.SimpleNamespace(create_random_augment=lambda **k: None, **{n: vns[n] for n in names})
    tns = dict(torch=torch, video_transforms=video_transforms, RandomErasing=lambda *a, **k: None, transforms=None)
    VideoTransform, _ = _reference_defs("app/vjepa/transforms.py", ["VideoTransform", "_tensor_normalize_inplace"], tns)

    seen = []
    real_interpolate = torch.nn.functional.interpolate

    def watching_interpolate(x, *a, **k):
        seen.append((int(x[0, 0, 0, 0]), int(x[1, 0, 0, 0]), x.shape[-2], x.shape[-1]))
        return real_interpolate(x, *a, **k)

    def draws(hw, side, shift):
        """(boxes [T,4], flip, np.random.uniform calls) of one reference transform on an hw source, from the current state."""
        fn = vns["random_resized_crop_with_shift"] if shift else vns["random_resized_crop"]
        del seen[:]
        _CountingRandom.calls = 0
        torch.nn.functional.interpolate = watching_interpolate
        try:
            out = fn(images=coord_image(hw), target_height=side, target_width=side, scale=(0.3, 1.0), ratio=(3 / 4, 4 / 3))
        finally:
            torch.nn.functional.interpolate = real_interpolate
        flipped, _ = vns["horizontal_flip"](0.5, out)
        boxes = list(seen) if shift else list(seen) * T
        assert len(boxes) == T, (len(boxes), shift)
        return np.array(boxes, dtype=np.int32), flipped is not out, _CountingRandom.calls

    out = {"T": np.array(T), "case_names": np.array([c[0] for c in CASES])}
    for name, hw, side, shift, want_flip, want_fallback in CASES:
        frames = frames_for(name, hw)
        seed = 0
        while True:
            random.seed(seed)
            np.random.seed(seed)
            boxes, flip, calls = draws(hw, side, shift)
            fallback = calls - 1 == 10 * (2 if shift else 1)
            if (want_flip is None or flip == want_flip) and fallback == want_fallback:
                break
            seed += 1
        state = (random.random(), np.random.uniform())
        random.seed(seed)
        np.random.seed(seed)
        ref = VideoTransform(motion_shift=shift, crop_size=side)(frames)
        assert state == (random.random(), np.random.uniform()), name     # the coordinate run drew what the real run drew
        assert ref.shape == (3, T, side, side) and ref.dtype == torch.float32
        out[f"{name}/seed"] = np.array(seed)
        out[f"{name}/frames"] = frames
        out[f"{name}/boxes"] = boxes
        out[f"{name}/flip"] = np.array(flip)
        out[f"{name}/shift"] = np.array(shift)
        out[f"{name}/side"] = np.array(side)
        out[f"{name}/fallback"] = np.array(fallback)
        out[f"{name}/ref"] = ref.numpy().copy()
        print(f"{name}: seed {seed} source {hw} boxes {boxes[0].tolist()} .. {boxes[-1].tolist()} flip {flip} fallback {fallback}")

    # what the fixture must contain
    c = {n: {k: out[f"{n}/{k}"] for k in ("frames", "boxes", "flip", "shift", "side", "fallback")} for n in out["case_names"]}
    assert any(bool(v["flip"]) for v in c.values()) and any(not bool(v["flip"]) for v in c.values())
    assert any(bool(v["shift"]) and len({tuple(b) for b in v["boxes"].tolist()}) > 1 for v in c.values())
    assert any(max(v["frames"].shape[1:3]) < int(v["side"]) for v in c.values())
    assert any(v["frames"].shape[1] != v["frames"].shape[2] for v in c.values())
    fb = c["fallback"]
    assert bool(fb["fallback"]) and fb["boxes"][0].tolist() == [0, (100 - 33) // 2, 25, 33]
    assert any(int(v["side"]) == 64 for v in c.values())

    # one long draw sequence
    random.seed(SEQ_SEED)
    np.random.seed(SEQ_SEED)
    seq_boxes, seq_flip, seq_hw, seq_shift, n_fallback = [], [], [], [], 0
    for k in range(SEQ_LEN):
        hw, shift = SEQ_SIZES[k % len(SEQ_SIZES)], k % 3 == 2
        boxes, flip, calls = draws(hw, 32, shift)
        n_fallback += calls - 1 >= 10 and not shift
        seq_boxes.append(boxes)
        seq_flip.append(flip)
        seq_hw.append(hw)
        seq_shift.append(shift)
    assert n_fallback > 0
    out["seq/seed"] = np.array(SEQ_SEED)
    out["seq/hw"] = np.array(seq_hw, dtype=np.int32)
    out["seq/shift"] = np.array(seq_shift)
    out["seq/boxes"] = np.stack(seq_boxes)
    out["seq/flip"] = np.array(seq_flip)
    out["seq/next"] = np.array([random.random(), np.random.uniform()], dtype=np.float64)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size <= 1 << 20, size
    print(f"wrote {OUT}: {size} bytes; {SEQ_LEN} sequence draws, {n_fallback} of them central-crop fallbacks")


if __name__ == "__main__":
    main()
