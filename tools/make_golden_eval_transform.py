#!/usr/bin/env python
"""Generate tests/golden/eval_transform_micro.npz from the reference's frozen-eval video transforms, on the CPU.

    JEPA_REFERENCE=/path/to/jepa python tools/make_golden_eval_transform.py

evals/video_classification_frozen/utils.py imports torchvision and the models, so make_transforms, VideoTransform,
EvalVideoTransform and tensor_normalize are taken out of it with `ast`, as tools/make_golden_transform.py does; so are Compose,
Resize, CenterCrop, Normalize and the crop / flip functions of src/datasets/utils/video/transforms.py, the helpers of
functional.py and ClipToTensor of volume_transforms.py.  Stubs: torchvision's ToPILImage is the identity and ToTensor is
uint8 [H,W,C] -> float32 [C,H,W] / 255 (what the pair does to a uint8 frame); PIL is a class nothing is an instance of; cv2 is never
reached, because every validation source already has the short side the reference's Resize asks for and resize_clip returns early;
create_random_augment is unused with auto_augment false.  src/datasets/utils/video/randerase.py is imported as it is.  One CPU
thread, so that a second run reproduces the file bit for bit.

Per case (T = 4): the seed given to `random`, `np.random` and `torch`, the uint8 frames, and
  train_*   the reference output fp32 [3,T,S,S] of VideoTransform(training=True), the per-frame boxes (i, j, h, w), the flip, the
            RandomErasing box (top, left, h, w; zeros: none) and its noise [T,3,h,w], and the next draw of each generator after the
            call.  Boxes and flip are read back as in make_golden_transform.py (the same spatial function under the same seed on a
            coordinate image while F.interpolate is watched); the erase box is read from the two `random.randint` calls and the
            shapes handed to randerase._get_pixels, whose return values are the noise.
  centre_*  the output [3,T,S,S] of VideoTransform(training=False) and the crop offsets (y1, x1).
  views_*   the outputs [V,3,T,S,S] of EvalVideoTransform and the view starts along the long side.
The script asserts what the cases must cover: odd source widths, output sides 16 and 32, with and without motion shift, with and
without flip, reprob 1.0 and 0.0, one and several views, portrait and landscape, and a centre-crop offset that Python rounds to even.
"""
import ast
import importlib.util
import math
import numbers
import os
import random
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("JEPA_REFERENCE", "")
OUT = os.path.join(ROOT, "tests", "golden", "eval_transform_micro.npz")

T = 4
FRAME_SEED = 911
# name, (H, W), output side, motion_shift, wanted flip (None: any), reprob
TRAIN_CASES = (
    ("train_flip_erase", (37, 53), 16, False, True, 1.0),
    ("train_noflip", (48, 40), 32, False, False, 0.0),
    ("train_shift_erase", (48, 40), 32, True, None, 1.0),
    ("train_shift", (37, 53), 16, True, None, 0.0),
)
# name, (H, W), output side: the short side is int(side * 256 / 224)
CENTRE_CASES = (
    ("centre_landscape", (18, 27), 16),     # (27 - 16) / 2 = 5.5 -> 6
    ("centre_portrait", (25, 18), 16),      # (25 - 16) / 2 = 4.5 -> 4: Python rounds to even
)
# name, (H, W), output side (= short side), views
VIEW_CASES = (
    ("views_landscape", (16, 37), 16, 3),
    ("views_portrait", (53, 16), 16, 3),
    ("views_side32", (32, 45), 32, 2),
)


def _reference_defs(rel_path, names, ns):
    src = open(os.path.join(REF, rel_path)).read()
    body = [n for n in ast.parse(src).body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert sorted(n.name for n in body) == sorted(names), (rel_path, names)
    exec(compile(ast.Module(body=body, type_ignores=[]), rel_path, "exec"), ns)
    return [ns[n] for n in names]


class _NoImage:
    """PIL.Image as the reference sees it here: nothing is an instance of Image.Image."""
    class Image:
        pass


class _RecordingRandom:
    """`random` as randerase.py sees it: the real module, with the results of randint() kept."""
    def __init__(self):
        self.randints = []

    def __getattr__(self, name):
        return getattr(random, name)

    def randint(self, a, b):
        v = random.randint(a, b)
        self.randints.append(v)
        return v


def frames_for(name, hw):
    g = torch.Generator().manual_seed(FRAME_SEED + sum(ord(c) for c in name))
    return torch.randint(0, 256, (T, hw[0], hw[1], 3), generator=g, dtype=torch.uint8).numpy()


def coord_image(hw):
    img = torch.zeros(3, T, hw[0], hw[1])
    img[0] = torch.arange(hw[0], dtype=torch.float32)[None, :, None]
    img[1] = torch.arange(hw[1], dtype=torch.float32)[None, None, :]
    return img


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def main():
    if not REF or not os.path.isfile(os.path.join(REF, "evals", "video_classification_frozen", "utils.py")):
        raise SystemExit("set JEPA_REFERENCE to the root of a facebookresearch/jepa checkout")
    torch.set_num_threads(1)
    pil = types.SimpleNamespace(Image=_NoImage)

    fns = dict(np=np, torch=torch, numbers=numbers, PIL=pil, cv2=None)
    fnames = ["_is_tensor_clip", "crop_clip", "resize_clip", "get_resize_sizes", "normalize"]
    _reference_defs("src/datasets/utils/video/functional.py", fnames, fns)
    FF = types.SimpleNamespace(**{n: fns[n] for n in fnames})

    vns = dict(torch=torch, np=np, math=math, random=random, numbers=numbers, PIL=pil, FF=FF)
    vnames = ["_get_param_spatial_crop", "random_resized_crop", "random_resized_crop_with_shift", "horizontal_flip", "Compose",
              "Resize", "CenterCrop", "Normalize"]
    _reference_defs("src/datasets/utils/video/transforms.py", vnames, vns)
    video_transforms = types.SimpleNamespace(create_random_augment=lambda **k: None, **{n: vns[n] for n in vnames})

    cns = dict(np=np, torch=torch, Image=_NoImage)
    _reference_defs("src/datasets/utils/video/volume_transforms.py", ["convert_img", "ClipToTensor"], cns)
    volume_transforms = types.SimpleNamespace(ClipToTensor=cns["ClipToTensor"])

    spec = importlib.util.spec_from_file_location("ref_randerase", os.path.join(REF, "src", "datasets", "utils", "video", "randerase.py"))
    randerase = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(randerase)

    tv = types.SimpleNamespace(ToPILImage=lambda: (lambda frame: frame),
                               ToTensor=lambda: (lambda img: torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1)
                                                 .contiguous().to(torch.float32).div(255)))
    ens = dict(np=np, torch=torch, transforms=tv, video_transforms=video_transforms, volume_transforms=volume_transforms,
               RandomErasing=randerase.RandomErasing, print=lambda *a, **k: None)
    make_transforms, _, _, _ = _reference_defs("evals/video_classification_frozen/utils.py",
                                               ["make_transforms", "VideoTransform", "EvalVideoTransform", "tensor_normalize"], ens)

    seen = []
    real_interpolate = torch.nn.functional.interpolate

    def watching_interpolate(x, *a, **k):
        seen.append((int(x[0, 0, 0, 0]), int(x[1, 0, 0, 0]), x.shape[-2], x.shape[-1]))
        return real_interpolate(x, *a, **k)

    def draws(hw, side, shift):
        """(boxes [T,4], flip) of the reference's spatial transform and flip on an hw source, from the current generator state."""
        fn = vns["random_resized_crop_with_shift"] if shift else vns["random_resized_crop"]
        del seen[:]
        torch.nn.functional.interpolate = watching_interpolate
        try:
            out = fn(images=coord_image(hw), target_height=side, target_width=side, scale=(0.3, 1.0), ratio=(3 / 4, 4 / 3))
        finally:
            torch.nn.functional.interpolate = real_interpolate
        flipped, _ = vns["horizontal_flip"](0.5, out)
        boxes = list(seen) if shift else list(seen) * T
        assert len(boxes) == T, (len(boxes), shift)
        return np.array(boxes, dtype=np.int32), flipped is not out

    out = {"T": np.array(T), "train_names": np.array([c[0] for c in TRAIN_CASES]),
           "centre_names": np.array([c[0] for c in CENTRE_CASES]), "views_names": np.array([c[0] for c in VIEW_CASES])}

    real_get_pixels = randerase._get_pixels
    for name, hw, side, shift, want_flip, reprob in TRAIN_CASES:
        frames = frames_for(name, hw)
        seed = 0
        while True:
            seed_all(seed)
            boxes, flip = draws(hw, side, shift)
            if want_flip is None or flip == want_flip:
                break
            seed += 1
        rec, shapes, noise = _RecordingRandom(), [], []

        def recording_get_pixels(per_pixel, rand_color, patch_size, **k):
            v = real_get_pixels(per_pixel, rand_color, patch_size, **k)
            shapes.append(tuple(patch_size))
            noise.append(v.clone())
            return v

        randerase.random, randerase._get_pixels = rec, recording_get_pixels
        try:
            seed_all(seed)
            tf = make_transforms(training=True, reprob=reprob, motion_shift=shift, crop_size=side)
            ref = tf(frames)
        finally:
            randerase.random, randerase._get_pixels = random, real_get_pixels
        nxt = np.array([random.random(), np.random.uniform(), float(torch.rand(1, dtype=torch.float64))], dtype=np.float64)
        assert isinstance(ref, list) and len(ref) == 1
        ref = ref[0]
        assert ref.shape == (3, T, side, side) and ref.dtype == torch.float32
        if noise:
            assert len(noise) == T and len(set(shapes)) == 1 and len(rec.randints) == 2
            ebox = np.array([rec.randints[0], rec.randints[1], shapes[0][1], shapes[0][2]], dtype=np.int32)
            nz = torch.stack(noise).numpy()
            t0, l0, eh, ew = (int(v) for v in ebox)
            assert np.array_equal(ref[:, :, t0:t0 + eh, l0:l0 + ew].permute(1, 0, 2, 3).numpy(), nz)    # the recorded box is where the noise went
        else:
            assert reprob == 0.0, (name, "100 erase boxes did not fit")
            ebox, nz = np.zeros(4, dtype=np.int32), np.zeros((T, 3, 0, 0), dtype=np.float32)
        out[f"{name}/seed"] = np.array(seed)
        out[f"{name}/frames"] = frames
        out[f"{name}/boxes"] = boxes
        out[f"{name}/flip"] = np.array(flip)
        out[f"{name}/shift"] = np.array(shift)
        out[f"{name}/side"] = np.array(side)
        out[f"{name}/reprob"] = np.array(reprob)
        out[f"{name}/ebox"] = ebox
        out[f"{name}/noise"] = nz
        out[f"{name}/next"] = nxt
        out[f"{name}/ref"] = ref.numpy().copy()
        print(f"{name}: seed {seed} source {hw} boxes {boxes[0].tolist()} .. {boxes[-1].tolist()} flip {flip} erase {ebox.tolist()}")

    for name, hw, side in CENTRE_CASES:
        frames = frames_for(name, hw)
        assert min(hw) == int(side * 256 / 224)
        ref = make_transforms(training=False, crop_size=side)(frames)
        assert isinstance(ref, list) and len(ref) == 1 and ref[0].shape == (3, T, side, side) and ref[0].dtype == torch.float32
        y1, x1 = int(round((hw[0] - side) / 2.)), int(round((hw[1] - side) / 2.))
        out[f"{name}/frames"] = frames
        out[f"{name}/side"] = np.array(side)
        out[f"{name}/offsets"] = np.array([y1, x1], dtype=np.int32)
        out[f"{name}/ref"] = ref[0].numpy().copy()
        print(f"{name}: source {hw} side {side} offsets {(y1, x1)}")

    for name, hw, side, views in VIEW_CASES:
        frames = frames_for(name, hw)
        assert min(hw) == side
        ref = make_transforms(training=False, crop_size=side, num_views_per_clip=views)(frames)
        assert isinstance(ref, list) and len(ref) == views and all(r.shape == (3, T, side, side) and r.dtype == torch.float32 for r in ref)
        step = (max(hw) - side) // (views - 1)
        out[f"{name}/frames"] = frames
        out[f"{name}/side"] = np.array(side)
        out[f"{name}/views"] = np.array(views)
        out[f"{name}/starts"] = np.array([i * step for i in range(views)], dtype=np.int32)
        out[f"{name}/ref"] = torch.stack(ref).numpy().copy()
        print(f"{name}: source {hw} side {side} view starts {out[f'{name}/starts'].tolist()}")

    # what the fixture must contain
    tc = {n: {k: out[f"{n}/{k}"] for k in ("frames", "boxes", "flip", "shift", "side", "reprob", "ebox")} for n in out["train_names"]}
    assert any(bool(v["flip"]) for v in tc.values()) and any(not bool(v["flip"]) for v in tc.values())
    assert any(bool(v["shift"]) and len({tuple(b) for b in v["boxes"].tolist()}) > 1 for v in tc.values())
    assert any(not bool(v["shift"]) for v in tc.values())
    assert {int(v["side"]) for v in tc.values()} == {16, 32}
    assert {float(v["reprob"]) for v in tc.values()} == {0.0, 1.0}
    assert all((int(v["ebox"][2]) > 0) == (float(v["reprob"]) == 1.0) for v in tc.values())
    assert any(v["frames"].shape[2] % 2 == 1 for v in tc.values())
    assert any(hw[0] > hw[1] for _, hw, _ in CENTRE_CASES) and any(hw[0] < hw[1] for _, hw, _ in CENTRE_CASES)
    assert any(hw[0] > hw[1] for _, hw, _, _ in VIEW_CASES) and any(hw[0] < hw[1] for _, hw, _, _ in VIEW_CASES)
    assert any(int(round((max(hw) - side) / 2.)) < (max(hw) - side) / 2. for _, hw, side in CENTRE_CASES)       # .5 rounded DOWN to even
    assert any(int(round((max(hw) - side) / 2.)) > (max(hw) - side) / 2. for _, hw, side in CENTRE_CASES)       # .5 rounded up to even
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size <= 1 << 20, size
    print(f"wrote {OUT}: {size} bytes")


if __name__ == "__main__":
    main()
