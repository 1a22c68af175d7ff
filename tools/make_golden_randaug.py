#!/usr/bin/env python
"""Generate tests/golden/randaug_micro.npz from the reference's RandAugment and its frozen-eval training transform, on the CPU.

    JEPA_REFERENCE=/path/to/jepa python tools/make_golden_randaug.py          (needs PIL)

src/datasets/utils/video/randaugment.py is imported as it is (as randerase.py is).  create_random_augment and _pil_interp are taken
out of src/datasets/utils/video/transforms.py with `ast`, and VideoTransform / tensor_normalize out of
evals/video_classification_frozen/utils.py, as tools/make_golden_eval_transform.py does; the crop / flip functions come the same
way.  Stubs: transforms.Compose is a plain call chain, ToPILImage is Image.fromarray, ToTensor is uint8 [H,W,C] -> float32
[C,H,W] / 255.  One CPU thread, so that a second run reproduces the file bit for bit.

The file holds outputs only.  Per case: the seed given to `random`, `np.random` and `torch`, the config string, the uint8 frames
[T,H,W,3], and
  ops / args  the plan: operation code per layer (0: not applied) and its six arguments.  Recorded by wrapping the entries of
              NAME_TO_OP (which operation ran in which layer, with which level argument) and Image.transform (the six coefficients
              PIL itself computed for the affine family; a rotation by 0 never gets there and is code 0)
  aug         the augmented uint8 frames
  next        the next draw of `random`, `np.random` and `torch` after the call
and for the train_* cases (the eval's VideoTransform(training=True, auto_augment=True, reprob=...)) also the final fp32
[3,T,S,S], the boxes, the flip, the erase box and its noise, read as make_golden_eval_transform.py reads them.

Candidates are enumerated in a fixed order (seed, source size, frame kind, config) and picked greedily until everything the
fixture must cover is covered; the script asserts that list at the end.
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
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("JEPA_REFERENCE", "")
OUT = os.path.join(ROOT, "tests", "golden", "randaug_micro.npz")

EVAL_CONFIG = "rand-m7-n4-mstd0.5-inc1"
CONFIGS = (EVAL_CONFIG, "rand-m10-n4-mstd0.5-inc1", "rand-m2-n4-mstd1", "rand-m9-n8-mstd2-inc0")
SIZES = ((16, 21), (19, 16), (23, 30), (37, 53), (27, 17), (20, 20))      # Hs*Ws*3 % 16 != 0 for all but the last
KINDS = ("random", "narrow", "constant", "smooth")
AFFINE = ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
ENHANCE = ("Color", "Contrast", "Brightness", "Sharpness")
FRAME_SEED = 4242
MAX_CASES = 40
# name, (H, W), output side, reprob, frame kind
TRAIN_CASES = (("train_erase", (37, 53), 16, 1.0, "random"), ("train_plain", (30, 23), 16, 0.0, "smooth"),
               ("train_narrow", (24, 31), 16, 1.0, "narrow"))


def _reference_defs(rel_path, names, ns):
    src = open(os.path.join(REF, rel_path)).read()
    body = [n for n in ast.parse(src).body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert sorted(n.name for n in body) == sorted(names), (rel_path, names)
    exec(compile(ast.Module(body=body, type_ignores=[]), rel_path, "exec"), ns)
    return [ns[n] for n in names]


def _import(name, *rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, *rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def next_draws():
    return np.array([random.random(), np.random.uniform(), float(torch.rand(1, dtype=torch.float64))], dtype=np.float64)


def frames_for(tag, hw, T, kind):
    g = np.random.RandomState(FRAME_SEED + sum(ord(c) for c in tag))
    H, W = hw
    if kind == "narrow":
        return g.randint(90, 140, (T, H, W, 3)).astype(np.uint8)
    f = g.randint(0, 256, (T, H, W, 3)).astype(np.uint8)
    if kind == "constant":
        f[..., 1] = 77
    elif kind == "smooth":
        yy, xx = np.mgrid[0:H, 0:W]
        for t in range(T):
            f[t] = np.stack([(xx * 5 + yy * 3 + 40 * t) % 256, (xx * yy + 7 * t) % 256, (255 - xx * 4 + yy) % 256], -1)
    return f


class _Chain:
    """transforms.Compose as the reference uses it here: a plain call chain."""
    def __init__(self, fns):
        self.fns = fns

    def __call__(self, x):
        for fn in self.fns:
            x = fn(x)
        return x


class Recorder:
    """Wraps the reference module so that every operation that runs leaves (layer, name, level argument, affine coefficients,
    input, output)."""

    def __init__(self, ra):
        self.ra, self.layer, self.calls, self._data = ra, -1, [], None
        rec = self
        real_call = ra.AugmentOp.__call__

        def counting_call(op, img_list):
            rec.layer += 1
            return real_call(op, img_list)

        ra.AugmentOp.__call__ = counting_call
        self._real_transform = real_transform = Image.Image.transform

        def watching_transform(img, size, method, data=None, *a, **k):
            rec._data = tuple(float(v) for v in data)
            return real_transform(img, size, method, data, *a, **k)

        Image.Image.transform = watching_transform
        for name, fn in list(ra.NAME_TO_OP.items()):
            ra.NAME_TO_OP[name] = self._wrap(name, fn)

    def _wrap(self, name, fn):
        def run(img, *level, **kw):
            self._data = None
            out = fn(img, *level, **kw)
            self.calls.append(dict(layer=self.layer, name=name, level=level, data=self._data, inp=np.asarray(img).copy(),
                                   out=np.asarray(out).copy()))
            return out
        return run

    def start(self):
        self.layer, self.calls = -1, []

    def close(self):
        Image.Image.transform = self._real_transform

    def plan(self, names, T):
        """(ops [8], args [8,6], flags) of the calls since start()."""
        ops, args, flags = np.zeros(8, dtype=np.int32), np.zeros((8, 6), dtype=np.float64), set()
        layers = sorted({c["layer"] for c in self.calls})
        for layer in layers:
            calls = [c for c in self.calls if c["layer"] == layer]
            assert len(calls) == T and len({(c["name"], c["level"], c["data"]) for c in calls}) == 1, (layer, len(calls))
            c = calls[0]
            base = c["name"].replace("Increasing", "")
            code = [n.replace("Increasing", "") for n in names].index(base) + 1
            if base in AFFINE:
                if c["data"] is None:                # PIL's shortcut for the angle 0: a copy
                    assert base == "Rotate" and c["level"][0] % 360.0 == 0
                    continue
                args[layer] = c["data"]
                sign = c["level"][0] > 0
                flags.add((base, "+" if sign else "-"))
                H, W = c["inp"].shape[:2]
                a = c["data"]
                if base == "Rotate":
                    x, y = a[0] * 0.5 + a[1] * 0.5 + a[2], a[3] * 0.5 + a[4] * 0.5 + a[5]
                    if not (0 <= x < W and 0 <= y < H):
                        flags.add("rotate_corner_out")
                if base.startswith("Translate") and max(abs(a[2]), abs(a[5])) >= 1:
                    flags.add("translate_fill_band")
            elif c["level"]:
                args[layer, 0] = c["level"][0]
                if base in ENHANCE:
                    flags.add((base, "<1" if c["level"][0] < 1 else ">1"))
                if base == "Posterize" and c["level"][0] == 0:
                    flags.add("posterize_0_bits")
            ops[layer] = code
            for c in calls:
                one = [len(np.unique(c["inp"][..., ch])) == 1 for ch in range(3)]
                if base == "AutoContrast":
                    flags.add("autocontrast_changes" if not np.array_equal(c["inp"], c["out"]) else "autocontrast_identity")
                    if any(one):
                        flags.add("autocontrast_constant_channel")
                if base == "Equalize":
                    if any(one):
                        flags.add("equalize_constant_channel")
                    for ch in range(3):
                        h = np.bincount(c["inp"][..., ch].reshape(-1), minlength=256)
                        nz = np.nonzero(h)[0]
                        step = (int(h.sum()) - int(h[nz[-1]])) // 255 if len(nz) > 1 else 0
                        if step:
                            flags.add("equalize_step")
                            if len(nz) < 64:
                                flags.add("equalize_step_narrow")
                            if (step // 2 + int(h[:255].sum())) // step > 255:
                                flags.add("equalize_clip_255")
        applied = [int(v) for v in ops if v]
        flags.add(f"applied_{len(applied)}")
        if any(ops[k] and ops[k] == ops[k + 1] for k in range(7)):
            flags.add("twice_in_a_row")
        for v in applied:
            flags.add(("op", v))
        return ops, args, flags


def wanted():
    w = {("op", k): 2 for k in range(1, 16)}
    for n in AFFINE:
        w[(n, "+")] = w[(n, "-")] = 1
    for n in ENHANCE:
        w[(n, "<1")] = w[(n, ">1")] = 1
    for f in ("autocontrast_changes", "autocontrast_constant_channel", "equalize_constant_channel", "equalize_step_narrow",
              "equalize_clip_255", "posterize_0_bits", "applied_4", "applied_0", "twice_in_a_row", "rotate_corner_out",
              "translate_fill_band"):
        w[f] = 1
    return w


class Reference:
    """The reference's RandAugment and eval training transform, loaded from a checkout at `root` with the recorder in place (also
    used by tests/test_randaug_host.py for its comparison against the live module)."""

    def __init__(self, root):
        global REF
        REF = root
        self.ra = ra = _import("ref_randaugment", "src", "datasets", "utils", "video", "randaugment.py")
        self.randerase = randerase = _import("ref_randerase", "src", "datasets", "utils", "video", "randerase.py")
        self.rec = Recorder(ra)

        class _NoImage:
            class Image:
                pass
        pil = types.SimpleNamespace(Image=_NoImage)
        fns = dict(np=np, torch=torch, numbers=numbers, PIL=pil, cv2=None)
        fnames = ["_is_tensor_clip", "crop_clip", "resize_clip", "get_resize_sizes", "normalize"]
        _reference_defs("src/datasets/utils/video/functional.py", fnames, fns)
        FF = types.SimpleNamespace(**{n: fns[n] for n in fnames})
        self.vns = vns = dict(torch=torch, np=np, math=math, random=random, numbers=numbers, PIL=pil, FF=FF, Image=Image,
                   transforms=types.SimpleNamespace(Compose=_Chain), rand_augment_transform=ra.rand_augment_transform)
        vnames = ["_get_param_spatial_crop", "random_resized_crop", "random_resized_crop_with_shift", "horizontal_flip", "Compose",
                  "Resize", "CenterCrop", "Normalize", "create_random_augment", "_pil_interp"]
        _reference_defs("src/datasets/utils/video/transforms.py", vnames, vns)
        video_transforms = types.SimpleNamespace(**{n: vns[n] for n in vnames})
        cns = dict(np=np, torch=torch, Image=_NoImage)
        _reference_defs("src/datasets/utils/video/volume_transforms.py", ["convert_img", "ClipToTensor"], cns)
        volume_transforms = types.SimpleNamespace(ClipToTensor=cns["ClipToTensor"])
        tv = types.SimpleNamespace(ToPILImage=lambda: Image.fromarray,
                                   ToTensor=lambda: (lambda img: torch.from_numpy(np.array(img)).permute(2, 0, 1)
                                                     .contiguous().to(torch.float32).div(255)))
        ens = dict(np=np, torch=torch, transforms=tv, video_transforms=video_transforms, volume_transforms=volume_transforms,
                   RandomErasing=randerase.RandomErasing, print=lambda *a, **k: None)
        self.VideoTransform, _ = _reference_defs("evals/video_classification_frozen/utils.py", ["VideoTransform", "tensor_normalize"], ens)

    def names_of(self, config):
        ra = self.ra
        return ra._RAND_INCREASING_TRANSFORMS if "inc" in [s.rstrip("0123456789.") for s in config.split("-")] else ra._RAND_TRANSFORMS

    def run_aug(self, config, frames, seed):
        """(ops, args, coverage flags, augmented frames, next draws) of the reference's RandAugment `config` on uint8 frames."""
        tf = self.vns["create_random_augment"](input_size=(16, 16), auto_augment=config, interpolation="bicubic")
        seed_all(seed)
        self.rec.start()
        out = tf([Image.fromarray(f) for f in frames])
        nxt = next_draws()
        ops, args, flags = self.rec.plan(self.names_of(config), len(frames))
        return ops, args, flags, np.stack([np.asarray(o) for o in out]), nxt


def main():
    if not REF or not os.path.isfile(os.path.join(REF, "src", "datasets", "utils", "video", "randaugment.py")):
        raise SystemExit("set JEPA_REFERENCE to the root of a facebookresearch/jepa checkout")
    torch.set_num_threads(1)
    R = Reference(REF)
    rec, vns, randerase, run_aug, names_of, VideoTransform = R.rec, R.vns, R.randerase, R.run_aug, R.names_of, R.VideoTransform

    out = {}
    want = wanted()
    have = {k: 0 for k in want}
    names, all_flags = [], set()

    def keep(name, config, seed, frames, ops, args, aug, nxt, flags):
        names.append(name)
        out[f"{name}/config"], out[f"{name}/seed"], out[f"{name}/frames"] = np.array(config), np.array(seed), frames
        out[f"{name}/ops"], out[f"{name}/args"], out[f"{name}/aug"], out[f"{name}/next"] = ops, args, aug, nxt
        for f in flags:
            all_flags.add(f)
            if f in have:
                have[f] += 1
        print(f"{name}: {config} seed {seed} source {frames.shape} ops {ops.tolist()}")

    # -- the eval's training transform, RandAugment first
    seen = []
    real_interpolate = torch.nn.functional.interpolate

    def watching_interpolate(x, *a, **k):
        seen.append((int(x[0, 0, 0, 0]), int(x[1, 0, 0, 0]), x.shape[-2], x.shape[-1]))
        return real_interpolate(x, *a, **k)

    real_get_pixels = randerase._get_pixels
    for name, hw, side, reprob, kind in TRAIN_CASES:
        T = 4
        frames = frames_for(name, hw, T, kind)
        seed = 5 * len(names)
        while True:      # a seed whose plan applies something
            ops, args, flags, aug, _ = run_aug(EVAL_CONFIG, frames, seed)
            if (ops != 0).sum() >= 2:
                break
            seed += 1
        # boxes and flip: the spatial function under the generator state that the RandAugment draws leave, on a coordinate image
        seed_all(seed)
        rec.start()
        vns["create_random_augment"](input_size=(side, side), auto_augment=EVAL_CONFIG, interpolation="bicubic")(
            [Image.fromarray(f) for f in frames])
        coord = torch.zeros(3, T, hw[0], hw[1])
        coord[0] = torch.arange(hw[0], dtype=torch.float32)[None, :, None]
        coord[1] = torch.arange(hw[1], dtype=torch.float32)[None, None, :]
        del seen[:]
        torch.nn.functional.interpolate = watching_interpolate
        try:
            res = vns["random_resized_crop"](images=coord, target_height=side, target_width=side, scale=(0.3, 1.0), ratio=(3 / 4, 4 / 3))
        finally:
            torch.nn.functional.interpolate = real_interpolate
        flipped, _ = vns["horizontal_flip"](0.5, res)
        boxes, flip = np.array(list(seen) * T, dtype=np.int32), flipped is not res
        assert len(boxes) == T

        class _RecordingRandom:
            def __init__(self):
                self.randints = []

            def __getattr__(self, n):
                return getattr(random, n)

            def randint(self, a, b):
                v = random.randint(a, b)
                self.randints.append(v)
                return v

        rr, shapes, noise = _RecordingRandom(), [], []

        def recording_get_pixels(per_pixel, rand_color, patch_size, **k):
            v = real_get_pixels(per_pixel, rand_color, patch_size, **k)
            shapes.append(tuple(patch_size))
            noise.append(v.clone())
            return v

        randerase.random, randerase._get_pixels = rr, recording_get_pixels
        try:
            tf = VideoTransform(training=True, auto_augment=True, reprob=reprob, crop_size=side)
            seed_all(seed)
            rec.start()
            ref = tf(frames)
        finally:
            randerase.random, randerase._get_pixels = random, real_get_pixels
        nxt = next_draws()
        ops2, args2, flags2 = rec.plan(names_of(EVAL_CONFIG), T)
        assert np.array_equal(ops, ops2) and np.array_equal(args, args2)
        assert isinstance(ref, list) and len(ref) == 1 and ref[0].shape == (3, T, side, side) and ref[0].dtype == torch.float32
        ref = ref[0]
        if noise:
            assert len(noise) == T and len(set(shapes)) == 1 and len(rr.randints) == 2
            ebox = np.array([rr.randints[0], rr.randints[1], shapes[0][1], shapes[0][2]], dtype=np.int32)
            nz = torch.stack(noise).numpy()
            t0, l0, eh, ew = (int(v) for v in ebox)
            assert np.array_equal(ref[:, :, t0:t0 + eh, l0:l0 + ew].permute(1, 0, 2, 3).numpy(), nz)
        else:
            assert reprob == 0.0
            ebox, nz = np.zeros(4, dtype=np.int32), np.zeros((T, 3, 0, 0), dtype=np.float32)
        keep(name, EVAL_CONFIG, seed, frames, ops, args, aug, nxt, flags)
        out[f"{name}/side"], out[f"{name}/reprob"] = np.array(side), np.array(reprob)
        out[f"{name}/boxes"], out[f"{name}/flip"], out[f"{name}/ebox"], out[f"{name}/noise"] = boxes, np.array(flip), ebox, nz
        out[f"{name}/ref"] = ref.numpy().copy()
    train_names = list(names)

    # -- RandAugment alone: candidates in a fixed order, kept while they add something that is still missing
    cand = 0
    while any(have[k] < want[k] for k in want):
        assert cand < 4000, {k: (have[k], want[k]) for k in want if have[k] < want[k]}
        config = CONFIGS[cand % len(CONFIGS)]
        hw = SIZES[(cand // len(CONFIGS)) % len(SIZES)]
        kind = KINDS[(cand // 3) % len(KINDS)]
        T = 2 + cand % 3
        name = f"aug_{cand:04d}"
        frames = frames_for(name, hw, T, kind)
        ops, args, flags, aug, nxt = run_aug(config, frames, cand)
        if any(f in want and have[f] < want[f] for f in flags):
            keep(name, config, cand, frames, ops, args, aug, nxt, flags)
        cand += 1
    assert len(names) <= MAX_CASES, len(names)
    out["names"], out["train_names"] = np.array(names), np.array(train_names)

    # what the fixture must contain
    assert all(have[k] >= want[k] for k in want), have
    assert {int(out[f"{n}/frames"].shape[0]) for n in names} == {2, 3, 4}
    sides = [s for n in names for s in out[f"{n}/frames"].shape[1:3]]
    assert min(sides) >= 16 and max(sides) <= 53
    assert any(out[f"{n}/frames"][0].size % 16 != 0 for n in names) and len({out[f"{n}/frames"].shape[1:3] for n in names}) > 1
    assert any(np.array_equal(out[f"{n}/frames"], out[f"{n}/aug"]) for n in names if not out[f"{n}/ops"].any())
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size <= 1 << 20, size
    print(f"wrote {OUT}: {size} bytes, {len(names)} cases")


if __name__ == "__main__":
    main()
