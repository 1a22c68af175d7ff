#!/usr/bin/env python
"""Generate tests/golden/image_autoaug_micro.npz: what PIL gives, through the reference's own operation functions, for the plans the
image evals' AutoAugment draws make.  CPU only.

    JEPA_REFERENCE=/path/to/jepa python tools/make_golden_image_autoaug.py          (needs Pillow)

src/datasets/utils/video/randaugment.py is imported as it is (as make_golden_randaug.py imports it).  Its AugmentOp -- the class
timm's AutoAugment runs, built on its NAME_TO_OP / LEVEL_TO_ARG tables -- is called with prob 1.0 and the image pipeline's
hparams, img_mean=(124, 116, 104) (timm's fill colour, round(255 * mean)) and interpolation=Image.BICUBIC, on Image.fromarray
images; the `rand-...` case goes through its rand_augment_transform with the same hparams.  The plan tables are the ones
jepa_amd.app.vjepa.randaugment.AutoAugmentDraw / RandAugmentDraw make under the same sign draws, so the fixture pairs "the tables
this package would upload" with "the bytes the reference's PIL path gives".

The file holds data only:
  pillow                    the Pillow version that made the bytes
  fill                      (124, 116, 104)
  level_name / level_mag / level_arg      for every (operation, magnitude) of the policy table what the reference's LEVEL_TO_ARG
                            function returned (NaN where the operation has no level function), signs not negated
  src_S                     uint8 [n,S,S,3] source images, a smooth ramp plus seeded noise, S in 20, 36, 96
  case_S/name, src, flip, ops, args, out   per case: its name, the source index, whether the source is mirrored first, the plan
                            (int32 [8], float64 [8,6]) and PIL's bytes uint8 [S,S,3]
  batch/...                 one mixed-size batch for the end-to-end test: source images (flat, with shapes), geometry rows, flips,
                            plans, erase boxes and noise, and PIL's bytes after crop + bicubic resize, flip and plan
Cases: all 25 sub-policies with both operations forced to apply, each signed operation in both signs, flipped and unflipped, at
S = 20 and S = 36; a handful at S = 96; one no-op plan; one `rand-m9-mstd0.5-inc1` plan with a translate.
"""
import importlib.util
import os
import random
import sys

import numpy as np
import PIL
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = os.environ.get("JEPA_REFERENCE", "")
OUT = os.path.join(ROOT, "tests", "golden", "image_autoaug_micro.npz")

from jepa_amd.app.vjepa import randaugment as RA  # noqa: E402
from jepa_amd.app.vjepa.transforms import draw_erase  # noqa: E402

FILL = (124, 116, 104)
SIDES = (20, 36)
BIG = 96
BIG_POLICIES = (0, 2, 14, 17, 18, 1)       # Rotate, Equalize twice, Color + Contrast, Sharpness, ShearX, AutoContrast
SIGNED = ("Rotate", "ShearX")
RAND_CONFIG = "rand-m9-mstd0.5-inc1"
BATCH_SIDE = 20
BATCH_SIZES = ((41, 53), (33, 47), (64, 48), (30, 30), (57, 39), (24, 70))
MAX_BYTES = 1 << 20


def _import(name, *rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, *rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def source_image(H, W, seed):
    """A smooth ramp plus seeded noise: every channel spans most but not all of 0..255, so Equalize / AutoContrast have work."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    chans = [40 + 150 * x / max(W - 1, 1), 30 + 170 * y / max(H - 1, 1), 60 + 120 * (x + y) / max(H + W - 2, 1)]
    img = np.stack(chans, axis=-1) + rng.randint(-28, 29, size=(H, W, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


class fixed_sign:
    """While active, `random.random()` returns 0.9 (negate=True: the level functions' `random.random() > 0.5`) or 0.1."""

    def __init__(self, negate):
        self.value = 0.9 if negate else 0.1

    def __enter__(self):
        self.saved = random.random
        random.random = lambda: self.value

    def __exit__(self, *exc):
        random.random = self.saved


def hparams():
    return dict(translate_const=250, img_mean=FILL, interpolation=Image.BICUBIC)


def reference_apply(ref, sub_policy, arr, negate):
    """Both operations of a sub-policy forced to apply, through the reference's AugmentOp, on a uint8 [S,S,3] array."""
    img = Image.fromarray(arr)
    with fixed_sign(negate):
        for name, _, magnitude in sub_policy:
            img = ref.AugmentOp(name, prob=1.0, magnitude=magnitude, hparams=hparams())(img)
    return np.asarray(img).copy()


def main():
    if not REF or not os.path.isfile(os.path.join(REF, "src", "datasets", "utils", "video", "randaugment.py")):
        raise SystemExit("set JEPA_REFERENCE to a checkout of the reference")
    torch.set_num_threads(1)
    ref = _import("ref_randaugment", "src", "datasets", "utils", "video", "randaugment.py")
    draw = RA.AutoAugmentDraw("original")
    out = {"pillow": np.array(PIL.__version__), "fill": np.array(FILL, dtype=np.int32)}

    # -- level arguments of the table, from the reference's functions
    pairs = sorted({(name, m) for sub in RA.POLICY_ORIGINAL for name, _, m in sub})
    vals = []
    with fixed_sign(False):
        for name, m in pairs:
            fn = ref.LEVEL_TO_ARG[name]
            vals.append(float("nan") if fn is None else float(fn(m, hparams())[0]))
    out["level_name"] = np.array([n for n, _ in pairs])
    out["level_mag"] = np.array([m for _, m in pairs], dtype=np.int32)
    out["level_arg"] = np.array(vals, dtype=np.float64)

    # -- the cases
    for S in SIDES + (BIG,):
        srcs = [source_image(S, S, 1000 * S + k) for k in range(3)]
        names, src_idx, flips, ops_l, args_l, outs = [], [], [], [], [], []

        def add(name, k, flip, ops, args, expected):
            names.append(name), src_idx.append(k), flips.append(int(flip)), ops_l.append(ops), args_l.append(args)
            outs.append(expected)

        policies = range(len(RA.POLICY_ORIGINAL)) if S != BIG else BIG_POLICIES
        for p in policies:
            sub = RA.POLICY_ORIGINAL[p]
            signs = (False, True) if any(n in SIGNED for n, _, _ in sub) else (False,)
            for negate in signs:
                for flip in ((False, True) if S != BIG else (bool(p % 2),)):
                    k = (p + int(flip)) % len(srcs)
                    with fixed_sign(negate):
                        ops, args = draw.plan(sub, (True, True), S, S)
                    arr = srcs[k][:, ::-1].copy() if flip else srcs[k]
                    add(f"policy{p:02d}_{'neg' if negate else 'pos'}_{'flip' if flip else 'plain'}", k, flip, ops, args,
                        reference_apply(ref, sub, arr, negate))
        if S == SIDES[0]:
            # a plan without an operation: sub-policy 12's first operation never applies and the second is forced off
            ops, args = draw.plan(RA.POLICY_ORIGINAL[12], (False, False), S, S)
            add("noop", 0, True, ops, args, srcs[0][:, ::-1].copy())
            # timm's RandAugment form with a translate: the fill colour shows along an edge
            ra_draw = RA.RandAugmentDraw(RAND_CONFIG)
            transl = (RA.TRANSLATE_X_REL, RA.TRANSLATE_Y_REL)
            for seed in range(1000):
                random.seed(seed), np.random.seed(seed)
                ops, args = ra_draw.draw(S, S)
                if any(int(o) in transl for o in ops):
                    break
            else:
                raise SystemExit("no seed gives a translate")
            random.seed(seed), np.random.seed(seed)
            img = ref.rand_augment_transform(RAND_CONFIG, hparams())(Image.fromarray(srcs[1]))
            add(f"rand_translate_seed{seed}", 1, False, ops, args, np.asarray(img).copy())
        out[f"src_{S}"] = np.stack(srcs)
        out[f"case_{S}/name"] = np.array(names)
        out[f"case_{S}/src"] = np.array(src_idx, dtype=np.int32)
        out[f"case_{S}/flip"] = np.array(flips, dtype=np.uint8)
        out[f"case_{S}/ops"] = np.stack(ops_l).astype(np.int32)
        out[f"case_{S}/args"] = np.stack(args_l).astype(np.float64)
        out[f"case_{S}/out"] = np.stack(outs)

    # -- one whole mixed-size batch
    S = BATCH_SIDE
    random.seed(77), np.random.seed(77), torch.manual_seed(77)
    images = [source_image(H, W, 500 + k) for k, (H, W) in enumerate(BATCH_SIZES)]
    subs = (0, 14, 12, 18, 2, 17)
    geom, flips, ops_l, args_l, eboxes, noises, expected = [], [], [], [], [], [], []
    for k, (img, p) in enumerate(zip(images, subs)):
        H, W = img.shape[:2]
        h, w = random.randint(H // 2, H), random.randint(W // 2, W)
        i, j = random.randint(0, H - h), random.randint(0, W - w)
        flip, negate = k % 2 == 0, k % 3 == 0
        sub = RA.POLICY_ORIGINAL[p]
        applied = (False, False) if p == 12 else (True, True)
        with fixed_sign(negate):
            ops, args = draw.plan(sub, applied, S, S)
        ebox, noise = draw_erase(1.0 if k % 2 else 0.0, num_frames=1, img_h=S, img_w=S)
        pil = Image.fromarray(img).crop((j, i, j + w, i + h)).resize((S, S), Image.BICUBIC)
        if flip:
            pil = pil.transpose(Image.FLIP_LEFT_RIGHT)
        arr = np.asarray(pil).copy()
        if applied[0]:
            arr = reference_apply(ref, sub, arr, negate)
        geom.append((i, j, h, w, S, S, 0, 0)), flips.append(int(flip)), ops_l.append(ops), args_l.append(args)
        eboxes.append(ebox), noises.append(np.zeros(0, np.float32) if noise is None else noise.numpy().reshape(-1))
        expected.append(arr)
    out["batch/side"] = np.array(S, dtype=np.int32)
    out["batch/shapes"] = np.array(BATCH_SIZES, dtype=np.int32)
    out["batch/images"] = np.concatenate([im.reshape(-1) for im in images])
    out["batch/geom"] = np.array(geom, dtype=np.int32)
    out["batch/flip"] = np.array(flips, dtype=np.uint8)
    out["batch/ops"] = np.stack(ops_l).astype(np.int32)
    out["batch/args"] = np.stack(args_l).astype(np.float64)
    out["batch/ebox"] = np.array(eboxes, dtype=np.int32)
    out["batch/noise_len"] = np.array([n.size for n in noises], dtype=np.int64)
    out["batch/noise"] = np.concatenate(noises).astype(np.float32)
    out["batch/out"] = np.stack(expected)

    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size <= MAX_BYTES, f"{OUT}: {size} bytes"
    n = sum(len(out[f"case_{S}/name"]) for S in SIDES + (BIG,))
    print(f"wrote {OUT}: {n} cases + a batch of {len(images)}, {size} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
