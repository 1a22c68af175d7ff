"""Helpers of the image AutoAugment tests: the fixture tests/golden/image_autoaug_micro.npz (tools/make_golden_image_autoaug.py:
the reference's operation functions through PIL), an independent replay of the draw protocol, and a PIL helper that carries a plan
out from its two tables alone."""
import os
import random

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "image_autoaug_micro.npz")
SIDES = (20, 36, 96)
FILL = (124, 116, 104)

# the issue's table, typed in again here (not imported): (name, probability, magnitude) twice per sub-policy
POLICY = [
    [("PosterizeOriginal", .4, 8), ("Rotate", .6, 9)], [("Solarize", .6, 5), ("AutoContrast", .6, 5)],
    [("Equalize", .8, 8), ("Equalize", .6, 3)], [("PosterizeOriginal", .6, 7), ("PosterizeOriginal", .6, 6)],
    [("Equalize", .4, 7), ("Solarize", .2, 4)], [("Equalize", .4, 4), ("Rotate", .8, 8)],
    [("Solarize", .6, 3), ("Equalize", .6, 7)], [("PosterizeOriginal", .8, 5), ("Equalize", 1., 2)],
    [("Rotate", .2, 3), ("Solarize", .6, 8)], [("Equalize", .6, 8), ("PosterizeOriginal", .4, 6)],
    [("Rotate", .8, 8), ("Color", .4, 0)], [("Rotate", .4, 9), ("Equalize", .6, 2)],
    [("Equalize", .0, 7), ("Equalize", .8, 8)], [("Invert", .6, 4), ("Equalize", 1., 8)],
    [("Color", .6, 4), ("Contrast", 1., 8)], [("Rotate", .8, 8), ("Color", 1., 2)],
    [("Color", .8, 8), ("Solarize", .8, 7)], [("Sharpness", .4, 7), ("Invert", .6, 8)],
    [("ShearX", .6, 5), ("Equalize", 1., 9)], [("Color", .4, 0), ("Equalize", .6, 3)],
    [("Equalize", .4, 7), ("Solarize", .2, 4)], [("Solarize", .6, 5), ("AutoContrast", .6, 5)],
    [("Invert", .6, 4), ("Equalize", 1., 8)], [("Color", .6, 4), ("Contrast", 1., 8)],
    [("Equalize", .8, 8), ("Equalize", .6, 3)],
]
CODES = {"AutoContrast": 1, "Equalize": 2, "Invert": 3, "Rotate": 4, "PosterizeOriginal": 5, "Solarize": 6, "Color": 8, "Contrast": 9,
         "Sharpness": 11, "ShearX": 12}


def seed_all(s):
    random.seed(s), np.random.seed(s), torch.manual_seed(s)


def cases(z, S):
    """[(name, source uint8 [S,S,3], flip, ops int32 [8], args float64 [8,6], expected uint8 [S,S,3])] of one side."""
    names = [str(n) for n in z[f"case_{S}/name"]]
    return [(n, z[f"src_{S}"][int(z[f"case_{S}/src"][k])], bool(z[f"case_{S}/flip"][k]), z[f"case_{S}/ops"][k], z[f"case_{S}/args"][k],
             z[f"case_{S}/out"][k]) for k, n in enumerate(names)]


def replay_draw(seed, H, W):
    """The plan of `random.seed(seed)` written straight from the stated order -- random.choice, a coin only when prob < 1, the sign
    draw of Rotate / ShearX -- with the rotation's coefficients from the package's own rotation_coefficients (PIL's arithmetic,
    pinned elsewhere).  Returns (sub-policy index, ops, args, coins drawn, the next random.random())."""
    from jepa_amd.app.vjepa.randaugment import rotation_coefficients
    random.seed(seed)
    p = random.choice(range(len(POLICY)))      # random.choice(POLICY) by its index: five sub-policies appear twice in the table
    sub = POLICY[p]
    ops, args, coins = np.zeros(8, np.int32), np.zeros((8, 6), np.float64), 0
    for layer, (name, prob, m) in enumerate(sub):
        if prob < 1.0:
            coins += 1
            if random.random() > prob:
                continue
        a = ()
        if name == "Rotate":
            deg = (m / 10) * 30.0
            deg = -deg if random.random() > 0.5 else deg
            a = rotation_coefficients(deg, H, W)
        elif name == "ShearX":
            f = (m / 10) * 0.3
            f = -f if random.random() > 0.5 else f
            a = (1, f, 0, 0, 1, 0)
        elif name in ("Color", "Contrast", "Sharpness"):
            a = ((m / 10) * 1.8 + 0.1,)
        elif name == "Solarize":
            a = (int((m / 10) * 256),)
        elif name == "PosterizeOriginal":
            bits = int((m / 10) * 4) + 4
            a = None if bits >= 8 else (bits,)
        if a is None:
            continue
        ops[layer] = CODES[name]
        args[layer, :len(a)] = a
    return p, ops, args, coins, random.random()


def pil_apply_plan(arr, ops, args, fill=FILL):
    """uint8 [H,W,3] through the plan, with PIL, from the two tables alone."""
    from PIL import Image, ImageEnhance, ImageOps
    img = Image.fromarray(np.ascontiguousarray(arr))
    for code, a in zip((int(c) for c in ops), args):
        if code == 0:
            continue
        if code == 1:
            img = ImageOps.autocontrast(img)
        elif code == 2:
            img = ImageOps.equalize(img)
        elif code == 3:
            img = ImageOps.invert(img)
        elif code in (4, 12, 13, 14, 15):
            img = img.transform(img.size, Image.AFFINE, tuple(float(v) for v in a), resample=Image.BICUBIC, fillcolor=tuple(fill))
        elif code == 5:
            img = ImageOps.posterize(img, int(a[0]))
        elif code == 6:
            img = ImageOps.solarize(img, int(a[0]))
        elif code == 7:
            lut = [min(255, i + int(a[0])) if i < 128 else i for i in range(256)]
            img = img.point(lut + lut + lut)
        else:
            enhance = {8: ImageEnhance.Color, 9: ImageEnhance.Contrast, 10: ImageEnhance.Brightness, 11: ImageEnhance.Sharpness}[code]
            img = enhance(img).enhance(float(a[0]))
    return np.asarray(img).copy()


def batch_items(z, with_plans=True, zero_plans=False):
    """The fixture's mixed batch as a list of RawImage (training form, bicubic, ImageNet mean / std)."""
    from jepa_amd.evals.image_classification_frozen.transforms import BICUBIC, RawImage
    t = torch.tensor(((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)), dtype=torch.float32)
    mean, std = tuple(t[0].tolist()), tuple(t[1].tolist())
    S, items, at, nat = int(z["batch/side"]), [], 0, 0
    for k, (H, W) in enumerate(z["batch/shapes"].tolist()):
        img = torch.from_numpy(z["batch/images"][at:at + H * W * 3].reshape(H, W, 3).copy())
        at += H * W * 3
        ebox = tuple(int(v) for v in z["batch/ebox"][k])
        n = int(z["batch/noise_len"][k])
        noise = torch.from_numpy(z["batch/noise"][nat:nat + n].copy()).reshape(1, 3, ebox[2], ebox[3]) if n else None
        nat += n
        plan = {}
        if with_plans:
            ops, args = z["batch/ops"][k].copy(), z["batch/args"][k].copy()
            if zero_plans:
                ops[:], args[:] = 0, 0
            plan = dict(aug_ops=ops, aug_args=args)
        items.append(RawImage(img, z["batch/geom"][k], bool(z["batch/flip"][k]), S, BICUBIC, mean, std, ebox=ebox, noise=noise, **plan))
    return items
