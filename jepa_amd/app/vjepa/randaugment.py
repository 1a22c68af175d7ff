"""Host half of RandAugment for video clips: the reference's DRAWS (src/datasets/utils/video/randaugment.py:324-369,449-518, built by
create_random_augment, src/datasets/utils/video/transforms.py:625-658), restated, with no pixel work.

The reference picks `n` operations per clip with one `np.random.choice`, and every picked operation then decides on `random` whether
it runs, draws its magnitude with `random.gauss` and, where it is signed, its sign -- once for all frames of the clip -- before PIL
does the pixels frame by frame.  `RandAugmentDraw.draw(H, W)` makes the same calls in the same order on the same global generators,
so a seeded stream is the reference's draw for draw, and returns the plan as two small tables that `vj_clip_randaug`
(csrc/clip_randaug.hip) carries out on the uint8 frames on the device:

    ops   int32 [8]      operation code per layer, in order; 0: nothing (not picked, skipped by its coin, or a rotation by 0)
    args  float64 [8,6]  the six affine coefficients (Rotate, ShearX/Y, TranslateX/YRel; computed here in Python floats, PIL's own
                         arithmetic for the rotation: PIL/Image.py rotate), or in column 0 the enhance factor, the bits kept, the
                         solarize threshold or the addend

Codes follow the reference's list (randaugment.py:372-407).  Not implemented, raising: the `w` section (weighted choice without
replacement) and more than 8 layers (the width of the table).

`AutoAugmentDraw('original')` is the image evals' learned policy: timm's `auto_augment='original'`, which the reference's image
training transform asks for (evals/image_classification_frozen/eval.py:392-403).  timm's AutoAugment.__call__ picks one of 25
sub-policies of two operations and runs both through AugmentOp.__call__ -- the class the reference restates at
randaugment.py:324-369, with the same LEVEL_TO_ARG table (PosterizeOriginal: line 243).  The draws are made on Python's `random`
alone, in timm's order: `random.choice(policy)`; per operation `random.random() > prob`, drawn only when prob < 1.0; then the sign
draw of Rotate / ShearX.  'original' has no magnitude noise, so there is no `gauss`.  It returns the same two tables, at most two
layers live, and shares the operation codes and the level arithmetic of this module with RandAugmentDraw.
  * The policy table below is restated from the AutoAugment paper's ImageNet policy as timm's auto_augment_policy_original lists
    it.  It was NOT checked against a timm install (none was at hand).
  * Stream parity with timm's draws is not claimed, as for the image evals' box and erase draws.
  * Given a plan, the pixels are PIL's byte for byte (vj_clip_randaug_fill with timm's fill colour, the rounded dataset mean).
`auto_augment_draw(value)` is the one parser of the image evals' `data.auto_augment` key: None, 'original' or a `rand-...` string.
"""
import math
import random
import re

import numpy as np

MAX_LAYERS = 8
NUM_ARGS = 6
(NONE, AUTO_CONTRAST, EQUALIZE, INVERT, ROTATE, POSTERIZE, SOLARIZE, SOLARIZE_ADD, COLOR, CONTRAST, BRIGHTNESS, SHARPNESS, SHEAR_X,
 SHEAR_Y, TRANSLATE_X_REL, TRANSLATE_Y_REL) = range(16)
NUM_OPS = 15
OP_NAMES = ("None", "AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast",
            "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
AFFINE_OPS = (ROTATE, SHEAR_X, SHEAR_Y, TRANSLATE_X_REL, TRANSLATE_Y_REL)
ENHANCE_OPS = (COLOR, CONTRAST, BRIGHTNESS, SHARPNESS)
MIN_SIDE = 3            # Sharpness filters 3 x 3 neighbourhoods

_MAX_LEVEL = 10.0


def _randomly_negate(v):
    return -v if random.random() > 0.5 else v


def rotation_coefficients(degrees, H, W):
    """The six coefficients PIL's Image.rotate hands to its affine transform for a W x H image (centre of the image, no
    translation, no expansion), or None for the angle 0, which PIL answers with a copy."""
    angle = degrees % 360.0
    if angle == 0:
        return None
    cx, cy = W / 2, H / 2
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    x, y = -cx - 0, -cy - 0
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def level_args(code, m, H, W, increasing=False, posterize_original=False):
    """The six arguments of one applied operation at magnitude m (randaugment.py:187-264), or None where the operation changes
    nothing (a rotation by 0; PosterizeOriginal keeping 8 bits or more).  increasing: the reference's `inc` variants;
    posterize_original: PosterizeOriginal's level, 4 up to 8 bits kept (randaugment.py:243-247), for the same Posterize code."""
    inc = increasing
    if code in (AUTO_CONTRAST, EQUALIZE, INVERT):
        return ()
    if code == ROTATE:
        return rotation_coefficients(_randomly_negate((m / _MAX_LEVEL) * 30.0), H, W)
    if code == POSTERIZE:
        bits = int((m / _MAX_LEVEL) * 4)
        if posterize_original:
            return (bits + 4,) if bits + 4 < 8 else None
        return (4 - bits if inc else bits,)
    if code == SOLARIZE:
        thresh = int((m / _MAX_LEVEL) * 256)
        return (256 - thresh if inc else thresh,)
    if code == SOLARIZE_ADD:
        return (int((m / _MAX_LEVEL) * 110),)
    if code in ENHANCE_OPS:
        if inc:
            return (1.0 + _randomly_negate((m / _MAX_LEVEL) * 0.9),)
        return ((m / _MAX_LEVEL) * 1.8 + 0.1,)
    if code in (SHEAR_X, SHEAR_Y):
        f = _randomly_negate((m / _MAX_LEVEL) * 0.3)
        return (1, f, 0, 0, 1, 0) if code == SHEAR_X else (1, 0, 0, f, 1, 0)
    pct = _randomly_negate((m / _MAX_LEVEL) * 0.45)
    return (1, 0, pct * W, 0, 1, 0) if code == TRANSLATE_X_REL else (1, 0, 0, 0, 1, pct * H)


class RandAugmentDraw:
    def __init__(self, config_str='rand-m7-n4-mstd0.5-inc1'):
        config = config_str.split("-")
        if config[0] != "rand":
            raise ValueError(f"RandAugmentDraw: {config_str!r} does not start with 'rand'")
        self.magnitude, self.num_layers, self.magnitude_std, self.increasing = _MAX_LEVEL, 2, 0, False
        for c in config[1:]:
            cs = re.split(r"(\d.*)", c)
            if len(cs) < 2:
                continue
            key, val = cs[:2]
            if key == "mstd":
                self.magnitude_std = float(val)
            elif key == "inc":
                self.increasing = self.increasing or bool(val)     # the reference's quirk: any digit, '0' included, is true
            elif key == "m":
                self.magnitude = int(val)
            elif key == "n":
                self.num_layers = int(val)
            elif key == "w":
                raise NotImplementedError(f"RandAugmentDraw: the 'w' section of {config_str!r} (weighted choice without "
                                          "replacement) is not implemented")
        if not 0 <= self.num_layers <= MAX_LAYERS:
            raise ValueError(f"RandAugmentDraw: n={self.num_layers} layers do not fit the table of {MAX_LAYERS}")
        self.config_str = config_str

    def _level(self, code, m, H, W):
        return level_args(code, m, H, W, increasing=self.increasing)

    def draw(self, H, W):
        """(ops int32 [8], args float64 [8,6]) for one clip of H x W frames; consumes `np.random` and `random` exactly as the
        reference's RandAugment.__call__ and AugmentOp.__call__ do."""
        ops = np.zeros(MAX_LAYERS, dtype=np.int32)
        args = np.zeros((MAX_LAYERS, NUM_ARGS), dtype=np.float64)
        picked = np.random.choice(NUM_OPS, self.num_layers, replace=True)
        for layer, k in enumerate(picked):
            if random.random() > 0.5:
                continue
            m = self.magnitude
            if self.magnitude_std and self.magnitude_std > 0:
                m = random.gauss(m, self.magnitude_std)
            m = min(_MAX_LEVEL, max(0, m))
            code = int(k) + 1
            a = self._level(code, m, H, W)
            if a is None:
                continue
            ops[layer] = code
            args[layer, :len(a)] = a
        return ops, args


# timm's auto_augment_policy_original: (name, probability, magnitude) twice per sub-policy (module docstring: restated from the
# AutoAugment paper's ImageNet policy, not checked against a timm install)
POLICY_ORIGINAL = (
    (("PosterizeOriginal", 0.4, 8), ("Rotate", 0.6, 9)),
    (("Solarize", 0.6, 5), ("AutoContrast", 0.6, 5)),
    (("Equalize", 0.8, 8), ("Equalize", 0.6, 3)),
    (("PosterizeOriginal", 0.6, 7), ("PosterizeOriginal", 0.6, 6)),
    (("Equalize", 0.4, 7), ("Solarize", 0.2, 4)),
    (("Equalize", 0.4, 4), ("Rotate", 0.8, 8)),
    (("Solarize", 0.6, 3), ("Equalize", 0.6, 7)),
    (("PosterizeOriginal", 0.8, 5), ("Equalize", 1.0, 2)),
    (("Rotate", 0.2, 3), ("Solarize", 0.6, 8)),
    (("Equalize", 0.6, 8), ("PosterizeOriginal", 0.4, 6)),
    (("Rotate", 0.8, 8), ("Color", 0.4, 0)),
    (("Rotate", 0.4, 9), ("Equalize", 0.6, 2)),
    (("Equalize", 0.0, 7), ("Equalize", 0.8, 8)),
    (("Invert", 0.6, 4), ("Equalize", 1.0, 8)),
    (("Color", 0.6, 4), ("Contrast", 1.0, 8)),
    (("Rotate", 0.8, 8), ("Color", 1.0, 2)),
    (("Color", 0.8, 8), ("Solarize", 0.8, 7)),
    (("Sharpness", 0.4, 7), ("Invert", 0.6, 8)),
    (("ShearX", 0.6, 5), ("Equalize", 1.0, 9)),
    (("Color", 0.4, 0), ("Equalize", 0.6, 3)),
    (("Equalize", 0.4, 7), ("Solarize", 0.2, 4)),
    (("Solarize", 0.6, 5), ("AutoContrast", 0.6, 5)),
    (("Invert", 0.6, 4), ("Equalize", 1.0, 8)),
    (("Color", 0.6, 4), ("Contrast", 1.0, 8)),
    (("Equalize", 0.8, 8), ("Equalize", 0.6, 3)),
)
AUTO_AUGMENT_POLICIES = ("original",)


def policy_code(name):
    """Operation code of a policy entry's name; PosterizeOriginal is the Posterize code with its own level function."""
    return POSTERIZE if name == "PosterizeOriginal" else OP_NAMES.index(name)


class AutoAugmentDraw:
    """timm's AutoAugment for `auto_augment='original'` as draws (module docstring).  `policy`: the table it draws from, a sequence
    of sub-policies of (name, probability, magnitude) entries (default: POLICY_ORIGINAL)."""

    def __init__(self, config_str='original', policy=None):
        if config_str not in AUTO_AUGMENT_POLICIES:
            raise ValueError(f"AutoAugmentDraw: policy {config_str!r} is not implemented; accepted: "
                             f"{', '.join(map(repr, AUTO_AUGMENT_POLICIES))} (no 'originalr', 'v0', 'v0r', '3a', 'augmix-*', and no "
                             "'-mstd' suffix)")
        self.config_str = config_str
        self.policy = POLICY_ORIGINAL if policy is None else tuple(policy)
        if any(len(sub) > MAX_LAYERS for sub in self.policy):
            raise ValueError(f"AutoAugmentDraw: a sub-policy has more than {MAX_LAYERS} operations")

    @staticmethod
    def _run(sub_policy, applies, H, W):
        """The tables of one sub-policy; applies(layer, prob) says whether an operation runs, and is asked right before the
        operation's own sign draw, as AugmentOp.__call__ decides and then computes its level."""
        ops = np.zeros(MAX_LAYERS, dtype=np.int32)
        args = np.zeros((MAX_LAYERS, NUM_ARGS), dtype=np.float64)
        for layer, (name, prob, magnitude) in enumerate(sub_policy):
            if not applies(layer, prob):
                continue
            code = policy_code(name)
            a = level_args(code, min(_MAX_LEVEL, max(0, magnitude)), H, W, posterize_original=name == "PosterizeOriginal")
            if a is None:
                continue
            ops[layer] = code
            args[layer, :len(a)] = a
        return ops, args

    def plan(self, sub_policy, applied, H, W):
        """The tables of `sub_policy` with operation l running when applied[l]: no coin is drawn, only the signs of Rotate / ShearX
        (on `random`).  What the fixture tool uses to force both operations."""
        return self._run(sub_policy, lambda layer, prob: bool(applied[layer]), H, W)

    def draw(self, H, W):
        """(ops int32 [8], args float64 [8,6]) for one H x W image; consumes Python's `random` as timm's AutoAugment.__call__ and
        AugmentOp.__call__ do, and no other generator."""
        sub_policy = random.choice(self.policy)
        return self._run(sub_policy, lambda layer, prob: not (prob < 1.0 and random.random() > prob), H, W)


def auto_augment_draw(value):
    """The image evals' `data.auto_augment` -> None (absent / null: off), AutoAugmentDraw('original'), or RandAugmentDraw for a
    `rand-...` string (timm's rand_augment_transform, e.g. 'rand-m9-mstd0.5-inc1'; its `w` section raises).  Anything else raises
    ValueError naming what is accepted."""
    if value is None:
        return None
    if isinstance(value, str) and value.startswith("rand-"):
        return RandAugmentDraw(value)
    if isinstance(value, str) and value in AUTO_AUGMENT_POLICIES:
        return AutoAugmentDraw(value)
    raise ValueError(f"data.auto_augment={value!r}: accepted are null (off), 'original' and a 'rand-...' string such as "
                     "'rand-m9-mstd0.5-inc1'; timm's 'originalr', 'v0', 'v0r', '3a', 'augmix-*' policies and '-mstd' suffixes of "
                     "the learned policies are not implemented")
