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
        """The six arguments of one applied operation at magnitude m (randaugment.py:187-264), or None for a rotation by 0."""
        inc = self.increasing
        if code in (AUTO_CONTRAST, EQUALIZE, INVERT):
            return ()
        if code == ROTATE:
            return rotation_coefficients(_randomly_negate((m / _MAX_LEVEL) * 30.0), H, W)
        if code == POSTERIZE:
            bits = int((m / _MAX_LEVEL) * 4)
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
