"""Writes tests/golden/image_resample_micro.npz: what Pillow gives for the crop-and-resize cases that pin vj_image_resample, and what
the reference's image transforms (evals/image_classification_frozen/eval.py:379-423: flip, ToTensor, Normalize, RandomErasing) make
of a few of them in fp32.  CPU only; needs Pillow.

    python tools/make_golden_image_resample.py

Per case: a source image (shared between cases), the geometry row (i, j, h, w, OH, OW, wy, wx), the output side S, the filter code
(0 bilinear, 1 bicubic) and Image.crop(box).resize((OW, OH), filter)[wy:wy+S, wx:wx+S].  Every sub-case exists for both filters and
for S = 8 and S = 12:
    up        5x7 -> S x S: upscale on both axes
    down      61x97 -> S x S: reduction on both axes
    thin      a 200x3 crop -> S x S: a 25x reduction on one axis with an upscale on the other
    ident     S x 23 -> S x S: one identity axis
    corner*   crops at the four corners of an image, and a 1x1 crop: the bound clamps at both ends
    checker*  0/255 checkerboards, reduced and enlarged: the bicubic overshoot clamps at both ends, in the intermediate too
    val*      the validation form: 30x47, 47x30 and 12x40 sources, short side to R, centre window (R = 12 for S = 8, 16 for S = 12)
The chain cases take the S = 8 bicubic results of `down`, `corner0`, `checker_up` and `val0` with and without flip and with an erase
box each, through PIL's FLIP_LEFT_RIGHT and fp32 torch operations.
"""
import os
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "image_resample_micro.npz")
PIL_FILTER = {0: Image.BILINEAR, 1: Image.BICUBIC}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def sources(rng):
    yy, xx = np.mgrid[0:61, 0:97]
    checker1 = np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    checker3 = np.repeat((((yy // 3 + xx // 3) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    checker3[:, :, 1] = 255 - checker3[:, :, 1]                 # the channels disagree
    shapes = [(5, 7), (61, 97), (210, 40), (8, 23), (12, 23), (30, 47), (47, 30), (12, 40)]
    src = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    return src + [checker1, checker3]


def short_side(H, W, R):
    return (R, int(R * W / H)) if H <= W else (int(R * H / W), R)


def cases_for(S):
    """[(name, source index, geometry row)] for output side S."""
    R = {8: 12, 12: 16}[S]
    c = [("up", 0, (0, 0, 5, 7, S, S, 0, 0)),
         ("down", 1, (0, 0, 61, 97, S, S, 0, 0)),
         ("thin", 2, (5, 17, 200, 3, S, S, 0, 0)),
         ("ident", 3 if S == 8 else 4, (0, 0, S, 23, S, S, 0, 0)),
         ("corner0", 1, (0, 0, 20, 31, S, S, 0, 0)),
         ("corner1", 1, (0, 66, 20, 31, S, S, 0, 0)),
         ("corner2", 1, (41, 0, 20, 31, S, S, 0, 0)),
         ("corner3", 1, (41, 66, 20, 31, S, S, 0, 0)),
         ("one_pixel", 1, (30, 50, 1, 1, S, S, 0, 0)),
         ("checker_down", 8, (0, 0, 61, 97, S, S, 0, 0)),
         ("checker3_down", 9, (1, 2, 59, 94, S, S, 0, 0)),
         ("checker_up", 8, (10, 20, 5, 6, S, S, 0, 0)),
         ("checker3_up", 9, (0, 0, 7, 9, S, S, 0, 0))]
    for k, (idx, (H, W)) in enumerate(((5, (30, 47)), (6, (47, 30)), (7, (12, 40)))):
        OH, OW = short_side(H, W, R)
        c.append((f"val{k}", idx, (0, 0, H, W, OH, OW, int(round((OH - S) / 2.0)), int(round((OW - S) / 2.0)))))
    return c


def pil_window(src, geom, S, filt):
    i, j, h, w, OH, OW, wy, wx = geom
    im = Image.fromarray(src).crop((j, i, j + w, i + h)).resize((OW, OH), PIL_FILTER[filt])
    return np.ascontiguousarray(np.asarray(im)[wy:wy + S, wx:wx + S])


def chain(window, flip, ebox, noise):
    im = Image.fromarray(window)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    x = torch.from_numpy(np.array(im)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)          # ToTensor
    x = x.sub(torch.tensor(MEAN, dtype=torch.float32)[:, None, None]).div(torch.tensor(STD, dtype=torch.float32)[:, None, None])
    top, left, eh, ew = ebox
    if eh > 0:
        x[:, top:top + eh, left:left + ew] = noise                                                       # RandomErasing, pixel mode
    return x.numpy()


def main():
    import PIL
    rng = np.random.RandomState(20240611)
    src = sources(rng)
    out = {f"src_{k}": s for k, s in enumerate(src)}
    names, src_index, geoms, sides, filters = [], [], [], [], []
    for S in (8, 12):
        for filt in (0, 1):
            for name, idx, geom in cases_for(S):
                out[f"want_{len(names)}"] = pil_window(src[idx], geom, S, filt)
                names.append(f"{name}-S{S}-{'bicubic' if filt else 'bilinear'}")
                src_index.append(idx), geoms.append(geom), sides.append(S), filters.append(filt)
    # the reference chain on a few S = 8 bicubic results
    g = torch.Generator().manual_seed(7)
    chain_case, chain_flip, chain_ebox = [], [], []
    plans = [("down", False, (0, 0, 0, 0)), ("down", True, (2, 1, 3, 4)), ("corner0", True, (0, 0, 0, 0)),
             ("checker_up", False, (0, 5, 7, 2)), ("val0", True, (4, 0, 2, 7)), ("val0", False, (0, 0, 0, 0))]
    noise_blocks = []
    for k, (name, flip, ebox) in enumerate(plans):
        n = names.index(f"{name}-S8-bicubic")
        noise = torch.empty((3, ebox[2], ebox[3]), dtype=torch.float32).normal_(generator=g)
        out[f"chain_{k}"] = chain(out[f"want_{n}"], flip, ebox, noise)
        out[f"chain_noise_{k}"] = noise.numpy()
        chain_case.append(n), chain_flip.append(int(flip)), chain_ebox.append(ebox)
        noise_blocks.append(noise)
    out.update(names=np.array(names), src_index=np.array(src_index, dtype=np.int32), geom=np.array(geoms, dtype=np.int32),
               S=np.array(sides, dtype=np.int32), filter=np.array(filters, dtype=np.int32), num_cases=np.int32(len(names)),
               chain_case=np.array(chain_case, dtype=np.int32), chain_flip=np.array(chain_flip, dtype=np.int32),
               chain_ebox=np.array(chain_ebox, dtype=np.int32), mean=np.array(MEAN, dtype=np.float64),
               std=np.array(STD, dtype=np.float64), pillow_version=np.array(PIL.__version__))
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(names)} cases, {len(plans)} chain cases, Pillow {PIL.__version__}, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    sys.exit(main())
