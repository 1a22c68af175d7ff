"""The image evals' input edge, measured (profiles/image_uint8_input.md): uint8 images of mixed sizes through vj_image_resample,
vj_clip_transform_pre and vj_clip_erase on the copy stream of engine.input.ImagePrefetcher.

python tools/image_input_bench.py [--launches 30] [--rounds 3] [--steps 12] [--no-edge]
  kernels   vj_image_resample in the training form (random-resized-crop boxes, bicubic, to 224 x 224) and the validation form (whole
            image, bilinear, short side 256, centre window) next to vj_clip_transform_pre on the same outputs: batch 16 and batch 256
            of 375x500 sources, one batch of four 3000x4000 sources.  Interleaved rounds; per kernel the median over the launches of a
            round, then the rounds side by side.
  bytes     what crosses PCIe per batch: the uint8 sources and their tables against the finished fp32 [B,3,224,224].
  edge      the wait of the compute stream at the input edge inside a loop of frozen forwards, batch 16 of 375x500 sources in the
            training form: the ViT-L/16-224 video encoder fed still images (the *_in1k configs) and the ViT-L/16 image model.
python tools/image_input_bench.py --pil     (CPU only, needs Pillow) the same two resizes through PIL on one core, for scale.
python tools/image_input_bench.py --auto-augment [--launches 30] [--rounds 3] [--steps 12] [--no-edge]   (profiles/image_autoaugment.md)
  the `data.auto_augment` path on batches in which EVERY image is flipped and has a two-layer plan of the 'original' policy:
  kernels   vj_image_hflip and vj_clip_randaug_fill per batch beside vj_image_resample for the same batch, batch 16 and 256 of
            224 x 224, and vj_image_hflip beside vj_copy_rows moving the same bytes.
  edge      the wait at the input edge inside the loop of frozen ViT-L forwards with the key on and off, interleaved; the off arm is
            the same loop `edge` above measures, so it can be set beside a run of the parent commit's tool.
python tools/image_input_bench.py --auto-augment --pil    (CPU only, needs Pillow) the same plans through PIL on one core.
Every line printed is one JSON record."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S = 224


def host_batch(n, hw, training, seed=0, pinned=False, two_layer_plans=False):
    """two_layer_plans: every image is flipped and carries a sub-policy of the 'original' policy with both operations applied (the
    most work the key can ask for), sub-policy after sub-policy."""
    from jepa_amd.evals.image_classification_frozen.transforms import make_transforms
    random.seed(seed), np.random.seed(seed), torch.manual_seed(seed)
    tf = make_transforms(training=training, resolution=S)
    g = torch.Generator().manual_seed(seed + 1)
    one = torch.randint(0, 256, hw + (3,), generator=g, dtype=torch.uint8)
    items = [tf(one.roll(k, 0)) for k in range(n)]
    if two_layer_plans:
        from jepa_amd.app.vjepa.randaugment import POLICY_ORIGINAL, AutoAugmentDraw
        draw = AutoAugmentDraw("original")
        for k, it in enumerate(items):
            ops_k, args_k = draw.plan(POLICY_ORIGINAL[k % len(POLICY_ORIGINAL)], (True, True), S, S)
            it.flip, it.aug_ops, it.aug_args = True, torch.from_numpy(ops_k), torch.from_numpy(args_k)
    raw = torch.utils.data.default_collate(items)
    return raw.pin_memory() if pinned else raw


def _median_us(fn, launches):
    fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    return round(statistics.median(us), 2)


def kernels(dev, launches, rounds):
    from jepa_amd.hip import ops
    for n, hw in ((16, (375, 500)), (256, (375, 500)), (4, (3000, 4000))):
        arms = {}
        for form in ("train", "val"):
            raw = host_batch(n, hw, form == "train")
            frames, desc, geom = raw.frames.to(dev), raw.desc.to(dev), raw.geom.to(dev)
            caps = raw.capacities()
            ws = torch.empty(ops.ImageResample.ws_bytes(n, S, *caps), dtype=torch.uint8, device=dev)
            u8 = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev)
            desc1, boxes1 = (t.to(dev) for t in raw.resampled_tables())
            out = torch.empty((n, 3, 1, S, S), dtype=torch.float32, device=dev)
            arms[form + "_resample"] = lambda f=frames, d=desc, g=geom, r=raw, c=caps, w=ws, u=u8: \
                ops.ImageResample.run(f, d, g, S, r.filter, *c, out=u, ws=w)
            arms[form + "_transform_pre"] = lambda u=u8, d=desc1, b=boxes1, r=raw, o=out: \
                ops.clip_transform(u.view(-1), d, b, S, r.mean, r.std, out=o, pre=True)
            arms[form + "_caps"] = caps
        names = [k for k in arms if not k.endswith("_caps")]
        rows = []
        for r in range(rounds):
            order = names if r % 2 == 0 else names[::-1]
            row = {k: _median_us(arms[k], launches) for k in order}
            rows.append({k: row[k] for k in names})
        print(json.dumps({"what": "kernel time, us, median over the launches of a round", "batch": n, "source": list(hw), "S": S,
                          "launches": launches, "capacities(taps_x,taps_y,rows)": {"train": arms["train_caps"], "val": arms["val_caps"]},
                          "rounds": rows}), flush=True)


def h2d_bytes():
    for n, hw in ((16, (375, 500)), (256, (375, 500)), (4, (3000, 4000))):
        raw = host_batch(n, hw, True)
        tables = sum(t.numel() * t.element_size() for t in (raw.desc, raw.geom) + raw.resampled_tables())
        erase = sum(t.numel() * t.element_size() for t in (raw.ebox, raw.noise, raw.noise_off)) if raw.erased else 0
        fp32 = n * 3 * S * S * 4
        print(json.dumps({"what": "host-to-device bytes per batch", "batch": n, "source": list(hw), "uint8_sources": raw.frames.numel(),
                          "tables": tables, "erase_tables_and_noise": erase, "finished_fp32": fp32,
                          "ratio": round((raw.frames.numel() + tables + erase) / fp32, 3)}), flush=True)


def edge(dev, steps, rounds, n=16, hw=(375, 500)):
    from jepa_amd.engine.input import ImagePrefetcher
    from jepa_amd.src.models import vision_transformer as vit
    raw = host_batch(n, hw, True, pinned=True)
    labels = torch.zeros(n, dtype=torch.int64)
    fp32 = torch.randn(n, 3, S, S).pin_memory()
    for name, frames in (("vit_large video encoder, 16 frames, fed still images", 16), ("vit_large image model", 1)):
        torch.manual_seed(0)
        kw = dict(num_frames=frames, tubelet_size=2, uniform_power=True) if frames > 1 else {}
        enc = vit.vit_large(img_size=S, patch_size=16, **kw).to(dev).eval()
        for p in enc.parameters():
            p.requires_grad = False
        rows = []
        for r in range(rounds):
            row = {}
            for arm in (("uint8", "fp32") if r % 2 == 0 else ("fp32", "uint8")):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.no_grad():
                    if arm == "uint8":
                        pf = ImagePrefetcher([(raw, labels)] * (steps + 1), dev, timing=True)
                        for k, (imgs, _) in enumerate(pf):
                            if k == 1:
                                e0.record()
                            enc(imgs)
                    else:               # the finished fp32 batch, copied in front of the forward as the evals do with `synthetic`
                        for k in range(steps + 1):
                            if k == 1:
                                e0.record()
                            enc(fp32.to(dev, non_blocking=True))
                e1.record()
                torch.cuda.synchronize()
                row[arm] = {"iteration_ms": round(e0.elapsed_time(e1) / steps, 3)}
                if arm == "uint8":
                    waits = [max(0.0, a.elapsed_time(b)) for a, b in pf.edge_events]
                    row[arm].update(edge_wait_ms_first=round(waits[0], 3), edge_wait_ms_rest_mean=round(statistics.mean(waits[1:]), 4),
                                    edge_wait_ms_rest_max=round(max(waits[1:]), 4))
            rows.append(row)
        print(json.dumps({"what": "input-edge wait inside a loop of frozen forwards, interleaved arms", "encoder": name, "batch": n,
                          "source": list(hw), "steps": steps, "rounds": rows}), flush=True)
        del enc
        torch.cuda.empty_cache()


def autoaug_kernels(dev, launches, rounds):
    from jepa_amd.evals.image_classification_frozen.transforms import fill_colour
    from jepa_amd.hip import ops
    for n in (16, 256):
        raw = host_batch(n, (375, 500), True, two_layer_plans=True)
        frames, desc, geom = raw.frames.to(dev), raw.desc.to(dev), raw.geom.to(dev)
        caps = raw.capacities()
        ws = torch.empty(ops.ImageResample.ws_bytes(n, S, *caps), dtype=torch.uint8, device=dev)
        u8 = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev)
        desc1 = raw.resampled_tables()[0]
        flips, desc1 = desc1[:, 3].tolist(), desc1.to(dev)
        live = (raw.aug_ops != 0).any(0)
        aug_ops, aug_args = raw.aug_ops[:, live].contiguous().to(dev), raw.aug_args[:, live].contiguous().to(dev)
        aug_ws = torch.empty(ops.clip_randaug_ws_bytes(u8.numel(), n, 1), dtype=torch.uint8, device=dev)
        fill = fill_colour(raw.mean)
        rows_bf16 = torch.empty((n * S, S * 3 // 2), dtype=torch.bfloat16, device=dev)      # the bytes of u8 as bf16 rows
        rows_dst = torch.empty_like(rows_bf16)
        M, D = rows_bf16.shape
        arms = {
            "image_resample": lambda: ops.ImageResample.run(frames, desc, geom, S, raw.filter, *caps, out=u8, ws=ws),
            "image_hflip": lambda: ops.image_hflip(u8, desc1, flips),
            "clip_randaug_fill": lambda: ops.clip_randaug(u8.view(-1), desc1, 1, aug_ops, aug_args, ws=aug_ws, fill=fill),
            "copy_rows_same_bytes": lambda: ops.copy_rows(rows_bf16, rows_dst, 1, M, 0, M, 0, M, D),
        }
        names, out_rows = list(arms), []
        for r in range(rounds):
            row = {k: _median_us(arms[k], launches) for k in (names if r % 2 == 0 else names[::-1])}
            out_rows.append({k: row[k] for k in names})
        print(json.dumps({"what": "auto_augment kernels, us per batch, median over the launches of a round; every image flipped, "
                          "two-layer plans of the 'original' policy", "batch": n, "S": S, "bytes": u8.numel(),
                          "layers": int(live.sum()), "launches": launches, "rounds": out_rows}), flush=True)


def autoaug_edge(dev, steps, rounds, n=16, hw=(375, 500)):
    """edge()'s loop on the ViT-L video encoder fed still images, with `data.auto_augment` on (every image a two-layer plan) and
    off (the batch of edge(): the launches of the parent commit)."""
    from jepa_amd.engine.input import ImagePrefetcher
    from jepa_amd.src.models import vision_transformer as vit
    arms = {"off": host_batch(n, hw, True, pinned=True), "on": host_batch(n, hw, True, pinned=True, two_layer_plans=True)}
    labels = torch.zeros(n, dtype=torch.int64)
    torch.manual_seed(0)
    enc = vit.vit_large(img_size=S, patch_size=16, num_frames=16, tubelet_size=2, uniform_power=True).to(dev).eval()
    for p in enc.parameters():
        p.requires_grad = False
    rows = []
    for r in range(rounds):
        row = {}
        for arm in (("off", "on") if r % 2 == 0 else ("on", "off")):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.no_grad():
                pf = ImagePrefetcher([(arms[arm], labels)] * (steps + 1), dev, timing=True)
                for k, (imgs, _) in enumerate(pf):
                    if k == 1:
                        e0.record()
                    enc(imgs)
            e1.record()
            torch.cuda.synchronize()
            waits = [max(0.0, a.elapsed_time(b)) for a, b in pf.edge_events]
            row[arm] = {"iteration_ms": round(e0.elapsed_time(e1) / steps, 3), "edge_wait_ms_first": round(waits[0], 3),
                        "edge_wait_ms_rest_mean": round(statistics.mean(waits[1:]), 4), "edge_wait_ms_rest_max": round(max(waits[1:]), 4)}
        rows.append(row)
    print(json.dumps({"what": "input-edge wait inside a loop of frozen forwards, data.auto_augment on / off interleaved",
                      "encoder": "vit_large video encoder, 16 frames, fed still images", "batch": n, "source": list(hw), "steps": steps,
                      "rounds": rows}), flush=True)


def autoaug_pil_one_core(n=16, reps=3):
    """The plans of autoaug_kernels through PIL on one core: flip, then the two operations, from the tables."""
    from PIL import Image, ImageEnhance, ImageOps
    from jepa_amd.evals.image_classification_frozen.transforms import fill_colour
    torch.set_num_threads(1)
    raw = host_batch(n, (375, 500), True, two_layer_plans=True)
    fill = fill_colour(raw.mean)
    g = torch.Generator().manual_seed(3)
    imgs = [Image.fromarray(torch.randint(0, 256, (S, S, 3), generator=g, dtype=torch.uint8).numpy()) for _ in range(n)]
    enhance = {8: ImageEnhance.Color, 9: ImageEnhance.Contrast, 10: ImageEnhance.Brightness, 11: ImageEnhance.Sharpness}
    table = {1: ImageOps.autocontrast, 2: ImageOps.equalize, 3: ImageOps.invert}

    def run(im, ops_k, args_k):
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
        for code, a in zip(ops_k, args_k):
            if code in table:
                im = table[code](im)
            elif code in (4, 12):
                im = im.transform(im.size, Image.AFFINE, tuple(a), resample=Image.BICUBIC, fillcolor=fill)
            elif code == 5:
                im = ImageOps.posterize(im, int(a[0]))
            elif code == 6:
                im = ImageOps.solarize(im, int(a[0]))
            elif code in enhance:
                im = enhance[code](im).enhance(a[0])
        im.load()

    plans = list(zip(raw.aug_ops.tolist(), raw.aug_args.tolist()))
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        for im, (o, a) in zip(imgs, plans):
            run(im, o, a)
        best = min(best, time.perf_counter() - t0)
    print(json.dumps({"what": "PIL on one core: flip + two-layer 'original' plans on 224 x 224, best of the repetitions", "batch": n,
                      "ms_per_image": round(1e3 * best / n, 3), "images_per_s_per_core": round(n / best, 1)}), flush=True)


def pil_one_core(reps=3):
    from PIL import Image
    torch.set_num_threads(1)
    for n, hw in ((16, (375, 500)), (4, (3000, 4000))):
        for form in ("train", "val"):
            raw = host_batch(n, hw, form == "train")
            imgs = [Image.fromarray(raw.image(b).numpy()) for b in range(n)]
            best = float("inf")
            for _ in range(reps):
                t0 = time.perf_counter()
                for im, (i, j, h, w, OH, OW, wy, wx) in zip(imgs, raw.geom.tolist()):
                    out = im.crop((j, i, j + w, i + h)).resize((OW, OH), Image.BICUBIC if form == "train" else Image.BILINEAR)
                    out.crop((wx, wy, wx + S, wy + S)).load()
                best = min(best, time.perf_counter() - t0)
            print(json.dumps({"what": "PIL on one core, crop + resize (+ centre crop), best of the repetitions", "form": form, "batch": n,
                              "source": list(hw), "ms_per_image": round(1e3 * best / n, 3),
                              "images_per_s_per_core": round(n / best, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--no-edge", action="store_true")
    ap.add_argument("--pil", action="store_true", help="CPU only: the same resizes through PIL on one core")
    ap.add_argument("--auto-augment", action="store_true", help="the data.auto_augment path: kernels and the input-edge wait")
    args = ap.parse_args()
    if args.pil:
        return autoaug_pil_one_core() if args.auto_augment else pil_one_core()
    dev = torch.device("cuda")
    if args.auto_augment:
        autoaug_kernels(dev, args.launches, args.rounds)
        if not args.no_edge:
            autoaug_edge(dev, args.steps, args.rounds)
        return
    kernels(dev, args.launches, args.rounds)
    h2d_bytes()
    if not args.no_edge:
        edge(dev, args.steps, args.rounds)


if __name__ == "__main__":
    main()
