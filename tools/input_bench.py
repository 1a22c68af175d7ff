#!/usr/bin/env python
"""Measure the device-side clip augmentation (vj_clip_transform) and the input edge that carries it.

    python tools/input_bench.py [--steps 12] [--no-step-loop]

Settings: B = 24, T = 16, S = 224 (the ViT-L/16 recipe), sources 240x320, 256x340 and 720x1280, motion shift off and on.
1. kernel time: HIP events around single launches after warm-up, median of >= 20; bytes moved (the source bytes inside the crop
   boxes, read once, + the fp32 output) per second against the 6.29 TB/s copy ceiling of DESIGN section 4.
2. H2D bytes per step of the uint8 path (frames + tables) and of the fp32 path (the clip tensor).
3. the time the compute stream waits in `prefetcher.next()` for `ready` in a loop of real ViT-L train steps, for both paths
   (events on the compute stream before and after next(); batches start in pinned host memory).
Prints one JSON line per measurement; nothing here is a gate.

    python tools/input_bench.py --randaug [--launches 30] [--steps 12] [--rounds 3]
    python tools/input_bench.py --randaug-pil          (CPU only, needs PIL)

--randaug measures the device-side RandAugment (vj_clip_randaug) on K400-shaped batches (16 frames of 256x340, B = 4 and 24):
4. kernel time per layer class -- every clip of the batch with the same operation in two layers (two launches per layer, no copy
   back), halved -- and of whole plans drawn by RandAugmentDraw('rand-m7-n4-mstd0.5-inc1') (live layers only, copy back included);
5. the wait of the compute stream on the input edge (EvalPrefetcher, timing events) inside a loop of frozen ViT-L forwards over
   B = 4 training clips, with and without the plans, the two arms interleaved round by round.
--randaug-pil times, for scale, the same plans carried out through PIL on one CPU core, per clip.

    python tools/input_bench.py --resize [--launches 30] [--steps 4] [--rounds 2]
    python tools/input_bench.py --resize-host          (CPU only, needs PIL)

--resize measures the validation resize of real frames (vj_clip_resample) on a K400 16x8x3 validation batch (batch 4, 8 segments of
16 frames of 256x340, resized to 224x297, 3 views):
6. kernel time of vj_clip_resample over the batch's 32 clips, and beside it vj_image_resample computing the same three 224x224
   windows of every frame -- the only way to express this without the clip kernel;
7. the wait of the compute stream on the input edge inside a loop of frozen ViT-L forwards over such batches, with sources that
   need the resize and with sources that arrive at 224x297, the two arms interleaved round by round.
--resize-host times Pillow's resize of one clip on one CPU core, and the frames per second FrameFolderVideoDataset reads per worker
from JPEG folders and from .npy arrays.
"""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from jepa_amd.app.vjepa.transforms import make_transforms  # noqa: E402
from jepa_amd.hip import ops  # noqa: E402

B, T, S = 24, 16, 224
SOURCES = ((240, 320), (256, 340), (720, 1280))
COPY_CEILING = 6.29e12   # bytes/s, DESIGN section 4


def raw_batch(hw, shift, seed, pinned=False):
    random.seed(seed)
    np.random.seed(seed)
    g = torch.Generator().manual_seed(seed)
    vt = make_transforms(crop_size=S, motion_shift=shift)
    base = torch.randint(0, 256, (T, hw[0], hw[1], 3), generator=g, dtype=torch.uint8)
    batch = torch.utils.data.default_collate([vt(base.roll(b, dims=1)) for b in range(B)])
    return batch.pin_memory() if pinned else batch


def kernel_times(dev, launches):
    for hw in SOURCES:
        for shift in (False, True):
            batch = raw_batch(hw, shift, seed=hw[0] + int(shift))
            frames, desc, boxes = batch.to(dev)
            out = torch.empty(B, 3, T, S, S, dtype=torch.float32, device=dev)
            for _ in range(5):
                ops.clip_transform(frames, desc, boxes, S, batch.mean, batch.std, out=out)
            torch.cuda.synchronize()
            ms = []
            for _ in range(launches):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.clip_transform(frames, desc, boxes, S, batch.mean, batch.std, out=out)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            med = statistics.median(ms)
            b64 = batch.boxes.to(torch.int64)
            src = int((b64[..., 2] * b64[..., 3]).sum()) * 3
            moved = src + out.numel() * 4
            print(json.dumps({"what": "vj_clip_transform", "source": list(hw), "motion_shift": shift, "launches": launches,
                              "median_us": round(1e3 * med, 2), "min_us": round(1e3 * min(ms), 2), "max_us": round(1e3 * max(ms), 2),
                              "bytes_moved": moved, "source_bytes_in_boxes": src, "TB_per_s": round(moved / (med * 1e-3) / 1e12, 3),
                              "frac_of_copy_ceiling": round(moved / (med * 1e-3) / COPY_CEILING, 3),
                              "h2d_bytes_uint8_path": int(batch.frames.numel() + batch.desc.numel() * 8 + batch.boxes.numel() * 4),
                              "h2d_bytes_fp32_path": out.numel() * 4}), flush=True)


def step_loop(dev, steps):
    import bench
    from jepa_amd.engine import dp
    from jepa_amd.engine.input import DevicePrefetcher
    wl = dict(bench.WORKLOADS["vitl16"])
    trainer, sched, wd_sched = bench.build(wl, dev, 1)
    dp.broadcast_parameters(trainer.arena, trainer.tarena)
    fp32 = bench.make_inputs(dict(wl, distinct_batches=4), 4, 0, dev, host=True)
    masks = [(me, mp) for _, me, mp in fp32]
    paths = {"fp32": [([c], me, mp) for c, me, mp in fp32]}
    for hw in SOURCES:
        paths[f"uint8 {hw[0]}x{hw[1]}"] = [([raw_batch(hw, k % 2 == 1, seed=k, pinned=True)], *masks[k]) for k in range(2)]
    ema0, ema1 = bench.HP["ema"]
    i = [0]
    for name, hb in paths.items():
        cnt = [0]

        def fetch():
            item = hb[cnt[0] % len(hb)]
            cnt[0] += 1
            return item
        pf = DevicePrefetcher(fetch, dev)
        waits, evs = [], []
        for k in range(3 + steps):
            if k == 3:
                torch.cuda.synchronize()
                b0, e_first = pf.bytes_copied, torch.cuda.Event(enable_timing=True)
                e_first.record()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            clips, me, mp = pf.next()
            b.record()
            if k >= 3:
                evs.append((a, b))
            trainer.train_step(clips, me, mp, lr=sched.step(), wd=wd_sched.step(), ema=ema0 + (ema1 - ema0) * 1e-4 * i[0])
            i[0] += 1
        e_last = torch.cuda.Event(enable_timing=True)
        e_last.record()
        torch.cuda.synchronize()
        waits = [a.elapsed_time(b) for a, b in evs]
        print(json.dumps({"what": "prefetcher.next() wait on ready inside a ViT-L B=24 train-step loop", "path": name, "steps": steps,
                          "median_wait_ms": round(statistics.median(waits), 3), "max_wait_ms": round(max(waits), 3),
                          "ms_per_step": round(e_first.elapsed_time(e_last) / steps, 3),
                          "h2d_bytes_per_step": int((pf.bytes_copied - b0) / steps)}), flush=True)


RA_T, RA_HW = 16, (256, 340)
RA_CLASSES = (("copy through (no operation)", 0, 0.0), ("table (Invert)", 3, 0.0), ("table + histogram (AutoContrast)", 1, 0.0),
              ("table + histogram (Equalize)", 2, 0.0), ("table + luma sum (Contrast)", 9, 1.63), ("Color", 8, 1.63),
              ("Sharpness", 11, 1.63), ("affine (Rotate)", 4, 21.0))


def _drawn_plans(n, seed=0):
    from jepa_amd.app.vjepa.randaugment import RandAugmentDraw
    random.seed(seed)
    np.random.seed(seed)
    draw = RandAugmentDraw()
    plans = [draw.draw(*RA_HW) for _ in range(n)]
    return np.stack([p[0] for p in plans]), np.stack([p[1] for p in plans])


def _timed_us(fn, launches):
    for _ in range(3):
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
    return us


def randaug_kernel_times(dev, launches):
    from jepa_amd.app.vjepa.randaugment import rotation_coefficients
    H, W = RA_HW
    clip_bytes = RA_T * H * W * 3
    assert clip_bytes % 16 == 0
    g = torch.Generator().manual_seed(0)
    for nb in (4, 24):
        frames = torch.randint(0, 256, (nb * clip_bytes,), generator=g, dtype=torch.uint8).to(dev)
        keep = frames.clone()
        desc = torch.tensor([[b * clip_bytes, H, W, 0] for b in range(nb)], dtype=torch.int64, device=dev)
        ws = torch.empty(ops.clip_randaug_ws_bytes(frames.numel(), nb, RA_T), dtype=torch.uint8, device=dev)
        for name, code, arg in RA_CLASSES:
            a = np.zeros((nb, 2, 6))
            a[:, :, 0] = arg
            if code == 4:
                a[:] = rotation_coefficients(arg, H, W)
            o = torch.full((nb, 2), code, dtype=torch.int32, device=dev)
            a = torch.from_numpy(a).to(dev)
            frames.copy_(keep)
            us = _timed_us(lambda: ops.clip_randaug(frames, desc, RA_T, o, a, ws=ws), launches)
            med = statistics.median(us) / 2
            print(json.dumps({"what": "vj_clip_randaug, one layer (table + apply launches)", "class": name, "batch": nb, "frames": RA_T,
                              "source": list(RA_HW), "launches": launches, "median_us_per_layer": round(med, 1),
                              "min_us_per_layer": round(min(us) / 2, 1), "max_us_per_layer": round(max(us) / 2, 1),
                              "TB_per_s_read_plus_written": round(2 * frames.numel() / (med * 1e-6) / 1e12, 3)}), flush=True)
        po, pa = _drawn_plans(nb)
        live = (po != 0).any(0)
        o, a = torch.from_numpy(po[:, live].copy()).to(dev), torch.from_numpy(pa[:, live].copy()).to(dev)
        frames.copy_(keep)
        us = _timed_us(lambda: ops.clip_randaug(frames, desc, RA_T, o, a, ws=ws), launches)
        print(json.dumps({"what": "vj_clip_randaug, drawn plans rand-m7-n4-mstd0.5-inc1 (copy back included when the layer count is odd)",
                          "batch": nb, "live_layers": int(live.sum()), "applied_operations": int((po != 0).sum()),
                          "median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}),
              flush=True)


def randaug_edge(dev, steps, rounds, nb=4):
    from jepa_amd.app.vjepa.randaugment import RandAugmentDraw
    from jepa_amd.engine.input import EvalPrefetcher
    from jepa_amd.evals.video_classification_frozen.utils import ClipAggregation
    from jepa_amd.evals.video_classification_frozen.utils import make_transforms as eval_transforms
    from jepa_amd.src.models import vision_transformer as vit
    torch.manual_seed(0)
    enc = ClipAggregation(vit.vit_large(img_size=S, patch_size=16, num_frames=RA_T, tubelet_size=2, uniform_power=True),
                          tubelet_size=2, attend_across_segments=True).to(dev).eval()
    for p in enc.parameters():
        p.requires_grad = False
    g = torch.Generator().manual_seed(1)
    src = [torch.randint(0, 256, (RA_T,) + RA_HW + (3,), generator=g, dtype=torch.uint8) for _ in range(nb)]

    def host_batch(aug):
        random.seed(2)
        np.random.seed(2)
        torch.manual_seed(2)
        tf = eval_transforms(training=True, random_horizontal_flip=False, random_resize_aspect_ratio=(0.75, 4 / 3),
                             random_resize_scale=(0.08, 1.0), reprob=0.25, crop_size=S)
        if aug:
            tf.rand_augment = RandAugmentDraw()
        raw = torch.utils.data.default_collate([tf(f) for f in src]).pin_memory()
        return ([raw], torch.zeros(nb, dtype=torch.int64), [torch.arange(RA_T)])

    arms = {"plain": host_batch(False), "randaug": host_batch(True)}
    rows = []
    for r in range(rounds):
        row = {}
        for arm in (("plain", "randaug") if r % 2 == 0 else ("randaug", "plain")):
            pf = EvalPrefetcher([arms[arm]] * (steps + 1), dev, timing=True)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.no_grad():
                for k, (clips, _, idx) in enumerate(pf):
                    if k == 1:
                        e0.record()
                    enc(clips, idx)
            e1.record()
            torch.cuda.synchronize()
            waits = [max(0.0, a.elapsed_time(b)) for a, b in pf.edge_events]
            row[arm] = dict(edge_wait_ms_first=round(waits[0], 3), edge_wait_ms_rest_mean=round(statistics.mean(waits[1:]), 4),
                            edge_wait_ms_rest_max=round(max(waits[1:]), 4), iteration_ms=round(e0.elapsed_time(e1) / steps, 3))
        rows.append(row)
    raw = arms["randaug"][0][0]
    print(json.dumps({"what": "input-edge wait inside a loop of frozen ViT-L forwards, EvalPrefetcher, interleaved arms", "batch": nb,
                      "frames": RA_T, "source": list(RA_HW), "steps": steps, "live_layers": int((raw.aug_ops != 0).any(0).sum()),
                      "applied_operations": int((raw.aug_ops != 0).sum()), "rounds": rows}), flush=True)


def randaug_pil(clips=8):
    """The plans of RandAugmentDraw carried out by PIL, frame by frame, on one CPU core: seconds per clip of 16 frames of 256x340."""
    import time

    from PIL import Image, ImageEnhance, ImageOps
    torch.set_num_threads(1)
    H, W = RA_HW
    po, pa = _drawn_plans(clips)
    g = np.random.RandomState(0)
    fill = dict(resample=Image.BICUBIC, fillcolor=(128, 128, 128))
    enhance = {8: ImageEnhance.Color, 9: ImageEnhance.Contrast, 10: ImageEnhance.Brightness, 11: ImageEnhance.Sharpness}

    def one(img, code, a):
        if code in (4, 12, 13, 14, 15):
            return img.transform(img.size, Image.AFFINE, tuple(a), **fill)
        if code in enhance:
            return enhance[code](img).enhance(a[0])
        if code == 7:
            return img.point([min(255, i + int(a[0])) if i < 128 else i for i in range(256)] * 3)
        return {1: ImageOps.autocontrast, 2: ImageOps.equalize, 3: ImageOps.invert, 5: lambda i: ImageOps.posterize(i, int(a[0])),
                6: lambda i: ImageOps.solarize(i, int(a[0]))}[code](img)

    secs = []
    for c in range(clips):
        frames = g.randint(0, 256, (RA_T, H, W, 3)).astype(np.uint8)
        t0 = time.perf_counter()
        imgs = [Image.fromarray(f) for f in frames]
        for code, a in zip(po[c], pa[c]):
            if code:
                imgs = [one(i, int(code), a) for i in imgs]
        np.stack([np.asarray(i) for i in imgs])
        secs.append(time.perf_counter() - t0)
    print(json.dumps({"what": "the same plans through PIL on one CPU core (uint8 in, uint8 out; the reference's ToTensor comes on top)",
                      "clips": clips, "frames": RA_T, "source": list(RA_HW), "applied_operations_per_clip": (po != 0).sum(1).tolist(),
                      "ms_per_clip_mean": round(1e3 * statistics.mean(secs), 1), "ms_per_clip_max": round(1e3 * max(secs), 1),
                      "ms_per_applied_operation": round(1e3 * sum(secs) / max(1, int((po != 0).sum())), 1)}), flush=True)


RS_B, RS_SEGMENTS, RS_VIEWS, RS_SRC, RS_OUT = 4, 8, 3, (256, 340), (224, 297)      # a K400 16x8x3 validation batch


def _k400_segments(native, nb=RS_B, segments=RS_SEGMENTS):
    """`segments` RawClipBatches of nb clips of 16 frames through EvalVideoTransform(3, 224): 256x340 sources that the device
    resizes to 224x297, or (native) 224x297 sources that need nothing."""
    from jepa_amd.evals.video_classification_frozen.utils import EvalVideoTransform
    tf = EvalVideoTransform(num_views_per_clip=RS_VIEWS, short_side_size=S)
    tf.device_resize = True
    g = torch.Generator().manual_seed(3)
    hw = RS_OUT if native else RS_SRC
    return [torch.utils.data.default_collate([tf(torch.randint(0, 256, (RA_T,) + hw + (3,), generator=g, dtype=torch.uint8))
                                              for _ in range(nb)]).pin_memory() for _ in range(segments)]


def resize_kernel_times(dev, launches):
    from jepa_amd.app.vjepa.transforms import RawClipBatch
    from jepa_amd.evals.image_classification_frozen.transforms import axis_span, axis_taps
    seg = _k400_segments(False, nb=RS_B * RS_SEGMENTS, segments=1)[0]          # all 32 clips of the batch in one launch
    assert isinstance(seg, RawClipBatch) and seg.resized
    nb = len(seg) // RS_VIEWS
    frames, desc = seg.frames.to(dev), seg.desc[:nb].to(dev)
    rgeom, desc_out, nbytes, caps = seg.resample_plan()
    out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ws = torch.empty(ops.clip_resample.ws_bytes(nb, RA_T, caps), dtype=torch.uint8, device=dev)
    rg, do = rgeom.to(dev), desc_out[:nb].to(dev)
    us = _timed_us(lambda: ops.clip_resample(frames, desc, rg, RA_T, ops.BILINEAR, caps, out, do, ws=ws), launches)
    med = statistics.median(us)
    moved = frames.numel() + nbytes
    print(json.dumps({"what": "vj_clip_resample, one launch for the batch", "clips": nb, "frames": RA_T, "source": list(RS_SRC),
                      "resized": list(RS_OUT), "launches": launches, "median_us": round(med, 1), "min_us": round(min(us), 1),
                      "max_us": round(max(us), 1), "source_plus_output_bytes": moved,
                      "TB_per_s": round(moved / (med * 1e-6) / 1e12, 3), "workspace_bytes": ws.numel()}), flush=True)
    # what the parent could express: every frame an image, every view an S x S window of its 224x297 resize (three launches)
    H, W = RS_SRC
    step = (max(RS_OUT) - S) // (RS_VIEWS - 1)
    n = nb * RA_T
    idesc = torch.tensor([[int(seg.desc[b, 0]) + t * H * W * 3, H, W, 0] for b in range(nb) for t in range(RA_T)], dtype=torch.int64)
    assert bool((idesc[:, 0] % 16 == 0).all())
    tx, ty = axis_taps(W, RS_OUT[1], ops.BILINEAR), axis_taps(H, RS_OUT[0], ops.BILINEAR)
    rows = axis_span(H, RS_OUT[0], ops.BILINEAR, 0, S)[1]
    idesc, u8 = idesc.to(dev), torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev)
    geoms = [torch.tensor([[0, 0, H, W, RS_OUT[0], RS_OUT[1], 0, v * step]] * n, dtype=torch.int32, device=dev) for v in range(RS_VIEWS)]
    iws = torch.empty(ops.ImageResample.ws_bytes(n, S, tx, ty, rows), dtype=torch.uint8, device=dev)

    def windows():
        for geom in geoms:
            ops.ImageResample.run(frames, idesc, geom, S, ops.BILINEAR, tx, ty, rows, out=u8, ws=iws)
    us = _timed_us(windows, launches)
    print(json.dumps({"what": "vj_image_resample, the same three 224x224 windows of every frame (three launches of clips x frames images)",
                      "images_per_launch": n, "launches": launches, "median_us": round(statistics.median(us), 1),
                      "min_us": round(min(us), 1), "max_us": round(max(us), 1)}), flush=True)


def resize_edge(dev, steps, rounds):
    from jepa_amd.engine.input import EvalPrefetcher
    from jepa_amd.evals.video_classification_frozen.utils import ClipAggregation
    from jepa_amd.src.models import vision_transformer as vit
    torch.manual_seed(0)
    enc = ClipAggregation(vit.vit_large(img_size=S, patch_size=16, num_frames=RA_T, tubelet_size=2, uniform_power=True),
                          tubelet_size=2, attend_across_segments=True).to(dev).eval()
    for p in enc.parameters():
        p.requires_grad = False
    arms = {}
    for arm, native in (("native 224x297 (no resize)", True), ("256x340, resized on the device", False)):
        segs = _k400_segments(native)
        arms[arm] = (segs, torch.zeros(RS_B, dtype=torch.int64), [torch.arange(RA_T) for _ in segs])
    rows = []
    for r in range(rounds):
        row = {}
        for arm in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
            pf = EvalPrefetcher([arms[arm]] * (steps + 1), dev, timing=True)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.no_grad():
                for k, (clips, _, idx) in enumerate(pf):
                    if k == 1:
                        e0.record()
                    enc(clips, idx)
            e1.record()
            torch.cuda.synchronize()
            waits = [max(0.0, a.elapsed_time(b)) for a, b in pf.edge_events]
            row[arm] = dict(edge_wait_ms_first=round(waits[0], 3), edge_wait_ms_rest_mean=round(statistics.mean(waits[1:]), 4),
                            edge_wait_ms_rest_max=round(max(waits[1:]), 4), iteration_ms=round(e0.elapsed_time(e1) / steps, 3),
                            h2d_bytes_per_batch=int(pf.bytes_copied / (steps + 1)))
        rows.append(row)
    print(json.dumps({"what": "input-edge wait inside a loop of frozen ViT-L forwards over K400 16x8x3 validation batches, EvalPrefetcher, "
                              "interleaved arms", "batch": RS_B, "segments": RS_SEGMENTS, "views": RS_VIEWS, "frames": RA_T,
                      "steps": steps, "rounds": rows}), flush=True)


def resize_host(videos=2, length=160):
    """CPU only: Pillow's resize of a clip on one core, and the frames per second one worker reads from JPEG folders and .npy."""
    import tempfile
    import time

    from PIL import Image

    from jepa_amd.src.datasets.frame_folder import FrameFolderVideoDataset
    torch.set_num_threads(1)
    g = np.random.RandomState(0)
    H, W = RS_SRC
    clip = g.randint(0, 256, (RA_T, H, W, 3)).astype(np.uint8)
    secs = []
    for _ in range(5):
        t0 = time.perf_counter()
        np.stack([np.asarray(Image.fromarray(f).resize((RS_OUT[1], RS_OUT[0]), Image.BILINEAR)) for f in clip])
        secs.append(time.perf_counter() - t0)
    print(json.dumps({"what": "Pillow Image.resize(BILINEAR) of one clip on one CPU core", "frames": RA_T, "source": list(RS_SRC),
                      "resized": list(RS_OUT), "ms_per_clip_median": round(1e3 * statistics.median(secs), 2),
                      "ms_per_k400_item_of_8_segments": round(8e3 * statistics.median(secs), 1)}), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        y, x = np.mgrid[0:H, 0:W]
        for v in range(videos):
            os.makedirs(os.path.join(tmp, f"jpg{v}"))
            video = np.stack([np.stack([(y + 3 * t + 40 * v) % 256, (x + 5 * t) % 256, (x + y + t) % 256], -1)
                              for t in range(length)]).astype(np.uint8)
            for t, f in enumerate(video):
                Image.fromarray(f).save(os.path.join(tmp, f"jpg{v}", f"{t:06d}.jpg"), quality=90)
            np.save(os.path.join(tmp, f"npy{v}.npy"), video)
        for kind in ("jpg", "npy"):
            index = os.path.join(tmp, f"{kind}.csv")
            with open(index, "w") as f:
                f.writelines(f"{kind}{v}{'.npy' if kind == 'npy' else ''} 0\n" for v in range(videos))
            ds = FrameFolderVideoDataset([index], frames_per_clip=RA_T, frame_step=4, num_clips=RS_SEGMENTS, allow_clip_overlap=True)
            np.random.seed(0)
            ds[0]
            t0, frames = time.perf_counter(), 0
            for k in range(6):
                clips, _, _ = ds[k % videos]
                frames += sum(len(c) for c in clips)
            dt = time.perf_counter() - t0
            print(json.dumps({"what": "FrameFolderVideoDataset items on one worker (8 clips of 16 frames, no transform)",
                              "storage": "JPEG folder (quality 90)" if kind == "jpg" else ".npy (memory-mapped)",
                              "source": list(RS_SRC), "frames_per_s": round(frames / dt, 1),
                              "ms_per_item": round(1e3 * dt / 6, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--no-step-loop", action="store_true")
    ap.add_argument("--randaug", action="store_true", help="the device-side RandAugment: kernel times and the input-edge wait")
    ap.add_argument("--randaug-pil", action="store_true", help="CPU only: the same plans through PIL, for scale")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--resize", action="store_true", help="the device-side validation resize: kernel times and the input-edge wait")
    ap.add_argument("--resize-host", action="store_true", help="CPU only: Pillow's resize and the frame-folder dataset's read rate")
    args = ap.parse_args()
    if args.randaug_pil:
        return randaug_pil()
    if args.resize_host:
        return resize_host()
    if args.resize:
        assert torch.cuda.is_available(), "needs an MI355X"
        dev = torch.device("cuda", 0)
        resize_kernel_times(dev, max(20, args.launches))
        if not args.no_step_loop:
            resize_edge(dev, args.steps, args.rounds)
        return
    if args.randaug:
        assert torch.cuda.is_available(), "needs an MI355X"
        dev = torch.device("cuda", 0)
        randaug_kernel_times(dev, max(20, args.launches))
        if not args.no_step_loop:
            randaug_edge(dev, args.steps, args.rounds)
        return
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    kernel_times(dev, max(20, args.launches))
    if not args.no_step_loop:
        step_loop(dev, args.steps)


if __name__ == "__main__":
    main()
