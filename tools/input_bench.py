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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--no-step-loop", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    kernel_times(dev, max(20, args.launches))
    if not args.no_step_loop:
        step_loop(dev, args.steps)


if __name__ == "__main__":
    main()
