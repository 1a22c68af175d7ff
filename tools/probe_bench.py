#!/usr/bin/env python
"""Attentive probe on frozen features (row f4 widened): time of one training step (forward + backward of AttentiveClassifier, no
optimizer) and of the cross-attention kernels alone, at the reference's eval shape (ViT-L tokens of one 16x224x224 clip per sample).
--tokens N [N ...] times ViT-L (head_dim 64) and ViT-H (head_dim 80) widths at those key counts instead, e.g. the probes of the K400
16x8x3 evals (8 segments attended across: 12 544 keys at 224, 36 864 at 384) or both sides of the single-workgroup limits
(forward 38 264, backward 19 132 keys), where the _ws entry points switch to the split-key kernels.
python tools/probe_bench.py [--batch 16] [--reps 20] [--tokens 12544 36864]
--bank P [P ...] compares instead, at each of those shapes, one step of an AttentiveClassifierBank of P probes (arm A) with P
sequential lone-probe steps on the same features (arm B); the arms take turns for --rounds rounds in this one process.  Also
printed: the bank step at 64 keys (the per-probe algebra and the norm2 / MLP / linear tail, which do not depend on N) and the peak
memory of each arm.
python tools/probe_bench.py --batch 4 --tokens 12544 --bank 1 5 20"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jepa_amd.hip import ops  # noqa: E402
from jepa_amd.hip.lib import load_library  # noqa: E402
from jepa_amd.src.models.attentive_pooler import AttentiveClassifier, AttentiveClassifierBank  # noqa: E402


def timeit(fn, reps):
    for _ in range(3):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def bank_bench(a, shapes):
    dev = "cuda"
    for tag, N, D, H in shapes:
        B = a.batch
        x = torch.randn(B, N, D, device=dev).to(torch.bfloat16)
        x_small = x[:, :64].contiguous()
        y = torch.randint(0, 400, (B,), device=dev)
        for P in a.bank:
            torch.manual_seed(0)
            bank = AttentiveClassifierBank(D, H, 400, P).to(dev)

            def bank_step(feat=x):
                for p in bank.parameters():
                    p.grad = None
                logits = bank(feat)
                sum(torch.nn.functional.cross_entropy(logits[p], y) for p in range(P)).backward()

            def lone_steps():
                for m in bank.probes:
                    for p in m.parameters():
                        p.grad = None
                    torch.nn.functional.cross_entropy(m(x), y).backward()

            peak = {}
            for name, fn in (("bank", bank_step), ("lone", lone_steps)):
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                fn()
                torch.cuda.synchronize()
                peak[name] = torch.cuda.max_memory_allocated() / 2 ** 20
            wins = 0
            for r in range(a.rounds):
                ua, ub = timeit(bank_step, a.reps), timeit(lone_steps, a.reps)
                wins += ua < ub
                print(f"{tag} B={B} P={P} round {r}: bank {ua / 1e3:8.3f} ms | {P} lone steps {ub / 1e3:8.3f} ms | x{ub / ua:5.2f}")
            tail = timeit(lambda: bank_step(x_small), a.reps)
            print(f"{tag} B={B} P={P}: bank faster in {wins}/{a.rounds} rounds; step at 64 keys (per-probe algebra + tail) "
                  f"{tail / 1e3:.3f} ms; peak memory bank {peak['bank']:.0f} MiB, lone {peak['lone']:.0f} MiB")
            del bank


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tokens", type=int, nargs="*", default=None, help="probe key counts N (default: one clip of ViT-L 224 / ViT-H 384)")
    ap.add_argument("--bank", type=int, nargs="*", default=None, help="probe counts P: bank of P against P lone steps")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda"
    lib = load_library()
    shapes = (("ViT-L 16x224", 1568, 1024, 16), ("ViT-H 16x384", 4608, 1280, 16)) if not a.tokens else \
        [(f"{w} N={N}", N, D, 16) for N in a.tokens for w, D in (("ViT-L", 1024), ("ViT-H", 1280))]
    if a.bank:
        return bank_bench(a, shapes)
    for tag, N, D, H in shapes:
        B, hd = a.batch, D // H
        torch.manual_seed(0)
        m = AttentiveClassifier(embed_dim=D, num_heads=H, depth=1, num_classes=400).to(dev)
        x = torch.randn(B, N, D, device=dev).to(torch.bfloat16)
        y = torch.randint(0, 400, (B,), device=dev)

        def step():
            for p in m.parameters():
                p.grad = None
            torch.nn.functional.cross_entropy(m(x), y).backward()
        us = timeit(step, a.reps)
        flop = 3 * 2.0 * B * N * D * 2 * D      # kv projection forward + dgrad + wgrad dominate
        print(f"{tag}: probe step B={B}: {us:8.1f} us  ({B / us * 1e6:7.0f} samples/s, kv-projection GEMMs {flop / us / 1e6:6.0f} TF/s)")
        q = torch.randn(1, D, device=dev).to(torch.bfloat16)
        kv = torch.randn(B * N, 2 * D, device=dev).to(torch.bfloat16)
        dy = torch.randn(B, D, device=dev).to(torch.bfloat16)
        out, lse = ops.xattn_fwd(q, kv, B, 1, N, H, hd, hd ** -0.5)
        uf = timeit(lambda: ops.xattn_fwd(q, kv, B, 1, N, H, hd, hd ** -0.5), a.reps)
        ub = timeit(lambda: ops.xattn_bwd(q, kv, dy, lse, B, N, H, hd, hd ** -0.5), a.reps)
        byt = B * N * 2 * D * 2.0
        fs = "split" if lib.vj_xattn_ws_bytes(B, 1, N, H, hd, 0) > 0 else "1-wg"
        bs = "split" if lib.vj_xattn_ws_bytes(B, 1, N, H, hd, 1) > 0 else "1-wg"
        # bwd: K+V read once, and the kernel's algorithmic bytes (single workgroup: K, V read twice + dK, dV written = 3x K+V, the
        # figure this tool printed before the split kernels; split: 2.5x K+V + 16 bytes of p / dP per key and head)
        alg = 3 * byt if bs == "1-wg" else 2.5 * byt + 16.0 * B * N * H
        print(f"{tag}: xattn fwd [{fs}] {uf:8.1f} us = {byt / uf / 1e6:5.2f} TB/s of K+V | bwd [{bs}] {ub:8.1f} us = {byt / ub / 1e6:5.2f} "
              f"TB/s of K+V, {alg / ub / 1e6:5.2f} TB/s algorithmic")


if __name__ == "__main__":
    main()
