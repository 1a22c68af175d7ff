#!/usr/bin/env python
"""Generate tests/golden/probe_bank_micro.npz from the REAL reference AttentiveClassifier (src/models/attentive_pooler.py:105-136),
CPU fp32, one thread.

    JEPA_REFERENCE=/path/to/jepa python tools/make_golden_probe_bank.py

Three probes built one after the other under one seed (the order AttentiveClassifierBank builds its own), B = 3 samples of N = 70
feature tokens, D = 32, 2 heads, 5 classes.  Every 1-D parameter is perturbed so that LayerNorm affines and biases matter, except
the key half of xattn.kv.bias, which stays at its initial zero: it shifts every score of a head alike, the soft-max drops it, and
its gradient in the reference is rounding noise.

Per probe (arrays only): initial weights, logits, loss and every gradient at step 0; then STEPS steps of
`clip_grad_norm_(1.0)` + `torch.optim.AdamW(lr_p, weight_decay=wd_p)` on the fixed batch with three distinct (lr, wd): the loss of
each step and the final weights.  Re-running reproduces the file bit for bit.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("JEPA_REFERENCE", "")
OUT = os.path.join(ROOT, "tests", "golden", "probe_bank_micro.npz")

P, B, N, D, H, C, STEPS = 3, 3, 70, 32, 2, 5, 3
HP = [(5e-4, 0.0), (1e-3, 0.01), (2e-3, 0.1)]   # (lr, weight_decay) per probe
SEED = 31


def main():
    if not REF:
        sys.exit("set JEPA_REFERENCE to a checkout of the reference")
    sys.path.insert(0, REF)
    from src.models.attentive_pooler import AttentiveClassifier
    torch.set_num_threads(1)
    torch.manual_seed(SEED)
    probes = [AttentiveClassifier(embed_dim=D, num_heads=H, depth=1, num_classes=C) for _ in range(P)]
    g = torch.Generator().manual_seed(SEED + 1)
    with torch.no_grad():
        for m in probes:
            for name, p in m.named_parameters():
                if p.dim() == 1:
                    p.add_(0.1 * torch.randn(p.shape, generator=g))
            m.pooler.cross_attention_block.xattn.kv.bias[:D] = 0.0
    x = torch.randn(B, N, D, generator=g)
    labels = torch.randint(0, C, (B,), generator=g)
    out = {"x": x.numpy(), "labels": labels.numpy()}
    for k, v in dict(P=P, B=B, N=N, D=D, H=H, C=C, steps=STEPS).items():
        out["meta_" + k] = np.int64(v)
    for i, (m, (lr, wd)) in enumerate(zip(probes, HP)):
        pre = f"p{i}."
        out[pre + "lr"], out[pre + "wd"] = np.float64(lr), np.float64(wd)
        for name, p in m.named_parameters():
            out[pre + "w0." + name] = p.detach().numpy().copy()
        opt = torch.optim.AdamW(m.parameters(), lr=lr, weight_decay=wd)
        losses = []
        for step in range(STEPS):
            opt.zero_grad(set_to_none=True)
            logits = m(x)
            loss = torch.nn.CrossEntropyLoss()(logits, labels)
            loss.backward()
            if step == 0:
                out[pre + "logits"], out[pre + "loss"] = logits.detach().numpy().copy(), loss.detach().numpy().copy()
                for name, p in m.named_parameters():
                    if p.grad is not None:
                        out[pre + "grad." + name] = p.grad.numpy().copy()
            torch.nn.utils.clip_grad_norm_([p for p in m.parameters() if p.grad is not None], 1.0)
            opt.step()
            losses.append(float(loss))
        out[pre + "losses"] = np.array(losses, dtype=np.float64)
        for name, p in m.named_parameters():
            out[pre + "w_final." + name] = p.detach().numpy().copy()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
