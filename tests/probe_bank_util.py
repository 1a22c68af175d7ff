"""Test helpers for the probe bank: a restatement of the pooled algebra (no K, no V) with explicit backward formulas, in the
dtype of its inputs, and the loader of tests/golden/probe_bank_micro.npz (tools/make_golden_probe_bank.py)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "probe_bank_micro.npz")
BLK = "pooler.cross_attention_block."


def rel_l2(a, b):
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-300))


def pooled_loss_and_grads(w, x, labels, heads, eps=1e-5):
    """Loss, logits and every parameter gradient of one AttentiveClassifier (reference state-dict names in `w`) through the
    pooled form: the cross-attention forward and backward are written out formula by formula; only the tail (q0 + y -> norm2 ->
    MLP -> linear -> cross-entropy) goes through autograd."""
    B, N, D = x.shape
    H, hd = heads, D // heads
    s = hd ** -0.5
    gam, bet = w[BLK + "norm1.weight"], w[BLK + "norm1.bias"]
    Wq, bq = w[BLK + "xattn.q.weight"], w[BLK + "xattn.q.bias"]
    Wkv, bkv = w[BLK + "xattn.kv.weight"], w[BLK + "xattn.kv.bias"]
    Wk, Wv, bv = Wkv[:D].view(H, hd, D), Wkv[D:].view(H, hd, D), bkv[D:].view(H, hd)
    q0 = w["pooler.query_tokens"].reshape(D)
    xh = F.layer_norm(x, (D,), None, None, eps)                       # x_hat: LayerNorm without affine
    # forward
    q = (Wq @ q0 + bq).view(H, hd)
    t = torch.einsum("hjd,hj->hd", Wk, q)
    u = s * gam * t
    S = torch.einsum("bnd,hd->bnh", xh, u)
    A = torch.softmax(S, dim=1)
    Z = torch.einsum("bnh,bnd->bhd", A, xh)
    R = gam * Z + bet
    y = (torch.einsum("hjd,bhd->bhj", Wv, R) + bv).reshape(B, D)
    # tail under autograd, from y
    names = ["pooler.query_tokens", BLK + "norm2.weight", BLK + "norm2.bias", BLK + "mlp.fc1.weight", BLK + "mlp.fc1.bias",
             BLK + "mlp.fc2.weight", BLK + "mlp.fc2.bias", "linear.weight", "linear.bias"]
    tw = {k: w[k].detach().clone().requires_grad_(True) for k in names}
    yl = y.detach().clone().requires_grad_(True)
    q1 = tw["pooler.query_tokens"].reshape(1, D) + yl
    h = F.layer_norm(q1, (D,), tw[BLK + "norm2.weight"], tw[BLK + "norm2.bias"], eps)
    h = F.linear(F.gelu(F.linear(h, tw[BLK + "mlp.fc1.weight"], tw[BLK + "mlp.fc1.bias"])), tw[BLK + "mlp.fc2.weight"],
                 tw[BLK + "mlp.fc2.bias"])
    logits = F.linear(q1 + h, tw["linear.weight"], tw["linear.bias"])
    loss = F.cross_entropy(logits, labels)
    loss.backward()
    g = {k: v.grad for k, v in tw.items()}
    dy = yl.grad.view(B, H, hd)
    # value path
    dbv = dy.sum(0)
    dWv = torch.einsum("bhj,bhd->hjd", dy, R)
    G = torch.einsum("hjd,bhj->bhd", Wv, dy)
    dbeta = G.sum((0, 1))
    dgam = (G * Z).sum((0, 1))
    dZ = gam * G
    # score path
    dA = torch.einsum("bnd,bhd->bnh", xh, dZ)
    delta = (dZ * Z).sum(-1)
    dS = A * (dA - delta[:, None, :])
    dU = torch.einsum("bnh,bnd->hd", dS, xh)
    dgam = dgam + (dU * s * t).sum(0)
    e = s * gam * dU
    dWk = torch.einsum("hj,hd->hjd", q, e)
    # query path
    dq = torch.einsum("hjd,hd->hj", Wk, e).reshape(D)
    g[BLK + "xattn.q.bias"] = dq
    g[BLK + "xattn.q.weight"] = torch.outer(dq, q0)
    g["pooler.query_tokens"] = g["pooler.query_tokens"] + (Wq.t() @ dq).view_as(g["pooler.query_tokens"])
    g[BLK + "xattn.kv.weight"] = torch.cat([dWk.reshape(D, D), dWv.reshape(D, D)])
    g[BLK + "xattn.kv.bias"] = torch.cat([torch.zeros(D, dtype=x.dtype), dbv.reshape(D)])   # the key half: exactly zero
    g[BLK + "norm1.weight"], g[BLK + "norm1.bias"] = dgam, dbeta
    return loss.detach(), logits.detach(), g


def load_fixture():
    """-> meta dict, x, labels, and per probe: dict(w0, logits, loss, grads, lr, wd, losses [3], w_final)."""
    z = np.load(GOLDEN)
    meta = {k: int(z["meta_" + k]) for k in ("P", "B", "N", "D", "H", "C", "steps")}
    t = lambda a: torch.from_numpy(np.array(a))   # noqa: E731
    probes = []
    for p in range(meta["P"]):
        pre = f"p{p}."
        pick = lambda kind: {k[len(pre + kind) + 1:]: t(z[k]) for k in z.files if k.startswith(pre + kind + ".")}   # noqa: E731
        probes.append(dict(w0=pick("w0"), grads=pick("grad"), w_final=pick("w_final"), logits=t(z[pre + "logits"]),
                           loss=float(z[pre + "loss"]), losses=[float(v) for v in z[pre + "losses"]], lr=float(z[pre + "lr"]),
                           wd=float(z[pre + "wd"])))
    return meta, t(z["x"]), t(z["labels"]), probes
