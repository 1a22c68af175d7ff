"""GPU: the probe bank (AttentiveClassifierBank over csrc/probe_bank.hip and the GEMM / weight-gradient kernels) -- the two
key-axis soft-max kernels per element against float64, the bank against the reference fixture and against the fp32 oracle at the
evals' shapes, and isolation / determinism between probes."""
import pytest
import torch

from tests.probe_bank_util import BLK, load_fixture, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
KVB = BLK + "xattn.kv.bias"
# the lone probe's bounds (tests/test_probe_gpu.py): logits rel-L2, every gradient tensor rel-L2, loss relative to max(1, |loss|)
TOL_LOGITS, TOL_GRAD, TOL_LOSS = 1e-2, 2e-2, 2e-2


# ---------------------------------------------------------------- the soft-max kernels
def _scores(B, N, C, real_cols, seed):
    """fp32 [B, N, C]: column scales cycle through 0.5 / 5 / 80 (uniform in +-scale, so the widest reach +-80), columns from
    `real_cols` on are the all-zero padding."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([0.5, 5.0, 80.0])[torch.arange(C) % 3]
    S = (torch.rand(B, N, C, generator=g) * 2 - 1) * scale
    S[:, :, real_cols:] = 0.0
    return S


def _softmax_cases():
    from jepa_amd.hip import lib as L
    c = int(L.load_library().vj_pool_softmax_chunk_keys())
    return [(B, N, C, real) for N in (1, c - 1, c, c + 1, 2 * c + 3) for (C, real) in ((64, 6), (320, 319)) for B in (1, 3)]


def test_pool_softmax_kernels_against_float64():
    """vj_pool_softmax_fwd / _bwd per element.  A is bf16(exp(s - lse)): bf16 keeps 8 significand bits, so round-to-nearest moves a
    value by at most half an ulp = 2^-8 of it (reached just above a power of two: 1/255 rounds to 1.0078 / 256, 3.9e-3 away), plus
    the fp32 evaluation (the argument s - lse, up to 160 + log N in magnitude, carries 2^-24 relative, i.e. <= 1e-5 absolute in
    the exponent, and lse itself a few fp32 ulps of ~90: 1e-4 relative in all), plus 1e-37 where fp32 underflows.  A column
    therefore sums to 1 within 2^-8 + 1e-4 (every key rounding the same way, as in the uniform padded column).  dS = bf16(A (dA -
    delta)) from the kernel's own bf16 A: the same 2^-8 plus the fp32 subtraction's rounding, A * (|dA| + |delta|) * 2^-22."""
    from jepa_amd.hip import ops
    for B, N, C, real in _softmax_cases():
        S = _scores(B, N, C, real, seed=N + C + B)
        Sd = S.to(DEV)
        A, lse = ops.pool_softmax_fwd(Sd)
        A2, lse2 = ops.pool_softmax_fwd(Sd.clone())
        assert torch.equal(A, A2) and torch.equal(lse, lse2), (B, N, C)
        assert torch.isfinite(A.float()).all() and torch.isfinite(lse).all()
        ref_lse = torch.logsumexp(S.double(), dim=1)
        ref_A = torch.exp(S.double() - ref_lse[:, None, :])
        Af = A.cpu().double()
        assert (lse.cpu().double() - ref_lse).abs().max() < 1e-4, (B, N, C, float((lse.cpu().double() - ref_lse).abs().max()))
        bound = ref_A * (2.0 ** -8 + 1e-4) + 1e-37
        assert ((Af - ref_A).abs() <= bound).all(), (B, N, C, float(((Af - ref_A).abs() - bound).max()))
        assert (Af.sum(dim=1) - 1.0).abs().max() <= 2.0 ** -8 + 1e-4, (B, N, C)   # every column sums to 1 within bf16 rounding
        assert (A[:, :, real:] == A[:, :1, real:]).all()                           # the all-zero padding: uniform (1 / N by the bound)
        g = torch.Generator().manual_seed(7 * N + C)
        dA = torch.randn(B, N, C, generator=g)
        delta = (Af * dA.double()).sum(dim=1)
        dS = ops.pool_softmax_bwd(A, dA.to(DEV), delta.float().to(DEV))
        dS2 = ops.pool_softmax_bwd(A, dA.to(DEV), delta.float().to(DEV))
        assert torch.equal(dS, dS2)
        d32 = delta.float().double()[:, None, :]
        ref_dS = Af * (dA.double() - d32)
        bound = ref_dS.abs() * 2.0 ** -8 + Af * (dA.double().abs() + d32.abs()) * 2.0 ** -22 + 1e-37
        assert ((dS.cpu().double() - ref_dS).abs() <= bound).all(), (B, N, C, float(((dS.cpu().double() - ref_dS).abs() - bound).max()))


# ---------------------------------------------------------------- the bank
def _bank(D, H, C, weights):
    from jepa_amd.src.models.attentive_pooler import AttentiveClassifierBank
    bank = AttentiveClassifierBank(D, H, C, len(weights)).to(DEV)
    for m, w in zip(bank.probes, weights):
        res = m.load_state_dict({k: v.to(DEV) for k, v in w.items()}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
    return bank


def _lone(D, H, C, w):
    from jepa_amd.src.models.attentive_pooler import AttentiveClassifier
    m = AttentiveClassifier(embed_dim=D, num_heads=H, depth=1, num_classes=C).to(DEV)
    m.load_state_dict({k: v.to(DEV) for k, v in w.items()}, strict=True)
    return m


def _step(bank, x, labels):
    """One forward + ONE backward of the summed per-probe losses -> logits [P, B, C], losses [P], per-probe {name: grad}."""
    for p in bank.parameters():
        p.grad = None
    logits = bank(x)
    losses = torch.stack([torch.nn.CrossEntropyLoss()(logits[p], labels) for p in range(logits.shape[0])])
    losses.sum().backward()
    grads = [{n: q.grad.detach().clone() for n, q in m.named_parameters() if q.grad is not None} for m in bank.probes]
    return logits.detach(), losses.detach(), grads


def _errors(logits, loss, grads, ref_logits, ref_loss, ref_grads, D):
    """-> {tensor name or 'logits' / 'loss': error}; kv.bias on its value half, whose key half must be exactly zero here."""
    out = {"logits": rel_l2(logits.cpu(), ref_logits), "loss": abs(float(loss) - float(ref_loss)) / max(1.0, abs(float(ref_loss)))}
    assert set(grads) == set(ref_grads), set(grads) ^ set(ref_grads)
    for k, ref in ref_grads.items():
        a, b = (grads[k][D:], ref[D:]) if k == KVB else (grads[k], ref)
        out[k] = rel_l2(a.cpu(), b.cpu())
    return out


def _assert_within(err, what):
    for k, e in err.items():
        tol = TOL_LOGITS if k == "logits" else TOL_LOSS if k == "loss" else TOL_GRAD
        assert e < tol, (what, k, e)


def _lone_errors(D, H, C, w, x, labels, ref_logits, ref_loss, ref_grads):
    m = _lone(D, H, C, w)
    logits = m(x)
    loss = torch.nn.CrossEntropyLoss()(logits, labels)
    loss.backward()
    grads = {n: q.grad for n, q in m.named_parameters() if q.grad is not None}
    return _errors(logits.detach(), loss.detach(), grads, ref_logits, ref_loss, ref_grads, D)


def _report(tag, bank_err, lone_err):
    print(f"\n{tag}: error of the bank | of the lone probe on the same inputs")
    for k in bank_err:
        print(f"  {k:55s} {bank_err[k]:.3e} | {lone_err[k]:.3e}")


def test_bank_matches_reference_fixture_and_three_optimizer_steps():
    """Step 0 against the real reference's logits / loss / gradients at the lone probe's bounds, then three steps of
    clip_grad_norm_(1.0) + AdamW(lr_p, wd_p) per probe: losses at 2e-2 relative (the eval fixtures' bound), final weights at 1e-1
    rel-L2 per tensor (kv.bias: value half; its key half bitwise where it was initialised)."""
    meta, x, labels, probes = load_fixture()
    D, H, C = meta["D"], meta["H"], meta["C"]
    bank = _bank(D, H, C, [p["w0"] for p in probes])
    xd, ld = x.to(DEV), labels.to(DEV)
    opts = [torch.optim.AdamW(m.parameters(), lr=p["lr"], weight_decay=p["wd"]) for m, p in zip(bank.probes, probes)]
    for step in range(meta["steps"]):
        logits, losses, grads = _step(bank, xd, ld)
        assert logits.dtype == torch.float32 and tuple(logits.shape) == (meta["P"], meta["B"], C)
        for i, p in enumerate(probes):
            if step == 0:
                assert torch.count_nonzero(grads[i][KVB][:D]) == 0
                err = _errors(logits[i], losses[i], grads[i], p["logits"], p["loss"], p["grads"], D)
                _report(f"fixture probe {i}", err, _lone_errors(D, H, C, p["w0"], xd, ld, p["logits"], p["loss"], p["grads"]))
                _assert_within(err, f"probe {i}")
            rel = abs(float(losses[i]) - p["losses"][step]) / abs(p["losses"][step])
            print(f"probe {i} step {step}: loss {float(losses[i]):.6f} reference {p['losses'][step]:.6f} rel {rel:.2e}")
            assert rel < 2e-2, (i, step, rel)
        for m, opt in zip(bank.probes, opts):
            torch.nn.utils.clip_grad_norm_([q for q in m.parameters() if q.grad is not None], 1.0)
            opt.step()
    for i, (m, p) in enumerate(zip(bank.probes, probes)):
        sd = bank.probe_state_dict(i)
        assert torch.equal(sd[KVB][:D].cpu(), p["w0"][KVB][:D])
        for k, ref in p["w_final"].items():
            a, b = (sd[k][D:], ref[D:]) if k == KVB else (sd[k], ref)
            e = rel_l2(a.cpu(), b)
            assert e < 1e-1, (i, k, e)
    finals = [bank.probe_state_dict(i)["linear.weight"] for i in range(3)]
    assert not torch.equal(finals[0], finals[1]) and not torch.equal(finals[1], finals[2])


@pytest.mark.parametrize("P,B,N,D,H,C", [(5, 2, 1568, 1024, 16, 174), (2, 2, 300, 1280, 16, 174)])
def test_bank_at_eval_shape_against_the_fp32_oracle(P, B, N, D, H, C):
    """ViT-L features of one clip per sample with 174 classes, and head_dim 80 (ViT-H), against oracle/probe_oracle.py run by eager
    PyTorch in fp32 on the device, probe by probe, at the lone probe's bounds."""
    from oracle import probe_oracle as po
    from jepa_amd.src.models.attentive_pooler import AttentiveClassifierBank
    torch.manual_seed(5)
    bank = AttentiveClassifierBank(D, H, C, P).to(DEV)
    with torch.no_grad():
        for q in bank.parameters():
            if q.dim() == 1:
                q.add_(0.05 * torch.randn_like(q))
    x = torch.randn(B, N, D, device=DEV)
    labels = torch.randint(0, C, (B,), device=DEV)
    logits, losses, grads = _step(bank, x, labels)
    for i, m in enumerate(bank.probes):
        w = {n: q.detach().clone() for n, q in m.named_parameters()}
        o_loss, o_logits, o_grads = po.probe_loss_and_grads(w, x, labels, H)
        assert torch.count_nonzero(grads[i][KVB][:D]) == 0
        err = _errors(logits[i], losses[i], grads[i], o_logits.cpu(), o_loss, o_grads, D)
        if i == 0:
            _report(f"P={P} N={N} D={D} probe 0", err, _lone_errors(D, H, C, w, x, labels, o_logits.cpu(), o_loss, o_grads))
        _assert_within(err, f"probe {i}")


def test_bank_isolation_and_determinism():
    """Probe j's weights do not reach probe i: perturbing probe 2 leaves the logits and every gradient of probes 0 and 1 bitwise
    unchanged; two identical calls are bitwise equal; a bank of one agrees with the same probe inside a bank of three within the
    bounds above (not bitwise: the GEMM may pick another tile shape for another column count).  N = 300 spans two key chunks."""
    B, N, D, H, C = 2, 300, 64, 2, 5
    torch.manual_seed(9)
    from jepa_amd.src.models.attentive_pooler import AttentiveClassifierBank
    bank = AttentiveClassifierBank(D, H, C, 3).to(DEV)
    with torch.no_grad():
        for q in bank.parameters():
            if q.dim() == 1:
                q.add_(0.1 * torch.randn_like(q))
    x = torch.randn(B, N, D, device=DEV)
    labels = torch.randint(0, C, (B,), device=DEV)
    l1, s1, g1 = _step(bank, x, labels)
    l2, s2, g2 = _step(bank, x, labels)
    assert torch.equal(l1, l2) and torch.equal(s1, s2)
    for a, b in zip(g1, g2):
        assert all(torch.equal(a[k], b[k]) for k in a)
    one = _bank(D, H, C, [{k: v.detach().cpu() for k, v in bank.probe_state_dict(0).items()}])
    lo, so, go = _step(one, x, labels)
    _assert_within(_errors(lo[0], so[0], go[0], l1[0].cpu(), s1[0], g1[0], D), "bank of one against probe 0 of three")
    with torch.no_grad():
        for q in bank.probes[2].parameters():
            q.mul_(1.5).add_(0.01)
    l3, s3, g3 = _step(bank, x, labels)
    assert not torch.equal(l3[2], l1[2])
    for i in (0, 1):
        assert torch.equal(l3[i], l1[i]) and torch.equal(s3[i], s1[i]), i
        assert all(torch.equal(g3[i][k], g1[i][k]) for k in g1[i]), i
