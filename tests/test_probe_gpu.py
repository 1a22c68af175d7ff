"""GPU: the trainable attentive probe (jepa_amd/src/models/attentive_pooler.py over csrc/xattn.hip and the GEMM / LayerNorm /
weight-gradient kernels) against (i) the fixture generated from the real reference AttentiveClassifier and (ii) the fp32 oracle
(oracle/probe_oracle.py, run by eager PyTorch as the checker) at the size the reference's evals use."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel_l2(a, b):
    a, b = a.detach().float().reshape(-1), b.detach().float().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-12))


def _load_fixture(name):
    from tests.test_probe_oracle import load_case
    return load_case(name)


def _build(D, H, C, w):
    from jepa_amd.src.models.attentive_pooler import AttentiveClassifier
    m = AttentiveClassifier(embed_dim=D, num_heads=H, depth=1, num_classes=C).to(DEV)
    missing = m.load_state_dict({k: v.to(DEV) for k, v in w.items()}, strict=True)   # the reference's state-dict names, all of them
    assert not missing.missing_keys and not missing.unexpected_keys
    return m


def _check(m, w, g_ref, x, labels, logits_ref, loss_ref, tol_logits, tol_grad):
    logits = m(x.to(DEV))
    assert logits.dtype == torch.float32 and logits.shape == logits_ref.shape
    assert rel_l2(logits.cpu(), logits_ref) < tol_logits, ("logits", rel_l2(logits.cpu(), logits_ref))
    loss = torch.nn.CrossEntropyLoss()(logits, labels.to(DEV))
    assert abs(float(loss.detach()) - float(loss_ref)) < 2e-2 * max(1.0, abs(float(loss_ref)))
    loss.backward()
    worst = ("", 0.0)
    for n, p in m.named_parameters():
        if n not in g_ref:
            assert p.grad is None, n   # xattn.proj.*: never applied by the reference's forward -> no gradient there, none here
            continue
        assert p.grad is not None and p.grad.shape == p.shape, n
        e = rel_l2(p.grad.cpu(), g_ref[n])
        worst = max(worst, (n, e), key=lambda t: t[1])
        assert e < tol_grad, (n, e)
    return worst


@pytest.mark.parametrize("name", ["a", "b"])
def test_attentive_classifier_matches_reference_fixture(name):
    (B, N, D, H, C), w, g, x, labels, logits, loss = _load_fixture(name)
    m = _build(D, H, C, w)
    worst = _check(m, w, g, x, labels, logits, loss, tol_logits=1e-2, tol_grad=2e-2)   # measured: gradients <= 7e-3 (xattn.q.weight)
    print("worst gradient", worst)


def test_attentive_classifier_at_eval_size_and_training_steps():
    """ViT-L features of one 16 x 224 x 224 clip per sample (N = 1568, D = 1024, 16 heads), 174 classes (not a multiple of 4: the head
    pads internally), against the fp32 oracle on the same device; then five AdamW steps of the reference's eval loop shape
    (eval.py:330-352) must reduce the loss on a fixed batch."""
    from oracle import probe_oracle as po
    from jepa_amd.src.models.attentive_pooler import AttentiveClassifier
    B, N, D, H, C = 4, 1568, 1024, 16, 174
    torch.manual_seed(5)
    m = AttentiveClassifier(embed_dim=D, num_heads=H, depth=1, num_classes=C).to(DEV)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    x = torch.randn(B, N, D, device=DEV)
    labels = torch.randint(0, C, (B,), device=DEV)
    w = {n: p.detach().clone() for n, p in m.named_parameters()}
    o_loss, o_logits, o_grads = po.probe_loss_and_grads(w, x, labels, H)
    worst = _check(m, w, {k: v.cpu() for k, v in o_grads.items()}, x.cpu(), labels.cpu(), o_logits.cpu(), o_loss.cpu(),
                   tol_logits=1e-2, tol_grad=2e-2)   # measured: gradients <= 7e-3 (xattn.q.weight)
    print("worst gradient", worst)
    opt = torch.optim.AdamW([p for n, p in m.named_parameters() if "xattn.proj" not in n], lr=1e-3, weight_decay=0.01)
    losses = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.CrossEntropyLoss()(m(x), labels)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0] - 0.05, losses


def test_xattn_kernel_against_sdpa():
    """vj_xattn_fwd / vj_xattn_bwd on their own: several queries forward (per-sample queries), one query backward, ragged N, head
    dims 24 / 64 / 80 / 128, against F.scaled_dot_product_attention in fp32."""
    from jepa_amd.hip import ops
    g = torch.Generator().manual_seed(3)
    # (the last case: eight 1568-token segments attended across (eval.py `attend_across_segments`), 109 KB of dynamic LDS in the backward)
    for B, NQ, N, H, hd in [(2, 3, 77, 2, 64), (1, 1, 1, 1, 24), (3, 1, 1568, 16, 64), (2, 1, 300, 4, 80), (1, 2, 130, 2, 128),
                            (1, 1, 12544, 2, 64)]:
        D = H * hd
        q = (torch.randn(B, NQ, D, generator=g)).to(torch.bfloat16).to(DEV)
        kv = (torch.randn(B * N, 2 * D, generator=g)).to(torch.bfloat16).to(DEV)
        out, lse = ops.xattn_fwd(q.reshape(B * NQ, D), kv, B, NQ, N, H, hd, hd ** -0.5, shared_q=False)
        qf = q.float().reshape(B, NQ, H, hd).permute(0, 2, 1, 3).requires_grad_(True)
        kvf = kv.float().reshape(B, N, 2, H, hd).permute(2, 0, 3, 1, 4)
        kf, vf = kvf[0].detach().requires_grad_(True), kvf[1].detach().requires_grad_(True)
        ref = torch.nn.functional.scaled_dot_product_attention(qf, kf, vf)
        assert rel_l2(out.reshape(B, NQ, H, hd).permute(0, 2, 1, 3), ref) < 8e-3, (B, NQ, N, H, hd)
        if NQ == 1:
            dy = torch.randn(B, D, generator=g).to(torch.bfloat16).to(DEV)
            dq, dkv = ops.xattn_bwd(q.reshape(B, D), kv, dy, lse, B, N, H, hd, hd ** -0.5, shared_q=False)
            ref.backward(dy.float().reshape(B, 1, H, hd).permute(0, 2, 1, 3))
            assert rel_l2(dq.reshape(B, 1, H, hd).permute(0, 2, 1, 3), qf.grad) < 1.5e-2
            dkvv = dkv.float().reshape(B, N, 2, H, hd).permute(2, 0, 3, 1, 4)
            assert rel_l2(dkvv[0], kf.grad) < 1.5e-2 and rel_l2(dkvv[1], vf.grad) < 1.5e-2


@pytest.mark.parametrize("N", [1, 255, 256, 257])
@pytest.mark.parametrize("hd", [8, 24, 80, 128])
def test_xattn_thread_mapping_edges(hd, N):
    """The edges of the single-workgroup kernels' thread mapping, at the bounds of test_xattn_kernel_against_sdpa.  Threads are
    (row group, 8-column chunk): hd = 8 is one chunk per row and 256 row groups, hd = 80 is 25 row groups with 6 idle threads,
    hd = 128 is 16 chunks; N = 1 / 255 / 256 / 257 is one partial pass of the 256-thread stride over the keys, one full pass, then
    two.  Three queries forward, one query forward and backward."""
    from jepa_amd.hip import ops
    B, H = 2, 2
    D = H * hd
    g = torch.Generator().manual_seed(1000 * hd + N)
    for NQ in (3, 1):
        q = torch.randn(B, NQ, D, generator=g).to(torch.bfloat16).to(DEV)
        kv = torch.randn(B * N, 2 * D, generator=g).to(torch.bfloat16).to(DEV)
        out, lse = ops.xattn_fwd(q.reshape(B * NQ, D), kv, B, NQ, N, H, hd, hd ** -0.5, shared_q=False)
        qf = q.float().reshape(B, NQ, H, hd).permute(0, 2, 1, 3).requires_grad_(True)
        kvf = kv.float().reshape(B, N, 2, H, hd).permute(2, 0, 3, 1, 4)
        kf, vf = kvf[0].detach().requires_grad_(True), kvf[1].detach().requires_grad_(True)
        ref = torch.nn.functional.scaled_dot_product_attention(qf, kf, vf)
        e = rel_l2(out.reshape(B, NQ, H, hd).permute(0, 2, 1, 3), ref)
        print("out", NQ, e)
        assert e < 8e-3, ("out", NQ, e)
        if NQ != 1:
            continue
        dy = torch.randn(B, D, generator=g).to(torch.bfloat16).to(DEV)
        dq, dkv = ops.xattn_bwd(q.reshape(B, D), kv, dy, lse, B, N, H, hd, hd ** -0.5, shared_q=False)
        ref.backward(dy.float().reshape(B, 1, H, hd).permute(0, 2, 1, 3))
        dkvv = dkv.float().reshape(B, N, 2, H, hd).permute(2, 0, 3, 1, 4)
        errs = {"dq": rel_l2(dq.reshape(B, 1, H, hd).permute(0, 2, 1, 3), qf.grad), "dk": rel_l2(dkvv[0], kf.grad),
                "dv": rel_l2(dkvv[1], vf.grad)}
        print(errs)
        # One key: p = 1 whatever q, so dq and dk are exactly zero.  fp32 SDPA leaves a rounding residue there at hd = 80 and 128
        # (|dq| 5.5e-7 and 9.8e-7; exactly 0 at hd = 8 and 24), against which an exact 0 has relative error 0.999998: the bound says
        # nothing.  Zero to the bit instead, which is what the kernels gave before their bodies were shared; dv as everywhere.
        if N == 1:
            print("reference |dq|, |dk|", float(qf.grad.norm()), float(kf.grad.norm()))
            assert not dq.any() and not dkvv[0].any()
            errs = {"dv": errs["dv"]}
        for name, e in errs.items():
            assert e < 1.5e-2, (name, e)


def test_frozen_eval_loop_encoder_to_probe():
    """The reference's frozen evaluation end to end on the HIP path (evals/video_classification_frozen/eval.py:330-352): clips ->
    frozen encoder under no_grad (every parameter requires_grad=False) -> AttentiveClassifier -> CrossEntropy -> backward ->
    clip_grad_norm_(1.0) -> AdamW.  First-step loss and probe gradients against the fp32 oracles chained the same way
    (vjepa_oracle.encoder_forward -> probe_oracle); then the loop must learn a fixed batch."""
    from oracle import probe_oracle as po
    from oracle import vjepa_oracle as O
    from jepa_amd.src.models.attentive_pooler import AttentiveClassifier
    from tests.step_util import TINY, build_models, oracle_cfg
    enc, _ = build_models(TINY, 2, perturb_small=True)
    vit = enc.backbone
    w_enc = {k: v.detach().clone() for k, v in vit.state_dict().items()}
    for p in vit.parameters():
        p.requires_grad = False
    vit.to(DEV)
    B, C = 6, 5
    g = torch.Generator().manual_seed(11)
    clips = torch.randn(B, 3, TINY["frames"], TINY["crop"], TINY["crop"], generator=g)
    labels = torch.randint(0, C, (B,), generator=g)
    torch.manual_seed(2)
    clf = AttentiveClassifier(embed_dim=TINY["embed_dim"], num_heads=TINY["heads"], depth=1, num_classes=C).to(DEV)
    w_clf = {n: p.detach().clone().cpu() for n, p in clf.named_parameters()}
    feats_ref = O.encoder_forward(w_enc, clips, oracle_cfg(TINY, 2))
    o_loss, o_logits, o_grads = po.probe_loss_and_grads(w_clf, feats_ref, labels, TINY["heads"])
    opt = torch.optim.AdamW([p for n, p in clf.named_parameters() if "xattn.proj" not in n], lr=2e-3, weight_decay=0.01)
    losses = []
    for it in range(8):
        with torch.no_grad():
            feats = vit(clips.to(DEV))
        logits = clf(feats)
        loss = torch.nn.CrossEntropyLoss()(logits, labels.to(DEV))
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if it == 0:
            assert abs(float(loss) - float(o_loss)) < 1e-2 * max(1.0, float(o_loss)), (float(loss), float(o_loss))
            assert rel_l2(logits.cpu(), o_logits) < 3e-2
            for n, p in clf.named_parameters():
                if n in o_grads:
                    assert rel_l2(p.grad.cpu(), o_grads[n]) < 5e-2, (n, rel_l2(p.grad.cpu(), o_grads[n]))
        torch.nn.utils.clip_grad_norm_([p for p in clf.parameters() if p.grad is not None], 1.0)
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0] - 0.1, losses
