"""GPU: the attentive probe passes the gradient on to its input features (fine-tuning an encoder through the probe).

dX of AttentiveClassifier + cross-entropy against oracle.probe_oracle.attentive_classifier in float64 on the bf16-rounded
features, per sample by rel-L2, and the exact properties of the new path: a sample without a loss gradient gets an exactly zero
dX, the parameter gradients and logits do not depend on whether the features ask for a gradient, the gradient has the features'
shape and dtype.  The probe bank keeps refusing features that require grad.

Bound: 2e-2, what tests/test_probe_gpu.py allows norm1.weight, which comes out of the same dkv -> GEMM -> layernorm_bwd
launches.  Measured worst per-sample rel-L2 on MI355X: 6.4e-3 (MEASURED below, per shape; profiles/finetune.md)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu
DEV = "cuda"

# The first key count at which vj_xattn_bwd_ws splits the keys: the single-workgroup backward keeps two fp32 arrays of N scores in
# (XA_LDS_MAX / 4 - XA_LDS_FIXED) = (160 KiB - 2 KiB) / 4 - (128 + 8 + 2048) = 38 264 floats of LDS, so it takes N <= 19 132
# (csrc/xattn.hip: xa_max_keys(2)); vj_xattn_ws_bytes(backward) is 0 up to there and the split form's workspace above.
N_SPLIT = 19133

SHAPES = [(2, 1, 64, 2), (2, 63, 64, 2), (2, 65, 64, 2), (3, 257, 96, 4), (2, N_SPLIT, 64, 2)]   # (B, N, D, H); the fourth: head_dim 24
BOUND = 2e-2
# measured worst per-sample rel-L2 of dX per shape, in SHAPES order (MI355X)
MEASURED = (4.64e-3, 5.16e-3, 5.26e-3, 6.42e-3, 5.28e-3)
C = 10


def rel_l2(a, b):
    a, b = a.detach().double().reshape(-1).cpu(), b.detach().double().reshape(-1).cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def _probe(D, H, seed=5):
    from jepa_amd.src.models.attentive_pooler import AttentiveClassifier
    torch.manual_seed(seed)
    m = AttentiveClassifier(embed_dim=D, num_heads=H, depth=1, num_classes=C)
    with torch.no_grad():
        for p in m.parameters():     # non-trivial biases and LayerNorm affines (0 / 1 at init)
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    return m.to(DEV)


def _inputs(B, N, D, seed=11):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, D, generator=g).to(torch.bfloat16)
    labels = torch.randint(0, C, (B,), generator=g)
    return x, labels


def _oracle_dx(m, x, labels, H):
    from oracle import probe_oracle as po
    w = {n: p.detach().double().cpu() for n, p in m.named_parameters()}
    xd = x.double().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(po.attentive_classifier(w, xd, H), labels)
    loss.backward()
    return xd.grad


def test_split_threshold_is_the_one_named():
    from jepa_amd.hip.lib import load_library
    lib = load_library()
    assert lib.vj_xattn_ws_bytes(2, 1, N_SPLIT - 1, 2, 32, 1) == 0
    assert lib.vj_xattn_ws_bytes(2, 1, N_SPLIT, 2, 32, 1) > 0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-N%d-D%d-H%d" % s)
def test_feature_gradient_against_float64(shape):
    B, N, D, H = shape
    m = _probe(D, H)
    x, labels = _inputs(B, N, D)
    xg = x.to(DEV).requires_grad_()
    loss = torch.nn.functional.cross_entropy(m(xg), labels.to(DEV))
    loss.backward()
    assert xg.grad is not None and xg.grad.shape == x.shape and xg.grad.dtype == torch.bfloat16
    ref = _oracle_dx(m, x, labels, H)
    errs = [rel_l2(xg.grad[b], ref[b]) for b in range(B)]
    print("dX rel-L2 per sample", shape, errs)
    assert max(errs) < BOUND, (shape, errs)


def test_sample_without_loss_gradient_gets_exactly_zero():
    B, N, D, H = 3, 65, 64, 2
    m = _probe(D, H)
    x, _ = _inputs(B, N, D)
    xg = x.to(DEV).requires_grad_()
    dlogits = torch.randn(B, C, generator=torch.Generator().manual_seed(2)).to(DEV)
    dlogits[1] = 0
    m(xg).backward(dlogits)
    assert torch.count_nonzero(xg.grad[1]) == 0
    assert torch.count_nonzero(xg.grad[0]) > 0 and torch.count_nonzero(xg.grad[2]) > 0


@pytest.mark.parametrize("shape", [(2, 65, 64, 2), (3, 257, 96, 4)], ids=lambda s: "B%d-N%d-D%d-H%d" % s)
def test_parameter_gradients_and_logits_do_not_depend_on_the_feature_gradient(shape):
    B, N, D, H = shape
    m = _probe(D, H)
    x, labels = _inputs(B, N, D)
    out = []
    for need in (False, True):
        m.zero_grad(set_to_none=True)
        xg = x.to(DEV).requires_grad_(need)
        logits = m(xg)
        torch.nn.functional.cross_entropy(logits, labels.to(DEV)).backward()
        assert (xg.grad is not None) == need
        out.append((logits.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
    (l0, g0), (l1, g1) = out
    assert torch.equal(l0, l1)
    assert g0.keys() == g1.keys() and len(g0) == 15
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gradient_has_the_features_shape_and_dtype(dtype):
    B, N, D, H = 2, 63, 64, 2
    m = _probe(D, H)
    x, labels = _inputs(B, N, D)
    xg = x.to(DEV).to(dtype).requires_grad_()
    torch.nn.functional.cross_entropy(m(xg), labels.to(DEV)).backward()
    assert xg.grad.dtype == dtype and xg.grad.shape == (B, N, D)
    if dtype == torch.float32:     # the same bf16 values: the cast is the only difference
        xb = x.to(DEV).requires_grad_()
        m.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(m(xb), labels.to(DEV)).backward()
        assert torch.equal(xg.grad, xb.grad.float())


def test_bank_still_refuses_features_that_require_grad():
    from jepa_amd.src.models.attentive_pooler import AttentiveClassifierBank
    bank = AttentiveClassifierBank(embed_dim=64, num_heads=2, num_classes=C, num_probes=2).to(DEV)
    x, _ = _inputs(2, 17, 64)
    with pytest.raises(NotImplementedError, match="trainable encoder"):
        bank(x.to(DEV).requires_grad_())
    with torch.no_grad():
        assert bank(x.to(DEV).requires_grad_()).shape == (2, 2, C)
