"""GPU: the probe's cross-attention past the single-workgroup key limits (vj_xattn_fwd_ws / vj_xattn_bwd_ws).

The single-workgroup kernels hold every score of a (sample, head) in LDS: the forward serves N <= 38 264 keys, the backward
N <= 19 132.  Above those limits the _ws entry points run the split-key kernels.  Checked against fp32
F.scaled_dot_product_attention with the bounds of tests/test_probe_gpu.py::test_xattn_kernel_against_sdpa; at and below the
limits the _ws entry points must give the bits of the original pair."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD_MAX, BWD_MAX = 38264, 19132


def rel_l2(a, b):
    a, b = a.detach().float().reshape(-1), b.detach().float().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-12))


def _inputs(B, NQ, N, H, hd, shared, seed):
    g = torch.Generator().manual_seed(seed)
    D = H * hd
    q = torch.randn(1 if shared else B, NQ, D, generator=g).to(torch.bfloat16).to(DEV)
    kv = torch.randn(B * N, 2 * D, generator=g).to(torch.bfloat16).to(DEV)
    resid = torch.randn(NQ, D, generator=g).to(torch.bfloat16).to(DEV)
    dy = torch.randn(B, D, generator=g).to(torch.bfloat16).to(DEV)
    return q, kv, resid, dy


# (B, N, H, hd, shared q): the split backward runs at every N here; the split forward only at 38 265 and 73 728, so 24 000 and
# 36 864 pair the single-workgroup forward with the split backward (the ViT-H/16-384 K400 probe: 8 x 4608 keys)
CASES = [(1, 19133, 2, 32, False), (4, 24000, 2, 80, True), (4, 36864, 2, 64, False), (1, 36864, 1, 128, True),
         (1, 38265, 2, 128, True), (4, 38265, 1, 32, False), (4, 73728, 1, 64, True), (1, 73728, 2, 80, False),
         # the split forms at their smallest N with one 8-column chunk per row (hd = 8) and three (hd = 24); then 20 chunks of exactly
         # XA_CHUNK = 2048 keys: the last chunk is full, where every case above has a ragged one
         (2, 19133, 1, 8, True), (2, 19133, 1, 24, False), (1, 38265, 1, 8, False), (1, 38265, 1, 24, True),
         (2, 40960, 2, 64, False)]


@pytest.mark.parametrize("B,N,H,hd,shared", CASES)
def test_split_xattn_against_sdpa(B, N, H, hd, shared):
    from jepa_amd.hip import ops
    from jepa_amd.hip.lib import load_library
    lib = load_library()
    assert lib.vj_xattn_ws_bytes(B, 1, N, H, hd, 1) > 0                        # the split backward runs
    assert (lib.vj_xattn_ws_bytes(B, 1, N, H, hd, 0) > 0) == (N > FWD_MAX)      # the split forward only above its own limit
    D, scale = H * hd, hd ** -0.5
    for NQ in (3, 1):
        q, kv, resid, dy = _inputs(B, NQ, N, H, hd, shared, seed=N + hd + NQ)
        qs = q.reshape(-1, D) if shared else q.reshape(B * NQ, D)
        out, lse = ops.xattn_fwd(qs, kv, B, NQ, N, H, hd, scale, resid=resid, shared_q=shared)
        qf = q.float().expand(B, NQ, D).reshape(B, NQ, H, hd).permute(0, 2, 1, 3).contiguous().requires_grad_(True)
        kvf = kv.float().reshape(B, N, 2, H, hd).permute(2, 0, 3, 1, 4)
        kf, vf = kvf[0].detach().requires_grad_(True), kvf[1].detach().requires_grad_(True)
        ref = torch.nn.functional.scaled_dot_product_attention(qf, kf, vf)
        full = ref.detach() + resid.float().reshape(1, NQ, H, hd).permute(0, 2, 1, 3)
        e = rel_l2(out.reshape(B, NQ, H, hd).permute(0, 2, 1, 3), full)
        assert e < 8e-3, ("out", NQ, e)
        lse_ref = torch.logsumexp(torch.einsum("bhqd,bhkd->bhqk", qf.detach(), kf.detach()) * scale, dim=-1) / math.log(2.0)
        assert torch.allclose(lse.reshape(B, H, NQ), lse_ref.reshape(B, H, NQ), atol=2e-3, rtol=1e-4)
        out2, lse2 = ops.xattn_fwd(qs, kv, B, NQ, N, H, hd, scale, resid=resid, shared_q=shared)
        assert torch.equal(out, out2) and torch.equal(lse, lse2)               # deterministic
        if NQ != 1:
            continue
        dq, dkv = ops.xattn_bwd(qs, kv, dy, lse, B, N, H, hd, scale, shared_q=shared)
        ref.backward(dy.float().reshape(B, 1, H, hd).permute(0, 2, 1, 3))
        e = rel_l2(dq.reshape(B, 1, H, hd).permute(0, 2, 1, 3), qf.grad)
        assert e < 1.5e-2, ("dq", e)
        dkvv = dkv.float().reshape(B, N, 2, H, hd).permute(2, 0, 3, 1, 4)
        assert rel_l2(dkvv[0], kf.grad) < 1.5e-2, ("dk", rel_l2(dkvv[0], kf.grad))
        assert rel_l2(dkvv[1], vf.grad) < 1.5e-2, ("dv", rel_l2(dkvv[1], vf.grad))
        dq2, dkv2 = ops.xattn_bwd(qs, kv, dy, lse, B, N, H, hd, scale, shared_q=shared)
        assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2)                 # deterministic: no atomics anywhere


@pytest.mark.parametrize("N", [1568, BWD_MAX])
def test_ws_entry_points_keep_the_bits_within_the_limits(N):
    """Within the limits the _ws forms launch the single-workgroup kernels: no workspace, the exact bits of vj_xattn_fwd / _bwd."""
    from jepa_amd.hip import ops
    from jepa_amd.hip.lib import check, load_library
    lib = load_library()
    B, H, hd, NQ = 2, 4, 64, 1
    D, scale = H * hd, hd ** -0.5
    assert lib.vj_xattn_ws_bytes(B, NQ, N, H, hd, 0) == 0 and lib.vj_xattn_ws_bytes(B, NQ, N, H, hd, 1) == 0
    q, kv, resid, dy = _inputs(B, NQ, N, H, hd, True, seed=N)
    qs = q.reshape(NQ, D)
    out_ws, lse_ws = ops.xattn_fwd(qs, kv, B, NQ, N, H, hd, scale, resid=resid)
    dq_ws, dkv_ws = ops.xattn_bwd(qs, kv, dy, lse_ws, B, N, H, hd, scale)
    out = torch.empty_like(out_ws)
    lse = torch.empty_like(lse_ws)
    dq, dkv = torch.empty_like(dq_ws), torch.empty_like(dkv_ws)
    s = ops._stream()
    check(lib.vj_xattn_fwd(ops._ptr(qs), 0, ops._ptr(kv), ops._ptr(resid), ops._ptr(out), ops._ptr(lse), B, NQ, N, H, hd, scale, s),
          "vj_xattn_fwd")
    check(lib.vj_xattn_bwd(ops._ptr(qs), 0, ops._ptr(kv), ops._ptr(dy), ops._ptr(lse), ops._ptr(dq), ops._ptr(dkv), B, 1, N, H, hd,
                           scale, s), "vj_xattn_bwd")
    assert torch.equal(out, out_ws) and torch.equal(lse, lse_ws)
    assert torch.equal(dq, dq_ws) and torch.equal(dkv, dkv_ws)


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("hd", [16, 64])
@pytest.mark.parametrize("N", [256, 1024, 32768, 65536])
def test_xattn_exact_on_zero_query(N, hd, shared):
    """An exact pin that holds in any summation order: with q = 0 every score is exactly 0, every p exactly 1 and their sum exactly N
    (a power of two); with integer V in [-4, 4] the sum of the v_j is an integer below 2^24.  So out is V.sum / N + resid to the bit,
    whichever chunk, key or head a workgroup starts from -- and a wrong start shows.  N = 256, 1024: the single-workgroup kernels;
    32 768: the single-workgroup forward with the split backward; 65 536: both split.
    Backward: dk = scale dS q is 0 everywhere; dv_j = p dy with p = 2^(-lse2): one bf16 rounding (2^-8) of dy / N, plus 1e-5 for p
    (lse2 within 2 fp32 ulps of 16: 16 * 2 * 2^-24 * ln 2 = 2.8e-6)."""
    from jepa_amd.hip import ops
    B, H = 2, 2
    D, scale = H * hd, hd ** -0.5
    g = torch.Generator().manual_seed(N + hd)
    q = torch.zeros(1 if shared else B, D, dtype=torch.bfloat16, device=DEV)
    k = torch.randn(B, N, H, hd, generator=g)
    v = torch.randint(-4, 5, (B, N, H, hd), generator=g).float()
    kv = torch.stack([k, v], dim=2).reshape(B * N, 2 * D).to(torch.bfloat16).to(DEV)
    resid = torch.randn(1, D, generator=g).to(torch.bfloat16).to(DEV)
    dy = torch.randn(B, D, generator=g).to(torch.bfloat16).to(DEV)
    out, lse = ops.xattn_fwd(q, kv, B, 1, N, H, hd, scale, resid=resid, shared_q=shared)
    kvf = kv.float().reshape(B, N, 2, D)
    expect = (kvf[:, :, 1].sum(dim=1) / N + resid.float()).to(torch.bfloat16)
    print("out elements that differ", int((out != expect).sum()), "lse2", lse.min().item(), lse.max().item())
    assert torch.equal(out, expect)
    assert torch.allclose(lse, torch.full_like(lse, math.log2(N)), atol=2e-3, rtol=1e-4)
    dq, dkv = ops.xattn_bwd(q, kv, dy, lse, B, N, H, hd, scale, shared_q=shared)
    dkv = dkv.reshape(B, N, 2, D)
    assert bool((dkv[:, :, 0] == 0).all())                                    # signed zeros compare equal
    want = (dy.double() / N).reshape(B, 1, D)
    excess = ((dkv[:, :, 1].double() - want).abs() - want.abs() * (2.0 ** -8 + 1e-5)).max().item()
    print("dv worst excess over the bound", excess)
    assert excess <= 0
    # dq against float64 attention on the same inputs, differentiated by autograd
    qd = q.double().expand(B, D).reshape(B, H, 1, hd).clone().requires_grad_(True)
    kd, vd = kvf.double().reshape(B, N, 2, H, hd).permute(2, 0, 3, 1, 4)
    ref = torch.softmax(qd @ kd.transpose(-1, -2) * scale, dim=-1) @ vd
    ref.backward(dy.double().reshape(B, H, 1, hd))
    e = rel_l2(dq.reshape(B, H, 1, hd).double(), qd.grad)
    print("dq", e)
    assert e < 1.5e-2, ("dq", e)
