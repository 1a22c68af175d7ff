"""The kernels of csrc/layernorm.hip (LayerNorm forward / backward + column sums of dx, row statistics, target rows), csrc/loss.hip
(latent loss, token_pstd, reg_grad, reg_finish; reference app/vjepa/train.py:424-459) and csrc/optim.hip (fused AdamW + EMA + bf16
re-cast, its guarded form, EMA alone, the bf16 cast and the gradient norm; train.py:461-487) against PyTorch references: fp32
tolerances where the arithmetic rounds, torch.equal where the inputs are chosen so that every intermediate is exact."""
import math
import pytest
import torch
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.golden_util import rel_l2  # noqa: E402
from tests.step_util import TINY, TINY_MASKS, build_trainer, draw_batch, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu


DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from jepa_amd.hip import ops as _ops
    return _ops


def rel_l2(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def bf(x):
    return x.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------ layernorm
# NCH = 1..4, a last chunk that only part of the lanes own (504, 520, 1032, 1544), one lane (8), fewer rows than waves;
# 17 rows give the backward two workgroups of 9 and 8 rows
LN_EDGES = [(1, 8), (3, 504), (3, 512), (17, 520), (17, 1032), (3, 1544), (5, 2048)]
LN_CASES = [(40, 192), (473, 1024), (1000, 384), (7, 1280), (5, 96)] + LN_EDGES


@pytest.mark.parametrize("rows,D", LN_CASES)
def test_layernorm_fwd_bwd(ops, rows, D):
    g = torch.Generator().manual_seed(5)
    x = bf(torch.randn(rows, D, generator=g) * 2 + 0.3).to(DEV)
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(D, generator=g)).to(DEV)
    dy = bf(torch.randn(rows, D, generator=g)).to(DEV)
    dres = bf(torch.randn(rows, D, generator=g)).to(DEV)
    eps = 1e-6
    y, mean, rstd = ops.layernorm_fwd(x, gamma, beta, eps)
    xr = x.float().requires_grad_(True)
    gr = gamma.clone().requires_grad_(True)
    br = beta.clone().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xr, (D,), gr, br, eps)
    assert rel_l2(y, yr) < 4e-3, rel_l2(y, yr)
    assert torch.allclose(mean, x.float().mean(-1), rtol=1e-4, atol=1e-5)
    yr.backward(dy.float())
    dgamma = torch.zeros(D, device=DEV)
    dbeta = torch.zeros(D, device=DEV)
    dx = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta, dres=dres)
    assert rel_l2(dx, xr.grad + dres.float()) < 6e-3, rel_l2(dx, xr.grad + dres.float())
    assert rel_l2(dgamma, gr.grad) < 1e-4, rel_l2(dgamma, gr.grad)
    assert rel_l2(dbeta, br.grad) < 1e-4, rel_l2(dbeta, br.grad)
    # accumulate + alpha
    dx2 = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta, alpha=2.0, accumulate=True)
    assert rel_l2(dgamma, 3 * gr.grad) < 1e-4
    assert rel_l2(dx2, xr.grad) < 6e-3


@pytest.mark.parametrize("rows,D", LN_CASES)
def test_ln_rowstats_equal_layernorm_fwd_statistics(ops, rows, D):
    """The folded-LayerNorm path of the target encoder takes {rstd, -mean * rstd} from ln_rowstats where the unfolded path takes mean and
    rstd from layernorm_fwd: the two kernels must produce the same statistics bit for bit (the product rounds once, in fp32)."""
    g = torch.Generator().manual_seed(5)
    x = bf(torch.randn(rows, D, generator=g) * 2 + 0.3).to(DEV)
    _, mean, rstd = ops.layernorm_fwd(x, torch.ones(D, device=DEV), torch.zeros(D, device=DEV), 1e-6)
    rs = ops.ln_rowstats(x, 1e-6)
    assert torch.equal(rs[:, 0], rstd)
    assert torch.equal(rs[:, 1], -(mean * rstd))


# ------------------------------------------------------------------------------------------------ LayerNorm backward + column sums
# (16385, 8): the cap of 1024 workgroups leaves 17 rows per workgroup and the trailing workgroups without a row; their partial rows are zeros
@pytest.mark.parametrize("rows,D", [(10560, 1024), (5533, 384), (777, 1280), (40, 192), (16385, 8)])
def test_layernorm_bwd_column_sums_of_dx(rows, D):
    """vj_layernorm_bwd_colsum: dx / dgamma / dbeta equal to the plain backward (up to fp contraction in a separately
    compiled variant); dxsum = alpha * column sums of dx
    (accumulated in fp32 BEFORE the bf16 rounding of dx) within 2e-3 relative of the fp32 sum of the rounded dx, and
    accumulating (beta = 1) adds to the previous value."""
    from jepa_amd.hip import ops
    g = torch.Generator(device=DEV).manual_seed(rows + D)
    x = torch.randn(rows, D, device=DEV, generator=g).to(torch.bfloat16)
    dy = torch.randn(rows, D, device=DEV, generator=g).to(torch.bfloat16)
    dres = torch.randn(rows, D, device=DEV, generator=g).to(torch.bfloat16)
    gamma = torch.randn(D, device=DEV, generator=g)
    beta = torch.randn(D, device=DEV, generator=g)
    _, mean, rstd = ops.layernorm_fwd(x, gamma, beta, 1e-6)
    outs = []
    for with_cs in (False, True):
        dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
        cs = torch.full((D,), 3.0, device=DEV) if with_cs else None
        dx = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dg, db, dres=dres, alpha=0.5, dxsum=cs)
        if with_cs:
            first = cs.clone()
            ops.layernorm_bwd(dy, x, gamma, mean, rstd, dg, db, dres=dres, alpha=0.5, accumulate=True, dxsum=cs)
            assert torch.allclose(cs, 2 * first, rtol=1e-6, atol=1e-6)
            cs = first
        outs.append((dx, dg.clone(), db.clone(), cs))
    # the two template variants are compiled separately under -ffp-contract=fast: dx may differ by one bf16 ulp in a few
    # elements, never more (C chain and Python chain call the same variant for the same tensor: their bit-identity holds)
    da, dbb = outs[0][0].float(), outs[1][0].float()
    frac = float((da != dbb).float().mean())
    print(f"layernorm_bwd colsum variant vs plain, rows={rows} D={D}: {100 * frac:.4f} % of dx elements differ, rel-L2 "
          f"{float((da - dbb).norm() / da.norm()):.2e}")
    assert frac < 2e-3 and float((da - dbb).norm() / da.norm()) < 2e-4
    ref = 0.5 * outs[1][0].float().sum(0)
    err = float((outs[1][3] - ref).norm() / ref.norm())
    assert err < 2e-3, err
    # the first call of the with_cs arm ran with beta = 0: dgamma/dbeta equal the plain call's halves after the accumulate
    assert torch.allclose(outs[1][1], 2 * outs[0][1], rtol=1e-6, atol=1e-5)
    assert torch.allclose(outs[1][2], 2 * outs[0][2], rtol=1e-6, atol=1e-5)


@pytest.mark.parametrize("B,N,K,D", [(2, 64, 32, 192), (1, 5, 3, 1032), (3, 7, 7, 2048)])
def test_target_rows_and_loss(ops, B, N, K, D):
    g = torch.Generator().manual_seed(12)
    x = bf(torch.randn(B * N, D, generator=g) * 3).to(DEV)
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(D, generator=g)).to(DEV)
    idx = torch.stack([torch.randperm(N, generator=g)[:K].sort().values for _ in range(B)]).to(DEV)
    h = ops.target_rows(x, gamma, beta, idx, B, N, 1e-6)
    F = torch.nn.functional
    hr = F.layer_norm(F.layer_norm(x.float().view(B, N, D), (D,), gamma, beta, 1e-6), (D,))
    hr = torch.gather(hr, 1, idx.unsqueeze(-1).repeat(1, 1, D))
    assert torch.allclose(h, hr, rtol=1e-4, atol=1e-4), (h - hr).abs().max()
    z = bf(torch.randn(B * K, D, generator=g)).to(DEV)
    loss = torch.zeros(1, device=DEV)
    dz = torch.empty_like(z)
    numel = z.numel()
    ops.latent_loss(z, h, loss, p=1.0, out_scale=1.0 / numel, dz=dz, gscale=0.25)
    ref = (z.float().view(B, K, D) - hr).abs().mean()
    assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item()) + 1e-7
    assert torch.equal(dz.float().view(B, K, D), 0.25 * torch.sign(z.float().view(B, K, D) - h))
    loss2 = torch.ones(1, device=DEV)
    ops.latent_loss(z, h, loss2, p=2.0, out_scale=1.0 / numel, accumulate=True)
    ref2 = 1.0 + ((z.float().view(B, K, D) - hr).abs() ** 2).mean() / 2
    assert abs(loss2.item() - ref2.item()) < 1e-4 * ref2.item()
    # variance regulariser (reg_fn)
    pstd = torch.zeros(B, D, device=DEV)
    ops.token_pstd(z, pstd, B, K, D, False)
    ref_p = torch.sqrt(z.float().view(B, K, D).var(dim=1) + 1e-4)
    assert torch.allclose(pstd, ref_p, rtol=1e-4, atol=1e-5)
    out = torch.zeros(1, device=DEV)
    ops.reg_finish(pstd, 1, out)
    assert abs(out.item() - torch.relu(1 - ref_p).mean().item()) < 1e-5


def test_adamw_ema_matches_torch(ops):
    g = torch.Generator().manual_seed(13)
    n = 4096 + 64
    p0 = torch.randn(n, generator=g)
    tgt0 = p0.clone()
    pr = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pr], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    p = p0.clone().to(DEV)
    m = torch.zeros(n, device=DEV)
    v = torch.zeros(n, device=DEV)
    tgt = tgt0.clone().to(DEV)
    pb = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    tb = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    tr = tgt0.clone()
    for step in range(1, 4):
        grad = torch.randn(n, generator=g)
        pr.grad = grad.clone()
        opt.step()
        tr.mul_(0.998).add_((1 - 0.998) * pr.detach())
        ops.adamw_ema(p, grad.to(DEV), m, v, pb, tgt, tb, 1e-3, 0.05, 0.9, 0.999, 1e-8, step, 1.0, 0.998)
    assert torch.allclose(p.cpu(), pr.detach(), rtol=1e-5, atol=1e-6), (p.cpu() - pr.detach()).abs().max()
    assert torch.allclose(tgt.cpu(), tr, rtol=1e-5, atol=1e-6)
    assert torch.equal(pb, bf(p))
    assert torch.equal(tb, bf(tgt))
    out2 = torch.zeros(2, device=DEV)
    ops.sqnorm(p, out2)
    assert abs(out2[0].item() - (p.double() ** 2).sum().item()) < 1e-4 * out2[0].item()
    assert out2[1].item() == 0
    p[3] = float("nan")
    ops.sqnorm(p, out2)
    assert out2[1].item() == 1


# ------------------------------------------------------------------------------------------ loss.hip, per op
def _int_pair(numel, seed):
    """z: bf16 integers in [-8, 8], h: fp32 integers in [-8, 8]: |z - h| <= 16 and every sum of them below 2^24 is exact in fp32"""
    g = torch.Generator().manual_seed(seed)
    z = bf(torch.randint(-8, 9, (numel,), generator=g).float()).to(DEV)
    h = torch.randint(-8, 9, (numel,), generator=g).float().to(DEV)
    return z, h


# numel = 40: n8 = 5, most of the 512 workgroups see nothing; 8 * (512 * 256 + 7): every thread one chunk, seven a second one
@pytest.mark.parametrize("numel", [40, 8 * (512 * 256 + 7)])
def test_latent_loss_exact_on_integers(ops, numel):
    z, h = _int_pair(numel, 21)
    d = z.double() - h.double()
    # p = 1: integer partial sums, out_scale a power of two: the result is exact whatever the order of the reduction
    ref = float(d.abs().sum()) * 2.0 ** -10
    loss = torch.full((1,), -5.0, device=DEV)
    dz = torch.empty_like(z)
    ops.latent_loss(z, h, loss, p=1.0, out_scale=2.0 ** -10, dz=dz, gscale=0.25)
    assert loss.item() == ref, (loss.item(), ref)
    assert torch.equal(dz.float(), 0.25 * torch.sign(z.float() - h))
    loss = torch.full((1,), 3.0, device=DEV)
    ops.latent_loss(z, h, loss, p=1.0, out_scale=2.0 ** -10, accumulate=True)
    assert loss.item() == 3.0 + ref, (loss.item(), 3.0 + ref)
    # p = 2: __powf rounds; the loss to 1e-4, dz within one bf16 rounding (2^-9 relative) + the error of __powf (orders below it for
    # |d| <= 16) of sign * |d| * gscale
    ref2 = float((d * d).sum()) / 2 * 2.0 ** -10
    loss = torch.zeros(1, device=DEV)
    ops.latent_loss(z, h, loss, p=2.0, out_scale=2.0 ** -10, dz=dz, gscale=0.25)
    assert abs(loss.item() - ref2) < 1e-4 * ref2, (loss.item(), ref2)
    refdz = d * 0.25
    err = (dz.double() - refdz).abs()
    print(f"latent_loss p=2 numel={numel}: loss rel err {abs(loss.item() - ref2) / ref2:.2e}, "
          f"max dz err / |ref| {float((err / refdz.abs().clamp_min(1e-30)).max()):.2e}")
    assert bool((err <= 2.0 ** -8 * refdz.abs()).all())


def test_token_pstd_stats_and_accumulate(ops):
    """D = 72: the second 64-column slab is partly empty.  stats[b, d] = {token mean, sqrt(var + 1e-4)} of this call; a second, accumulating
    call adds the same value again."""
    B, K, D = 2, 5, 72
    g = torch.Generator().manual_seed(22)
    z = bf(torch.randn(B, K, D, generator=g)).to(DEV)
    pstd = torch.full((B, D), 7.0, device=DEV)
    stats = torch.full((B, D, 2), 7.0, device=DEV)
    ops.token_pstd(z, pstd, B, K, D, False, stats=stats)
    first = pstd.clone()
    ops.token_pstd(z, pstd, B, K, D, True, stats=stats)
    assert torch.equal(pstd, 2 * first)
    ref_std = torch.sqrt(z.double().var(dim=1) + 1e-4)
    assert torch.allclose(first.double(), ref_std, rtol=1e-4, atol=1e-5)
    assert torch.allclose(stats[..., 0].double(), z.double().mean(dim=1), rtol=1e-4, atol=1e-5)
    assert torch.allclose(stats[..., 1].double(), ref_std, rtol=1e-4, atol=1e-5)


def test_reg_grad_against_float64(ops):
    """dz -= coef * active * (z - stats0) / ((K - 1) * stats1), active = [pstd_sum / n_masks < 1], from the kernel's own inputs in float64.
    Bound per element: one bf16 rounding of the result (2^-8 |ref|, a factor 2 to spare) + a handful of fp32 roundings of the operands
    (2^-24 each; 2^-20 (|dz| + |term|) leaves a factor 16)."""
    B, K, D, n_masks = 2, 5, 72, 2
    g = torch.Generator().manual_seed(23)
    z = bf(torch.randn(B, K, D, generator=g)).to(DEV)
    dz0 = bf(torch.randn(B, K, D, generator=g)).to(DEV)
    below = torch.rand(B, D, generator=g) < 0.5
    u = torch.rand(B, D, generator=g)
    pstd_sum = torch.where(below, 0.5 + 1.4 * u, 2.1 + 1.4 * u).to(DEV)    # both sides of n_masks, none within 1e-3 of it
    assert below.any() and not below.all() and bool(((pstd_sum - n_masks).abs() > 1e-3).all())
    stats = torch.stack([torch.randn(B, D, generator=g), 0.5 + torch.rand(B, D, generator=g)], dim=-1).contiguous().to(DEV)
    coef = 0.375
    dz = dz0.clone()
    ops.reg_grad(z, pstd_sum, stats, dz, B, K, D, n_masks, coef)
    active = (pstd_sum.double() / n_masks < 1.0).double().unsqueeze(1)
    term = coef * active * (z.double() - stats[..., 0].double().unsqueeze(1)) / ((K - 1) * stats[..., 1].double().unsqueeze(1))
    ref = dz0.double() - term
    err = (dz.double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -20 * (dz0.double().abs() + term.abs())
    print(f"reg_grad: max err / bound {float((err / bound.clamp_min(1e-30)).max()):.3f}")
    assert bool((err <= bound).all())
    off = (active == 0).expand(B, K, D)
    assert bool(off.any()) and torch.equal(dz[off], dz0[off])


# ------------------------------------------------------------------------------------------ optim.hip, per op
def _specials():
    return torch.tensor([float("inf"), float("-inf"), 0.0, -0.0, 1e-40, -1e-40, float("nan"), 1.5])


# n = 4: one thread; 4 * (2048 * 256 + 3): past the cap of 2048 workgroups, so the kernel strides
@pytest.mark.parametrize("n", [4, 4 * (2048 * 256 + 3)])
def test_cast_f32_to_bf16_equals_torch(ops, n):
    g = torch.Generator().manual_seed(24)
    sp = _specials()
    srcs = [sp[:4].clone(), sp[4:].clone()] if n == 4 else [torch.randn(n, generator=g)]
    if n > 4:
        srcs[0][:8] = sp
        srcs[0][-8:] = sp
    for src in srcs:
        src = src.to(DEV)
        out = torch.full((n,), 3.0, dtype=torch.bfloat16, device=DEV)
        ops.cast_bf16(src, out)
        ref = src.to(torch.bfloat16)
        nan = torch.isnan(ref)
        assert torch.equal(torch.isnan(out), nan)
        assert torch.equal(out[~nan], ref[~nan])
        assert torch.equal(torch.signbit(out[~nan]), torch.signbit(ref[~nan]))


def _int_weights(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-512, 513, (n,), generator=g).float().to(DEV), torch.randint(-512, 513, (n,), generator=g).float().to(DEV))


@pytest.mark.parametrize("shadow", [True, False])
def test_ema_update_exact(ops, shadow):
    """m = 0.5 on integers in [-512, 512]: every product and sum is exact in fp32 however the compiler contracts them"""
    n = 4 * 259
    tgt0, src = _int_weights(n, 25)
    tgt = tgt0.clone()
    tb = torch.full((n,), 3.0, dtype=torch.bfloat16, device=DEV) if shadow else None
    ops.ema_update(tgt, src, tb, 0.5)
    assert torch.equal(tgt, 0.5 * tgt0 + 0.5 * src)
    if shadow:
        assert torch.equal(tb, bf(tgt))


def test_adamw_ema_guarded_skips_on_nonfinite(ops):
    """gstat[1] > 0 (a non-finite gradient was seen): no optimizer step, no step count; the EMA still runs, against the unchanged weights"""
    n = 4 * 259
    tgt0, p0 = _int_weights(n, 25)
    g = torch.Generator().manual_seed(26)
    grad = torch.randn(n, generator=g).to(DEV)
    m0, v0 = torch.randn(n, generator=g).to(DEV), torch.rand(n, generator=g).to(DEV)
    p, m, v, tgt = p0.clone(), m0.clone(), v0.clone(), tgt0.clone()
    pb0 = torch.full((n,), 3.0, dtype=torch.bfloat16, device=DEV)
    pb, tb = pb0.clone(), torch.full((n,), 3.0, dtype=torch.bfloat16, device=DEV)
    gstat = torch.tensor([16.0, 1.0, 0.0, 0.0], device=DEV)
    step_dev = torch.full((1,), 2.0, device=DEV)
    ops.step_advance(gstat, step_dev)
    ops.adamw_ema_guarded(p, grad, m, v, pb, tgt, tb, 1e-3, 0.05, 0.9, 0.999, 1e-8, 1.0, 0.5, gstat, 0, 0.5, 0.5, step_dev)
    assert step_dev.item() == 2.0
    assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0) and torch.equal(pb, pb0)
    assert torch.equal(tgt, 0.5 * tgt0 + 0.5 * p0)
    assert torch.equal(tb, bf(tgt))


def test_adamw_ema_guarded_clips_like_torch(ops):
    """gstat = [s, 0, 0, 0] with sqrt(s) * norm_scale = 4 * clip: the step of torch.optim.AdamW on grad * clip / (4 * clip + 1e-6), the
    step count advanced on the device (the bounds of test_adamw_ema_matches_torch)"""
    g = torch.Generator().manual_seed(27)
    n = 4096 + 64
    clip, norm_scale, s = 0.5, 0.5, 16.0
    p0 = torch.randn(n, generator=g)
    pr = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pr], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    p, tgt = p0.clone().to(DEV), p0.clone().to(DEV)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    pb = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    tb = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    tr = p0.clone()
    gstat = torch.tensor([s, 0.0, 0.0, 0.0], device=DEV)
    step_dev = torch.zeros(1, device=DEV)
    for _ in range(3):
        grad = torch.randn(n, generator=g)
        pr.grad = grad * (clip / (4 * clip + 1e-6))
        opt.step()
        tr.mul_(0.998).add_((1 - 0.998) * pr.detach())
        ops.step_advance(gstat, step_dev)
        ops.adamw_ema_guarded(p, grad.to(DEV), m, v, pb, tgt, tb, 1e-3, 0.05, 0.9, 0.999, 1e-8, 1.0, 0.998, gstat, 0, clip, norm_scale,
                              step_dev)
    assert step_dev.item() == 3.0
    assert torch.allclose(p.cpu(), pr.detach(), rtol=1e-5, atol=1e-6), (p.cpu() - pr.detach()).abs().max()
    assert torch.allclose(tgt.cpu(), tr, rtol=1e-5, atol=1e-6)
    assert torch.equal(pb, bf(p))
    assert torch.equal(tb, bf(tgt))


# n = 4: one thread of 1024 workgroups; 4 * (1024 * 256 + 5): every thread one float4, five a second one
@pytest.mark.parametrize("n", [4, 4 * (1024 * 256 + 5)])
def test_sqnorm_exact_on_integers(ops, n):
    g = torch.Generator().manual_seed(28)
    x = torch.randint(-2, 3, (n,), generator=g).float().to(DEV)
    s = float((x.double() ** 2).sum())
    out = torch.full((2,), 9.0, device=DEV)
    ops.sqnorm(x, out)
    assert out.tolist() == [s, 0.0], (out.tolist(), s)
    ops.sqnorm(x, out, accumulate=True)
    assert out.tolist() == [2 * s, 0.0]
    x[1] = float("nan")
    x[n - 2] = float("inf")
    ops.sqnorm(x, out)
    assert out[1].item() == 2.0
    ops.sqnorm(x, out, accumulate=True)
    assert out[1].item() == 4.0
