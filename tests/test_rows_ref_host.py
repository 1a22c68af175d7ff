"""CPU: the references, data and case lists of tests/rows_ref_util.py hold what tests/test_rows_elementwise_gpu.py relies on.

Every reference agrees with an independent spelling (torch.gather / scatter_, Conv3d, explicit loops); the bit patterns of the movers
contain what they claim and survive the round trip through their float dtype; the guarded allocation notices a stray write.  For every
summing case: the integer data meet the precondition under which fp32 sums are exact in any order (max sum|x| < 2^24, the result a
multiple of 0.5 below 2^23), and plain fp32 sums in three orders then EQUAL the float64 reference while a dropped, doubled or
mis-windowed row does not; on the normal draws the same fp32 sums stay inside the derived bound, and a dropped row leaves it wherever the
bound is smaller than a row (asserted below: up to 1170 rows; beyond that sum|x| * gamma exceeds one element, and the integer data are the
check that misses no row)."""
import pytest
import torch

from tests import rows_ref_util as R
from tests.rows_ref_util import BF16, F32


# ------------------------------------------------------------------------------------------------ guards and bit patterns
def test_embedded_notices_writes_outside_the_view():
    e = R.Embedded((3, 8), BF16, "cpu", float("nan"), shift=2)
    assert e.view.shape == (3, 8) and e.lo == 66 and e.flat.numel() == 64 + 2 + 24 + 64
    assert bool(torch.isnan(e.flat.float()).all()) and e.guards_untouched()
    e.put(torch.ones(3, 8, dtype=BF16))
    assert e.guards_untouched() and bool((e.flat[e.lo:e.hi] == 1).all())
    for pos in (0, e.lo - 1, e.hi, e.flat.numel() - 1):
        keep = e.flat[pos].clone()
        e.flat[pos] = 0.0
        assert not e.guards_untouched()
        e.flat[pos] = keep
        assert e.guards_untouched()
    o = R.Embedded((4,), F32, "cpu", -7.0, inner=float("nan"))
    assert bool(torch.isnan(o.view).all()) and bool((o.flat[:64] == -7.0).all()) and bool((o.flat[68:] == -7.0).all())
    o.flat.view(torch.int32)[70] ^= 1                                  # one bit of a sentinel
    assert not o.guards_untouched()


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_payload_holds_nan_payloads_zeros_infinities_subnormals(dtype):
    bits = R.payload((40, 6), dtype, 1)
    f = bits.view(dtype)
    assert torch.equal(f.view(R.INT_VIEW[dtype]), bits)                 # the round trip through the float dtype keeps every bit
    v = f.float().view(-1)
    tiny = 2.0 ** -126
    assert bool(torch.isnan(v).sum() >= 6) and bool((v == float("inf")).any()) and bool((v == float("-inf")).any())
    assert bool(((v != 0) & (v.abs() < tiny)).sum() >= 4)               # subnormals of either sign
    mask = 0xFFFF if dtype == BF16 else 0xFFFFFFFF
    head = [int(b) & mask for b in bits.view(-1)[:9]]
    assert head == R.SPECIAL_BITS[dtype] and [int(b) & mask for b in bits.view(-1).flip(0)[:9]] == head
    zeros = [b for b in head if f.view(-1)[head.index(b)] == 0]
    assert len(zeros) == 2 and zeros[0] != zeros[1]                     # +0 and -0
    nans = {b for i, b in enumerate(head) if torch.isnan(v[i])}
    assert len(nans) == 3                                               # three different NaN patterns
    assert torch.unique(bits, dim=0).shape[0] == 40                     # no two rows alike
    assert R.payload((2, 2), dtype, 1).shape == (2, 2) and R.payload((3, 0, 4), dtype, 1).numel() == 0


def test_gather_and_scatter_references():
    B, N, K, D = 3, 11, 7, 6
    src = R.payload((B, N, D), BF16, 2)
    idx = R.any_idx(B, N, 17, 3)
    assert int(idx.min()) == 0 and int(idx.max()) == N - 1 and any(len(set(r.tolist())) < 17 for r in idx)
    assert not all(bool((r[1:] >= r[:-1]).all()) for r in idx)          # unsorted
    assert torch.equal(R.gather_ref(src, idx), torch.gather(src, 1, idx.unsqueeze(-1).expand(B, 17, D)))
    assert torch.equal(R.gather_ref(src[0], idx), src[0][idx]) and torch.equal(R.gather_ref(src[:1], idx), src[0][idx])
    u = R.unique_idx(B, N, K, 4)
    assert all(len(set(r.tolist())) == K for r in u)
    g = R.gather_ref(src, u)
    back = R.scatter_ref(g, u, N)
    assert torch.equal(back, torch.zeros_like(src).scatter_(1, u.unsqueeze(-1).expand(B, K, D), g))
    assert torch.equal(R.gather_ref(back, u), g) and int((back != 0).any(-1).sum()) <= B * K
    assert R.gather_ref(src, idx[:, :0]).shape == (B, 0, D) and not R.scatter_ref(g[:, :0], u[:, :0], N).any()


# ------------------------------------------------------------------------------------------------ position adds
def test_position_add_references_against_loops():
    B, K, D, N = 2, 3, 8, 5
    x, pos = R.rows_bf16((B * K, D), 5), R.table_f32((N, D), 6)
    idx = R.any_idx(B, N, K, 7)
    one = lambda a, b: (a.float() + b).to(BF16)       # noqa: E731
    ref = R.add_pos_ref(x, pos, B, K, idx)
    ref0 = R.add_pos_ref(x, pos, B, K)
    for b in range(B):
        for k in range(K):
            assert torch.equal(ref[b * K + k], one(x[b * K + k], pos[idx[b, k]])) and torch.equal(ref0[b * K + k], one(x[b * K + k], pos[k]))
    S, Gt = 3, 2
    posb = R.table_f32((Gt * S, D), 8)
    rb = R.add_pos_bcast_ref(x, posb, B, S, Gt)
    assert rb.shape == (B * Gt * S, D)
    for b in range(B):
        for t in range(Gt):
            for s in range(S):
                assert torch.equal(rb[(b * Gt + t) * S + s], one(x[b * S + s], posb[t * S + s]))
    F, Nf = 3, 2
    xf = R.rows_bf16((B, F * Nf, D), 9)
    fidx = R.any_idx(B, N, F, 10)
    rf = R.add_pos_frames_ref(xf, pos, fidx, Nf)
    for b in range(B):
        for r in range(F * Nf):
            assert torch.equal(rf[b, r], one(xf[b, r], pos[fidx[b, r // Nf]]))
    Ke, Kp = 2, 3
    e, tok = R.rows_bf16((B * Ke, D), 11), R.table_f32((D,), 12)
    ie, ip = R.any_idx(B, N, Ke, 13), R.any_idx(B, N, Kp, 14)
    rp = R.pred_assemble_ref(e, tok, pos, ie, ip)
    assert rp.shape == (B, Ke + Kp, D) and len(set(tok.tolist())) == D
    for b in range(B):
        for j in range(Ke + Kp):
            want = one(e[b * Ke + j], pos[ie[b, j]]) if j < Ke else (tok + pos[ip[b, j - Ke]]).to(BF16)
            assert torch.equal(rp[b, j], want)
    assert R.pred_assemble_ref(e[:0], tok, pos, ie[:, :0], ip).shape == (B, Kp, D)
    assert torch.equal(R.pred_assemble_ref(e, tok, pos, ie, ip[:, :0]), rp[:, :Ke])
    # the data round: the fp32 sum is not representable in bf16 almost everywhere
    s = x.float() + pos[idx.reshape(-1)]
    assert float((s.to(BF16).float() != s).float().mean()) > 0.9


# ------------------------------------------------------------------------------------------------ packers
@pytest.mark.parametrize("p,tub,C", R.PACK_COMBOS)
def test_unfold_is_conv3d_im2col(p, tub, C):
    """integer pixels and weights: Conv3d over the clip equals the unfolded rows times the flattened weight, exactly"""
    B, T, H, W = (R.PACK_SMALL[k] for k in "BTHW")
    g = torch.Generator().manual_seed(p + tub + C)
    clips = torch.randint(-3, 4, (B, C, T, H, W), generator=g).float()
    w = torch.randint(-2, 3, (5, C, tub, p, p), generator=g).float()
    conv = torch.nn.functional.conv3d(clips, w, stride=(tub, p, p)).flatten(2).transpose(1, 2)
    rows = R.unfold_rows(clips, tub, p)
    assert rows.shape == (B, (T // tub) * (H // p) * (W // p), C * tub * p * p)
    assert torch.equal(rows @ w.view(5, -1).t(), conv)
    assert torch.equal(R.tubelet_ref(clips, tub, p), rows.to(BF16))
    idx = R.any_idx(B, rows.shape[1], 5, 1)
    assert torch.equal(R.tubelet_ref(clips, tub, p, idx)[1, 2], rows[1, idx[1, 2]].to(BF16))
    # a still image: the rows of the clip that repeats it, indices taken modulo the cells
    img = clips[:, :, 0]
    cells = (H // p) * (W // p)
    rep = R.tubelet_ref(img.unsqueeze(2).repeat(1, 1, 3 * tub, 1, 1), tub, p)           # three tubelets deep
    assert torch.equal(R.image_ref(img, tub, p), rep[:, :cells])
    iidx = R.any_idx(B, 3 * cells, 7, 2)
    assert int(iidx.max()) >= cells and torch.equal(R.image_ref(img, tub, p, iidx), R.gather_ref(rep, iidx))


def test_big_shapes_cross_the_caps():
    b = R.PACK_BIG
    K = (b["T"] // b["tub"]) * (b["H"] // b["p"]) * (b["W"] // b["p"])
    assert R.pack_chunks(b["B"], K, b["C"], b["tub"], b["p"]) == 2102784 > R.FLAT_CAP == 2097152
    assert R.pack_chunks(b["B"] * b["T"], (b["H"] // b["p"]) * (b["W"] // b["p"]), b["C"], 1, b["p"]) == 2102784
    assert b["B"] * b["C"] * b["T"] * b["H"] * b["W"] * 4 < 68e6
    assert R.BIG_B * R.BIG_K == 16389 > R.ROW_CAP == 16384
    assert [w // 8 for w in R.WIDTHS] == [1, 64, 65, 129]
    assert [(b // 16, b % 16) for b in R.MOVE_BYTES] == [(0, 8), (0, 12), (16, 8), (1, 0), (64, 0), (65, 0)] and 264 // 4 == 66


# ------------------------------------------------------------------------------------------------ sums
def fp32_sums(x, rows=None):
    """plain fp32 column sums in three orders: torch's, row after row, and eight interleaved lanes added in turn"""
    xf = x.float() if rows is None else x.float()[rows]
    N = xf.shape[1]
    seq = torch.zeros(N)
    for r in range(min(xf.shape[0], 600)):           # (row after row is slow in Python: the first 600 rows, the rest by torch)
        seq = seq + xf[r]
    seq = seq + xf[600:].sum(0)
    lanes = torch.zeros(N)
    for lane in range(8):
        lanes = lanes + xf[lane::8].sum(0)
    return [xf.sum(0), seq, lanes]


def finish(s, alpha, old):
    t = s * torch.tensor(alpha, dtype=F32)
    return t if old is None else t + old


def _sum_cases():
    """(label, shape of the operand, rows summed, dtype, bool row mask or None) of every summing case of the GPU test"""
    out = [(R.colsum_id(c), (c.M, c.N), BF16, R.colsum_rows(c)) for c in R.COLSUM_CASES]
    out += [(f"tcolsum-M{M}", (M, R.TCOLSUM_N), BF16, None) for M in R.TCOLSUM_M]
    out += [(f"reduce-P{P}-N{N}", (P, N), F32, None) for P in R.REDUCE_P for N in R.REDUCE_N]
    out += [(f"segment{i}-P{P}-N{N}", (P, N), F32, None) for i, (P, N, _) in enumerate(R.SEGMENTS)]
    return out


SUM_CASES = _sum_cases()


@pytest.mark.parametrize("label,shape,dtype,rows", SUM_CASES, ids=[c[0] for c in SUM_CASES])
def test_integer_sums_are_exact_in_every_order_and_defects_show(label, shape, dtype, rows):
    M, N = shape
    x = R.int_data(shape, 21, dtype)
    assert not x.numel() or (float(x.abs().max()) <= 128 and bool((x != 0).any()))
    n = M if rows is None else int(rows.sum())
    for alpha, acc in R.COLSUM_RUNS:
        old = R.int_old(N, 22) if acc else None
        ref, _, a = R.sum_ref(x, alpha, old, rows)
        assert float(a.max() if a.numel() else 0) < 2.0 ** 24 and R.exact_in_fp32(a, alpha, old)      # the precondition
        for s in fp32_sums(x, rows):
            assert torch.equal(finish(s, alpha, old).double(), ref), label
        if n == 0 or N == 0:
            continue
        keep = torch.ones(M, dtype=torch.bool) if rows is None else rows.clone()
        live = keep.nonzero().view(-1)
        r = int(live[len(live) // 2])
        nz = x[r] != 0                                                   # (a zero entry tells nothing in its column)
        assert bool(nz.any())
        dropped = keep.clone()
        dropped[r] = False
        assert bool((finish(x.float()[dropped].sum(0), alpha, old).double() != ref)[nz].all())         # a dropped row
        assert bool((finish(x.float()[keep].sum(0) + x[r].float(), alpha, old).double() != ref)[nz].all())   # a doubled row
    if rows is not None and n:                                           # the window moved by one row at either end
        c = next(c for c in R.COLSUM_CASES if R.colsum_id(c) == label)
        ref = R.sum_ref(x, 1.0, None, rows)[0]
        for lo, hi in ((c.lo, c.hi + 1), (c.lo + 1, c.hi), (c.lo - 1, c.hi)):
            if 0 <= lo and hi <= c.group:
                assert not torch.equal(x.float()[R.window_rows(M, c.group, lo, hi)].sum(0).double(), ref), (label, lo, hi)


@pytest.mark.parametrize("label,shape,dtype,rows", SUM_CASES, ids=[c[0] for c in SUM_CASES])
def test_normal_sums_stay_inside_the_bound_and_a_dropped_row_leaves_it(label, shape, dtype, rows):
    M, N = shape
    x = R.normal_data(shape, 23, dtype)
    n = M if rows is None else int(rows.sum())
    for alpha, acc in R.COLSUM_RUNS:
        old = R.normal_old(N, 24) if acc else None
        ref, tol, a = R.sum_ref(x, alpha, old, rows)
        for s in fp32_sums(x, rows):
            err = (finish(s, alpha, old).double() - ref).abs()
            assert bool((err <= tol).all()), (label, float((err / tol).max()))
        if 2 <= n <= 1170 and N:
            keep = torch.ones(M, dtype=torch.bool) if rows is None else rows.clone()
            keep[int(keep.nonzero().view(-1)[n // 2])] = False
            err = (finish(x.float()[keep].sum(0), alpha, old).double() - ref).abs()
            assert bool((err > tol).any()), (label, float((err / tol).max()))


def test_bound_and_window_spelled_out():
    assert R.gamma(0) == 2 * R.U / (1 - 2 * R.U) and abs(R.gamma(16448) / (16450 * 2.0 ** -24) - 1) < 1e-3
    assert R.window_rows(7, 3, 1, 3).tolist() == [False, True, True, False, True, True, False]
    assert not R.window_rows(9, 3, 2, 2).any() and bool(R.window_rows(9, 9, 0, 9).all())
    x = torch.tensor([[1.0, -2.0], [3.0, 4.0], [5.0, -6.0]])
    ref, tol, a = R.sum_ref(x, 0.5, torch.tensor([10.0, -20.0]), torch.tensor([True, False, True]))
    assert ref.tolist() == [13.0, -24.0] and a.tolist() == [6.0, 8.0]
    assert torch.allclose(tol, R.gamma(2) * torch.tensor([13.0, 24.0], dtype=torch.float64))
    assert not R.exact_in_fp32(torch.tensor([2.0 ** 24]), 1.0) and not R.exact_in_fp32(torch.tensor([8.0]), 0.25)
    assert R.exact_in_fp32(torch.tensor([128.0 * 16448]), 0.5, torch.tensor([1000.0]))
    # every case the issue names is in the lists
    plain = {(c.M, c.N) for c in R.COLSUM_CASES if not c.group and c.rows == c.M}
    assert plain == {(M, 8) for M in (1, 8, 9, 512, 513, 8192, 16384, 16448)} | {(513, 264), (513, 2056), (8192, 2056)}
    wins = [c for c in R.COLSUM_CASES if c.group]
    assert any(c.lo == 0 for c in wins) and any(c.hi == c.group for c in wins) and any(c.lo == c.hi for c in wins)
    assert any(c.M == 9 * 130 and c.group == 130 for c in wins) and any(c.rows > c.M for c in R.COLSUM_CASES)
    assert len(R.SEGMENTS) == 16 and all(stride >= N for _, N, stride in R.SEGMENTS)
    t = R.transpose_ref(torch.arange(12, dtype=torch.int16).view(4, 3) + 1, 3)
    assert t.shape == (3, 64) and t[:, :3].tolist() == [[1, 4, 7], [2, 5, 8], [3, 6, 9]] and not t[:, 3:].any()
