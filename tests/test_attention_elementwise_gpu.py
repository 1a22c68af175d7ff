"""GPU: every element of the attention outputs (csrc/attention.hip: forward, dQ, dK/dV, column partials) against a float64 reference
and its derived bound (tests/attn_ref_util.py), at every tile edge: S around the 16-query tile, the 64-key tile, the 128-query
workgroup and the 64 * KT key block, all 16 accepted head sizes, scale folded / pre-scaled / power of two.  The backward is fed
o / lse2 derived from the float64 forward, so it is checked independently of the forward kernel.  Exact cases (uniform, one-hot) pin
bits; the last two tests embed every operand in poisoned memory and poison the neighbouring (sample, head) slices."""
import ctypes

import pytest
import torch

from tests import attn_ref_util as A
from tests.attn_ref_util import bf

pytestmark = pytest.mark.gpu
DEV = "cuda"
B0, H0 = 2, 2


@pytest.fixture(scope="module")
def ops():
    from jepa_amd.hip import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from jepa_amd.hip.lib import load_library
    return load_library()


def _colsum_rows(lib, B, S, hd):
    from jepa_amd.hip.lib import check
    rq, rkv = ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib.vj_attn_bwd_colsum_rows(B, S, hd, ctypes.byref(rq), ctypes.byref(rkv)), "vj_attn_bwd_colsum_rows")
    return rq.value, rkv.value


def _fwd_bwd_against_bounds(ops, lib, case):
    """forward, then the backward on o / lse2 of the float64 forward (rounded once): every element inside its bound.  Returns the worst
    err/tol per output (information)."""
    B, S, H, hd = case.B, case.S, case.H, case.hd
    case = case.to(DEV)
    fref = A.forward_reference(case)
    o, lse = ops.attn_fwd(case.qkv, B, S, H, hd, case.scale)
    w = A.check_forward(case, o, lse, ref=fref)
    o_in, lse_in = A.merge_heads(bf(fref["o"].float())).contiguous(), fref["lse"].float().contiguous()
    dqkv, colq, colkv = ops.attn_bwd_colsum(case.qkv, o_in, case.dout, lse_in, B, S, H, hd, case.scale)
    assert (colq.shape[0], colkv.shape[0]) == (B * -(-S // 128), B * -(-S // (64 * A.dkdv_kt(hd)))) == _colsum_rows(lib, B, S, hd)
    w.update(A.check_backward(case, o_in, lse_in, dqkv, colq, colkv))
    print(f"B{B} S{S} H{H} hd{hd} {case.mode} {case.variant}: worst err/tol " + " ".join(f"{n} {x:.2f}" for n, x in w.items()))
    return w


@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("S,hd", A.SHAPES)
def test_every_element_within_its_bound(ops, lib, S, hd, mode):
    """every input variant of the pair (A.VARIANTS[mode]): the plain case and the sharpened ones on which tests/test_attn_bound_host.py
    proves that each planted defect leaves its bound."""
    for variant in A.VARIANTS[mode]:
        case = A.variant_case(B0, S, H0, hd, mode, variant)
        if mode == "pow2":
            assert case.pow2_exact      # bf16(x * sc) == x * 0.125 for the fp32 sc the host computes: u_fold = 0, the tight bound
        _fwd_bwd_against_bounds(ops, lib, case)


# workgroup counts of all three kernels no multiple of 8 (the XCD remap), and fewer than 8 workgroups per launch
@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("B,H,S,hd", [(3, 5, 129, 64), (3, 5, 193, 24), (1, 2, 65, 80), (1, 1, 129, 128), (1, 3, 17, 32)])
def test_workgroup_counts_off_the_xcd_multiple(ops, lib, B, H, S, hd, mode):
    nq, nk = B * H * -(-S // 128), B * H * -(-S // (64 * A.dkdv_kt(hd)))
    assert (nq % 8 != 0 and nk % 8 != 0) or max(nq, nk) < 8
    _fwd_bwd_against_bounds(ops, lib, A.random_case(B, S, H, hd, mode, seed=5))


@pytest.mark.parametrize("hd", A.HD_MAIN)
@pytest.mark.parametrize("S", A.SEQ_LENS)
def test_uniform_scores_exact_row_sums(ops, S, hd):
    """q = 0: P is 2^-5 in every slot and the row sum is exact, so the forward has to meet the bound with eps = 0 (u |ref| and the e terms:
    one dropped or doubled tail key violates it, tests/test_attn_bound_host.py) and lse2 = log2(S) within 2 e (|lse| + 8)."""
    case = A.uniform_case(B0, S, H0, hd, "fold").to(DEV)
    o, lse = ops.attn_fwd(case.qkv, B0, S, H0, hd, case.scale)
    w = A.check_forward(case, o, lse, exact_scores=True)
    print(f"uniform S{S} hd{hd}: worst err/tol o {w['o']:.2f} lse2 {w['lse2']:.2f}")


@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("S,hd", A.ONEHOT_SHAPES)
def test_onehot_rows_select_their_key_bit_for_bit(ops, S, hd, mode):
    """k rows = +-g sign codes, q_i = k_pi(i), runner-up gap >= 32 log2 units: o[i] == v[pi(i)] and, with the forward's own lse2,
    dV[pi(i)] == dO[i], bit for bit; dQ, dK (references ~ 0) inside their bounds."""
    case, pi = A.onehot_case(B0, S, H0, hd, mode)
    A.onehot_conditions(case, pi)
    case = case.to(DEV)
    o_exp, dv_exp = A.onehot_expected(case, pi)
    o, lse = ops.attn_fwd(case.qkv, B0, S, H0, hd, case.scale)
    A.assert_bit_equal(o, o_exp, f"o S{S} hd{hd} {mode}")
    dqkv, colq, colkv = ops.attn_bwd_colsum(case.qkv, o, case.dout, lse, B0, S, H0, hd, case.scale)
    dv = A.merge_heads(A.split_qkv(dqkv, B0, S, H0, hd)[2])
    A.assert_bit_equal(dv, dv_exp, f"dV S{S} hd{hd} {mode}")
    w = A.check_backward(case, o, lse, dqkv, colq, colkv)
    print(f"one-hot S{S} hd{hd} {mode}: worst err/tol dq {w['dq']:.2f} dk {w['dk']:.2f}")


# ------------------------------------------------------------------------------------------------ memory safety, cross-talk
def _plain_bwd(ops, lib, qkv, o, dout, lse, B, S, H, hd, scale):
    """vj_attn_bwd_colsum on contiguous tensors with a workspace of its own: (dqkv, colq, colkv, delta [H*B*S])."""
    from jepa_amd.hip.lib import check
    rq, rkv = _colsum_rows(lib, B, S, hd)
    dqkv = torch.empty_like(qkv)
    colq = torch.empty(rq, H * hd, dtype=torch.float32, device=DEV)
    colkv = torch.empty(rkv, 2 * H * hd, dtype=torch.float32, device=DEV)
    ws = torch.empty(H * B * S, dtype=torch.float32, device=DEV)
    check(lib.vj_attn_bwd_colsum(ops._ptr(qkv), ops._ptr(o), ops._ptr(dout), ops._ptr(lse), ops._ptr(dqkv), B, S, H, hd, scale,
                                 ops._ptr(ws), ws.numel() * 4, ops._ptr(colq), ops._ptr(colkv), ops._stream()), "vj_attn_bwd_colsum")
    return dqkv, colq, colkv, ws


@pytest.mark.parametrize("S,hd", A.SAFETY_SHAPES)
def test_segments_inside_poisoned_memory(ops, lib, S, hd):
    """vj_attn_fwd_segs / vj_attn_bwd_segs on two segments with row0 > 0 and unowned rows between and after them, every operand inside a
    larger allocation: NaN around and between the inputs' segments, the 0xA5 pattern around and between the outputs'.  The segments hold
    the bits of the plain contiguous calls; every byte outside them (gap rows, bands, the delta workspace's gaps) keeps the pattern."""
    from jepa_amd.hip.lib import check
    H, scale = 2, A.f32(hd ** -0.5)
    segs = [(3, 2, S), (3 + 2 * S + 5, 2, 17)]
    M = segs[1][0] + 2 * 17 + 2
    g = torch.Generator().manual_seed(S + hd)
    data = bf(torch.randn(M, 3 * H * hd, generator=g)).to(DEV)
    ddata = bf(torch.randn(M, H * hd, generator=g)).to(DEV)
    nan = float("nan")
    qkv = torch.full_like(data, nan)
    dout = torch.full_like(ddata, nan)
    o_in = torch.full_like(ddata, nan)
    lse_in = torch.full((1, H * M), nan, dtype=torch.float32, device=DEV)
    o_exp = A.pattern_like(M, H * hd, torch.bfloat16, DEV)
    dqkv_exp = A.pattern_like(M, 3 * H * hd, torch.bfloat16, DEV)
    lse_exp = A.pattern_like(1, H * M, torch.float32, DEV)
    nws = lib.vj_attn_bwd_segs_ws_bytes(ops._seg_array(segs), len(segs), H, hd)
    assert nws == 4 * H * (M - 2)
    ws_exp = A.pattern_like(1, nws // 4, torch.float32, DEV)
    cq_exp, ckv_exp = [], []
    for row0, B, Ss in segs:
        sl, fl = slice(row0, row0 + B * Ss), slice(H * row0, H * (row0 + B * Ss))
        qkv[sl], dout[sl] = data[sl], ddata[sl]
        o1, lse1 = ops.attn_fwd(qkv[sl], B, Ss, H, hd, scale)
        d1, cq1, ckv1, ws1 = _plain_bwd(ops, lib, qkv[sl], o1, dout[sl], lse1, B, Ss, H, hd, scale)
        o_in[sl], o_exp[sl], dqkv_exp[sl] = o1, o1, d1
        lse_in[0, fl], lse_exp[0, fl], ws_exp[0, fl] = lse1.reshape(-1), lse1.reshape(-1), ws1
        cq_exp.append(cq1)
        ckv_exp.append(ckv1)
    cq_exp, ckv_exp = torch.cat(cq_exp), torch.cat(ckv_exp)
    e_qkv, e_dout = A.embed_rows(qkv, True, 8), A.embed_rows(dout, True, 8)
    e_o = A.embed_rows(A.pattern_like(M, H * hd, torch.bfloat16, DEV), False, 8)
    e_lse = A.embed_rows(A.pattern_like(1, H * M, torch.float32, DEV), False, 4)
    seg_arr = ops._seg_array(segs)
    check(lib.vj_attn_fwd_segs(ops._ptr(e_qkv.view), ops._ptr(e_o.view), ops._ptr(e_lse.view), seg_arr, len(segs), H, hd, scale,
                               ops._stream()), "vj_attn_fwd_segs")
    assert A.raw_equal(e_o.view, o_exp), "o: a segment differs from the plain call or a gap row was written"
    assert A.raw_equal(e_lse.view, lse_exp), "lse2: a segment differs from the plain call or a gap was written"
    assert e_o.surroundings_intact() and e_lse.surroundings_intact()
    e_oin, e_lin = A.embed_rows(o_in, True, 8), A.embed_rows(lse_in, True, 4)
    e_d = A.embed_rows(A.pattern_like(M, 3 * H * hd, torch.bfloat16, DEV), False, 8)
    e_ws = A.embed_rows(A.pattern_like(1, nws // 4, torch.float32, DEV), False, 4)
    e_cq = A.embed_rows(A.pattern_like(*cq_exp.shape, torch.float32, DEV), False, 4)
    e_ckv = A.embed_rows(A.pattern_like(*ckv_exp.shape, torch.float32, DEV), False, 4)
    check(lib.vj_attn_bwd_segs(ops._ptr(e_qkv.view), ops._ptr(e_oin.view), ops._ptr(e_dout.view), ops._ptr(e_lin.view), ops._ptr(e_d.view),
                               seg_arr, len(segs), H, hd, scale, ops._ptr(e_ws.view), nws, ops._ptr(e_cq.view), ops._ptr(e_ckv.view),
                               ops._stream()), "vj_attn_bwd_segs")
    assert A.raw_equal(e_d.view, dqkv_exp), "dqkv: a segment differs from the plain call or a gap row was written"
    assert A.raw_equal(e_ws.view, ws_exp), "delta workspace: differs from the plain call or a gap was written"
    assert A.raw_equal(e_cq.view, cq_exp) and A.raw_equal(e_ckv.view, ckv_exp), "column partials differ from the plain calls"
    for e in (e_d, e_ws, e_cq, e_ckv, e_o, e_lse):
        assert e.surroundings_intact()


@pytest.mark.parametrize("S,hd", A.SAFETY_SHAPES)
def test_poisoned_neighbour_slices_do_not_leak(ops, lib, S, hd):
    """one clean run, then one run per (sample, head) slice with every OTHER slice of qkv / dout (and of the o / lse2 the backward reads)
    NaN: the slice keeps its exact bits in o, lse2, dqkv and its column partials."""
    B, H, scale = B0, H0, A.f32(hd ** -0.5)
    case = A.random_case(B, S, H, hd, "fold", seed=3).to(DEV)
    o, lse = ops.attn_fwd(case.qkv, B, S, H, hd, scale)
    dqkv, colq, colkv = ops.attn_bwd_colsum(case.qkv, o, case.dout, lse, B, S, H, hd, scale)
    nq, nk = colq.shape[0] // B, colkv.shape[0] // B
    nan = float("nan")
    for b in range(B):
        for h in range(H):
            qkv_p, dout_p = torch.full_like(case.qkv, nan), torch.full_like(case.dout, nan)
            qkv_p.view(B, S, 3, H, hd)[b, :, :, h] = case.qkv.view(B, S, 3, H, hd)[b, :, :, h]
            dout_p.view(B, S, H, hd)[b, :, h] = case.dout.view(B, S, H, hd)[b, :, h]
            o_p, lse_p = ops.attn_fwd(qkv_p, B, S, H, hd, scale)
            d_p, cq_p, ckv_p = ops.attn_bwd_colsum(qkv_p, o_p, dout_p, lse_p, B, S, H, hd, scale)
            tag = f"S{S} hd{hd} slice ({b}, {h})"
            A.assert_bit_equal(o_p.view(B, S, H, hd)[b, :, h], o.view(B, S, H, hd)[b, :, h], "o " + tag)
            A.assert_bit_equal(lse_p[b, h][:, None], lse[b, h][:, None], "lse2 " + tag)
            A.assert_bit_equal(d_p.view(B, S, 3, H, hd)[b, :, :, h].reshape(S, -1), dqkv.view(B, S, 3, H, hd)[b, :, :, h].reshape(S, -1),
                               "dqkv " + tag)
            A.assert_bit_equal(cq_p.view(B, nq, H, hd)[b, :, h], colq.view(B, nq, H, hd)[b, :, h], "colq " + tag)
            A.assert_bit_equal(ckv_p.view(B, nk, 2, H, hd)[b, :, :, h].reshape(nk, -1), colkv.view(B, nk, 2, H, hd)[b, :, :, h].reshape(nk, -1),
                               "colkv " + tag)
