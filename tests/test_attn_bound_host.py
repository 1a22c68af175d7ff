"""CPU: the per-element attention bounds of tests/attn_ref_util.py admit a correct kernel and reject planted defects.

A plain torch emulation of the kernels' arithmetic (bf16(q c) or bf16(k c) in fp32, fp32 scores, base = row maximum + 5, bf16 P, fp32 sums,
one bf16 rounding of every output) has to satisfy every bound at every (shape, mode) of the issue's section 3; the same emulation with one
planted defect has to violate a bound at every (shape, mode) where the defect exists.  The exact cases (uniform, one-hot) are checked
against float64: the gap conditions hold and the expected bits follow from the reference alone."""
import numpy as np
import pytest
import torch

from tests import attn_ref_util as A
from tests.attn_ref_util import bf

B0, H0 = 2, 2
FWD_DEFECTS = ["drop", "double", "next", "chunk"]          # seen by the forward's bound (and planted in the backward as well)
BWD_DEFECTS = ["drop", "double", "next", "chunk", "lse", "delta"]


def defect_exists(defect, case):
    if defect == "next":
        return case.B >= 2
    if defect == "delta":
        return case.S >= 2
    if defect == "chunk":
        return A.has_pad_chunk(case.hd)
    return True


# ------------------------------------------------------------------------------------------------ the emulation
def _sc(case):
    return np.float32(A.host_sc(case.scale))


def emu_forward(case, defect=None, row=0):
    """(o [B*S, H*hd] bf16, lse2 [B, H, S] fp32).  Defects act on slice (b, h) = (0, 0): `drop` / `double` the last key of query `row`,
    `next` = key 0 of sample 1 in its place, `chunk` = head-dim chunk 0 contracted a second time (a pad chunk not ignored)."""
    S = case.S
    q, k, v = [t.float() for t in A.split_qkv(case.qkv, case.B, S, case.H, case.hd)]
    qs = q if case.pre else bf(q * _sc(case)).float()
    s = qs @ k.transpose(-1, -2)
    if defect == "chunk":
        s[0, 0] += qs[0, 0][:, :8] @ k[0, 0][:, :8].t()
    if defect == "next":
        s[0, 0, row, S - 1] = (qs[0, 0, row] * k[1, 0, 0]).sum()
    base = s.amax(-1, keepdim=True) + A.HEADROOM
    P = bf(torch.exp2(s - base)).float()
    if defect == "drop":
        P[0, 0, row, S - 1] = 0.0
    if defect == "double":
        P[0, 0, row, S - 1] *= 2.0
    l = P.sum(-1, keepdim=True)
    acc = P @ v
    if defect == "next":
        acc[0, 0, row] += P[0, 0, row, S - 1] * (v[1, 0, 0] - v[0, 0, S - 1])
    return A.merge_heads(bf(acc / l)), (base + torch.log2(l)).squeeze(-1)


def emu_backward(case, o_in, lse_in, defect=None, row=0):
    """(dqkv [B*S, 3*H*hd] bf16, colq, colkv fp32) as the dQ kernel (scale folded into q) and the dK/dV kernel (folded into k) compute them.
    Further defects: `lse` = lse2 of query `row` off by 2^-6, `delta` = the row term of query `row` taken from the next row."""
    B, S, H, hd = case.B, case.S, case.H, case.hd
    q, k, v = [t.float() for t in A.split_qkv(case.qkv, B, S, H, hd)]
    dO = A.split_heads(case.dout, B, S, H, hd).float()
    o = A.split_heads(o_in, B, S, H, hd).float()
    lse = lse_in.float().view(B, H, S, 1).clone()
    sc, sa, ksc = _sc(case), np.float32(case.sabs), np.float32(case.kscale)
    delta = (dO * o).sum(-1, keepdim=True)
    if defect == "lse":
        lse[0, 0, row] += 2.0 ** -6
    if defect == "delta":
        delta[0, 0, row] = delta[0, 0, (row + 1) % S]
    last = S - 1

    def probs(s):
        P = torch.exp2(s - lse)
        if defect == "drop":
            P[0, 0, row, last] = 0.0
        if defect == "double":
            P[0, 0, row, last] *= 2.0
        return P
    # dQ kernel
    qs = q if case.pre else bf(q * sc).float()
    s = qs @ k.transpose(-1, -2)
    X = dO @ v.transpose(-1, -2) - delta
    if defect == "chunk":
        s[0, 0] += qs[0, 0][:, :8] @ k[0, 0][:, :8].t()
    if defect == "next":
        s[0, 0, row, last] = (qs[0, 0, row] * k[1, 0, 0]).sum()
        X = X.clone()
        X[0, 0, row, last] = (dO[0, 0, row] * v[1, 0, 0]).sum() - delta[0, 0, row, 0]
    dS = bf(probs(s) * X).float()
    dq = dS @ k
    if defect == "next":
        dq[0, 0, row] += dS[0, 0, row, last] * (k[1, 0, 0] - k[0, 0, last])
    dq = dq * sa
    # dK/dV kernel
    ks = k if case.pre else bf(k * sc).float()
    s = q @ ks.transpose(-1, -2)
    if defect == "chunk":
        s[0, 0] += q[0, 0][:, :8] @ ks[0, 0][:, :8].t()
    X = dO @ v.transpose(-1, -2) - delta
    P = probs(s)
    dv = bf(P).float().transpose(-1, -2) @ dO
    dk = (bf(P * X).float().transpose(-1, -2) @ q) * ksc
    kb = 64 * A.dkdv_kt(hd)
    colq = A._block_sums(dq, 128)
    colkv = torch.cat([A._block_sums(dk, kb), A._block_sums(dv, kb)], 1)
    dqkv = torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4).reshape(B * S, 3 * H * hd)
    return bf(dqkv), colq, colkv


def reference_inputs(fref):
    """o / lse2 the backward is fed with: the float64 forward rounded once (independent of any forward under test)."""
    return A.merge_heads(bf(fref["o"].float())), fref["lse"].float()


# ------------------------------------------------------------------------------------------------ the bounds admit the emulation
@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("S,hd", A.SHAPES)
def test_emulation_within_bounds_and_defects_rejected(S, hd, mode):
    """On every input variant of the pair (A.VARIANTS[mode]: exactly the cases tests/test_attention_elementwise_gpu.py runs the kernels on)
    the emulation stays inside every bound; every planted defect that exists at the pair violates a bound on at least one of those
    variants -- the forward's bound for the defects a forward can have AND the backward's for all six.  Prints, per defect, the variants
    that reject it (`plain` first: what the unsharpened inputs already show)."""
    seen = {}
    for variant in A.VARIANTS[mode]:
        case = A.variant_case(B0, S, H0, hd, mode, variant)
        if mode == "pow2":
            assert case.pow2_exact, "bf16(q * sc) != q * 0.125: the general bound applies"   # holds for every input drawn here
        fref = A.forward_reference(case)
        w = A.check_forward(case, *emu_forward(case), ref=fref)
        o_in, lse_in = reference_inputs(fref)
        bref = A.backward_reference(case, o_in, lse_in)
        w.update(A.check_backward(case, o_in, lse_in, *emu_backward(case, o_in, lse_in), ref=bref))
        print(f"emulation S{S} hd{hd} {mode} {variant[0]}: worst err/tol " + " ".join(f"{n} {x:.2f}" for n, x in w.items()))
        r_last, r_minq = A.sparse_rows(case)
        for defect in BWD_DEFECTS:
            if not defect_exists(defect, case):
                continue
            row = r_minq if defect == "lse" else r_last
            if defect == "delta":       # the row whose neighbour's delta differs most from its own
                dl = (case.dout64() * A.split_heads(o_in, B0, S, H0, hd).double()).sum(-1)[0, 0]
                row = int((dl - dl.roll(-1)).abs().argmax())
            hit = True
            if defect in FWD_DEFECTS:
                rep = {}
                A.check_forward(case, *emu_forward(case, defect, row), collect=rep, ref=fref)
                hit = not all(r["ok"] for r in rep.values())
            rep = {}
            A.check_backward(case, o_in, lse_in, *emu_backward(case, o_in, lse_in, defect, row), collect=rep, ref=bref)
            hit = hit and not all(r["ok"] for r in rep.values())
            seen.setdefault(defect, [])
            if hit:
                seen[defect].append(variant[0])
    print(f"defects S{S} hd{hd} {mode}: " + " ".join(f"{d}[{','.join(v) or 'MISSED'}]" for d, v in seen.items()))
    missed = [d for d, v in seen.items() if not v]
    assert not missed, f"S{S} hd{hd} {mode}: planted defects inside the bound on every input variant: {missed}"


# ------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("hd", A.HD_MAIN)
@pytest.mark.parametrize("S", A.SEQ_LENS)
def test_uniform_case_rejects_a_dropped_or_doubled_tail_key(S, hd):
    """q = 0: the bound with eps = 0 (u |ref| and the e terms) admits the emulation, pins lse2 = log2(S) to 2 e (|lse| + 8), and a single
    dropped or doubled last key of one row violates it at every S."""
    case = A.uniform_case(B0, S, H0, hd, "fold")
    fref = A.forward_reference(case, exact_scores=True)
    assert float((fref["lse"] - np.log2(S)).abs().max()) < 1e-12
    assert float(fref["tol_lse"].max()) <= 2 * A.E_F32 * (np.log2(S) + 8) * 1.0001 + np.log2(1 + (S + 2) * A.E_F32)
    A.check_forward(case, *emu_forward(case), exact_scores=True, ref=fref)
    for defect in ("drop", "double"):
        rep = {}
        A.check_forward(case, *emu_forward(case, defect, row=S // 2), collect=rep, ref=fref)
        assert not all(r["ok"] for r in rep.values()), (S, hd, defect)
        if S > 1:
            assert not rep["o"]["ok"], (S, hd, defect, "o alone must show it")


@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("S,hd", A.ONEHOT_SHAPES)
def test_onehot_case_conditions_and_expected_bits(S, hd, mode):
    """the gap conditions hold in float64, and under them the emulation gives o[i] = v[pi(i)] and dV[pi(i)] = dO[i] bit for bit; dQ and dK
    stay inside their bounds."""
    case, pi = A.onehot_case(B0, S, H0, hd, mode)
    gap, leak = A.onehot_conditions(case, pi)
    fref = A.forward_reference(case)
    assert torch.equal(fref["p"].argmax(-1), pi)
    o_exp, dv_exp = A.onehot_expected(case, pi)
    # the reference alone: float64 o rounded once is the expected pattern
    A.assert_bit_equal(A.merge_heads(bf(fref["o"].float())), o_exp, "float64 o")
    o, lse = emu_forward(case)
    A.assert_bit_equal(o, o_exp, f"emulated o S{S} hd{hd} {mode}")
    dqkv, colq, colkv = emu_backward(case, o, lse)
    dv = A.merge_heads(A.split_qkv(dqkv, B0, S, H0, hd)[2])
    A.assert_bit_equal(dv, dv_exp, f"emulated dV S{S} hd{hd} {mode}")
    A.check_backward(case, o, lse, dqkv, colq, colkv)
    print(f"one-hot S{S} hd{hd} {mode}: gap {gap:.1f} log2 units, leak {leak:.2e}")
