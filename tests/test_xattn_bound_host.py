"""CPU: the per-element cross-attention bounds of tests/xattn_ref_util.py admit correct arithmetic and reject planted defects.

A plain torch fp32 emulation of the two paths of csrc/xattn.hip -- the single workgroup, and the split forms with chunks of 2048 keys
merged in ascending order; fp32 q * (scale log2e), fp32 scores, fp32 probabilities, sums in the kernels' (row group, pass) order, one
bf16 rounding of every stored output -- has to satisfy every bound, and the exact pin of the aimed cases, on every input variant of
every shape tests/test_xattn_elementwise_gpu.py runs the kernels at.  The same emulation with ONE planted defect has to violate a
bound (or the pin) on at least one variant of every shape where the defect exists, in the forward where a forward can have it AND in
the backward where a backward can; the test prints which variant rejected it.

A defect acts on one (sample, head) slice, so only that slice is emulated again and checked, and a defect is tried on the next variant
only while no earlier one has rejected it.  B = H = 2 at every shape, as on the GPU."""
import numpy as np
import pytest
import torch

from tests import xattn_ref_util as X
from tests.xattn_ref_util import bf

# (defect, in the forward, in the backward); `split`: only where the split forms run
DEFECTS = [("drop_seq", True, True),        # the last key of the sequence dropped ...
           ("twice_seq", True, True),       # ... or counted twice
           ("drop_chunk", True, True),      # the last key of chunk 0 dropped (split) ...
           ("twice_chunk", True, True),     # ... or counted twice
           ("chunk_shift", True, True),     # chunk 1 reads its keys from j0 + 1 (split)
           ("tail_pass", True, True),       # the keys of the last, partial row-group pass skipped in the weighted-row sum and the dK/dV store
           ("head_q", True, True),          # head h uses head h + 1's query columns
           ("sample_q", True, True),        # sample 1 uses sample 0's q under a per-sample stride
           ("resid_row", True, False),      # the residual row of query 0 used for query 1
           ("lse_off", False, True),        # lse2_in of one (b, h) off by 2^-6
           ("delta_c0", False, True),       # delta taken from the first chunk's partial only (split)
           ("no_weight", True, False),      # the forward combine without the 2^(m_c - M) weight (split)
           ("dq_noscale", False, True)]     # dq without the final `scale`
SPLIT_ONLY = {"drop_chunk", "twice_chunk", "chunk_shift", "delta_c0", "no_weight"}


def defect_exists(defect, case, split):
    if defect in SPLIT_ONLY:
        return split
    if defect == "tail_pass":
        return X.chunks_of(case.N, split)[-1][1] % X.n_groups(case.hd) != 0
    if defect == "head_q":
        return case.H >= 2
    if defect == "sample_q":
        return case.B >= 2 and not case.shared
    if defect == "resid_row":
        return case.NQ >= 2
    if defect == "dq_noscale":
        return case.N >= 2      # one key: P = 1, delta = dP, so dS and with it dq are 0 whatever multiplies them
    return True


def defect_key(defect, case, split):
    """the key a defect acts on (None: no particular one): an aimed case shows it in the slice that is aimed at that key."""
    j0, n = X.chunks_of(case.N, split)[-1]
    return {"drop_seq": case.N - 1, "twice_seq": case.N - 1, "drop_chunk": X.XA_CHUNK - 1, "twice_chunk": X.XA_CHUNK - 1,
            "chunk_shift": X.XA_CHUNK, "tail_pass": j0 + (n - 1) // X.n_groups(case.hd) * X.n_groups(case.hd)}.get(defect)


def defect_slice(defect, case, split):
    """(b, h) the defect is planted in: (1, 0) for `sample_q`, else (0, 0) -- or, in an aimed case, a slice aimed at the defect's key."""
    if defect == "sample_q":
        return 1, 0
    key = defect_key(defect, case, split)
    if case.jstar is not None and key is not None:
        hit = (case.jstar == key).any(-1).nonzero()
        if hit.shape[0]:
            return int(hit[0, 0]), int(hit[0, 1])
    return 0, 0


# ------------------------------------------------------------------------------------------------ the emulation, one (b, h) slice
def _sc(case):
    return torch.tensor(np.float32(case.scale) * X.LOG2E_F32)      # the fp32 product the kernels form


def _block_sum(x):
    """sum over dim 0 as a workgroup forms it: thread t adds x[t], x[t + 256], ... in turn, then the 256 partials are combined."""
    n = x.shape[0]
    pad = -n % X.XA_THREADS
    if pad:
        x = torch.cat([x, x.new_zeros(pad, *x.shape[1:])])
    return x.view(-1, X.XA_THREADS, *x.shape[1:]).sum(0).sum(0)


def _weighted_rows(w, rows, ngrp, skip_tail):
    """sum_j w[j] rows[j] as xa_weighted_rows: row group g adds keys g, g + ngrp, ... in turn, then the ngrp partials are added.
    skip_tail: the last pass, where it is partial, is left out (the planted defect)."""
    n = rows.shape[0]
    x = w[:, None] * rows
    if skip_tail and n % ngrp:
        x[n // ngrp * ngrp:] = 0.0
    pad = -n % ngrp
    if pad:
        x = torch.cat([x, x.new_zeros(pad, x.shape[1])])
    return x.view(-1, ngrp, x.shape[1]).sum(0).sum(0)


def _slice_inputs(case, b, h, defect):
    """q [NQ, hd], k, v [N, hd], resid [NQ, hd] | None, dy [hd] of slice (b, h) in fp32, with the defects that read a wrong operand."""
    k, v = [t[b, h].float() for t in case.kv4()]
    q4 = case.q4()
    q = q4[0 if defect == "sample_q" else b, h + 1 if defect == "head_q" else h].float()
    resid = None if case.resid is None else case.resid4()[0, h].float()
    if defect == "resid_row" and resid is not None:
        resid = resid.clone()
        resid[1] = resid[0]
    return q, k, v, resid, case.dy3()[b, h].float()


def _touch(p, defect, ci, nchunks, split):
    """the defects that drop or double one key of chunk `ci`: p [n, ...] in place."""
    if ci == nchunks - 1 and defect in ("drop_seq", "twice_seq"):
        p[-1] *= 0.0 if defect == "drop_seq" else 2.0
    if split and ci == 0 and defect in ("drop_chunk", "twice_chunk"):
        p[-1] *= 0.0 if defect == "drop_chunk" else 2.0


def emu_forward_slice(case, b, h, split, defect=None):
    """(out [NQ, hd] bf16, lse2 [NQ] fp32) of slice (b, h)."""
    q, k, v, resid, _ = _slice_inputs(case, b, h, defect)
    qv = q * _sc(case)
    ngrp, chunks = X.n_groups(case.hd), X.chunks_of(case.N, split)
    ms, ls, ys = [], [], []
    for ci, (j0, n) in enumerate(chunks):
        r0 = j0 + 1 if (defect == "chunk_shift" and ci == 1) else j0
        kk, vv = k[r0:r0 + n], v[r0:r0 + n]
        s = kk @ qv.t()                                                          # [n, NQ]
        m = s.amax(0)
        p = torch.exp2(s - m)
        _touch(p, defect, ci, len(chunks), split)
        ms.append(m)
        ls.append(_block_sum(p))
        tail = defect == "tail_pass" and ci == len(chunks) - 1
        ys.append(torch.stack([_weighted_rows(p[:, iq], vv, ngrp, tail) for iq in range(case.NQ)]))   # [NQ, hd]
    if not split:
        M, L, y = ms[0], ls[0], ys[0]
    else:
        M = torch.stack(ms).amax(0)
        L, y = torch.zeros_like(M), torch.zeros_like(ys[0])
        for m, l, yc in zip(ms, ls, ys):                                          # ascending chunk order
            wgt = torch.ones_like(M) if defect == "no_weight" else torch.exp2(m - M)
            L = L + wgt * l
            y = y + wgt[:, None] * yc
    o = y / L[:, None]
    if resid is not None:
        o = o + resid
    return bf(o), M + torch.log2(L)


def emu_backward_slice(case, b, h, lse_in, split, defect=None):
    """(dq [hd], dk [N, hd], dv [N, hd] bf16) of slice (b, h) from lse_in [B, H] fp32.  Rows a defect leaves unwritten stay 0."""
    q, k, v, _, dy = _slice_inputs(case, b, h, defect)
    q = q[0]
    qv = q * _sc(case)
    scale = torch.tensor(np.float32(case.scale))
    l2 = lse_in[b, h].float().cpu() + (2.0 ** -6 if defect == "lse_off" else 0.0)
    ngrp, chunks = X.n_groups(case.hd), X.chunks_of(case.N, split)
    ps, es, dls = [], [], []
    for ci, (j0, n) in enumerate(chunks):
        r0 = j0 + 1 if (defect == "chunk_shift" and ci == 1) else j0
        p = torch.exp2(k[r0:r0 + n] @ qv - l2)
        _touch(p, defect, ci, len(chunks), split)
        e = v[r0:r0 + n] @ dy
        ps.append(p)
        es.append(e)
        dls.append(_block_sum(p * e))
    delta = torch.zeros(())
    for dl in dls[:1] if defect == "delta_c0" else dls:                           # ascending chunk order
        delta = delta + dl
    dq = torch.zeros(case.hd)
    dk, dv = torch.zeros(case.N, case.hd), torch.zeros(case.N, case.hd)
    for ci, (j0, n) in enumerate(chunks):
        r0 = j0 + 1 if (defect == "chunk_shift" and ci == 1) else j0
        ds = ps[ci] * (es[ci] - delta)
        tail = defect == "tail_pass" and ci == len(chunks) - 1
        dq = dq + _weighted_rows(ds, k[r0:r0 + n], ngrp, tail)
        keep = n // ngrp * ngrp if (tail and n % ngrp) else n
        dk[j0:j0 + keep] = (ds[:, None] * (q * scale))[:keep]
        dv[j0:j0 + keep] = (ps[ci][:, None] * dy)[:keep]
    return bf(dq if defect == "dq_noscale" else dq * scale), bf(dk), bf(dv)


def emu_forward(case, split):
    """(out [B*NQ, D] bf16, lse2 [B, H, NQ] fp32): every slice."""
    out = torch.empty(case.B, case.H, case.NQ, case.hd, dtype=torch.bfloat16)
    lse = torch.empty(case.B, case.H, case.NQ)
    for b in range(case.B):
        for h in range(case.H):
            out[b, h], lse[b, h] = emu_forward_slice(case, b, h, split)
    return out.permute(0, 2, 1, 3).reshape(case.B * case.NQ, case.D), lse


def emu_backward(case, lse_in, split):
    """(dq [B, D], dkv [B*N, 2*D] bf16): every slice."""
    dq = torch.empty(case.B, case.H, case.hd, dtype=torch.bfloat16)
    dkv = torch.empty(case.B, case.N, 2, case.H, case.hd, dtype=torch.bfloat16)
    for b in range(case.B):
        for h in range(case.H):
            dq[b, h], dkv[b, :, 0, h], dkv[b, :, 1, h] = emu_backward_slice(case, b, h, lse_in, split)
    return dq.reshape(case.B, case.D), dkv.reshape(case.B * case.N, 2 * case.D)


# ------------------------------------------------------------------------------------------------ one (shape, q sharing, NQ) job
def _rejected(rep):
    return not all(r["ok"] for r in rep.values())


def run_job(N, hd, H, shared, NQ, fwd, bwd):
    """Every variant inside every bound (and the aimed pin exact); every existing defect rejected.  Returns the printed summary."""
    fsplit, bsplit = N > X.FWD_MAX, N > X.BWD_MAX
    seen = {}
    for variant in X.VARIANTS:
        case = X.make_case(X.B0, NQ, N, H, hd, shared, variant, split=fsplit if fwd else bsplit)
        worst = {}
        if fwd:
            fref = X.forward_reference(case, fsplit)
            out, lse = emu_forward(case, fsplit)
            worst.update(X.check_forward(case, out, lse, fref))
            if variant == "aimed":
                X.assert_bit_equal(out, X.aimed_expected(case), f"emulated out {case.label}")
        if bwd:
            lse_in = X.lse_input(case)
            bref = X.backward_reference(case, lse_in, bsplit)
            worst.update(X.check_backward(case, *emu_backward(case, lse_in, bsplit), bref))
        print(f"emulation {case.label}: worst err/tol " + " ".join(f"{n} {x:.2f}" for n, x in worst.items())
              + (f"; gap {case.gap:.0f} log2 units" if variant == "aimed" else ""))
        for defect, in_fwd, in_bwd in DEFECTS:
            if fwd and in_fwd and defect_exists(defect, case, fsplit) and not (defect == "resid_row" and case.resid is None):
                hits = seen.setdefault((defect, "fwd"), [])
                if not hits:
                    b, h = defect_slice(defect, case, fsplit)
                    o, l = emu_forward_slice(case, b, h, fsplit, defect)
                    full_o, full_l = X.out4(case, out).clone(), lse.clone()
                    full_o[b, h], full_l[b, h] = o, l
                    full_o = full_o.permute(0, 2, 1, 3).reshape(case.B * NQ, case.D)
                    rep = {}
                    X.check_forward(case, full_o, full_l, fref, sl=(b, h), collect=rep)
                    pin = variant == "aimed" and not torch.equal(full_o, X.aimed_expected(case))
                    if _rejected(rep) or pin:
                        hits.append(variant + ("" if _rejected(rep) else "(pin)"))
            if bwd and in_bwd and defect_exists(defect, case, bsplit):
                hits = seen.setdefault((defect, "bwd"), [])
                if not hits:
                    b, h = defect_slice(defect, case, bsplit)
                    dq, dk, dv = emu_backward_slice(case, b, h, lse_in, bsplit, defect)
                    rep = {}
                    for name, o_, key in (("dq", dq, "dq"), ("dk", dk, "dk"), ("dv", dv, "dv")):
                        r_, t_ = bref[key][b, h], bref["tol_" + key][b, h]
                        rep[name] = X.elementwise_report(o_.reshape(-1, hd), r_.reshape(-1, hd), t_.reshape(-1, hd))
                    if _rejected(rep):
                        hits.append(variant)
    line = f"defects N{N} hd{hd} H{H} NQ{NQ} {'shared' if shared else 'per-sample'}: " + " ".join(
        f"{d}/{way}[{','.join(v) or 'MISSED'}]" for (d, way), v in seen.items())
    print(line)
    missed = [k for k, v in seen.items() if not v]
    assert not missed, f"planted defects inside the bound on every input variant: {missed}\n{line}"
    return seen


@pytest.mark.parametrize("N,hd", X.SINGLE_SHAPES)
def test_single_workgroup_emulation_within_bounds_and_defects_rejected(N, hd):
    """NQ = 3 forward, NQ = 1 forward + backward, q shared and per sample, B = H = 2."""
    for shared in X.shared_settings(N, hd):
        run_job(N, hd, X.H0, shared, 3, True, False)
        run_job(N, hd, X.H0, shared, 1, True, True)


@pytest.mark.parametrize("N,hd", X.LARGE_BWD_SHAPES)
def test_large_backward_emulation_within_bounds_and_defects_rejected(N, hd):
    """the backward at its LDS limit and on the split path."""
    for shared in X.shared_settings(N, hd):
        seen = run_job(N, hd, X.H0, shared, 1, False, True)
        assert (("delta_c0", "bwd") in seen) == (N > X.BWD_MAX)


@pytest.mark.parametrize("N,hd", X.LARGE_FWD_SHAPES)
def test_large_forward_emulation_within_bounds_and_defects_rejected(N, hd):
    """the forward at its LDS limit and on the split path."""
    for shared in X.shared_settings(N, hd):
        seen = run_job(N, hd, X.H0, shared, 3, True, False)
        assert (("no_weight", "fwd") in seen) == (N > X.FWD_MAX)


def test_chain_length_and_aimed_keys():
    """the numbers the bounds and the aimed cases rest on, spelled out for a few shapes."""
    assert X.chain_len(257, 128, False) == 17 + 16               # 16 row groups, 17 passes
    assert X.chain_len(257, 8, False) == 2 + 256                 # 256 row groups
    assert X.chain_len(38264, 128, False) == 2392 + 16
    assert X.chain_len(40961, 128, True) == 128 + 16 + 21        # 2048-key chunks, 21 of them
    assert X.chain_len(19133, 8, True) == 8 + 256 + 10
    assert X.aimed_keys(19133, 24, True) == [19132, 2047, 2048, 18432 + 8 * 85]     # the last chunk holds 701 keys: passes of 85
    assert X.aimed_keys(20481, 128, True) == [20480, 2047, 2048, 0]                 # a chunk of one key: it is its own last pass
    assert X.aimed_keys(86, 24, False) == [85, 0, 1, 2]
    assert X.aimed_keys(1, 8, False) == [0]
    for N, hd, split in ((257, 80, False), (19133, 24, True), (40961, 8, True)):
        case = X.make_case(X.B0, 3 if N != 19133 else 1, N, X.H0, hd, False, "aimed", split=split)
        assert case.gap >= 40 + np.log2(N)
        assert len({int(j) for j in case.jstar[:, :, 0].reshape(-1)}) == 4     # the four slices aim at four different keys
