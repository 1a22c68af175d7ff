"""GPU: the data-movement kernels at their edges, element for element against plain torch on the CPU (tests/rows_ref_util.py).

csrc/rows.hip (gather / scatter / copy of rows, the four position adds, the slice sum), csrc/reduce.hip (transposes, column sums, partial
and segment reductions) and tubelet_pack / image_pack of csrc/input_pack.hip: the second pass of every grid-stride loop (more than
16 384 rows, more than 2 097 152 chunks), the 4-byte form of the row movers and its second lane trip, every width at which a lane loop
changes its trip count, the row loop and every chunk count of the column sum, row windows across chunk boundaries, empty operands.
Operands sit inside one allocation each: inputs that feed arithmetic between NaN guards, outputs between sentinels that must survive, and
whatever a kernel has to zero or overwrite is prefilled with NaN.  Movers are compared bit for bit on arbitrary bit patterns; position
adds bit for bit with one fp32 add and one rounding; sums exactly on integer data and inside a derived bound on normal draws."""
import ctypes

import pytest
import torch

from tests import rows_ref_util as R
from tests.rows_ref_util import BF16, F32, Embedded

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
DTYPES = [BF16, F32]
DT_ID = {BF16: "bf16", F32: "fp32"}


@pytest.fixture(scope="module")
def ops():
    from jepa_amd.hip import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from jepa_amd.hip.lib import load_library
    return load_library()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _emb(t, fill=NAN, shift=0, dtype=None):
    """the CPU tensor t (or the integer view of a `dtype` tensor) on the device, inside a guarded allocation"""
    return Embedded(tuple(t.shape), dtype or t.dtype, DEV, fill, shift=shift).put(t.to(DEV))


def _out(shape, dtype, shift=0, inner=NAN):
    """an output: NaN where the result goes, a sentinel around it"""
    return Embedded(tuple(shape), dtype, DEV, -7.0, shift=shift, inner=inner)


def _same_bits(e, ref):
    """the guarded tensor holds ref's bits (ref: a CPU tensor of the same dtype or of its integer view) and its surroundings are untouched"""
    torch.cuda.synchronize()
    iv = R.INT_VIEW.get(ref.dtype)
    return torch.equal(e.bits().cpu(), ref if iv is None else ref.view(iv)) and e.guards_untouched()


# ------------------------------------------------------------------------------------------------ gather / scatter
def _gather(ops, dtype, B, N, K, D, seed, table=False, src_shift=0, out_shift=0, use_out=True):
    bits = R.payload((N, D) if table else (B, N, D), dtype, seed)
    idx = R.any_idx(B, N, K, seed + 1)
    src = _emb(bits, shift=src_shift, dtype=dtype)
    ref = R.gather_ref(bits, idx)
    if use_out:
        out = _out((B, K, D), dtype, shift=out_shift)
        got = ops.gather_rows(src.view, idx.to(DEV), out=out.view)
        assert got.data_ptr() == out.view.data_ptr()
        assert _same_bits(out, ref)
    else:
        got = ops.gather_rows(src.view, idx.to(DEV))
        assert got.shape == (B, K, D) and got.dtype == dtype
        assert torch.equal(got.view(R.INT_VIEW[dtype]).cpu(), ref)
    assert _same_bits(src, bits)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("row_bytes", R.MOVE_BYTES)
def test_gather_rows_moves_bits_at_every_width(ops, dtype, row_bytes):
    """repeated, unsorted indices (17 rows out of 11); the plain, the out= and the broadcast-table form"""
    D = row_bytes // (2 if dtype == BF16 else 4)
    _gather(ops, dtype, 3, 11, 17, D, 100 + row_bytes, use_out=False)
    _gather(ops, dtype, 3, 11, 17, D, 200 + row_bytes)
    _gather(ops, dtype, 3, 11, 17, D, 300 + row_bytes, table=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("src_shift,out_shift", [(1, 0), (0, 1), (1, 1)])
def test_gather_rows_on_a_4_byte_aligned_base(ops, dtype, src_shift, out_shift):
    """a 16-divisible row (1040 bytes) on a base 4 bytes past a 16-byte boundary: the 4-byte form, five lane trips"""
    per = 2 if dtype == BF16 else 1       # elements per 4 bytes
    _gather(ops, dtype, 2, 9, 7, 1040 // (2 if dtype == BF16 else 4), 400, src_shift=src_shift * per, out_shift=out_shift * per)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_gather_rows_past_the_launch_cap_and_empty(ops, dtype):
    D = 16 // (2 if dtype == BF16 else 4)
    assert R.BIG_B * R.BIG_K > R.ROW_CAP
    _gather(ops, dtype, R.BIG_B, 64, R.BIG_K, D, 500)
    _gather(ops, dtype, 1, 64, R.BIG_B * R.BIG_K, D, 501, table=True)
    _gather(ops, dtype, 2, 8, 0, D, 502)                     # K = 0: nothing is written


def _scatter(lib, dtype, B, N, K, D, seed, src_shift=0, dst_shift=0):
    from jepa_amd.hip.lib import check
    bits = R.payload((B, K, D), dtype, seed)
    idx = R.unique_idx(B, N, K, seed + 1)
    src = _emb(bits, shift=src_shift, dtype=dtype)
    dst = _out((B, N, D), dtype, shift=dst_shift)            # NaN inside: every row not indexed has to come back as zero
    didx = idx.to(DEV)
    check(lib.vj_scatter_rows(_p(src.view), _p(dst.view), _p(didx), B, N, K, D * bits.element_size(), _stream()), "vj_scatter_rows")
    assert _same_bits(dst, R.scatter_ref(bits, idx, N))
    assert _same_bits(src, bits)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("row_bytes", R.MOVE_BYTES)
def test_scatter_rows_moves_bits_and_zeroes_the_rest(lib, dtype, row_bytes):
    D = row_bytes // (2 if dtype == BF16 else 4)
    _scatter(lib, dtype, 3, 11, 7, D, 600 + row_bytes)
    _scatter(lib, dtype, 2, 5, 5, D, 700 + row_bytes)        # every row indexed


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_scatter_rows_misaligned_past_the_cap_and_empty(lib, dtype):
    es = 2 if dtype == BF16 else 4
    per = 4 // es
    for src_shift, dst_shift in ((per, 0), (0, per), (per, per)):
        _scatter(lib, dtype, 2, 9, 7, 1040 // es, 800, src_shift=src_shift, dst_shift=dst_shift)
    _scatter(lib, dtype, R.BIG_B, R.BIG_K + 7, R.BIG_K, 16 // es, 801)
    _scatter(lib, dtype, 2, 8, 0, 16 // es, 802)             # K = 0: all zero


def test_ops_scatter_rows_is_the_adjoint_of_gather(ops):
    """the wrapper (it allocates its own output): gather of its result gives the rows back, everything else is zero"""
    bits = R.payload((3, 7, 6), BF16, 810)
    idx = R.unique_idx(3, 11, 7, 811)
    got = ops.scatter_rows(bits.view(BF16).to(DEV), idx.to(DEV), 11)
    assert torch.equal(got.view(torch.int16).cpu(), R.scatter_ref(bits, idx, 11))


# ------------------------------------------------------------------------------------------------ copy_rows
def _copy(ops, B, src_rows, src_off, dst_rows, dst_off, n, D, seed):
    bits = R.payload((B, src_rows, D), BF16, seed)
    fill = R.payload((B, dst_rows, D), BF16, seed + 1)
    fill[fill == 0] = 0x0101                                  # no zero anywhere in the destination
    src = _emb(bits, dtype=BF16)
    for zero in (False, True):
        dst = _emb(fill, fill=-7.0, dtype=BF16)
        ops.copy_rows(None if zero else src.view, dst.view, B, src_rows, src_off, dst_rows, dst_off, n, D)
        ref = fill.clone()
        ref[:, dst_off:dst_off + n] = 0 if zero else bits[:, src_off:src_off + n]
        assert _same_bits(dst, ref)
    assert _same_bits(src, bits)


@pytest.mark.parametrize("D", [8, 512, 1024])
def test_copy_rows_widths_windows_and_zero_fill(ops, D):
    _copy(ops, 3, 7, 2, 9, 4, 3, D, 900 + D)
    _copy(ops, 2, 7, 1, 4, 0, 4, D, 910 + D)                 # the window touches both ends of the destination
    _copy(ops, 2, 7, 3, 9, 5, 0, D, 920 + D)                 # n = 0: nothing moves


def test_copy_rows_past_the_launch_cap(ops):
    _copy(ops, R.BIG_B, R.BIG_K + 2, 1, R.BIG_K + 3, 2, R.BIG_K, 8, 930)


# ------------------------------------------------------------------------------------------------ position adds
def _shape_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


ADD_SHAPES = [(2, 5, D) for D in R.WIDTHS] + [(R.BIG_B, R.BIG_K, 8)]


@pytest.mark.parametrize("with_idx", [False, True], ids=["arange", "idx"])
@pytest.mark.parametrize("B,K,D", ADD_SHAPES, ids=lambda v: str(v))
def test_add_pos(ops, B, K, D, with_idx):
    N = K + 6
    x0, pos = R.rows_bf16((B * K, D), 1000 + D), R.table_f32((N, D), 1001 + D)
    idx = R.any_idx(B, N, K, 1002) if with_idx else None
    x, tab = _emb(x0), _emb(pos)
    ops.add_pos(x.view, tab.view, B, K, None if idx is None else idx.to(DEV))
    assert _same_bits(x, R.add_pos_ref(x0, pos, B, K, idx))
    assert _same_bits(tab, pos)


@pytest.mark.parametrize("Gt", [1, 3])
@pytest.mark.parametrize("B,S,D", ADD_SHAPES, ids=lambda v: str(v))
def test_add_pos_bcast(ops, B, S, D, Gt):
    y0, pos = R.rows_bf16((B * S, D), 1100 + D), R.table_f32((Gt * S, D), 1101 + D)
    y, tab, out = _emb(y0), _emb(pos), _out((B * Gt * S, D), BF16)
    got = ops.add_pos_bcast(y.view, tab.view, B, S, Gt, out=out.view)
    assert got.data_ptr() == out.view.data_ptr()
    assert _same_bits(out, R.add_pos_bcast_ref(y0, pos, B, S, Gt))
    assert _same_bits(y, y0) and _same_bits(tab, pos)


@pytest.mark.parametrize("B,F,N,D", [(2, 3, 4, D) for D in R.WIDTHS] + [(3, 9, 607, 8)], ids=lambda v: str(v))
def test_add_pos_frames(ops, B, F, N, D):
    max_frames = 7
    assert B * F * N == 24 or B * F * N > R.ROW_CAP
    x0, pos = R.rows_bf16((B, F * N, D), 1200 + D), R.table_f32((max_frames, D), 1201 + D)
    idx = R.any_idx(B, max_frames, F, 1202)
    assert int(idx.min()) == 0 and int(idx.max()) == max_frames - 1
    x, tab = _emb(x0), _emb(pos)
    ops.add_pos_frames(x.view, tab.view, idx.to(DEV), N)
    assert _same_bits(x, R.add_pos_frames_ref(x0, pos, idx, N))
    assert _same_bits(tab, pos)


@pytest.mark.parametrize("Ke,Kp", [(3, 4), (0, 4), (3, 0)])
@pytest.mark.parametrize("D", R.WIDTHS)
def test_pred_assemble(ops, D, Ke, Kp):
    _pred_assemble(ops, 2, Ke, Kp, D, 1300 + D)


def test_pred_assemble_past_the_launch_cap(ops):
    _pred_assemble(ops, R.BIG_B, 2000, R.BIG_K - 2000, 8, 1310)


def _pred_assemble(ops, B, Ke, Kp, D, seed):
    N = Ke + Kp + 5
    e0, tok0, pos0 = R.rows_bf16((B * Ke, D), seed), R.table_f32((D,), seed + 1), R.table_f32((N, D), seed + 2)
    idx_e, idx_p = R.any_idx(B, N, Ke, seed + 3), R.any_idx(B, N, Kp, seed + 4)
    ref = R.pred_assemble_ref(e0, tok0, pos0, idx_e, idx_p).view(B * (Ke + Kp), D)
    e, tok, pos, out = _emb(e0), _emb(tok0), _emb(pos0), _out((B * (Ke + Kp), D), BF16)
    got = ops.pred_assemble(e.view, tok.view, pos.view, idx_e.to(DEV), idx_p.to(DEV), out=out.view)
    assert got.data_ptr() == out.view.data_ptr()
    assert _same_bits(out, ref)
    assert _same_bits(e, e0) and _same_bits(tok, tok0) and _same_bits(pos, pos0)
    own = ops.pred_assemble(e.view, tok.view, pos.view, idx_e.to(DEV), idx_p.to(DEV))      # the form that allocates its output
    assert own.shape == ref.shape and torch.equal(own.view(torch.int16).cpu(), ref.view(torch.int16))


def test_slice_sum_past_the_launch_cap(ops):
    B, S, Gt, D = R.BIG_B, R.BIG_K, 2, 8
    x0 = R.rows_bf16((B, Gt, S, D), 1400)
    x, out = _emb(x0.view(B * Gt * S, D)), _out((B * S, D), BF16)
    ops.slice_sum(x.view, B, S, Gt, out=out.view)
    assert _same_bits(out, (x0[:, 0].float() + x0[:, 1].float()).to(BF16).view(B * S, D))


# ------------------------------------------------------------------------------------------------ packers
def _pixels(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g)


@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("p,tub,C", R.PACK_COMBOS, ids=lambda v: str(v))
def test_tubelet_pack_against_the_permutation(ops, p, tub, C, masked):
    B, T, H, W = (R.PACK_SMALL[k] for k in "BTHW")
    N = (T // tub) * (H // p) * (W // p)
    clips0 = _pixels((B, C, T, H, W), 1500 + p + tub + C)
    idx = R.any_idx(B, N, N // 2 + 3, 1501) if masked else None        # unsorted, with repeats
    ref = R.tubelet_ref(clips0, tub, p, idx)
    clips, out = _emb(clips0), _out((B * ref.shape[1], ref.shape[2]), BF16)
    got = ops.tubelet_pack(clips.view, tub, p, None if idx is None else idx.to(DEV), out=out.view)
    assert got.data_ptr() == out.view.data_ptr()
    assert _same_bits(out, ref.reshape(out.view.shape))
    assert _same_bits(clips, clips0)


@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("p,tub,C", R.PACK_COMBOS, ids=lambda v: str(v))
def test_image_pack_against_the_permutation(ops, p, tub, C, masked):
    B, H, W = (R.PACK_SMALL[k] for k in "BHW")
    cells = (H // p) * (W // p)
    img0 = _pixels((B, C, H, W), 1600 + p + tub + C)
    idx = R.any_idx(B, 3 * cells, cells // 2 + 3, 1601) if masked else None     # indices into the (t, h, w) grid of a 3-slice clip
    ref = R.image_ref(img0, tub, p, idx)
    img, out = _emb(img0), _out((B * ref.shape[1], ref.shape[2]), BF16)
    got = ops.image_pack(img.view, tub, p, None if idx is None else idx.to(DEV), out=out.view)
    assert got.data_ptr() == out.view.data_ptr()
    assert _same_bits(out, ref.reshape(out.view.shape))
    assert _same_bits(img, img0)


@pytest.fixture(scope="module")
def big_pixels():
    b = R.PACK_BIG
    return _pixels((b["B"], b["C"], b["T"], b["H"], b["W"]), 1700)


def test_tubelet_pack_past_the_flat_cap(ops, big_pixels):
    b = R.PACK_BIG
    K = (b["T"] // b["tub"]) * (b["H"] // b["p"]) * (b["W"] // b["p"])
    assert R.pack_chunks(b["B"], K, b["C"], b["tub"], b["p"]) == 2102784 > R.FLAT_CAP
    ref = R.tubelet_ref(big_pixels, b["tub"], b["p"])
    out = _out((b["B"] * K, ref.shape[2]), BF16)
    ops.tubelet_pack(big_pixels.to(DEV), b["tub"], b["p"], out=out.view)
    assert _same_bits(out, ref.reshape(out.view.shape))


def test_image_pack_past_the_flat_cap(ops, big_pixels):
    """the same pixels read as 4 images of 3 planes, one tubelet deep: 2 102 784 input chunks"""
    b = R.PACK_BIG
    img0 = big_pixels.view(b["B"] * b["T"], b["C"], b["H"], b["W"])
    cells = (b["H"] // b["p"]) * (b["W"] // b["p"])
    assert R.pack_chunks(img0.shape[0], cells, b["C"], 1, b["p"]) == 2102784 > R.FLAT_CAP
    ref = R.image_ref(img0, 1, b["p"])
    out = _out((img0.shape[0] * cells, ref.shape[2]), BF16)
    ops.image_pack(img0.to(DEV), 1, b["p"], out=out.view)
    assert _same_bits(out, ref.reshape(out.view.shape))


# ------------------------------------------------------------------------------------------------ transposes
@pytest.mark.parametrize("M,N", R.TRANSPOSE_SHAPES, ids=lambda v: str(v))
def test_transpose_into_a_dirty_output(ops, M, N):
    """whole matrix and the row-prefix form (M rows of M + 5), into out= prefilled with NaN: the pad columns come back zero"""
    bits = R.payload((M + 5, N), BF16, 1800 + M)
    x = _emb(bits, dtype=BF16)
    for m in (M + 5, M, M - 3):
        out = _out((N, R.pad64(m)), BF16)
        got = ops.transpose(x.view, M=m, out=out.view)
        assert got.data_ptr() == out.view.data_ptr()
        assert _same_bits(out, R.transpose_ref(bits, m))
    own = ops.transpose(x.view[:M])                                     # the form that allocates its output
    assert torch.equal(own.view(torch.int16).cpu(), R.transpose_ref(bits, M))


def test_transpose_multi_into_dirty_outputs(ops):
    """the four shapes in one launch, the third read through a row stride wider than its rows"""
    srcs, outs, desc, blocks = [], [], [], []
    for ti, (M, N) in enumerate(R.TRANSPOSE_SHAPES):
        ld = N + 8 if ti == 2 else N
        bits = R.payload((M, ld), BF16, 1900 + M)
        x, t = _emb(bits, dtype=BF16), _out((N, R.pad64(M)), BF16)
        srcs.append((bits[:, :N], x))
        outs.append(t)
        desc += [x.view.data_ptr(), t.view.data_ptr(), M, N, ld, R.pad64(M)]
        blocks += [v for tm in range(R.pad64(M) // 64) for tn in range(R.cdiv(N, 64)) for v in (ti, tm, tn, 0)]
    ops.transpose_multi(torch.tensor(desc, dtype=torch.int64, device=DEV), torch.tensor(blocks, dtype=torch.int32, device=DEV), len(blocks) // 4)
    for (bits, x), t in zip(srcs, outs):
        assert _same_bits(t, R.transpose_ref(bits, bits.shape[0]))
        assert x.guards_untouched()


@pytest.mark.parametrize("M", R.TCOLSUM_M)
def test_transpose_colsum_on_integers(ops, M):
    """alpha = 0.5 onto an integer-valued old sum: exact in fp32, so equal to the float64 sum; the transpose bit for bit"""
    N = R.TCOLSUM_N
    x0, old = R.int_data((M, N), 2000 + M), R.int_old(N, 2001 + M)
    ref, _, a = R.sum_ref(x0, 0.5, old)
    assert R.exact_in_fp32(a, 0.5, old)
    x, cs = _emb(x0), _emb(old, fill=-7.0)
    t = ops.transpose_colsum(x.view, cs.view, alpha=0.5, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(cs.view.double().cpu(), ref) and cs.guards_untouched()
    assert torch.equal(t.cpu(), R.transpose_ref(x0, M))
    cs2 = _out((N,), F32)                                               # overwrite: the NaN underneath must not reach the result
    ops.transpose_colsum(x.view, cs2.view, alpha=1.0, accumulate=False)
    torch.cuda.synchronize()
    assert torch.equal(cs2.view.double().cpu(), R.sum_ref(x0, 1.0)[0]) and cs2.guards_untouched()


# ------------------------------------------------------------------------------------------------ column sums
def _check_sum(label, got, ref, tol, exact):
    got = got.double().cpu()
    err = (got - ref).abs()
    print(f"{label}: worst |error| {float(err.max()) if err.numel() else 0.0:.3e}, worst error / bound "
          f"{float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0:.3f}")
    if exact:
        assert torch.equal(got, ref), f"{label}: {int((got != ref).sum())} of {ref.numel()} columns differ from the exact sum"
    else:
        assert bool((err <= tol).all()), f"{label}: worst error / bound {float((err / tol.clamp_min(1e-300)).max()):.3f}"


@pytest.mark.parametrize("case", R.COLSUM_CASES, ids=R.colsum_id)
def test_colsum(ops, case):
    c = case
    rows = R.colsum_rows(c)
    for kind in ("int", "normal"):
        x0 = R.int_data((c.rows, c.N), 2100 + c.M) if kind == "int" else R.normal_data((c.rows, c.N), 2101 + c.M)
        x = _emb(x0)
        for alpha, acc in R.COLSUM_RUNS:
            old = None if not acc else (R.int_old(c.N, 2102) if kind == "int" else R.normal_old(c.N, 2103))
            ref, tol, a = R.sum_ref(x0[:c.M], alpha, old, rows)
            if kind == "int":
                assert R.exact_in_fp32(a, alpha, old)
            out = _out((c.N,), F32, shift=8) if old is None else _emb(old, fill=-7.0, shift=8)     # an offset view, NaN where overwritten
            win = {} if not c.group else dict(group=c.group, row_lo=c.lo, row_hi=c.hi)
            ops.colsum(x.view, out.view, M=None if c.rows == c.M else c.M, alpha=alpha, accumulate=acc, **win)
            torch.cuda.synchronize()
            _check_sum(f"colsum {R.colsum_id(c)} {kind} alpha={alpha} accumulate={acc}", out.view, ref, tol, kind == "int")
            assert out.guards_untouched()
        assert _same_bits(x, x0)


# ------------------------------------------------------------------------------------------------ partial and segment reductions
@pytest.mark.parametrize("P", R.REDUCE_P)
def test_reduce_partials(lib, P):
    from jepa_amd.hip.lib import check
    for N in R.REDUCE_N:
        for kind in ("int", "normal"):
            part0 = R.int_data((P, N), 2200 + N, F32) if kind == "int" else R.normal_data((P, N), 2201 + N, F32)
            part = _emb(part0)
            for alpha in (1.0, 0.5):
                for beta in (0.0, 1.0):
                    old = None if beta == 0.0 else (R.int_old(N, 2202) if kind == "int" else R.normal_old(N, 2203))
                    ref, tol, a = R.sum_ref(part0, alpha, old)
                    if kind == "int":
                        assert R.exact_in_fp32(a, alpha, old)
                    out = _out((N,), F32) if old is None else _emb(old, fill=-7.0)
                    check(lib.vj_reduce_partials(_p(part.view), _p(out.view), P, N, alpha, beta, _stream()), "vj_reduce_partials")
                    torch.cuda.synchronize()
                    _check_sum(f"reduce_partials P{P} N{N} {kind} alpha={alpha} beta={beta}", out.view, ref, tol, kind == "int")
                    assert out.guards_untouched()


def _segments(kind, acc):
    """[(part Embedded (the full [P, stride] matrix), part0 [P, N] on the CPU, old or None, out Embedded)] of R.SEGMENTS"""
    segs = []
    for i, (P, N, stride) in enumerate(R.SEGMENTS):
        wide = R.int_data((P, stride), 2300 + i, F32) if kind == "int" else R.normal_data((P, stride), 2301 + i, F32)
        old = None if not acc else (R.int_old(N, 2302 + i) if kind == "int" else R.normal_old(N, 2303 + i))
        segs.append((_emb(wide), wide[:, :N], old, _out((N,), F32) if old is None else _emb(old, fill=-7.0)))
    return segs


@pytest.mark.parametrize("kind", ["int", "normal"])
def test_reduce_segments_sixteen_at_once(ops, kind):
    assert len(R.SEGMENTS) == 16 and any(N == 0 for _, N, _ in R.SEGMENTS) and any(P == 0 and N for P, N, _ in R.SEGMENTS)
    for alpha, acc in R.COLSUM_RUNS:
        segs = _segments(kind, acc)
        ops.reduce_segments([(part.view[:, :p0.shape[1]], out.view) for part, p0, _, out in segs], alpha=alpha, accumulate=acc)
        torch.cuda.synchronize()
        for i, (part, p0, old, out) in enumerate(segs):
            ref, tol, a = R.sum_ref(p0, alpha, old)
            if kind == "int":
                assert R.exact_in_fp32(a, alpha, old)
            _check_sum(f"reduce_segments #{i} P{p0.shape[0]} N{p0.shape[1]} {kind} alpha={alpha} accumulate={acc}", out.view, ref, tol, kind == "int")
            assert out.guards_untouched() and part.guards_untouched()


def test_reduce_segments_refuses_seventeen(ops):
    from jepa_amd.hip.lib import HipKernelError
    segs = [(torch.ones((2, 8), device=DEV), torch.full((8,), -7.0, device=DEV)) for _ in range(17)]
    with pytest.raises(HipKernelError, match="segments"):
        ops.reduce_segments(segs)
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for _, o in segs)
    ops.reduce_segments(segs[:16])
    torch.cuda.synchronize()
    assert all(bool((o == 2.0).all()) for _, o in segs[:16]) and bool((segs[16][1] == -7.0).all())
