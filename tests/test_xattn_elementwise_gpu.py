"""GPU: every element of the attentive probe's cross-attention outputs (csrc/xattn.hip: out, lse2, dq, dkv) against a float64 reference
and its derived bound (tests/xattn_ref_util.py).  tests/test_probe_gpu.py and tests/test_xattn_long_gpu.py compare whole tensors by a
relative L2 norm against fp32 SDPA: a few wrong key rows of dkv pass, and no input of theirs makes a single key matter to out.  Here:

  * every output buffer starts as NaN; every element satisfies |out - ref| <= tol with the bound DERIVED in the util, nothing is
    excluded, NaN / inf fail.  The backward is fed lse2 of the float64 forward, so it is checked independently of the forward kernel;
  * the aimed cases put all of the probability on one edge key per (sample, head, query) -- the last key, the last key of chunk 0, the
    first of chunk 1, the first key of the last row-group pass: without residual out must equal v[j*] bit for bit;
  * single-workgroup path: N = 1, 2, ngrp - 1 | ngrp | ngrp + 1 for every row-group count ngrp = 256 / (hd / 8), 513; every head size;
    NQ = 3 forward, NQ = 1 forward + backward; q shared and per sample; B = H = 2 everywhere;
  * the last LDS score slot (backward N = 19 132, forward N = 38 264) and the split forms just above (ragged last chunk, full chunks
    only, a chunk of one key);
  * layouts by direct ABI calls: q_bstride above NQ * D and every operand a 16-byte-aligned view inside a poisoned allocation
    (bit-identical to the contiguous twin, surroundings untouched); a split workspace of exactly vj_xattn_ws_bytes inside a guard
    band, pre-filled with NaN (inside the bounds, bit-identical to a run on a zeroed workspace, band untouched).

tests/test_xattn_bound_host.py proves on the CPU that the checker admits a correct emulation and rejects planted defects at these
shapes.

Worst err / tol seen on the MI355X over all shapes and variants (information only; the assertion is the derived bound; printed again
by every run with -s).  205 tests, every element inside its bound, every aimed forward bit-exact, every layout bit-identical; no kernel
change was needed.

  entry point       path                      out     lse2    dq      dk      dv
  vj_xattn_fwd      single workgroup          0.996   0.041
  vj_xattn_fwd_ws   single (N = 38 264)       0.912   0.040
  vj_xattn_fwd_ws   split                     0.955   0.041
  vj_xattn_bwd      single workgroup                          0.923   0.989   0.995
  vj_xattn_bwd_ws   single (N = 19 132)                       0.610   0.989   0.995
  vj_xattn_bwd_ws   split                                     0.866   0.991   0.995
  (the bf16 outputs sit just under 1: among 10^5 ... 10^7 elements some value always lands next to a rounding tie, and half a bf16 ulp
   IS the bound's first term; lse2, an fp32 output, shows how little of the accumulation terms a correct kernel uses.)
"""
import functools

import pytest
import torch

from tests import xattn_ref_util as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
WORST = {}                           # (entry point, path, output) -> worst err / tol over the shapes


@pytest.fixture(scope="module")
def ops():
    from jepa_amd.hip import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib():
    from jepa_amd.hip.lib import load_library
    return load_library()


@pytest.fixture(scope="module", autouse=True)
def _print_worst():
    yield
    print()
    for (entry, path, name), w in sorted(WORST.items()):
        print(f"[xattn element-wise] {entry:<16} {path:<7} {name:<5} worst err/tol {w:.3f}")


def _note(entry, path, worst):
    for name, w in worst.items():
        WORST[(entry, path, name)] = max(WORST.get((entry, path, name), 0.0), w)


@functools.lru_cache(maxsize=16)
def _problem(NQ, N, hd, shared, variant, backward):
    """(case, lse_in | None, float64 reference) of one (shape, variant, direction) on the device: computed once, never modified."""
    split = N > (X.BWD_MAX if backward else X.FWD_MAX)
    case = X.make_case(X.B0, NQ, N, X.H0, hd, shared, variant, split=split).to(DEV)
    if backward:
        lse_in = X.lse_input(case).contiguous()
        return case, lse_in, X.backward_reference(case, lse_in, split)
    return case, None, X.forward_reference(case, split)


def _qstride(case):
    return 0 if case.shared else case.NQ * case.D


def _nan_ws(lib, case, backward):
    """a NaN-filled workspace of the size the entry point asks for (None below the single-workgroup limit)."""
    n = lib.vj_xattn_ws_bytes(case.B, case.NQ, case.N, case.H, case.hd, int(backward))
    assert n >= 0 and n % 4 == 0
    return (torch.full((n // 4,), NAN, dtype=torch.float32, device=DEV) if n else None), n


def call_forward(ops, lib, case, q, q_bstride, kv, resid, out, lse, ws, nws, entry):
    from jepa_amd.hip.lib import check
    c, p = case, ops._ptr
    if entry == "vj_xattn_fwd":
        rc = lib.vj_xattn_fwd(p(q), q_bstride, p(kv), p(resid), p(out), p(lse), c.B, c.NQ, c.N, c.H, c.hd, c.scale, ops._stream())
    else:
        rc = lib.vj_xattn_fwd_ws(p(q), q_bstride, p(kv), p(resid), p(out), p(lse), c.B, c.NQ, c.N, c.H, c.hd, c.scale, p(ws), nws,
                                 ops._stream())
    check(rc, entry)


def call_backward(ops, lib, case, q, q_bstride, kv, dy, lse_in, dq, dkv, ws, nws, entry):
    from jepa_amd.hip.lib import check
    c, p = case, ops._ptr
    if entry == "vj_xattn_bwd":
        rc = lib.vj_xattn_bwd(p(q), q_bstride, p(kv), p(dy), p(lse_in), p(dq), p(dkv), c.B, 1, c.N, c.H, c.hd, c.scale, ops._stream())
    else:
        rc = lib.vj_xattn_bwd_ws(p(q), q_bstride, p(kv), p(dy), p(lse_in), p(dq), p(dkv), c.B, 1, c.N, c.H, c.hd, c.scale, p(ws), nws,
                                 ops._stream())
    check(rc, entry)


def run_forward(ops, lib, case, entry):
    """(out, lse2) of the contiguous case on NaN-filled outputs and a NaN-filled workspace."""
    out = torch.full((case.B * case.NQ, case.D), NAN, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((case.B, case.H, case.NQ), NAN, dtype=torch.float32, device=DEV)
    ws, nws = _nan_ws(lib, case, False) if entry.endswith("_ws") else (None, 0)
    call_forward(ops, lib, case, case.q, _qstride(case), case.kv, case.resid, out, lse, ws, nws, entry)
    return out, lse


def run_backward(ops, lib, case, lse_in, entry):
    dq = torch.full((case.B, case.D), NAN, dtype=torch.bfloat16, device=DEV)
    dkv = torch.full((case.B * case.N, 2 * case.D), NAN, dtype=torch.bfloat16, device=DEV)
    ws, nws = _nan_ws(lib, case, True) if entry.endswith("_ws") else (None, 0)
    call_backward(ops, lib, case, case.q, _qstride(case), case.kv, case.dy, lse_in, dq, dkv, ws, nws, entry)
    return dq, dkv


def forward_within_bounds(ops, lib, NQ, N, hd, shared, variant, entry):
    case, _, ref = _problem(NQ, N, hd, shared, variant, False)
    path = "split" if N > X.FWD_MAX else "single"
    assert (lib.vj_xattn_ws_bytes(case.B, NQ, N, case.H, hd, 0) > 0) == (path == "split")
    out, lse = run_forward(ops, lib, case, entry)
    w = X.check_forward(case, out, lse, ref)
    if variant == "aimed":
        X.assert_bit_equal(out, X.aimed_expected(case), f"out == v[j*] {case.label}")
    _note(entry, path, w)
    print(f"{entry} {path} {case.label}: worst err/tol " + " ".join(f"{n} {x:.2f}" for n, x in w.items()))


def backward_within_bounds(ops, lib, N, hd, shared, variant, entry):
    case, lse_in, ref = _problem(1, N, hd, shared, variant, True)
    path = "split" if N > X.BWD_MAX else "single"
    assert (lib.vj_xattn_ws_bytes(case.B, 1, N, case.H, hd, 1) > 0) == (path == "split")
    dq, dkv = run_backward(ops, lib, case, lse_in, entry)
    w = X.check_backward(case, dq, dkv, ref)
    _note(entry, path, w)
    print(f"{entry} {path} {case.label}: worst err/tol " + " ".join(f"{n} {x:.2f}" for n, x in w.items()))


# ------------------------------------------------------------------------------------------------ every element inside its bound
def test_single_workgroup_limits(lib):
    """the limits the shapes below are built around are the library's own."""
    for hd in (8, 128):
        assert lib.vj_xattn_ws_bytes(X.B0, 3, X.FWD_MAX, X.H0, hd, 0) == 0 and lib.vj_xattn_ws_bytes(X.B0, 3, X.FWD_MAX + 1, X.H0, hd, 0) > 0
        assert lib.vj_xattn_ws_bytes(X.B0, 1, X.BWD_MAX, X.H0, hd, 1) == 0 and lib.vj_xattn_ws_bytes(X.B0, 1, X.BWD_MAX + 1, X.H0, hd, 1) > 0


@pytest.mark.parametrize("N,hd", X.SINGLE_SHAPES)
def test_single_workgroup_every_element_within_its_bound(ops, lib, N, hd):
    """the thread mapping's edges through vj_xattn_fwd / vj_xattn_bwd: NQ = 3 forward, NQ = 1 forward + backward; every variant; q shared
    and per sample."""
    for shared in X.shared_settings(N, hd):
        for variant in X.VARIANTS:
            forward_within_bounds(ops, lib, 3, N, hd, shared, variant, "vj_xattn_fwd")
            forward_within_bounds(ops, lib, 1, N, hd, shared, variant, "vj_xattn_fwd")
            backward_within_bounds(ops, lib, N, hd, shared, variant, "vj_xattn_bwd")


@pytest.mark.parametrize("variant", X.VARIANTS)
@pytest.mark.parametrize("N,hd", X.LARGE_BWD_SHAPES)
def test_backward_at_the_lds_limit_and_split(ops, lib, N, hd, variant):
    """vj_xattn_bwd_ws at the last LDS score slot (single workgroup) and just above it (split: ragged last chunk, ten full chunks, a
    chunk of one key)."""
    for shared in X.shared_settings(N, hd):
        backward_within_bounds(ops, lib, N, hd, shared, variant, "vj_xattn_bwd_ws")


@pytest.mark.parametrize("variant", X.VARIANTS)
@pytest.mark.parametrize("N,hd", X.LARGE_FWD_SHAPES)
def test_forward_at_the_lds_limit_and_split(ops, lib, N, hd, variant):
    """vj_xattn_fwd_ws, NQ = 3, at the last LDS score slot and just above it; the aimed queries select three different edge keys."""
    for shared in X.shared_settings(N, hd):
        forward_within_bounds(ops, lib, 3, N, hd, shared, variant, "vj_xattn_fwd_ws")


# ------------------------------------------------------------------------------------------------ layouts
def _embed(t, nan_fill, ld=None, offset=8):
    """t [rows, cols] as a view (row stride ld, base `offset` elements = 16 bytes past an aligned address) inside a poisoned allocation."""
    return X.Embedded(t.shape[0], t.shape[1], ld or t.shape[1], offset, t.dtype, t.device, nan_fill, t if nan_fill else None)


def _out_like(rows, cols, dtype):
    return _embed(torch.empty(rows, cols, dtype=dtype, device=DEV), False, offset=8 if dtype == torch.bfloat16 else 4)


LAYOUT_SHAPES = [(257, 24), (257, 80), (19133, 24), (38265, 24)]     # single workgroup; the split backward; both split


@pytest.mark.parametrize("N,hd", LAYOUT_SHAPES)
def test_operands_as_views_inside_poisoned_memory(ops, lib, N, hd):
    """per-sample q with q_bstride = NQ * D + 24; q, kv, resid, dy, lse2_in surrounded by NaN; out, lse2, dq, dkv surrounded by the 0xA5
    pattern: the bits of the contiguous twin, inside the bounds, and not a byte changed around the outputs."""
    for NQ in (3, 1):
        case, _, ref = _problem(NQ, N, hd, False, "plain", False)
        B, D = case.B, case.D
        twin_out, twin_lse = run_forward(ops, lib, case, "vj_xattn_fwd_ws")
        e_q = _embed(case.q.view(B, NQ * D), True, ld=NQ * D + 24)
        e_kv, e_res = _embed(case.kv, True), _embed(case.resid, True)
        e_out, e_lse = _out_like(B * NQ, D, torch.bfloat16), _out_like(1, B * case.H * NQ, torch.float32)
        ws, nws = _nan_ws(lib, case, False)
        call_forward(ops, lib, case, e_q.view, e_q.ld, e_kv.view, e_res.view, e_out.view, e_lse.view, ws, nws, "vj_xattn_fwd_ws")
        X.assert_bit_equal(e_out.view, twin_out, f"out {case.label}")
        X.assert_bit_equal(e_lse.view, twin_lse.view(1, -1), f"lse2 {case.label}")
        assert e_out.surroundings_intact() and e_lse.surroundings_intact()
        X.check_forward(case, e_out.view.contiguous(), e_lse.view.contiguous(), ref)
    case, lse_in, ref = _problem(1, N, hd, False, "plain", True)
    twin_dq, twin_dkv = run_backward(ops, lib, case, lse_in, "vj_xattn_bwd_ws")
    e_q = _embed(case.q.view(B, D), True, ld=D + 24)
    e_kv, e_dy, e_lin = _embed(case.kv, True), _embed(case.dy, True), _embed(lse_in.view(1, -1), True, offset=4)
    e_dq, e_dkv = _out_like(B, D, torch.bfloat16), _out_like(B * N, 2 * D, torch.bfloat16)
    ws, nws = _nan_ws(lib, case, True)
    call_backward(ops, lib, case, e_q.view, e_q.ld, e_kv.view, e_dy.view, e_lin.view, e_dq.view, e_dkv.view, ws, nws, "vj_xattn_bwd_ws")
    X.assert_bit_equal(e_dq.view, twin_dq, f"dq {case.label}")
    X.assert_bit_equal(e_dkv.view, twin_dkv, f"dkv {case.label}")
    assert e_dq.surroundings_intact() and e_dkv.surroundings_intact()
    X.check_backward(case, e_dq.view.contiguous(), e_dkv.view.contiguous(), ref)


@pytest.mark.parametrize("N,hd,backward", [(19133, 24, True), (20481, 128, True), (38265, 24, False), (40961, 8, False)])
def test_split_workspace_of_exact_size_starts_dirty(ops, lib, N, hd, backward):
    """the workspace is exactly vj_xattn_ws_bytes long, a view inside a guard band, and full of NaN: the outputs stay inside their
    bounds and hold the bits of a run on a zeroed workspace; the band is untouched."""
    NQ = 1 if backward else 3
    case, lse_in, ref = _problem(NQ, N, hd, X.shared_settings(N, hd)[0], "plain", backward)
    nws = lib.vj_xattn_ws_bytes(case.B, NQ, N, case.H, hd, int(backward))
    assert nws > 0 and nws % 4 == 0
    dirty = X.Embedded(1, nws // 4, nws // 4, 0, torch.float32, DEV, True)
    assert bool(torch.isnan(dirty.view).all())
    clean = torch.zeros(nws // 4, dtype=torch.float32, device=DEV)
    res = []
    for ws in (dirty.view, clean):
        if backward:
            o1 = torch.full((case.B, case.D), NAN, dtype=torch.bfloat16, device=DEV)
            o2 = torch.full((case.B * N, 2 * case.D), NAN, dtype=torch.bfloat16, device=DEV)
            call_backward(ops, lib, case, case.q, _qstride(case), case.kv, case.dy, lse_in, o1, o2, ws, nws, "vj_xattn_bwd_ws")
        else:
            o1 = torch.full((case.B * NQ, case.D), NAN, dtype=torch.bfloat16, device=DEV)
            o2 = torch.full((case.B, case.H, NQ), NAN, dtype=torch.float32, device=DEV)
            call_forward(ops, lib, case, case.q, _qstride(case), case.kv, case.resid, o1, o2, ws, nws, "vj_xattn_fwd_ws")
        res.append((o1, o2))
    (X.check_backward if backward else X.check_forward)(case, res[0][0], res[0][1], ref)
    X.assert_bit_equal(res[0][0], res[1][0], f"first output, dirty against zeroed workspace {case.label}")
    X.assert_bit_equal(res[0][1].reshape(res[0][1].shape[0], -1), res[1][1].reshape(res[1][1].shape[0], -1),
                       f"second output, dirty against zeroed workspace {case.label}")
    assert dirty.surroundings_intact()
