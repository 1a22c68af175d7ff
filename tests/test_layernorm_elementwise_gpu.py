"""GPU: every element of every output of the LayerNorm family (csrc/layernorm.hip: layernorm_fwd, ln_rowstats, ln_fold_weights,
layernorm_bwd + column sums through csrc/reduce.hip, target_rows) against a float64 reference and its derived bound
(tests/ln_ref_util.py).  tests/test_norm_loss_optim_gpu.py compares whole tensors by a relative L2 norm at one input distribution
(row variance 4, eps 1e-6), never looks at rstd, and sees ln_fold_weights only through the GEMM that consumes it.  Here:

  * every output buffer (and the backward's workspace) starts as NaN; every element satisfies |out - ref| <= tol with the bound DERIVED
    in the util, nothing is excluded, NaN / inf fail.  The backward is fed the float64 statistics rounded to fp32, so it is checked
    independently of the forward kernel;
  * inputs: today's distribution, rows at 64 +- 3 (cancellation), rows whose variance is ~ eps (at two eps), constant rows (y ==
    bf16(beta) bit for bit, dgamma == 0 exactly, accumulated dgamma == the old value); target_rows also with gamma ~ 2^-9 and
    eps_norm != eps_ln both ways round;
  * D = 8 (one lane) and 1..4 chunks, each full and ragged; 1, 3, 4, 5 rows (fewer than, as many as, more than the waves of a
    workgroup), 8200 rows (waves 0..7 of the capped grid take a second row); the backward also at 16 | 17 | 33 rows (1, 2, 3
    workgroups), at its workgroup cap with trailing workgroups that own no row, and at D % 64 != 0 (one reduction launch per output);
    both template variants (with and without dxsum), with and without dres, alpha 1 and 0.5, overwriting and accumulating;
  * dx holds the same bits whatever alpha is, and sits within one bf16 ulp of the other template variant's;
  * by direct ABI calls: a workspace of exactly vj_layernorm_bwd_ws_bytes(D) inside a NaN guard band (inside the bounds, bit-identical to
    a run on a zeroed workspace, band untouched); every operand a 16-byte-aligned view inside a poisoned allocation (the bits of the
    contiguous twin, surroundings untouched).

tests/test_ln_bound_host.py proves on the CPU that the checker admits a correct emulation and rejects planted defects at these shapes.

Worst err / tol seen on the MI355X over all shapes and variants (information only; the assertion is the derived bound; printed again by
every run with -s):

  kernel                            y / dx   mean    rstd    rs0     rs1     dgamma  dbeta   dxsum   cvec    bf      h
  layernorm_fwd                     0.995    0.109   0.283
  ln_rowstats                                                0.283   0.155
  layernorm_bwd, overwriting        0.996                                    0.229   0.052   0.071
  layernorm_bwd, accumulating       0.996                                    0.964   0.929   0.312
  ln_fold_weights                                                                                    0.011   0.099
  target_rows                                                                                                        0.057
  (146 tests, every element inside its bound, every pin bit-exact, every twin bit-identical; no kernel change was needed.  The bf16
   outputs sit just under 1: some value always lands next to a rounding tie, and half a bf16 ulp IS the bound's first term.  The
   accumulating column sums do so for the same reason: the one fp32 add of the old value is the bound's last term.)
"""
import pytest
import torch

from tests import ln_ref_util as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
WORST = {}                           # (kernel, output) -> worst err / tol over the shapes


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
    for (kernel, name), w in sorted(WORST.items()):
        print(f"[layernorm element-wise] {kernel:<16} {name:<7} worst err/tol {w:.3f}")


def _note(kernel, label, worst):
    for name, w in worst.items():
        WORST[(kernel, name)] = max(WORST.get((kernel, name), 0.0), w)
    print(f"{kernel} {label}: worst err/tol " + " ".join(f"{n} {x:.2f}" for n, x in worst.items()))


def nan(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


# ------------------------------------------------------------------------------------------------ the calls, on the raw ABI
def call_fwd(ops, lib, x, gamma, beta, y, mean, rstd, rows, D, eps):
    from jepa_amd.hip.lib import check
    p = ops._ptr
    check(lib.vj_layernorm_fwd(p(x), p(gamma), p(beta), p(y), p(mean), p(rstd), rows, D, eps, ops._stream()), "vj_layernorm_fwd")


def call_bwd(ops, lib, dy, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, dxsum, alpha, beta_acc, rows, D, ws, nws):
    from jepa_amd.hip.lib import check
    p = ops._ptr
    check(lib.vj_layernorm_bwd_colsum(p(dy), p(x), p(gamma), p(mean), p(rstd), p(dres), p(dx), p(dgamma), p(dbeta), p(dxsum), alpha,
                                      beta_acc, rows, D, p(ws), nws, ops._stream()), "vj_layernorm_bwd_colsum")


def run_forward(ops, lib, case, save_stats=True):
    y = nan((case.rows, case.D), torch.bfloat16)
    mean, rstd = (nan((case.rows,)), nan((case.rows,))) if save_stats else (None, None)
    call_fwd(ops, lib, case.x, case.gamma, case.beta, y, mean, rstd, case.rows, case.D, case.eps)
    return y, mean, rstd


_WS = {}


def nan_workspace(lib, D):
    """a workspace of exactly the size the library asks for, full of NaN before every run."""
    nws = lib.vj_layernorm_bwd_ws_bytes(D)
    assert nws == L.LN_BWD_MAX_BLOCKS * 3 * D * 4
    if D not in _WS:
        _WS.clear()
        _WS[D] = torch.empty(nws // 4, dtype=torch.float32, device=DEV)
    _WS[D].fill_(NAN)
    return _WS[D], nws


def run_backward(ops, lib, case, mean_in, rstd_in, cs, with_dres, alpha, old=None, ws=None):
    """(dx, dgamma, dbeta, dxsum | None): overwriting NaN outputs, or accumulating onto old [3, D]."""
    D = case.D
    dx = nan((case.rows, D), torch.bfloat16)
    outs = [nan((D,)) if old is None else old[i].clone() for i in range(3)]
    if not cs:
        outs[2] = None
    ws, nws = nan_workspace(lib, D) if ws is None else (ws, ws.numel() * 4)
    call_bwd(ops, lib, case.dy, case.x, case.gamma, mean_in, rstd_in, case.dres if with_dres else None, dx, outs[0], outs[1], outs[2],
             alpha, 0.0 if old is None else 1.0, case.rows, D, ws, nws)
    return dx, outs[0], outs[1], outs[2]


# ------------------------------------------------------------------------------------------------ forward + rowstats
@pytest.mark.parametrize("rows,D", L.FWD_SHAPES)
def test_forward_and_rowstats_every_element_within_its_bound(ops, lib, rows, D):
    """y, mean, rstd of layernorm_fwd and both columns of ln_rowstats, every variant; y without the statistics has the same bits."""
    for variant, eps in L.STAT_VARIANTS:
        case = L.make_case(rows, D, variant, eps).to(DEV)
        ref = L.forward_reference(case)
        y, mean, rstd = run_forward(ops, lib, case)
        _note("layernorm_fwd", case.label, L.check(case.label, L.forward_pairs(ref, y, mean, rstd)))
        y2, _, _ = run_forward(ops, lib, case, save_stats=False)
        L.assert_bit_equal(y2, y, f"y without statistics {case.label}")
        if variant == "const":
            L.assert_bit_equal(y, L.bf(case.beta).expand(rows, D).contiguous(), f"y == bf16(beta) {case.label}")
        rs = ops.ln_rowstats(case.x, case.eps, out=nan((rows, 2)))
        _note("ln_rowstats", case.label, L.check(case.label, L.rowstats_pairs(ref, rs)))


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("rows,D", L.BWD_SHAPES)
def test_backward_every_element_within_its_bound(ops, lib, rows, D):
    """dx, dgamma, dbeta, dxsum over both template variants, with and without dres, both alphas; overwriting NaN, then accumulating
    onto known values with the OTHER alpha: dx keeps its bits (alpha never reaches it); across the template variants dx stays within
    one ulp."""
    for variant, eps in L.BWD_VARIANTS:
        case = L.make_case(rows, D, variant, eps).to(DEV)
        mean_in, rstd_in = L.stats_input(case)
        refs, dxs, worst, worst_acc = {}, {}, {}, {}
        for cs, with_dres, alpha in L.BWD_CONFIGS:
            if with_dres not in refs:
                refs[with_dres] = L.backward_reference(case, mean_in, rstd_in, with_dres)
            ref = refs[with_dres]
            out = run_backward(ops, lib, case, mean_in, rstd_in, cs, with_dres, alpha)
            w = L.check(case.label, L.backward_pairs(ref, *out, alpha))
            alpha2 = 1.5 - alpha
            acc = run_backward(ops, lib, case, mean_in, rstd_in, cs, with_dres, alpha2, old=case.old)
            w2 = L.check(case.label + " accumulate", L.backward_pairs(ref, *acc, alpha2, old=case.old))
            L.assert_bit_equal(acc[0], out[0], f"dx under alpha {alpha2} against alpha {alpha} {case.label}")
            for k in w:
                worst[k], worst_acc[k] = max(worst.get(k, 0.0), w[k]), max(worst_acc.get(k, 0.0), w2[k])
            if variant == "const":
                assert not bool(out[1].any()), f"dgamma != 0 {case.label}"
                L.assert_bit_equal(acc[1][None], case.old[0][None], f"accumulated dgamma == old {case.label}")
            if with_dres in dxs:
                assert L.one_ulp_apart(ref, dxs[with_dres], out[0]), f"dx with / without dxsum more than one ulp apart {case.label}"
            dxs[with_dres] = out[0]
        _note("layernorm_bwd", case.label, worst)
        _note("layernorm_bwd +=", case.label, worst_acc)


WS_SHAPES = [(33, 520), (17, 2048), (777, 1280), (16385, 8)]


@pytest.mark.parametrize("rows,D", WS_SHAPES)
def test_backward_workspace_of_exact_size_starts_dirty(ops, lib, rows, D):
    """the workspace is exactly vj_layernorm_bwd_ws_bytes(D) long, a view inside a guard band, and full of NaN: the outputs stay inside
    their bounds and hold the bits of a run on a zeroed workspace; the band is untouched."""
    case = L.make_case(rows, D, "rand", 1e-6).to(DEV)
    mean_in, rstd_in = L.stats_input(case)
    ref = L.backward_reference(case, mean_in, rstd_in, True)
    nws = lib.vj_layernorm_bwd_ws_bytes(D)
    dirty = L.Embedded(1, nws // 4, nws // 4, 0, torch.float32, DEV, True)
    assert bool(torch.isnan(dirty.view).all())
    clean = torch.zeros(nws // 4, dtype=torch.float32, device=DEV)
    res = [run_backward(ops, lib, case, mean_in, rstd_in, True, True, 0.5, ws=ws) for ws in (dirty.view, clean)]
    L.check(case.label, L.backward_pairs(ref, *res[0], 0.5))
    for name, a, b in zip(("dx", "dgamma", "dbeta", "dxsum"), res[0], res[1]):
        L.assert_bit_equal(a.reshape(-1, D), b.reshape(-1, D), f"{name}, dirty against zeroed workspace {case.label}")
    assert dirty.surroundings_intact()


def _embed(t, nan_fill):
    """t (1-D or 2-D, contiguous) as a view 16 bytes past an aligned address inside a poisoned allocation."""
    t2 = t.reshape(1, -1) if t.dim() == 1 else t
    e = L.Embedded(t2.shape[0], t2.shape[1], t2.shape[1], 8 if t.dtype == torch.bfloat16 else 4, t.dtype, t.device, nan_fill,
                   t2 if nan_fill else None)
    assert e.view.data_ptr() % 16 == 0 and e.view.is_contiguous()
    return e


def _out(shape, dtype=torch.float32):
    return _embed(torch.empty(shape, dtype=dtype, device=DEV), False)


LAYOUT_SHAPES = [(5, 8), (17, 520), (33, 1544), (5, 2048)]


@pytest.mark.parametrize("rows,D", LAYOUT_SHAPES)
def test_operands_as_views_inside_poisoned_memory(ops, lib, rows, D):
    """every input surrounded by NaN, every output by the 0xA5 pattern: the bits of the contiguous twin, inside the bounds, and not a
    byte changed around the outputs.  Forward, rowstats and backward."""
    case = L.make_case(rows, D, "rand", 1e-6).to(DEV)
    ref = L.forward_reference(case)
    e_x, e_g, e_b = _embed(case.x, True), _embed(case.gamma, True), _embed(case.beta, True)
    twin = run_forward(ops, lib, case)
    e_y, e_m, e_r = _out((rows, D), torch.bfloat16), _out((rows,)), _out((rows,))
    call_fwd(ops, lib, e_x.view, e_g.view, e_b.view, e_y.view, e_m.view, e_r.view, rows, D, case.eps)
    for name, e, t in (("y", e_y, twin[0]), ("mean", e_m, twin[1]), ("rstd", e_r, twin[2])):
        L.assert_bit_equal(e.view, t.reshape(e.view.shape), f"{name} {case.label}")
        assert e.surroundings_intact(), name
    L.check(case.label, L.forward_pairs(ref, e_y.view, e_m.view.reshape(-1), e_r.view.reshape(-1)))
    e_rs = _out((rows, 2))
    ops.ln_rowstats(e_x.view, case.eps, out=e_rs.view)
    L.assert_bit_equal(e_rs.view, ops.ln_rowstats(case.x, case.eps, out=nan((rows, 2))), f"rowstats {case.label}")
    assert e_rs.surroundings_intact()
    L.check(case.label, L.rowstats_pairs(ref, e_rs.view))

    mean_in, rstd_in = L.stats_input(case)
    bref = L.backward_reference(case, mean_in, rstd_in, True)
    twin = run_backward(ops, lib, case, mean_in, rstd_in, True, True, 0.5)
    e_dy, e_dres, e_mi, e_ri = _embed(case.dy, True), _embed(case.dres, True), _embed(mean_in, True), _embed(rstd_in, True)
    e_dx, e_o = _out((rows, D), torch.bfloat16), [_out((D,)) for _ in range(3)]
    ws, nws = nan_workspace(lib, D)
    call_bwd(ops, lib, e_dy.view, e_x.view, e_g.view, e_mi.view, e_ri.view, e_dres.view, e_dx.view, e_o[0].view, e_o[1].view, e_o[2].view,
             0.5, 0.0, rows, D, ws, nws)
    for name, e, t in zip(("dx", "dgamma", "dbeta", "dxsum"), [e_dx] + e_o, twin):
        L.assert_bit_equal(e.view, t.reshape(e.view.shape), f"{name} {case.label}")
        assert e.surroundings_intact(), name
    L.check(case.label, L.backward_pairs(bref, e_dx.view, *(e.view.reshape(-1) for e in e_o), 0.5))


# ------------------------------------------------------------------------------------------------ ln_fold_weights
@pytest.mark.parametrize("N,K", L.FOLD_SHAPES)
def test_fold_weights_pinned_and_within_bounds(ops, N, K):
    """Wf bit-equal to (W * gamma).to(bfloat16); cvec against the float64 sum of the kernel's own Wf, bf against b + W beta; with b and
    without; contiguous and as views inside poisoned memory."""
    case = L.make_fold_case(N, K).to(DEV)
    for with_b in (True, False):
        b = case.b if with_b else None
        Wf, cvec, bfv = ops.ln_fold_weights(case.W, b, case.gamma, case.beta, Wf=nan((N, K), torch.bfloat16), cvec=nan((N,)), bf=nan((N,)))
        ref = L.fold_reference(case, Wf, with_b)
        L.assert_bit_equal(Wf, ref["Wf"], f"Wf {case.label}")
        _note("ln_fold_weights", f"{case.label} b={with_b}",
              L.check(case.label, [("cvec", cvec, ref["cvec"], ref["tol_cvec"]), ("bf", bfv, ref["bf"], ref["tol_bf"])]))
        e_W, e_g, e_be = _embed(case.W, True), _embed(case.gamma, True), _embed(case.beta, True)
        e_b = _embed(case.b, True) if with_b else None
        e_Wf, e_c, e_bf = _out((N, K), torch.bfloat16), _out((N,)), _out((N,))
        ops.ln_fold_weights(e_W.view, e_b.view.reshape(-1) if with_b else None, e_g.view.reshape(-1), e_be.view.reshape(-1), Wf=e_Wf.view,
                            cvec=e_c.view, bf=e_bf.view)
        for name, e, t in (("Wf", e_Wf, Wf), ("cvec", e_c, cvec), ("bf", e_bf, bfv)):
            L.assert_bit_equal(e.view, t.reshape(e.view.shape), f"{name} as a view {case.label}")
            assert e.surroundings_intact(), name


# ------------------------------------------------------------------------------------------------ target_rows
@pytest.mark.parametrize("K,D", L.TARGET_SHAPES)
def test_target_rows_every_element_within_its_bound(ops, K, D):
    """B = 2, N = 7; index rows with 0, N - 1, duplicates and descending order; every variant, eps_norm != eps_ln both ways round; h of a
    duplicated index has the same bits at both positions."""
    for variant, e1, e2 in L.TARGET_VARIANTS:
        case = L.make_target_case(K, D, variant, e1, e2).to(DEV)
        ref = L.target_reference(case)
        h = ops.target_rows(case.x, case.gamma, case.beta, case.idx, case.B, case.N, case.eps_norm, case.eps_ln, out=nan((case.B, K, D)))
        _note("target_rows", case.label, L.check(case.label, [("h", h.view(-1, D), ref["h"], ref["tol_h"])]))
        for b, row in enumerate(case.idx.tolist()):
            for k1 in range(K):
                for k2 in range(k1 + 1, K):
                    if row[k1] == row[k2]:
                        L.assert_bit_equal(h[b, k1][None], h[b, k2][None], f"h of the duplicated index {row[k1]} {case.label}")
    e_x, e_g, e_b, e_h = _embed(case.x, True), _embed(case.gamma, True), _embed(case.beta, True), _out((case.B * K, D))
    ops.target_rows(e_x.view, e_g.view.reshape(-1), e_b.view.reshape(-1), case.idx, case.B, case.N, case.eps_norm, case.eps_ln, out=e_h.view)
    L.assert_bit_equal(e_h.view, h.view(-1, D), f"h as a view {case.label}")
    assert e_h.surroundings_intact()
