"""GPU: every element of every output of the kernels a training step ends in -- csrc/loss.hip (latent_loss, token_pstd, reg_grad,
reg_finish) and csrc/optim.hip (adamw_ema, its guarded form with step_advance, ema_update, sqnorm, grad_stats_multi) -- against a
float64 reference and its derived bound, and bit for bit against the pins (tests/step_end_ref_util.py: the derivations, the variants
and the shapes).  tests/test_norm_loss_optim_gpu.py compares AdamW with torch.optim.AdamW at one size after three steps from zero
moments, the EMA at a momentum of 0.5 on integers, token_pstd below 33 rows and the loss's power branch on integers.  Here:

  * every output buffer starts as NaN (or as the known old value of an accumulating run); every element satisfies |out - ref| <= tol,
    nothing is excluded, NaN / inf fail -- except where the reference itself is non-finite (latent_loss, `nonfinite`), and there the
    class is pinned: NaN where torch's autograd gives NaN, the same infinity where it gives one;
  * every loop edge: one chunk, a partly filled workgroup, the grid-stride trip of latent_loss (512 x 256 chunks), reg_grad and AdamW /
    EMA (2048 x 256), sqnorm (1024 x 256); token_pstd's second row per lane (K > 32) and ragged column slabs; grad_stats' empty
    trailing chunks and scalar tail, inside an arena whose every gap is NaN;
  * AdamW from arbitrary state, one step per call, all eight present / None combinations of the nullable buffers, every operand a view
    inside poisoned memory whose surroundings must not change; the guarded form with both selectors, clipping on, capped and off,
    skipped through either counter; the EMA's contraction bit for bit in all three call sites.

tests/test_step_end_bound_host.py proves on the CPU that these checks admit a correct emulation and reject planted defects at these
shapes.  The worst err / tol per output is printed at the end of every run (-s)."""
import pytest
import torch

from tests import step_end_ref_util as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
WORST = {}
REL = {}                             # token_pstd: variant -> worst relative error of pstd (what the shift by row 0 costs)


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
        print(f"[step-end element-wise] {kernel:<20} {name:<9} worst err/tol {w:.3f}")
    for variant, r in REL.items():
        print(f"[step-end element-wise] token_pstd {variant:<13} worst relative error of pstd {r:.2e}")


def _note(kernel, label, worst):
    for name, w in worst.items():
        WORST[(kernel, name)] = max(WORST.get((kernel, name), 0.0), w)
    print(f"{kernel} {label}: worst err/tol " + " ".join(f"{n} {x:.2f}" for n, x in worst.items()))


def nan(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def embed(t, poison_nan=False):
    """a 1-D tensor as a 16-byte-aligned view inside a poisoned allocation (NaN around inputs, the byte pattern around outputs)."""
    e = S.Embedded(1, t.numel(), t.numel(), 8 if t.dtype == torch.bfloat16 else 4, t.dtype, DEV, poison_nan, t.reshape(1, -1))
    assert e.view.data_ptr() % 16 == 0
    return e


def flat(e):
    return None if e is None else e.view.reshape(-1)


# ------------------------------------------------------------------------------------------------ latent_loss
@pytest.mark.parametrize("p", S.LOSS_P)
@pytest.mark.parametrize("numel", S.LOSS_NUMEL)
def test_latent_loss_every_element_within_its_bound(ops, numel, p):
    """loss and dz, every variant, with and without dz, overwriting NaN and accumulating onto a known value; dz has the same bits in
    both; the signs of zero gradients and the class of non-finite ones are pinned."""
    for variant in S.LOSS_VARIANTS:
        case = S.make_loss_case(numel, variant).to(DEV)
        worst, dzs = {}, []
        for old in (None, S.LOSS_OLD):
            ref = S.loss_reference(case, p, old=old)
            for with_dz in (True, False):
                loss = nan((1,)) if old is None else torch.full((1,), old, device=DEV)
                dz = nan((numel,), torch.bfloat16) if with_dz else None
                ops.latent_loss(case.z, case.h, loss, p=p, out_scale=case.out_scale, accumulate=old is not None, dz=dz, gscale=S.LOSS_GSCALE)
                w = S.check(f"{case.label} p={p}", S.loss_pairs(ref, loss[0], dz))
                assert S.loss_pins_hold(case, ref, p, loss[0], dz), f"zero / non-finite pins {case.label} p={p} dz={with_dz} old={old}"
                for k, x in w.items():
                    worst[k] = max(worst.get(k, 0.0), x)
                if with_dz:
                    dzs.append(dz)
        assert torch.equal(dzs[0].view(torch.int16), dzs[1].view(torch.int16)), f"dz differs between overwriting and accumulating {case.label}"
        _note(f"latent_loss p={p:g}", case.label, worst)


# ------------------------------------------------------------------------------------------------ token_pstd
@pytest.mark.parametrize("K,D", S.PSTD_SHAPES)
def test_token_pstd_every_element_within_its_bound(ops, K, D):
    """pstd and both columns of stats; with and without stats, overwriting and accumulating; the const variant bit for bit."""
    for variant in S.PSTD_VARIANTS:
        case = S.make_pstd_case(K, D, variant).to(DEV)
        ref = S.pstd_reference(case)
        worst = {}
        for with_stats, acc in S.PSTD_RUNS:
            pstd = case.old.clone() if acc else nan((case.B, D))
            stats = nan((case.B, D, 2)) if with_stats else None
            ops.token_pstd(case.z, pstd, case.B, K, D, acc, stats=stats)
            w = S.check(case.label, S.pstd_pairs(ref, pstd, stats, case.old if acc else None))
            for k, x in w.items():
                worst[k] = max(worst.get(k, 0.0), x)
            if not acc:
                REL[variant] = max(REL.get(variant, 0.0), float(((pstd.double() - ref["pstd"]).abs() / ref["pstd"]).max()))
                if variant == "const":
                    assert S.pstd_const_pins_hold(case, pstd, stats), f"const pins {case.label}"
        _note("token_pstd", case.label, worst)


# ------------------------------------------------------------------------------------------------ reg_grad, reg_finish
@pytest.mark.parametrize("B,K,D", S.REG_SHAPES)
def test_reg_grad_every_element_within_its_bound(ops, B, K, D):
    for n_masks in S.REG_MASKS:
        case = S.make_reg_case(B, K, D, n_masks).to(DEV)
        ref = S.reg_grad_reference(case)
        dz = case.dz0.clone()
        ops.reg_grad(case.z, case.pstd_sum, case.stats, dz, B, K, D, n_masks, S.REG_COEF)
        _note("reg_grad", case.label, S.check(case.label, [("dz", dz, ref["dz"], ref["tol_dz"])]))
        off = ref["inactive"]
        assert bool(off.any()) and not bool(off.all())
        assert torch.equal(dz[off].view(torch.int16), case.dz0[off].view(torch.int16)), f"inactive elements changed {case.label}"


@pytest.mark.parametrize("n", S.FINISH_N)
def test_reg_finish_within_its_bound(ops, n):
    for n_masks in S.FINISH_MASKS:
        case = S.make_finish_case(n, n_masks).to(DEV)
        ref = S.reg_finish_reference(case)
        out = nan((1,))
        ops.reg_finish(case.pstd, n_masks, out)
        _note("reg_finish", case.label, S.check(case.label, [("reg", out, ref["out"].reshape(1), ref["tol_out"].reshape(1))]))


# ------------------------------------------------------------------------------------------------ adamw + ema
def run_adam(ops, case, c):
    """one call on fresh copies of the case's state, every operand inside poisoned memory: (out for adam_check, the Embedded list)."""
    n = case.n
    has_pb, has_tgt, has_tb = bool(c["nulls"] & 1), bool(c["nulls"] & 2), bool(c["nulls"] & 4)
    e = dict(p=embed(case.p), g=embed(case.g, True), m=embed(case.m), v=embed(case.v),
             pb=embed(torch.full((n,), S.PB_FILL, dtype=torch.bfloat16, device=DEV)) if has_pb else None,
             tgt=embed(case.tgt) if has_tgt else None,
             tb=embed(torch.full((n,), S.TB_FILL, dtype=torch.bfloat16, device=DEV)) if has_tb else None)
    args = [flat(e[k]) for k in ("p", "g", "m", "v", "pb", "tgt", "tb")]
    hp = [S.HP["lr"], c["wd"], S.HP["beta1"], S.HP["beta2"], S.HP["eps"]]
    step = None
    if c["kind"] == "plain":
        ops.adamw_ema(*args, *hp, c["step"], c["gscale"], c["ema"])
    else:
        gstat = torch.tensor(c["gstat"], dtype=torch.float32, device=DEV)
        step_dev = torch.full((1,), c["t0"], dtype=torch.float32, device=DEV)
        ops.step_advance(gstat, step_dev)
        ops.adamw_ema_guarded(*args, *hp, c["gscale"], c["ema"], gstat, c["sel"], c["clip"], c["norm_scale"], step_dev)
        step = step_dev.item()
    out = {k: flat(e[k]) for k in ("p", "m", "v", "pb", "tgt", "tb")}
    out["step"] = step
    return out, [x for x in e.values() if x is not None]


@pytest.mark.parametrize("n", S.ADAM_N)
def test_adamw_ema_one_step_from_arbitrary_state(ops, n):
    """p, m, v inside their bounds; tgt inside its bound and bit-equal to the fma of its branch; the shadows bit-equal to the cast of
    the kernel's own fp32 outputs; a skipped step leaves p, m, v, p_bf16 and step_dev alone; nothing around any operand changes."""
    worst = {}
    for variant in S.ADAM_VARIANTS:
        case = S.make_adam_case(n, variant).to(DEV)
        for c in S.adam_configs(n):
            out, embedded = run_adam(ops, case, c)
            w = S.adam_check(case, c, out)
            for k, x in w.items():
                worst[k] = max(worst.get(k, 0.0), x)
            assert torch.equal(embedded[1].view, case.g.reshape(1, -1)), "the gradient was written"
            for x in embedded:
                assert x.surroundings_intact(), f"memory around an operand changed: {case.label} {S.config_label(c)}"
    _note("adamw_ema", f"n{n}", worst)


@pytest.mark.parametrize("n", S.EMA_N)
def test_ema_update_contraction_pinned(ops, n):
    """ema_kernel: fmaf(fl(1 - m), src, fl(m * tgt)) bit for bit at both momenta, with and without the bf16 shadow."""
    case = S.make_ema_case(n).to(DEV)
    for ema in S.EMA_MOMENTA:
        expect, ties = S.ema_expected(case.tgt, case.src, ema, False)
        assert ties == 0
        ref, tol = S.ema_reference(case.tgt, case.src, ema)
        for shadow in (True, False):
            e_t, e_s = embed(case.tgt), embed(case.src, True)
            e_b = embed(torch.full((n,), S.TB_FILL, dtype=torch.bfloat16, device=DEV)) if shadow else None
            ops.ema_update(flat(e_t), flat(e_s), flat(e_b), ema)
            _note("ema_update", f"{case.label} m={ema:.3f}", S.check(case.label, [("tgt", flat(e_t), ref, tol)]))
            S.assert_bit_equal(e_t.view, expect.reshape(1, -1), f"tgt == fmaf(1 - m, src, fl(m tgt)) {case.label} m={ema}")
            if shadow:
                S.assert_bit_equal(e_b.view, S.bf(e_t.view), f"tgt_bf16 == bf16(tgt) {case.label}")
            for x in (e_t, e_s, e_b):
                assert x is None or x.surroundings_intact()


# ------------------------------------------------------------------------------------------------ sqnorm
@pytest.mark.parametrize("n", S.SQ_N)
def test_sqnorm_within_its_bound(ops, n):
    """n = 0 writes [0, 0] and leaves the old values when accumulating; a non-finite value is counted wherever it sits."""
    case = S.make_sq_case(n).to(DEV)
    for old in (None, S.SQ_OLD):
        ref, tol = S.sq_reference(case, None if old is None else old[0])
        out = nan((2,)) if old is None else torch.tensor(old, dtype=torch.float32, device=DEV)
        ops.sqnorm(case.x, out, accumulate=old is not None)
        _note("sqnorm", f"{case.label} accumulate={old is not None}", S.check(case.label, [("sumsq", out[:1], ref.reshape(1), tol.reshape(1))]))
        assert out[1].item() == (0.0 if old is None else old[1])
        if n == 0:
            assert out[0].item() == (0.0 if old is None else old[0])
    for name, i in S.sq_nonfinite_positions(n).items():
        x = case.x.clone()
        x[i] = NAN
        x[i ^ 1] = float("inf")
        out = nan((2,))
        ops.sqnorm(x, out)
        assert out[1].item() == 2.0 and not bool(torch.isfinite(out[0])), (name, out.tolist())


# ------------------------------------------------------------------------------------------------ grad_stats_multi
def test_grad_stats_every_partial_within_its_bound(ops, lib):
    """the raw [n_tensors, 8, 3] output of one launch over an arena whose gaps are NaN: every per-chunk partial finite and inside its
    bound, chunks past a tensor's end exactly 0; with both moment arenas and with neither (columns 1, 2 exactly 0)."""
    from jepa_amd.hip.lib import check
    case = S.make_gs_case().to(DEV)
    T, p = len(case.offsets), ops._ptr
    assert lib.vj_grad_stats_chunks() == S.GS_CHUNKS
    for moments in (True, False):
        ref, tol = S.gs_reference(case, moments)
        out = nan((T, S.GS_CHUNKS, 3))
        check(lib.vj_grad_stats_multi(p(case.G), p(case.M1 if moments else None), p(case.M2 if moments else None), p(case.desc), T, p(out),
                                      ops._stream()), "vj_grad_stats_multi")
        assert bool(torch.isfinite(out).all()), "a partial is not finite: an element outside [offset, offset + numel) was read"
        _note("grad_stats_multi", f"moments={moments}", S.check(case.label, [("partials", out.view(-1, 3), ref.view(-1, 3), tol.view(-1, 3))]))
        assert bool((out[tol == 0] == 0).all())
        total = ops.grad_stats_multi(case.G, case.M1 if moments else None, case.M2 if moments else None, case.desc, T)
        assert torch.equal(total, out.sum(dim=1))
