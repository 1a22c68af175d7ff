"""bf16 MFMA GEMM family (csrc/gemm*.hip) checked PER ELEMENT against a float64 reference, and on strided, minimally aligned, aliasing
operands.  tests/test_gemm_gpu.py compares whole matrices by a relative L2 norm (a few hundred wrong elements pass) and only ever passes
contiguous operands from fresh allocations; the other GEMM tests assert bit-identity TO the flags = 0 kernel it checks.  Here:

  * every element of every output satisfies |out - ref| <= tol with the bound DERIVED in tests/gemm_ref_util.py (bf16 rounding of the one
    stored value + the gamma_K bound of an fp32 dot product, doubled); nothing is excluded, NaN / inf fail;
  * integer operands (every partial sum < 2^24): outputs bit-equal to the rounded float64 result, ties included;
  * every operand as a view into a larger poisoned allocation (lda / ldb / ldc / ldr / ldaux above the row length, bases 8- or 16-byte
    aligned only, in-place residual, column slices of one buffer): bit-identical to the contiguous twin, padding and bands untouched.

The shapes are the smallest that reach every tile edge, pipeline prologue and kernel route (gemm_ref_util.NT_SHAPES); the float64
references are computed on the device once per shape and shared.  tests/test_gemm_bound_host.py proves on the CPU that the checker
rejects planted errors.

Worst err / tol seen on the MI355X over all shapes (information only; the assertion is the derived bound; printed again by every run
with -s).  107 cases, all inside the bound, every integer case bit-exact, every layout bit-identical; no kernel change was needed.

  vj_gemm_bf16_nt, by kernel family (flags)     plain   bias+res  dgelu   qkv     f32 (alpha 0.5, beta 2)
    0x000  automatic (128x128 BK64; persistent  0.987   0.981     0.978   0.975   0.008
           256x256 at 2305 x 2312)
    0x020  256x256 BK64                         0.987   0.981     0.978   0.975   0.008
    0x080  BK32 ring                            0.987   0.981     0.978   0.975   0.008
    0x0c0  8-phase / persistent                 0.987   0.981     0.976   0.961   0.008
    0x100  4-wave, two workgroups per CU        0.987   0.981     0.976   0.961   0.008
  (the bf16 forms sit just under 1: with 10^5 ... 10^6 elements some value always lands next to a rounding tie, and half a bf16 ulp IS
   the bound's first term; the fp32 form shows how little of the accumulation term a correct kernel uses.  0xc0 / 0x100 skip the
   K % 64 != 0 shape, hence their own maxima.)
  vj_gemm_bf16_nt_splitk, every flag:  0.008 (alpha 0.5, beta 2)   0.009 (alpha 0.25, beta 0)
  vj_gemm_bf16_tn_splitk:              0.114 (beta 2; at T = 1 the one rounding of the result is 1/8 of a (K + 3) e bound)   0.010 (beta 0)
  vj_gemm_bf16_tn_grouped:             0.009 (beta 2)   0.010 (beta 0)
  fused column sums of vj_gemm_bf16_nt_dgelu_colsum at 2305 x 2312 x 256:  below 0.001
"""
import ctypes
import functools

import pytest
import torch

from tests import gemm_ref_util as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
QS = 0.125 * 1.4426950408889634      # head_dim^-0.5 * log2(e) of a 64-wide head
WORST = {}                           # (entry point, flags, form) -> worst err / tol over the shapes


@pytest.fixture(scope="module")
def ops():
    from jepa_amd.hip import ops as _ops
    return _ops


@pytest.fixture(scope="module", autouse=True)
def _print_worst():
    yield
    for (entry, flags, form), w in sorted(WORST.items(), key=lambda kv: (kv[0][0], kv[0][1], kv[0][2])):
        print(f"[gemm element-wise] {entry:<10} flags {flags:#05x} {form:<9} worst err/tol {w:.3f}")


def _ids(params):
    return [f"{M}x{N}x{K}-{f:#x}" for M, N, K, f in params]


def _note(entry, flags, form, worst):
    key = (entry, flags, form)
    WORST[key] = max(WORST.get(key, 0.0), worst)


@functools.lru_cache(maxsize=None)
def _case(M, N, K, kind):
    """operands + float64 acc / S of one (shape, kind), on the device, computed once and never modified."""
    d = (R.random_case if kind == "random" else R.integer_case)(M, N, K, 1000 + M + N + K, DEV)
    acc, S = R.acc_and_s(d["A"], d["B"])
    return d, acc, S


def _forms(d, N, kind):
    """(label, epilogue, gemm_nt kwargs, reference kwargs) of the output forms of one problem."""
    a4 = QS if kind == "random" else 0.25
    forms = [("plain", R.EPI_BF16, {}, {}),
             ("bias+res", R.EPI_BF16, dict(bias=d["bias"], residual=d["res"]), dict(bias=d["bias"], res=d["res"])),
             ("dgelu", R.EPI_DGELU, dict(aux_in=d["aux"]), dict(aux_in=d["aux"])),
             ("f32", R.EPI_F32, dict(alpha=0.5, beta=2.0), dict(alpha=0.5, beta=2.0, C0=d["C0"]))]
    if N % 12 == 0:
        forms.append(("qkv", R.EPI_QKV, dict(bias=d["bias"], alpha=a4), dict(bias=d["bias"], alpha=a4)))
    return forms


def _check(out, ref, tol, kind, entry, flags, form, where):
    label = f"{entry} flags={flags:#x} {form} {kind} {where}"
    if kind == "integer":
        R.assert_bit_equal(out, R.exact_output(ref, out.dtype), label)
    else:
        _note(entry, flags, form, R.assert_elementwise(out, ref, tol, label))


# ================================================================================================ 3. element-wise: vj_gemm_bf16_nt
NT_PARAMS = [(M, N, K, f) for (M, N, K) in R.NT_SHAPES + R.QKV_EXTRA_SHAPES for f in R.NT_FLAGS if R.flags_apply(f, K)]


@pytest.mark.parametrize("M,N,K,flags", NT_PARAMS, ids=_ids(NT_PARAMS))
def test_gemm_nt_every_element_inside_the_derived_bound(ops, M, N, K, flags):
    """vj_gemm_bf16_nt under every kernel selection: epilogue 0 without and with bias + residual, epilogue 2, epilogue 4 (N % 12 == 0),
    epilogue 3 with alpha = 0.5, beta = 2 on a non-zero C0 -- random data against the per-element bound, integer data bit-exact.  Outputs
    start as NaN, so an element nobody wrote fails too."""
    for kind in ("random", "integer"):
        d, acc, S = _case(M, N, K, kind)
        for form, epi, kw, rkw in _forms(d, N, kind):
            if epi == R.EPI_F32:
                out = d["C0"].clone()
            else:
                out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
            ops.gemm_nt(d["A"], d["B"], out=out, epilogue=epi, flags=flags, **kw)
            ref, tol = R.reference(epi, acc, S, K, **rkw)
            _check(out, ref, tol, kind, "nt", flags, form, (M, N, K))


# ================================================================================================ 3. split-K, TN, grouped (fp32 outputs)
def _f32_check(out, acc, S, K, alpha, beta, C0, kind, entry, flags, where):
    ref, tol = R.reference(R.EPI_F32, acc, S, K, alpha=alpha, beta=beta, C0=C0)
    _check(out, ref, tol, kind, entry, flags, f"a{alpha:g}b{beta:g}", where)


@pytest.mark.parametrize("M,N,K", R.NT_SPLITK_SHAPES)
@pytest.mark.parametrize("flags", R.NT_FLAGS)
def test_gemm_nt_splitk_every_element(ops, M, N, K, flags):
    """vj_gemm_bf16_nt_splitk (workspace given: K = 4096 has 64 K-tiles to split; K = 64 is the one-slice edge): accumulate and overwrite."""
    for kind in ("random", "integer"):
        d, acc, S = _case(M, N, K, kind)
        for alpha, beta in ((0.5, 2.0), (0.25, 0.0)):
            out = d["C0"].clone() if beta != 0.0 else torch.full((M, N), float("nan"), device=DEV)
            ops.gemm_wgrad(d["A"], d["B"], out, alpha=alpha, beta=beta, flags=flags)
            _f32_check(out, acc, S, K, alpha, beta, d["C0"], kind, "nt_splitk", flags, (M, N, K))


@functools.lru_cache(maxsize=None)
def _tn_case(T, N1, N2, kind):
    """dY [T, N1], X [T, N2] row-major as the backward pass leaves them; acc / S of dW = dY^T X (reduction length T)."""
    d, acc, S = _case(N1, N2, (T + 31) // 32 * 32, kind)      # drawn as the NT problem A = dY^T, B = X^T ...
    dY, X = d["A"][:, :T].t().contiguous(), d["B"][:, :T].t().contiguous()   # ... cut to T tokens
    acc, S = R.acc_and_s(dY.t(), X.t())
    return dY, X, d["C0"], acc, S


@pytest.mark.parametrize("T,N1,N2", R.TN_SHAPES)
def test_gemm_tn_splitk_every_element(ops, T, N1, N2):
    """vj_gemm_bf16_tn_splitk: T <= 64 is one partial token tile, 65 and 129 sit one past a tile, 4099 is long enough for the split."""
    for kind in ("random", "integer"):
        dY, X, C0, acc, S = _tn_case(T, N1, N2, kind)
        for alpha, beta in ((0.5, 2.0), (0.25, 0.0)):
            out = C0.clone() if beta != 0.0 else torch.full((N1, N2), float("nan"), device=DEV)
            ops.gemm_wgrad_tn(dY, X, out, alpha=alpha, beta=beta)
            _f32_check(out, acc, S, T, alpha, beta, C0, kind, "tn_splitk", 0, (T, N1, N2))


@pytest.mark.parametrize("T", R.GROUPED_T)
def test_gemm_tn_grouped_every_element(ops, T):
    """vj_gemm_bf16_tn_grouped: four problems with different N1 / N2 over the same T tokens in one launch."""
    for kind in ("random", "integer"):
        cases = [_tn_case(T, n1, n2, kind) for n1, n2 in R.GROUPED_DIMS]
        for alpha, beta in ((0.5, 2.0), (0.25, 0.0)):
            outs = [c[2].clone() if beta != 0.0 else torch.full_like(c[2], float("nan")) for c in cases]
            ops.gemm_wgrad_tn_grouped([(c[0], c[1], o) for c, o in zip(cases, outs)], alpha=alpha, beta=beta)
            for (dY, X, C0, acc, S), o, dims in zip(cases, outs, R.GROUPED_DIMS):
                _f32_check(o, acc, S, T, alpha, beta, C0, kind, "tn_grouped", 0, (T,) + dims)


# ================================================================================================ 4. layouts
LDC_OFFS = [(4, 0), (8, 0), (64, 0), (4, 4), (8, 4), (64, 4)]      # (ldc - N, base offset in elements; 4 bf16 = 8-byte aligned only)
LAYOUT_PARAMS = [(M, N, K, f) for (M, N, K) in [(129, 132, 96), (257, 264, 256), (300, 384, 320), (513, 520, 256)]
                 for f in (0, 0x20, 0xC0, 0x100) if R.flags_apply(f, K)] + [(2305, 2312, 256, 0)]


def _strided_inputs(d, K, N):
    return (R.embed_input(d["A"], K + 8), R.embed_input(d["B"], K + 24), R.embed_input(d["res"], N + 12))


@pytest.mark.parametrize("M,N,K,flags", LAYOUT_PARAMS, ids=_ids(LAYOUT_PARAMS))
def test_gemm_nt_strided_operands_are_bit_identical(ops, M, N, K, flags):
    """Every operand a view into a larger poisoned allocation: lda = K + 8, ldb = K + 24 (bases shifted by 16 bytes, NaN around), ldr = N + 12,
    ldaux = N + 4 / N + 8, C (and aux_out) with ldc in {N + 4, N + 8, N + 64} at a 16-byte and at an 8-byte-only aligned base inside a
    0xA5 byte pattern.  Each output must equal the contiguous twin bit for bit -- whichever epilogue variant or kernel the layout routes
    it to (gemm_epilogue_try_staged refuses ldc % 8 != 0 or C & 15; the persistent kernel declines them) -- and every byte around it must
    be unchanged."""
    d, _, _ = _case(M, N, K, "random")
    A, B, bias, res, aux, C0 = d["A"], d["B"], d["bias"], d["res"], d["aux"], d["C0"]
    Ae, Be, Re = _strided_inputs(d, K, N)
    run = functools.partial(ops.gemm_nt, flags=flags)
    twin_res = run(A, B, bias=bias, residual=res)
    dg_twin = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    twin_gelu = run(A, B, bias=bias, aux_out=dg_twin, epilogue=R.EPI_GELU)
    twin_dgelu = run(A, B, aux_in=aux, epilogue=R.EPI_DGELU)
    twin_qkv = run(A, B, bias=bias, epilogue=R.EPI_QKV, alpha=QS) if N % 12 == 0 else None
    twin_f32 = run(A, B, out=C0.clone(), epilogue=R.EPI_F32, alpha=0.5, beta=2.0)
    assert not torch.isnan(twin_res.float()).any()

    def out_c(pad, off, dtype=torch.bfloat16, value=None):
        return R.embed_output(M, N, N + pad, off, dtype, DEV, value)

    for pad, off in LDC_OFFS:
        where = f"{(M, N, K)} flags={flags:#x} ldc=N+{pad} off={off}"
        Ce = out_c(pad, off)
        run(Ae.view, Be.view, out=Ce.view, bias=bias, residual=Re.view)
        R.assert_bit_equal(Ce.view, twin_res, "bias+res " + where)
        assert Ce.surroundings_intact(), "bias+res: bytes around C changed, " + where
        for auxpad, auxoff in ((4, 4), (8, 4), (8, 0)):
            Xe = R.embed_input(aux, N + auxpad, 8 if auxoff == 0 else 4)
            Ce = out_c(pad, off)
            run(Ae.view, Be.view, out=Ce.view, aux_in=Xe.view, epilogue=R.EPI_DGELU)
            R.assert_bit_equal(Ce.view, twin_dgelu, f"dgelu ldaux=N+{auxpad} " + where)
            assert Ce.surroundings_intact(), "dgelu: bytes around C changed, " + where
            Ce, De = out_c(pad, off), out_c(auxpad, auxoff)
            run(Ae.view, Be.view, out=Ce.view, bias=bias, aux_out=De.view, epilogue=R.EPI_GELU)
            R.assert_bit_equal(Ce.view, twin_gelu, f"gelu ldaux=N+{auxpad} auxoff={auxoff} " + where)
            R.assert_bit_equal(De.view, dg_twin, f"gelu' ldaux=N+{auxpad} auxoff={auxoff} " + where)
            assert Ce.surroundings_intact() and De.surroundings_intact(), "gelu: bytes around C / aux_out changed, " + where
        if twin_qkv is not None:
            Ce = out_c(pad, off)
            run(Ae.view, Be.view, out=Ce.view, bias=bias, epilogue=R.EPI_QKV, alpha=QS)
            R.assert_bit_equal(Ce.view, twin_qkv, "qkv " + where)
            assert Ce.surroundings_intact(), "qkv: bytes around C changed, " + where
    for off in (0, 4):      # fp32 C: base 16-byte aligned, ldc = N + 4
        Ce = out_c(4, off, torch.float32, C0)
        run(Ae.view, Be.view, out=Ce.view, epilogue=R.EPI_F32, alpha=0.5, beta=2.0)
        R.assert_bit_equal(Ce.view, twin_f32, f"f32 {(M, N, K)} flags={flags:#x} off={off}")
        assert Ce.surroundings_intact(), "f32: bytes around C changed"
    for E, t in ((Ae, A), (Be, B), (Re, res)):
        assert E.surroundings_intact() and torch.equal(E.view, t)


@pytest.mark.parametrize("M,N,K,flags", LAYOUT_PARAMS, ids=_ids(LAYOUT_PARAMS))
def test_gemm_nt_aliasing_operands_are_bit_identical(ops, M, N, K, flags):
    """residual == C (in place); C and residual as the two column halves of one [M, 2N] buffer (the address RANGES overlap although no
    element does: the persistent kernel, whose shifted edge tiles rewrite their neighbours' rows, must decline and the fallback give the
    same bits); A and C as column slices of one buffer."""
    d, _, _ = _case(M, N, K, "random")
    A, B, bias, res = d["A"], d["B"], d["bias"], d["res"]
    run = functools.partial(ops.gemm_nt, flags=flags)
    twin = run(A, B, bias=bias, residual=res)
    twin_nb = run(A, B, residual=res)
    where = f"{(M, N, K)} flags={flags:#x}"
    for pad, off in ((0, 0), (8, 0), (4, 4)):
        Ce = R.embed_output(M, N, N + pad, off, torch.bfloat16, DEV, res)
        run(A, B, out=Ce.view, bias=bias, residual=Ce.view)
        R.assert_bit_equal(Ce.view, twin, f"in place ldc=N+{pad} off={off} " + where)
        assert Ce.surroundings_intact(), "in place: bytes around C changed, " + where
        Ce = R.embed_output(M, N, N + pad, off, torch.bfloat16, DEV, res)
        run(A, B, out=Ce.view, residual=Ce.view)
        R.assert_bit_equal(Ce.view, twin_nb, f"in place, no bias ldc=N+{pad} off={off} " + where)
    # two column halves of one buffer
    He = R.embed_output(M, 2 * N, 2 * N, 0, torch.bfloat16, DEV, torch.cat([torch.full_like(res, float("nan")), res], dim=1))
    c_half, r_half = He.view[:, :N], He.view[:, N:]
    run(A, B, out=c_half, bias=bias, residual=r_half)
    R.assert_bit_equal(c_half, twin, "column halves " + where)
    assert torch.equal(r_half, res) and He.surroundings_intact(), "column halves: the residual half or the bands changed, " + where
    # A and C as column slices of one buffer (row stride a multiple of 8 elements: lda % 8 == 0)
    ld = (K + N + 7) // 8 * 8
    Se = R.embed_output(M, K + N, ld, 0, torch.bfloat16, DEV, torch.cat([A, torch.full_like(res, float("nan"))], dim=1))
    a_sl, c_sl = Se.view[:, :K], Se.view[:, K:]
    run(a_sl, B, out=c_sl, bias=bias, residual=res)
    R.assert_bit_equal(c_sl, twin, "A | C slices " + where)
    assert torch.equal(a_sl, A) and Se.surroundings_intact(), "A | C slices: A or the padding changed, " + where


def _ln_operands(ops, M, N, K):
    g = torch.Generator().manual_seed(5 * M + N + K)
    x = R.bf(torch.randn(M, K, generator=g) * (1.0 + 2.0 * torch.rand(M, 1, generator=g)) + 0.5 * torch.randn(M, 1, generator=g)).to(DEV)
    W = (torch.randn(N, K, generator=g) * 0.03).to(DEV)
    b = (torch.randn(N, generator=g) * 0.1).to(DEV)
    gamma = (1.0 + 0.3 * torch.randn(K, generator=g)).to(DEV)
    beta = (0.2 * torch.randn(K, generator=g)).to(DEV)
    Wf, cvec, bfold = ops.ln_fold_weights(W, b, gamma, beta)
    return x, Wf, cvec, bfold, ops.ln_rowstats(x, 1e-6)


LNFOLD_PARAMS = [(257, 264, 256, 0), (257, 264, 256, 0x20), (257, 264, 256, 0xC0), (300, 384, 320, 0), (300, 384, 320, 0x20),
                 (300, 384, 320, 0xC0), (2305, 2304, 256, 0)]


@pytest.mark.parametrize("M,N,K,flags", LNFOLD_PARAMS, ids=_ids(LNFOLD_PARAMS))
def test_gemm_lnfold_strided_operands_are_bit_identical(ops, M, N, K, flags):
    """vj_gemm_bf16_nt_lnfold, epilogues 0, 1 and 4, with strided X, Wf and C: bit-identical to the contiguous call (the 2305-row case
    is taken by the persistent kernel on its own when the layout allows it)."""
    x, Wf, cvec, bfold, rs = _ln_operands(ops, M, N, K)
    Xe, We = R.embed_input(x, K + 8), R.embed_input(Wf, K + 24)
    for epi, alpha in ((R.EPI_BF16, 1.0), (R.EPI_GELU, 1.0), (R.EPI_QKV, QS)):
        twin = ops.gemm_nt_lnfold(x, Wf, bfold, rs, cvec, epilogue=epi, alpha=alpha, flags=flags)
        assert not torch.isnan(twin.float()).any()
        for pad, off in LDC_OFFS:
            Ce = R.embed_output(M, N, N + pad, off, torch.bfloat16, DEV)
            ops.gemm_nt_lnfold(Xe.view, We.view, bfold, rs, cvec, out=Ce.view, epilogue=epi, alpha=alpha, flags=flags)
            R.assert_bit_equal(Ce.view, twin, f"lnfold epilogue {epi} {(M, N, K)} flags={flags:#x} ldc=N+{pad} off={off}")
            assert Ce.surroundings_intact(), f"lnfold epilogue {epi}: bytes around C changed (ldc=N+{pad} off={off})"
    assert Xe.surroundings_intact() and We.surroundings_intact()


def _dgelu_colsum(ops, A, B, C, aux, colpart, flags=0):
    lib = ops.load_library()
    fused = ctypes.c_int(-1)
    M, K = A.shape
    N = B.shape[0]
    ops.check(lib.vj_gemm_bf16_nt_dgelu_colsum(ops._ptr(A), A.stride(0), ops._ptr(B), B.stride(0), ops._ptr(C), C.stride(0), M, N, K,
                                               ops._ptr(aux), aux.stride(0), ops._ptr(colpart), colpart.shape[0], flags,
                                               ctypes.byref(fused), ops._stream()), "vj_gemm_bf16_nt_dgelu_colsum")
    return fused.value


@pytest.mark.parametrize("M,N,K", [(257, 264, 256), (513, 520, 256), (2305, 2312, 256)])
def test_gemm_dgelu_colsum_strided_operands(ops, M, N, K):
    """vj_gemm_bf16_nt_dgelu_colsum with strided A, B, C, aux_in: C is the plain epilogue-2 GEMM's bit for bit on every layout; at the
    2305-row shape the column sums are fused (*fused = 1) on the contiguous AND on the strided 16-byte aligned layout, with partial rows
    that reduce to the same sums -- and those sums are the float64 column sums of acc * aux_in within (K + 1 + M) e sum_m S |aux_in| (the
    fp32 dot products, the product, M fp32 adds) -- while the layouts that make the persistent kernel decline (ldc % 8 == 4, C 8-byte
    aligned only) give *fused = 0 and the same C."""
    d, acc, S = _case(M, N, K, "random")
    A, B, aux = d["A"], d["B"], d["aux"]
    lib = ops.load_library()
    rows = lib.vj_gemm_colsum_rows(M)
    big = M >= 2305
    twin = ops.gemm_nt(A, B, aux_in=aux, epilogue=R.EPI_DGELU)
    C = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    cp = torch.full((rows, N), float("nan"), device=DEV)
    assert _dgelu_colsum(ops, A, B, C, aux, cp) == (1 if big else 0)
    R.assert_bit_equal(C, twin, f"dgelu_colsum contiguous {(M, N, K)}")
    sums = cp.sum(0) if big else None
    if big:
        ref = (acc * aux.double()).sum(0)
        tol = (K + 1 + M) * R.E_F32 * (S * aux.double().abs()).sum(0)
        _note("dgelu_csum", 0, "colsum", R.assert_elementwise(sums[None].double(), ref[None], tol[None], "fused column sums"))
    Ae, Be = R.embed_input(A, K + 8), R.embed_input(B, K + 24)
    for pad, off, auxpad in ((8, 0, 8), (64, 0, 4), (4, 0, 8), (8, 4, 8), (64, 4, 4)):
        Xe = R.embed_input(aux, N + auxpad)
        Ce = R.embed_output(M, N, N + pad, off, torch.bfloat16, DEV)
        cp2 = torch.full((rows, N), float("nan"), device=DEV)
        fused = _dgelu_colsum(ops, Ae.view, Be.view, Ce.view, Xe.view, cp2)
        where = f"{(M, N, K)} ldc=N+{pad} off={off} ldaux=N+{auxpad}"
        aligned = (N + pad) % 8 == 0 and off == 0
        assert fused == (1 if big and aligned else 0), (fused, where)
        R.assert_bit_equal(Ce.view, twin, "dgelu_colsum " + where)
        assert Ce.surroundings_intact(), "dgelu_colsum: bytes around C changed, " + where
        if fused:
            assert torch.equal(cp2.sum(0), sums), "fused column sums differ from the contiguous call's, " + where


def _tn_call(ops, dY, X, out, T, alpha, beta):
    lib = ops.load_library()
    ws = ops.Scratch.get(ops.WGRAD_WS_BYTES, dY.device, "wgrad")
    ops.check(lib.vj_gemm_bf16_tn_splitk(ops._ptr(dY), dY.stride(0), ops._ptr(X), X.stride(0), ops._ptr(out), out.stride(0), T,
                                         dY.shape[1], X.shape[1], alpha, beta, ops._ptr(ws), ops.WGRAD_WS_BYTES, ops._stream()),
              "vj_gemm_bf16_tn_splitk")


@pytest.mark.parametrize("T,N1,N2", [(63, 8, 264), (65, 136, 72), (129, 256, 256), (4099, 128, 136)])
def test_gemm_tn_strided_operands_are_bit_identical(ops, T, N1, N2):
    """vj_gemm_bf16_tn_splitk through the C ABI (the ops wrapper insists on contiguous tensors) with ldy = N1 + 8, ldx = N2 + 24 inside NaN
    and ldw = N2 + 4 inside the byte pattern: the contiguous call's bits, accumulate and overwrite."""
    dY, X, C0, _, _ = _tn_case(T, N1, N2, "random")
    Ye, Xe = R.embed_input(dY, N1 + 8), R.embed_input(X, N2 + 24)
    for alpha, beta in ((0.5, 2.0), (0.25, 0.0)):
        twin = C0.clone()
        _tn_call(ops, dY, X, twin, T, alpha, beta)
        for off in (0, 4):
            We = R.embed_output(N1, N2, N2 + 4, off, torch.float32, DEV, C0)
            _tn_call(ops, Ye.view, Xe.view, We.view, T, alpha, beta)
            R.assert_bit_equal(We.view, twin, f"tn_splitk {(T, N1, N2)} beta={beta} off={off}")
            assert We.surroundings_intact(), "tn_splitk: bytes around dW changed"
    assert Ye.surroundings_intact() and Xe.surroundings_intact()


@pytest.mark.parametrize("T", R.GROUPED_T)
def test_gemm_tn_grouped_strided_operands_are_bit_identical(ops, T):
    """vj_gemm_bf16_tn_grouped through the C ABI: four problems whose dY, X and dW all have row strides above their row lengths."""
    lib = ops.load_library()
    cases = [_tn_case(T, n1, n2, "random") for n1, n2 in R.GROUPED_DIMS]
    ws = ops.Scratch.get(ops.GROUP_WS_BYTES, DEV, "wgrad_group")

    def call(probs, alpha, beta):
        flat = []
        for dy, x, out in probs:
            flat += [dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), dy.shape[1], x.shape[1]]
        arr = (ctypes.c_int64 * len(flat))(*[int(v) for v in flat])
        ops.check(lib.vj_gemm_bf16_tn_grouped(ctypes.addressof(arr), len(probs), T, alpha, beta, ops._ptr(ws), ops.GROUP_WS_BYTES,
                                              ops._stream()), "vj_gemm_bf16_tn_grouped")
        torch.cuda.synchronize()

    ins = [(R.embed_input(c[0], c[0].shape[1] + 8), R.embed_input(c[1], c[1].shape[1] + 24)) for c in cases]
    for alpha, beta in ((0.5, 2.0), (0.25, 0.0)):
        twins = [c[2].clone() for c in cases]
        call([(c[0], c[1], t) for c, t in zip(cases, twins)], alpha, beta)
        outs = [R.embed_output(c[2].shape[0], c[2].shape[1], c[2].shape[1] + 4, 4 * (i & 1), torch.float32, DEV, c[2]) for i, c in enumerate(cases)]
        call([(ye.view, xe.view, o.view) for (ye, xe), o in zip(ins, outs)], alpha, beta)
        for o, t, dims in zip(outs, twins, R.GROUPED_DIMS):
            R.assert_bit_equal(o.view, t, f"tn_grouped T={T} {dims} beta={beta}")
            assert o.surroundings_intact(), "tn_grouped: bytes around dW changed"
    assert all(ye.surroundings_intact() and xe.surroundings_intact() for ye, xe in ins)


@pytest.mark.parametrize("flags", [0, 0x20, 0xC0])
def test_gemm_nt_splitk_strided_operands_are_bit_identical(ops, flags):
    """vj_gemm_bf16_nt_splitk with lda = K + 8, ldb = K + 24, ldc = N + 4 (the partials in the workspace stay dense)."""
    M, N, K = R.NT_SPLITK_SHAPES[1]
    d, _, _ = _case(M, N, K, "random")
    twin = d["C0"].clone()
    ops.gemm_wgrad(d["A"], d["B"], twin, alpha=0.5, beta=2.0, flags=flags)
    Ae, Be = R.embed_input(d["A"], K + 8), R.embed_input(d["B"], K + 24)
    for off in (0, 4):
        Ce = R.embed_output(M, N, N + 4, off, torch.float32, DEV, d["C0"])
        ops.gemm_wgrad(Ae.view, Be.view, Ce.view, alpha=0.5, beta=2.0, flags=flags)
        R.assert_bit_equal(Ce.view, twin, f"nt_splitk flags={flags:#x} off={off}")
        assert Ce.surroundings_intact(), "nt_splitk: bytes around C changed"
