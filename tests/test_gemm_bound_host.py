"""The element-wise GEMM checker of tests/gemm_ref_util.py, tested on the CPU: it accepts what a correct kernel computes (the plain
fp32-accumulate emulation of every epilogue, at every shape the GPU tests use) and REJECTS each planted error -- a failure here means
tests/test_gemm_elementwise_gpu.py could not fail either.  The bound is derived (module docstring of gemm_ref_util), not measured."""
import functools

import pytest
import torch

from tests import gemm_ref_util as R

ALL_NT = R.NT_SHAPES + R.QKV_EXTRA_SHAPES + R.NT_SPLITK_SHAPES
# the TN / grouped entry points as the NT problem they are: dW[N1, N2] = dY^T X, reduction length T
ALL_TN = [(n1, n2, T) for T, n1, n2 in R.TN_SHAPES] + [(n1, n2, T) for T in R.GROUPED_T for n1, n2 in R.GROUPED_DIMS]
QS = 0.125 * 1.4426950408889634


@functools.lru_cache(maxsize=None)
def _case(M, N, K, kind):
    d = (R.random_case if kind == "random" else R.integer_case)(M, N, K, 1000 + M + N + K)
    acc, S = R.acc_and_s(d["A"], d["B"])
    return d, acc, S


def _forms(N, a4):
    """(label, epilogue, reference kwargs, emulation kwargs) of the output forms of section 3; a4 = the alpha of epilogue 4."""
    forms = [("plain", R.EPI_BF16, {}, dict(with_bias=False, with_res=False)),
             ("bias+res", R.EPI_BF16, dict(bias=True, res=True), {}),
             ("dgelu", R.EPI_DGELU, dict(aux_in=True), {}),
             ("f32", R.EPI_F32, dict(alpha=0.5, beta=2.0, C0=True), dict(alpha=0.5, beta=2.0))]
    if N % 12 == 0:
        forms.append(("qkv", R.EPI_QKV, dict(bias=True, alpha=a4), dict(alpha=a4)))
    return forms


def _ref(d, acc, S, K, epi, kw):
    kw = dict(kw)
    for name, key in (("bias", "bias"), ("res", "res"), ("aux_in", "aux"), ("C0", "C0")):
        if kw.get(name) is True:
            kw[name] = d[key]
    return R.reference(epi, acc, S, K, **kw)


@pytest.mark.parametrize("M,N,K", sorted(set(ALL_NT + ALL_TN)))
def test_bound_is_safe_for_a_correct_result(M, N, K):
    """fp32 accumulation in ANY order stays inside the bound: the CPU's fp32 matmul (its own blocking and order) with the epilogue in
    fp32 and one rounding, for every output form; the worst err / tol is printed."""
    d, acc, S = _case(M, N, K, "random")
    for label, epi, rkw, ekw in _forms(N, QS):
        ref, tol = _ref(d, acc, S, K, epi, rkw)
        worst = R.assert_elementwise(R.emulate_fp32(epi, d, **ekw), ref, tol, f"{label} {(M, N, K)}")
        print(f"fp32 emulation {(M, N, K)} {label}: worst err/tol {worst:.3f}")
        assert worst <= 1.0


@pytest.mark.parametrize("M,N,K", [(129, 132, 96), (257, 264, 256), (65, 136, 4096)])
def test_integer_reference_is_exact(M, N, K):
    """Integer operands: the float64 reference equals a float64 -> fp32 -> bf16 computation bit for bit (every partial sum < 2^24 is an
    fp32 number), fp32 accumulation reproduces it exactly, and the draws do reach bf16 ties (odd sums above 256) where K allows."""
    d, acc, S = _case(M, N, K, "integer")
    assert float(S.max()) + 16 < 2 ** 24
    for label, epi, rkw, ekw in _forms(N, 0.25):
        ref, _ = _ref(d, acc, S, K, epi, rkw)
        assert torch.equal(ref.float().double(), ref), label              # exact in fp32
        dtype = torch.float32 if epi == R.EPI_F32 else torch.bfloat16
        expect = R.exact_output(ref, dtype)
        assert torch.equal(expect, ref.to(dtype)), label                 # float64 -> bf16 directly: the same bits
        assert torch.equal(R.emulate_fp32(epi, d, **ekw), expect), label   # fp32 accumulation is exact, whatever its order
    if K >= 256:
        ref, _ = _ref(d, acc, S, K, R.EPI_BF16, dict(bias=True, res=True))
        ties = (ref.abs() > 256) & (ref.abs() < 512) & (ref % 2 != 0)
        assert int(ties.sum()) > 100, int(ties.sum())
        assert not torch.equal(R.exact_output(ref, torch.bfloat16).double(), ref)   # the rounding is not the identity


# ------------------------------------------------------------------------------------------------ planted errors
PLANT = (257, 264, 256)


def _plant_case():
    d, acc, S = _case(*PLANT, "random")
    ref, tol = R.reference(R.EPI_BF16, acc, S, PLANT[2], bias=d["bias"], res=d["res"])
    return d, ref, tol


def _rejected(out, ref, tol):
    rep = R.elementwise_report(out, ref, tol)
    with pytest.raises(AssertionError):
        R.assert_elementwise(out, ref, tol, "planted")
    assert not rep["ok"] and rep["count"] > 0
    return rep


def test_checker_accepts_the_unplanted_case():
    d, ref, tol = _plant_case()
    assert R.assert_elementwise(R.emulate_fp32(R.EPI_BF16, d), ref, tol) <= 1.0


@pytest.mark.parametrize("M,N,K", [(129, 132, 32), (257, 260, 64), (300, 520, 320), (64, 8, 4096)])
def test_checker_rejects_one_dropped_k_term(M, N, K):
    """One k-term out of K missing from every dot product: rejected at every K (the share of elements that leave the bound is printed:
    most of them at short K, where the missing term dwarfs the fp32 part of the bound; a tenth at K = 4096)."""
    d, acc, S = _case(M, N, K, "random")
    ref, tol = R.reference(R.EPI_BF16, acc, S, K, bias=d["bias"], res=d["res"])
    A = d["A"].clone()
    A[:, K // 2] = 0
    rep = _rejected(R.emulate_fp32(R.EPI_BF16, d, acc32=A.float() @ d["B"].float().t()), ref, tol)
    print(f"dropped k-term {(M, N, K)}: {rep['count'] / ref.numel():.1%} outside, worst {rep['worst']:.3g}")
    assert rep["worst"] > 2.0


def test_checker_rejects_a_k_block_dropped_in_one_subtile():
    """One k-block of 32 missing for a single 16 x 16 sub-tile (one MFMA block of one K step): rejected, and every offender lies inside
    that sub-tile."""
    d, ref, tol = _plant_case()
    acc32 = d["A"].float() @ d["B"].float().t()
    m0, n0 = 240, 256      # the sub-tile at the shifted edge of the 257 x 264 problem
    acc32[m0:m0 + 16, n0:n0 + 16] -= d["A"][m0:m0 + 16, 32:64].float() @ d["B"][n0:n0 + 16, 32:64].float().t()
    rep = _rejected(R.emulate_fp32(R.EPI_BF16, d, acc32=acc32), ref, tol)
    bad = rep["bad_index"]
    assert bool(((bad[:, 0] >= m0) & (bad[:, 0] < m0 + 16) & (bad[:, 1] >= n0) & (bad[:, 1] < n0 + 16)).all())
    assert rep["count"] > 64      # most of the 128 elements (16 rows x 8 existing columns)


def test_checker_rejects_a_bias_shifted_by_one_column_group():
    d, ref, tol = _plant_case()
    wrong = dict(d, bias=torch.roll(d["bias"], 4))
    rep = _rejected(R.emulate_fp32(R.EPI_BF16, wrong), ref, tol)
    assert rep["count"] > 0.5 * ref.numel()


def test_checker_rejects_the_last_row_residual_taken_from_the_row_before():
    d, ref, tol = _plant_case()
    res = d["res"].clone()
    res[-1] = res[-2]
    rep = _rejected(R.emulate_fp32(R.EPI_BF16, dict(d, res=res)), ref, tol)
    assert bool((rep["bad_index"][:, 0] == PLANT[0] - 1).all()) and rep["count"] > PLANT[1] // 2


@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf")])
def test_checker_rejects_one_non_finite_element(value):
    d, ref, tol = _plant_case()
    out = R.emulate_fp32(R.EPI_BF16, d)
    out[200, 100] = value
    rep = _rejected(out, ref, tol)
    assert rep["count"] == 1 and rep["bad_index"].tolist() == [[200, 100]] and rep["worst"] == float("inf")
    out32 = R.emulate_fp32(R.EPI_F32, d, alpha=0.5, beta=2.0)
    _, acc, S = _case(*PLANT, "random")
    ref3, tol3 = R.reference(R.EPI_F32, acc, S, PLANT[2], alpha=0.5, beta=2.0, C0=d["C0"])
    R.assert_elementwise(out32, ref3, tol3)
    out32[0, 0] = value
    assert R.elementwise_report(out32, ref3, tol3)["count"] == 1


def test_checker_rejects_the_q_scale_applied_after_rounding():
    """bf16(bf16(acc + bias) * alpha) -- the scale applied to the already rounded q, which is what scaling inside the attention kernels
    gave -- rounds twice.  Stated share: more than 1 % of the q elements leave the bound, none of the other columns does.  Reasoning:
    the two roundings contribute relative errors r1 ~ U(-u / mx, u / mx), r2 ~ U(-u / my, u / my) with mx, my in [1, 2) the significands
    of the unscaled and the scaled value, and the bound allows |r1 + r2| <= u (plus the small fp32 term, K = 32 here).  Where both
    significands are below 1.25 (about log2(1.25)^2 = 10 % of the elements) both ranges are at least 0.8 u wide and the triangular
    density of their sum puts (1.6 - 1)^2 / (4 * 0.64) = 14 % beyond u: 1.4 % from that corner alone."""
    M, N, K = 129, 132, 32
    d, acc, S = _case(M, N, K, "random")
    ref, tol = R.reference(R.EPI_QKV, acc, S, K, bias=d["bias"], alpha=QS)
    R.assert_elementwise(R.emulate_fp32(R.EPI_QKV, d, alpha=QS), ref, tol, "one rounding")
    twice = R.emulate_fp32(R.EPI_BF16, d, with_res=False).float()
    twice[:, : N // 3] *= QS
    rep = _rejected(R.bf(twice), ref, tol)
    bad = rep["bad_index"]
    assert bool((bad[:, 1] < N // 3).all())
    share = rep["count"] / (M * (N // 3))
    print(f"q-scale after rounding: {share:.1%} of the q elements outside the bound")
    assert share > 0.01
