"""GPU: vj_slice_sum (ops.slice_sum), the adjoint of vj_add_pos_bcast: dy[b,s] = bf16(sum_t dx[b, t*S+s]) with the fp32 sum
taken from slice 0 in ascending t by plain adds and rounded once.  The order is part of the contract, so the check is equality
with the same sum on the CPU -- on data whose fp32 sums are inexact (normal draws times 2^randint(-12, 12) per element), where
another order gives other bits (asserted below for every case with more than two slices)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(2, 16, 4, 64), (1, 15, 3, 1280), (2, 7, 1, 72), (3, 196, 8, 1024)]
# bf16 summands carry 8 significant bits, so an fp32 sum is inexact only where exponents lie more than 16 apart: with these seeds the
# descending sum differs from the ascending one in 1 of 19200 and 11 of 602112 elements of these two cases (counted on the CPU) and
# in none of the 2048 of the smallest
ORDER_SHOWS = [(1, 15, 3, 1280), (3, 196, 8, 1024)]


def _input(B, S, Gt, D):
    """bf16 [B, Gt, S, D] on the CPU: normal draws scaled by a power of two per element."""
    g = torch.Generator().manual_seed(1000 * B + 10 * S + Gt)
    x = torch.randn(B, Gt, S, D, generator=g) * torch.exp2(torch.randint(-12, 13, (B, Gt, S, D), generator=g).float())
    return x.to(torch.bfloat16)


def _ref(x, order=None):
    """The contract on the CPU: fp32, slice by slice in `order` (default ascending), one rounding."""
    order = list(range(x.shape[1])) if order is None else order
    acc = x[:, order[0]].float()
    for t in order[1:]:
        acc = acc + x[:, t].float()
    return acc.to(torch.bfloat16)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def case(request):
    B, S, Gt, D = request.param
    x = _input(B, S, Gt, D)
    return (B, S, Gt, D), x, _ref(x)


def test_slice_sum_equals_the_ascending_fp32_sum(case):
    from jepa_amd.hip import ops
    (B, S, Gt, D), x, ref = case
    out = ops.slice_sum(x.to(DEV).view(B * Gt * S, D), B, S, Gt)
    assert out.shape == (B * S, D) and out.dtype == torch.bfloat16
    assert torch.equal(out.cpu().view(B, S, D), ref)
    if (B, S, Gt, D) in ORDER_SHOWS:      # the reference is not order-blind on this data: the descending sum differs somewhere
        assert not torch.equal(_ref(x, list(range(Gt - 1, -1, -1))), ref)
    if Gt == 1:     # one slice: the input's bits
        assert torch.equal(out.cpu().view(torch.int16), x.view(B * S, D).view(torch.int16))


def test_one_slice_moves_nan_and_signed_zero_bits():
    from jepa_amd.hip import ops
    x = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), 1.5, -2.0 ** -130, 3.0e38, float("nan")] * 9).to(torch.bfloat16).view(1, 72)
    out = ops.slice_sum(x.to(DEV), 1, 1, 1)
    assert torch.equal(out.cpu().view(torch.int16), x.view(torch.int16))


def test_slice_sum_is_the_adjoint_of_add_pos_bcast(case):
    """With pos = 0 the broadcast fans y out unchanged, and the sum over the Gt copies is y added to itself Gt - 1 times."""
    from jepa_amd.hip import ops
    (B, S, Gt, D), x, _ = case
    y = x[:, 0].contiguous()
    fanned = ops.add_pos_bcast(y.to(DEV).view(B * S, D), torch.zeros(Gt * S, D, device=DEV), B, S, Gt)
    back = ops.slice_sum(fanned, B, S, Gt)
    assert torch.equal(back.cpu().view(B, S, D), _ref(y.unsqueeze(1).expand(B, Gt, S, D)))


def test_out_argument_and_guard_rows(case):
    """The operand sits between NaN guard rows in one allocation: nothing outside it is read (a NaN would reach the sum), and
    the result lands in the tensor given as out= without touching its neighbours."""
    from jepa_amd.hip import ops
    (B, S, Gt, D), x, ref = case
    rows, guard = B * Gt * S, 4
    buf = torch.full((rows + 2 * guard, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    buf[guard:guard + rows] = x.to(DEV).view(rows, D)
    obuf = torch.full((B * S + 2 * guard, D), -7.0, dtype=torch.bfloat16, device=DEV)
    out = obuf[guard:guard + B * S]
    got = ops.slice_sum(buf[guard:guard + rows], B, S, Gt, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert bool(torch.isfinite(out.float()).all()) and torch.equal(out.cpu().view(B, S, D), ref)
    assert bool((obuf[:guard] == -7.0).all()) and bool((obuf[guard + B * S:] == -7.0).all())


def test_shape_mismatch_raises():
    from jepa_amd.hip import ops
    dx = torch.zeros(2 * 4 * 16, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="do not match"):
        ops.slice_sum(dx, 2, 16, 3)
    with pytest.raises(ValueError, match="do not match"):
        ops.slice_sum(dx, 2, 16, 4, out=torch.zeros(2 * 15, 64, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(TypeError):
        ops.slice_sum(dx.float(), 2, 16, 4)
