"""Float64 references, derived per-element bounds and strided / poisoned operand layouts for the bf16 MFMA GEMM family
(csrc/gemm*.hip).  Imported by tests/test_gemm_bound_host.py (CPU) and tests/test_gemm_elementwise_gpu.py; never collected.

Everything is computed in float64 from the bf16-ROUNDED inputs: acc = A B^T and S = |A| |B|^T.  With u = 2^-8 (half a bf16 ulp,
relative) and e = 2^-23 (twice the fp32 unit roundoff: the standard gamma_K bound on an fp32 dot product of exact bf16 products,
doubled, which covers any accumulation order, split-K and the MFMA's internal adds):

  epilogue 0 (bf16, bias / residual)   ref = acc + bias + res         tol = u |ref| + (K+2) e (S + |bias| + |res|)
  epilogue 2 (dgelu)                   ref = acc * aux_in             tol = u |ref| + (K+1) e S |aux_in|
  epilogue 4 (q third times alpha)     q:  (acc + bias) * alpha       tol = u |ref| + (K+2) e (S + |bias|) |alpha|   (others: epilogue 0)
  epilogue 3 (fp32; split-K, TN, grouped)  alpha acc + beta C0        tol = (K+3) e (|alpha| S + |beta| |C0|)

The bf16 term is the rounding of the one stored value.  The numbers are derived, not measured; every element has to satisfy
|out - ref| <= tol (NaN / inf fail).  The second reference is exact: integer operands whose every partial sum stays below 2^24, so that
fp32 holds it in any order and the output must equal the rounded float64 result bit for bit."""
import torch

EPI_BF16, EPI_GELU, EPI_DGELU, EPI_F32, EPI_QKV = 0, 1, 2, 3, 4
U_BF16 = 2.0 ** -8
E_F32 = 2.0 ** -23

# section 3 of the issue: the smallest shapes that reach every tile edge, pipeline prologue and kernel route (M, N, K)
NT_SHAPES = [
    (1, 4, 32),            # a single row and a single 4-column group; one K-tile
    (127, 124, 64),        # just under one 128 tile; BK32 ring shorter than its depth under 0x80; one BK64 tile
    (129, 132, 96),        # just over; N % 8 == 4 (straight epilogue); K % 64 != 0 forces the BK32 ring
    (255, 260, 128),       # around the 256 tile; N % 8 == 4
    (257, 264, 256),       # smallest problem the persistent kernel accepts; shifted edge tiles in both directions
    (300, 384, 320),       # half tile (N % 256 == 128); odd K-tile count (ring-half toggle across tiles)
    (513, 520, 256),       # three row tiles, edge in both directions
    (2305, 2312, 256),     # 10 x 10 tiles of 256: flags = 0 picks the persistent kernel by itself
]
QKV_EXTRA_SHAPES = [(257, 276, 256)]   # epilogue 4 only: N % 12 == 0 and the q boundary N / 3 = 92 inside a tile, N % 8 == 4
NT_FLAGS = [0, 0x20, 0x80, 0xC0, 0x100]   # auto | 256x256 | BK32 ring | 8-phase | 4-wave 2 WG/CU
TN_SHAPES = [(1, 8, 8), (63, 8, 264), (65, 136, 72), (129, 256, 256), (4099, 128, 136)]   # (T, N1, N2), T = reduction length
NT_SPLITK_SHAPES = [(96, 288, 64), (128, 136, 4096)]
GROUPED_DIMS = [(8, 264), (136, 72), (256, 256), (128, 136)]   # four problems (N1, N2) of one grouped launch
GROUPED_T = [65, 4099]


def flags_apply(flags, K):
    """False where vj_gemm_bf16_nt routes the flag elsewhere by contract: the 8-phase (0xC0) and 4-wave (0x100) kernels need K % 64 == 0."""
    return K % 64 == 0 or flags not in (0xC0, 0x100)


# ------------------------------------------------------------------------------------------------ operands
def bf(x):
    return x.to(torch.bfloat16)


def random_case(M, N, K, seed, device="cpu"):
    """A ~ N(0,1), B ~ 0.05 N(0,1) as tests/test_gemm_gpu.py; bias fp32, residual / aux_in bf16, C0 fp32 -- drawn on the CPU (the same
    values on every machine), moved to `device`."""
    g = torch.Generator().manual_seed(seed)
    d = dict(A=bf(torch.randn(M, K, generator=g)), B=bf(torch.randn(N, K, generator=g) * 0.05), bias=torch.randn(N, generator=g),
             res=bf(torch.randn(M, N, generator=g)), aux=bf(torch.rand(M, N, generator=g) * 1.26 - 0.13),   # gelu' lives in [-0.13, 1.13]
             C0=torch.randn(M, N, generator=g))
    return {k: v.to(device) for k, v in d.items()}


def integer_case(M, N, K, seed, device="cpu"):
    """A, B in {-2..2}; bias, residual, C0 integers in {-8..8}; aux_in in {-2..2}.  |partial sums| <= 4 K + 16 < 2^24: exact in fp32 in
    any order.  The first half of A's and of B's rows is made non-negative, so that a quarter of the outputs has sums around 1.44 K:
    above 256 bf16 carries even integers only and every odd sum is a tie (round-to-nearest-even is exercised)."""
    assert 4 * K + 16 < 2 ** 24
    g = torch.Generator().manual_seed(seed)

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float()
    A, B = ints(-2, 2, M, K), ints(-2, 2, N, K)
    A[: (M + 1) // 2].abs_()
    B[: (N + 1) // 2].abs_()
    d = dict(A=bf(A), B=bf(B), bias=ints(-8, 8, N), res=bf(ints(-8, 8, M, N)), aux=bf(ints(-2, 2, M, N)), C0=ints(-8, 8, M, N))
    return {k: v.to(device) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ float64 reference + bound
def acc_and_s(A, B):
    """(A B^T, |A| |B|^T) in float64 from the bf16 operands A [M, K], B [N, K]."""
    a, b = A.double(), B.double()
    return a @ b.t(), a.abs() @ b.abs().t()


def reference(epi, acc, S, K, bias=None, res=None, aux_in=None, alpha=1.0, beta=0.0, C0=None):
    """(ref, tol) in float64 for one epilogue, from acc / S of acc_and_s (module docstring)."""
    zero = torch.zeros((), dtype=torch.float64, device=acc.device)
    b = bias.double() if bias is not None else zero
    if epi == EPI_BF16:
        r = res.double() if res is not None else zero
        ref = acc + b + r
        return ref, U_BF16 * ref.abs() + (K + 2) * E_F32 * (S + b.abs() + r.abs())
    if epi == EPI_DGELU:
        x = aux_in.double()
        ref = acc * x
        return ref, U_BF16 * ref.abs() + (K + 1) * E_F32 * S * x.abs()
    if epi == EPI_QKV:
        N = acc.shape[1]
        sc = torch.ones(N, dtype=torch.float64, device=acc.device)
        sc[: N // 3] = alpha
        ref = (acc + b) * sc
        return ref, U_BF16 * ref.abs() + (K + 2) * E_F32 * (S + b.abs()) * sc.abs()
    if epi == EPI_F32:
        c0 = C0.double() if (C0 is not None and beta != 0.0) else zero
        ref = alpha * acc + beta * c0
        return ref, (K + 3) * E_F32 * (abs(alpha) * S + abs(beta) * c0.abs())
    raise ValueError(f"no element-wise bound for epilogue {epi}")


def emulate_fp32(epi, d, alpha=1.0, beta=0.0, with_bias=True, with_res=True, acc32=None):
    """The plain fp32-accumulate emulation of an epilogue (bf16 inputs -> fp32 matmul -> fp32 epilogue -> one rounding): what a correct
    kernel computes up to the accumulation order.  `acc32` replaces the product (planted errors)."""
    acc = d["A"].float() @ d["B"].float().t() if acc32 is None else acc32
    if epi == EPI_BF16:
        y = acc
        if with_bias:
            y = y + d["bias"]
        if with_res:
            y = y + d["res"].float()
        return bf(y)
    if epi == EPI_DGELU:
        return bf(acc * d["aux"].float())
    if epi == EPI_QKV:
        y = acc + d["bias"]
        y[:, : y.shape[1] // 3] *= alpha
        return bf(y)
    if epi == EPI_F32:
        return alpha * acc + beta * d["C0"]
    raise ValueError(epi)


def exact_output(ref64, dtype):
    """The bit pattern an exact (integer) case must produce: float64 -> fp32 (exact: |ref| < 2^24 or a power-of-two multiple of such an
    integer) -> one bf16 rounding."""
    return ref64.float().to(dtype)


# ------------------------------------------------------------------------------------------------ the checker
def elementwise_report(out, ref, tol, n_show=6):
    """Every element against its own bound.  Returns dict(ok, count, worst, offenders): ok is False as soon as ONE element has
    |out - ref| > tol or is NaN / inf (the comparison is `<=`, which NaN fails); worst = max err / tol; offenders = the first few
    (m, n, m % 256, n % 256, out, ref, tol) so that the position inside the tile shows."""
    assert out.shape == ref.shape == tol.shape, (out.shape, ref.shape, tol.shape)
    err = (out.double() - ref).abs()
    good = err <= tol
    ok = bool(good.all())
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    bad = (~good).nonzero()
    offenders = []
    for m, n in bad[:n_show].tolist():
        offenders.append((m, n, m % 256, n % 256, float(out[m, n]), float(ref[m, n]), float(tol[m, n])))
    return dict(ok=ok, count=int(bad.shape[0]), worst=worst, offenders=offenders, bad_index=bad)


def assert_elementwise(out, ref, tol, label=""):
    """assert every element inside its bound; returns the worst err / tol (information only)."""
    rep = elementwise_report(out, ref, tol)
    assert rep["ok"], (f"{label}: {rep['count']} of {out.numel()} elements outside the derived bound, worst err/tol {rep['worst']:.3g}; "
                       f"first (m, n, m%256, n%256, out, ref, tol): {rep['offenders']}")
    return rep["worst"]


def assert_bit_equal(out, expect, label=""):
    """torch.equal with a useful message: count and first offenders with their tile positions."""
    assert out.shape == expect.shape and out.dtype == expect.dtype, (label, out.shape, expect.shape, out.dtype, expect.dtype)
    if torch.equal(out, expect):
        return
    o2, e2 = out.reshape(out.shape[0], -1), expect.reshape(expect.shape[0], -1)
    bad = ((o2 != e2) | torch.isnan(o2.float())).nonzero()
    first = [(m, n, m % 256, n % 256, float(o2[m, n]), float(e2[m, n])) for m, n in bad[:6].tolist()]
    raise AssertionError(f"{label}: {int(bad.shape[0])} of {out.numel()} elements differ; first (m, n, m%256, n%256, out, expected): {first}")


# ------------------------------------------------------------------------------------------------ strided, poisoned layouts
PATTERN_BYTE = 0xA5
BAND_ELEMS = 4096          # elements before and after every embedded matrix (a multiple of 64: keeps the 128-byte alignment of the base)
_INT_OF = {torch.bfloat16: torch.int16, torch.float32: torch.int32}


class Embedded:
    """A [rows, cols] matrix as a view (row stride ld, base `offset` elements past an aligned address) into a larger allocation whose every
    other element -- the padding columns between the rows, a band before and a band after -- holds a fill: NaN for inputs (a read of
    anything outside [rows, cols] poisons the result) or the byte pattern 0xA5 for outputs (compared afterwards as raw integers)."""

    def __init__(self, rows, cols, ld, offset, dtype, device, nan_fill, value=None):
        assert ld >= cols
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, dtype
        self.start = BAND_ELEMS + offset
        n = self.start + rows * ld + BAND_ELEMS
        it = _INT_OF[dtype]
        self.raw = torch.empty(n, dtype=it, device=device)
        self.raw.view(torch.uint8).fill_(PATTERN_BYTE)
        if nan_fill:
            self.raw.view(dtype).fill_(float("nan"))
        self.view = torch.as_strided(self.raw.view(dtype), (rows, cols), (ld, 1), self.start)
        self._iview = torch.as_strided(self.raw, (rows, cols), (ld, 1), self.start)
        if value is not None:
            self.view.copy_(value)
        self._before = self.raw.clone()
        assert self.view.data_ptr() % 8 == 0

    def surroundings_intact(self):
        """True when nothing outside the [rows, cols] view changed since construction (raw integer comparison)."""
        now = self.raw.clone()
        torch.as_strided(now, (self.rows, self.cols), (self.ld, 1), self.start).copy_(
            torch.as_strided(self._before, (self.rows, self.cols), (self.ld, 1), self.start))
        return torch.equal(now, self._before)


def embed_input(t, ld, offset=8):
    """t as a strided view surrounded by NaN (inputs: base shifted by `offset` elements, 8 = 16 bytes)."""
    return Embedded(t.shape[0], t.shape[1], ld, offset, t.dtype, t.device, True, t)


def embed_output(rows, cols, ld, offset, dtype, device, value=None):
    """an output view surrounded by the byte pattern; `value` pre-loads it (in-place residual, beta * C0)."""
    return Embedded(rows, cols, ld, offset, dtype, device, False, value)
