"""CPU references, data and the shared case lists of the data-movement kernels (csrc/rows.hip, csrc/reduce.hip, the two pack kernels of
csrc/input_pack.hip): tests/test_rows_elementwise_gpu.py runs the kernels against them, tests/test_rows_ref_host.py holds them to
independent spellings and to planted defects on the CPU.  Plain torch only; nothing here knows how a kernel walks its rows.

Movers (gather, scatter, copy, transpose) are compared bit for bit under an integer view on arbitrary bit patterns -- NaN payloads, both
zeros, both infinities and subnormals among them.  Position adds are (x.float() + pos).to(bfloat16), one rounding.  Column sums and partial
reductions get two kinds of data:
  * integers (|x| <= 128, integer-valued old output, alpha 1 or 0.5): while sum|x| < 2^24 every fp32 partial sum of every order is an
    integer below 2^24, hence exact, and alpha * sum + old is a multiple of 0.5 below 2^23, exact too.  The result must EQUAL the float64
    sum whatever row chunking the launcher picks, so a dropped, doubled or mis-windowed row shows without copying the launcher's heuristic;
  * normal draws against float64 within gamma * (|alpha| * sum|x| + |beta * old|), gamma = (n+2)u / (1 - (n+2)u), u = 2^-24, n the number
    of rows summed: the textbook bound of a sum of n terms in ANY order (n - 1 roundings on the path of a term) plus the roundings of the
    product with alpha, of beta * old and of the last add.  Adding the exact zeros of idle lanes and empty chunks rounds nothing."""
import collections

import torch

BF16, F32 = torch.bfloat16, torch.float32
INT_VIEW = {BF16: torch.int16, F32: torch.int32}
U = 2.0 ** -24
ROW_CAP = 4096 * 4             # rows_grid: at most 4096 workgroups of 4 waves, one row per wave and pass
FLAT_CAP = 256 * 32 * 256      # flat_grid(total, 256 * 32): at most 8192 workgroups of 256 threads, one chunk per thread and pass
BIG_B, BIG_K = 3, 5463         # 16 389 rows: 5 rows into the second pass, in three samples
WIDTHS = [8, 512, 520, 1032]   # bf16 row widths of the position adds: one chunk; exactly one trip of the 512-element lane loop; a
                               # ragged second trip of one chunk; a ragged third trip
MOVE_BYTES = [8, 12, 264, 16, 1024, 1040]      # 4-byte form with 2, 3 and 66 (a second lane trip) words; 16-byte form with 1, 64, 65 chunks


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ one allocation, guarded
class Embedded:
    """A tensor of `shape` inside ONE flat allocation, `guard` (+ `shift`) elements of `fill` before it and `guard` after it.  An input
    that feeds arithmetic takes fill = NaN (a read outside the operand reaches the result); an output takes a sentinel, and
    guards_untouched() compares the surroundings bit for bit with what they held when they were made.  shift moves the base by that many
    elements (a base that is 4- but not 16-byte aligned)."""

    def __init__(self, shape, dtype, device, fill, guard=64, shift=0, inner=None):
        n = 1
        for s in shape:
            n *= s
        self.lo, self.hi = guard + shift, guard + shift + n
        self.flat = torch.full((self.hi + guard,), fill, dtype=dtype, device=device)
        self.view = self.flat[self.lo:self.hi].view(shape)
        if inner is not None:
            self.view.fill_(inner)
        self.before = self.flat.clone()

    def put(self, t):
        """the content, copied in bit for bit (t of the view's dtype, or of its integer view)"""
        if t.dtype == self.view.dtype:
            self.view.copy_(t)
        else:
            self.bits().copy_(t)
        return self

    def bits(self):
        iv = INT_VIEW.get(self.view.dtype)
        return self.view if iv is None else self.view.view(iv)

    def guards_untouched(self):
        iv = INT_VIEW.get(self.flat.dtype)
        now, was = (self.flat, self.before) if iv is None else (self.flat.view(iv), self.before.view(iv))
        return torch.equal(now[:self.lo], was[:self.lo]) and torch.equal(now[self.hi:], was[self.hi:])


# ------------------------------------------------------------------------------------------------ movers
# sign | exponent | mantissa patterns a mover must not touch: +0, -0, +inf, -inf, the default quiet NaN, a signalling NaN with a payload,
# a negative quiet NaN with a payload, the smallest subnormal, the largest negative subnormal
SPECIAL_BITS = {BF16: [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x7F81, 0xFFC5, 0x0001, 0x807F],
                F32: [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC12345, 0x00000001, 0x807FFFFF]}


def _signed(v, bits):
    return v - (1 << bits) if v >= (1 << (bits - 1)) else v


def payload(shape, dtype, seed):
    """Integer view (int16 for bf16, int32 for fp32) of `shape` elements of arbitrary bits: uniform over all patterns, so every exponent
    and about one NaN in 256 (bf16) occurs, with SPECIAL_BITS planted at the front and, reversed, at the back of the flat order (as far
    as they fit).  No two rows of a few elements are equal by chance, so a row taken from the wrong place shows."""
    g = torch.Generator().manual_seed(seed)
    iv = INT_VIEW[dtype]
    nb = 16 if dtype == BF16 else 32
    t = torch.randint(-(1 << (nb - 1)), 1 << (nb - 1), tuple(shape), generator=g, dtype=torch.int64).to(iv)
    flat = t.view(-1)
    sp = torch.tensor([_signed(v, nb) for v in SPECIAL_BITS[dtype]], dtype=iv)
    k = min(len(sp), flat.numel() // 2)
    if k:
        flat[:k] = sp[:k]
        flat[flat.numel() - k:] = sp[:k].flip(0)
    return t


def gather_ref(src, idx):
    """out[b, k] = src[b, idx[b, k]] (src [B, N, D]) or table[idx[b, k]] (src [N, D] / [1, N, D] with B > 1)."""
    B = idx.shape[0]
    if src.dim() == 2 or (src.shape[0] == 1 and B > 1):
        return src.reshape(-1, src.shape[-1])[idx]
    return torch.stack([src[b][idx[b]] for b in range(B)]) if B else src[:, :0]


def scatter_ref(src, idx, N):
    """zeros [B, N, D] with out[b, idx[b, k]] = src[b, k]; idx unique per b."""
    B, K = idx.shape
    out = torch.zeros((B, N, src.shape[-1]), dtype=src.dtype)
    for b in range(B):
        out[b][idx[b]] = src[b]
    return out


def unique_idx(B, N, K, seed):
    """[B, K] distinct per sample, unsorted."""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(N, generator=g)[:K] for _ in range(B)]) if B else torch.zeros((0, K), dtype=torch.int64)


def any_idx(B, N, K, seed):
    """[B, K] in [0, N), unsorted, with repeats as soon as K is not small against N; 0 and N - 1 occur when K >= 2."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, N, (B, K), generator=g)
    if K >= 2:
        idx[:, 0], idx[:, -1] = N - 1, 0
    return idx


# ------------------------------------------------------------------------------------------------ position adds
def rows_bf16(shape, seed):
    """bf16 normal draws times a power of two per element (2^-6 .. 2^6): sums with the fp32 table round at every bit position."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * torch.exp2(torch.randint(-6, 7, shape, generator=g).float())).to(BF16)


def table_f32(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * torch.exp2(torch.randint(-6, 7, shape, generator=g).float())


def add_ref(x, pos_rows):
    """THE position add: fp32, one rounding."""
    return (x.float() + pos_rows).to(BF16)


def add_pos_ref(x, pos, B, K, idx=None):
    """x [B*K, D] + pos[idx[b, k]] (idx None: pos[k])."""
    rows = pos[idx.reshape(-1)] if idx is not None else pos[:K].repeat(B, 1)
    return add_ref(x, rows)


def add_pos_bcast_ref(y, pos, B, S, Gt):
    """out[b, t*S + s] = y[b, s] + pos[t*S + s]: [B*Gt*S, D]."""
    D = y.shape[-1]
    return add_ref(y.view(B, 1, S, D).expand(B, Gt, S, D), pos.view(1, Gt, S, D)).reshape(B * Gt * S, D)


def add_pos_frames_ref(x, pos, idx, N):
    """x [B, F*N, D] + pos[idx[b, f]] on the N rows of frame f."""
    B, F = idx.shape
    D = x.shape[-1]
    return add_ref(x.view(B, F, N, D), pos[idx].view(B, F, 1, D)).view(B, F * N, D)


def pred_assemble_ref(e, tok, pos, idx_e, idx_p):
    """[B, Ke + Kp, D]: e[b, j] + pos[idx_e[b, j]], then tok + pos[idx_p[b, j]]."""
    B, Ke = idx_e.shape
    D = pos.shape[-1]
    ctx = e.float().view(B, Ke, D) + pos[idx_e]
    tgt = tok.view(1, 1, D) + pos[idx_p]
    return torch.cat([ctx, tgt], 1).to(BF16)


# ------------------------------------------------------------------------------------------------ packers
def unfold_rows(clips, tub, p):
    """[B, C, T, H, W] -> [B, N, C*tub*p*p]: token (t', h', w') row-major, element (c, dt, dh, dw) -- Conv3d's im2col."""
    B, C, T, H, W = clips.shape
    u = clips.reshape(B, C, T // tub, tub, H // p, p, W // p, p).permute(0, 2, 4, 6, 1, 3, 5, 7)
    return u.reshape(B, (T // tub) * (H // p) * (W // p), C * tub * p * p)


def tubelet_ref(clips, tub, p, idx=None):
    u = unfold_rows(clips.to(BF16), tub, p)      # the rounding is per element: it commutes with the permutation
    return u if idx is None else gather_ref(u, idx)


def image_ref(images, tub, p, idx=None):
    """the rows of the clip that repeats each image `tub` times along time (one tubelet deep): one per spatial cell, or per idx entry
    taken modulo the number of cells."""
    u = unfold_rows(images.to(BF16).unsqueeze(2).repeat(1, 1, tub, 1, 1), tub, p)
    return u if idx is None else gather_ref(u, idx % u.shape[1])


PACK_COMBOS = [(p, tub, C) for p in (8, 16) for tub in (1, 2) for C in (1, 3)]
PACK_SMALL = dict(B=2, T=4, H=32, W=48)        # H != W; 4 x 6 cells at patch 8, 2 x 3 at patch 16
PACK_BIG = dict(B=2, C=3, T=2, H=1184, W=1184, tub=2, p=16)


def pack_chunks(B, K, C, tub, p):
    """16-byte output chunks of tubelet_pack (one per thread and pass)."""
    return B * K * (C * tub * p * p // 8)


# ------------------------------------------------------------------------------------------------ sums
def gamma(n):
    k = (n + 2) * U
    return k / (1.0 - k)


def int_data(shape, seed, dtype=BF16, lim=128):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-lim, lim + 1, shape, generator=g).to(dtype)


def normal_data(shape, seed, dtype=BF16):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype)


def int_old(N, seed):
    return int_data((N,), seed, F32, lim=1000)


def normal_old(N, seed):
    return normal_data((N,), seed, F32) * 3.0


def window_rows(M, group, lo, hi):
    """bool [M]: the rows m with lo <= m % group < hi."""
    j = torch.arange(M) % group
    return (j >= lo) & (j < hi)


def sum_ref(x, alpha, old=None, rows=None):
    """(ref, tol, abs_sum), float64 [N]: alpha * the column sums of x (over the rows of the bool mask) + old, its bound, sum|x|."""
    xd = x.double() if rows is None else x.double()[rows]
    s, a = xd.sum(0), xd.abs().sum(0)
    o = torch.zeros_like(s) if old is None else old.double()
    return alpha * s + o, gamma(xd.shape[0]) * (abs(alpha) * a + o.abs()), a


def exact_in_fp32(abs_sum, alpha, old=None):
    """the precondition of the integer data: every partial sum an integer below 2^24, the result a multiple of 0.5 below 2^23."""
    top = float(abs_sum.max()) if abs_sum.numel() else 0.0
    o = 0.0 if old is None or not old.numel() else float(old.abs().max())
    return top < 2.0 ** 24 and alpha in (1.0, 0.5) and abs(alpha) * top + o < 2.0 ** 23


ColsumCase = collections.namedtuple("ColsumCase", "M N group lo hi rows")


def _cs(M, N, group=0, lo=0, hi=None, rows=None):
    return ColsumCase(M, N, group, lo, hi, M if rows is None else rows)


COLSUM_CASES = [_cs(M, 8) for M in (1, 8, 9, 512, 513, 8192, 16384, 16448)] + [
    _cs(513, 264), _cs(513, 2056), _cs(8192, 2056),
    _cs(9 * 130, 8, 130, 37, 130),       # row_hi = group; 130 divides no row chunk, the windows straddle the chunk boundaries
    _cs(9 * 130, 8, 130, 0, 41),         # row_lo = 0: row 41 of every group lies just outside
    _cs(9 * 130, 8, 130, 50, 50),        # an empty window
    _cs(513, 264, 27, 5, 26),
    _cs(513, 8, rows=600),               # the M= prefix form: 87 more rows follow in the tensor
]
COLSUM_RUNS = [(1.0, False), (0.5, True)]       # (alpha, accumulate)


def colsum_id(c):
    s = f"M{c.M}-N{c.N}"
    if c.group:
        s += f"-g{c.group}[{c.lo},{c.hi})"
    return s + (f"-of{c.rows}" if c.rows != c.M else "")


def colsum_rows(c):
    return None if not c.group else window_rows(c.M, c.group, c.lo, c.hi)


TRANSPOSE_SHAPES = [(63, 8), (64, 64), (65, 72), (128, 136)]
TCOLSUM_M, TCOLSUM_N = [64, 65, 513], 72
REDUCE_P, REDUCE_N = [0, 1, 7, 8, 9, 17], [8, 63, 64, 65]
# (P, N, stride) of a 16-segment launch: an N = 0 and a P = 0 segment among ragged ones; stride > N: a column slice of a wider matrix
SEGMENTS = [(7, 8, 8), (0, 64, 64), (9, 63, 80), (17, 65, 65), (5, 0, 8), (8, 64, 192), (1, 8, 8), (17, 64, 64), (9, 65, 72), (7, 63, 63),
            (8, 8, 16), (1, 65, 65), (17, 8, 8), (9, 64, 64), (8, 63, 64), (7, 65, 130)]


def pad64(m):
    return (m + 63) // 64 * 64


def transpose_ref(x, M):
    """x [>= M, N] -> [N, pad64(M)]: the first M rows transposed, the pad columns zero (any dtype, integer views included)."""
    out = torch.zeros((x.shape[1], pad64(M)), dtype=x.dtype)
    out[:, :M] = x[:M].t()
    return out
