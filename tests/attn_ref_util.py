"""Float64 references, derived per-element bounds, exact cases and poisoned layouts for the attention kernels (csrc/attention.hip:
forward, dQ, dK/dV).  Imported by tests/test_attn_bound_host.py (CPU) and tests/test_attention_elementwise_gpu.py; never collected.

Everything is computed in float64 from the bf16-ROUNDED inputs, per (sample, head) slice [B, H, S, hd].  u = 2^-8 (half a bf16 ulp,
relative), e = 2^-23 (twice the fp32 unit roundoff, as tests/gemm_ref_util.py), N = S keys, hd = the real head dimension.

FORWARD.  c = scale * log2(e) (c = 1 for the pre-scaled form, scale < 0: the stored q already carries it).
  s2 = c q k^T, T = |c| |q| |k|^T.
  eps[q,k] = (u_fold + (hd+1) e) T + e |s2| + 3 e (max_k |s2[q,:]| + 5)     error of a score relative to its base, log2 units
     u_fold T      the kernel folds c into the stationary operand, bf16(c x): one more bf16 rounding of every factor of the product;
                   0 when scale < 0 or when the fold is exact (the fp32 factor acts as a power of two on every stored value)
     (hd+1) e T    fp32 accumulation of hd exact bf16 products (any order, the MFMA's internal adds included)
     e |s2|        the fp32 factor c itself (host product scale * log2 e) and its product with q before the bf16 rounding
     3 e (M + 5)   NOT in the issue's list, derived here: the score accumulator starts at -base (the seed of the first MFMA), and
                   |base| <= max_k |s2| + 5 (the base is some earlier maximum plus the 2^5 headroom and is never lowered).  Every one
                   of the KS <= 4 MFMA roundings of a score, and the two roundings of a re-base (base += shift, acc -= shift), acts
                   on a value of magnitude <= |base| + T: (4 + 2) roundings of e / 2 each on |base|; the T part is inside (hd+1) e T.
  eta[q,k] = 2^eps (1 + u) (1 + (N+2) e) - 1      relative error of one probability: exp2 of a perturbed score, the bf16 rounding of P
                   (numerator and denominator use the SAME rounded P: the pad column / all-ones MFMA row sums), and the fp32 sums,
                   v_exp_f32 (1 ulp) and the reciprocal (1 ulp) in (N+2) e.
  o' - o = sum_k p_k eta_k (v_k - o) / (1 + sum_k p_k eta_k), hence
  tol_o[q,d]  = u |ref| + sum_k p eta |v[k,d] - ref[q,d]| / (1 - sum_k p eta) + (N+hd+3) e (p |v|)[q,d] + N 2^-120 max|v|
  tol_lse[q]  = max_k eps[q,k] + log2(1 + u + (N+2) e) + 2 e (|lse| + 8)
     N 2^-120 max|v|: flush of denormal probabilities (NOT in the issue's list, derived): v_exp_f32 and the bf16 conversion may flush
                   results below 2^-126 to zero, an ABSOLUTE error of 2^-126 on a probability measured against the base, whose row sum
                   is >= 2^-5 (1 - u) (the largest score of the tile that set the base sits exactly 5 below it): 2^-120 after
                   normalisation, times |v|, for each of the N keys.
     2 e (|lse| + 8): log2f of a row sum in [2^-5, 2 N] (|log2| <= 8 + ...) and the final add base + log2(l).

BACKWARD.  A function of the backward's OWN inputs (qkv, o_in, dO, lse2_in): nothing of the forward enters.
  P = 2^(s2 - lse2_in), delta = rowsum(dO o_in), dP = dO V^T, dS = P (dP - delta)
  dQ = |scale| dS K,  dK = |scale| dS^T Q  (q stored pre-scaled: dS^T Q' / log2 e),  dV = P^T dO
  eps' = eps-without-the-base-term + e |lse2_in|     (the accumulator starts at -lse2_in)
  eta' = 2^eps' (1 + 2 e) - 1                        (v_exp_f32 and no bf16 rounding yet)
  err(dS) = P [eta' |dP - delta| + (1 + eta') ((hd+1) e (|dO| |V|^T + sum_d |dO| |o_in|) + e |dP - delta|)]
  err_b   = err + u (|dS| + err)                     (dS is rounded to bf16 for the second product)
  tol_dQ  = u |ref| + |scale| (err_b |K|) + (N+3) e |scale| (|dS| |K|) + flush;   tol_dK: the transposed analogue with |Q|
  tol_dV  = u |ref| + (P (eta' + u (1 + eta')))^T |dO| + (N+2) e P^T |dO| + flush
     flush (NOT in the issue's list, derived): P and P (dP - delta) below 2^-126 may be flushed to zero: an absolute 2^-126 on each of
                   the N addends of an output element, times the other factor: N 2^-125 (1 + max|dP - delta|) max|K| (|Q|, |dO|).

OUTPUT ROUNDING.  In every tol above `u |ref| + R` is evaluated as u |ref| + (1 + u) R: the one bf16 rounding of a stored output is relative
to the computed fp32 value, which lies within R of ref (second order, kept so that the bound is rigorous).  The column partials subtract
u |ref| and keep the rest.

COLUMN PARTIALS.  Row b * nb + j of colq is the sum over the 128-query block j of sample b of the fp32 dQ (before its rounding); colkv
the same per block of 64 * KT keys (KT = 2 in the 32-wide head-dim class, 1 otherwise), dK | dV side by side.
  ref = block sums of the float64 dQ / dK / dV;  tol = sum_block (tol - u |ref|) + n e sum_block |ref|  (n = rows of the block).

EXACT CASES.  uniform_case: q = 0, so every score is 0, every P the same power of two and the row sum exact: the forward bound with
eps = 0.  onehot_case: k rows are +-g sign codes of pairwise Hamming distance >= dmin, q_i = k_pi(i): the winner's score exceeds every
other by 2 c g^2 dmin >= 32 + rounding, o[i] must equal v[pi(i)] and dV[pi(i)] must equal dO[i] bit for bit (onehot_conditions)."""
import math

import numpy as np
import torch

from tests.gemm_ref_util import E_F32, U_BF16, Embedded, assert_bit_equal  # noqa: F401  (re-exported for the two test modules)

LOG2E = math.log2(math.e)
LOG2E_F32 = np.float32(1.4426950408889634)      # the kernels' constant
HEADROOM = 5.0
FLUSH = 2.0 ** -126

# section 3 of the issue
SEQ_LENS = [1, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257, 321]
HD_MAIN = [24, 32, 64, 80, 128]
HD_ALL = list(range(8, 129, 8))
S_ALL_HD = [65, 193]
MODES = ["fold", "pre", "pow2"]
SHAPES = [(S, hd) for S in SEQ_LENS for hd in HD_MAIN] + [(S, hd) for S in S_ALL_HD for hd in HD_ALL if hd not in HD_MAIN]
ONEHOT_SHAPES = [(S, hd) for S in (65, 193, 257) for hd in HD_MAIN]
SAFETY_SHAPES = [(S, hd) for S in (65, 129) for hd in (24, 80, 128)]


def bf(x):
    return x.to(torch.bfloat16)


def f32(x):
    return float(np.float32(x))


def hd_class(hd):
    return 32 if hd <= 32 else 64 if hd <= 64 else 96 if hd <= 80 else 128


def dkdv_kt(hd):
    """16-key tiles per wave of the dK/dV kernel: its key block is 64 * KT keys (asserted against vj_attn_bwd_colsum_rows on the GPU)."""
    return 2 if hd_class(hd) == 32 else 1


def has_pad_chunk(hd):
    """head-dim chunks >= hd exist in the LDS image (they re-read chunk 0)."""
    return hd < hd_class(hd)


def host_sc(scale):
    """the fp32 factor the host entry points hand to the kernels: scale * LOG2E in fp32 (1 for the pre-scaled form)."""
    return 1.0 if scale < 0 else float(np.float32(scale) * LOG2E_F32)


# ------------------------------------------------------------------------------------------------ layouts
def split_heads(x, B, S, H, hd):
    """[B*S, H*hd] -> [B, H, S, hd]"""
    return x.view(B, S, H, hd).permute(0, 2, 1, 3)


def split_qkv(qkv, B, S, H, hd):
    """[B*S, 3*H*hd] -> q, k, v each [B, H, S, hd]"""
    t = qkv.view(B, S, 3, H, hd).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def merge_heads(x):
    """[B, H, S, hd] -> [B*S, H*hd]"""
    B, H, S, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * S, H * hd)


# ------------------------------------------------------------------------------------------------ cases
class Case:
    """One attention problem: bf16 operands and what the reference needs to know about the mode.
    scale   the value handed to the C ABI (exactly representable in fp32)
    c       the float64 factor of the reference scores on the STORED q (1 for the pre-scaled form)
    u_fold  the extra bf16 rounding of the folded operand (0 where there is none)
    sabs    |scale|: the factor of dQ;  kscale: the factor of dK (|scale|, or 1 / log2 e on a pre-scaled q)"""

    def __init__(self, B, S, H, hd, mode, qkv, dout):
        self.B, self.S, self.H, self.hd, self.mode = B, S, H, hd, mode
        self.qkv, self.dout = qkv, dout
        if mode == "pre":
            self.scale = -f32(hd ** -0.5)
            self.c, self.u_fold = 1.0, 0.0
            self.sabs, self.kscale = -self.scale, 1.0 / LOG2E
        elif mode == "fold":
            self.scale = f32(hd ** -0.5)
            self.c, self.u_fold = self.scale * LOG2E, U_BF16
            self.sabs = self.kscale = self.scale
        elif mode == "pow2":
            self.scale = f32(0.125 / LOG2E)
            sc = host_sc(self.scale)
            x = qkv.float()     # the fold reaches q (forward, dQ) and k (dK/dV): both must come out as exact multiples
            exact = torch.equal(bf(x * sc), bf(x * 0.125)) and torch.equal(bf(x * 0.125).float(), x * 0.125)
            self.c, self.u_fold = (0.125, 0.0) if exact else (self.scale * LOG2E, U_BF16)
            self.pow2_exact = exact
            self.sabs = self.kscale = self.scale
        else:
            raise ValueError(mode)
        self.pre = mode == "pre"

    def to(self, device):
        c = Case(self.B, self.S, self.H, self.hd, self.mode, self.qkv.to(device), self.dout.to(device))
        c.c, c.u_fold = self.c, self.u_fold
        c.variant = getattr(self, "variant", "plain")
        return c

    def qkv64(self):
        return [t.double() for t in split_qkv(self.qkv, self.B, self.S, self.H, self.hd)]

    def dout64(self):
        return split_heads(self.dout, self.B, self.S, self.H, self.hd).double()


def random_case(B, S, H, hd, mode, seed=0, qmul=1.0):
    """q, k, v, dO ~ N(0, 1) rounded to bf16, drawn on the CPU (the same values on every machine).  `qmul` multiplies q (sharper or flatter
    soft-max rows); the pre-scaled form stores bf16(q * |scale| log2 e) as the qkv GEMM's epilogue would."""
    g = torch.Generator().manual_seed(1000 * S + hd + seed)
    t = torch.randn(B, S, 3, H, hd, generator=g)
    dout = bf(torch.randn(B * S, H * hd, generator=g))
    t[:, :, 0] *= qmul
    if mode == "pre":
        t[:, :, 0] *= f32(hd ** -0.5) * LOG2E
    return Case(B, S, H, hd, mode, bf(t.reshape(B * S, 3 * H * hd)), dout)


# The inputs every (shape, mode) pair is tested with, on the host AND on the GPU: (name, qmul, sparse_dO).  The plain case, and the sharpened
# ones a planted defect needs where the plain inputs keep it inside the bound (tests/test_attn_bound_host.py proves that every defect is
# rejected by at least one variant of every pair, and prints which):
#   peaked  q x 4: the soft-max rows are dominated by few keys, so one key's probability, or one row's delta, moves an output by more
#           than the u-level terms of its bound (the issue's own sharpening);
#   flat    q / 4, folded scale only.  NOT among the issue's sharpenings (q x 2 ... 4, or the pre-scaled / power-of-two form), and argued
#           here: an lse2 shift of 2^-6 changes every P of its row by 1.1 %, while the folded scale's own term u_fold T allows
#           2^(u T) - 1; at q x 1 ... 4 and hd >= 24, u T exceeds 2^-6 for every key, so under the issue's wording a folded pair cannot
#           show this defect at all (its pre-scaled and power-of-two pairs, u_fold = 0, do).  u T < 2^-6 needs T < 4, i.e. a smaller q.
# sparse_dO (the sharpened variants): dO column 0 of slice (0, 0) keeps only the entry of the row that gives the LAST key its largest
# probability, column 1 only that of the row with the smallest |q| (sparse_rows); column d of dV then holds one query row's
# probabilities alone, P[r, :] dO[r, d], so a relative error of that one row is not averaged away over the S rows of the column sum.
VARIANTS = {"fold": [("plain", 1.0, False), ("peaked", 4.0, True), ("flat", 0.25, True)],
            "pre": [("plain", 1.0, False), ("peaked", 4.0, True)],
            "pow2": [("plain", 1.0, False), ("peaked", 4.0, True)]}


def sparse_rows(case):
    """(row of slice (0, 0) with the largest probability on the last key, row with the smallest sum |q|): functions of qkv alone."""
    q, k, _ = case.qkv64()
    s_last = case.c * (q[0, 0] @ k[0, 0].t())
    p_last = torch.softmax(s_last * math.log(2.0), -1)[:, case.S - 1]
    return int(p_last.argmax()), int(q[0, 0].abs().sum(-1).argmin())


def variant_case(B, S, H, hd, mode, variant, seed=0):
    """the case of one entry of VARIANTS[mode]."""
    name, qmul, sparse = variant
    case = random_case(B, S, H, hd, mode, seed=seed, qmul=qmul)
    if sparse:
        d = case.dout.view(B, S, H, hd)
        for col, row in enumerate(sparse_rows(case)):
            keep = d[0, row, 0, col].clone()
            d[0, :, 0, col] = 0.0
            d[0, row, 0, col] = keep if float(keep) != 0.0 else 1.0
    case.variant = name
    return case


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def uniform_case(B, S, H, hd, mode, seed=0):
    """q = 0, k random, v and dO integers in {-8..8}: every score is 0 and P is 2^-5 in every slot (module docstring)."""
    g = torch.Generator().manual_seed(77 + 1000 * S + hd + seed)
    t = torch.randn(B, S, 3, H, hd, generator=g)
    t[:, :, 0] = 0.0
    t[:, :, 2] = _ints(g, -8, 8, B, S, H, hd)
    dout = bf(_ints(g, -8, 8, B * S, H * hd))
    return Case(B, S, H, hd, mode, bf(t.reshape(B * S, 3 * H * hd)), dout)


def sign_codes(n, hd, dmin, g):
    """n rows of +-1 of length hd with pairwise Hamming distance >= dmin (greedy rejection)."""
    codes = torch.empty(0, hd)
    while codes.shape[0] < n:
        cand = torch.randint(0, 2, (4 * n, hd), generator=g).float() * 2 - 1
        for row in cand:
            if codes.shape[0] == n:
                break
            if codes.shape[0] == 0 or float(((codes != row).sum(1)).min()) >= dmin:
                codes = torch.cat([codes, row[None]])
    return codes


def onehot_dmin(hd):
    return 5 if hd <= 24 else 8 if hd <= 32 else hd // 4


def onehot_case(B, S, H, hd, mode, seed=0):
    """k rows = g * sign codes (pairwise Hamming distance >= dmin), q_i = k_pi(i) (the pre-scaled form stores bf16(q c), exact up to one
    rounding of g c), v and dO = +-[0.25, 4).  g is the smallest power of two that meets onehot_conditions.  Returns (case, pi [B, H, S])."""
    g_ = torch.Generator().manual_seed(4242 + 1000 * S + hd + seed)
    dmin = onehot_dmin(hd)
    c_eff = 0.125 if mode == "pow2" else f32(hd ** -0.5) * LOG2E
    u_fold = U_BF16 if mode == "fold" else 0.0
    gg = 1.0
    while 2 * c_eff * gg * gg * dmin - 2 * (u_fold + (hd + 1) * E_F32) * c_eff * gg * gg * hd < 33.0:
        gg *= 2.0
        assert gg <= 64.0, "no power-of-two amplitude meets the gap condition"
    t = torch.empty(B, S, 3, H, hd)
    pi = torch.empty(B, H, S, dtype=torch.int64)
    for b in range(B):
        for h in range(H):
            codes = sign_codes(S, hd, dmin, g_) * gg
            p = torch.randperm(S, generator=g_)
            pi[b, h] = p
            t[b, :, 1, h] = codes
            t[b, :, 0, h] = codes[p] * (c_eff if mode == "pre" else 1.0)

    def pm(*shape):
        return (0.25 + 3.75 * torch.rand(shape, generator=g_)) * (torch.randint(0, 2, shape, generator=g_).float() * 2 - 1)
    t[:, :, 2] = pm(B, S, H, hd)
    dout = bf(pm(B * S, H * hd))
    return Case(B, S, H, hd, mode, bf(t.reshape(B * S, 3 * H * hd)), dout), pi


def onehot_conditions(case, pi):
    """The conditions under which the one-hot outputs follow from the reference alone (asserted on the host), from float64:
    (1) the winner of query i is key pi(i) and its score exceeds the runner-up's by >= 32 log2 units after subtracting the worst-case
        rounding 2 (u_fold + (hd+1) e) T of the two scores;
    (2) S 2^-gap max|x| / min|x| (x = v, dO) plus the fp32 roundings (N + hd + 8) e stays below 2^-11: the weight every other key adds to
        the winner's value cannot move its bf16 rounding, not even below a power of two.
    Returns (gap, leak)."""
    q, k, v = case.qkv64()
    s2 = case.c * q @ k.transpose(-1, -2)
    T = abs(case.c) * q.abs() @ k.abs().transpose(-1, -2)
    noise = (case.u_fold + (case.hd + 1) * E_F32) * T
    win = torch.gather(s2 - noise, -1, pi[..., None].to(s2.device))
    rest = (s2 + noise).scatter(-1, pi[..., None].to(s2.device), float("-inf"))
    gap = float((win - rest.amax(-1, keepdim=True)).min()) if case.S > 1 else float("inf")
    assert gap >= 32.0, gap
    d = case.dout.double().abs()
    ratio = max(float(v.abs().max() / v.abs().min()), float(d.max() / d.min()))
    leak = case.S * 2.0 ** -gap * ratio + (case.S + case.hd + 8) * E_F32
    assert leak < 2.0 ** -11, leak
    return gap, leak


def onehot_expected(case, pi):
    """(o_expected [B*S, H*hd], scatter index) : o[i] = v[pi(i)];  dV[pi(i)] = dO[i]."""
    _, _, v = split_qkv(case.qkv, case.B, case.S, case.H, case.hd)
    idx = pi[..., None].expand(-1, -1, -1, case.hd).to(v.device)
    o_exp = torch.gather(v, 2, idx)                                         # [B, H, S, hd]
    dO = split_heads(case.dout, case.B, case.S, case.H, case.hd)
    dv_exp = torch.empty_like(o_exp).scatter_(2, idx, dO)
    return merge_heads(o_exp), merge_heads(dv_exp)


# ------------------------------------------------------------------------------------------------ float64 references + bounds
def _wabs_diff(w, v, ref, chunk=8):
    """A[.., q, d] = sum_k w[.., q, k] |v[.., k, d] - ref[.., q, d]|, the [S, S, d] term chunked over d."""
    out = torch.empty_like(ref)
    for d0 in range(0, v.shape[-1], chunk):
        dv = (v[..., None, :, d0:d0 + chunk] - ref[..., :, None, d0:d0 + chunk]).abs()       # [.., q, k, c]
        out[..., d0:d0 + chunk] = (w[..., None] * dv).sum(-2)
    return out


def _rounded(ref, r):
    """bound of a bf16-stored value whose fp32 value lies within r of ref: the rounding is relative to the COMPUTED value,
    u (|ref| + r), so the total is u |ref| + (1 + u) r."""
    return U_BF16 * ref.abs() + (1 + U_BF16) * r


def forward_reference(case, exact_scores=False):
    """dict(o, tol_o [B, H, S, hd], lse, tol_lse [B, H, S], p) in float64.  exact_scores: eps = 0 and no bf16 rounding of P (every P is
    the same power of two: the uniform case)."""
    q, k, v = case.qkv64()
    N, hd = case.S, case.hd
    s2 = case.c * q @ k.transpose(-1, -2)
    m = s2.amax(-1, keepdim=True)
    pu = torch.exp2(s2 - m)
    l = pu.sum(-1, keepdim=True)
    p = pu / l
    lse = (m + torch.log2(l)).squeeze(-1)
    ref = p @ v
    if exact_scores:
        eps = torch.zeros_like(s2)
        eta = torch.full_like(s2, (1 + (N + 2) * E_F32) - 1)
    else:
        T = abs(case.c) * q.abs() @ k.abs().transpose(-1, -2)
        eps = (case.u_fold + (hd + 1) * E_F32) * T + E_F32 * s2.abs() + 3 * E_F32 * (s2.abs().amax(-1, keepdim=True) + HEADROOM)
        eta = torch.exp2(eps) * (1 + U_BF16) * (1 + (N + 2) * E_F32) - 1
    w = p * eta
    sw = w.sum(-1, keepdim=True)
    lead = _wabs_diff(w, v, ref) / (1 - sw)
    lead = torch.where(sw < 1, lead, torch.full_like(lead, float("inf")))
    tol_o = _rounded(ref, lead + (N + hd + 3) * E_F32 * (p @ v.abs()) + N * FLUSH * 2.0 ** 6 * float(v.abs().max()))
    tol_lse = eps.amax(-1) + math.log2(1 + (0 if exact_scores else U_BF16) + (N + 2) * E_F32) + 2 * E_F32 * (lse.abs() + 8)
    return dict(o=ref, tol_o=tol_o, lse=lse, tol_lse=tol_lse, p=p)


def backward_reference(case, o_in, lse_in):
    """dict(dq, dk, dv, tol_dq, tol_dk, tol_dv) [B, H, S, hd] float64 from (case.qkv, o_in [B*S, H*hd] bf16, case.dout, lse_in [B, H, S] fp32)."""
    q, k, v = case.qkv64()
    dO = case.dout64()
    o = split_heads(o_in, case.B, case.S, case.H, case.hd).double()
    lse = lse_in.double().view(case.B, case.H, case.S, 1)
    N, hd, sa, ks = case.S, case.hd, case.sabs, case.kscale
    s2 = case.c * q @ k.transpose(-1, -2)
    T = abs(case.c) * q.abs() @ k.abs().transpose(-1, -2)
    eps = (case.u_fold + (hd + 1) * E_F32) * T + E_F32 * s2.abs() + E_F32 * lse.abs()
    P = torch.exp2(s2 - lse)
    delta = (dO * o).sum(-1, keepdim=True)
    X = dO @ v.transpose(-1, -2) - delta
    dS = P * X
    etap = torch.exp2(eps) * (1 + 2 * E_F32) - 1
    G = dO.abs() @ v.abs().transpose(-1, -2) + (dO.abs() * o.abs()).sum(-1, keepdim=True)
    err = P * (etap * X.abs() + (1 + etap) * ((hd + 1) * E_F32 * G + E_F32 * X.abs()))
    errb = err + U_BF16 * (dS.abs() + err)
    fl = N * 2 * FLUSH * (1 + float(X.abs().max()))
    r = dict(dq=sa * dS @ k, dk=ks * dS.transpose(-1, -2) @ q, dv=P.transpose(-1, -2) @ dO)
    r["tol_dq"] = _rounded(r["dq"], sa * (errb @ k.abs()) + (N + 3) * E_F32 * sa * (dS.abs() @ k.abs()) + fl * sa * float(k.abs().max()))
    r["tol_dk"] = _rounded(r["dk"], ks * (errb.transpose(-1, -2) @ q.abs()) + (N + 3) * E_F32 * ks * (dS.abs().transpose(-1, -2) @ q.abs())
                           + fl * ks * float(q.abs().max()))
    r["tol_dv"] = _rounded(r["dv"], (P * (etap + U_BF16 * (1 + etap))).transpose(-1, -2) @ dO.abs()
                           + (N + 2) * E_F32 * (P.transpose(-1, -2) @ dO.abs()) + fl * float(dO.abs().max()))
    return r


def _block_sums(x, rows):
    """[B, H, S, hd] -> [B * nb, H * hd]: sums over blocks of `rows` token rows (the layout of a column-partial matrix)."""
    B, H, S, hd = x.shape
    nb = (S + rows - 1) // rows
    pad = torch.zeros(B, H, nb * rows - S, hd, dtype=x.dtype, device=x.device)
    y = torch.cat([x, pad], 2).view(B, H, nb, rows, hd).sum(3)                # [B, H, nb, hd]
    return y.permute(0, 2, 1, 3).reshape(B * nb, H * hd)


def partial_reference(ref, tol, rows):
    """(ref, tol) of a column-partial matrix from the per-element (ref, tol) of dQ / dK / dV (module docstring)."""
    S = ref.shape[2]
    n = min(rows, S)
    return _block_sums(ref, rows), _block_sums(tol - U_BF16 * ref.abs(), rows) + n * E_F32 * _block_sums(ref.abs(), rows)


# ------------------------------------------------------------------------------------------------ checker + reporter
def elementwise_report(out, ref, tol, n_show=6):
    """Every element of out [B, H, rows, d] (or [B, H, rows]) against its own bound; NaN / inf fail (`<=` is False for NaN).
    offenders: (b, h, row, row % 128, row % 64, d, out, ref, tol) of the first few."""
    if out.dim() == 3:
        out, ref, tol = out[..., None], ref[..., None], tol[..., None]
    assert out.shape == ref.shape == tol.shape, (out.shape, ref.shape, tol.shape)
    err = (out.double() - ref).abs()
    good = (err <= tol) & torch.isfinite(out.double())      # a NaN / inf output fails whatever its bound
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    bad = (~good).nonzero()
    offenders = [(b, h, r, r % 128, r % 64, d, float(out[b, h, r, d]), float(ref[b, h, r, d]), float(tol[b, h, r, d]))
                 for b, h, r, d in bad[:n_show].tolist()]
    return dict(ok=bool(good.all()), count=int(bad.shape[0]), worst=float(ratio.max()) if ratio.numel() else 0.0,
                offenders=offenders, nonfinite=int((~torch.isfinite(out.double())).sum()))


def assert_elementwise(out, ref, tol, label=""):
    rep = elementwise_report(out, ref, tol)
    assert rep["ok"], (f"{label}: {rep['count']} of {out.numel()} elements outside the derived bound ({rep['nonfinite']} not finite), worst err/tol "
                       f"{rep['worst']:.3g}; first (b, h, row, row%128, row%64, d, out, ref, tol): {rep['offenders']}")
    return rep["worst"]


def check_forward(case, o, lse, exact_scores=False, collect=None, ref=None):
    """o [B*S, H*hd], lse [B, H, S] against forward_reference.  collect = None: assert, return the worst ratios; collect = a dict: no
    assertion, the reports are stored (planted defects)."""
    ref = forward_reference(case, exact_scores) if ref is None else ref
    pairs = [("o", split_heads(o, case.B, case.S, case.H, case.hd), ref["o"], ref["tol_o"]),
             ("lse2", lse.view(case.B, case.H, case.S), ref["lse"], ref["tol_lse"])]
    return _run_pairs(case, pairs, collect)


def _run_pairs(case, pairs, collect):
    worst = {}
    for name, out, r, t in pairs:
        assert bool(torch.isfinite(t).all()) and bool(torch.isfinite(r).all()), f"{name}: the bound is vacuous (non-finite tolerance or reference)"
        label = f"{name} B{case.B} S{case.S} H{case.H} hd{case.hd} {case.mode}"
        if collect is None:
            worst[name] = assert_elementwise(out, r, t, label)
        else:
            collect[name] = elementwise_report(out, r, t)
            worst[name] = collect[name]["worst"]
    return worst


def check_backward(case, o_in, lse_in, dqkv, colq=None, colkv=None, collect=None, ref=None):
    """dqkv [B*S, 3*H*hd] (and the column partials) against backward_reference of the backward's own inputs."""
    B, S, H, hd = case.B, case.S, case.H, case.hd
    ref = backward_reference(case, o_in, lse_in) if ref is None else ref
    dq, dk, dv = split_qkv(dqkv, B, S, H, hd)
    pairs = [("dq", dq, ref["dq"], ref["tol_dq"]), ("dk", dk, ref["dk"], ref["tol_dk"]), ("dv", dv, ref["dv"], ref["tol_dv"])]
    if colq is not None:
        rq, tq = partial_reference(ref["dq"], ref["tol_dq"], 128)
        kb = 64 * dkdv_kt(hd)
        rk, tk = partial_reference(ref["dk"], ref["tol_dk"], kb)
        rv, tv = partial_reference(ref["dv"], ref["tol_dv"], kb)
        assert colq.shape == rq.shape and colkv.shape == (rk.shape[0], 2 * H * hd), (colq.shape, colkv.shape, rq.shape, rk.shape)

        def as4(x):   # [rows, H*hd] -> [1, H, rows, hd]: the reporter's row is the partial row
            return x.view(x.shape[0], H, hd).permute(1, 0, 2)[None]
        pairs += [("colq", as4(colq), as4(rq), as4(tq)), ("colk", as4(colkv[:, :H * hd]), as4(rk), as4(tk)),
                  ("colv", as4(colkv[:, H * hd:]), as4(rv), as4(tv))]
    return _run_pairs(case, pairs, collect)


# ------------------------------------------------------------------------------------------------ poisoned layouts
def embed_rows(value, nan_fill, offset):
    """value [rows, cols] contiguous inside a larger allocation: a band before and after (NaN for inputs, the 0xA5 pattern for outputs);
    the base is `offset` elements (16 bytes) past an aligned address."""
    return Embedded(value.shape[0], value.shape[1], value.shape[1], offset, value.dtype, value.device, nan_fill, value)


def pattern_like(rows, cols, dtype, device):
    """[rows, cols] of the 0xA5 byte pattern (what an untouched output row must still hold)."""
    it = {torch.bfloat16: torch.int16, torch.float32: torch.int32}[dtype]
    t = torch.empty(rows, cols, dtype=it, device=device)
    t.view(torch.uint8).fill_(0xA5)
    return t.view(dtype)


def raw_equal(a, b):
    """bit equality of two tensors of one dtype (NaN patterns included)."""
    it = {torch.bfloat16: torch.int16, torch.float32: torch.int32}[a.dtype]
    return a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))
