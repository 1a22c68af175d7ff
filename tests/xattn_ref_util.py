"""Float64 references, derived per-element bounds, cases and shapes for the attentive probe's cross-attention (csrc/xattn.hip: the
single-workgroup kernels and the split-key forms).  Imported by tests/test_xattn_bound_host.py (CPU) and
tests/test_xattn_elementwise_gpu.py; never collected.

Everything is computed in float64 from the bf16-ROUNDED inputs, per (sample, head[, query]).  u = 2^-8 (half a bf16 ulp, relative),
e = 2^-23 (twice the fp32 unit roundoff, as tests/gemm_ref_util.py), c = scale * log2(e), N keys, hd the head dimension,
T_j = |c| sum_d |q_d| |k_jd|.

FORWARD (out [B*NQ, D] bf16, lse2 [B, H, NQ] fp32).   s2_j = c q.k_j, lse = log2 sum_j 2^s2_j, P_j = 2^(s2_j - lse), o = sum_j P_j v_j,
ref = o + resid.
  eps_j = (hd + 3) e T_j + 2 e |s2_j| + 2 e max_j |s2|        error of s_j - max as the kernel forms it, log2 units
     (hd + 3) e T   the fp32 factor sc = fl(scale * log2e) against c (<= e), fl(q_d sc) (e / 2; there is no bf16 fold), hd fp32
                    products and hd fp32 adds in any order (e / 2 each)
     2 e (|s2_j| + max |s2|)   the rounding of s_j - max (e / 2 of either operand).  The split forms subtract the chunk maximum m_c
                    and later multiply by 2^(m_c - M): two roundings, (e / 2)(|s_j| + 2 |m_c| + |M|), still inside this term
  eta_j = 2^(eps_j + max_j eps) (1 + (n_add + 4) e) - 1       relative error of one term of the numerator OR of the denominator.  P is
     never rounded to bf16; the sums of the numerator and of the denominator have independent rounding errors (n_add adds on top of
     v_exp_f32, the product p v, the weight 2^(m_c - M) of the split forms and the division: <= 4 e), and the computed maximum sits
     within max eps of the true one.
  o' - o = sum_j P_j eta_j (v_j - o) / (1 + sum_j P_j eta_j), hence
  R       = sum_j P_j eta_j |v_j - o| / (1 - sum_j P_j eta_j) + (n_add + hd + 3) e sum_j P_j |v_j| + e |ref| + flush
  tol_out = u |ref| + (1 + u) R          (the bf16 rounding is relative to the computed value, which lies within R of ref)
  tol_lse = max_j eps + log2(1 + (n_add + 4) e) + 2 e (|lse| + 8)          (log2f of the sum, the final add)
     e |ref|  the fp32 add of the residual.
     flush    NOT in the issue's list, derived here as in tests/attn_ref_util.py: v_exp_f32 may flush a result below 2^-126 to zero,
              an absolute 2^-126 on a probability measured against a denominator >= 1; the split forms also flush the weight
              2^(m_c - M), which multiplies l_c <= 2^11 and |y_c| <= 2^11 max |v|.  (N + 2^11 chunks) 2^-125 max |v|.

  n_add is NOT N.  With n_add = N the sum term alone is 3 u |ref| at N = 4 * 10^4, and a dropped or doubled key hides under it.  The
  kernels add in a FIXED order, and the error of a sum is bounded by (depth) e / 2 sum |x|, depth = the longest chain of additions
  one addend passes through (Higham, Accuracy and Stability of Numerical Algorithms, 4.2: any summation tree).  chain_len(N, hd,
  split) derives it from the kernels' loops, n = the keys of one workgroup (N, or XA_CHUNK = 2048 in the split forms):
     block sums (denominator, delta)    ceil(n / 256) adds of the per-thread stride loop + 6 levels of the wave tree + 4 waves
     weighted rows (numerator, dq)      ngrp = 256 / (hd / 8) row groups: ceil(n / ngrp) adds per thread + ngrp partials added in turn
     split forms                        + the chunks, merged in ascending order
  and takes the larger of the two, so that one number serves every sum.

BACKWARD (dq [B, D], dkv [B*N, 2*D] bf16; one query per sample).  A function of its OWN inputs (q, kv, dy, lse2_in): nothing of the
forward enters.  P_j = 2^(s2_j - lse2_in), dP_j = dy.v_j, G_j = |dy|.|v_j|, delta = sum_j P_j dP_j, X_j = dP_j - delta, dS_j = P_j X_j,
dq = scale sum_j dS_j k_j, dk_j = dS_j (q scale), dv_j = P_j dy.
  eps'_j = (hd + 3) e T_j + 2 e |s2_j| + e |lse2_in|         (the rounding of s_j - lse2_in in place of the maximum term)
  eta'_j = 2^eps'_j (1 + 2 e) - 1                            (v_exp_f32; no sum, no bf16 rounding)
  err(dP_j) = (hd + 1) e G_j
  err(delta) = sum_j P_j (eta'_j |dP_j| + (1 + eta'_j) err(dP_j)) + (n_add + 2) e sum_j P_j (1 + eta'_j) (|dP_j| + err(dP_j))
               (derived here: the propagated errors of p_j and dP_j, then the fp32 products and the fixed-order sum)
  err(dS_j) = P_j [eta'_j |X_j| + (1 + eta'_j) (err(dP_j) + err(delta) + 2 e |X_j|)]       (the subtraction and the product: 2 e |X|)
  tol_dq = u |ref| + (1 + u) (|scale| sum_j err(dS_j) |k_j| + (n_add + 3) e |scale| sum_j (|dS_j| + err(dS_j)) |k_j| + N fl |scale| max |k|)
  tol_dk = u |ref| + (1 + u) |scale| |q| (err(dS_j) + 2 e (|dS_j| + err(dS_j)) + fl)         (fl(q scale) and the product with dS_j)
  tol_dv = u |ref| + (1 + u) |dy| (P_j eta'_j + 2 e P_j (1 + eta'_j) + fl)
     fl = 2^-125 (1 + max |X|): p_j, dS_j, or a product below 2^-126 flushed to zero (derived as in tests/attn_ref_util.py).

CASES, drawn on the CPU and seeded by shape (make_case).  plain: q, k, v, dy, resid ~ N(0, 1).  peaked: q x 4.  aimed: resid = None,
every k clamped to |k| <= 4, then for up to four edge keys (aimed_keys: the last key, the last key of chunk 0 and the first of chunk 1
in the split forms, the first key that only the last row-group pass reaches; padded with keys 0, 1, ... where those coincide)
k_j* = 8 r with four sign vectors r at pairwise Hamming distance hd / 2, and every query = 8 r of the key it is aimed at (jstar
[B, H, NQ]: the four (sample, head) slices of B = H = 2 aim at four different keys, the NQ = 3 queries of a slice at three).  The aimed
key scores 64 hd c = 92 sqrt(hd), the other edge keys exactly 0, every other key at most half of that; aimed_conditions asserts in
float64 that the gap to the runner-up, after the worst-case rounding eps of both scores, is >= 40 + log2 N, and that what all other
keys together add (N 2^-gap max |v| / min |v_j*|) stays below 2^-11 of the smallest element of v_j*: then out == v[j*] bit for bit.
The q = 0 integer pin stays in tests/test_xattn_long_gpu.py."""
import math

import numpy as np
import torch

from tests.gemm_ref_util import (E_F32, U_BF16, Embedded, assert_bit_equal, assert_elementwise,  # noqa: F401  (re-exported)
                                 elementwise_report)

LOG2E = math.log2(math.e)
LOG2E_F32 = np.float32(1.4426950408889634)      # the kernels' constant
FLUSH = 2.0 ** -126
XA_THREADS, XA_CHUNK = 256, 2048
FWD_MAX, BWD_MAX = 38264, 19132                 # keys the single-workgroup kernels hold in LDS (asserted against vj_xattn_ws_bytes on the GPU)
B0, H0 = 2, 2
VARIANTS = ["plain", "peaked", "aimed"]

# section 3 of the issue.  ngrp = 256 / (hd / 8) row groups: 16 (hd 128), 25 (80), 32 (64), 85 (24), 256 (8)
N_SINGLE = [1, 2, 15, 16, 17, 24, 25, 26, 31, 32, 33, 84, 85, 86, 255, 256, 257, 513]
HD_MAIN = [8, 24, 64, 80, 128]
HD_ALL = list(range(8, 129, 8))
SINGLE_SHAPES = [(N, hd) for N in N_SINGLE for hd in HD_MAIN] + [(N, hd) for N in (86, 257) for hd in HD_ALL if hd not in HD_MAIN]
HD_LARGE = [8, 24, 80, 128]
LIMIT_BWD_SHAPES = [(BWD_MAX, hd) for hd in (8, 128)]            # the last LDS score slot: (XA_LDS_FIXED + 2 N) * 4 == XA_LDS_MAX
LIMIT_FWD_SHAPES = [(FWD_MAX, hd) for hd in (8, 128)]
SPLIT_BWD_SHAPES = [(N, hd) for N in (19133, 20480, 20481) for hd in HD_LARGE]   # ragged last chunk | ten full chunks | a chunk of one key
SPLIT_FWD_SHAPES = [(N, hd) for N in (38265, 40960, 40961) for hd in HD_LARGE]
LARGE_BWD_SHAPES = LIMIT_BWD_SHAPES + SPLIT_BWD_SHAPES           # NQ = 1, backward
LARGE_FWD_SHAPES = LIMIT_FWD_SHAPES + SPLIT_FWD_SHAPES           # NQ = 3, forward


def shared_settings(N, hd):
    """q shared by the samples (q_bstride = 0) and per sample: both at the small shapes, alternating by shape at the large ones."""
    return (True, False) if N <= 513 else ((N + hd // 8) % 2 == 0,)


def bf(x):
    return x.to(torch.bfloat16)


def f32(x):
    return float(np.float32(x))


def n_groups(hd):
    return XA_THREADS // (hd // 8)


def chunks_of(N, split):
    """[(j0, n)] of the workgroups of one (b, h[, query]): the whole sequence, or chunks of XA_CHUNK keys."""
    return [(j0, min(XA_CHUNK, N - j0)) for j0 in range(0, N, XA_CHUNK)] if split else [(0, N)]


def chain_len(N, hd, split):
    """the longest chain of fp32 additions one addend of any of the kernels' sums passes through (module docstring)."""
    n = min(N, XA_CHUNK) if split else N
    ngrp = n_groups(hd)
    block = -(-n // XA_THREADS) + 6 + XA_THREADS // 64
    rows = -(-n // ngrp) + ngrp
    return max(block, rows) + (-(-N // XA_CHUNK) if split else 0)


def aimed_keys(N, hd, split):
    """the edge keys of the aimed cases, most telling first; distinct, at most four (padded with keys 0, 1, ... up to min(4, N))."""
    j0, n = chunks_of(N, split)[-1]
    ngrp = n_groups(hd)
    keys = [N - 1] + ([XA_CHUNK - 1, XA_CHUNK] if split else []) + [j0 + (n - 1) // ngrp * ngrp]
    out = []
    for j in keys + list(range(min(4, N))):
        if j not in out and len(out) < 4:
            out.append(j)
    return out


# ------------------------------------------------------------------------------------------------ cases
class Case:
    """One cross-attention problem in the layouts of the C ABI: q [Bq, NQ, D] (Bq = 1: shared by the samples), kv [B*N, 2*D] (row =
    [K | V] of one key), resid [NQ, D] or None, dy [B, D]; bf16.  scale is exactly representable in fp32; c = scale * log2(e)."""

    def __init__(self, B, NQ, N, H, hd, shared, variant, q, kv, resid, dy, jstar=None):
        self.B, self.NQ, self.N, self.H, self.hd, self.shared, self.variant = B, NQ, N, H, hd, shared, variant
        self.q, self.kv, self.resid, self.dy, self.jstar = q, kv, resid, dy, jstar
        self.D = H * hd
        self.scale = f32(hd ** -0.5)
        self.c = self.scale * LOG2E

    def to(self, device):
        mv = lambda t: None if t is None else t.to(device)   # noqa: E731
        return Case(self.B, self.NQ, self.N, self.H, self.hd, self.shared, self.variant, mv(self.q), mv(self.kv), mv(self.resid),
                    mv(self.dy), mv(self.jstar))

    @property
    def label(self):
        return f"B{self.B} NQ{self.NQ} N{self.N} H{self.H} hd{self.hd} {'shared' if self.shared else 'per-sample'} q {self.variant}"

    def q4(self):
        """[B, H, NQ, hd] (a view; expanded over the samples when shared)"""
        return self.q.view(-1, self.NQ, self.H, self.hd).expand(self.B, -1, -1, -1).permute(0, 2, 1, 3)

    def kv4(self):
        """k, v [B, H, N, hd] (views)"""
        t = self.kv.view(self.B, self.N, 2, self.H, self.hd).permute(2, 0, 3, 1, 4)
        return t[0], t[1]

    def resid4(self):
        """[1, H, NQ, hd] or None"""
        return None if self.resid is None else self.resid.view(1, self.NQ, self.H, self.hd).permute(0, 2, 1, 3)

    def dy3(self):
        """[B, H, hd]"""
        return self.dy.view(self.B, self.H, self.hd)


def _sign_masks(hd):
    """four +-1 masks: multiplied into one sign vector they give four vectors at pairwise Hamming distance hd / 2 (inner product 0)."""
    d = torch.arange(hd)
    first, alt = torch.where(d < hd // 2, -1.0, 1.0), torch.where(d % 2 == 0, -1.0, 1.0)
    return torch.stack([torch.ones(hd), first, alt, first * alt])


def make_case(B, NQ, N, H, hd, shared, variant, split=False, seed=0):
    """The case of one (shape, variant) (module docstring); `split`: the aimed keys are those of the split forms."""
    g = torch.Generator().manual_seed(1000 * N + 8 * hd + 2 * NQ + int(shared) + 100003 * seed)
    D, Bq = H * hd, 1 if shared else B
    q = torch.randn(Bq, NQ, H, hd, generator=g)
    kv = torch.randn(B, N, 2, H, hd, generator=g)
    resid = torch.randn(NQ, D, generator=g)
    dy = torch.randn(B, D, generator=g)
    jstar = None
    if variant == "peaked":
        q *= 4.0
    elif variant == "aimed":
        keys = aimed_keys(N, hd, split)
        r = (torch.randint(0, 2, (Bq, H, hd), generator=g).float() * 2 - 1)[:, :, None, :] * _sign_masks(hd)     # [Bq, H, 4, hd]
        kv[:, :, 0].clamp_(-4.0, 4.0)
        jstar = torch.empty(B, H, NQ, dtype=torch.int64)
        for b in range(B):
            for h in range(H):
                for pos in range(len(keys)):           # vector `pos` sits on another key in every sample, so a shared q aims elsewhere
                    kv[b, keys[(pos + b * H) % len(keys)], 0, h] = 8.0 * r[b % Bq, h, pos]
                for iq in range(NQ):
                    pos = (h + iq) % len(keys)
                    q[b % Bq, iq, h] = 8.0 * r[b % Bq, h, pos]
                    jstar[b, h, iq] = keys[(pos + b * H) % len(keys)]
        resid = None
    elif variant != "plain":
        raise ValueError(variant)
    case = Case(B, NQ, N, H, hd, shared, variant, bf(q.reshape(Bq, NQ, D)), bf(kv.reshape(B * N, 2 * D)),
                None if resid is None else bf(resid), bf(dy), jstar)
    if variant == "aimed":
        case.gap, case.leak = aimed_conditions(case)
    return case


def score_noise(case, s2, T, smax):
    """eps of the forward (module docstring) from s2, T [.., N] and smax [.., 1]."""
    return (case.hd + 3) * E_F32 * T + 2 * E_F32 * s2.abs() + 2 * E_F32 * smax


def aimed_conditions(case):
    """The conditions under which out == v[j*] follows from the reference alone (module docstring), from float64.  Returns (gap, leak)."""
    q, (k, v) = case.q4().double(), [t.double() for t in case.kv4()]
    s2 = case.c * q @ k.transpose(-1, -2)
    T = abs(case.c) * q.abs() @ k.abs().transpose(-1, -2)
    noise = score_noise(case, s2, T, s2.abs().amax(-1, keepdim=True))
    idx = case.jstar[..., None].to(s2.device)
    win = torch.gather(s2 - noise, -1, idx)
    rest = (s2 + noise).scatter(-1, idx, float("-inf"))
    gap = float((win - rest.amax(-1, keepdim=True)).min()) if case.N > 1 else float("inf")
    assert gap >= 40.0 + math.log2(case.N), (case.label, gap)
    vstar = torch.gather(v, 2, idx.expand(-1, -1, -1, case.hd))                     # [B, H, NQ, hd]
    leak = case.N * 2.0 ** -gap * float(v.abs().max()) / float(vstar.abs().min())
    assert leak < 2.0 ** -11, (case.label, leak)      # 2^-40 max |v| / min |v_j*| in fact: no fp32 add of the chain even rounds
    return gap, leak


def aimed_expected(case):
    """out [B*NQ, D] of an aimed forward without residual: v[j*], bit for bit."""
    _, v = case.kv4()
    idx = case.jstar[..., None].expand(-1, -1, -1, case.hd).to(v.device)
    return torch.gather(v, 2, idx).permute(0, 2, 1, 3).reshape(case.B * case.NQ, case.D)


# ------------------------------------------------------------------------------------------------ float64 references + bounds
def _rounded(ref, r):
    return U_BF16 * ref.abs() + (1 + U_BF16) * r


def forward_reference(case, split):
    """dict(out, tol_out [B, H, NQ, hd], lse, tol_lse [B, H, NQ]) in float64 on the case's device."""
    q, (k, v) = case.q4().double(), [t.double() for t in case.kv4()]
    N, hd = case.N, case.hd
    n_add = chain_len(N, hd, split)
    s2 = case.c * q @ k.transpose(-1, -2)                                        # [B, H, NQ, N]
    T = abs(case.c) * q.abs() @ k.abs().transpose(-1, -2)
    m = s2.amax(-1, keepdim=True)
    lse = m + torch.log2(torch.exp2(s2 - m).sum(-1, keepdim=True))
    P = torch.exp2(s2 - lse)
    o = P @ v
    ref = o if case.resid is None else o + case.resid4().double()
    eps = score_noise(case, s2, T, s2.abs().amax(-1, keepdim=True))
    eta = torch.exp2(eps + eps.amax(-1, keepdim=True)) * (1 + (n_add + 4) * E_F32) - 1
    w = P * eta
    sw = w.sum(-1, keepdim=True)
    lead = torch.empty_like(o)
    for iq in range(case.NQ):                                                       # sum_j w_j |v_j - o|, one [B, H, N, hd] at a time
        lead[:, :, iq] = ((v - o[:, :, iq, None]).abs_() * w[:, :, iq, :, None]).sum(-2)
    lead = torch.where(sw < 1, lead / (1 - sw), torch.full_like(lead, float("inf")))
    vabs = v.abs()
    flush = (N + XA_CHUNK * (-(-N // XA_CHUNK))) * 2 * FLUSH * float(vabs.max())
    R = lead + (n_add + hd + 3) * E_F32 * (P @ vabs) + E_F32 * ref.abs() + flush
    tol_lse = eps.amax(-1) + math.log2(1 + (n_add + 4) * E_F32) + 2 * E_F32 * (lse.squeeze(-1).abs() + 8)
    return dict(out=ref, tol_out=_rounded(ref, R), lse=lse.squeeze(-1), tol_lse=tol_lse)


def lse_input(case):
    """lse2 [B, H] fp32 a backward is fed with: the float64 value rounded once (independent of any forward under test)."""
    assert case.NQ == 1
    q, k = case.q4().double(), case.kv4()[0].double()
    s2 = (case.c * q @ k.transpose(-1, -2)).squeeze(2)
    m = s2.amax(-1, keepdim=True)
    return (m + torch.log2(torch.exp2(s2 - m).sum(-1, keepdim=True))).squeeze(-1).float()


def backward_reference(case, lse_in, split):
    """dict(dq, tol_dq [B, H, hd], dk, dv, tol_dk, tol_dv [B, H, N, hd]) in float64 from (q, kv, dy, lse_in [B, H] fp32)."""
    assert case.NQ == 1
    q, (k, v), dy = case.q4().double().squeeze(2), [t.double() for t in case.kv4()], case.dy3().double()        # q, dy [B, H, hd]
    N, hd, sa = case.N, case.hd, abs(case.scale)
    n_add = chain_len(N, hd, split)
    kabs = k.abs()
    s2 = case.c * torch.einsum("bhnd,bhd->bhn", k, q)
    T = abs(case.c) * torch.einsum("bhnd,bhd->bhn", kabs, q.abs())
    lse = lse_in.double().view(case.B, case.H, 1)
    eps = (hd + 3) * E_F32 * T + 2 * E_F32 * s2.abs() + E_F32 * lse.abs()
    P = torch.exp2(s2 - lse)
    etap = torch.exp2(eps) * (1 + 2 * E_F32) - 1
    dP = torch.einsum("bhnd,bhd->bhn", v, dy)
    edP = (hd + 1) * E_F32 * torch.einsum("bhnd,bhd->bhn", v.abs(), dy.abs())
    delta = (P * dP).sum(-1, keepdim=True)
    err_delta = ((P * (etap * dP.abs() + (1 + etap) * edP)).sum(-1, keepdim=True)
                 + (n_add + 2) * E_F32 * (P * (1 + etap) * (dP.abs() + edP)).sum(-1, keepdim=True))
    X = dP - delta
    dS = P * X
    errS = P * (etap * X.abs() + (1 + etap) * (edP + err_delta + 2 * E_F32 * X.abs()))
    fl = 2 * FLUSH * (1 + float(X.abs().max()))
    r = dict(dq=case.scale * torch.einsum("bhn,bhnd->bhd", dS, k), dk=case.scale * dS[..., None] * q[:, :, None, :],
             dv=P[..., None] * dy[:, :, None, :])
    tot = dS.abs() + errS
    r["tol_dq"] = _rounded(r["dq"], sa * torch.einsum("bhn,bhnd->bhd", errS + (n_add + 3) * E_F32 * tot, kabs) + N * fl * sa * float(kabs.max()))
    r["tol_dk"] = _rounded(r["dk"], sa * (errS + 2 * E_F32 * tot + fl)[..., None] * q.abs()[:, :, None, :])
    r["tol_dv"] = _rounded(r["dv"], (P * (etap + 2 * E_F32 * (1 + etap)) + fl)[..., None] * dy.abs()[:, :, None, :])
    return r


# ------------------------------------------------------------------------------------------------ the checker
def out4(case, out):
    """out [B*NQ, D] -> [B, H, NQ, hd] (a view)"""
    return out.view(case.B, case.NQ, case.H, case.hd).permute(0, 2, 1, 3)


def dkv4(case, dkv):
    """dkv [B*N, 2*D] -> dk, dv [B, H, N, hd] (views)"""
    t = dkv.view(case.B, case.N, 2, case.H, case.hd).permute(2, 0, 3, 1, 4)
    return t[0], t[1]


def _run_pairs(case, pairs, sl, collect):
    """every (name, out, ref, tol) -- the whole tensors, or the (b, h) slice `sl` of each -- through the element-wise checker of
    tests/gemm_ref_util.py as [rows, columns].  collect = None: assert; a dict: the reports are stored (planted defects).  Returns the
    worst err/tol per name."""
    worst = {}
    for name, out, ref, tol in pairs:
        if sl is not None:
            out, ref, tol = out[sl], ref[sl], tol[sl]
        assert bool(torch.isfinite(tol).all()) and bool(torch.isfinite(ref).all()), f"{name} {case.label}: the bound is vacuous"
        o2, r2, t2 = [x.reshape(-1, x.shape[-1]) for x in (out, ref, tol)]
        if collect is None:
            worst[name] = assert_elementwise(o2, r2, t2, f"{name} {case.label} (row = ((b * H + h) * rows + row of the slice)")
        else:
            collect[name] = elementwise_report(o2, r2, t2)
            worst[name] = collect[name]["worst"]
    return worst


def check_forward(case, out, lse, ref, sl=None, collect=None):
    """out [B*NQ, D] bf16, lse [B, H, NQ] fp32 against forward_reference."""
    pairs = [("out", out4(case, out), ref["out"], ref["tol_out"]), ("lse2", lse.view(case.B, case.H, case.NQ), ref["lse"], ref["tol_lse"])]
    return _run_pairs(case, pairs, sl, collect)


def check_backward(case, dq, dkv, ref, sl=None, collect=None):
    """dq [B, D], dkv [B*N, 2*D] bf16 against backward_reference."""
    dk, dv = dkv4(case, dkv)
    pairs = [("dq", dq.view(case.B, case.H, case.hd), ref["dq"], ref["tol_dq"]), ("dk", dk, ref["dk"], ref["tol_dk"]),
             ("dv", dv, ref["dv"], ref["tol_dv"])]
    return _run_pairs(case, pairs, sl, collect)
