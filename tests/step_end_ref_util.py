"""Float64 references, derived per-element bounds, pins, input variants and shapes for the kernels every training step ends in:
csrc/loss.hip (latent_loss + scalar_finish, token_pstd, reg_grad, reg_finish) and csrc/optim.hip (adamw_ema and its guarded form,
step_advance, ema, sqnorm, grad_stats_multi).  Imported by tests/test_step_end_bound_host.py (CPU: an fp32 emulation of every kernel in
its own order has to pass, the same emulation with one planted defect has to fail) and tests/test_step_end_elementwise_gpu.py (the real
kernels); never collected.

Everything is computed in float64 from the kernel's own inputs (bf16 / fp32 tensors; scalars as the fp32 values the C ABI receives).
u = 2^-8 (one bf16 rounding, relative), e = 2^-24 (one fp32 operation, relative).  A sum of fp32 terms has |error| <= depth e sum |term|,
depth = the longest chain of additions a term passes through (Higham, Accuracy and Stability, 4.2).  LEVELS = 6 + 3: the xor butterfly
over the 64 lanes of a wave (wave_sum) and wave 0 + 1 + 2 + 3 (block4_total), as written in common.hpp.  Contraction (-ffp-contract=fast)
only removes roundings from the lists below, so the bounds hold for either choice of the compiler; the pins name the places where the
source fixes the choice.  NaN and inf fail every bound; nothing is excluded.

latent_loss     d = z - h (one fp32 subtraction: a = |d| carries e), term = a^p / p (p = 1: a).
  loss          ref = out_scale sum term (+ old);  tol = |out_scale| (depth e sum term + sum terr) + e |out_scale sum| (+ e |ref| when
                accumulating).  depth = 8 ceil(n8 / (512 * 256)) + LEVELS + 2 + LEVELS: a thread adds the EIGHT terms of a chunk in turn
                (not one add per chunk), one chunk per trip; scalar_finish adds 2 of the 512 partials per thread, then its own levels.
                terr = e a (p = 1), else (p e + pow(a, p) + e) term: the rounding of d taken to the power p, __powf, the division.
  dz (bf16)     ref = sign(d) a^(p-1) gscale;  tol = u |ref| (1 + F) + F |ref|,  F = |p - 1| e + pow(a, p - 1) + e (p = 1: F = 0, the
                value is +-gscale rounded once).  d == 0: tol = 0 and the sign of the zero is pinned: +0 for p = 1 (also for d = -0),
                -0 for p != 1 (m = 0, and -m * gscale is what both d = +0 and d = -0 take).
  pow(a, q)     = (C |q log2 a| + K) e, the relative error of __powf(a, q) = exp2(q * log2(a)), C = 2.1, K = 2.  ASSUMPTION: the hardware
                log2 and exp2 are each good to one ulp = 2 e.  log2's ulp and the rounding of the product q * log2(a) move the exponent by
                at most 3 e |q log2 a|; exp2 turns an absolute error D of its argument into the relative error 2^D - 1 <= ln 2 D (1 + D):
                3 ln 2 = 2.0794 < 2.1 = C (the difference covers the second order while 3 e |q log2 a| < 2^-7, i.e. for every fp32 a);
                K = exp2's own ulp.  (The toolchain this was measured with lowers __powf to the library pow, which is more accurate than
                the form assumed; the bound is the one of the form the source asks for.)
  non-finite    torch autograd of mean(|z - h|^p) / p on the CPU (float32; NaN, +inf, -inf in z or in h, and inf - inf):
                p = 1: d = NaN -> grad 0 (abs' backward multiplies by sgn, and sgn(NaN) is 0), d = +-inf -> +-1/n;  p = 2 and 1.5:
                d = NaN -> NaN, d = +-inf -> +-inf.  The loss is NaN (inf without a NaN) in every case.  So for p = 1 the kernel already
                agreed with torch (a NaN target row gives a NaN loss and a ZERO gradient there too: the reference's GradScaler does not
                skip that step either) and its behaviour is pinned as it was; for p != 1 it wrote -0 where torch writes NaN, and
                latent_loss_kernel now passes the NaN on.  Finite inputs keep every bit (the select takes the same arm).
token_pstd      t = z - z[row 0] (exact for bf16 rows within 2^16 of each other, counted as a rounding anyway), K rows, var the float64
                unbiased variance, x = var + fl32(1e-4), pstd = sqrt(x).
  var           tv = (depth + 7) e (sum t^2 + (sum |t|)^2 / K) / (K - 1) + e x,  depth = ceil(K / 32) + 32: a row lane adds its rows
                in turn, then one thread adds the 32 lanes in turn.  + 7: the rounding of t (twice in t^2), the product t * t, ss * ss,
                / K, the subtraction, / (K - 1); e x: the addition of eps.
  pstd, stats1  tol = tv / (2 pstd) (1 + tv / x) + e pstd  (sqrt is concave: the second factor bounds the second order, tv / x < 1/8 is
                asserted; e pstd: sqrtf, correctly rounded).  Accumulating: ref = old + pstd, + e |ref|.
  stats0        ref = mean,  tol = depth e sum |t| / K + e |sum t| / K + e |mean|  (the sum, / K, the shift added back)
  const         every column constant: t == 0, so pstd == sqrtf(1e-4f) and stats0 == the constant, bit for bit.
  row0_outlier  column mean ~ 24 N(0,1), sigma 1, row 0 at mean + 16 sigma.  The bound grows with the shift: (sum t^2 + (sum |t|)^2 / K)
                is about 2 * 257 (K - 1) var instead of 2 (K - 1) var -- the shifted single pass is ALLOWED to lose a factor ~ 250 when
                row 0 is 16 sigma out.  What it loses: see MEASURED below.
  far_mean      the same columns without the outlier: the bound is as tight as on `rand` while E[z^2] is ~ 600 var, which is what
                rejects the unshifted pass (E[z^2] - E[z]^2) from K = 3 on.  (`offset`, integers near 64, cannot: every z^2, their sums
                and ss * ss are exact in fp32 up to K = 63, and so they are for any two bf16 rows, K = 2.)
reg_grad        term = coef active (z - stats0) / ((K - 1) stats1), active = [pstd_sum / n_masks < 1] (no pstd_sum within 1 % of the
                threshold), ref = dz0 - term;  tol = u |ref| + e (6 |term| + 2 |ref|): the subtraction, the product by coef, (K - 1) *
                stats1, the division, fl(1 / n_masks) and one to spare; the final subtraction and the second order of the bf16 rounding.
                Inactive elements are bit-unchanged.
reg_finish      x = pstd / n_masks, term = max(0, 1 - x), ref = sum term / n;  tol = ((ceil(n / 256) + LEVELS) e sum term + sum terr) / n
                + e |ref|,  terr = 2 e x [x < 1 + 2^-20] + e term  (fl(1 / n_masks) and the product: absolute errors of a term near 0).
adamw           one step in float64 from arbitrary state.  g' = g gs, gs = gscale * min(1, clip / (sqrt(gstat[2 sel]) * norm_scale +
                1e-6)) in float64; G = 1 (plain) or 6 (clipping: sqrt, *, +, /, * gscale, * g) roundings of g'.
  m             ref = m + (g' - m)(1 - b1);  tol = e |ref| + (1 - b1)(3 e |g' - m| + G e |g'|)
  v             ref = v b2 + (1 - b2) g'^2;  tol = e |ref| + e |v b2| + (1 - b2) g'^2 (3 + 2 G) e
  p             den = sqrt(v) / bc2 + eps: tol_den = sqrt(v) / bc2 (tol_v / (2 v) + 3 e) + e den (sqrtf, the rounding of bc2, /; the add)
                upd = (lr / bc1)(m / den):  tol_upd = |upd| (tol_den / den (1 + 2^-10) + 4 e) + (lr / bc1) tol_m / den
                ref = p (1 - lr wd) - upd;  tol = 3 e |p| + tol_upd + e |ref|   (lr * wd, 1 - ., p * decay; the subtraction)
                bc1 = fl32(1 - b1^t), bc2 = fl32(sqrt(1 - b2^t)) enter as the fp32 values both entry points form in double.
  tgt           ref = ema tgt + fl32(1 - ema) p_new with p_new the fp32 value the KERNEL wrote: tol = e (|ema tgt| + |(1 - ema) p_new|) +
                e |ref|; and the bit pin below.
  pins          p_bf16 == bf16(p), tgt_bf16 == bf16(tgt) on the kernel's own fp32 outputs; every operand lives inside poisoned memory
                and a None buffer's neighbours (all surroundings) stay untouched; a skipped step leaves p, m, v, p_bf16, step_dev alone.
ema             tgt' = fmaf(ema, tgt, fl(fl(1 - ema) p))  in the update branch of adamw_ema_kernel (SRC_ROUNDED),
                tgt' = fmaf(fl(1 - ema), src, fl(ema tgt)) in ema_kernel and in the skip branch, bit for bit.  fmaf(a, b, c) is emulated as
                the exact product (48 bits) plus c in float64, rounded once to fp32: a true fma unless the float64 sum lands exactly on
                an fp32 rounding tie.  fma_tie() finds those; the host test asserts that the seeded inputs hold none.
sqnorm          ref = sum g^2 (+ old);  tol = (depth + 1) e sum g^2 (+ e |ref|),  depth = 3 (inside a float4) + ceil(n4 / (1024 * 256))
                + LEVELS + 4 + LEVELS (the finish kernel adds 4 of the 1024 partials per thread).  n = 0 writes [0, 0] (old + 0 when
                accumulating).  out[1] counts the non-finite values exactly.
grad_stats      per chunk c of a tensor: lo = c per, hi = min(lo + per, n), per = ceil(ceil(n / 8) / 4) 4;  ref = the float64 sums over
                [lo, hi);  tol = (3 + ceil(ceil((hi - lo) / 4) / 256) + 1 + LEVELS + 1) e sum |term|;  a chunk with lo >= n is exactly 0;
                NaN fills everything outside [offset, offset + numel), so one element read outside poisons a partial.

MEASURED, worst err / tol over all shapes and variants (the float64 reference is the yardstick, never a kernel's own output; both test
files print these again with -s):

  output                       host emulation   MI355X
  latent_loss  loss            0.10             0.10 (p = 1)  0.07 (p = 2)  0.05 (p = 1.5)
  latent_loss  dz              1.00             0.60 (p = 1)  1.00 (p = 2)  1.00 (p = 1.5)
  token_pstd   pstd            0.91             0.91
  token_pstd   stats0          0.67             0.67
  token_pstd   stats1          0.25             0.25
  reg_grad     dz              1.00             1.00
  reg_finish                   0.13             0.13
  adamw        p / m / v       0.53 0.99 0.99   0.35 0.90 0.52
  adamw        tgt             0.97             0.97
  ema_update   tgt             0.99             0.99
  sqnorm                       0.03             0.03
  grad_stats   partials        0.13             0.13
  (bf16 outputs and single fp32 roundings sit just under 1: some value always lands next to a rounding tie, and half an ulp IS the
   bound's leading term.  __powf: the host's exp2(p * log2(a)) and the GPU both stay inside the assumed bound; the loss uses a twentieth
   of its tolerance.  No bound was widened after a run; the only kernel change is the NaN gradient of latent_loss for p != 1.)
  row0_outlier: worst relative error of pstd over all shapes, host emulation: 9.0e-7 on `rand`, 7.3e-7 on `far_mean`, 1.5e-5 on
  `row0_outlier`; MI355X: the same three figures.  A row 0 that lies 16 sigma out costs the shifted single pass a factor ~ 16 in accuracy, of the
  ~ 250 its bound allows (err / tol 0.11 there): pstd keeps 16 good bits, and the kernel needed no change."""
import functools
import math

import numpy as np
import torch

from tests.gemm_ref_util import U_BF16, Embedded, assert_bit_equal, assert_elementwise, elementwise_report  # noqa: F401  (re-exported)
from tests.ln_ref_util import bf, cdiv, check, f32  # noqa: F401

E24 = 2.0 ** -24
LEVELS = 6 + 3
LOSS_BLOCKS, SQ_BLOCKS, FLAT_CAP, GS_CHUNKS = 512, 1024, 2048, 8
POW_C, POW_K = 2.1, 2.0
PSTD_EPS = f32(1e-4)
NAN, INF = float("nan"), float("inf")


def seed_of(*key):
    return sum((i + 1) * 1000003 * (sum(map(ord, k)) if isinstance(k, str) else int(k)) for i, k in enumerate(key)) % (2 ** 31)


def gen(*key):
    return torch.Generator().manual_seed(seed_of(*key))


class Case:
    """named tensors + attributes; .to(device) moves the tensors."""

    def __init__(self, label, tensors, **attrs):
        self.label, self.t, self.attrs = label, tensors, attrs
        for k, v in {**attrs, **tensors}.items():
            setattr(self, k, v)

    def to(self, device):
        return Case(self.label, {k: v.to(device) for k, v in self.t.items()}, **self.attrs)


def odd(t):
    """fp32 values with the last bit of the significand set: their product with a momentum has a set bit far below any fp32 rounding
    position, so the float64 sum of fma32() cannot sit on a rounding tie (short of a cancellation by 2^-20)."""
    t = torch.where(t.abs() < 2.0 ** -20, torch.full_like(t, 2.0 ** -20), t)          # no denormals
    return (t.contiguous().view(torch.int32) | 1).view(torch.float32)


def wide(shape, g, lo, hi):
    """+-2^U(lo, hi)."""
    mag = torch.exp2(lo + (hi - lo) * torch.rand(shape, generator=g))
    return mag * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


# ================================================================================================ latent_loss
LOSS_NUMEL = [8, 8 * 255, 8 * 256, 8 * 257, 8 * (512 * 256), 8 * (512 * 256 + 1)]
LOSS_P = [1.0, 2.0, 1.5]
LOSS_VARIANTS = ["rand", "equal", "wide", "nonfinite"]
LOSS_GSCALE = f32(0.37)
LOSS_OLD = f32(1.25)
NONFINITE_PATTERN = [("z", NAN), ("z", INF), ("z", -INF), ("h", NAN), ("h", INF), ("h", -INF), ("both", INF), (None, 0.0)]


@functools.lru_cache(maxsize=None)
def make_loss_case(numel, variant):
    g = gen("loss", numel, variant)
    z = bf(torch.randn(numel, generator=g))
    h = torch.randn(numel, generator=g)
    if variant == "equal":
        i = torch.arange(numel)
        h = torch.where(i % 3 == 0, z.float(), h)                      # d == +0 on a third
        z = torch.where(i % 9 == 0, bf(torch.tensor(-0.0)), z)          # d = -0 - +0 = -0
        h = torch.where(i % 9 == 0, torch.tensor(0.0), h)
        z = torch.where(i % 9 == 3, bf(torch.tensor(0.0)), z)           # d = +0 - -0 = +0
        h = torch.where(i % 9 == 3, torch.tensor(-0.0), h)
    elif variant == "wide":
        h = z.float() - wide((numel,), g, -12.0, 6.0)
    elif variant == "nonfinite":
        z, h = z.clone(), h.clone()
        for base in (0, numel - 8):
            for j, (where, val) in enumerate(NONFINITE_PATTERN):
                if where in ("z", "both"):
                    z[base + j] = val
                if where in ("h", "both"):
                    h[base + j] = val
    return Case(f"numel{numel} {variant}", dict(z=z, h=h), numel=numel, variant=variant, out_scale=f32(1.0 / numel))


def pow_rel(a, q):
    """relative error bound of __powf(a, q) (module docstring); 0 where a == 0 (exp2(-inf) = 0 exactly)."""
    l2 = torch.where(a > 0, torch.log2(a.clamp_min(1e-300)), torch.zeros_like(a))
    return (POW_C * (q * l2).abs() + POW_K) * E24


def loss_depth(numel):
    return 8 * cdiv(numel // 8, LOSS_BLOCKS * 256) + LEVELS + 2 + LEVELS


def loss_reference(case, p, gscale=LOSS_GSCALE, old=None):
    """dict(loss, tol_loss (0-dim), dz, tol_dz [numel]) in float64; non-finite where torch's autograd is (module docstring)."""
    d = case.z.double() - case.h.double()
    a = d.abs()
    if p == 1.0:
        term, terr = a, E24 * a
        dz = torch.where(torch.isnan(d), torch.zeros_like(d), torch.sign(d) * gscale)
        F = torch.zeros_like(a)
    else:
        term = a ** p / p
        terr = (p * E24 + pow_rel(a, p) + E24) * term
        dz = torch.sign(d) * a ** (p - 1.0) * gscale
        dz = torch.where(torch.isnan(d), d, dz)
        F = abs(p - 1.0) * E24 + pow_rel(a, p - 1.0) + E24
    S = term.sum()
    ref = case.out_scale * S
    tol = abs(case.out_scale) * (loss_depth(case.numel) * E24 * S + terr.sum()) + E24 * ref.abs()
    if old is not None:
        ref = ref + old
        tol = tol + E24 * ref.abs()
    return dict(loss=ref, tol_loss=tol, dz=dz, tol_dz=U_BF16 * dz.abs() * (1 + F) + F * dz.abs())


def nonfinite_agrees(out, ref):
    """NaN exactly where the reference is NaN, the same infinity where it is infinite."""
    o = out.double()
    return bool((torch.isnan(o) == torch.isnan(ref)).all()) and bool((o[torch.isinf(ref)] == ref[torch.isinf(ref)]).all()) \
        and bool((torch.isinf(o) == torch.isinf(ref)).all())


def loss_pairs(ref, loss, dz):
    """the (name, out, ref, tol) of check(); the non-finite elements of the reference are compared by nonfinite_agrees() and enter the
    bound as zeros on both sides."""
    fin = torch.isfinite(ref["dz"])
    zero = torch.zeros((), dtype=torch.float64, device=fin.device)
    pairs = []
    if bool(torch.isfinite(ref["loss"])):
        pairs.append(("loss", loss.reshape(1), ref["loss"].reshape(1), ref["tol_loss"].reshape(1)))
    if dz is not None:
        pairs.append(("dz", torch.where(fin, dz.double(), zero), torch.where(fin, ref["dz"], zero), torch.where(fin, ref["tol_dz"], zero)))
    return pairs


def loss_pins_hold(case, ref, p, loss, dz):
    """the sign of a zero gradient, the class of every non-finite one and of the loss."""
    ok = True
    if not bool(torch.isfinite(ref["loss"])):
        ok = ok and ((math.isnan(float(loss)) and math.isnan(float(ref["loss"]))) or float(loss) == float(ref["loss"]))
    if dz is not None:
        ok = ok and nonfinite_agrees(dz, ref["dz"])
        zero = ref["dz"] == 0
        if bool(zero.any()):
            neg = torch.signbit(dz[zero])
            ok = ok and bool((~neg).all() if p == 1.0 else neg.all())
    return ok


# ================================================================================================ token_pstd
PSTD_B = 3
PSTD_SHAPES = [(K, D) for K in (2, 3, 31, 32, 33, 64, 65) for D in (8, 56, 64, 72, 136)]
PSTD_VARIANTS = ["rand", "offset", "const", "row0_outlier", "far_mean"]
PSTD_RUNS = [(True, False), (False, False), (True, True), (False, True)]        # (stats, accumulate)


@functools.lru_cache(maxsize=None)
def make_pstd_case(K, D, variant):
    B, g = PSTD_B, gen("pstd", K, D, variant)
    if variant == "rand":
        z = torch.randn(B, K, D, generator=g)
    elif variant == "offset":
        z = 64.0 + torch.randint(-3, 4, (B, K, D), generator=g).float()
    elif variant == "const":
        z = torch.randn(B, 1, D, generator=g).expand(B, K, D)
    else:
        mu = 24.0 * torch.randn(B, 1, D, generator=g)
        z = mu + torch.randn(B, K, D, generator=g)
        if variant == "row0_outlier":
            z[:, 0] = mu[:, 0] + 16.0
    return Case(f"B{B} K{K} D{D} {variant}", dict(z=bf(z).contiguous(), old=torch.randn(B, D, generator=g)), B=B, K=K, D=D, variant=variant)


def pstd_depth(K):
    return cdiv(K, 32) + 32


def pstd_reference(case):
    z, K = case.z.double(), case.K
    t = z - z[:, :1]
    depth = pstd_depth(K)
    var = z.var(dim=1, unbiased=True)
    if case.variant == "const":
        var = torch.zeros_like(var)
    S1 = t.abs().sum(1)
    x = var + PSTD_EPS
    tv = (depth + 7) * E24 * ((t * t).sum(1) + S1 ** 2 / K) / (K - 1) + E24 * x
    assert float((tv / x).max()) < 0.125, case.label
    s = x.sqrt()
    mean = z.mean(1)
    return dict(pstd=s, tol_pstd=tv / (2 * s) * (1 + tv / x) + E24 * s, mean=mean,
                tol_mean=depth * E24 * S1 / K + E24 * t.sum(1).abs() / K + E24 * mean.abs())


def pstd_pairs(ref, pstd, stats, old=None):
    r, tol = ref["pstd"], ref["tol_pstd"]
    if old is not None:
        r = r + old.double()
        tol = tol + E24 * r.abs()
    pairs = [("pstd", pstd, r, tol)]
    if stats is not None:
        pairs += [("stats0", stats[..., 0], ref["mean"], ref["tol_mean"]), ("stats1", stats[..., 1], ref["pstd"], ref["tol_pstd"])]
    return pairs


def pstd_const_pins_hold(case, pstd, stats):
    """overwriting run of the const variant: pstd == sqrtf(1e-4f), stats == {the constant, sqrtf(1e-4f)}."""
    s = torch.full_like(pstd, float(np.sqrt(np.float32(1e-4))))
    ok = torch.equal(pstd, s)
    if stats is not None:
        ok = ok and torch.equal(stats[..., 0], case.z[:, 0].float()) and torch.equal(stats[..., 1], s)
    return ok


# ================================================================================================ reg_grad, reg_finish
REG_SHAPES = [(1, 2, 8), (2, 5, 72), (3, 33, 520), (174763, 3, 8)]      # the last: B K D / 8 = 2048 * 256 + 1, one thread strides
REG_MASKS = [1, 2, 3]
REG_COEF = f32(0.37)


@functools.lru_cache(maxsize=None)
def make_reg_case(B, K, D, n_masks):
    g = gen("reg", B, K, D, n_masks)
    below = torch.rand(B, D, generator=g) < 0.5
    below.view(-1)[0], below.view(-1)[1] = True, False
    u = torch.rand(B, D, generator=g)
    pstd_sum = n_masks * torch.where(below, 0.25 + 0.74 * u, 1.01 + 0.7 * u)     # both sides of n_masks, none within 1 % (> 1e-3) of it
    assert bool(((pstd_sum - n_masks).abs() > 1e-3).all())
    stats = torch.stack([torch.randn(B, D, generator=g), 0.5 + torch.rand(B, D, generator=g)], dim=-1).contiguous()
    return Case(f"B{B} K{K} D{D} masks{n_masks}", dict(z=bf(torch.randn(B, K, D, generator=g)), dz0=bf(torch.randn(B, K, D, generator=g)),
                                                     pstd_sum=pstd_sum, stats=stats), B=B, K=K, D=D, n_masks=n_masks)


def reg_grad_reference(case):
    active = (case.pstd_sum.double() / case.n_masks < 1.0).double().unsqueeze(1)
    term = REG_COEF * active * (case.z.double() - case.stats[..., 0].double().unsqueeze(1)) / ((case.K - 1) * case.stats[..., 1].double().unsqueeze(1))
    ref = case.dz0.double() - term
    return dict(dz=ref, tol_dz=U_BF16 * ref.abs() + E24 * (6 * term.abs() + 2 * ref.abs()), inactive=(active == 0).expand_as(ref))


FINISH_N = [1, 255, 256, 257, 1031]
FINISH_MASKS = [1, 3]


@functools.lru_cache(maxsize=None)
def make_finish_case(n, n_masks):
    g = gen("finish", n, n_masks)
    pstd = n_masks * 2.0 * torch.rand(n, generator=g)
    pstd[0] = 0.25 * n_masks
    return Case(f"n{n} masks{n_masks}", dict(pstd=pstd), n=n, n_masks=n_masks)


def reg_finish_reference(case):
    x = case.pstd.double() / case.n_masks
    term = (1.0 - x).clamp_min(0.0)
    terr = 2 * E24 * x * (x < 1 + 2.0 ** -20) + E24 * term
    ref = term.sum() / case.n
    return dict(out=ref, tol_out=((cdiv(case.n, 256) + LEVELS) * E24 * term.sum() + terr.sum()) / case.n + E24 * ref.abs())


# ================================================================================================ adamw + ema
ADAM_N = [4, 1020, 1024, 1028, 4 * (2048 * 256 + 3)]
ADAM_BIG = ADAM_N[-1]
ADAM_VARIANTS = ["rand", "zero_grad", "tiny_v"]
HP = dict(lr=f32(1e-3), beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-8))
EMA_MOMENTA = [f32(0.998), f32(0.9)]
# index i: p_bf16 present = i & 1, tgt = i & 2, tgt_bf16 = i & 4
_STEP, _WD, _GS = [1, 7, 100000, 7, 1, 100000, 1, 7], [0.05, 0.0, 0.05, 0.0, 0.0, 0.05, 0.0, 0.05], [1.0, 0.37, 0.37, 1.0, 0.37, 1.0, 1.0, 0.37]
PLAIN_CONFIGS = [dict(kind="plain", nulls=i, step=_STEP[i], wd=f32(_WD[i]), gscale=f32(_GS[i]), ema=EMA_MOMENTA[i % 2]) for i in range(8)]
GSTAT = (16.0, 2.25)                       # sumsq of module 0 and 1: norms 4 and 1.5, times norm_scale 0.5: 2 and 0.75


def _guarded(nulls, sel, clip, t0, wd, gscale, bad=(0.0, 0.0), ema=EMA_MOMENTA[0]):
    return dict(kind="guarded", nulls=nulls, sel=sel, clip=f32(clip), t0=float(t0), wd=f32(wd), gscale=f32(gscale), norm_scale=0.5,
                gstat=(GSTAT[0], bad[0], GSTAT[1], bad[1]), ema=ema)


GUARDED_CONFIGS = [
    _guarded(7, 0, 0.5, 0, 0.05, 1.0),                              # clip below the norm 2: coefficient 0.25; first step
    _guarded(7, 1, 0.5, 6, 0.0, 0.37, ema=EMA_MOMENTA[1]),          # the other module's norm 0.75: coefficient 2/3
    _guarded(6, 0, 3.0, 99999, 0.05, 0.37),                         # clip above the norm: coefficient 1; no p_bf16
    _guarded(3, 1, -1.0, 6, 0.05, 1.0),                             # no clipping (clip < 0); no tgt_bf16
    _guarded(5, 0, 0.0, 0, 0.0, 0.37),                              # no clipping (clip = 0); no tgt: tgt_bf16 stays untouched
    _guarded(7, 0, 0.5, 6, 0.05, 1.0, bad=(1.0, 0.0)),              # skipped through gstat[1] alone
    _guarded(7, 1, 0.5, 6, 0.05, 1.0, bad=(0.0, 2.0), ema=EMA_MOMENTA[1]),   # through gstat[3] alone
    _guarded(5, 0, 0.5, 6, 0.05, 1.0, bad=(1.0, 0.0)),              # skipped without a target: nothing is written at all
    _guarded(3, 1, 0.5, 6, 0.05, 1.0, bad=(0.0, 1.0)),              # skipped, target without a shadow
]
BIG_CONFIGS = [PLAIN_CONFIGS[7], GUARDED_CONFIGS[1], GUARDED_CONFIGS[2], GUARDED_CONFIGS[6]]


def adam_configs(n):
    return BIG_CONFIGS if n == ADAM_BIG else PLAIN_CONFIGS + GUARDED_CONFIGS


def config_label(c):
    if c["kind"] == "plain":
        return f"plain nulls{c['nulls']} step{c['step']} wd{c['wd']:g} gs{c['gscale']:.2f}"
    return f"guarded nulls{c['nulls']} sel{c['sel']} clip{c['clip']:g} t0={c['t0']:g} bad{c['gstat'][1]:g}/{c['gstat'][3]:g}"


@functools.lru_cache(maxsize=None)
def make_adam_case(n, variant):
    g = gen("adam", n, variant)
    p, tgt = odd(torch.randn(n, generator=g)), odd(torch.randn(n, generator=g))     # no rounding tie in the fma emulation: see odd()
    if variant == "rand":
        grad, m, v = torch.randn(n, generator=g), 0.3 * torch.randn(n, generator=g), torch.rand(n, generator=g)
    elif variant == "zero_grad":
        grad, m, v = torch.zeros(n), torch.zeros(n), torch.zeros(n)
    else:                                   # sqrt(v) / bc2 of the order of eps = 1e-8
        grad, m, v = 1e-8 * torch.randn(n, generator=g), 1e-8 * torch.randn(n, generator=g), 1e-16 * torch.rand(n, generator=g)
    return Case(f"n{n} {variant}", dict(p=p, g=grad, m=m, v=v, tgt=tgt), n=n, variant=variant)


def adam_scalars(c):
    """the scalars of one call as float64 values: skip, t (the Adam step), gs, gs_uncapped, G (roundings of g'), bc1, bc2s."""
    s = dict(skip=False, G=1, gs=c["gscale"], gs_uncapped=c["gscale"], coef=1.0)
    if c["kind"] == "plain":
        t = float(c["step"])
    else:
        gst = c["gstat"]
        s["skip"] = (gst[1] + gst[3]) > 0
        t = c["t0"] + (0.0 if s["skip"] else 1.0)
        if c["clip"] > 0:
            raw = c["clip"] / (math.sqrt(gst[2 * c["sel"]]) * c["norm_scale"] + f32(1e-6))
            s.update(coef=min(1.0, raw), gs=c["gscale"] * min(1.0, raw), gs_uncapped=c["gscale"] * raw, G=6)
    s["t"] = t
    s["bc1"] = f32(1.0 - HP["beta1"] ** t)
    s["bc2s"] = f32(math.sqrt(1.0 - HP["beta2"] ** t))
    return s


def adam_reference(case, c):
    """one AdamW step in float64: dict(p, m, v and their tol_)."""
    sc = adam_scalars(c)
    lr, b1, b2, eps, wd = HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], c["wd"]
    p, g, m, v = (case.t[k].double() for k in ("p", "g", "m", "v"))
    G = sc["G"] * E24
    g1 = g * sc["gs"]
    m1 = m + (g1 - m) * (1 - b1)
    tol_m = E24 * m1.abs() + (1 - b1) * (3 * E24 * (g1 - m).abs() + G * g1.abs())
    v1 = v * b2 + (1 - b2) * g1 * g1
    tol_v = E24 * v1 + E24 * v * b2 + (1 - b2) * g1 * g1 * (3 * E24 + 2 * G)
    sq = v1.sqrt() / sc["bc2s"]
    den = sq + eps
    tol_den = sq * (torch.where(v1 > 0, tol_v / (2 * v1.clamp_min(1e-300)), torch.zeros_like(v1)) + 3 * E24) + E24 * den
    step = lr / sc["bc1"]
    upd = step * (m1 / den)
    tol_upd = upd.abs() * (tol_den / den * (1 + 2.0 ** -10) + 4 * E24) + step * tol_m / den
    p1 = p * (1 - lr * wd) - upd
    return dict(p=p1, tol_p=3 * E24 * p.abs() + tol_upd + E24 * p1.abs(), m=m1, tol_m=tol_m, v=v1, tol_v=tol_v)


def one_minus(ema):
    return float(np.float32(1.0) - np.float32(ema))


def ema_reference(tgt0, src, ema):
    """(ref, tol) of tgt = ema tgt0 + fl32(1 - ema) src from the fp32 tensors the kernel read."""
    a, b = ema * tgt0.double(), one_minus(ema) * src.double()
    ref = a + b
    return ref, E24 * (a.abs() + b.abs()) + E24 * ref.abs()


def fma32(a, b, c):
    """(fmaf(a, b, c) as fp32, the float64 sum it was rounded from): a, b, c fp32 tensors or fp32-valued floats."""
    def d(x):
        return x.double() if torch.is_tensor(x) else torch.tensor(x, dtype=torch.float64)
    s = d(a) * d(b) + d(c)
    return s.float(), s


def fma_tie(s):
    """the elements of a float64 sum that sit exactly half way between two fp32 values (normal range): the only ones where rounding
    the float64 sum can differ from a true fma."""
    return (s.contiguous().view(torch.int64) & ((1 << 29) - 1)) == (1 << 28)


def ema_expected(tgt0, src, ema, src_rounded):
    """(the bits ema4<SRC_ROUNDED> must write, the number of rounding ties among them)."""
    om = one_minus(ema)
    if src_rounded:
        out, s = fma32(ema, tgt0, src * om)
    else:
        out, s = fma32(om, src, tgt0 * ema)
    return out, int(fma_tie(s).sum())


EMA_N = [4, 1028, ADAM_BIG]


@functools.lru_cache(maxsize=None)
def make_ema_case(n):
    """tgt, src with odd significands; drawn again (another salt) until, for both momenta, the two product orders give different bits
    somewhere: the inputs have to be able to tell the orders apart (at n = 4 one draw in five cannot)."""
    for salt in range(64):
        g = gen("ema", n, salt)
        tgt, src = odd(torch.randn(n, generator=g)), odd(torch.randn(n, generator=g))
        if all(not torch.equal(ema_expected(tgt, src, m, False)[0], ema_expected(tgt, src, m, True)[0]) for m in EMA_MOMENTA):
            return Case(f"n{n}", dict(tgt=tgt, src=src), n=n, salt=salt)
    raise AssertionError(n)


# ================================================================================================ sqnorm
SQ_N = [0, 4, 4 * (1024 * 256), 4 * (1024 * 256 + 5)]
SQ_OLD = (f32(3.7), 2.0)


@functools.lru_cache(maxsize=None)
def make_sq_case(n):
    x = wide((n,), gen("sq", n), -20.0, 10.0)
    x[-4:] = torch.tensor([1024.0, -1024.0, 512.0, 1024.0])[:min(n, 4)]          # the last float4 weighs enough to be missed
    return Case(f"n{n}", dict(x=x), n=n)


def sq_depth(n):
    return 3 + cdiv(n // 4, SQ_BLOCKS * 256) + LEVELS + 4 + LEVELS


def sq_reference(case, old=None):
    S = (case.x.double() ** 2).sum()
    ref, tol = S, (sq_depth(case.n) + 1) * E24 * S
    if old is not None:
        ref = ref + old
        tol = tol + E24 * ref.abs()
    return ref, tol


def sq_nonfinite_positions(n):
    """name -> element index: in the first float4, in the last, and (where a thread takes a second float4) in the strided trip."""
    pos = {}
    if n >= 4:
        pos = {"first": 1, "last": n - 2}
    if n > 4 * SQ_BLOCKS * 256:
        pos["strided"] = 4 * SQ_BLOCKS * 256 + 6
    return pos


# ================================================================================================ grad_stats_multi
GS_NUMEL = [1, 3, 4, 5, 31, 32, 33, 8 * 4 * 256, 8 * 4 * 256 + 5]


@functools.lru_cache(maxsize=None)
def make_gs_case():
    g = gen("grad_stats")
    desc, off = [], 64
    for n in GS_NUMEL:
        desc.append((off, n))
        off = cdiv(off + n, 64) * 64 + 64                 # a NaN gap of at least 64 elements after every tensor, one of 64 before the first
    live = torch.zeros(off, dtype=torch.bool)
    for o, n in desc:
        live[o:o + n] = True
    nan = torch.full((off,), NAN)
    G = torch.where(live, wide((off,), g, -20.0, 10.0), nan)
    for o, n in desc:
        G[o + n - 1] = 1024.0                             # the last element (the scalar tail's, where there is one) weighs enough to be missed
    M1 = torch.where(live, 0.3 * torch.randn(off, generator=g), nan)
    M2 = torch.where(live, torch.rand(off, generator=g), nan)
    return Case("arena", dict(G=G, M1=M1, M2=M2, desc=torch.tensor(desc, dtype=torch.int64)), offsets=desc)


def gs_chunks(n):
    """[(lo, hi)] of the 8 chunks; hi <= lo for an empty one."""
    per = cdiv(cdiv(n, GS_CHUNKS), 4) * 4
    return [(c * per, min(c * per + per, n)) for c in range(GS_CHUNKS)]


def gs_reference(case, moments):
    """(ref, tol) [n_tensors, 8, 3] float64; empty chunks and absent moments are exactly 0 (tol 0)."""
    T = len(case.offsets)
    ref = torch.zeros(T, GS_CHUNKS, 3, dtype=torch.float64, device=case.G.device)
    tol = torch.zeros_like(ref)
    for t, (off, n) in enumerate(case.offsets):
        for c, (lo, hi) in enumerate(gs_chunks(n)):
            if hi <= lo:
                continue
            depth = 3 + cdiv(cdiv(hi - lo, 4), 256) + 1 + LEVELS + 1
            terms = [case.G[off + lo:off + hi].double() ** 2]
            if moments:
                terms += [case.M1[off + lo:off + hi].double().abs(), case.M2[off + lo:off + hi].double().abs()]
            for k, x in enumerate(terms):
                ref[t, c, k] = x.sum()
                tol[t, c, k] = depth * E24 * x.sum()
    return ref, tol


# ================================================================================================ the AdamW verdict, shared by CPU and GPU
PB_FILL, TB_FILL = 3.0, -5.0          # what the bf16 shadows hold before a call


def adam_check(case, c, out, collect=None):
    """out = dict(p, m, v, tgt fp32; pb, tb bf16; step float | None) after ONE call on the case's tensors (tgt / pb / tb None where
    the config passes no buffer; for tgt = None with a shadow, tb is the untouched shadow).  Bounds through check(); pins bit for bit.
    collect = None: assert; a dict: the reports and collect["pins"] = dict(ok=...) are stored.  Returns the worst err / tol."""
    sc = adam_scalars(c)
    label = f"{case.label} {config_label(c)}"
    pins, worst, ties = [], {}, 0
    has_pb, has_tgt, has_tb = bool(c["nulls"] & 1), bool(c["nulls"] & 2), bool(c["nulls"] & 4)
    if sc["skip"]:
        pins += [("p unchanged", out["p"], case.p), ("m unchanged", out["m"], case.m), ("v unchanged", out["v"], case.v)]
        if has_pb:
            pins.append(("p_bf16 unchanged", out["pb"], torch.full_like(out["pb"], PB_FILL)))
        src, src_rounded = case.p, False
    else:
        ref = adam_reference(case, c)
        worst = check(label, [(k, out[k], ref[k], ref["tol_" + k]) for k in ("p", "m", "v")], collect)
        if has_pb:
            pins.append(("p_bf16 == bf16(p)", out["pb"], bf(out["p"])))
        src, src_rounded = out["p"], True
    if has_tgt:
        r, tol = ema_reference(case.tgt, src, c["ema"])
        worst.update(check(label, [("tgt", out["tgt"], r, tol)], collect))
        expect, ties = ema_expected(case.tgt, src, c["ema"], src_rounded)
        pins.append(("tgt == the fma of its branch", out["tgt"], expect))
        if has_tb:
            pins.append(("tgt_bf16 == bf16(tgt)", out["tb"], bf(out["tgt"])))
    elif has_tb:
        pins.append(("tgt_bf16 untouched without tgt", out["tb"], torch.full_like(out["tb"], TB_FILL)))
    if c["kind"] == "guarded":
        pins.append(("step_dev", torch.tensor([out["step"]]), torch.tensor([sc["t"]])))
    assert ties == 0, f"{label}: {ties} rounding ties in the fma emulation: draw other inputs"
    bad = [name for name, a, b in pins if not torch.equal(a, b)]
    if collect is None:
        for name, a, b in pins:
            assert_bit_equal(a.reshape(1, -1), b.reshape(1, -1), f"{name} {label}")
    else:
        collect["pins"] = dict(ok=not bad, which=bad)
    return worst
