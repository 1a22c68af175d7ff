"""Float64 references, derived per-element bounds, cases and shapes for the LayerNorm family (csrc/layernorm.hip: layernorm_fwd,
ln_rowstats, ln_fold_weights, layernorm_bwd with its column sums through reduce_column of csrc/reduce.hip, target_rows).  Imported by
tests/test_ln_bound_host.py (CPU) and tests/test_layernorm_elementwise_gpu.py; never collected.

Everything is computed in float64 from the kernel's own bf16 / fp32 inputs (eps as the fp32 value the C ABI receives).  u = 2^-8 (half a
bf16 ulp, relative), e = 2^-24 (the fp32 unit roundoff), f = 2^-20 = 16 e.  Per row: m = mean, var the biased variance, r = rstd =
(var + eps)^-1/2, xhat = (x - m) r, a = mean_row |x|.  NaN and inf fail; nothing is excluded.

WHERE f COMES FROM.  A row sum is formed by 64 lanes adding their <= 32 values in turn, then 6 butterfly levels.  The rounding of one add
is at most e times the partial sum it produces; over a lane's chain of n the partial sums add up to at most (n / 2 + 1/2) of the lane's
sum of magnitudes, every butterfly level adds e sum |x| once more, the product with fl(1 / D) two more: (n / 2 + 8.5) e <= 16 e = f for
D <= 1024, 24.5 e at D = 2048 if every one of the 38 roundings errs by its maximum in the same direction.  The forms below keep the
single constant f for every D <= 2048 (roundings of either sign: the fp32 emulation of tests/test_ln_bound_host.py uses less than a
third of it at every shape); they are stated per output, each a sum of the terms the listed operations can contribute.

  mean (fp32)     tol = f a
  rstd (fp32)     tol = f r + r^3 tol_mean^2 / 2
      TIGHTER than f r (1 + r a): the kernels take the variance of the CENTRED values, and sum_j (x_j - m - d)^2 / D = var + d^2
      exactly, so an error d of the mean enters the variance squared.  The looser form admits E[x^2] - mean^2 at power-of-two D on the
      offset rows (var = 4 under mean^2 = 4096: an fp32 rounding of mean^2 moves rstd by 3e-5 relative, the loose form allows 3.1e-5).
      f r: the relative error of the variance (sub, square, sum, 1 / D, + eps: as the sum above, all terms positive) halves in
      rsqrt, plus v_rsq_f32's own ulp.
  rs[:, 0]        = rstd.   rs[:, 1] = -m r: tol = |m| tol_rstd + r tol_mean + tol_mean tol_rstd + e |m r| (the product, rounded once)
  y (bf16)        ref = xhat gamma + beta,  tol = u |ref| + f A,  A = |xhat gamma| + |beta| + r |gamma| a
      r |gamma| a f: the mean's error shifts every element of the row by tol_mean r |gamma|; |xhat gamma| f: rstd's relative error and
      the three fp32 operations; |beta| f: the add.  u |ref|: the one bf16 rounding.
  dx (bf16)       g = dy gamma, c1 = mean_row g, c2 = mean_row (g xhat), ref = r (g - c1 - xhat c2) + dres,
                  tol = u |ref| + f A,  A = |dres| + r (|g| + mean_row |g| + |xhat| mean_row |g xhat|)
      m, r are the fp32 values the kernel is GIVEN (float64 statistics rounded once), exact in the reference: nothing of a forward kernel
      enters.  The three terms of the bracket are the magnitudes whose roundings (and the two row sums' f) the cancellation can expose.
  column sums (fp32: dgamma = sum_rows dy xhat, dbeta = sum_rows dy, dxsum = sum_rows dx BEFORE its bf16 rounding)
                  tol = |alpha| (depth e sum_rows |term| [+ sum_rows f A_dx for dxsum]) [+ e |ref| when accumulating]
      depth = the longest chain of fp32 additions a term passes through (Higham, Accuracy and Stability, 4.2: any summation tree has
      |error| <= depth e sum |x|): col_depth(rows) = ceil(rows_per_workgroup / 4) adds of a wave's accumulator + 4 waves combined in
      LDS + ceil(nb / 8) adds of one of reduce_column's 8 partial lanes + 8 lanes combined.  The first add of each stage is onto a zero
      (exact), which leaves 3 e: the rounding of a term itself (x - m, times r, times dy) and of the product with alpha.  alpha and
      the old value enter the reference exactly; accumulating is one more fp32 add, e |ref|.  A dxsum term is the fp32 dx: within
      f A_dx of the float64 one.
  Wf (bf16)       bit-equal to (W * gamma).to(bfloat16): one fp32 product, one RNE.
  cvec (fp32)     referenced to the float64 sum of the kernel's OWN Wf (its contract: the epilogue's acc - mean * cvec cancels what the
                  matrix pipe summed).  tol = fold_depth(K) e sum_k |Wf|, fold_depth = ceil(K / 256) trips of a lane + 2 adds of the
                  4-element tree inside a trip + 6 butterfly levels.
  bf (fp32)       ref = b + sum_k W beta,  tol = (fold_depth(K) + 2) e (sum_k |W beta| + |b|)         (+ the product, + the add of b)
  h (fp32)        z = xhat gamma + beta of the gathered row (float64), dz = f A_y (y's term without the bf16 part); m2, r2 the float64
                  statistics of z under eps_ln, h = (z - m2) r2:
                  tol = (1 + 4 rho) r2 (dz + mean_row dz + |h| mean_row (|h| dz)) + f (|h| + r2 mean_row |z|)
      the first bracket is the derivative of the second normalisation applied to |dz| (dh_j = r2 (d_j - mean d) - h_j r2 mean (h d)),
      rho = r2 max dz bounds the relative size of the second-order terms (rho < 1/8 is asserted: else the bound would be vacuous);
      the second is the second normalisation's own fp32 error, y's form with gamma = 1, beta = 0.

INPUT VARIANTS (make_rows; drawn on the CPU, seeded by shape).  rand: x = 2 N(0,1) + 0.3, today's distribution.  offset: x = 64 +
integers in [-3, 3]: cancellation in a one-pass variance.  tiny: x = 2^-10 N(0,1), row variance ~ eps: eps decides the result; run at
eps 1e-6 and 1e-5.  const: every row a constant c: var = 0, r = eps^-1/2; c is drawn from the values for which the fp32 mean is c
EXACTLY (k c is exact for k <= 2048, c of <= 2 significant bits; fl(fl(D c) fl(1 / D)) == c is checked in fp32 here), so xhat = 0
and y == bf16(beta) bit for bit, dgamma == 0.  target_rows also: smallgamma, gamma ~ 2^-9 (beta likewise), z has variance ~ 2^-18 and
eps_ln decides; eps_norm != eps_ln both ways round."""
import functools

import numpy as np
import torch

from tests.gemm_ref_util import U_BF16, Embedded, assert_bit_equal, assert_elementwise, elementwise_report  # noqa: F401  (re-exported)

E24 = 2.0 ** -24
F20 = 2.0 ** -20
LN_BWD_MAX_BLOCKS = 1024            # layernorm.hip; the workspace holds 3 D floats for each (asserted against vj_layernorm_bwd_ws_bytes)
FWD_GRID_CAP = 2048                 # workgroups of 4 waves: above 8192 rows a wave takes a second row

D_EDGES = [8, 504, 512, 520, 1024, 1032, 1536, 1544, 2048]          # chunk counts 1..4, each full and ragged; one lane
FWD_SHAPES = [(r, D) for D in D_EDGES for r in (1, 3, 4, 5)] + [(8200, 8)]
BWD_D = [8, 72] + D_EDGES[1:]                                        # 72, 520: D % 64 != 0, one reduction launch per output
BWD_SHAPES = [(r, D) for D in BWD_D for r in (1, 3, 4, 5, 16, 17, 33)] + [(16385, 8), (777, 1280)]
FOLD_SHAPES = [(N, K) for N in (1, 3, 4, 5) for K in (4, 252, 256, 260, 1028)]
TARGET_B, TARGET_N = 2, 7
TARGET_SHAPES = [(K, D) for K in (1, 3, 7) for D in (8, 520, 2048)]
TARGET_IDX = {1: [[6], [0]], 3: [[6, 6, 0], [0, 3, 6]], 7: [[6, 6, 5, 3, 2, 0, 0], [0, 6, 3, 3, 1, 6, 0]]}   # 0, N-1, duplicates, descending
STAT_VARIANTS = [("rand", 1e-6), ("offset", 1e-6), ("tiny", 1e-6), ("tiny", 1e-5), ("const", 1e-6)]
BWD_VARIANTS = [("rand", 1e-6), ("offset", 1e-6), ("tiny", 1e-5), ("const", 1e-6)]
TARGET_VARIANTS = [("rand", 1e-6, 1e-5), ("offset", 1e-6, 1e-5), ("tiny", 1e-6, 1e-5), ("tiny", 1e-5, 1e-6), ("const", 1e-6, 1e-5),
                   ("smallgamma", 1e-6, 1e-5), ("smallgamma", 1e-5, 1e-6)]
# (dxsum, dres, alpha) of the backward runs: both template variants CS, with and without the residual gradient, both alphas
BWD_CONFIGS = [(True, True, 0.5), (False, True, 1.0), (True, False, 1.0), (False, False, 0.5)]
CONST_VALUES = [1.0, -2.0, 0.5, -1.0, 2.0, -0.5, 0.25, 1.5, -0.75]


def bf(x):
    return x.to(torch.bfloat16)


def f32(x):
    return float(np.float32(x))


def cdiv(a, b):
    return -(-a // b)


def n_chunks(D):
    return cdiv(D, 512)


def bwd_grid(rows):
    """(workgroups, rows per workgroup) of layernorm_bwd."""
    nb = min(max(cdiv(rows, 16), 1), LN_BWD_MAX_BLOCKS)
    return nb, cdiv(rows, nb)


def col_depth(rows):
    nb, rows_per = bwd_grid(rows)
    return cdiv(rows_per, 4) + 4 + cdiv(nb, 8) + 8


def fold_depth(K):
    return cdiv(K, 256) + 2 + 6


# ------------------------------------------------------------------------------------------------ cases
def const_values(D):
    """the constants c whose fp32 row mean fl(fl(D c) fl(1 / D)) is c itself (module docstring)."""
    inv = np.float32(1.0) / np.float32(D)
    ok = [c for c in CONST_VALUES if np.float32(np.float32(D * c) * inv) == np.float32(c)]
    assert len(ok) >= 2, (D, ok)
    return ok


def make_rows(rows, D, variant, g):
    if variant in ("rand", "smallgamma"):
        return bf(torch.randn(rows, D, generator=g) * 2 + 0.3)
    if variant == "offset":
        return bf(64.0 + torch.randint(-3, 4, (rows, D), generator=g).float())
    if variant == "tiny":
        return bf(torch.randn(rows, D, generator=g) * 2.0 ** -10)
    if variant == "const":
        vals = torch.tensor(const_values(D))
        return bf(vals[torch.randint(0, len(vals), (rows,), generator=g)][:, None].expand(rows, D).contiguous())
    raise ValueError(variant)


class Case:
    """x, dy, dres [rows, D] bf16; gamma, beta [D] fp32; eps an fp32 value."""

    def __init__(self, rows, D, variant, eps, **t):
        self.rows, self.D, self.variant, self.eps = rows, D, variant, f32(eps)
        self.t = t
        for k, v in t.items():
            setattr(self, k, v)

    def to(self, device):
        return Case(self.rows, self.D, self.variant, self.eps, **{k: v.to(device) for k, v in self.t.items()})

    @property
    def label(self):
        return f"rows{self.rows} D{self.D} {self.variant} eps{self.eps:.0e}"


@functools.lru_cache(maxsize=None)
def make_case(rows, D, variant, eps):
    g = torch.Generator().manual_seed(100003 * rows + 17 * D + sum(map(ord, variant)))
    x = make_rows(rows, D, variant, g)
    return Case(rows, D, variant, eps, x=x, gamma=1 + 0.1 * torch.randn(D, generator=g), beta=0.1 * torch.randn(D, generator=g),
                dy=bf(torch.randn(rows, D, generator=g)), dres=bf(torch.randn(rows, D, generator=g)),
                old=torch.randn(3, D, generator=g))


class FoldCase:
    def __init__(self, N, K, **t):
        self.N, self.K, self.t = N, K, t
        for k, v in t.items():
            setattr(self, k, v)

    def to(self, device):
        return FoldCase(self.N, self.K, **{k: v.to(device) for k, v in self.t.items()})

    label = property(lambda self: f"N{self.N} K{self.K}")


@functools.lru_cache(maxsize=None)
def make_fold_case(N, K):
    g = torch.Generator().manual_seed(7919 * N + K)
    return FoldCase(N, K, W=0.05 * torch.randn(N, K, generator=g), b=0.1 * torch.randn(N, generator=g),
                    gamma=1 + 0.1 * torch.randn(K, generator=g), beta=0.1 * torch.randn(K, generator=g))


class TargetCase:
    """x [B * N, D] bf16, idx [B, K] int64, gamma / beta [D]; eps_norm (first LayerNorm), eps_ln (second)."""

    def __init__(self, K, D, variant, eps_norm, eps_ln, **t):
        self.B, self.N, self.K, self.D, self.variant = TARGET_B, TARGET_N, K, D, variant
        self.eps_norm, self.eps_ln, self.t = f32(eps_norm), f32(eps_ln), t
        for k, v in t.items():
            setattr(self, k, v)

    def to(self, device):
        return TargetCase(self.K, self.D, self.variant, self.eps_norm, self.eps_ln, **{k: v.to(device) for k, v in self.t.items()})

    label = property(lambda self: f"B{self.B} N{self.N} K{self.K} D{self.D} {self.variant} eps {self.eps_norm:.0e}/{self.eps_ln:.0e}")


@functools.lru_cache(maxsize=None)
def make_target_case(K, D, variant, eps_norm, eps_ln):
    g = torch.Generator().manual_seed(31 * K + 17 * D + sum(map(ord, variant)))
    x = make_rows(TARGET_B * TARGET_N, D, variant, g)
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    if variant == "smallgamma":
        gamma, beta = gamma * 2.0 ** -9, beta * 2.0 ** -9
    return TargetCase(K, D, variant, eps_norm, eps_ln, x=x, gamma=gamma, beta=beta, idx=torch.tensor(TARGET_IDX[K], dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ float64 references + bounds
def _stats(x64, eps):
    m = x64.mean(-1, keepdim=True)
    var = ((x64 - m) ** 2).mean(-1, keepdim=True)
    return m, (var + eps) ** -0.5, x64.abs().mean(-1, keepdim=True)


def _normalised(x64, gamma, beta, eps):
    """(z, dz, m, r, a): z = xhat gamma + beta and the fp32 part dz = f A of y's bound."""
    m, r, a = _stats(x64, eps)
    xg = (x64 - m) * r * gamma
    return xg + beta, F20 * (xg.abs() + beta.abs() + r * gamma.abs() * a), m, r, a


def forward_reference(case):
    """dict(y, tol_y [rows, D], mean, rstd, rs0, rs1 and their tol_ [rows]) in float64 on the case's device."""
    z, dz, m, r, a = _normalised(case.x.double(), case.gamma.double(), case.beta.double(), case.eps)
    tol_m = F20 * a
    tol_r = F20 * r + 0.5 * r ** 3 * tol_m ** 2
    ref = dict(y=z, tol_y=U_BF16 * z.abs() + dz, mean=m, tol_mean=tol_m, rstd=r, tol_rstd=tol_r, rs0=r, tol_rs0=tol_r, rs1=-m * r,
               tol_rs1=m.abs() * tol_r + r * tol_m + tol_m * tol_r + E24 * (m * r).abs())
    return {k: (v if k in ("y", "tol_y") else v.squeeze(-1)) for k, v in ref.items()}


def stats_input(case):
    """(mean, rstd) fp32 [rows] a backward is fed with: the float64 statistics rounded once (independent of any forward under test)."""
    m, r, _ = _stats(case.x.double(), case.eps)
    return m.squeeze(-1).float().contiguous(), r.squeeze(-1).float().contiguous()


def backward_reference(case, mean_in, rstd_in, with_dres):
    """dict(dx, A [rows, D]; the column sums dgamma, dbeta, dxsum and S_<name> = sum_rows |term| [D]; FA = sum_rows f A) from the
    statistics the kernel is given.  column_bound() turns it into the reference and bound of one (alpha, old value)."""
    x, dy, gam = case.x.double(), case.dy.double(), case.gamma.double()
    m, r = mean_in.double()[:, None], rstd_in.double()[:, None]
    xh, g = (x - m) * r, dy * gam
    c1, c2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    dres = case.dres.double() if with_dres else torch.zeros_like(x)
    dx = r * (g - c1 - xh * c2) + dres
    A = dres.abs() + r * (g.abs() + g.abs().mean(-1, keepdim=True) + xh.abs() * (g * xh).abs().mean(-1, keepdim=True))
    return dict(dx=dx, A=A, tol_dx=U_BF16 * dx.abs() + F20 * A, dgamma=(dy * xh).sum(0), S_dgamma=(dy * xh).abs().sum(0), dbeta=dy.sum(0),
                S_dbeta=dy.abs().sum(0), dxsum=dx.sum(0), S_dxsum=dx.abs().sum(0), FA=F20 * A.sum(0), depth=col_depth(case.rows))


def column_bound(ref, name, alpha, old=None):
    """(ref, tol) [D] of out = alpha * sum (+ old)."""
    tol = ref["depth"] * E24 * ref["S_" + name] + (ref["FA"] if name == "dxsum" else 0.0)
    out, tol = alpha * ref[name], abs(alpha) * tol
    if old is not None:
        out = out + old.double()
        tol = tol + E24 * out.abs()
    return out, tol


def fold_reference(case, Wf_kernel, with_b):
    """dict(Wf bf16 (the pin), cvec, tol_cvec, bf, tol_bf [N]); cvec from the kernel's own Wf."""
    W, beta = case.W.double(), case.beta.double()
    b = case.b.double() if with_b else torch.zeros(case.N, dtype=torch.float64, device=case.W.device)
    d = fold_depth(case.K)
    return dict(Wf=bf(case.W * case.gamma), cvec=Wf_kernel.double().sum(-1), tol_cvec=d * E24 * Wf_kernel.double().abs().sum(-1),
                bf=b + (W * beta).sum(-1), tol_bf=(d + 2) * E24 * ((W * beta).abs().sum(-1) + b.abs()))


def target_reference(case):
    """dict(h, tol_h [B * K, D]) in float64."""
    rows = (torch.arange(case.B, device=case.idx.device)[:, None] * case.N + case.idx).reshape(-1)
    z, dz, _, _, _ = _normalised(case.x.double()[rows], case.gamma.double(), case.beta.double(), case.eps_norm)
    m2, r2, a2 = _stats(z, case.eps_ln)
    h = (z - m2) * r2
    rho = r2 * dz.amax(-1, keepdim=True)
    assert float(rho.max()) < 0.125, (case.label, float(rho.max()))
    lead = r2 * (dz + dz.mean(-1, keepdim=True) + h.abs() * (h.abs() * dz).mean(-1, keepdim=True))
    return dict(h=h, tol_h=(1 + 4 * rho) * lead + F20 * (h.abs() + r2 * a2))


# ------------------------------------------------------------------------------------------------ the checker
def as2d(t):
    return t.reshape(-1, 1) if t.dim() == 1 else t.reshape(-1, t.shape[-1])


def check(label, pairs, collect=None):
    """every (name, out, ref, tol) through the element-wise checker of tests/gemm_ref_util.py.  collect = None: assert; a dict: the
    reports are stored (planted defects).  Returns the worst err/tol per name."""
    worst = {}
    for name, out, ref, tol in pairs:
        assert bool(torch.isfinite(tol).all()) and bool(torch.isfinite(ref).all()), f"{name} {label}: the bound is vacuous"
        o2, r2, t2 = as2d(out), as2d(ref), as2d(tol)
        if collect is None:
            worst[name] = assert_elementwise(o2, r2, t2, f"{name} {label}")
        else:
            collect[name] = elementwise_report(o2, r2, t2)
            worst[name] = collect[name]["worst"]
    return worst


def forward_pairs(ref, y, mean, rstd):
    return [("y", y, ref["y"], ref["tol_y"]), ("mean", mean, ref["mean"], ref["tol_mean"]), ("rstd", rstd, ref["rstd"], ref["tol_rstd"])]


def rowstats_pairs(ref, rs):
    return [("rs0", rs[:, 0], ref["rs0"], ref["tol_rs0"]), ("rs1", rs[:, 1], ref["rs1"], ref["tol_rs1"])]


def backward_pairs(ref, dx, dgamma, dbeta, dxsum, alpha, old=None):
    """old: None (overwrite) or the [3, D] values the outputs held before."""
    pairs = [("dx", dx, ref["dx"], ref["tol_dx"])]
    for i, (name, out) in enumerate((("dgamma", dgamma), ("dbeta", dbeta), ("dxsum", dxsum))):
        if out is not None:
            pairs.append((name, out) + column_bound(ref, name, alpha, None if old is None else old[i]))
    return pairs


def one_ulp_apart(ref, dx_a, dx_b):
    """dx of the two template variants (compiled separately, fp contraction may differ): each within its bound of the same reference,
    so apart by at most one bf16 ulp of the larger (2^-7 relative) plus twice the fp32 term."""
    a, b = dx_a.double(), dx_b.double()
    return bool(((a - b).abs() <= 2.0 ** -7 * torch.maximum(a.abs(), b.abs()) + 2 * F20 * ref["A"]).all())
