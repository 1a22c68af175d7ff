"""CPU: the per-element LayerNorm bounds of tests/ln_ref_util.py admit correct arithmetic and reject planted defects.

A plain torch fp32 emulation of csrc/layernorm.hip in the kernels' own order -- lane l owns columns l*8 + i*512 .. +7 and adds them in
turn, the xor butterfly over the 64 lanes, the mean first and the variance of the centred values second, one bf16 rounding of every
stored element, the column sums per wave (rows r, r + 4, ...), per workgroup (wave 0 + 1 + 2 + 3) and through reduce_column's 8 partial
lanes -- has to satisfy every bound and every pin on every input variant of every shape tests/test_layernorm_elementwise_gpu.py runs the
kernels at.  The same emulation with ONE planted defect has to violate a bound or a pin on at least one variant of every shape where the
defect exists; the test prints which variant rejected it."""
import numpy as np
import pytest
import torch

from tests import ln_ref_util as L
from tests.ln_ref_util import bf

LANE = torch.arange(64)


# ------------------------------------------------------------------------------------------------ the emulation
def lanes(t, D):
    """[R, D] fp32 -> [R, chunks, 64, 8] (zero-padded past D) and the mask of the live chunks [chunks, 64, 1]."""
    nch = L.n_chunks(D)
    p = torch.zeros(t.shape[0], nch * 512, dtype=torch.float32)
    p[:, :D] = t
    live = (torch.arange(nch * 512) < D).view(nch, 64, 8)[:, :, :1]
    return p.view(-1, nch, 64, 8), live


def wave_sum(s):
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, LANE ^ o]
    return s[:, 0]


def row_sum(v4):
    """per-lane sequential sum over its chunks, then the butterfly: [R]."""
    s = torch.zeros(v4.shape[0], 64)
    for i in range(v4.shape[1]):
        for j in range(8):
            s = s + v4[:, i, :, j]
    return wave_sum(s)


def emu_stats(x, D, eps, defect=None):
    """(mean, rstd) fp32 [R] of the fp32 rows x [R, D]: ln_row_mean / ln_row_rstd."""
    v4, live = lanes(x, D)
    invD = torch.tensor(np.float32(1.0) / np.float32(D))
    if defect == "skip_last_chunk":                      # the last live 8-column chunk of the row (columns D - 8 ..) left out of both sums
        live = live & (torch.arange(v4.shape[1] * 512) < D - 8).view(-1, 64, 8)[:, :, :1]
        v4 = torch.where(live, v4, torch.zeros(()))
    mean = row_sum(v4) * invD
    if defect == "one_pass":
        var = row_sum(v4 * v4) * invD - mean * mean
    else:
        d = torch.where(live, v4 - mean[:, None, None, None], torch.zeros(()))
        q = row_sum(d * d)
        var = q * (torch.tensor(np.float32(1.0) / np.float32(D - 1)) if defect == "unbiased" else invD)
    eps = torch.tensor(np.float32(0.0 if defect == "no_eps" else eps))
    return mean, torch.rsqrt(var + eps)


def prev_chunk(p, D):
    """gamma / beta as lane 0 sees them when its last chunk is read from chunk i - 1 (the planted defect)."""
    c0 = (L.n_chunks(D) - 1) * 512
    p = p.clone()
    p[c0:c0 + 8] = p[c0 - 512:c0 - 504]
    return p


def emu_forward(case, defect=None):
    x = case.x.float()
    mean, rstd = emu_stats(x, case.D, case.eps, defect)
    gamma, beta = (prev_chunk(p, case.D) for p in (case.gamma, case.beta)) if defect == "param_prev_chunk" else (case.gamma, case.beta)
    return bf((x - mean[:, None]) * rstd[:, None] * gamma + beta), mean, rstd


def emu_rowstats(case, defect=None):
    mean, rstd = emu_stats(case.x.float(), case.D, case.eps, defect)
    return torch.stack([rstd, -mean * rstd], 1)


def seq_sum(t, stride):
    """[n, ...] -> [stride, ...]: slot k adds t[k], t[k + stride], ... in turn."""
    n = t.shape[0]
    p = torch.zeros(L.cdiv(n, stride) * stride, *t.shape[1:])
    p[:n] = t
    p = p.view(-1, stride, *t.shape[1:])
    s = torch.zeros_like(p[0])
    for k in range(p.shape[0]):
        s = s + p[k]
    return s


def in_turn(s):
    t = s[0]
    for k in range(1, s.shape[0]):
        t = t + s[k]
    return t


def emu_colsum(terms, alpha, old, defect=None):
    """alpha * column sums of terms [rows, D] (+ old) in the kernels' order: wave, workgroup, reduce_column."""
    rows, D = terms.shape
    nb, rows_per = L.bwd_grid(rows)
    terms = terms.clone()
    if defect in ("drop_last_row", "twice_last_row"):
        for k in range(nb):
            last = min((k + 1) * rows_per, rows) - 1
            if last >= k * rows_per:
                terms[last] *= 0.0 if defect == "drop_last_row" else 2.0
    p = torch.zeros(nb * rows_per, D)
    p[:rows] = terms
    part = in_turn(seq_sum(p.view(nb, rows_per, D).transpose(0, 1), 4))                 # wave w: rows w, w + 4, ... -> [nb, D]
    t = in_turn(seq_sum(part, 8)) * torch.tensor(np.float32(alpha))
    if old is not None:
        t = t + old
    elif defect == "read_old":
        t = t + 0.0 * torch.full_like(t, float("nan"))          # beta_acc * the NaN the output held
    return t


def emu_backward(case, mean_in, rstd_in, cs, with_dres, alpha, old=None, defect=None):
    """(dx bf16, dgamma, dbeta, dxsum | None); old: [3, D] to accumulate onto, None to overwrite."""
    D = case.D
    x, dy = case.x.float(), case.dy.float()
    gamma = prev_chunk(case.gamma, D) if defect == "param_prev_chunk" else case.gamma
    dres = case.dres.float() if with_dres else torch.zeros_like(x)
    mean, rstd = mean_in.clone(), rstd_in.clone()
    if defect == "dres_row4":
        dres = dres.clone()
        dres[0] = dres[4]
    if defect == "stats_row4":
        mean[0], rstd[0] = mean[4], rstd[4]
    mean, rstd = mean[:, None], rstd[:, None]
    xh, g = (x - mean) * rstd, dy * gamma
    invD = torch.tensor(np.float32(1.0) / np.float32(D))
    c1 = (row_sum(lanes(g, D)[0]) * invD)[:, None]
    c2 = (row_sum(lanes(g * xh, D)[0]) * invD)[:, None]
    o = dres + rstd * (g - c1 - xh * c2)
    dx = bf(o * alpha) if defect == "alpha_on_dx" else bf(o)
    od = (None, None, None) if old is None else old
    cdef = defect if defect in ("drop_last_row", "twice_last_row", "read_old") else None
    dgamma = emu_colsum(dy * xh, alpha, od[0], cdef)
    dbeta = emu_colsum(dy, alpha, od[1], "read_old" if cdef == "read_old" else None)
    dxsum = emu_colsum(dx.float() if defect == "dxsum_rounded" else o, alpha, od[2]) if cs else None
    return dx, dgamma, dbeta, dxsum


def emu_fold(case, with_b, defect=None):
    """(Wf bf16, cvec, bf): lane l takes 4 columns at l*4 + 256 t, sums them as (a + b) + (c + d), adds trip after trip; butterfly."""
    N, K = case.W.shape
    prod = case.W * case.gamma
    Wf = bf(prod)

    def lane_sum(t):
        p = torch.zeros(N, L.cdiv(K, 256) * 256)
        p[:, :K] = t
        p = p.view(N, -1, 64, 4)
        s = torch.zeros(N, 64)
        for k in range(p.shape[1]):
            s = s + ((p[:, k, :, 0] + p[:, k, :, 1]) + (p[:, k, :, 2] + p[:, k, :, 3]))
        return wave_sum(s)
    cvec = lane_sum(prod if defect == "cvec_unrounded" else Wf.float())
    sb = lane_sum(case.W * case.beta)
    return Wf, cvec, sb + case.b if (with_b and defect != "bf_without_b") else sb


def emu_target(case, defect=None):
    """h [B * K, D] fp32: gather, LayerNorm(gamma, beta, eps_norm), LayerNorm(eps_ln)."""
    B, N, K, D = case.B, case.N, case.K, case.D
    r = torch.arange(B * K)
    idx = case.idx.reshape(-1)
    if defect == "idx_prev_row":
        idx = torch.cat([idx[:1], idx[:-1]])
    rows = (r // K) * (K if defect == "batch_stride_K" else N) + idx
    e1, e2 = (case.eps_ln, case.eps_norm) if defect == "eps_swapped" else (case.eps_norm, case.eps_ln)
    x = case.x.float()[rows]
    mean, rstd = emu_stats(x, D, e1, defect)
    z = (x - mean[:, None]) * rstd[:, None] * case.gamma + case.beta
    mean, rstd = emu_stats(z, D, e2, defect)
    return (z - mean[:, None]) * rstd[:, None]


# ------------------------------------------------------------------------------------------------ pins
def const_pins_forward(case, y):
    return torch.equal(y, bf(case.beta).expand_as(y))


def _rejected(rep):
    return not all(r["ok"] for r in rep.values())


def _summary(kind, label, seen):
    line = f"defects {kind} {label}: " + " ".join(f"{d}[{','.join(v) or 'MISSED'}]" for d, v in seen.items())
    print(line)
    missed = [d for d, v in seen.items() if not v]
    assert not missed, f"planted defects inside the bound on every input variant: {missed}\n{line}"


# ------------------------------------------------------------------------------------------------ forward + rowstats
STAT_DEFECTS = ["no_eps", "one_pass", "unbiased", "skip_last_chunk", "param_prev_chunk"]


def stat_defect_exists(defect, rows, D):
    if defect == "one_pass":
        return D > 8        # 8 bf16 values of one binade: x^2, their sum, the mean and its square are all exact in fp32 -- no defect to see
    if defect == "skip_last_chunk":
        return D % 512 != 0
    if defect == "param_prev_chunk":
        return D > 512
    return True


@pytest.mark.parametrize("rows,D", L.FWD_SHAPES)
def test_forward_and_rowstats_emulation_within_bounds_and_defects_rejected(rows, D):
    seen = {d: [] for d in STAT_DEFECTS if stat_defect_exists(d, rows, D)}
    for variant, eps in L.STAT_VARIANTS:
        case = L.make_case(rows, D, variant, eps)
        ref = L.forward_reference(case)
        y, mean, rstd = emu_forward(case)
        rs = emu_rowstats(case)
        w = L.check(case.label, L.forward_pairs(ref, y, mean, rstd) + L.rowstats_pairs(ref, rs))
        if variant == "const":
            assert const_pins_forward(case, y), case.label
        print(f"emulation {case.label}: worst err/tol " + " ".join(f"{n} {x:.2f}" for n, x in w.items()))
        for defect, hits in seen.items():
            if not hits:
                rep = {}
                y, mean, rstd = emu_forward(case, defect)
                L.check(case.label, L.forward_pairs(ref, y, mean, rstd) + L.rowstats_pairs(ref, emu_rowstats(case, defect)), collect=rep)
                pin = variant == "const" and not const_pins_forward(case, y)
                if _rejected(rep) or pin:
                    hits.append(f"{variant}@{eps:g}" + ("" if _rejected(rep) else "(pin)"))
    _summary("forward", f"rows{rows} D{D}", seen)


# ------------------------------------------------------------------------------------------------ backward
BWD_DEFECTS = ["param_prev_chunk", "dres_row4", "stats_row4", "drop_last_row", "twice_last_row", "dxsum_rounded", "read_old", "alpha_on_dx"]


def bwd_defect_exists(defect, rows, D):
    if defect == "param_prev_chunk":
        return D > 512
    if defect in ("dres_row4", "stats_row4"):
        return rows >= 5
    return True


def bwd_defect_config(defect):
    """the run a defect shows in: (dxsum, dres, alpha)."""
    return L.BWD_CONFIGS[0] if defect in ("dres_row4", "dxsum_rounded", "alpha_on_dx") else L.BWD_CONFIGS[2]


@pytest.mark.parametrize("rows,D", L.BWD_SHAPES)
def test_backward_emulation_within_bounds_and_defects_rejected(rows, D):
    seen = {d: [] for d in BWD_DEFECTS if bwd_defect_exists(d, rows, D)}
    for variant, eps in L.BWD_VARIANTS:
        case = L.make_case(rows, D, variant, eps)
        mean_in, rstd_in = L.stats_input(case)
        refs, worst = {}, {}
        for cs, with_dres, alpha in L.BWD_CONFIGS:
            ref = refs.setdefault(with_dres, L.backward_reference(case, mean_in, rstd_in, with_dres))
            out = emu_backward(case, mean_in, rstd_in, cs, with_dres, alpha)
            w = L.check(case.label, L.backward_pairs(ref, *out, alpha))
            alpha2 = 1.5 - alpha                                          # the accumulating run takes the other alpha, as on the GPU
            acc = emu_backward(case, mean_in, rstd_in, cs, with_dres, alpha2, old=case.old)
            w2 = L.check(case.label + " accumulate", L.backward_pairs(ref, *acc, alpha2, old=case.old))
            assert torch.equal(acc[0], out[0])
            for k in w:
                worst[k] = max(worst.get(k, 0.0), w[k], w2[k])
            if variant == "const":
                assert not bool(out[1].any()) and torch.equal(acc[1], case.old[0]), f"dgamma != 0 {case.label}"
        print(f"emulation {case.label}: worst err/tol " + " ".join(f"{n} {x:.2f}" for n, x in worst.items()))
        for defect, hits in seen.items():
            if not hits:
                cs, with_dres, alpha = bwd_defect_config(defect)
                rep = {}
                out = emu_backward(case, mean_in, rstd_in, cs, with_dres, alpha, defect=defect)
                L.check(case.label, L.backward_pairs(refs[with_dres], *out, alpha), collect=rep)
                pin = variant == "const" and bool(out[1].any())
                if _rejected(rep) or pin:
                    hits.append(variant + ("" if _rejected(rep) else "(pin)"))
    if rows > 1024 and not seen["dxsum_rounded"]:
        # the issue asks for this rejection up to 1024 rows: above, the sum of the roundings (~ sqrt(rows) 2^-9 |dx|) sinks under the
        # summation term of the bound (~ rows / 8 e sum |dx|)
        print(f"dxsum_rounded NOT rejected at rows{rows} D{D} (more than 1024 rows)")
        seen["dxsum_rounded"].append("not required above 1024 rows")
    _summary("backward", f"rows{rows} D{D}", seen)


# ------------------------------------------------------------------------------------------------ ln_fold_weights
@pytest.mark.parametrize("N,K", L.FOLD_SHAPES)
def test_fold_weights_emulation_within_bounds_and_defects_rejected(N, K):
    case = L.make_fold_case(N, K)
    seen = {"cvec_unrounded": [], "bf_without_b": []}
    for with_b in (True, False):
        Wf, cvec, bfv = emu_fold(case, with_b)
        ref = L.fold_reference(case, Wf, with_b)
        L.assert_bit_equal(Wf, ref["Wf"], f"Wf {case.label}")
        w = L.check(case.label, [("cvec", cvec, ref["cvec"], ref["tol_cvec"]), ("bf", bfv, ref["bf"], ref["tol_bf"])])
        print(f"emulation {case.label} b={with_b}: worst err/tol " + " ".join(f"{n} {x:.2f}" for n, x in w.items()))
        for defect, hits in seen.items():
            if not hits and (with_b or defect != "bf_without_b"):
                rep = {}
                _, c2, b2 = emu_fold(case, with_b, defect)
                L.check(case.label, [("cvec", c2, ref["cvec"], ref["tol_cvec"]), ("bf", b2, ref["bf"], ref["tol_bf"])], collect=rep)
                if _rejected(rep):
                    hits.append("b" if with_b else "no b")
    _summary("fold", case.label, seen)


# ------------------------------------------------------------------------------------------------ target_rows
# (no one-pass variance here: the second normalisation divides a relative error of the first rstd out again, h cannot show it; the
#  ln_row_rstd that target_rows shares is held by rstd of layernorm_fwd and ln_rowstats)
TARGET_DEFECTS = ["no_eps", "eps_swapped", "unbiased", "skip_last_chunk", "batch_stride_K", "idx_prev_row"]


def target_defect_exists(defect, K, D):
    if defect == "batch_stride_K":
        return K != L.TARGET_N
    return stat_defect_exists(defect, L.TARGET_B * K, D)


@pytest.mark.parametrize("K,D", L.TARGET_SHAPES)
def test_target_rows_emulation_within_bounds_and_defects_rejected(K, D):
    seen = {d: [] for d in TARGET_DEFECTS if target_defect_exists(d, K, D)}
    for variant, e1, e2 in L.TARGET_VARIANTS:
        case = L.make_target_case(K, D, variant, e1, e2)
        ref = L.target_reference(case)
        w = L.check(case.label, [("h", emu_target(case), ref["h"], ref["tol_h"])])
        print(f"emulation {case.label}: worst err/tol h {w['h']:.2f}")
        for defect, hits in seen.items():
            if not hits:
                rep = {}
                L.check(case.label, [("h", emu_target(case, defect), ref["h"], ref["tol_h"])], collect=rep)
                if _rejected(rep):
                    hits.append(f"{variant}@{e1:g}/{e2:g}")
    _summary("target_rows", f"K{K} D{D}", seen)


def test_depths_and_grids():
    """the numbers the column-sum bounds rest on, spelled out."""
    assert L.bwd_grid(1) == (1, 1) and L.bwd_grid(16) == (1, 16) and L.bwd_grid(17) == (2, 9) and L.bwd_grid(33) == (3, 11)
    assert L.bwd_grid(16385) == (1024, 17) and 963 * 17 < 16385 <= 964 * 17          # workgroups 964 .. 1023 have no row
    assert L.col_depth(1) == 1 + 4 + 1 + 8 and L.col_depth(777) == 4 + 4 + 7 + 8 and L.col_depth(16385) == 5 + 4 + 128 + 8
    assert L.fold_depth(4) == 9 and L.fold_depth(1028) == 5 + 8
    for D in L.D_EDGES + [72]:
        assert len(L.const_values(D)) >= 2
