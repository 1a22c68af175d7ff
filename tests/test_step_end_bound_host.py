"""CPU: the per-element bounds and pins of tests/step_end_ref_util.py admit correct arithmetic and reject planted defects.

A plain torch / numpy fp32 emulation of csrc/loss.hip and csrc/optim.hip in the kernels' own order -- a thread's terms added in turn
(eight per chunk in latent_loss, one float4 as ((x + y) + z) + w), trip after trip of the grid stride, the xor butterfly over the 64
lanes, wave 0 + 1 + 2 + 3, the finish kernels' second stage; token_pstd's 32 row lanes and the 32 adds in turn; AdamW operation by
operation with the scalars formed in fp32 as the kernel forms them; the EMA with the product the source rounds -- has to satisfy every
bound and every pin on every input variant of every shape tests/test_step_end_elementwise_gpu.py runs the kernels at.  The same
emulation with ONE planted defect has to violate a bound or a pin on at least one variant of every shape where the defect exists; the
test prints which variant rejected it.  The fma emulation's no-tie condition is asserted on the seeded inputs."""
import numpy as np
import pytest
import torch

from tests import step_end_ref_util as S
from tests.step_end_ref_util import bf

LANE = torch.arange(64)
F = np.float32


def t32(x):
    return torch.tensor(x, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ shared pieces
def block_sum(acc):
    """[..., 256] per-thread values -> [...]: block4_stage + block4_total."""
    w = acc.reshape(*acc.shape[:-1], 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., LANE ^ o]
    w = w[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def seq_sum(t, stride):
    """[n, ...] -> [stride, ...]: slot k adds t[k], t[k + stride], ... in turn, starting from 0."""
    n = t.shape[0]
    p = torch.zeros(max(S.cdiv(n, stride), 1) * stride, *t.shape[1:], dtype=t.dtype)
    p[:n] = t
    p = p.view(-1, stride, *t.shape[1:])
    s = torch.zeros_like(p[0])
    for k in range(p.shape[0]):
        s = s + p[k]
    return s


def in_turn(s):
    t = torch.zeros_like(s[0])
    for k in range(s.shape[0]):
        t = t + s[k]
    return t


def sum4(v):
    return ((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3]


def _rejected(rep):
    return not all(r["ok"] for r in rep.values())


def _summary(kind, label, seen):
    line = f"defects {kind} {label}: " + " ".join(f"{d}[{','.join(v) or 'MISSED'}]" for d, v in seen.items())
    print(line)
    missed = [d for d, v in seen.items() if not v]
    assert not missed, f"planted defects inside every bound and pin on every input variant: {missed}\n{line}"


def _fmt(w):
    return " ".join(f"{n} {x:.2f}" for n, x in w.items())


# ------------------------------------------------------------------------------------------------ latent_loss
def fast_pow(a, q):
    return torch.exp2(t32(q) * torch.log2(a))


def emu_loss(case, p, gscale, old, defect=None):
    """(loss 0-dim, dz bf16): latent_loss_kernel + scalar_finish_kernel."""
    z, h, gs = case.z.float(), case.h, t32(gscale)
    d = z - h
    a = d.abs()
    zero = torch.zeros(())
    if p == 1.0:
        term = a
        g = torch.where(d > 0, gs, torch.where(d < 0, -gs, -gs if defect == "sign0_neg" else zero))
    else:
        term = fast_pow(a, p) if defect == "no_div_p" else fast_pow(a, p) / t32(p)
        m = torch.where(a > 0, fast_pow(a, p if defect == "pow_p" else p - 1.0), zero)
        g = torch.where(d > 0, m * gs, torch.where((d <= 0) | (defect == "nan_dropped"), -m * gs, d))
    if defect == "skip_last_chunk":
        term = term.clone()
        term[-8:] = 0.0
    acc = torch.zeros(S.LOSS_BLOCKS * 256)
    terms = seq_sum_chunks(term.view(-1, 8), S.LOSS_BLOCKS * 256)
    for trip in terms:
        for j in range(8):
            acc = acc + trip[:, j]
    part = block_sum(acc.view(S.LOSS_BLOCKS, 256))
    v = block_sum(part[:256] + part[256:]) * t32(case.out_scale)          # 0 + part[i] is exact: two adds per thread, one rounded
    if old is not None and defect != "no_accumulate":
        v = t32(old) + v
    return v, bf(g)


def seq_sum_chunks(t, stride):
    """[n, 8] -> [trips, stride, 8], zero-padded: the chunk a thread takes in each trip."""
    n = t.shape[0]
    p = torch.zeros(S.cdiv(n, stride) * stride, 8)
    p[:n] = t
    return p.view(-1, stride, 8)


LOSS_DEFECTS = ["no_div_p", "skip_last_chunk", "sign0_neg", "no_accumulate", "pow_p", "nan_dropped"]


def loss_defect_exists(defect, p):
    return {"no_div_p": p != 1.0, "pow_p": p != 1.0, "nan_dropped": p != 1.0, "sign0_neg": p == 1.0}.get(defect, True)


@pytest.mark.parametrize("p", S.LOSS_P)
@pytest.mark.parametrize("numel", S.LOSS_NUMEL)
def test_latent_loss_emulation_within_bounds_and_defects_rejected(numel, p):
    seen = {d: [] for d in LOSS_DEFECTS if loss_defect_exists(d, p)}
    for variant in S.LOSS_VARIANTS:
        case = S.make_loss_case(numel, variant)
        worst = {}
        for old in (None, S.LOSS_OLD):
            ref = S.loss_reference(case, p, old=old)
            loss, dz = emu_loss(case, p, S.LOSS_GSCALE, old)
            w = S.check(case.label, S.loss_pairs(ref, loss, dz))
            assert S.loss_pins_hold(case, ref, p, loss, dz), f"pins {case.label} p={p}"
            worst.update({k: max(worst.get(k, 0.0), x) for k, x in w.items()})
            for defect, hits in seen.items():
                if not hits and (old is not None or defect != "no_accumulate"):
                    rep = {}
                    l2, dz2 = emu_loss(case, p, S.LOSS_GSCALE, old, defect)
                    S.check(case.label, S.loss_pairs(ref, l2, dz2), collect=rep)
                    pin = not S.loss_pins_hold(case, ref, p, l2, dz2)
                    if _rejected(rep) or pin:
                        hits.append(variant + ("" if _rejected(rep) else "(pin)"))
        print(f"emulation latent_loss {case.label} p={p}: worst err/tol {_fmt(worst)}")
    _summary("latent_loss", f"numel{numel} p={p}", seen)


def test_latent_loss_nonfinite_follows_torch_autograd():
    """the evidence the non-finite contract rests on: autograd of the reference expression mean(|z - h|^p) / p, element for element
    against loss_reference (finiteness and sign) and the emulation of the kernel."""
    case = S.make_loss_case(8, "nonfinite")
    for p in S.LOSS_P:
        z = case.z.float().requires_grad_(True)
        (torch.mean(torch.abs(z - case.h) ** p) / p).backward()
        grad = z.grad.double() * case.numel
        ref = S.loss_reference(case, p, gscale=1.0)
        assert S.nonfinite_agrees(grad, ref["dz"]), (p, grad, ref["dz"])
        fin = torch.isfinite(grad)
        assert torch.equal(torch.sign(grad[fin]), torch.sign(ref["dz"][fin]))
        loss, dz = emu_loss(case, p, 1.0, None)
        assert S.nonfinite_agrees(dz, ref["dz"]) and bool(torch.isnan(loss))
        nan_d = torch.isnan(case.z.float() - case.h)
        assert bool(nan_d.any()) and bool((grad[nan_d] == 0).all() if p == 1.0 else torch.isnan(grad[nan_d]).all())


# ------------------------------------------------------------------------------------------------ token_pstd
def emu_pstd(case, old=None, defect=None):
    """(pstd [B, D], stats [B, D, 2]): token_pstd_kernel."""
    z, K = case.z.float().permute(1, 0, 2), case.K                        # [K, B, D]
    sh = torch.zeros_like(z[0]) if defect == "one_pass" else z[0]
    t = z - sh
    if defect == "drop_rows_ge32":
        t = t[:32]
    ss, qq = in_turn(seq_sum(t, 32)), in_turn(seq_sum(t * t, 32))
    var = (qq - ss * ss / t32(float(K))) / t32(float(K if defect == "biased" else K - 1))
    v = torch.sqrt(var.clamp_min(0.0) + (0.0 if defect == "no_eps" else t32(1e-4)))
    mean = ss / t32(float(K)) if defect == "mean_no_shift" else sh + ss / t32(float(K))
    return (v if old is None else old + v), torch.stack([mean, v], -1)


PSTD_DEFECTS = ["biased", "no_eps", "drop_rows_ge32", "one_pass", "mean_no_shift"]


def pstd_defect_exists(defect, K):
    if defect == "drop_rows_ge32":
        return K > 32
    if defect == "one_pass":
        return K >= 3           # K = 2: every z^2, their sum, ss * ss and its half are exact in fp32 (bf16 inputs): nothing to show
    return True


@pytest.mark.parametrize("K,D", S.PSTD_SHAPES)
def test_token_pstd_emulation_within_bounds_and_defects_rejected(K, D):
    seen = {d: [] for d in PSTD_DEFECTS if pstd_defect_exists(d, K)}
    for variant in S.PSTD_VARIANTS:
        case = S.make_pstd_case(K, D, variant)
        ref = S.pstd_reference(case)
        worst = {}
        for with_stats, acc in S.PSTD_RUNS:
            old = case.old if acc else None
            pstd, stats = emu_pstd(case, old)
            w = S.check(case.label, S.pstd_pairs(ref, pstd, stats if with_stats else None, old))
            worst.update({k: max(worst.get(k, 0.0), x) for k, x in w.items()})
        pstd, stats = emu_pstd(case)
        if variant == "const":
            assert S.pstd_const_pins_hold(case, pstd, stats), case.label
        rel = float(((pstd.double() - ref["pstd"]).abs() / ref["pstd"]).max())
        print(f"emulation token_pstd {case.label}: worst err/tol {_fmt(worst)}; worst relative error of pstd {rel:.2e}")
        for defect, hits in seen.items():
            if not hits:
                rep = {}
                p2, s2 = emu_pstd(case, None, defect)
                S.check(case.label, S.pstd_pairs(ref, p2, s2), collect=rep)
                pin = variant == "const" and not S.pstd_const_pins_hold(case, p2, s2)
                if _rejected(rep) or pin:
                    hits.append(variant + ("" if _rejected(rep) else "(pin)"))
    _summary("token_pstd", f"K{K} D{D}", seen)


# ------------------------------------------------------------------------------------------------ reg_grad, reg_finish
def emu_reg_grad(case, defect=None):
    B, K, D = case.B, case.K, case.D
    r = torch.arange(B * K)
    b = r // (K + 1) if defect == "wrong_row_stride" else r // K
    inv = t32(float(F(1.0) / F(case.n_masks)))
    active = torch.ones(B, D) if defect == "threshold_ignored" else (case.pstd_sum * inv < 1.0).float()
    z, gv = case.z.float().view(B * K, D), case.dz0.float().view(B * K, D)
    coef = t32(-S.REG_COEF if defect == "sign_flipped" else S.REG_COEF)
    den = t32(float(K if defect == "K_for_Km1" else K - 1)) * case.stats[..., 1][b]
    return bf(gv - coef * active[b] * (z - case.stats[..., 0][b]) / den).view(B, K, D)


REG_DEFECTS = ["K_for_Km1", "threshold_ignored", "wrong_row_stride", "sign_flipped"]


@pytest.mark.parametrize("B,K,D", S.REG_SHAPES)
def test_reg_grad_emulation_within_bounds_and_defects_rejected(B, K, D):
    seen = {d: [] for d in REG_DEFECTS if B > 1 or d != "wrong_row_stride"}
    for n_masks in S.REG_MASKS:
        case = S.make_reg_case(B, K, D, n_masks)
        ref = S.reg_grad_reference(case)
        dz = emu_reg_grad(case)
        w = S.check(case.label, [("dz", dz, ref["dz"], ref["tol_dz"])])
        off = ref["inactive"]
        assert bool(off.any()) and not bool(off.all()) and torch.equal(dz[off], case.dz0[off])
        print(f"emulation reg_grad {case.label}: worst err/tol {_fmt(w)}")
        for defect, hits in seen.items():
            if not hits:
                rep = {}
                d2 = emu_reg_grad(case, defect)
                S.check(case.label, [("dz", d2, ref["dz"], ref["tol_dz"])], collect=rep)
                pin = not torch.equal(d2[off], case.dz0[off])
                if _rejected(rep) or pin:
                    hits.append(f"masks{n_masks}" + ("" if _rejected(rep) else "(pin)"))
    _summary("reg_grad", f"B{B} K{K} D{D}", seen)


def emu_reg_finish(case, defect=None):
    inv = t32(float(F(1.0) / F(1 if defect == "masks_ignored" else case.n_masks)))
    term = 1.0 - case.pstd * inv
    if defect != "no_relu":
        term = term.clamp_min(0.0)
    return block_sum(seq_sum(term, 256)) / t32(float(case.n))


@pytest.mark.parametrize("n", S.FINISH_N)
def test_reg_finish_emulation_within_bounds_and_defects_rejected(n):
    seen = {"no_relu": [], "masks_ignored": []}
    for n_masks in S.FINISH_MASKS:
        case = S.make_finish_case(n, n_masks)
        ref = S.reg_finish_reference(case)
        w = S.check(case.label, [("reg", emu_reg_finish(case).reshape(1), ref["out"].reshape(1), ref["tol_out"].reshape(1))])
        print(f"emulation reg_finish {case.label}: worst err/tol {_fmt(w)}")
        for defect, hits in seen.items():
            if not hits and (defect != "masks_ignored" or n_masks != 1) and (defect != "no_relu" or bool((case.pstd > n_masks).any())):
                rep = {}
                S.check(case.label, [("reg", emu_reg_finish(case, defect).reshape(1), ref["out"].reshape(1), ref["tol_out"].reshape(1))], collect=rep)
                if _rejected(rep):
                    hits.append(f"masks{n_masks}")
    if n == 1:
        seen.pop("no_relu")                  # the one value lies below the threshold: the relu does nothing
    _summary("reg_finish", f"n{n}", seen)


# ------------------------------------------------------------------------------------------------ adamw + ema
def emu_adam(case, c, defect=None):
    """the state after ONE call of vj_adamw_ema / vj_step_advance + vj_adamw_ema_guarded: the dict adam_check() takes."""
    lr, b1, b2, eps, wd, ema = [F(S.HP[k]) for k in ("lr", "beta1", "beta2", "eps")] + [F(c["wd"]), c["ema"]]
    has_pb, has_tgt, has_tb = bool(c["nulls"] & 1), bool(c["nulls"] & 2), bool(c["nulls"] & 4)
    gs, skip, step = F(c["gscale"]), False, None
    if c["kind"] == "plain":
        t = float(c["step"])
    else:
        gst = [F(x) for x in c["gstat"]]
        skip = bool((gst[1] + gst[3]) > 0)
        step = t = float(F(c["t0"]) + F(0.0 if skip else 1.0))               # step_advance
        if c["clip"] > 0:
            sel = 0 if defect == "sel_ignored" else c["sel"]
            coef = F(c["clip"]) / (np.sqrt(gst[2 * sel]) * F(c["norm_scale"]) + F(1e-6))
            gs = gs * (coef if defect == "no_cap" else min(F(1.0), coef))
    bc1 = F(1.0 - float(b1) ** t)
    bc2s = F(1.0 - float(b2) ** t) if defect == "bc2_nosqrt" else F(np.sqrt(1.0 - float(b2) ** t))
    p0, g, m0, v0, tgt0 = case.p, case.g, case.m, case.v, case.tgt
    out = dict(p=p0, m=m0, v=v0, pb=torch.full((case.n,), S.PB_FILL, dtype=torch.bfloat16) if has_pb else None, tgt=tgt0 if has_tgt else None,
               tb=torch.full((case.n,), S.TB_FILL, dtype=torch.bfloat16) if has_tb else None, step=step)
    om = F(1.0) - F(ema)
    if skip:
        src, src_rounded = p0, False
    else:
        stp = lr if defect == "no_bc1" else lr / bc1
        decay = F(1.0) - lr * wd
        gg = g * t32(gs)
        if defect == "l2":
            gg, decay = gg + t32(wd) * p0, F(1.0)
        pp = p0 * t32(decay)
        mm = m0 + (gg - m0) * t32(F(1.0) - b1)
        gv = g if defect == "v_unscaled" else gg
        vv = v0 * t32(b2) + t32(F(1.0) - b2) * gv * gv
        denom = (torch.sqrt(vv + t32(eps)) / t32(bc2s)) if defect == "eps_in_sqrt" else (torch.sqrt(vv) / t32(bc2s) + t32(eps))
        pp = pp - t32(stp) * (mm / denom)
        out.update(p=pp, m=mm, v=vv)
        if has_pb:
            out["pb"] = bf(pp)
        src, src_rounded = (p0 if defect == "ema_pre_update_p" else pp), True
    if has_tgt:
        if defect == "ema_other_product":
            src_rounded = not src_rounded
        out["tgt"] = S.ema_expected(tgt0, src, ema, src_rounded)[0]
        if has_tb:
            out["tb"] = bf(tgt0 if defect == "shadow_old_target" else out["tgt"])
    return out


ADAM_DEFECTS = ["no_bc1", "bc2_nosqrt", "eps_in_sqrt", "l2", "v_unscaled", "ema_pre_update_p", "no_cap", "sel_ignored", "ema_other_product",
                "shadow_old_target"]


def adam_defect_exists(defect, c):
    sc = S.adam_scalars(c)
    has_tgt, has_tb = bool(c["nulls"] & 2), bool(c["nulls"] & 4)
    if defect in ("ema_other_product", "shadow_old_target"):
        return has_tgt and (has_tb or defect == "ema_other_product")
    if sc["skip"]:
        return False
    clipping = c["kind"] == "guarded" and c["clip"] > 0
    return {"no_bc1": sc["bc1"] != 1.0, "bc2_nosqrt": S.f32(sc["bc2s"] ** 2) != sc["bc2s"], "l2": c["wd"] != 0, "v_unscaled": sc["gs"] != 1.0,
            "ema_pre_update_p": has_tgt, "no_cap": clipping and sc["gs_uncapped"] > sc["gs"],
            "sel_ignored": clipping and c["sel"] == 1}.get(defect, True)


@pytest.mark.parametrize("n", S.ADAM_N)
def test_adamw_emulation_within_bounds_and_defects_rejected(n):
    """every configuration of S.adam_configs(n) x every variant: p, m, v inside their bounds, tgt inside its bound and bit-equal to the
    fma of its branch (no rounding tie among the seeded inputs: asserted inside adam_check), the shadows bit-equal, a skipped step
    untouched.  A defect has to be rejected at this n in at least one (configuration, variant) where it exists."""
    configs = S.adam_configs(n)
    seen = {d: [] for d in ADAM_DEFECTS if any(adam_defect_exists(d, c) for c in configs)}
    worst = {}
    for variant in S.ADAM_VARIANTS:
        case = S.make_adam_case(n, variant)
        for i, c in enumerate(configs):
            w = S.adam_check(case, c, emu_adam(case, c))
            worst.update({k: max(worst.get(k, 0.0), x) for k, x in w.items()})
            for defect, hits in seen.items():
                if not hits and adam_defect_exists(defect, c):
                    rep = {}
                    S.adam_check(case, c, emu_adam(case, c, defect), collect=rep)
                    if _rejected(rep):
                        bound = all(r["ok"] for k, r in rep.items() if k != "pins")
                        hits.append(f"{variant}/{S.config_label(c)}" + ("(pin)" if bound else ""))
    print(f"emulation adamw n{n}: worst err/tol {_fmt(worst)}")
    _summary("adamw", f"n{n}", seen)


@pytest.mark.parametrize("n", S.EMA_N)
def test_ema_contraction_pinned_and_other_product_rejected(n):
    """ema_kernel rounds ema * tgt and fuses fl(1 - ema) * src.  The float64 emulation of the fma holds no rounding tie on the seeded
    inputs, for either product order and both momenta; the other order gives other bits at every n."""
    case = S.make_ema_case(n)
    seen = {"ema_other_product": []}
    for ema in S.EMA_MOMENTA:
        own, ties = S.ema_expected(case.tgt, case.src, ema, False)
        other, ties2 = S.ema_expected(case.tgt, case.src, ema, True)
        assert ties == 0 and ties2 == 0, (case.label, ema, ties, ties2)
        ref, tol = S.ema_reference(case.tgt, case.src, ema)
        w = S.check(case.label, [("tgt", own, ref, tol)])
        differ = int((own != other).sum())
        print(f"emulation ema {case.label} m={ema:.3f}: worst err/tol {_fmt(w)}; {differ} of {n} elements differ under the other product order")
        if differ:
            seen["ema_other_product"].append(f"m={ema:.3f}")
    _summary("ema", case.label, seen)


def test_fma_tie_detector():
    """fma_tie() flags exactly the float64 sums half way between two fp32 values."""
    one, ulp = np.float64(1.0), np.float64(2.0 ** -23)
    s = torch.tensor([one + ulp / 2, one + ulp / 2 + 2.0 ** -52, one + ulp, one + 3 * ulp / 2, 2.0 ** -100 * (one + ulp / 2)], dtype=torch.float64)
    assert S.fma_tie(s).tolist() == [True, False, False, True, True]


# ------------------------------------------------------------------------------------------------ sqnorm
def emu_sqnorm(x, old=None, defect=None):
    """(sum of squares, count of non-finite): sqnorm_kernel + sqnorm_finish_kernel."""
    v = x.view(-1, 4)
    if defect == "drop_last_float4":
        v = v[:-1]
    threads = S.SQ_BLOCKS * 256
    s = seq_sum(sum4(v * v), threads)
    bad = seq_sum(sum4((~torch.isfinite(v)).float()), threads)
    out = []
    for acc in (s, bad):
        part = block_sum(acc.view(S.SQ_BLOCKS, 256))
        out.append(block_sum(in_turn(part.view(4, 256))))
    if old is not None:
        out = [t32(o) + a for o, a in zip(old, out)]
    return out[0], out[1]


@pytest.mark.parametrize("n", S.SQ_N)
def test_sqnorm_emulation_within_bounds_and_defects_rejected(n):
    case = S.make_sq_case(n)
    seen = {"drop_last_float4": []} if n else {}
    for old in (None, S.SQ_OLD):
        ref, tol = S.sq_reference(case, None if old is None else old[0])
        s, bad = emu_sqnorm(case.x, old)
        w = S.check(case.label, [("sumsq", s.reshape(1), ref.reshape(1), tol.reshape(1))])
        assert float(bad) == (0.0 if old is None else old[1])
        if n == 0:
            assert float(s) == (0.0 if old is None else old[0])
        print(f"emulation sqnorm {case.label} accumulate={old is not None}: worst err/tol {_fmt(w)}")
        for defect, hits in seen.items():
            if not hits:
                rep = {}
                S.check(case.label, [("sumsq", emu_sqnorm(case.x, old, defect)[0].reshape(1), ref.reshape(1), tol.reshape(1))], collect=rep)
                if _rejected(rep):
                    hits.append("accumulate" if old else "overwrite")
    for name, i in S.sq_nonfinite_positions(n).items():
        x = case.x.clone()
        x[i] = S.NAN
        x[i ^ 1] = S.INF
        s, bad = emu_sqnorm(x)
        assert float(bad) == 2.0 and not bool(torch.isfinite(s)), (name, float(bad), float(s))
    _summary("sqnorm", case.label, seen)


# ------------------------------------------------------------------------------------------------ grad_stats_multi
def emu_grad_stats(case, moments, defect=None):
    """[n_tensors, 8, 3] fp32: grad_stats_multi_kernel, one workgroup per (tensor, chunk)."""
    out = torch.zeros(len(case.offsets), S.GS_CHUNKS, 3)
    M2 = case.M1 if defect == "m2_from_m1" else case.M2
    for t, (off, n) in enumerate(case.offsets):
        per = S.cdiv(S.cdiv(n, S.GS_CHUNKS), 4) * 4
        for c, (lo, hi) in enumerate(S.gs_chunks(n)):
            if defect == "hi_overrun":
                hi = lo + per
            n4 = (hi - lo) >> 2 if hi > lo else 0
            srcs = [(case.G, lambda x: x * x)] + ([(case.M1, torch.abs), (M2, torch.abs)] if moments else [])
            for k, (A, fn) in enumerate(srcs):
                acc = seq_sum(sum4(fn(A[off + lo:off + lo + 4 * n4].view(-1, 4))), 256)
                if defect != "tail_dropped" and hi > lo + 4 * n4:
                    tail = torch.zeros(256)
                    tail[:hi - lo - 4 * n4] = fn(A[off + lo + 4 * n4:off + hi])
                    acc = acc + tail
                out[t, c, k] = block_sum(acc)
    return out


def test_grad_stats_emulation_within_bounds_and_defects_rejected():
    """every per-chunk partial of every tensor of the arena; a defect has to be rejected at every tensor where it exists."""
    case = S.make_gs_case()
    for moments in (True, False):
        ref, tol = S.gs_reference(case, moments)
        out = emu_grad_stats(case, moments)
        w = S.check(case.label, [("partials", out.view(-1, 3), ref.view(-1, 3), tol.view(-1, 3))])
        print(f"emulation grad_stats moments={moments}: worst err/tol {_fmt(w)}")
        exists = {"tail_dropped": lambda n: n % 4 != 0, "hi_overrun": lambda n: any(lo + (S.cdiv(S.cdiv(n, 8), 4) * 4) > n for lo, _ in S.gs_chunks(n)),
                  "m2_from_m1": lambda n: moments}
        for t, (off, n) in enumerate(case.offsets):
            seen = {d: [] for d, f in exists.items() if f(n)}
            for defect, hits in seen.items():
                o2 = emu_grad_stats(case, moments, defect)
                rep = {}
                S.check(case.label, [("partials", o2[t], ref[t], tol[t])], collect=rep)
                if _rejected(rep):
                    hits.append("moments" if moments else "gradients only")
            _summary("grad_stats", f"numel{n} moments={moments}", seen)


def test_depths_and_shapes():
    """the numbers the bounds rest on, spelled out."""
    assert S.LEVELS == 9
    assert S.loss_depth(8) == 8 + 9 + 2 + 9 and S.loss_depth(8 * 512 * 256) == 28 and S.loss_depth(8 * (512 * 256 + 1)) == 36
    assert S.pstd_depth(2) == 33 and S.pstd_depth(32) == 33 and S.pstd_depth(33) == 34 and S.pstd_depth(65) == 35
    assert S.sq_depth(4) == 3 + 1 + 9 + 4 + 9 and S.sq_depth(4 * (1024 * 256 + 5)) == 27
    assert S.gs_chunks(1) == [(0, 1)] + [(4 * c, 1) for c in range(1, 8)]
    assert S.gs_chunks(8197)[-1] == (7 * 1028, 8197) and S.gs_chunks(8192)[-1] == (7168, 8192)
    B, K, D = S.REG_SHAPES[-1]
    assert B * K * D // 8 == S.FLAT_CAP * 256 + 1 and S.ADAM_BIG // 4 == S.FLAT_CAP * 256 + 3
    assert all(o % 64 == 0 for o, _ in S.make_gs_case().offsets)
    sc = S.adam_scalars(S.GUARDED_CONFIGS[0])
    assert abs(sc["coef"] - 0.25) < 1e-6 and S.adam_scalars(S.GUARDED_CONFIGS[2])["coef"] == 1.0 and S.adam_scalars(S.GUARDED_CONFIGS[5])["skip"]
