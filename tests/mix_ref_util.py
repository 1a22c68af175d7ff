"""float64 numpy restatements of vj_clip_mix and vj_soft_ce, of the soft target, and the checkers the GPU tests hold the kernels'
outputs against (tests/test_mix_host.py plants errors to see that the checkers reject them).

The references take the fp32 inputs of the kernels at their exact values (lam, the smoothing and the logits are fp32 by the
kernels' interface) and compute everything else in float64."""
import numpy as np

# ---------------------------------------------------------------------------------------------------------------------- clip_mix
OWN, SWAPPED, BLENDED = 0, 1, 2


def clip_mix_ref(x, lam, box):
    """x fp32 [B,P,H,W], lam fp32 [B], box int [B,4] = (y0, y1, x0, x1) -> (ref float64 [B,P,H,W], kind int8 [B,P,H,W] in
    {OWN, SWAPPED, BLENDED}, bound float64 [B,P,H,W]).  Sample i pairs with B-1-i; the middle sample of an odd B is OWN.  bound is
    2^-22 * (|lam x_i| + |(1 - lam) x_j|) on blended elements: three fp32 roundings of relative 2^-24 each -- of 1 - lam, of the
    product (1 - lam) * x_j and of the fused lam * x_i + product -- and 0 elsewhere (those are compared bit for bit)."""
    assert x.dtype == np.float32 and lam.dtype == np.float32
    B, P, H, W = x.shape
    xd, ld = x.astype(np.float64), lam.astype(np.float64)
    ref, kind, bound = xd.copy(), np.zeros(x.shape, np.int8), np.zeros(x.shape, np.float64)
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    for i in range(B):
        j = B - 1 - i
        if i == j:
            continue
        y0, y1, x0, x1 = (int(v) for v in box[i])
        inside = np.broadcast_to((ys >= y0) & (ys < y1) & (xs >= x0) & (xs < x1), (P, H, W))
        ref[i] = np.where(inside, xd[j], xd[i])
        kind[i] = np.where(inside, SWAPPED, OWN)
        if lam[i] != np.float32(1.0):
            a, b = ld[i] * xd[i], (1.0 - ld[i]) * xd[j]
            ref[i] = np.where(inside, ref[i], a + b)
            kind[i] = np.where(inside, kind[i], BLENDED)
            bound[i] = np.where(inside, 0.0, 2.0 ** -22 * (np.abs(a) + np.abs(b)))
    return ref, kind, bound


def check_clip_mix(out, x, lam, box):
    """Raises AssertionError unless out (fp32 [B,P,H,W]) is what vj_clip_mix may leave of x: own and swapped elements bit for bit,
    blended ones within the bound.  Returns the worst |out - ref| / bound over the blended elements (0 without any)."""
    ref, kind, bound = clip_mix_ref(x, lam, box)
    assert out.dtype == np.float32 and out.shape == x.shape
    j = x[::-1]
    want_bits = np.where(kind == SWAPPED, j.view(np.int32), x.view(np.int32))
    exact = kind != BLENDED
    bad = exact & (out.view(np.int32) != want_bits)
    assert not bad.any(), f"{int(bad.sum())} element(s) that must keep their own or take their partner's bits differ, first at " \
                          f"{tuple(int(v) for v in np.argwhere(bad)[0])}"
    blended = ~exact
    if not blended.any():
        return 0.0
    err = np.abs(out.astype(np.float64) - ref)
    over = blended & ~(err <= bound)
    assert not over.any(), f"{int(over.sum())} blended element(s) outside 2^-22 (|lam x_i| + |(1 - lam) x_j|), first at " \
                           f"{tuple(int(v) for v in np.argwhere(over)[0])}: {err[over][0]} > {bound[over][0]}"
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, 0.0)
    return float(ratio[blended].max())


# ----------------------------------------------------------------------------------------------------------------------- soft_ce
def soft_target(label_a, label_b, lam, eps, C):
    """t[r,c] = eps / C + (1 - eps) * (lam[r] * [c == a[r]] + (1 - lam[r]) * [c == b[r]]) in float64."""
    a, b = np.asarray(label_a), np.asarray(label_b)
    lam = np.asarray(lam).astype(np.float64)
    R = a.shape[0]
    t = np.zeros((R, C), np.float64)
    t[np.arange(R), a] += lam
    t[np.arange(R), b] += 1.0 - lam
    return float(eps) / C + (1.0 - float(eps)) * t


def soft_ce_ref(z, label_a, label_b, lam, eps):
    """z fp32 [R,C] -> (loss [R], dlogits [R,C] = softmax - target, softmax [R,C]) in float64; loss = -sum_c t_c log_softmax(z)_c."""
    zd = np.asarray(z).astype(np.float64)
    R, C = zd.shape
    m = zd.max(axis=1, keepdims=True)
    e = np.exp(zd - m)
    s = e.sum(axis=1, keepdims=True)
    logp = zd - m - np.log(s)
    t = soft_target(label_a, label_b, lam, eps, C)
    return -(t * logp).sum(axis=1), e / s - t, e / s


def soft_ce_errors(loss, dlogits, probs, ref):
    """(worst |loss - ref| / max(1, |ref|), worst |dlogits - ref|, worst |probs - ref| or 0) against soft_ce_ref's result."""
    rl, rd, rp = ref
    el = float(np.max(np.abs(np.asarray(loss, np.float64) - rl) / np.maximum(1.0, np.abs(rl)))) if rl.size else 0.0
    ed = float(np.max(np.abs(np.asarray(dlogits, np.float64) - rd))) if rd.size else 0.0
    ep = float(np.max(np.abs(np.asarray(probs, np.float64) - rp))) if probs is not None and rp.size else 0.0
    return el, ed, ep


def check_soft_ce(loss, dlogits, probs, ref, loss_bound, grad_bound):
    """Raises AssertionError unless the outputs lie within the bounds of the float64 reference and have the structure of a
    soft-max minus a target: finite, probs >= 0, sum_c dlogits = 0 within C * 2^-23.  Returns soft_ce_errors."""
    dl = np.asarray(dlogits, np.float64)
    C = dl.shape[1]
    assert np.isfinite(np.asarray(loss)).all() and np.isfinite(dl).all(), "non-finite output"
    el, ed, ep = soft_ce_errors(loss, dlogits, probs, ref)
    assert el <= loss_bound, f"loss off by {el} (relative to max(1, |ref|)), bound {loss_bound}"
    assert ed <= grad_bound, f"dlogits off by {ed}, bound {grad_bound}"
    assert ep <= grad_bound, f"probs off by {ep}, bound {grad_bound}"
    rows = np.abs(dl.sum(axis=1))
    assert (rows <= C * 2.0 ** -23).all(), f"sum_c dlogits = {rows.max()} exceeds C * 2^-23 = {C * 2.0 ** -23}"
    if probs is not None:
        assert (np.asarray(probs) >= 0).all(), "negative probability"
    return el, ed, ep


SOFT_CE_CAP = 1e-5          # both bounds of vj_soft_ce are capped here, see tests/test_mix_gpu.py
SOFT_CE_CLASSES = (1, 2, 63, 64, 65, 400, 1000, 8142)


def soft_ce_cases(C):
    """The inputs both the GPU test of vj_soft_ce and the CPU check of the cap run: (name, z fp32 [R,C], a, b int32 [R], lam fp32
    [R], eps) for R in {1, 3}; logits N(0, 3^2), rows with entries at +-80, rows of equal logits; a == b and a != b (where C
    allows); lam in {1, 0.25}; eps in {0, 0.1}."""
    rng = np.random.RandomState(7000 + C)
    for R in (1, 3):
        normal = (3.0 * rng.randn(R, C)).astype(np.float32)
        pm80 = normal.copy()
        pm80[:, 0] = 80.0
        pm80[:, C // 2] = -80.0 if C > 1 else 80.0
        if C > 4:
            pm80[:, C - 1] = 80.0
        equal = np.full((R, C), 1.5, np.float32)
        a = rng.randint(C, size=R).astype(np.int32)
        other = ((a + 1 + rng.randint(max(C - 1, 1), size=R)) % C).astype(np.int32)       # != a when C > 1
        for zname, z in (("normal", normal), ("pm80", pm80), ("equal", equal)):
            for bname, b in (("a==b", a), ("a!=b", other)):
                for lam in (1.0, 0.25):
                    for eps in (0.0, 0.1):
                        yield (f"R={R} {zname} {bname} lam={lam} eps={eps}", z, a, b, np.full((R,), lam, np.float32), np.float32(eps))
