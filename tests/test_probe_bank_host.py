"""CPU: the probe bank's algebra, fixture, construction and host-side argument checks (no kernel is launched here)."""
import pytest
import torch

from oracle import probe_oracle as po
from tests.probe_bank_util import BLK, load_fixture, pooled_loss_and_grads, rel_l2

KVB = BLK + "xattn.kv.bias"


def _random_probe(B, N, D, H, C, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    w = {"pooler.query_tokens": 0.5 * r(1, 1, D), "linear.weight": 0.3 * r(C, D), "linear.bias": 0.1 * r(C)}
    for n_, shape, scale in (("norm1.weight", (D,), None), ("norm1.bias", (D,), 0.1), ("xattn.q.weight", (D, D), 0.3),
                             ("xattn.q.bias", (D,), 0.1), ("xattn.kv.weight", (2 * D, D), 0.3), ("xattn.kv.bias", (2 * D,), 0.1),
                             ("norm2.weight", (D,), None), ("norm2.bias", (D,), 0.1), ("mlp.fc1.weight", (4 * D, D), 0.3),
                             ("mlp.fc1.bias", (4 * D,), 0.1), ("mlp.fc2.weight", (D, 4 * D), 0.3), ("mlp.fc2.bias", (D,), 0.1)):
        w[BLK + n_] = 1.0 + 0.1 * r(*shape) if scale is None else scale * r(*shape)
    return w, r(B, N, D), torch.randint(0, C, (B,), generator=g)


@pytest.mark.parametrize("B,N,D,H", [(3, 37, 48, 4), (1, 1, 32, 2)])
def test_pooled_restatement_matches_the_oracle_in_float64(B, N, D, H):
    """The pooled form (no K, no V; norm1.bias and the key bias dropped from the scores) is the reference's probe: logits to 1e-10,
    every gradient to 1e-10 relative against autograd of oracle/probe_oracle.py, both in float64.  The key half of kv.bias gets an
    exactly-zero gradient (the oracle's is rounding noise)."""
    w, x, labels = _random_probe(B, N, D, H, 7, seed=100 + N)
    o_loss, o_logits, o_g = po.probe_loss_and_grads(w, x, labels, H)
    loss, logits, g = pooled_loss_and_grads(w, x, labels, H)
    assert (logits - o_logits).abs().max() < 1e-10
    assert abs(float(loss - o_loss)) < 1e-10
    assert set(g) == set(o_g)
    assert torch.count_nonzero(g[KVB][:D]) == 0
    assert o_g[KVB][:D].abs().max() < 1e-12 * o_g[KVB][D:].abs().max()
    gmax = max(float(v.norm()) for v in o_g.values())
    for k in o_g:
        a, b = (g[k][D:], o_g[k][D:]) if k == KVB else (g[k], o_g[k])
        if float(b.norm()) == 0.0:   # N = 1: the soft-max over one key is constant, the whole score path has gradient zero; "relative"
            assert float(a.norm()) < 1e-10 * gmax, (k, float(a.norm()))   # then means relative to the largest gradient tensor
        else:
            assert rel_l2(a, b) < 1e-10, (k, rel_l2(a, b))


def test_pooled_restatement_matches_the_reference_fixture():
    """Against the step-0 logits, loss and gradients the REAL reference module produced in fp32 (tests/golden/probe_bank_micro.npz):
    the restatement in float64 on the fixture's fp32 weights differs only by the reference's own fp32 rounding and summation
    order (1e-5 relative per tensor; sums of at most B*N = 210 terms of fp32 eps 6e-8 each)."""
    meta, x, labels, probes = load_fixture()
    assert (meta["P"], meta["B"], meta["N"], meta["D"], meta["H"], meta["C"]) == (3, 3, 70, 32, 2, 5)
    assert len({(p["lr"], p["wd"]) for p in probes}) == 3
    D = meta["D"]
    for p in probes:
        w = {k: v.double() for k, v in p["w0"].items()}
        loss, logits, g = pooled_loss_and_grads(w, x.double(), labels, meta["H"])
        assert rel_l2(logits, p["logits"]) < 1e-5
        assert abs(float(loss) - p["loss"]) < 1e-5 * max(1.0, abs(p["loss"]))
        assert set(g) == set(p["grads"])
        for k, ref in p["grads"].items():
            a, b = (g[k][D:], ref[D:]) if k == KVB else (g[k], ref)
            assert rel_l2(a, b) < 1e-5, (k, rel_l2(a, b))
        assert torch.count_nonzero(p["w0"][KVB][:D]) == 0
        assert len(p["losses"]) == meta["steps"] == 3 and abs(p["losses"][0] - p["loss"]) < 1e-6


def test_bank_initialisation_and_names():
    """Probe 0 of a bank under seed s is the lone classifier under seed s; the state dict is `probes.{p}.` + the reference's names;
    probe_state_dict(p) loads strictly into a lone AttentiveClassifier."""
    from jepa_amd.src.models.attentive_pooler import AttentiveClassifier, AttentiveClassifierBank
    torch.manual_seed(5)
    bank = AttentiveClassifierBank(64, 2, 5, 3)
    torch.manual_seed(5)
    lone = AttentiveClassifier(embed_dim=64, num_heads=2, depth=1, num_classes=5)
    torch.manual_seed(5)
    lone_b = AttentiveClassifier(embed_dim=64, num_heads=2, depth=1, num_classes=5)
    second = AttentiveClassifier(embed_dim=64, num_heads=2, depth=1, num_classes=5)   # the next draw of the same generator
    ref_names = list(lone.state_dict())
    assert isinstance(bank.probes, torch.nn.ModuleList) and len(bank.probes) == 3
    assert list(bank.state_dict()) == [f"probes.{p}.{n}" for p in range(3) for n in ref_names]
    for n, v in lone.state_dict().items():
        assert torch.equal(bank.state_dict()["probes.0." + n], v), n
        assert torch.equal(lone_b.state_dict()[n], v), n
        assert torch.equal(bank.state_dict()["probes.1." + n], second.state_dict()[n]), n
    assert not torch.equal(bank.probes[1].linear.weight, bank.probes[0].linear.weight)
    fresh = AttentiveClassifier(embed_dim=64, num_heads=2, depth=1, num_classes=5)
    res = fresh.load_state_dict(bank.probe_state_dict(2), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(fresh.linear.weight, bank.probes[2].linear.weight)
    meta, _, _, probes = load_fixture()   # the reference's own names, from the real module
    assert list(probes[0]["w0"]) == [n for n, _ in AttentiveClassifier(embed_dim=32, num_heads=2, num_classes=5).named_parameters()]


def test_bank_refuses_cpu_tensors_and_features_that_require_grad():
    from jepa_amd.src.models.attentive_pooler import AttentiveClassifierBank
    bank = AttentiveClassifierBank(64, 2, 5, 2)
    with pytest.raises(ValueError, match="no CPU fallback"):
        bank(torch.zeros(1, 4, 64))
    with pytest.raises(ValueError):
        AttentiveClassifierBank(64, 2, 5, 0)
    with pytest.raises(NotImplementedError):
        AttentiveClassifierBank(48, 4, 5, 2)   # the lone probe's own limit (embed_dim % 32): every probe is the lone classifier


def test_pool_softmax_entry_points_validate_on_the_host():
    """Bad dimensions, null pointers, misaligned buffers and a short workspace are refused with a message before any launch (this
    host has no GPU: a launch would fail differently).  Pointers here are made-up addresses that nothing dereferences."""
    from jepa_amd import build
    from jepa_amd.hip import lib as L
    build.build(verbose=False)
    lib = L.load_library()
    c = lib.vj_pool_softmax_chunk_keys()
    assert c > 0
    B, N, C = 2, 2 * c + 3, 64
    need = lib.vj_pool_softmax_fwd_ws_bytes(B, N, C)
    assert need == 2 * B * 3 * C * 4
    assert lib.vj_pool_softmax_fwd_ws_bytes(B, N, 6) < 0 and b"multiple of 4" in lib.vj_last_error()
    assert lib.vj_pool_softmax_fwd_ws_bytes(0, N, C) < 0 and b"positive" in lib.vj_last_error()
    assert lib.vj_pool_softmax_fwd_ws_bytes(70000, N, C) < 0 and b"65535" in lib.vj_last_error()
    ok = 0x10000
    fwd = lambda S=ok, A=ok, lse=ok, b=B, n=N, cc=C, ws=ok, nws=need: lib.vj_pool_softmax_fwd(S, A, lse, b, n, cc, ws, nws, None)   # noqa: E731
    bwd = lambda A=ok, dA=ok, d=ok, dS=ok, b=B, n=N, cc=C: lib.vj_pool_softmax_bwd(A, dA, d, dS, b, n, cc, None)   # noqa: E731
    for bad, msg in ((dict(cc=6), b"multiple of 4"), (dict(n=0), b"positive"), (dict(b=-1), b"positive"), (dict(S=None), b"null"),
                     (dict(A=None), b"null"), (dict(lse=None), b"null"), (dict(ws=None), b"null"), (dict(S=ok + 4), b"aligned"),
                     (dict(A=ok + 2), b"aligned"), (dict(lse=ok + 8), b"aligned"), (dict(nws=need - 1), b"workspace")):
        assert fwd(**bad) < 0 and msg in lib.vj_last_error(), (bad, lib.vj_last_error())
    for bad, msg in ((dict(cc=2), b"multiple of 4"), (dict(n=-5), b"positive"), (dict(A=None), b"null"), (dict(dA=None), b"null"),
                     (dict(d=None), b"null"), (dict(dS=None), b"null"), (dict(dA=ok + 4), b"aligned"), (dict(d=ok + 8), b"aligned"),
                     (dict(dS=ok + 4), b"aligned")):
        assert bwd(**bad) < 0 and msg in lib.vj_last_error(), (bad, lib.vj_last_error())


def test_multihead_kwargs_overrides_and_fallbacks():
    """`optimization.multihead_kwargs`: each entry overrides lr / start_lr / final_lr / weight_decay / warmup, the rest falls back to
    `optimization`; without the key the parser answers None, which is what keeps both mains on their single-probe code."""
    import inspect
    from jepa_amd.evals.image_classification_frozen import eval as EI
    from jepa_amd.evals.multihead import parse_multihead_kwargs
    from jepa_amd.evals.video_classification_frozen import eval as EV
    opt = {'lr': 0.01, 'start_lr': 0.002, 'final_lr': 0.0, 'weight_decay': 0.01, 'warmup': 0.5, 'num_epochs': 2, 'batch_size': 4}
    assert parse_multihead_kwargs(opt) is None
    hps = parse_multihead_kwargs(dict(opt, multihead_kwargs=[{}, {'lr': 0.1}, {'weight_decay': 0.4, 'warmup': 0.0, 'final_lr': 1e-4,
                                                                                 'start_lr': 0.05}]))
    base = {k: opt[k] for k in ('lr', 'start_lr', 'final_lr', 'weight_decay', 'warmup')}
    assert hps == [base, dict(base, lr=0.1), dict(base, weight_decay=0.4, warmup=0.0, final_lr=1e-4, start_lr=0.05)]
    for bad in ([], {}, [3], [{'momentum': 0.9}]):
        with pytest.raises(ValueError):
            parse_multihead_kwargs(dict(opt, multihead_kwargs=bad))
    for E in (EV, EI):   # the bank branch is entered only on a parsed list; everything else in main is the single-probe eval
        src = inspect.getsource(E.main)
        assert src.count("multihead is not None") == 1 and src.count("multihead is None") == 2
        assert src.index("if multihead is not None") < src.index("init_opt(classifier=classifier")
