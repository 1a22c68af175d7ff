"""CPU: the host half of the image evals' AutoAugment -- the policy table, the level arguments against the reference's functions'
values, the draw protocol against an independent replay, the fixture against PIL on this machine, the transform / collate /
validate path and the `data.auto_augment` key.  Every comparison is exact."""
import random

import numpy as np
import pytest
import torch

from tests import image_autoaug_util as U

SEEDS = range(400)


@pytest.fixture(scope="module")
def z():
    return np.load(U.GOLDEN)


def test_policy_table_is_the_25_rows():
    from jepa_amd.app.vjepa import randaugment as RA
    assert len(RA.POLICY_ORIGINAL) == 25
    assert [[tuple(op) for op in sub] for sub in RA.POLICY_ORIGINAL] == [[tuple(op) for op in sub] for sub in U.POLICY]
    for sub in RA.POLICY_ORIGINAL:
        assert len(sub) == 2
        for name, prob, m in sub:
            assert RA.policy_code(name) == U.CODES[name] and 0.0 <= prob <= 1.0 and 0 <= m <= 10


def test_level_arguments_equal_the_reference_functions(z, monkeypatch):
    """For every (operation, magnitude) of the table: what this package's plan holds is what the reference's LEVEL_TO_ARG function
    returned (signs not negated: random.random() is held at 0.1 here as in the tool)."""
    from jepa_amd.app.vjepa import randaugment as RA
    monkeypatch.setattr(random, "random", lambda: 0.1)
    draw, H, W = RA.AutoAugmentDraw("original"), 20, 20
    seen = set()
    for name, m, want in zip((str(n) for n in z["level_name"]), z["level_mag"].tolist(), z["level_arg"].tolist()):
        seen.add((name, m))
        ops, args = draw.plan([(name, 1.0, m)], (True,), H, W)
        if name in ("AutoContrast", "Equalize", "Invert"):
            assert np.isnan(want) and ops[0] == U.CODES[name] and not args.any()
        elif name == "Rotate":
            assert ops[0] == 4 and tuple(args[0]) == tuple(RA.rotation_coefficients(want, H, W))
        elif name == "ShearX":
            assert ops[0] == 12 and tuple(args[0]) == (1.0, want, 0.0, 0.0, 1.0, 0.0)
        elif name == "PosterizeOriginal" and want >= 8:
            assert ops[0] == 0 and not args.any()              # eight bits kept: the identity, code 0
        else:
            assert ops[0] == U.CODES[name] and args[0, 0] == want and not args[0, 1:].any(), (name, m)
    assert seen == {(n, m) for sub in U.POLICY for n, _, m in sub}


def test_draw_protocol_against_an_independent_replay():
    from jepa_amd.app.vjepa.randaugment import AutoAugmentDraw
    draw, first_of_12, certain = AutoAugmentDraw("original"), 0, 0
    np.random.seed(5), torch.manual_seed(5)
    np_state, torch_state = np.random.get_state()[1].copy(), torch.get_rng_state().clone()
    hit = set()
    for s in SEEDS:
        H = W = (20, 36, 224)[s % 3]
        p, ops, args, coins, nxt = U.replay_draw(s, H, W)
        random.seed(s)
        got_ops, got_args = draw.draw(H, W)
        assert got_ops.dtype == np.int32 and got_ops.shape == (8,) and got_args.dtype == np.float64 and got_args.shape == (8, 6)
        assert np.array_equal(got_ops, ops) and np.array_equal(got_args, args), s
        assert random.random() == nxt, s                       # the same number of draws was consumed
        assert not got_ops[2:].any()
        hit.add(p)
        if p == 12:
            first_of_12 += 1
            assert got_ops[0] == 0                             # probability 0.0: never applies
        ones = sum(1 for _, prob, _ in U.POLICY[p] if prob == 1.0)
        assert coins == 2 - ones                               # a prob = 1.0 operation consumes no coin
        certain += ones
    assert hit == set(range(25)) and first_of_12 > 0 and certain > 0
    assert np.array_equal(np.random.get_state()[1], np_state) and torch.equal(torch.get_rng_state(), torch_state)


def test_a_certain_operation_consumes_no_coin(monkeypatch):
    """Sub-policy 14 = Color .6, Contrast 1.: exactly one coin; with every coin refusing, Contrast still applies."""
    from jepa_amd.app.vjepa import randaugment as RA
    draw = RA.AutoAugmentDraw("original", policy=[RA.POLICY_ORIGINAL[14]])
    calls = []
    monkeypatch.setattr(random, "random", lambda: calls.append(1) or 0.99)
    ops, args = draw.draw(20, 20)
    assert len(calls) == 1 and ops[:2].tolist() == [0, 9] and args[1, 0] == (8 / 10) * 1.8 + 0.1


def test_fixture_is_reproduced_by_pil_from_the_tables_alone(z):
    """The tables carry everything the device needs: PIL here, fed only (ops, args, fill), gives every expected image."""
    pytest.importorskip("PIL")
    total, affine_fill = 0, 0
    assert tuple(z["fill"].tolist()) == U.FILL
    for S in U.SIDES:
        for name, src, flip, ops, args, want in U.cases(z, S):
            arr = src[:, ::-1] if flip else src
            got = U.pil_apply_plan(arr, ops, args)
            assert got.shape == (S, S, 3) and np.array_equal(got, want), name
            total += 1
            affine_fill += int(any(int(c) in (4, 12, 14, 15) for c in ops) and (want == np.array(U.FILL, np.uint8)).all(-1).any())
    assert total == len(z["case_20/name"]) + len(z["case_36/name"]) + len(z["case_96/name"]) >= 2 * 64 + 5
    assert affine_fill > 10                                    # the fill colour shows in the affine cases
    names = [str(n) for n in z["case_20/name"]]
    assert "noop" in names and any(n.startswith("rand_translate") for n in names)
    for p in range(25):
        for S in (20, 36):
            have = [str(n) for n in z[f"case_{S}/name"] if str(n).startswith(f"policy{p:02d}_")]
            signed = any(n in ("Rotate", "ShearX") for n, _, _ in U.POLICY[p])
            assert len(have) == (4 if signed else 2), (p, S, have)
    # the mixed batch: crop + bicubic resize, flip, plan
    from PIL import Image
    at = 0
    for k, (H, W) in enumerate(z["batch/shapes"].tolist()):
        img = z["batch/images"][at:at + H * W * 3].reshape(H, W, 3)
        at += H * W * 3
        i, j, h, w, S = (int(v) for v in z["batch/geom"][k][:5])
        pil = Image.fromarray(img).crop((j, i, j + w, i + h)).resize((S, S), Image.BICUBIC)
        arr = np.asarray(pil)[:, ::-1] if z["batch/flip"][k] else np.asarray(pil)
        assert np.array_equal(U.pil_apply_plan(arr, z["batch/ops"][k], z["batch/args"][k]), z["batch/out"][k]), k


def test_transform_draws_box_flip_plan_erase_at_the_output_side(monkeypatch):
    from jepa_amd.evals.image_classification_frozen import transforms as T
    order, inside = [], []
    real_box, real_erase, real_uniform = T._draw_box, T.draw_erase, np.random.uniform

    def box(*a, **kw):
        inside.append(1)
        out = real_box(*a, **kw)
        inside.pop()
        order.append("box")
        return out

    def uniform(*a, **kw):
        if not inside:
            order.append("flip")
        return real_uniform(*a, **kw)

    def erase(*a, **kw):
        order.append("erase")
        return real_erase(*a, **kw)

    monkeypatch.setattr(T, "_draw_box", box)
    monkeypatch.setattr(T, "draw_erase", erase)
    monkeypatch.setattr(np.random, "uniform", uniform)
    tr = T.make_transforms(training=True, resolution=20, auto_augment="original")
    real_plan, sizes = tr.auto_augment.draw, []

    def plan(H, W):
        order.append("plan")
        sizes.append((H, W))
        return real_plan(H, W)

    tr.auto_augment.draw = plan
    U.seed_all(3)
    raw = tr(np.zeros((31, 47, 3), np.uint8))
    assert order == ["box", "flip", "plan", "erase"] and sizes == [(20, 20)]
    assert raw.aug_ops.dtype == torch.int32 and tuple(raw.aug_ops.shape) == (8,)
    assert raw.aug_args.dtype == torch.float64 and tuple(raw.aug_args.shape) == (8, 6)
    # a `rand-...` string goes to RandAugmentDraw at (S, S)
    from jepa_amd.app.vjepa.randaugment import AutoAugmentDraw, RandAugmentDraw
    assert isinstance(tr.auto_augment, AutoAugmentDraw)
    tr = T.make_transforms(training=True, resolution=20, auto_augment="rand-m9-mstd0.5-inc1")
    assert isinstance(tr.auto_augment, RandAugmentDraw) and tr.auto_augment.magnitude == 9 and tr.auto_augment.increasing
    assert tr(np.zeros((31, 47, 3), np.uint8)).aug_ops is not None


def test_validation_draws_nothing_and_the_key_absent_gives_no_plan():
    from jepa_amd.evals.image_classification_frozen import transforms as T
    val = T.make_transforms(training=False, resolution=20, auto_augment="original")
    assert val.auto_augment is None
    U.seed_all(9)
    before = (random.getstate(), np.random.get_state()[1].copy(), torch.get_rng_state().clone())
    raw = val(np.zeros((31, 47, 3), np.uint8))
    assert raw.aug_ops is None and raw.aug_args is None
    assert random.getstate() == before[0] and np.array_equal(np.random.get_state()[1], before[1])
    assert torch.equal(torch.get_rng_state(), before[2])
    # the key absent: no plan, and the draws of today (the same stream with and without the keyword's default)
    U.seed_all(4)
    a = T.make_transforms(training=True, resolution=20)(np.zeros((31, 47, 3), np.uint8))
    U.seed_all(4)
    b = T.ImageTransform(training=True, resolution=20, auto_augment=None)(np.zeros((31, 47, 3), np.uint8))
    assert a.aug_ops is None and b.aug_ops is None and (a.geom, a.flip, a.ebox) == (b.geom, b.flip, b.ebox)
    batch = T.collate_raw_images([a, b])
    assert batch.aug_ops is None and batch.aug_args is None and not batch.augmented
    with pytest.raises(ValueError, match="accepted"):
        T.make_transforms(training=False, resolution=20, auto_augment="v0")


def test_collate_shapes_and_validation_before_any_copy(z, monkeypatch):
    from jepa_amd.evals.image_classification_frozen import transforms as T
    items = U.batch_items(z)
    batch = T.collate_raw_images(items)
    B = len(items)
    assert batch.aug_ops.dtype == torch.int32 and tuple(batch.aug_ops.shape) == (B, 8)
    assert batch.aug_args.dtype == torch.float64 and tuple(batch.aug_args.shape) == (B, 8, 6) and batch.augmented
    assert np.array_equal(batch.aug_ops.numpy(), z["batch/ops"]) and np.array_equal(batch.aug_args.numpy(), z["batch/args"])
    # images without a plan beside images with one: zero rows
    mixed = T.collate_raw_images(U.batch_items(z)[:2] + U.batch_items(z, with_plans=False)[2:4])
    assert tuple(mixed.aug_ops.shape) == (4, 8) and not mixed.aug_ops[2:].any() and not mixed.aug_args[2:].any()
    assert not T.collate_raw_images(U.batch_items(z, zero_plans=True)).augmented
    # the positional constructors still work
    a = items[0]
    assert T.RawImage(a.image, a.geom, a.flip, a.crop_size, a.filter, a.mean, a.std).aug_ops is None
    assert T.RawImageBatch(batch.frames, batch.desc, batch.geom, batch.crop_size, batch.filter, batch.mean, batch.std).aug_ops is None
    # refused on the host, before pack_buffers copies a byte
    copies = []
    monkeypatch.setattr(T, "pack_buffers", lambda *a, **kw: copies.append(1))
    for bad_ops, bad_args, match in ((16, None, "operation code"), (-1, None, "operation code"), (None, float("nan"), "non-finite"),
                                     (None, float("inf"), "non-finite")):
        items = U.batch_items(z)
        if bad_ops is not None:
            items[1].aug_ops[0] = bad_ops
        else:
            items[1].aug_args[0, 2] = bad_args
        with pytest.raises(ValueError, match=match):
            T.collate_raw_images(items)
    assert not copies
    with pytest.raises(ValueError, match="come together"):
        T.RawImage(a.image, a.geom, a.flip, a.crop_size, a.filter, a.mean, a.std, aug_ops=np.zeros(8, np.int32))
    bad = T.RawImageBatch(batch.frames, batch.desc, batch.geom, batch.crop_size, batch.filter, batch.mean, batch.std,
                          aug_ops=batch.aug_ops[:, :4].contiguous(), aug_args=batch.aug_args)
    with pytest.raises(ValueError, match="malformed"):
        bad.validate()
    assert T.fill_colour(batch.mean) == U.FILL


@pytest.mark.parametrize("which", ["frozen", "finetune"])
def test_config_key(which):
    if which == "frozen":
        from jepa_amd.evals.image_classification_frozen.eval import make_dataloader, parse_auto_augment
    else:
        from jepa_amd.evals.image_classification_finetune.eval import parse_auto_augment
        from jepa_amd.evals.image_classification_frozen.eval import make_dataloader
    for name in ("synthetic_images", "image_folder"):
        assert parse_auto_augment({"dataset_name": name}) is None
        assert parse_auto_augment({"dataset_name": name, "auto_augment": None}) is None
        assert parse_auto_augment({"dataset_name": name, "auto_augment": "original"}) == "original"
        assert parse_auto_augment({"dataset_name": name, "auto_augment": "rand-m9-mstd0.5-inc1"}) == "rand-m9-mstd0.5-inc1"
        for bad in ("originalr", "v0", "v0r", "3a", "augmix-m5-w4-d2", "original-mstd0.5", "v0-mstd0.5", True, 1, "", "Original"):
            with pytest.raises(ValueError, match="'original'"):
                parse_auto_augment({"dataset_name": name, "auto_augment": bad})
        with pytest.raises(NotImplementedError, match="'w' section"):
            parse_auto_augment({"dataset_name": name, "auto_augment": "rand-m9-w0"})
    assert parse_auto_augment({"dataset_name": "synthetic"}) is None
    for value in ("original", "rand-m9-mstd0.5-inc1"):
        with pytest.raises(ValueError, match="uint8 images"):
            parse_auto_augment({"dataset_name": "synthetic", "auto_augment": value})
    common = dict(root_path=None, image_folder=None, batch_size=2, world_size=1, rank=0, resolution=20, num_classes=2, synthetic_length=4)
    with pytest.raises(ValueError, match="uint8 images"):
        make_dataloader("synthetic", training=True, auto_augment="original", **common)
    U.seed_all(0)
    raw, labels = next(iter(make_dataloader("synthetic_images", training=True, auto_augment="original", **common)))
    assert tuple(raw.aug_ops.shape) == (2, 8) and tuple(raw.aug_args.shape) == (2, 8, 6)
    raw, labels = next(iter(make_dataloader("synthetic_images", training=False, auto_augment="original", **common)))
    assert raw.aug_ops is None
    raw, labels = next(iter(make_dataloader("synthetic_images", training=True, **common)))
    assert raw.aug_ops is None
