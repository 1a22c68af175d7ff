"""CPU: the host half of the device-side RandAugment.  `RandAugmentDraw` (jepa_amd/app/vjepa/randaugment.py) against the plans and
the generator states that the reference's own module left in tests/golden/randaug_micro.npz (tools/make_golden_randaug.py), its
parser, the plan's way through RawClip / collate / RawClipBatch.validate, the eval's VideoTransform with and without the
`rand_augment` attribute, the numpy restatement of the device arithmetic (tests/randaug_util.py) against the reference's augmented
frames, and the argument checks of vj_clip_randaug (no launch: there is no GPU here)."""
import importlib.util
import os
import random
import warnings

import numpy as np
import pytest
import torch

from . import eval_transform_util as EU
from . import randaug_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with warnings.catch_warnings():
    warnings.simplefilter("ignore")          # `reference` is not a registered marker: the pytest settings are not this file's to change
    reference = pytest.mark.reference


def _next_draws():
    return np.array([random.random(), np.random.uniform(), float(torch.rand(1, dtype=torch.float64))], dtype=np.float64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_draws_reproduce_every_fixture_plan():
    from jepa_amd.app.vjepa.randaugment import RandAugmentDraw
    z = U.fixture()
    seen = set()
    for n in U.names():
        T, H, W, _ = z[f"{n}/frames"].shape
        U.seed_all(int(z[f"{n}/seed"]))
        ops, args = RandAugmentDraw(str(z[f"{n}/config"])).draw(H, W)
        assert ops.dtype == np.int32 and ops.shape == (8,) and args.dtype == np.float64 and args.shape == (8, 6)
        assert np.array_equal(ops, z[f"{n}/ops"]), (n, ops, z[f"{n}/ops"])
        assert np.array_equal(_bits(args), _bits(z[f"{n}/args"])), (n, args, z[f"{n}/args"])
        if n not in z["train_names"]:           # (the train cases go on drawing: below)
            assert np.array_equal(_bits(_next_draws()), _bits(z[f"{n}/next"])), n
        seen.update(int(v) for v in ops)
    assert seen == set(range(16))


def test_parser():
    from jepa_amd.app.vjepa import randaugment as R
    d = R.RandAugmentDraw()
    assert (d.magnitude, d.num_layers, d.magnitude_std, d.increasing) == (7, 4, 0.5, True)
    d = R.RandAugmentDraw('rand-m9-n3-mstd0.5')
    assert (d.magnitude, d.num_layers, d.magnitude_std, d.increasing) == (9, 3, 0.5, False)
    assert R.RandAugmentDraw('rand-m9-inc0').increasing            # the reference's quirk: bool("0") is true
    d = R.RandAugmentDraw('rand')
    assert (d.magnitude, d.num_layers, d.magnitude_std, d.increasing) == (10.0, 2, 0, False)
    assert R.RandAugmentDraw('rand-n8').num_layers == 8
    with pytest.raises(NotImplementedError, match="w"):
        R.RandAugmentDraw('rand-m9-w0')
    with pytest.raises(ValueError, match="n=9"):
        R.RandAugmentDraw('rand-m9-n9')
    with pytest.raises(ValueError):
        R.RandAugmentDraw('augmix-m3')
    # the increasing and the plain list: the same draws, other arguments (randaugment.py:229-259)
    for inc, bits, thresh in ((True, 4 - 2, 256 - 179), (False, 2, 179)):
        d = R.RandAugmentDraw('rand-m7-n2' + ('-inc1' if inc else ''))
        assert d._level(R.POSTERIZE, 7, 20, 20) == (bits,) and d._level(R.SOLARIZE, 7, 20, 20) == (thresh,)
    assert R.RandAugmentDraw('rand-m7')._level(R.COLOR, 7, 20, 20) == ((7 / 10.0) * 1.8 + 0.1,)
    assert R.rotation_coefficients(0.0, 20, 30) is None and R.rotation_coefficients(360.0, 20, 30) is None
    assert R.rotation_coefficients(90.0, 20, 30) == pytest.approx((0, -1, 25, 1, 0, -5))


def _clip(hw=(20, 24), T=2, plan=None, S=16):
    from jepa_amd.app.vjepa.transforms import RawClip
    g = torch.Generator().manual_seed(hw[0] * 100 + hw[1])
    frames = torch.randint(0, 256, (T, hw[0], hw[1], 3), generator=g, dtype=torch.uint8)
    boxes = torch.tensor([0, 0, hw[0], hw[1]], dtype=torch.int32).repeat(T, 1)
    ops, args = plan if plan is not None else (None, None)
    return RawClip(frames, boxes, False, S, (0.5, 0.5, 0.5), (0.25, 0.25, 0.25), pre=True, aug_ops=ops, aug_args=args)


def _plan(*codes):
    ops, args = np.zeros(8, dtype=np.int32), np.zeros((8, 6), dtype=np.float64)
    ops[:len(codes)] = codes
    args[:, 0] = 1.5
    return ops, args


def test_collate_packs_plans_and_leaves_clips_without_one_alone():
    from jepa_amd.app.vjepa.transforms import collate_raw_clips
    a, b, c = _clip((20, 24), plan=_plan(3, 0, 10)), _clip((17, 19)), _clip((30, 21), plan=_plan(0, 0, 0, 0))
    batch = collate_raw_clips([a, b, c])
    assert batch.aug_ops.dtype == torch.int32 and tuple(batch.aug_ops.shape) == (3, 8)
    assert batch.aug_args.dtype == torch.float64 and tuple(batch.aug_args.shape) == (3, 8, 6)
    assert batch.aug_ops.tolist() == [[3, 0, 10, 0, 0, 0, 0, 0], [0] * 8, [0] * 8]
    assert torch.equal(batch.aug_args[0], a.aug_args) and not batch.aug_args[1].any()
    assert batch.augmented
    plain = collate_raw_clips([_clip((20, 24)), _clip((17, 19))])
    assert plain.aug_ops is None and plain.aug_args is None and not plain.augmented      # absent means no work, as ebox / noise
    assert not collate_raw_clips([c, _clip((17, 19))]).augmented                          # a plan of zeros is no work either
    with pytest.raises(ValueError, match="come together"):
        _clip(plan=(np.zeros(8, dtype=np.int32), None))


def test_validate_refuses_bad_plans():
    from jepa_amd.app.vjepa.transforms import RawClip, collate_raw_clips

    def batch(*clips):
        return collate_raw_clips(list(clips))

    ok = batch(_clip(plan=_plan(1, 15)), _clip((17, 19)))
    assert ok.validate() is ok
    bad = batch(_clip(plan=_plan(1, 15)), _clip((17, 19)))
    bad.aug_ops[0, 1] = 16
    with pytest.raises(ValueError, match="unknown RandAugment operation"):
        bad.validate()
    bad.aug_ops[0, 1] = -1
    with pytest.raises(ValueError, match="unknown RandAugment operation"):
        bad.validate()
    for v in (float("nan"), float("inf")):
        bad = batch(_clip(plan=_plan(8)), _clip((17, 19)))
        bad.aug_args[0, 0, 0] = v
        with pytest.raises(ValueError, match="non-finite"):
            bad.validate()
    with pytest.raises(ValueError, match="side below 3"):
        batch(_clip((2, 24), plan=_plan(11)))
    batch(_clip((2, 24), plan=_plan(0)))                                  # a clip without an operation may be that small
    bad = batch(_clip(plan=_plan(1, 15)), _clip((17, 19)))
    bad.aug_args = bad.aug_args.to(torch.float32)
    with pytest.raises(ValueError, match="malformed RandAugment tables"):
        bad.validate()
    bad = batch(_clip(plan=_plan(1, 15)), _clip((17, 19)))
    bad.aug_args = None
    with pytest.raises(ValueError, match="come together"):
        bad.validate()
    # two views of one clip share its frames: the in-place pass must not be given them
    c = _clip((16, 30), plan=_plan(3))
    two = RawClip(c.frames, c.boxes[None].repeat(2, 1, 1), False, 16, c.mean, c.std, pre=True, aug_ops=c.aug_ops, aug_args=c.aug_args)
    with pytest.raises(ValueError, match="shares its byte offset"):
        batch(two)
    two = RawClip(c.frames, c.boxes[None].repeat(2, 1, 1), False, 16, c.mean, c.std, pre=True, aug_ops=_plan(0)[0], aug_args=_plan(0)[1])
    assert len(batch(two)) == 2


def _eval_transform(name, z, rand_augment):
    from jepa_amd.app.vjepa.randaugment import RandAugmentDraw
    from jepa_amd.evals.video_classification_frozen.utils import make_transforms
    tf = make_transforms(training=True, reprob=float(z[f"{name}/reprob"]), crop_size=int(z[f"{name}/side"]))
    assert tf.rand_augment is None
    if rand_augment:
        tf.rand_augment = RandAugmentDraw(str(z[f"{name}/config"]))
    return tf


def test_eval_transform_draws_the_plan_first():
    """The eval's training transform with `rand_augment` set: plan, boxes, flip, erase box and noise, and the state of all three
    generators afterwards, are the reference's VideoTransform(training=True, auto_augment=True)'s."""
    z = U.fixture()
    assert len(z["train_names"]) >= 3
    for n in (str(v) for v in z["train_names"]):
        tf = _eval_transform(n, z, True)
        U.seed_all(int(z[f"{n}/seed"]))
        clip = tf(z[f"{n}/frames"])
        nxt = _next_draws()
        assert np.array_equal(clip.aug_ops.numpy(), z[f"{n}/ops"]) and np.array_equal(_bits(clip.aug_args.numpy()), _bits(z[f"{n}/args"]))
        assert np.array_equal(clip.boxes.numpy(), z[f"{n}/boxes"]) and clip.flip == bool(z[f"{n}/flip"]), n
        assert clip.pre and np.array_equal(clip.frames.numpy(), z[f"{n}/frames"])         # the frames go on untouched
        if float(z[f"{n}/reprob"]) > 0:
            assert list(clip.ebox) == z[f"{n}/ebox"].tolist() and np.array_equal(clip.noise.numpy(), z[f"{n}/noise"])
        else:
            assert clip.noise is None
        assert np.array_equal(_bits(nxt), _bits(z[f"{n}/next"])), n
        tf.training = False                                                               # validation never augments


def test_eval_transform_without_the_attribute_draws_what_it_drew_before():
    """`rand_augment` unset: exactly the draws of tests/golden/eval_transform_micro.npz, and no plan on the clip."""
    z = EU.fixture()
    for n in EU.names("train"):
        clip = EU.train_clip(n)
        nxt = _next_draws()
        assert clip.aug_ops is None and clip.aug_args is None
        assert np.array_equal(clip.boxes.numpy(), z[f"{n}/boxes"]) and clip.flip == bool(z[f"{n}/flip"])
        assert list(clip.ebox) == z[f"{n}/ebox"].tolist()
        assert np.array_equal(_bits(nxt), _bits(z[f"{n}/next"])), n


def test_make_transforms_still_refuses_auto_augment():
    from jepa_amd.app.vjepa.transforms import make_transforms as pretrain_transforms
    from jepa_amd.evals.video_classification_frozen.utils import make_transforms
    for mk in (pretrain_transforms, make_transforms):
        with pytest.raises(NotImplementedError, match="RandAugment"):
            mk(auto_augment=True)


def test_make_dataloader_sets_the_attribute_only_when_asked():
    from jepa_amd.app.vjepa.randaugment import RandAugmentDraw
    from jepa_amd.app.vjepa.transforms import RawClipBatch
    from jepa_amd.evals.video_classification_frozen.eval import make_dataloader
    kw = dict(root_path=[None], batch_size=3, world_size=1, rank=0, dataset_type="synthetic_frames", resolution=32, frames_per_clip=4,
              num_segments=2, num_classes=5, synthetic_length=6, num_workers=0)
    assert make_dataloader(training=True, **kw).dataset.transform.rand_augment is None
    assert make_dataloader(training=False, rand_augment=True, **kw).dataset.transform.rand_augment is None
    loader = make_dataloader(training=True, rand_augment=True, **kw)
    ra = loader.dataset.transform.rand_augment
    assert isinstance(ra, RandAugmentDraw) and ra.config_str == 'rand-m7-n4-mstd0.5-inc1'
    U.seed_all(3)
    segments, labels, idx = next(iter(loader))
    assert len(segments) == 2 and all(isinstance(s, RawClipBatch) and tuple(s.aug_ops.shape) == (3, 8) for s in segments)
    assert any(s.augmented for s in segments)
    with pytest.raises(ValueError, match="rand_augment"):
        make_dataloader(training=True, rand_augment=True, **dict(kw, dataset_type="synthetic"))


def test_restatement_of_the_device_arithmetic_gives_the_reference_frames():
    """tests/randaug_util.py restate() -- the arithmetic csrc/clip_randaug.hip implements, in numpy -- against PIL's output for every
    fixture case: equal bytes."""
    z = U.fixture()
    for n in U.names():
        got = U.restate(z[f"{n}/frames"], z[f"{n}/ops"], z[f"{n}/args"])
        assert got.dtype == np.uint8 and np.array_equal(got, z[f"{n}/aug"]), (n, int((got != z[f"{n}/aug"]).sum()))


def test_entry_point_checks_its_arguments_on_the_host():
    from jepa_amd.hip import lib as L
    from jepa_amd.hip import ops
    lib = L.load_library()
    assert lib.vj_clip_randaug_ws_bytes(1000, 2, 4) == 1024 + 2 * 4 * 768 and lib.vj_clip_randaug_ws_bytes(-1, 2, 4) < 0
    assert lib.vj_clip_randaug(None, 0, None, 0, 4, None, None, 4, None, 0, None) == 0          # an empty batch launches nothing
    assert lib.vj_clip_randaug(None, 100, None, 2, 4, None, None, 0, None, 0, None) == 0        # no layer either
    for args in ((None, 100, None, 2, 0, None, None, 4, None, 0, None), (None, -1, None, 2, 4, None, None, 4, None, 0, None),
                 (None, 1 << 31, None, 2, 4, None, None, 4, None, 0, None), (None, 100, None, 65536, 4, None, None, 4, None, 0, None)):
        assert lib.vj_clip_randaug(*args) < 0 and b"vj_clip_randaug: bad dims" in lib.vj_last_error()
    assert lib.vj_clip_randaug(None, 100, None, 2, 4, None, None, 9, None, 0, None) < 0 and b"at most 8" in lib.vj_last_error()
    assert lib.vj_clip_randaug(None, 100, None, 2, 4, None, None, 4, None, 0, None) < 0 and b"null pointer" in lib.vj_last_error()
    frames, desc = torch.zeros(64, dtype=torch.uint8), torch.zeros((1, 4), dtype=torch.int64)
    with pytest.raises(ValueError, match="GPU"):                                                # no CPU path
        ops.clip_randaug(frames, desc, 2, torch.zeros((1, 8), dtype=torch.int32), torch.zeros((1, 8, 6), dtype=torch.float64))


@reference
@pytest.mark.skipif(not os.environ.get("JEPA_REFERENCE") or importlib.util.find_spec("PIL") is None,
                    reason="needs JEPA_REFERENCE (a checkout of the reference) and PIL")
def test_draws_against_the_live_reference():
    """200 further seeds: plan and following draws of RandAugmentDraw against the reference's module run on small frames, and the
    numpy restatement of the pixels against what PIL made of them."""
    from jepa_amd.app.vjepa.randaugment import RandAugmentDraw
    spec = importlib.util.spec_from_file_location("make_golden_randaug", os.path.join(ROOT, "tools", "make_golden_randaug.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    R = tool.Reference(os.environ["JEPA_REFERENCE"])
    try:
        for seed in range(1000, 1200):
            config = tool.CONFIGS[seed % len(tool.CONFIGS)]
            hw = tool.SIZES[seed % len(tool.SIZES)]
            frames = tool.frames_for(f"live{seed}", hw, 2, tool.KINDS[seed % len(tool.KINDS)])
            ops, args, _, aug, nxt = R.run_aug(config, frames, seed)
            U.seed_all(seed)
            mine = RandAugmentDraw(config).draw(*hw)
            assert np.array_equal(mine[0], ops) and np.array_equal(_bits(mine[1]), _bits(args)), seed
            assert np.array_equal(_bits(_next_draws()), _bits(nxt)), seed
            assert np.array_equal(U.restate(frames, ops, args), aug), seed
    finally:
        R.rec.close()
