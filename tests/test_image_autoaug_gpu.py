"""GPU: the image evals' AutoAugment on the device against tests/golden/image_autoaug_micro.npz (PIL's bytes through the reference's
own operation functions, tools/make_golden_image_autoaug.py): vj_image_hflip, vj_clip_randaug_fill, the staged batch of
engine.input.ImagePrefetcher and both image evals with `data.auto_augment`.  No tolerance anywhere: uint8 is compared with ==, fp32
bit for bit.  The fixture is all these tests read; Pillow is not needed."""
import numpy as np
import pytest
import torch

from tests import image_autoaug_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def z():
    return np.load(U.GOLDEN)


def _desc(B, S, flips):
    return torch.tensor([[b * S * S * 3, S, S, int(f)] for b, f in zip(range(B), flips)], dtype=torch.int64).reshape(B, 4)


@pytest.fixture
def launched(monkeypatch):
    """The names that go through the wrappers' launch path while the test runs."""
    from jepa_amd.hip import ops
    names, real = [], ops._launch

    def recording(name, *a, **kw):
        names.append(name)
        return real(name, *a, **kw)

    monkeypatch.setattr(ops, "_launch", recording)
    return names


@pytest.mark.parametrize("S", [4, 20, 36])
def test_image_hflip_mirrors_the_flagged_images_only(S, launched):
    from jepa_amd.hip import ops
    rng = np.random.RandomState(S)
    B, guard = 5, 64
    flips = [True, False, True, True, False]
    host = rng.randint(0, 256, size=guard + B * S * S * 3 + guard).astype(np.uint8)
    whole = torch.from_numpy(host).to(DEV)
    images = whole[guard:guard + B * S * S * 3].view(B, S, S, 3)
    assert images.data_ptr() % 16 == 0
    out = ops.image_hflip(images, _desc(B, S, flips).to(DEV), flips)
    torch.cuda.synchronize()
    assert out.data_ptr() == images.data_ptr() and launched == ["vj_image_hflip"]
    got = whole.cpu().numpy()
    assert np.array_equal(got[:guard], host[:guard]) and np.array_equal(got[-guard:], host[-guard:])
    before, after = host[guard:-guard].reshape(B, S, S, 3), got[guard:-guard].reshape(B, S, S, 3)
    for b, f in enumerate(flips):
        assert np.array_equal(after[b], np.flip(before[b], axis=1) if f else before[b]), b


def test_image_hflip_launches_nothing_without_a_flagged_image_and_refuses_bad_dims(launched):
    from jepa_amd.hip import ops
    from jepa_amd.hip.lib import load_library
    S = 8
    images = torch.arange(3 * S * S * 3, dtype=torch.int32).to(torch.uint8).view(3, S, S, 3).to(DEV)
    before = images.clone()
    ops.image_hflip(images, _desc(3, S, [0, 0, 0]).to(DEV), [False, False, False])
    ops.image_hflip(images[:0], torch.zeros((0, 4), dtype=torch.int64, device=DEV), [])
    torch.cuda.synchronize()
    assert launched == [] and torch.equal(images, before)
    lib = load_library()
    assert lib.vj_image_hflip(None, None, 0, 8, 0, None) == 0 and lib.vj_image_hflip(None, None, 4, 8, 0, None) == 0
    assert lib.vj_image_hflip(None, None, 1, 6, 1, None) < 0 and b"multiple of 4" in lib.vj_last_error()
    assert lib.vj_image_hflip(None, None, 1, 0, 1, None) < 0 and b"bad dims" in lib.vj_last_error()
    assert lib.vj_image_hflip(None, None, 40000, 224, 1, None) < 0 and b"2^31" in lib.vj_last_error()
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.image_hflip(torch.zeros((1, 6, 6, 3), dtype=torch.uint8, device=DEV), _desc(1, 6, [1]).to(DEV), [True])
    big = torch.zeros(1, dtype=torch.uint8, device=DEV).expand(14267, 224, 224, 3)      # 14267 * 224 * 224 * 3 >= 2^31: no memory behind it
    with pytest.raises(ValueError, match="2.31"):
        ops.image_hflip(big, torch.zeros((14267, 4), dtype=torch.int64, device=DEV), [True] * 14267)
    with pytest.raises(ValueError, match="host flags"):
        ops.image_hflip(images, _desc(3, S, [0, 0, 0]).to(DEV), [True])
    assert launched == []


@pytest.mark.parametrize("S", U.SIDES)
def test_every_fixture_case_byte_for_byte(z, S, launched):
    """ops.clip_randaug(..., fill=(124, 116, 104)) on all cases of one side in ONE batch of one-frame clips: unflipped sources
    directly, flipped ones after image_hflip.  S = 20, 36: partial 16-wide tiles and unaligned 12-byte reads at the row ends;
    S = 96: whole tiles and histogram bins far above 255 counts."""
    from jepa_amd.hip import ops
    cs = U.cases(z, S)
    B = len(cs)
    flips = [c[2] for c in cs]
    images = torch.from_numpy(np.stack([c[1] for c in cs])).to(DEV)
    desc = _desc(B, S, flips).to(DEV)
    ops.image_hflip(images, desc, flips)
    aug_ops = torch.from_numpy(np.stack([c[3] for c in cs]))
    aug_args = torch.from_numpy(np.stack([c[4] for c in cs]))
    live = (aug_ops != 0).any(0)
    assert int(live.sum()) == 2
    ops.clip_randaug(images.view(-1), desc, 1, aug_ops[:, live].contiguous().to(DEV), aug_args[:, live].contiguous().to(DEV), fill=U.FILL)
    torch.cuda.synchronize()
    assert launched == ["vj_image_hflip", "vj_clip_randaug_fill"]
    got = images.cpu().numpy()
    wrong = [(c[0], int((got[b] != c[5]).sum())) for b, c in enumerate(cs) if not np.array_equal(got[b], c[5])]
    assert not wrong, wrong


def test_fill_keyword_none_is_the_old_entry_and_the_colour_reaches_the_pixels(z, launched):
    """A translate by a third of the side: the uncovered band is the colour given, and (128, 128, 128) through the old entry."""
    from jepa_amd.hip import ops
    S = 20
    src = torch.from_numpy(z["src_20"][:1].copy())
    desc = _desc(1, S, [0]).to(DEV)
    aug_ops = torch.tensor([[14]], dtype=torch.int32, device=DEV)
    aug_args = torch.tensor([[[1, 0, 7.0, 0, 1, 0]]], dtype=torch.float64, device=DEV)
    outs = {}
    for fill in (None, U.FILL, (128, 128, 128), (0, 255, 7)):
        buf = src.clone().to(DEV)
        ops.clip_randaug(buf.view(-1), desc, 1, aug_ops, aug_args, fill=fill)
        outs[fill] = buf.cpu().numpy()[0]
    assert launched == ["vj_clip_randaug"] + ["vj_clip_randaug_fill"] * 3
    assert np.array_equal(outs[None], outs[(128, 128, 128)])
    for fill in (U.FILL, (0, 255, 7)):
        assert (outs[fill][:, -7:] == np.array(fill, np.uint8)).all() and (outs[None][:, -7:] == 128).all()
        assert np.array_equal(outs[fill][:, :-7], outs[None][:, :-7])
    for bad in ((1, 2), (1, 2, 256), (-1, 0, 0), (1.5, 0, 0)):
        with pytest.raises(ValueError, match="three bytes"):
            ops.clip_randaug(src.clone().to(DEV).view(-1), desc, 1, aug_ops, aug_args, fill=bad)


def _reference_chain(z, items):
    """The existing chain on PIL's expected bytes uploaded as a [B,S,S,3] buffer: vj_clip_transform_pre with no flip, vj_clip_erase."""
    from jepa_amd.evals.image_classification_frozen.transforms import collate_raw_images
    from jepa_amd.hip import ops
    raw = collate_raw_images(items)
    B, S = len(raw), raw.crop_size
    u8 = torch.from_numpy(z["batch/out"].copy()).to(DEV)
    desc, boxes = raw.resampled_tables()
    desc[:, 3] = 0
    out = ops.clip_transform(u8.view(-1), desc.to(DEV), boxes.to(DEV), S, raw.mean, raw.std, pre=True)
    assert raw.erased
    ops.clip_erase(out, raw.ebox.to(DEV), raw.noise.to(DEV), raw.noise_off.to(DEV))
    torch.cuda.synchronize()
    return out.view(B, 3, S, S).cpu().numpy()


def _staged(items, rounds=3):
    from jepa_amd.engine.input import ImagePrefetcher
    from jepa_amd.evals.image_classification_frozen.transforms import collate_raw_images
    labels = torch.arange(len(items))
    pf = ImagePrefetcher([(collate_raw_images(items), labels) for _ in range(rounds)], DEV)
    outs = [imgs.cpu().numpy() for imgs, _ in pf]
    assert len(outs) == rounds
    for o in outs[1:]:
        assert np.array_equal(o.view(np.uint32), outs[0].view(np.uint32))       # both slots, and a slot used again
    return outs[0]


def test_staged_batch_equals_the_chain_on_pils_bytes_bit_for_bit(z, launched):
    want = _reference_chain(z, U.batch_items(z))
    del launched[:]
    got = _staged(U.batch_items(z), rounds=1)
    assert launched == ["vj_image_resample", "vj_image_hflip", "vj_clip_randaug_fill", "vj_clip_transform_pre", "vj_clip_erase"]
    assert got.shape == want.shape == (6, 3, 20, 20)
    for k in range(len(got)):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    _staged(U.batch_items(z), rounds=3)


def test_zeroed_plans_are_the_batch_without_plan_tables(z, launched):
    plain = _staged(U.batch_items(z, with_plans=False), rounds=1)
    names_plain = list(launched)
    del launched[:]
    zeroed = _staged(U.batch_items(z, zero_plans=True), rounds=1)
    assert np.array_equal(zeroed.view(np.uint32), plain.view(np.uint32))
    assert launched == names_plain == ["vj_image_resample", "vj_clip_transform_pre", "vj_clip_erase"]
    # and the late flip is the early one: the augmented batch differs from it only where a plan has an operation
    full = _staged(U.batch_items(z), rounds=1)
    same = [k for k in range(len(full)) if np.array_equal(full[k].view(np.uint32), plain[k].view(np.uint32))]
    assert same == [k for k in range(len(full)) if not z["batch/ops"][k].any()] and len(same) == 1


# ---------------------------------------------------------------------------------------------------------------------- the evals

def _cfg(folder, auto_augment, **over):
    cfg = {
        'pretrain': {'model_name': 'vit_tiny', 'checkpoint_key': 'target_encoder', 'patch_size': 16, 'folder': folder,
                     'checkpoint': 'tiny-latest.pth.tar', 'write_tag': 'tiny', 'tubelet_size': 2, 'frames_per_clip': 8,
                     'uniform_power': True, 'use_sdpa': True, 'use_silu': False, 'tight_silu': False},
        'data': {'dataset_name': 'synthetic_images', 'num_classes': 2, 'root_path': None, 'image_folder': None, 'resolution': 32,
                 'synthetic_length': 48, 'auto_augment': auto_augment},
        'optimization': {'batch_size': 8, 'num_epochs': 1, 'weight_decay': 0.01, 'start_lr': 0.001, 'lr': 0.001, 'final_lr': 0.0,
                         'warmup': 0.0, 'use_bfloat16': False},
        'tag': 'autoaug_eval',
    }
    for k, v in over.items():
        cfg[k].update(v)
    return cfg


def _checkpoint(tmp_path):
    from jepa_amd.src.models import vision_transformer as vit
    torch.manual_seed(1)
    enc = vit.vit_tiny(img_size=32, patch_size=16, num_frames=8, tubelet_size=2, uniform_power=True)
    torch.save({'target_encoder': {'module.backbone.' + k: v for k, v in enc.state_dict().items()}, 'epoch': 10},
               tmp_path / 'tiny-latest.pth.tar')


def _check_run(rec, tmp_path, launched, sub):
    assert len(rec['train_history']) == 6 and all(np.isfinite(ls) for _, ls in rec['train_history'])
    assert np.isfinite(rec['train_acc'] + rec['val_acc']).all()
    assert "vj_image_hflip" in launched and "vj_clip_randaug_fill" in launched and "vj_clip_randaug" not in launched
    written = list((tmp_path / sub).glob("**/*latest.pth.tar"))
    assert written, list(tmp_path.rglob("*"))


def test_frozen_eval_with_auto_augment(tmp_path, launched):
    from jepa_amd.evals.image_classification_frozen import eval as E
    _checkpoint(tmp_path)
    U.seed_all(0)
    _check_run(E.main(_cfg(str(tmp_path), 'original')), tmp_path, launched, 'image_classification_frozen')


@pytest.mark.parametrize("auto_augment,mix", [('original', False), ('original', True), ('rand-m9-mstd0.5-inc1', False)],
                         ids=["original", "original-mix", "rand"])
def test_finetune_eval_with_auto_augment(tmp_path, launched, auto_augment, mix):
    from jepa_amd.evals.image_classification_finetune import eval as FT
    _checkpoint(tmp_path)
    ft = {'encoder_lr': 0.0001, 'drop_path': 0.1}
    if mix:
        ft['mix'] = {'mixup_alpha': 0.8, 'cutmix_alpha': 1.0, 'prob': 1.0, 'switch_prob': 0.5, 'label_smoothing': 0.1}
    U.seed_all(0)
    rec = FT.main(_cfg(str(tmp_path), auto_augment, optimization={'finetune': ft}))
    _check_run(rec, tmp_path, launched, 'image_classification_finetune')
    assert ("vj_clip_mix" in launched) == mix
