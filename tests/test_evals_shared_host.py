"""CPU checks of what the frozen evals share (jepa_amd/evals/frozen.py) and of the synthetic classification datasets
(src/datasets/data_manager.py): the items are pinned by digest, the `module.` prefix convention of the checkpoints round-trips,
the probe update is the written-out sequence, and the shared config parser answers the evals' defaults."""
import hashlib

import numpy as np
import pytest
import torch

# sha256 of (item bytes, label, index tables) of items 0, 1 and 5 at crop 16, 2 frames, 2 segments, 3 classes, per split seed: the
# three datasets share one label draw, one class wave and one index table, and the evals' committed records depend on every byte
PINS = {
    ("video", 0): ["6326e263f1ecf6bc21d300eb0749d24e629923f76f2e298b52992b8ad1315a3d",
                   "7f2180c5e63c4a8bfb2e48e19cf9609e59aa35e2d63fdf1388f3d12cf562edc2",
                   "92c202426eb8e0995a1d3e4a6f3bd186d19a53abe4b5ea8c844029d2a282027d"],
    ("video", 1): ["ab036b70a5f30b0702afa0d94da3f96c7f2966391942d1d9effcff0da92eab8f",
                   "fae615cc547f3634bcb8106848df354d256d1acb7833aec0deaf91695cbe7bad",
                   "be3c878f373da970eaf6ce512ba4c5562337bd759aab731db26d1086c6bb9e19"],
    ("frames", 0): ["e7c46727715f71e2601e28ffa1ff44d0df5eea64bd3390a90075cc030ffc2174",
                    "9c8112b73e80ca013b0b461d893fb27ca9a798de009ddcafc06350c0509a14e4",
                    "273b09d2f012acf5bbfb4721afcaa8c43fd7b59a968c5b09bdf0a4097ebe27b8"],
    ("frames", 1): ["01107b45d9f49aa20bc80111f1695c689a059918f44d2f44f4be310eb1e34f5b",
                    "b005e6c37991be1c58a5241ecc9cba4429cef044e751b48fc17c50b1e8e57ae3",
                    "a64603699ac48635ff6d62489eaca28a772bdfa24fb18a0054be2bc1e107eeda"],
    ("image", 0): ["16ad2bf263612f89499973643ffacefc300e2935fb454b6c43bfe4d98289442a",
                   "479843cb07840ca76266f7d885aed43268c2084e33892ad0472c761b32f50427",
                   "57c19fadd93dad14b86fd60e3da533d430c9612c64b339f0f48059b2131b64dc"],
    ("image", 1): ["2f861022311551fc870d2c670545e3ba0008db5f362ce20d86e766833bd16d14",
                   "4b3c2f8f3751ce2059ce3f9ba1b90e9e961fbcf7ae470e17b9edb23821e2ab22",
                   "83daef7855c6693c54ec1cbe34f34161f5cc353a7b454b339f0b12e22a1a3ca0"],
}


def _digest(item):
    h = hashlib.sha256()

    def feed(x):
        if isinstance(x, (list, tuple)):
            h.update(b"[%d" % len(x))
            for e in x:
                feed(e)
        elif isinstance(x, (torch.Tensor, np.ndarray)):
            a = x.contiguous().numpy() if isinstance(x, torch.Tensor) else np.ascontiguousarray(x)
            h.update(f"{a.dtype}{a.shape}".encode())
            h.update(a.tobytes())
        else:
            h.update(repr(x).encode())

    feed(item)
    return h.hexdigest()


def _dataset(kind, seed):
    from jepa_amd.src.datasets import data_manager as dm
    if kind == "video":
        return dm.SyntheticVideoClassification(8, 3, 2, 16, num_segments=2, num_views_per_segment=2, frame_step=4, seed=seed)
    if kind == "frames":    # as the eval's loader builds its splits: any source size to train (seed 0), a fixed short side to validate
        return dm.SyntheticFramesClassification(8, 3, 2, 16, lambda frames: frames, num_segments=2,
                                                short_side=None if seed == 0 else 18, frame_step=4, seed=seed)
    return dm.SyntheticImageClassification(8, 3, 16, seed=seed)


@pytest.mark.parametrize("kind,seed", sorted(PINS))
def test_dataset_items_are_pinned(kind, seed):
    ds = _dataset(kind, seed)
    got = [_digest(ds[i]) for i in (0, 1, 5)]
    print(kind, seed, got)
    assert got == PINS[(kind, seed)]


class _Bank(torch.nn.Module):
    """What multihead.load_checkpoint reads of a probe bank: `.probes`."""

    def __init__(self, P):
        super().__init__()
        self.probes = torch.nn.ModuleList([torch.nn.Linear(4, 3) for _ in range(P)])


def _state(m):
    return {k: v.clone() for k, v in m.state_dict().items()}


def _same(m, state):
    return all(torch.equal(v, state[k]) for k, v in m.state_dict().items())


def test_checkpoint_prefix_round_trip(tmp_path):
    from jepa_amd.evals import frozen, multihead
    from jepa_amd.evals.image_classification_frozen import eval as EI
    from jepa_amd.evals.video_classification_frozen import eval as EV
    assert EV.classifier_state_dict is frozen.classifier_state_dict and EI.load_checkpoint is frozen.load_checkpoint
    torch.manual_seed(0)
    src = torch.nn.Linear(4, 3)
    saved = frozen.classifier_state_dict(src)
    assert list(saved) == ['module.weight', 'module.bias'] and all(k.startswith('module.') for k in saved)
    assert all(torch.equal(saved['module.' + k], v) for k, v in src.state_dict().items())
    assert list(frozen.strip_module_prefix(saved)) == ['weight', 'bias']
    assert list(frozen.strip_module_prefix({'weight': 0, 'module.module.bias': 1})) == ['weight', 'module.bias']

    # the single-probe form into a plain module
    opt = torch.optim.AdamW(src.parameters(), lr=0.1)
    src(torch.randn(2, 4)).sum().backward()
    opt.step()
    path = str(tmp_path / "single.pth.tar")
    torch.save({'classifier': frozen.classifier_state_dict(src), 'opt': opt.state_dict(), 'scaler': None, 'epoch': 3}, path)
    dst = torch.nn.Linear(4, 3)
    dst_opt = torch.optim.AdamW(dst.parameters(), lr=0.5)
    m, o, s, epoch = frozen.load_checkpoint(device='cpu', r_path=path, classifier=dst, opt=dst_opt, scaler=None)
    assert m is dst and o is dst_opt and s is None and epoch == 3
    assert _same(dst, src.state_dict()) and dst_opt.param_groups[0]['lr'] == 0.1

    # the per-probe list form
    bank = _Bank(2)
    opts = [torch.optim.AdamW(p.parameters(), lr=0.1 * (i + 1)) for i, p in enumerate(bank.probes)]
    path = str(tmp_path / "bank.pth.tar")
    torch.save({'classifier': [frozen.add_module_prefix(p.state_dict()) for p in bank.probes],
                'opt': [o.state_dict() for o in opts], 'scaler': [None, None], 'epoch': 2}, path)
    other = _Bank(2)
    other_opts = [torch.optim.AdamW(p.parameters(), lr=0.7) for p in other.probes]
    assert multihead.load_checkpoint(path, other, other_opts, [None, None]) == 2
    assert all(_same(a, b.state_dict()) for a, b in zip(other.probes, bank.probes))
    assert [o.param_groups[0]['lr'] for o in other_opts] == [0.1, 0.2]

    # the wrong probe count, or no file: epoch 0 and nothing touched
    three = _Bank(3)
    before = [_state(p) for p in three.probes]
    three_opts = [torch.optim.AdamW(p.parameters(), lr=0.7) for p in three.probes]
    assert multihead.load_checkpoint(path, three, three_opts, [None] * 3) == 0
    assert multihead.load_checkpoint(str(tmp_path / "none.pth.tar"), three, three_opts, [None] * 3) == 0
    assert all(_same(p, b) for p, b in zip(three.probes, before)) and all(o.param_groups[0]['lr'] == 0.7 for o in three_opts)
    lone = torch.nn.Linear(4, 3)
    before = _state(lone)
    lone_opt = torch.optim.AdamW(lone.parameters(), lr=0.7)
    assert frozen.load_checkpoint(device='cpu', r_path=str(tmp_path / "none.pth.tar"), classifier=lone, opt=lone_opt,
                                  scaler=None)[3] == 0
    assert frozen.load_checkpoint(device='cpu', r_path=path, classifier=lone, opt=lone_opt, scaler=None)[3] == 0   # lists: no keys
    assert _same(lone, before) and lone_opt.param_groups[0]['lr'] == 0.7


def test_probe_update_is_the_written_out_sequence():
    from jepa_amd.evals import frozen
    torch.manual_seed(0)
    mine, ref = torch.nn.Linear(6, 4), torch.nn.Linear(6, 4)
    ref.load_state_dict(mine.state_dict())
    opt_mine, opt_ref = (torch.optim.AdamW(m.parameters(), lr=0.05, weight_decay=0.1) for m in (mine, ref))
    criterion = torch.nn.CrossEntropyLoss()
    for _ in range(2):
        x, labels = 30.0 * torch.randn(5, 6), torch.randint(0, 4, (5,))          # large inputs: the clip to norm 1.0 acts
        frozen.probe_update(mine, opt_mine, None, False, loss=criterion(mine(x), labels))
        assert all(p.grad is None for p in mine.parameters())
        loss = criterion(ref(x), labels)
        loss.backward()
        assert float(torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)) > 1.0
        opt_ref.step()
        opt_ref.zero_grad()
    assert all(torch.equal(a, b) for a, b in zip(mine.parameters(), ref.parameters()))
    # the bank's form: the backward has been done (one, of the summed losses); the update alone
    criterion(mine(x), labels).backward()
    criterion(ref(x), labels).backward()
    frozen.probe_update(mine, opt_mine, None, False)
    torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
    opt_ref.step()
    assert all(torch.equal(a, b) for a, b in zip(mine.parameters(), ref.parameters()))


def test_parse_config_defaults():
    from jepa_amd.evals import frozen
    cfg = frozen.parse_config({'pretrain': {'folder': '/f', 'checkpoint': 'c.pth.tar'}, 'optimization': {}})
    assert {k: v for k, v in vars(cfg).items() if k not in ('args_pretrain', 'args_opt')} == dict(
        checkpoint_key='target_encoder', model_name=None, patch_size=None, pretrain_folder='/f', ckp_fname='c.pth.tar', tag=None,
        use_sdpa=True, use_SiLU=False, tight_SiLU=True, uniform_power=False, pretrained_path='/f/c.pth.tar', tubelet_size=2,
        frames_per_clip=1, batch_size=None, num_epochs=None, wd=None, start_lr=None, lr=None, final_lr=None, warmup=None,
        use_bfloat16=None, multihead=None, resume_checkpoint=False, eval_tag=None)
    assert cfg.args_pretrain == {'folder': '/f', 'checkpoint': 'c.pth.tar'} and cfg.args_opt == {}
    full = frozen.parse_config({'pretrain': {'folder': '/f', 'checkpoint': 'c', 'write_tag': 't', 'frames_per_clip': 16},
                                'optimization': {'lr': 0.01, 'weight_decay': 0.2, 'multihead_kwargs': [{'lr': 0.1}]}, 'tag': 'x'},
                               resume_preempt=True)
    assert full.resume_checkpoint is True and full.eval_tag == 'x' and full.tag == 't' and full.frames_per_clip == 16
    assert full.wd == 0.2 and full.multihead == [dict(lr=0.1, start_lr=None, final_lr=None, weight_decay=0.2, warmup=None)]
    with pytest.raises(ValueError):
        frozen.parse_config({'pretrain': {'folder': '/f', 'checkpoint': 'c'}, 'optimization': {'multihead_kwargs': []}})
