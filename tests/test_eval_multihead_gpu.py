"""GPU: both frozen evals' main() with `optimization.multihead_kwargs` on the micro synthetic configs of the existing eval tests
(three probes, two epochs): per-probe CSVs and checkpoint lists, resume after epoch 1, different learning rates giving different
weights; and the same configs WITHOUT the key against the record the single-probe eval gave before the bank existed
(tests/golden/eval_single_probe_records.json, written by tools/make_golden_eval_records.py)."""
import copy
import csv
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

MULTIHEAD = [{'lr': 0.01}, {'lr': 0.003, 'weight_decay': 0.1}, {'lr': 0.03, 'start_lr': 0.01, 'warmup': 0.25}]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_single_probe_records.json")


def setup_eval(kind, folder, monkeypatch=None):
    """-> (eval module, config) of the micro synthetic run of tests/test_eval_frozen_gpu.py ('video') or
    tests/test_image_eval_micro_gpu.py ('image'), with the encoder checkpoint written into `folder`."""
    from jepa_amd.src.models import vision_transformer as vit
    os.makedirs(folder, exist_ok=True)
    if kind == "video":
        from jepa_amd.evals.video_classification_frozen import eval as E
        from tests.test_eval_frozen_gpu import _micro_cfg, _micro_vit
        make = lambda **kw: _micro_vit(**{k: v for k, v in kw.items() if k != "use_sdpa"})   # noqa: E731
        if monkeypatch is not None:
            monkeypatch.setattr(vit, "vit_micro", make, raising=False)
        else:
            vit.vit_micro = make
        torch.manual_seed(1)
        sd = _micro_vit().state_dict()
        cfg, name = _micro_cfg(folder), 'micro-latest.pth.tar'
    else:
        from jepa_amd.evals.image_classification_frozen import eval as E
        from tests.test_image_eval_micro_gpu import _cfg
        torch.manual_seed(1)
        sd = vit.vit_tiny(img_size=64, patch_size=16, num_frames=8, tubelet_size=2, uniform_power=True).state_dict()
        cfg, name = _cfg(folder), 'tiny-latest.pth.tar'
    torch.save({'target_encoder': {'module.backbone.' + k: v for k, v in sd.items()}, 'epoch': 10}, os.path.join(folder, name))
    return E, cfg


def single_probe_record(kind, folder, monkeypatch=None):
    E, cfg = setup_eval(kind, folder, monkeypatch)
    torch.manual_seed(0)
    rec = E.main(cfg)
    return dict(train_acc=rec['train_acc'], val_acc=rec['val_acc'], lrs=[h[0] for h in rec['train_history']],
                losses=[h[1] for h in rec['train_history']])


@pytest.mark.parametrize("kind", ["video", "image"])
def test_main_with_a_bank_of_three_probes(kind, tmp_path, monkeypatch):
    from jepa_amd.evals import multihead as M
    from jepa_amd.src.models.attentive_pooler import AttentiveClassifier
    E, cfg = setup_eval(kind, str(tmp_path / "a"), monkeypatch)
    cfg['optimization']['multihead_kwargs'] = copy.deepcopy(MULTIHEAD)
    torch.manual_seed(0)
    rec = E.main(copy.deepcopy(cfg))
    out = tmp_path / "a" / f"{kind}_classification_frozen" / cfg['tag']
    tag = cfg['pretrain']['write_tag']
    assert not os.path.exists(out / f"{tag}_r0.csv")
    assert len(rec['train_acc']) == 2 and all(len(a) == 3 for a in rec['train_acc'] + rec['val_acc'])
    for p in range(3):
        rows = list(csv.reader(open(out / f"{tag}_p{p}_r0.csv")))
        assert rows[0] == ["epoch", "loss", "acc"] and [r[0] for r in rows[1:]] == ["1", "2"]
        assert [float(r[1]) for r in rows[1:]] == pytest.approx([a[p] for a in rec['train_acc']], abs=1e-5)
        assert [float(r[2]) for r in rows[1:]] == pytest.approx([a[p] for a in rec['val_acc']], abs=1e-5)
    ck = torch.load(out / f"{tag}-latest.pth.tar", map_location="cpu", weights_only=False)
    assert ck['epoch'] == 2 and ck['lr'] == [0.01, 0.003, 0.03] and ck['scaler'] == [None] * 3
    assert all(len(ck[k]) == 3 for k in ('classifier', 'opt', 'scaler'))
    D, H = (64, 2) if kind == "video" else (192, 3)
    lone = AttentiveClassifier(embed_dim=D, num_heads=H, num_classes=4)
    for sd in ck['classifier']:                                                    # each probe: the reference's checkpoint format
        assert list(sd) == ['module.' + k for k in lone.state_dict()]
        lone.load_state_dict({k[len('module.'):]: v for k, v in sd.items()}, strict=True)
    assert all(int(o['state'][0]['step']) == 8 for o in ck['opt'])                 # 2 epochs x 16 items / batch 4
    hist = rec['train_history']
    assert len(hist) == 8 and all(len(lrs) == 3 and len(ls) == 3 for lrs, ls in hist)
    # each probe on its own schedule: warmup 0.5 x 4 iterations from start_lr 0.002 for probes 0 and 1, 0.25 x 4 for probe 2
    assert hist[0][0] == pytest.approx([0.006, 0.0025, 0.03]) and hist[1][0][:2] == pytest.approx([0.01, 0.003])
    w = [sd['module.linear.weight'] for sd in ck['classifier']]
    assert not torch.equal(w[0], w[1]) and not torch.equal(w[0], w[2])             # different learning rates, different weights
    assert rec['best_probe'] == max(range(3), key=lambda p: rec['val_acc'][-1][p])

    # preempted after epoch 1 and resumed: epoch 2 as in the straight run (losses at the evals' own resume bound, 1e-2)
    E, cfg_b = setup_eval(kind, str(tmp_path / "b"), monkeypatch)
    cfg_b['optimization']['multihead_kwargs'] = copy.deepcopy(MULTIHEAD)
    real, calls = M.run_one_epoch, []

    def preempt(*a, **kw):
        calls.append(1)
        if len(calls) == 3:
            raise KeyboardInterrupt("preempted")
        return real(*a, **kw)

    monkeypatch.setattr(M, "run_one_epoch", preempt)
    torch.manual_seed(0)
    with pytest.raises(KeyboardInterrupt):
        E.main(copy.deepcopy(cfg_b))
    monkeypatch.setattr(M, "run_one_epoch", real)
    path_b = tmp_path / "b" / f"{kind}_classification_frozen" / cfg['tag'] / f"{tag}-latest.pth.tar"
    ck_1 = torch.load(path_b, map_location="cpu", weights_only=False)             # half way down each probe's own decay schedule
    assert ck_1['epoch'] == 1 and [o['param_groups'][0]['weight_decay'] for o in ck_1['opt']] == pytest.approx(
        [1e-6 + (wd - 1e-6) * 0.5 for wd in (0.01, 0.1, 0.01)])
    rec_b = E.main(copy.deepcopy(cfg_b), resume_preempt=True)
    assert rec_b['start_epoch'] == 1 and len(rec_b['train_history']) == 4 and len(rec_b['val_acc']) == 1
    for (lrs_b, ls_b), (lrs_a, ls_a) in zip(rec_b['train_history'], hist[4:]):
        assert lrs_b == lrs_a
        assert ls_b == pytest.approx(ls_a, rel=1e-2)
    print("epoch 2 straight", rec['train_acc'][1], rec['val_acc'][1], "resumed", rec_b['train_acc'][0], rec_b['val_acc'][0])
    one_item = 100.0 / 16 + 1e-3                                                   # 16 items per split
    assert rec_b['train_acc'][0] == pytest.approx(rec['train_acc'][1], abs=one_item)
    assert rec_b['val_acc'][0] == pytest.approx(rec['val_acc'][1], abs=one_item)
    ck_b = torch.load(path_b, map_location="cpu", weights_only=False)
    assert ck_b['epoch'] == 2 and all(int(o['state'][0]['step']) == 8 for o in ck_b['opt'])


@pytest.mark.parametrize("kind", ["video", "image"])
def test_main_without_the_key_gives_the_single_probe_record(kind, tmp_path, monkeypatch):
    """No `multihead_kwargs`: the single-probe eval, whose record on these configs was written down before the bank was added."""
    gold = json.load(open(GOLDEN))[kind]
    rec = single_probe_record(kind, str(tmp_path), monkeypatch)
    print(kind, rec)
    assert rec['lrs'] == gold['lrs']
    assert rec['losses'] == pytest.approx(gold['losses'], rel=1e-4)
    assert rec['train_acc'] == pytest.approx(gold['train_acc'], abs=1e-3)
    assert rec['val_acc'] == pytest.approx(gold['val_acc'], abs=1e-3)
    out = tmp_path / f"{kind}_classification_frozen"
    assert [f for _, _, fs in os.walk(out) for f in fs if "_p0_" in f] == []
