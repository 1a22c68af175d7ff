"""GPU: real videos as frame folders through the video eval's loader and input edge (dataset_type: frame_folder).  Validation
frames of any size are resized on the device (vj_clip_resample) before the views are cut: the finished fp32 views equal, bit for
bit, what the reference's EvalVideoTransform / VideoTransform(training=False) make from the same frames as PIL images
(tests/golden/frame_folder_micro.npz) -- the resample is integer arithmetic and the identity-box path of vj_clip_transform_pre is
bit-exact (tests/test_eval_transform_gpu.py), so no tolerance applies.  Then the three entry points on a micro folder."""
import csv
import os

import numpy as np
import pytest
import torch

from tests.frame_folder_util import case, centre_names, smooth_video, view_names, write_frames, write_index

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 16


def _folder_of_cases(tmp_path, names):
    """Every fixture case as a PNG folder, labelled by its position in `names`."""
    rows = [(write_frames(str(tmp_path / n), case(n)["frames"]), k) for k, n in enumerate(names)]
    return write_index(tmp_path / "cases.csv", rows)


def _loader(index, views, batch):
    from jepa_amd.evals.video_classification_frozen.eval import make_dataloader
    return make_dataloader(root_path=[index], batch_size=batch, world_size=1, rank=0, dataset_type="frame_folder", resolution=S,
                           frames_per_clip=2, frame_step=1, num_segments=1, num_views_per_segment=views, training=False,
                           allow_segment_overlap=False, num_workers=0)      # two-frame videos give frames 0 and 1


def _check_batches(pf, names, views):
    seen = []
    for clips, labels, idx in pf:
        torch.cuda.synchronize()
        assert len(clips) == 1 and len(clips[0]) == views and len(idx) == 1
        for b, label in enumerate(labels.tolist()):
            c = case(names[label])
            frames = idx[0][b].tolist()
            for v in range(views):
                got = clips[0][v][b].cpu()
                assert got.shape == (3, 2, S, S) and got.dtype == torch.float32
                assert torch.equal(got, torch.from_numpy(c["views"][v][:, frames])), (names[label], v, frames)
            seen.append(label)
    assert sorted(seen) == list(range(len(names)))


def test_multi_view_validation_views_equal_the_reference_bit_for_bit(tmp_path):
    from jepa_amd.engine.input import EvalPrefetcher
    names = view_names()
    pf = EvalPrefetcher(_loader(_folder_of_cases(tmp_path, names), 3, 4), torch.device(DEV))
    np.random.seed(0)
    _check_batches(pf, names, 3)
    assert any(("resized", 0) in d for d in pf._dev)


def test_centre_crop_validation_views_equal_the_reference_bit_for_bit(tmp_path):
    from jepa_amd.engine.input import EvalPrefetcher
    names = centre_names()
    pf = EvalPrefetcher(_loader(_folder_of_cases(tmp_path, names), 1, 2), torch.device(DEV))
    np.random.seed(0)
    _check_batches(pf, names, 1)


def test_a_batch_of_native_frames_launches_no_resample_and_keeps_its_bits(tmp_path):
    from jepa_amd.engine.input import EvalPrefetcher
    names = ["views_native"]
    index = _folder_of_cases(tmp_path, names)
    other = np.ascontiguousarray(case("views_native")["frames"].transpose(0, 2, 1, 3))        # 30 x 16: portrait, native too
    write_frames(str(tmp_path / "portrait"), other)
    index = write_index(tmp_path / "native.csv", [(str(tmp_path / "views_native"), 0), (str(tmp_path / "portrait"), 1)])
    pf = EvalPrefetcher(_loader(index, 3, 2), torch.device(DEV))
    np.random.seed(0)
    (clips, labels, idx), = list(pf)
    torch.cuda.synchronize()
    assert all(("resized", 0) not in d and ("resample_ws", 0) not in d and ("rgeom", 0) not in d for d in pf._dev)
    c = case("views_native")
    for b, label in enumerate(labels.tolist()):
        for v in range(3):
            want = torch.from_numpy(c["views"][v])
            want = want if label == 0 else want.transpose(2, 3)        # the transposed video's views are the transposed views
            assert torch.equal(clips[0][v][b].cpu(), want[:, idx[0][b].tolist()]), (label, v)


# ------------------------------------------------------------------------------------------------ the entry points
SIZES = ((20, 28), (33, 24), (16, 16), (18, 40), (40, 56), (25, 18), (16, 30), (47, 31))


@pytest.fixture()
def micro_folder(tmp_path):
    """8 videos of 9 frames, mixed sizes (landscape, portrait, square, native short sides 16 and 18), 4 classes: PNG folders and
    two .npy videos, one index for training and validation."""
    rows = []
    for k, (H, W) in enumerate(SIZES):
        video = smooth_video(9, H, W, 40 + k)
        if k % 4 == 3:
            np.save(tmp_path / f"v{k}.npy", video)
            rows.append((f"v{k}.npy", k % 4))
        else:
            write_frames(str(tmp_path / f"v{k}"), video)
            rows.append((f"v{k}", k % 4))
    return write_index(tmp_path / "videos.csv", rows)


def _micro_vit(**kw):
    from tests.test_eval_frozen_gpu import _micro_vit as micro
    return micro(**{**dict(img_size=S, patch_size=8, num_frames=4), **{k: v for k, v in kw.items() if k != "use_sdpa"}})


def _eval_cfg(folder, index, finetune):
    cfg = {
        'pretrain': {'model_name': 'vit_micro', 'checkpoint_key': 'target_encoder', 'patch_size': 8, 'folder': folder,
                     'checkpoint': 'micro-latest.pth.tar', 'write_tag': 'micro', 'tubelet_size': 2, 'frames_per_clip': 4,
                     'frame_step': 2, 'uniform_power': True, 'use_sdpa': True, 'use_silu': False, 'tight_silu': False},
        'data': {'dataset_type': 'frame_folder', 'dataset_train': index, 'dataset_val': index, 'num_classes': 4,
                 'frames_per_clip': 4, 'num_segments': 2, 'num_views_per_segment': 3, 'num_workers': 0},
        'optimization': {'resolution': S, 'batch_size': 4, 'attend_across_segments': True, 'num_epochs': 1,
                         'weight_decay': 0.01, 'start_lr': 0.002, 'lr': 0.01, 'final_lr': 0.0, 'warmup': 0.5,
                         'use_bfloat16': False},
        'tag': 'micro_ff',
    }
    if finetune:
        cfg['optimization']['finetune'] = {'encoder_lr': 1e-3, 'layer_decay': 0.75, 'encoder_weight_decay': 0.05}
    return cfg


@pytest.mark.parametrize("finetune", [False, True])
def test_the_eval_mains_run_an_epoch_on_a_frame_folder(finetune, micro_folder, tmp_path, monkeypatch):
    from jepa_amd.src.models import vision_transformer as vit
    if finetune:
        from jepa_amd.evals.video_classification_finetune import eval as M
        out = "video_classification_finetune"
    else:
        from jepa_amd.evals.video_classification_frozen import eval as M
        out = "video_classification_frozen"
    monkeypatch.setattr(vit, "vit_micro", _micro_vit, raising=False)
    folder = str(tmp_path / "run")
    os.makedirs(folder)
    torch.manual_seed(1)
    sd = _micro_vit().state_dict()
    torch.save({'target_encoder': {'module.backbone.' + k: v for k, v in sd.items()}, 'epoch': 10},
               os.path.join(folder, 'micro-latest.pth.tar'))
    torch.manual_seed(0)
    np.random.seed(0)
    rec = M.main(_eval_cfg(folder, micro_folder, finetune))
    assert len(rec['train_history']) == 2 and len(rec['val_acc']) == 1            # 8 videos / batch 4, one epoch
    assert np.isfinite(np.array([h[1] for h in rec['train_history']] + rec['train_acc'] + rec['val_acc'], dtype=np.float64)).all()
    rows = list(csv.reader(open(os.path.join(folder, out, "micro_ff", "micro_r0.csv"))))
    assert rows[0] == ["epoch", "loss", "acc"] and [r[0] for r in rows[1:]] == ["1"]
    ck = torch.load(os.path.join(folder, out, "micro_ff", "micro-latest.pth.tar"), map_location="cpu", weights_only=False)
    assert ck['epoch'] == 1 and ('encoder' in ck) == finetune


@pytest.mark.parametrize("keys", ["rand_augment and a probe bank", "mix, drop_path and recompute"])
def test_the_extension_keys_of_the_evals_work_on_a_frame_folder(keys, micro_folder, tmp_path, monkeypatch):
    """data.rand_augment and optimization.multihead_kwargs on the frozen eval; optimization.finetune.mix / drop_path / recompute on
    the fine-tuning eval: one epoch each, finite records."""
    from jepa_amd.src.models import vision_transformer as vit
    finetune = keys.startswith("mix")
    cfg = _eval_cfg(str(tmp_path / "run"), micro_folder, finetune)
    if finetune:
        from jepa_amd.evals.video_classification_finetune import eval as M
        cfg['optimization']['finetune'].update(mix={'mixup_alpha': 0.8, 'cutmix_alpha': 1.0}, drop_path=0.1, recompute='block')
    else:
        from jepa_amd.evals.video_classification_frozen import eval as M
        cfg['data']['rand_augment'] = True
        cfg['optimization']['multihead_kwargs'] = [{'lr': 0.01}, {'lr': 0.003, 'weight_decay': 0.1}]
    monkeypatch.setattr(vit, "vit_micro", _micro_vit, raising=False)
    os.makedirs(cfg['pretrain']['folder'])
    torch.manual_seed(1)
    torch.save({'target_encoder': {'module.backbone.' + k: v for k, v in _micro_vit().state_dict().items()}, 'epoch': 10},
               os.path.join(cfg['pretrain']['folder'], 'micro-latest.pth.tar'))
    torch.manual_seed(0)
    np.random.seed(0)
    rec = M.main(cfg)
    losses = np.array([h[1] for h in rec['train_history']], dtype=np.float64)
    assert losses.size >= 2 and np.isfinite(losses).all()
    assert np.isfinite(np.array(rec['val_acc'], dtype=np.float64)).all()


def test_pretraining_runs_two_iterations_on_a_frame_folder(micro_folder, tmp_path):
    from jepa_amd.app.vjepa.train import main
    from tests.test_train_loop_gpu import read_csv, tiny_args
    folder = str(tmp_path / "pretrain")
    args = tiny_args(folder, epochs=1)
    args['data'].update(dataset_type='frame_folder', datasets=[micro_folder], sampling_rate=1)
    args['data_aug'] = {'random_resize_aspect_ratio': [0.75, 1.35], 'random_resize_scale': [0.3, 1.0], 'motion_shift': False,
                        'reprob': 0.0, 'auto_augment': False}
    args['optimization']['ipe'] = 2
    main(args)
    rows = read_csv(os.path.join(folder, 'jepa_r0.csv'))
    assert len(rows) == 2 and all(np.isfinite(float(r['loss'])) and float(r['loss']) > 0 for r in rows)
    assert os.path.isfile(os.path.join(folder, 'jepa-latest.pth.tar'))
