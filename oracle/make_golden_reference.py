"""Generate tests/golden/reference_api.npz from the REAL reference (facebookresearch/jepa, read-only; its root is
taken from $JEPA_REFERENCE).  Run where the reference is present:  JEPA_REFERENCE=/path/to/jepa python oracle/make_golden_reference.py

Records what the reference's own code does with the inputs the tests build, so that the tests need no reference:
  init/*     -- app.vjepa.utils.init_video_model (vit_tiny, seed 0): state-dict names, shapes, fingerprints, trainable names
  coll/*     -- src.masks.multiblock3d / random_tube MaskCollator over tests.golden_util.collator_trials(): one digest per draw
  ckpt/*     -- app.vjepa.utils.load_checkpoint of a jepa_amd checkpoint into reference modules + the reference's init_opt
                AdamW: the epoch it returns, the loaded module tensors and optimizer state by parameter name, the groups
  eval/*     -- evals/video_classification_frozen/eval.py load_pretrained of the same kind of checkpoint into a bare
                reference vit_tiny: the loaded state and the CPU forward of two clips
Float tensors are kept as tests.golden_util.tensor_fingerprint (size, sum, sum of squares, 64 values: CPU kernels of another
host may differ in the last bit), collator draws as tensor_digest (sha256 of dtype, shape and bytes); no program text.
"""
import ast
import copy
import logging
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("JEPA_REFERENCE", "")
OUT = os.path.join(ROOT, "tests", "golden", "reference_api.npz")

INIT_KW = dict(device="cpu", patch_size=16, num_frames=8, tubelet_size=2, model_name="vit_tiny", crop_size=64,
               pred_depth=2, pred_embed_dim=96, uniform_power=True, use_mask_tokens=True, num_mask_tokens=2,
               zero_init_mask_tokens=True, use_sdpa=True)
INIT_ATTRS = ("embed_dim", "num_heads", "num_patches", "patch_size", "tubelet_size", "num_frames", "input_size")


def _state(prefix, sd, out):
    from tests.golden_util import tensor_fingerprint
    out[prefix + "_keys"] = np.array(list(sd.keys()))
    out[prefix + "_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    out[prefix + "_fp"] = np.stack([tensor_fingerprint(v) for v in sd.values()])


def _reference_function(rel_path, name, extra_globals):
    """ONE function definition of a reference file whose module cannot be imported here (torchvision / decord)."""
    src = open(os.path.join(REF, rel_path)).read()
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == name)
    ns = dict(extra_globals)
    exec(compile(ast.Module(body=[node], type_ignores=[]), rel_path, "exec"), ns)
    return ns[name]


def main():
    if not REF or not os.path.isdir(os.path.join(REF, "src")):
        raise SystemExit("set JEPA_REFERENCE to the root of a facebookresearch/jepa checkout")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, REF)
    import app.vjepa.utils as RU
    import src.models.vision_transformer as RV
    from src.masks.multiblock3d import MaskCollator as RefMB
    from src.masks.random_tube import MaskCollator as RefTube
    from tests.golden_util import collator_digests, tensor_fingerprint  # noqa: F401
    from tests.step_util import TINY, oracle_cfg  # noqa: F401
    from tests.test_checkpoint_reference import _DDPLike, _checkpoint, _fake_trained_state
    from tests.step_util import build_models
    import tempfile
    out = {}

    # -- init_video_model, seed for seed
    torch.manual_seed(0)
    re_, rp = RU.init_video_model(**INIT_KW)
    for tag, m in (("enc", re_), ("pred", rp)):
        _state(f"init/{tag}", m.state_dict(), out)
        out[f"init/{tag}_trainable"] = np.array([n for n, p in m.named_parameters() if p.requires_grad])
    out["init/attrs"] = np.array([int(getattr(re_.backbone, a)) for a in INIT_ATTRS], dtype=np.int64)

    # -- collators
    mb, tube = collator_digests(RefMB, RefTube)
    out["coll/multiblock_sha"], out["coll/tube_sha"] = np.array(mb), np.array(tube)

    tmp = tempfile.mkdtemp()
    # -- load_checkpoint (the checkpoint exactly as tests/test_checkpoint_reference.py builds it)
    enc, pred = build_models(TINY, 2, perturb_small=True)
    tgt = copy.deepcopy(enc)
    with torch.no_grad():
        for p in tgt.parameters():
            p.mul_(0.97)
    opt_sd, *_ = _fake_trained_state(enc, pred, step=5)
    path = os.path.join(tmp, "jepa-latest.pth.tar")
    torch.save(_checkpoint(enc, pred, tgt, opt_sd, epoch=7), path)
    torch.manual_seed(123)
    r_enc, r_pred = RU.init_video_model(device="cpu", patch_size=16, num_frames=TINY["frames"], tubelet_size=2,
                                        model_name="vit_tiny", crop_size=TINY["crop"], pred_depth=TINY["pred_depth"],
                                        pred_embed_dim=TINY["pred_dim"], uniform_power=True, use_mask_tokens=True,
                                        num_mask_tokens=2, zero_init_mask_tokens=True, use_sdpa=True)
    r_tgt = copy.deepcopy(r_enc)
    r_opt, r_scaler, _, _ = RU.init_opt(encoder=r_enc, predictor=r_pred, wd=0.04, final_wd=0.4, start_lr=2e-4, ref_lr=6e-4,
                                        final_lr=1e-6, iterations_per_epoch=10, warmup=1, num_epochs=4, ipe_scale=1.25,
                                        mixed_precision=False, betas=(0.9, 0.999), eps=1e-8)
    w_enc, w_pred, w_tgt = _DDPLike(r_enc), _DDPLike(r_pred), _DDPLike(r_tgt)
    *_, epoch = RU.load_checkpoint(r_path=path, encoder=w_enc, predictor=w_pred, target_encoder=w_tgt, opt=r_opt,
                                   scaler=r_scaler)
    out["ckpt/epoch"] = np.array([epoch], dtype=np.int64)
    for tag, m in (("enc", w_enc), ("pred", w_pred), ("tgt", w_tgt)):
        _state(f"ckpt/{tag}", m.state_dict(), out)
    name_of = {id(p): pre + n for pre, m in (("e.", r_enc), ("p.", r_pred)) for n, p in m.named_parameters()}
    groups, wd, wd_ex = [], [], []
    for g in r_opt.param_groups:
        groups.append([name_of[id(p)] for p in g["params"]])
        wd.append(float(g.get("weight_decay", 0.0)))
        wd_ex.append(bool(g.get("WD_exclude", False)))
    out["ckpt/group_names"] = np.array([n for g in groups for n in g])
    out["ckpt/group_sizes"] = np.array([len(g) for g in groups], dtype=np.int64)
    out["ckpt/group_wd_exclude"] = np.array(wd_ex)
    st_names, st_fp = [], []
    for g in r_opt.param_groups:
        for p in g["params"]:
            if p in r_opt.state:
                s = r_opt.state[p]
                st_names.append(name_of[id(p)])
                st_fp.append(np.stack([tensor_fingerprint(s["exp_avg"]), tensor_fingerprint(s["exp_avg_sq"])]))
                assert float(s["step"]) == 5.0
    out["ckpt/opt_state_names"], out["ckpt/opt_state_fp"] = np.array(st_names), np.stack(st_fp)

    # -- eval.py load_pretrained into a bare reference ViT + its CPU forward
    enc, pred = build_models(TINY, 2, perturb_small=True)
    tgt = copy.deepcopy(enc)
    with torch.no_grad():
        for p in tgt.parameters():
            p.mul_(0.97)
    opt_sd, *_ = _fake_trained_state(enc, pred)
    path = os.path.join(tmp, "jepa-eval.pth.tar")
    torch.save(_checkpoint(enc, pred, tgt, opt_sd, epoch=3), path)
    load_pretrained = _reference_function("evals/video_classification_frozen/eval.py", "load_pretrained",
                                          {"torch": torch, "logger": logging.getLogger("ref-eval")})
    torch.manual_seed(99)
    bare = RV.vit_tiny(img_size=TINY["crop"], patch_size=16, num_frames=TINY["frames"], tubelet_size=2,
                       uniform_power=True, use_sdpa=True)
    bare = load_pretrained(encoder=bare, pretrained=path, checkpoint_key="target_encoder")
    _state("eval/bare", bare.state_dict(), out)
    clips = torch.randn(2, 3, TINY["frames"], TINY["crop"], TINY["crop"], generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        out["eval/y"] = bare(clips).numpy().astype(np.float32)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
