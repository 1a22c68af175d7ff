#!/usr/bin/env python
"""Frozen video-classification eval (jepa_amd/evals/video_classification_frozen): one training and one validation iteration of a
shipped eval config with random weights, B = 4 as in the configs.  Reports the frozen forward (clips/s), the probe (ms for the
training step -- forward, backward, clip_grad_norm_, AdamW -- and for the validation forward over every view), the whole
run_one_epoch iteration and the peak memory.  One JSON line per config.
python tools/eval_bench.py [--configs vitl16_k400_16x8x3 vith16_384_k400_16x8x3] [--reps 3]
--bank P adds the same training iteration with `optimization.multihead_kwargs` of P entries (one AttentiveClassifierBank, P
optimizers; jepa_amd/evals/multihead.py): bank_train_iteration_ms beside train_iteration_ms of the single probe.

--image: the frozen image-classification eval (jepa_amd/evals/image_classification_frozen) in the in1k setup (batch 16, 1000 classes)
for ViT-L/16-224 and ViT-H/16-384: frozen images/s, probe ms, one training and one validation iteration, peak memory; the still-image
path against the only route there was before it (the ATen repeat to 16 frames, timed, followed by the 5-D forward), the two arms
taking turns inside this process in both orders (as tools/abab.py does for the step); and vj_pos_interp3d once per new size.
python tools/eval_bench.py --image [--image-configs vitl16_in1k vith16_384_in1k] [--rounds 4] [--reps 3]

--frames: FrameAggregation on the ViT-L/16 image (num_frames=1) model at 224: 2 videos x 8 segments x 3 views x 16 frames = 768 frames
of 196 tokens.  The direct route (patch rows packed straight from the [B,C,T,H,W] clips) against the reference's route (views
concatenated along the batch, segments along time, the permuted [B*T,C,H,W] fp32 copy through ATen, then the model) and against the
direct route with one (segment, view) tensor per trunk call, the arms taking turns inside this process in both orders; frames/s and peak memory of each; the temporal position pass (vj_add_pos_frames);
and vj_pos_interp2d_bicubic once per new size.
python tools/eval_bench.py --frames [--rounds 4] [--reps 3]

--uint8: the input edge of the video eval on the K400 16x8x3 protocol (ViT-L/16-224, batch 4): one training and one validation
iteration of run_one_epoch fed pinned fp32 views that it moves with `.to(device)` in front of the forward (the path of
`dataset_type: synthetic`, and of the parent commit) against uint8 frames through EvalPrefetcher (the views made on the device, batch
k+1 uploading under batch k's frozen forward), the two arms taking turns inside this process in both orders.  Per arm and round:
host-to-device bytes per iteration, wall time per iteration, the wait at the input edge (fp32: the copies themselves, timed alone;
uint8: how long the compute stream stood at the prefetcher's event), and the two kernels timed alone.  The host batches are built
once, before the clock starts: what a loader costs to decode and draw is not part of these figures.
python tools/eval_bench.py --uint8 [--rounds 3] [--reps 3]

--finetune: one fine-tuning iteration (jepa_amd/evals/video_classification_finetune: ClipAggregation with gradients, the probe's
update, EncoderFineTuner.step) against the frozen iteration of the same config -- ViT-L/16 16x224x224, batch 4, attend_across_segments
with --segments segments (default 1 and 8) -- the two arms taking turns inside this process in both orders; ms and peak memory
of each, and EncoderFineTuner.step timed alone (its launches, ms, share of the iteration).  --drop-path R adds a third arm taking
turns with the two: the same fine-tuning iteration with stochastic depth at rate R (the fine-tuning arm itself runs at rate 0), and
times vj_drop_path_add / vj_drop_path_scale alone on the trunk's M x D rows, every sample kept, beside vj_copy_rows (ms, bytes/s).
--mix adds another arm in the same rotation: the fine-tuning iteration (rate 0) with `optimization.finetune.mix` at the recipe's
values (mixup 0.8, cutmix 1.0, prob 1, switch 0.5, label smoothing 0.1: vj_clip_mix on every segment, vj_soft_ce for the loss), and
times vj_clip_mix alone on one segment batch [4,3,16,224,224] (a mixup plan, which moves every byte, and a cutmix plan with a box of
half the side) beside vj_copy_rows on the same bytes, and vj_soft_ce at R = 4, C in {400, 1000}.
--recompute MODE (mlp or block) adds another arm in the same rotation: the fine-tuning iteration (rate 0) with
VisionTransformer.set_activation_recompute(MODE); ms and peak memory as the other arms', the per-round difference to the plain
fine-tuning arm, and for every arm the peak of what the allocator held (the whole process, after an empty_cache before the arm).
--model NAME RES, --batch B and --no-frozen (no frozen arm) reach the configs the default does not, e.g. vit_huge 384.
--dp1 adds another arm in the same rotation, in a one-rank `nccl` (RCCL) process group this tool creates: the fine-tuning iteration
with the data-parallel reducer forced (VJ_FORCE_DP=1: engine.dp.GradReducer on dp.finetune_bucket_plan, launched by the encoder's
backward) on the SAME encoder and tuner as the plain arm, which runs with the encoder's reducer hook withdrawn.  Reports the arm's ms
per round and their spread, the per-round difference to the plain arm, reducer.exposed_ms(), coll_check, the route and the number of
collectives per iteration.  A one-rank all-reduce moves nothing: what is timed is the bucket walk, its events and stream joins.
python tools/eval_bench.py --finetune [--segments 1 8] [--rounds 4] [--reps 3] [--drop-path 0.1] [--mix] [--recompute block] [--dp1]
                           [--model vit_huge 384] [--batch 4] [--no-frozen]

--image --finetune: one fine-tuning iteration of the image eval (jepa_amd/evals/image_classification_finetune: batch 16, 1000 classes,
ViT-L/16-224 and ViT-H/16-384 at 16 frames) on still images, the same iteration on the materialised repeated clip (the ATen repeat
inside it) and the frozen iteration, the three arms taking turns inside this process in rotating order: ms and peak memory of each,
the rows the patch-embed GEMM and its weight gradient see on either route, and vj_slice_sum alone beside vj_copy_rows moving the same
bytes (ms, GB/s).  --recompute MODE adds the still-image iteration with that activation-recomputation mode as a fourth arm.
python tools/eval_bench.py --image --finetune [--image-configs vitl16_in1k vith16_384_in1k] [--rounds 4] [--reps 3] [--recompute mlp]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jepa_amd.evals.video_classification_frozen.eval import init_opt, run_one_epoch  # noqa: E402
from jepa_amd.evals.video_classification_frozen.utils import ClipAggregation  # noqa: E402
from jepa_amd.src.models import vision_transformer as vit  # noqa: E402
from jepa_amd.src.models.attentive_pooler import AttentiveClassifier  # noqa: E402

# configs/evals/<name>.yaml of the reference: (model_name, resolution, num_segments, num_views_per_segment, num_classes)
CONFIGS = {
    "vitl16_k400_16x8x3": ("vit_large", 224, 8, 3, 400), "vith16_k400_16x8x3": ("vit_huge", 224, 8, 3, 400),
    "vith16_384_k400_16x8x3": ("vit_huge", 384, 8, 3, 400), "vitl16_ssv2_16x2x3": ("vit_large", 224, 2, 3, 174),
    "vith16_ssv2_16x2x3": ("vit_huge", 224, 2, 3, 174), "vith16_384_ssv2_16x2x3": ("vit_huge", 384, 2, 3, 174),
}


def timed(fn, reps):
    fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def bench(name, reps, B=4, bank=0):
    model_name, res, S, V, C = CONFIGS[name]
    dev = "cuda"
    torch.manual_seed(0)
    enc = ClipAggregation(vit.__dict__[model_name](img_size=res, patch_size=16, num_frames=16, tubelet_size=2, uniform_power=True),
                          tubelet_size=2, attend_across_segments=True).to(dev).eval()
    for p in enc.parameters():
        p.requires_grad = False
    clf = AttentiveClassifier(embed_dim=enc.embed_dim, num_heads=enc.num_heads, depth=1, num_classes=C).to(dev)
    opt, scaler, sched, wd_sched = init_opt(clf, iterations_per_epoch=1, start_lr=1e-4, ref_lr=1e-4, warmup=0,
                                            num_epochs=10 ** 6, wd=0.01)
    labels = torch.randint(0, C, (B,))
    idx = [torch.arange(16) for _ in range(S)]
    train = ([[torch.randn(B, 3, 16, res, res, device=dev)] for _ in range(S)], labels, idx)
    val = ([[torch.randn(B, 3, 16, res, res, device=dev) for _ in range(V)] for _ in range(S)], labels, idx)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()

    def fwd(batch):
        with torch.no_grad():
            return enc(batch[0])

    t_enc_train = timed(lambda: fwd(train), reps)
    t_enc_val = timed(lambda: fwd(val), reps)
    ftrain, fval = fwd(train), fwd(val)
    crit = torch.nn.CrossEntropyLoss()
    lab = labels.to(dev)

    def probe_train():
        loss = sum(crit(clf(o), lab) for o in ftrain) / len(ftrain)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(clf.parameters(), 1.0)
        opt.step()
        opt.zero_grad()

    def probe_val():
        with torch.no_grad():
            return [clf(o) for o in fval]

    t_probe_train = timed(probe_train, reps)
    t_probe_val = timed(probe_val, reps)
    del ftrain, fval
    it_train = timed(lambda: run_one_epoch(dev, True, enc, clf, scaler, opt, sched, wd_sched, [train], False, 1, S, True), reps)
    it_val = timed(lambda: run_one_epoch(dev, False, enc, clf, scaler, opt, sched, wd_sched, [val], False, V, S, True), reps)
    peak = torch.cuda.max_memory_allocated() - base
    extra = {}
    if bank:
        from functools import partial
        from jepa_amd.evals import multihead as M
        from jepa_amd.evals.video_classification_frozen.eval import _view_features
        from jepa_amd.src.models.attentive_pooler import AttentiveClassifierBank
        del clf, opt
        probes = AttentiveClassifierBank(enc.embed_dim, enc.num_heads, C, bank).to(dev)
        opts, scalers, scheds, wd_scheds = (list(t) for t in zip(*[
            init_opt(m, iterations_per_epoch=1, start_lr=1e-4, ref_lr=1e-4 * (1 + p), warmup=0, num_epochs=10 ** 6, wd=0.01)
            for p, m in enumerate(probes.probes)]))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        it_bank = timed(lambda: M.run_one_epoch(dev, True, partial(_view_features, True), enc, probes, scalers, opts, scheds,
                                                wd_scheds, [train], False), reps)
        extra = dict(bank_probes=bank, bank_train_iteration_ms=round(it_bank, 2),
                     bank_peak_mem_gib=round((torch.cuda.max_memory_allocated() - base) / 2 ** 30, 2))
    return dict(config=name, batch=B, probe_keys=S * enc.model.num_patches, clips_train=S * B, clips_val=S * V * B, **extra,
                frozen_fwd_clips_per_s_train=round(S * B / t_enc_train * 1e3, 1),
                frozen_fwd_clips_per_s_val=round(S * V * B / t_enc_val * 1e3, 1),
                probe_train_step_ms=round(t_probe_train, 3), probe_val_ms=round(t_probe_val, 3),
                train_iteration_ms=round(it_train, 2), val_iteration_ms=round(it_val, 2),
                peak_mem_gib=round(peak / 2 ** 30, 2),
                max_clips_per_call=enc.max_clips_per_call)


IMAGE_CONFIGS = {"vitl16_in1k": ("vit_large", 224, 1000), "vith16_in1k": ("vit_huge", 224, 1000),
                 "vith16_384_in1k": ("vit_huge", 384, 1000)}
# (model, native token grid) -> token grids to interpolate the position table to
INTERP_CASES = [("vit_large", 1024, (8, 14, 14), (8, 24, 24)), ("vit_huge", 1280, (8, 24, 24), (8, 14, 14)),
                ("vit_huge", 1280, (8, 24, 24), (16, 24, 24))]


def bench_image(name, reps, rounds, B=16, frames=16):
    import statistics
    from jepa_amd.evals.image_classification_frozen import eval as IE
    model_name, res, C = IMAGE_CONFIGS[name]
    dev = "cuda"
    torch.manual_seed(0)
    enc = vit.__dict__[model_name](img_size=res, patch_size=16, num_frames=frames, tubelet_size=2, uniform_power=True).to(dev).eval()
    for p in enc.parameters():
        p.requires_grad = False
    clf = AttentiveClassifier(embed_dim=enc.embed_dim, num_heads=enc.num_heads, depth=1, num_classes=C).to(dev)
    opt, scaler, sched, wd_sched = IE.init_opt(clf, iterations_per_epoch=1, start_lr=1e-4, ref_lr=1e-4, warmup=0, num_epochs=10 ** 6,
                                               wd=0.01)
    images = torch.randn(B, 3, res, res, device=dev)
    labels = torch.randint(0, C, (B,))
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()

    def still():
        with torch.no_grad():
            return enc(images)

    def repeated():      # the route before the still-image front end: the repeated fp32 clip through ATen, then the 5-D forward
        with torch.no_grad():
            return enc(images.unsqueeze(2).repeat(1, 1, frames, 1, 1))

    arms = {"still": still, "repeat": repeated}
    peak = {}
    for arm, fn in arms.items():    # warm-up (workspace growth, code load) and the peak memory of each route on its own
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[arm] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 30, 3)
    ms = {arm: [] for arm in arms}
    for r in range(rounds):
        for arm in (("still", "repeat") if r % 2 == 0 else ("repeat", "still")):
            ms[arm].append(timed(arms[arm], reps))
    mean = {arm: statistics.mean(v) for arm, v in ms.items()}
    spread = {arm: max(v) - min(v) for arm, v in ms.items()}
    feats = still()
    crit = torch.nn.CrossEntropyLoss()
    lab = labels.to(dev)

    def probe_train():
        loss = crit(clf(feats), lab)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(clf.parameters(), 1.0)
        opt.step()
        opt.zero_grad()

    def probe_val():
        with torch.no_grad():
            return clf(feats)

    torch.cuda.reset_peak_memory_stats()
    t_probe_train = timed(probe_train, reps)
    t_probe_val = timed(probe_val, reps)
    del feats
    it_train = timed(lambda: IE.run_one_epoch(dev, True, enc, clf, scaler, opt, sched, wd_sched, [(images, labels)], False), reps)
    it_val = timed(lambda: IE.run_one_epoch(dev, False, enc, clf, scaler, opt, sched, wd_sched, [(images, labels)], False), reps)
    torch.cuda.synchronize()
    return dict(config=name, batch=B, tokens_per_image=enc.num_patches, rounds=rounds, reps=reps,
                still_ms_rounds=[round(v, 3) for v in ms["still"]], repeat_ms_rounds=[round(v, 3) for v in ms["repeat"]],
                still_ms_mean=round(mean["still"], 3), repeat_ms_mean=round(mean["repeat"], 3),
                still_ms_spread=round(spread["still"], 3), repeat_ms_spread=round(spread["repeat"], 3),
                still_minus_repeat_ms=round(mean["still"] - mean["repeat"], 3),
                still_not_slower_than_repeat_plus_its_spread=bool(mean["still"] <= mean["repeat"] + spread["repeat"]),
                frozen_images_per_s=round(B / mean["still"] * 1e3, 1), frozen_images_per_s_repeat=round(B / mean["repeat"] * 1e3, 1),
                probe_train_step_ms=round(t_probe_train, 3), probe_val_ms=round(t_probe_val, 3),
                train_iteration_ms=round(it_train, 2), val_iteration_ms=round(it_val, 2),
                peak_mem_gib_forward_still=peak["still"], peak_mem_gib_forward_repeat=peak["repeat"],
                peak_mem_gib_iterations=round((torch.cuda.max_memory_allocated() - base) / 2 ** 30, 3))


def bench_slice_sum(B, S, Gt, D, reps=20):
    """vj_slice_sum alone on the trunk's input gradient [B*Gt*S, D] beside vj_copy_rows moving the same number of bytes (reads plus
    writes): ms and GB/s by the bytes each must move."""
    from jepa_amd.hip import ops
    dev = "cuda"
    dx = torch.randn(B * Gt * S, D, device=dev).to(torch.bfloat16)
    dy = torch.empty(B * S, D, device=dev, dtype=torch.bfloat16)
    nbytes = (dx.numel() + dy.numel()) * 2
    M = nbytes // (2 * 2 * D)
    src, dst = torch.randn(M, D, device=dev).to(torch.bfloat16), torch.empty(M, D, device=dev, dtype=torch.bfloat16)
    t_sum = timed(lambda: ops.slice_sum(dx, B, S, Gt, out=dy), reps)
    t_copy = timed(lambda: ops.copy_rows(src, dst, 1, M, 0, M, 0, M, D), reps)
    return dict(shape=[B, S, Gt, D], mbytes=round(nbytes / 1e6, 1),
                slice_sum=dict(ms=round(t_sum, 4), gb_per_s=round(nbytes / (t_sum * 1e-3) / 1e9, 1)),
                copy_rows=dict(ms=round(t_copy, 4), gb_per_s=round(2 * M * D * 2 / (t_copy * 1e-3) / 1e9, 1)))


def bench_image_finetune(name, reps, rounds, B=16, frames=16, recompute=None):
    """One fine-tuning iteration of the image eval on still images against the same iteration on the materialised repeated clip (the
    ATen repeat inside the iteration: the only route there was) and against the frozen iteration, the three arms taking turns inside
    this process in rotating order; ms and peak memory of each, the rows the patch-embed GEMM and its weight gradient see, and
    vj_slice_sum alone beside vj_copy_rows."""
    import statistics
    from jepa_amd.engine.finetune import EncoderFineTuner
    from jepa_amd.evals.image_classification_frozen import eval as IE
    model_name, res, C = IMAGE_CONFIGS[name]
    dev = "cuda"
    torch.manual_seed(0)

    def make(trainable):
        enc = vit.__dict__[model_name](img_size=res, patch_size=16, num_frames=frames, tubelet_size=2, uniform_power=True).to(dev)
        tuner = None
        if trainable:
            tuner = EncoderFineTuner(enc, layer_decay=0.75)
            enc.train_on_any_input()
        else:
            enc.eval()
            for p in enc.parameters():
                p.requires_grad = False
        clf = AttentiveClassifier(embed_dim=enc.embed_dim, num_heads=enc.num_heads, depth=1, num_classes=C).to(dev)
        return enc, tuner, clf, IE.init_opt(clf, iterations_per_epoch=1, start_lr=1e-4, ref_lr=1e-4, warmup=0, num_epochs=10 ** 6, wd=0.01)

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    enc_f, _, clf_f, opt_f = make(False)
    enc_t, tuner, clf_t, opt_t = make(True)
    images = torch.randn(B, 3, res, res, device=dev)
    labels = torch.randint(0, C, (B,))

    def step(optimizer, grad_scale):
        tuner.step(optimizer.param_groups[0]['lr'], 0.05, grad_scale=grad_scale)

    def repeated(imgs):     # a plain callable: run_one_epoch hands it the batch as it is
        return enc_t(imgs.unsqueeze(2).repeat(1, 1, frames, 1, 1))

    def iteration(encoder, clf, opt, mode=None, **kw):
        optimizer, scaler, sched, wd_sched = opt

        def run():
            enc_t.set_activation_recompute(mode)
            IE.run_one_epoch(dev, True, encoder, clf, scaler, optimizer, sched, wd_sched, [(images, labels)], False, **kw)
        return run

    tune = dict(features_grad=True, after_update=step)
    arms = {"still": iteration(enc_t, clf_t, opt_t, **tune), "repeat": iteration(repeated, clf_t, opt_t, **tune),
            "frozen": iteration(enc_f, clf_f, opt_f)}
    if recompute:
        arms[f"still_{recompute}"] = iteration(enc_t, clf_t, opt_t, mode=recompute, **tune)
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated() - base
    for fn in arms.values():        # warm-up: code load, and what stays allocated afterwards (workspaces, scratch, the probes' .grad
        fn()                        # tensors and Adam state) is in place before any arm's peak is taken
    peak = {}
    for arm, fn in arms.items():    # the peak memory of each arm's iteration on its own, above what is resident
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[arm] = round((torch.cuda.max_memory_allocated() - before) / 2 ** 30, 3)
    ms = {arm: [] for arm in arms}
    names = list(arms)
    for r in range(rounds):
        order = names[r % len(names):] + names[:r % len(names)]
        for arm in (order if r % 2 == 0 else order[::-1]):
            ms[arm].append(timed(arms[arm], reps))
    mean = {arm: statistics.mean(v) for arm, v in ms.items()}
    cells, gt = (res // 16) ** 2, frames // 2
    out = dict(config=f"{name}_finetune", batch=B, frames=frames, rounds=rounds, reps=reps, tokens_per_image=gt * cells,
               patch_embed_rows_still=B * cells, patch_embed_rows_repeat=B * gt * cells,
               packed_token_mib_still=round(B * cells * 1536 * 2 / 2 ** 20, 1),
               packed_token_mib_repeat=round(B * gt * cells * 1536 * 2 / 2 ** 20, 1),
               repeated_clip_mib=round(B * 3 * frames * res * res * 4 / 2 ** 20, 1),
               resident_gib_both_models=round(resident / 2 ** 30, 2))
    for arm in arms:
        out[f"{arm}_ms_rounds"] = [round(v, 2) for v in ms[arm]]
        out[f"{arm}_iteration_ms"] = round(mean[arm], 2)
        out[f"{arm}_ms_spread"] = round(max(ms[arm]) - min(ms[arm]), 2)
        out[f"peak_mem_gib_{arm}_iteration"] = peak[arm]
    out["still_minus_repeat_ms_rounds"] = [round(a - b, 2) for a, b in zip(ms["still"], ms["repeat"])]
    out["still_minus_repeat_ms"] = round(mean["still"] - mean["repeat"], 2)
    if recompute:
        enc_t.set_activation_recompute(None)
        out["recompute"] = recompute
        out[f"{recompute}_minus_still_ms_rounds"] = [round(a - b, 2) for a, b in zip(ms[f"still_{recompute}"], ms["still"])]
        out[f"{recompute}_over_still"] = round(mean[f"still_{recompute}"] / mean["still"], 3)
    out["slice_sum_kernel"] = bench_slice_sum(B, cells, gt, enc_t.embed_dim)
    return out


def bench_interp():
    """vj_pos_interp3d, one launch per new size (the table is cached afterwards), timed by events after an unrelated warm-up launch."""
    from jepa_amd.hip import ops
    from jepa_amd.src.models.utils.pos_embs import get_3d_sincos_pos_embed
    dev = "cuda"
    warm = torch.zeros(2, 2, 2, 64, device=dev)
    ops.pos_interp3d(warm, (2.0, 2.0, 2.0))
    torch.cuda.synchronize()
    out = []
    for model, D, src, dst in INTERP_CASES:
        table = torch.from_numpy(get_3d_sincos_pos_embed(D, src[1], src[0], cls_token=False, uniform_power=True)).float().to(dev)
        table = table.view(*src, D)
        scale = tuple(d / s for d, s in zip(dst, src))
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        o = ops.pos_interp3d(table, scale)
        e.record()
        torch.cuda.synchronize()
        out.append(dict(model=model, D=D, src_grid=list(src), dst_grid=list(dst), first_call_us=round(s.elapsed_time(e) * 1e3, 1),
                        repeat_call_us=round(timed(lambda: ops.pos_interp3d(table, scale), 20) * 1e3, 1),
                        out_mib=round(o.numel() * 4 / 2 ** 20, 2)))
    return dict(pos_interp3d=out)


def bench_frames(reps, rounds, B=2, S=8, V=3, T=16, res=224, max_frames=1024):
    import math
    import statistics
    from jepa_amd.evals.video_classification_frozen.utils import FrameAggregation
    from jepa_amd.hip import ops
    from jepa_amd.src.models.utils.pos_embs import get_2d_sincos_pos_embed
    dev = "cuda"
    torch.manual_seed(0)
    model = vit.vit_large(img_size=res, patch_size=16).to(dev).eval()
    for p in model.parameters():
        p.requires_grad = False
    agg = FrameAggregation(model).to(dev)
    agg_pos = FrameAggregation(model, max_frames=max_frames, use_pos_embed=True).to(dev)
    agg_one = FrameAggregation(model).to(dev)
    agg_one.max_tokens_per_call = B * T * model.num_patches      # one (segment, view) tensor per trunk call: what the batching buys
    clips = [[torch.randn(B, 3, T, res, res, device=dev) for _ in range(V)] for _ in range(S)]
    idx = [torch.arange(s * T * 4, (s + 1) * T * 4, 4, device=dev).repeat(B, 1) for s in range(S)]
    N = model.num_patches
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()

    def direct():
        with torch.no_grad():
            return agg(clips, idx)

    def permuted():     # the reference's FrameAggregation.forward (utils.py:53-72) on this model
        with torch.no_grad():
            x = torch.cat([torch.cat(xi, dim=0) for xi in clips], dim=2)
            b, c, t, h, w = x.size()
            out = model(x.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w)).reshape(b, t, N, -1).flatten(1, 2)
            return [out[i * B:(i + 1) * B] for i in range(V)]

    def per_clip():
        with torch.no_grad():
            return agg_one(clips, idx)

    arms = {"direct": direct, "permuted": permuted, "per_clip": per_clip}
    peak, outs = {}, {}
    for arm, fn in arms.items():    # warm-up (workspace growth, code load) and the peak memory of each route on its own
        torch.cuda.reset_peak_memory_stats()
        outs[arm] = fn()
        torch.cuda.synchronize()
        peak[arm] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 30, 3)
    equal = all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(outs["direct"], outs["permuted"], outs["per_clip"]))
    del outs
    ms = {arm: [] for arm in arms}
    for r in range(rounds):
        for arm in (("direct", "permuted", "per_clip") if r % 2 == 0 else ("per_clip", "permuted", "direct")):
            ms[arm].append(timed(arms[arm], reps))
    mean = {arm: statistics.mean(v) for arm, v in ms.items()}
    spread = {arm: max(v) - min(v) for arm, v in ms.items()}

    def with_pos():
        with torch.no_grad():
            return agg_pos(clips, idx)

    t_pos = timed(with_pos, reps)
    frames = B * S * V * T
    # the bicubic table of a new size: one launch (cached afterwards), timed by events after an unrelated warm-up launch
    ops.pos_interp2d_bicubic(torch.zeros(2, 2, 64, device=dev), 2.0)
    table = torch.from_numpy(get_2d_sincos_pos_embed(1024, 14, cls_token=False)).float().to(dev).view(14, 14, 1024)
    scale = math.sqrt(24 * 24 / (14 * 14))
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    ops.pos_interp2d_bicubic(table, scale)
    e.record()
    torch.cuda.synchronize()
    return dict(config="vitl16_image_frames", frames=frames, tokens_per_frame=N, rounds=rounds, reps=reps, outputs_equal=equal,
                direct_ms_rounds=[round(v, 3) for v in ms["direct"]], permuted_ms_rounds=[round(v, 3) for v in ms["permuted"]],
                per_clip_ms_rounds=[round(v, 3) for v in ms["per_clip"]], per_clip_ms_mean=round(mean["per_clip"], 3),
                per_clip_ms_spread=round(spread["per_clip"], 3), peak_mem_gib_per_clip=peak["per_clip"],
                direct_ms_mean=round(mean["direct"], 3), permuted_ms_mean=round(mean["permuted"], 3),
                direct_ms_spread=round(spread["direct"], 3), permuted_ms_spread=round(spread["permuted"], 3),
                direct_minus_permuted_ms=round(mean["direct"] - mean["permuted"], 3),
                direct_not_slower_than_permuted_plus_its_spread=bool(mean["direct"] <= mean["permuted"] + spread["permuted"]),
                frames_per_s_direct=round(frames / mean["direct"] * 1e3, 1), frames_per_s_permuted=round(frames / mean["permuted"] * 1e3, 1),
                peak_mem_gib_direct=peak["direct"], peak_mem_gib_permuted=peak["permuted"],
                with_temporal_pos_ms=round(t_pos, 3), temporal_pos_extra_ms=round(t_pos - mean["direct"], 3),
                bicubic_14x14x1024_to_24x24=dict(first_call_us=round(s.elapsed_time(e) * 1e3, 1),
                                                 repeat_call_us=round(timed(lambda: ops.pos_interp2d_bicubic(table, scale), 20) * 1e3, 1)))


def bench_uint8(reps, rounds, B=4, name="vitl16_k400_16x8x3"):
    import random
    import statistics
    import time

    import numpy as np
    from jepa_amd.engine.input import EvalPrefetcher
    from jepa_amd.evals.video_classification_frozen.utils import make_transforms
    from jepa_amd.hip import ops
    model_name, res, S, V, C = CONFIGS[name]
    dev, T = "cuda", 16
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    enc = ClipAggregation(vit.__dict__[model_name](img_size=res, patch_size=16, num_frames=T, tubelet_size=2, uniform_power=True),
                          tubelet_size=2, attend_across_segments=True).to(dev).eval()
    for p in enc.parameters():
        p.requires_grad = False
    clf = AttentiveClassifier(embed_dim=enc.embed_dim, num_heads=enc.num_heads, depth=1, num_classes=C).to(dev)
    opt, scaler, sched, wd_sched = init_opt(clf, iterations_per_epoch=1, start_lr=1e-4, ref_lr=1e-4, warmup=0,
                                            num_epochs=10 ** 6, wd=0.01)
    g = torch.Generator().manual_seed(0)
    labels = torch.randint(0, C, (B,), generator=g)

    def host_batch(training):
        """(uint8 batch, the same batch as pinned fp32 views) in the loader's layout."""
        tf = make_transforms(training=training, num_views_per_clip=1 if training else V, random_horizontal_flip=False,
                             random_resize_aspect_ratio=(0.75, 4 / 3), random_resize_scale=(0.08, 1.0), reprob=0.25, crop_size=res)
        hw = (240, 320) if training else (res, res * 4 // 3)       # a 4:3 source as decoded / after the reference's Resize(224)
        items = [([tf(torch.randint(0, 256, (T,) + hw + (3,), generator=g, dtype=torch.uint8)) for _ in range(S)], int(labels[b]),
                  [torch.arange(T) * 4 + s * 64 for s in range(S)]) for b in range(B)]
        segs, lab, idx = torch.utils.data.default_collate(items)
        segs = [s.pin_memory() for s in segs]
        views = []
        for raw in segs:
            frames, desc, boxes = raw.to(dev)
            out = ops.clip_transform(frames, desc, boxes, raw.crop_size, raw.mean, raw.std, pre=True)
            if raw.erased:
                ops.clip_erase(out, raw.ebox.to(dev), raw.noise.to(dev), raw.noise_off.to(dev))
            n = len(raw) // raw.num_views
            views.append([out[v * n:(v + 1) * n].cpu().pin_memory() for v in range(raw.num_views)])
        return (segs, lab, idx), (views, lab, idx)

    def kernels_alone(segs):
        raw = segs[0]
        frames, desc, boxes = raw.to(dev)
        out = torch.empty((len(raw), 3, T, res, res), device=dev)
        t_tf = timed(lambda: ops.clip_transform(frames, desc, boxes, raw.crop_size, raw.mean, raw.std, out=out, pre=True), 10)
        er = next((s for s in segs if s.erased), None)
        t_er = None
        if er is not None:
            eb, nz, no = er.ebox.to(dev), er.noise.to(dev), er.noise_off.to(dev)
            t_er = timed(lambda: ops.clip_erase(out, eb, nz, no), 10)
        return t_tf, t_er

    def copies_alone(views):
        return timed(lambda: [[v.to(dev, non_blocking=True) for v in seg] for seg in views], 3)

    out = {}
    for training in (True, False):
        raw, fp32 = host_batch(training)
        args = (1, S, True) if training else (V, S, True)
        n_it = reps + 1
        rows = []
        for r in range(rounds):
            order = ("fp32", "uint8") if r % 2 == 0 else ("uint8", "fp32")
            row = {}
            for arm in order:
                pf = EvalPrefetcher([raw] * n_it, torch.device(dev), timing=True) if arm == "uint8" else None
                loader = pf if pf is not None else [fp32] * n_it
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_one_epoch(dev, training, enc, clf, scaler, opt, sched, wd_sched, loader, False, *args)
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) * 1e3 / n_it
                if pf is not None:
                    waits = [max(0.0, a.elapsed_time(b)) for a, b in pf.edge_events]
                    row[arm] = dict(h2d_mb=round(pf.bytes_copied / n_it / 1e6, 1), iteration_ms=round(wall, 2),
                                    edge_wait_ms_first=round(waits[0], 2), edge_wait_ms_rest=round(statistics.mean(waits[1:]), 3))
                else:
                    nbytes = sum(v.numel() * 4 for seg in fp32[0] for v in seg)
                    row[arm] = dict(h2d_mb=round(nbytes / 1e6, 1), iteration_ms=round(wall, 2),
                                    edge_wait_ms=round(copies_alone(fp32[0]), 2))
            row["uint8_faster"] = row["uint8"]["iteration_ms"] < row["fp32"]["iteration_ms"]
            rows.append(row)
        t_tf, t_er = kernels_alone(raw[0])
        out["train" if training else "val"] = dict(
            rounds=rows, uint8_faster_in_every_round=all(r["uint8_faster"] for r in rows),
            clip_transform_pre_ms_per_segment=round(t_tf, 3), clip_erase_ms_per_segment=None if t_er is None else round(t_er, 4),
            rows_per_segment=len(raw[0][0]), erased_clips=int(sum(int((s.ebox[:, 2] > 0).sum()) for s in raw[0])),
            noise_mb=round(sum(s.noise.numel() for s in raw[0]) * 4 / 1e6, 3))
        del raw, fp32
        torch.cuda.empty_cache()
    return dict(config=name, batch=B, reps=reps, iterations_per_arm=reps + 1, **out)


def bench_drop_path_kernels(M, D, B, reps=20):
    """The two stochastic-depth kernels and vj_copy_rows alone on M x D bf16 rows of B samples, every sample kept (the most
    bytes: a dropped sample's branch rows are not read): ms and bytes/s by the bytes each must move."""
    from jepa_amd.hip import ops
    dev = "cuda"
    x = torch.randn(M, D, device=dev).to(torch.bfloat16)
    y = torch.randn(M, D, device=dev).to(torch.bfloat16)
    out = torch.empty_like(x)
    s = torch.ones(B, device=dev)          # y <- x + y: stays finite over the repetitions
    S = M // B
    ms = dict(drop_path_add=(timed(lambda: ops.drop_path_add(x, y, s, B, S), reps), 3),
              drop_path_scale=(timed(lambda: ops.drop_path_scale(x, s, B, S, out=out), reps), 2),
              copy_rows=(timed(lambda: ops.copy_rows(x, out, 1, M, 0, M, 0, M, D), reps), 2))
    res = {}
    for k, (t, streams) in ms.items():
        res[k] = dict(ms=round(t, 4), streams=streams, tb_per_s=round(streams * M * D * 2 / (t * 1e-3) / 1e12, 3))
    return dict(rows=M, cols=D, samples=B, **res)


MIX_RECIPE = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, label_smoothing=0.1, seed=0)


def bench_mix_kernels(B=4, T=16, res=224, reps=20):
    """vj_clip_mix alone on one segment batch [B,3,T,res,res] -- a mixup plan (every byte is read and written once) and a cutmix
    plan with a centred box of half the side (a quarter of the bytes) -- beside vj_copy_rows on the bytes of the batch (read and
    written once each as well); vj_soft_ce with the soft-max output at R = B rows of 400 and 1000 classes."""
    from jepa_amd.hip import ops
    dev = "cuda"
    x = torch.randn(B, 3, T, res, res, device=dev)
    nbytes = x.numel() * 4
    D = 1024
    M = nbytes // (2 * D)
    src, dst = torch.randn(M, D, device=dev).to(torch.bfloat16), torch.empty(M, D, device=dev, dtype=torch.bfloat16)
    q = res // 4
    mixup = ops.mix_tables([0.5] * B, [[0, 0, 0, 0]] * B, res, res, dev)
    cutmix = ops.mix_tables([1.0] * B, [[q, 3 * q, q, 3 * q]] * B, res, res, dev)
    t_mixup = timed(lambda: ops.clip_mix(x, *mixup), reps)
    t_cutmix = timed(lambda: ops.clip_mix(x, *cutmix), reps)
    t_copy = timed(lambda: ops.copy_rows(src, dst, 1, M, 0, M, 0, M, D), reps)
    res_ = dict(shape=list(x.shape), mbytes=round(nbytes / 1e6, 1),
                clip_mix_mixup=dict(ms=round(t_mixup, 4), tb_per_s=round(2 * nbytes / (t_mixup * 1e-3) / 1e12, 3)),
                clip_mix_cutmix_quarter=dict(ms=round(t_cutmix, 4), tb_per_s=round(2 * (nbytes // 4) / (t_cutmix * 1e-3) / 1e12, 3)),
                copy_rows=dict(ms=round(t_copy, 4), tb_per_s=round(2 * M * D * 2 / (t_copy * 1e-3) / 1e12, 3)))
    for C in (400, 1000):
        z = torch.randn(B, C, device=dev)
        labels = torch.randint(0, C, (B,))
        tables = ops.soft_ce_tables(labels, labels.flip(0), [0.5] * B, C, dev)
        res_[f"soft_ce_C{C}_ms"] = round(timed(lambda: ops.soft_ce(z, *tables, 0.1, probs=True), reps), 4)
    return res_


def _one_rank_group():
    """The one-rank RCCL group of --dp1, created once per process."""
    import socket
    import torch.distributed as dist
    if dist.is_initialized():
        return
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))


def bench_finetune(reps, rounds, S, B=4, model_name="vit_large", res=224, C=400, drop_path=None, mix=False, recompute=None,
                   frozen_arm=True, dp1=False):
    from jepa_amd.evals.mix import MixDraw
    import statistics
    from jepa_amd.engine.finetune import EncoderFineTuner
    dev = "cuda"
    torch.manual_seed(0)

    def make(trainable):
        model = vit.__dict__[model_name](img_size=res, patch_size=16, num_frames=16, tubelet_size=2, uniform_power=True).to(dev)
        agg = ClipAggregation(model, tubelet_size=2, attend_across_segments=True).to(dev)
        tuner = None
        if trainable:
            if dp1:
                _one_rank_group()
                forced = os.environ.get("VJ_FORCE_DP")
                os.environ["VJ_FORCE_DP"] = "1"
            tuner = EncoderFineTuner(model, layer_decay=0.75)
            if dp1 and forced is None:
                del os.environ["VJ_FORCE_DP"]
            elif dp1:
                os.environ["VJ_FORCE_DP"] = forced
        else:
            agg.eval()
            for p in agg.parameters():
                p.requires_grad = False
        clf = AttentiveClassifier(embed_dim=agg.embed_dim, num_heads=agg.num_heads, depth=1, num_classes=C).to(dev)
        return agg, tuner, clf, init_opt(clf, iterations_per_epoch=1, start_lr=1e-4, ref_lr=1e-4, warmup=0, num_epochs=10 ** 6, wd=0.01)

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    enc_f, _, clf_f, (opt_f, scaler_f, sched_f, wd_f) = make(False)
    enc_t, tuner, clf_t, (opt_t, scaler_t, sched_t, wd_t) = make(True)
    labels = torch.randint(0, C, (B,))
    train = ([[torch.randn(B, 3, 16, res, res, device=dev)] for _ in range(S)], labels, [torch.arange(16) for _ in range(S)])

    def step(optimizer, grad_scale):
        tuner.step(optimizer.param_groups[0]['lr'], 0.05, grad_scale=grad_scale)

    def finetune_at(rate, mix=None, recompute=None, reducer=None):
        def run():
            enc_t.model.grad_reducer = reducer      # (None: the backward issues the call it always has)
            enc_t.model.set_drop_path_rate(rate)
            enc_t.model.set_activation_recompute(recompute)
            run_one_epoch(dev, True, enc_t, clf_t, scaler_t, opt_t, sched_t, wd_t, [train], False, 1, S, True,
                          features_grad=True, after_update=step, mix=mix)
        return run

    arms = {"frozen": lambda: run_one_epoch(dev, True, enc_f, clf_f, scaler_f, opt_f, sched_f, wd_f, [train], False, 1, S, True),
            "finetune": finetune_at(0.0)}
    if drop_path:
        arms["finetune_drop"] = finetune_at(drop_path)
    if mix:
        # (the clips are mixed in place iteration after iteration: convex combinations and swaps, they stay what they were in scale)
        arms["finetune_mix"] = finetune_at(0.0, MixDraw(num_classes=C, **MIX_RECIPE))
    if recompute:
        arms[f"finetune_{recompute}"] = finetune_at(0.0, recompute=recompute)
    if dp1:
        arms["finetune_dp1"] = finetune_at(0.0, reducer=tuner.reducer)
    if not frozen_arm:      # (a model too large for two copies and the plain arm's activations: the fine-tuning arms alone)
        del arms["frozen"]
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated() - base
    peak, reserved = {}, {}
    for arm, fn in arms.items():    # warm-up (workspace growth, code load) and the peak memory of each arm on its own
        torch.cuda.synchronize()
        torch.cuda.empty_cache()    # so that what the allocator holds at this arm's peak is this arm's
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[arm] = round((torch.cuda.max_memory_allocated() - before) / 2 ** 30, 2)
        reserved[arm] = round(torch.cuda.max_memory_reserved() / 2 ** 30, 2)
    ms = {arm: [] for arm in arms}
    names = list(arms)
    for r in range(rounds):
        # two arms: the two orders in turn; three: the order rotates, reversed every other round
        order = names[r % len(names):] + names[:r % len(names)]
        for arm in (order if r % 2 == 0 or len(names) == 2 else order[::-1]):
            ms[arm].append(timed(arms[arm], reps))
    enc_t.model.set_drop_path_rate(0.0)
    enc_t.model.set_activation_recompute(None)
    mean = {arm: statistics.mean(v) for arm, v in ms.items()}
    drop = {}
    if dp1:
        red, d = tuner.reducer, ms["finetune_dp1"]
        arms["finetune_dp1"]()      # (the last arm timed may have been another: `launched` and the exposed samples are this arm's)
        drop.update(finetune_dp1_ms_rounds=[round(v, 2) for v in d], finetune_dp1_iteration_ms=round(mean["finetune_dp1"], 2),
                    finetune_dp1_ms_spread=round(max(d) - min(d), 2),
                    dp1_minus_plain_ms_rounds=[round(a - b, 2) for a, b in zip(d, ms["finetune"])],
                    dp1_minus_plain_ms=round(mean["finetune_dp1"] - mean["finetune"], 2),
                    peak_mem_gib_finetune_dp1_iteration=peak["finetune_dp1"],
                    dp=dict(world=1, route=red.route, coll_mode=red.coll_mode, coll_check=red.coll_check,
                            buckets=len(red.buckets), tail_collectives=len(red.tail), collectives_per_iteration=len(red.launched),
                            exposed_ms=None if red.exposed_ms() is None else round(red.exposed_ms(), 4),
                            exposed_samples=red.exposed_samples,
                            bucket_mib=[round((hi - lo) * 4 / 2 ** 20, 2) for lo, hi in sorted({r for rs in red.buckets.values() for r in rs})][:3],
                            tail_kib=round(sum(hi - lo for lo, hi in red.tail) * 4 / 2 ** 10, 1)))
        enc_t.model.grad_reducer = None
    if recompute:
        arm = f"finetune_{recompute}"
        d = ms[arm]
        drop.update({"recompute": recompute, f"{arm}_ms_rounds": [round(v, 2) for v in d], f"{arm}_iteration_ms": round(mean[arm], 2),
                     f"{arm}_ms_spread": round(max(d) - min(d), 2),
                     f"{recompute}_minus_plain_ms_rounds": [round(a - b, 2) for a, b in zip(d, ms["finetune"])],
                     f"{recompute}_minus_plain_ms": round(mean[arm] - mean["finetune"], 2),
                     f"{recompute}_over_plain": round(mean[arm] / mean["finetune"], 3),
                     f"peak_mem_gib_{arm}_iteration": peak[arm]})
    drop["peak_reserved_gib_process"] = reserved     # (the whole process: both models and the clips included)
    if not frozen_arm:
        ms["frozen"], mean["frozen"], peak["frozen"] = [float("nan")], float("nan"), None
    if drop_path:
        d = ms["finetune_drop"]
        drop = dict(drop_path=drop_path, finetune_drop_ms_rounds=[round(v, 2) for v in d],
                    finetune_drop_iteration_ms=round(mean["finetune_drop"], 2), finetune_drop_ms_spread=round(max(d) - min(d), 2),
                    drop_minus_rate0_ms_rounds=[round(a - b, 2) for a, b in zip(d, ms["finetune"])],
                    drop_minus_rate0_ms=round(mean["finetune_drop"] - mean["finetune"], 2),
                    peak_mem_gib_finetune_drop_iteration=peak["finetune_drop"],
                    drop_path_kernels=bench_drop_path_kernels(S * B * enc_t.model.num_patches, enc_t.embed_dim, S * B))
    if mix:
        d = ms["finetune_mix"]
        drop.update(mix=MIX_RECIPE, finetune_mix_ms_rounds=[round(v, 2) for v in d],
                    finetune_mix_iteration_ms=round(mean["finetune_mix"], 2), finetune_mix_ms_spread=round(max(d) - min(d), 2),
                    mix_minus_plain_ms_rounds=[round(a - b, 2) for a, b in zip(d, ms["finetune"])],
                    mix_minus_plain_ms=round(mean["finetune_mix"] - mean["finetune"], 2),
                    peak_mem_gib_finetune_mix_iteration=peak["finetune_mix"], mix_kernels=bench_mix_kernels(B=B, res=res))
    t_step = [timed(lambda: tuner.step(1e-4, 0.05), 10) for _ in range(3)]
    t_refresh = timed(tuner.arena.refresh_transposed, 10)
    upd = statistics.mean(t_step)
    return dict(config=f"{model_name}_16x{res}_finetune", batch=B, segments=S, clips=S * B, rounds=rounds, reps=reps,
                frozen_ms_rounds=[round(v, 2) for v in ms["frozen"]], finetune_ms_rounds=[round(v, 2) for v in ms["finetune"]],
                frozen_iteration_ms=round(mean["frozen"], 2), finetune_iteration_ms=round(mean["finetune"], 2),
                frozen_ms_spread=round(max(ms["frozen"]) - min(ms["frozen"]), 2),
                finetune_ms_spread=round(max(ms["finetune"]) - min(ms["finetune"]), 2),
                peak_mem_gib_frozen_iteration=peak["frozen"], peak_mem_gib_finetune_iteration=peak["finetune"],
                resident_gib_both_models=round(resident / 2 ** 30, 2),
                update_ranges=len(tuner.param_groups), update_launches=len(tuner.param_groups) + 4,
                update_ms_runs=[round(v, 3) for v in t_step], update_ms=round(upd, 3), update_transposed_refresh_ms=round(t_refresh, 3),
                update_share_of_iteration_pct=round(100 * upd / mean["finetune"], 2), **drop)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--finetune", action="store_true", help="one fine-tuning iteration against the frozen iteration (ViT-L/16, batch 4)")
    ap.add_argument("--segments", nargs="*", type=int, default=[1, 8])
    ap.add_argument("--drop-path", type=float, default=None, help="with --finetune: a third arm, fine-tuning with stochastic depth at this rate")
    ap.add_argument("--mix", action="store_true", help="with --finetune: another arm, fine-tuning with mixup / cutmix / label smoothing")
    ap.add_argument("--recompute", choices=["mlp", "block"], default=None,
                    help="with --finetune: another arm, fine-tuning with this activation-recomputation mode")
    ap.add_argument("--dp1", action="store_true",
                    help="with --finetune: another arm, the fine-tuning iteration with the data-parallel reducer forced in a one-rank RCCL group")
    ap.add_argument("--model", nargs=2, default=["vit_large", "224"], metavar=("NAME", "RES"),
                    help="with --finetune: the encoder factory and the clip resolution (default vit_large 224)")
    ap.add_argument("--batch", type=int, default=4, help="with --finetune: clips per segment")
    ap.add_argument("--no-frozen", action="store_true", help="with --finetune: leave the frozen arm out (the fine-tuning arms alone)")
    ap.add_argument("--uint8", action="store_true", help="the video eval's input edge: fp32 views + .to(device) against uint8 frames + prefetch")
    ap.add_argument("--frames", action="store_true", help="FrameAggregation on the ViT-L/16 image model instead of the video eval")
    ap.add_argument("--image", action="store_true", help="the image-classification eval instead of the video one")
    ap.add_argument("--image-configs", nargs="*", default=["vitl16_in1k", "vith16_384_in1k"], choices=sorted(IMAGE_CONFIGS))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--configs", nargs="*", default=["vitl16_k400_16x8x3", "vith16_384_k400_16x8x3"], choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--bank", type=int, default=0, help="also time the training iteration with a bank of this many probes")
    a = ap.parse_args()
    if a.image and a.finetune:
        for name in a.image_configs:
            print(json.dumps(bench_image_finetune(name, a.reps, a.rounds, recompute=a.recompute)), flush=True)
            torch.cuda.empty_cache()
        return
    if a.finetune:
        for S in a.segments:
            print(json.dumps(bench_finetune(a.reps, a.rounds, S, drop_path=a.drop_path, mix=a.mix, recompute=a.recompute,
                                            B=a.batch, model_name=a.model[0], res=int(a.model[1]), frozen_arm=not a.no_frozen,
                                            dp1=a.dp1)),
                  flush=True)
            torch.cuda.empty_cache()
        return
    if a.uint8:
        print(json.dumps(bench_uint8(a.reps, a.rounds)), flush=True)
        return
    if a.frames:
        print(json.dumps(bench_frames(a.reps, a.rounds)), flush=True)
        return
    if a.image:
        for name in a.image_configs:
            print(json.dumps(bench_image(name, a.reps, a.rounds)), flush=True)
            torch.cuda.empty_cache()
        print(json.dumps(bench_interp()), flush=True)
        return
    for name in a.configs:
        print(json.dumps(bench(name, a.reps, bank=a.bank)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
