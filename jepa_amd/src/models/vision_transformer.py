"""Vision Transformer (video, and image with num_frames=1) with the reference's constructor, factories, attributes and state-dict names
(src/models/vision_transformer.py:21-307), computing on MI355X through the jepa_amd HIP kernels.

    vit = vit_large(img_size=224, patch_size=16, num_frames=16, tubelet_size=2, uniform_power=True)
    out = vit(clips)                  # [B, N, D]
    out = vit(clips, masks=[idx])     # [B*len(masks), K, D]   (reference contract: masks share K)

`forward` is differentiable (one autograd node per call whose backward is the hand-written layer chain; with `drop_path_rate` > 0
a training-mode forward that records a backward applies stochastic depth, see set_drop_path_rate), but
the pretraining step (jepa_amd.engine.step.Trainer) bypasses autograd entirely and shares this module's
parameters through flat arenas.  With gradients enabled the video model takes clips of its native size; still images [B,3,H,W] and
other clip sizes are frozen / no-grad inputs unless the module opted in (train_on_any_input).

    img = vit_large(img_size=224, patch_size=16)       # num_frames=1: the 2-D image ViT (Conv2d patch embed, 2-D sincos table)
    out = img(images)                                  # [B, N, D] from fp32 [B,3,H,W]; frozen / no-grad path only

The image model is the frozen evals' encoder for image-pretrained checkpoints: its position table is interpolated
bicubically at other square sizes (vj_pos_interp2d_bicubic) and FrameAggregation drives it frame by frame through
`forward_frames`.
"""
import math
import weakref
from functools import partial
from typing import NamedTuple

import torch
import torch.nn as nn

from ...engine import hipmodule
from ...engine.chain import Workspace
from ...engine.layers import encoder_backward, encoder_forward, recompute_mode
from ...engine.streams import side_stream
from ..utils.tensors import trunc_normal_
from .utils.modules import Block
from .utils.patch_embed import PatchEmbed, PatchEmbed3D
from .utils.pos_embs import get_2d_sincos_pos_embed, get_3d_sincos_pos_embed


class _Input(NamedTuple):
    """What VisionTransformer._describe found an input to be."""
    T: int          # the clip the input stands for
    H: int
    W: int
    still: bool     # a video encoder's still images [B,C,H,W]
    native: bool    # (T, H, W) is the size the model was built for: the arena's position table fits
    drops: bool     # stochastic depth applies: a video encoder's clips and still images; never the image model


class VisionTransformer(nn.Module, hipmodule.HipModule):
    """ Vision Transformer """

    def __init__(self, img_size=224, patch_size=16, num_frames=1, tubelet_size=2, in_chans=3, embed_dim=768,
                 depth=12, num_heads=12, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop_rate=0.0,
                 attn_drop_rate=0.0, norm_layer=nn.LayerNorm, init_std=0.02, out_layers=None, uniform_power=False,
                 drop_path_rate=0.0, **kwargs):
        super().__init__()
        self.drop_path_generator = None     # a torch.Generator of the model's device for the draws; None: the default generator
        self.last_drop_path_scales = None   # fp32 [L, 2, B]: the scales of the latest forward that dropped anything
        self.set_drop_path_rate(drop_path_rate, depth)
        self.any_input_trains = False       # train_on_any_input: still images and off-native sizes with gradients enabled
        self.activation_recompute = None    # set_activation_recompute: None (off), "mlp" or "block"
        self.grad_reducer = None            # an engine.dp.GradReducer over the arena that owns the parameters (set by a data-parallel
        #                                     EncoderFineTuner; not part of the state dict): the backward launches its buckets
        self.num_features = self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.out_layers = out_layers
        self.input_size = img_size
        self.patch_size = patch_size
        self.num_frames = num_frames
        self.tubelet_size = tubelet_size
        self.is_video = num_frames > 1
        if in_chans != 3 or not qkv_bias or out_layers is not None:
            raise NotImplementedError("only in_chans=3, qkv_bias=True, out_layers=None (the pretraining setup)")
        grid_size = img_size // patch_size
        grid_depth = num_frames // tubelet_size
        if self.is_video:
            self.patch_embed = PatchEmbed3D(patch_size=patch_size, tubelet_size=tubelet_size, in_chans=in_chans,
                                            embed_dim=embed_dim)
            self.num_patches = grid_depth * grid_size * grid_size
        else:
            if patch_size % 8:
                raise ValueError(f"image ViT: patch_size={patch_size} must be a multiple of 8 (the patch rows are packed 8 pixels "
                                 "at a time, vj_tubelet_pack)")
            self.patch_embed = PatchEmbed(patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim)
            self.num_patches = grid_size * grid_size
        self.uniform_power = uniform_power
        self.pos_embed = nn.Parameter(torch.zeros(1, self.num_patches, embed_dim), requires_grad=False)
        self.blocks = nn.ModuleList([
            Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                  drop=drop_rate, act_layer=nn.GELU, grid_size=grid_size, grid_depth=grid_depth,
                  attn_drop=attn_drop_rate, norm_layer=norm_layer) for _ in range(depth)])
        self.norm = norm_layer(embed_dim)
        # ---- weights: sincos table, trunc-normal(0.02) matrices, zero biases, unit norms, depth rescale
        if self.is_video:
            sincos = get_3d_sincos_pos_embed(embed_dim, grid_size, grid_depth, cls_token=False,
                                             uniform_power=uniform_power)
        else:
            sincos = get_2d_sincos_pos_embed(embed_dim, grid_size, cls_token=False)
        self.pos_embed.data.copy_(torch.from_numpy(sincos).float().unsqueeze(0))
        self.init_std = init_std
        self.apply(self._init_weights)
        self._rescale_blocks()

    def _init_weights(self, m):
        if isinstance(m, (nn.Linear, nn.Conv2d, nn.Conv3d)):
            trunc_normal_(m.weight, std=self.init_std)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def _rescale_blocks(self):
        for layer_id, layer in enumerate(self.blocks):
            layer.attn.proj.weight.data.div_(math.sqrt(2.0 * (layer_id + 1)))
            layer.mlp.fc2.weight.data.div_(math.sqrt(2.0 * (layer_id + 1)))

    def get_num_layers(self):
        return len(self.blocks)

    # ---- stochastic depth ---------------------------------------------------------------------------------
    def set_drop_path_rate(self, rate, depth=None):
        """Block i of L drops each of its two branches (attention, MLP) per sample with probability rate * i / (L - 1), the ViT
        lineage's torch.linspace(0, rate, L) -- while the module is in training mode and the forward records a backward; the
        frozen / no-grad path, eval() and the image encoder never drop."""
        rate = float(rate)
        if not 0.0 <= rate < 1.0:
            raise ValueError(f"drop_path_rate={rate} must lie in [0, 1)")
        depth = len(self.blocks) if depth is None else depth
        self.drop_path_rate = rate
        self.drop_path_rates = [rate * i / (depth - 1) if depth > 1 else 0.0 for i in range(depth)]
        self.__dict__.pop("_drop_keep", None)

    def set_drop_path_scales(self, scales):
        """The next forward that records a backward in training mode takes these scales instead of drawing: fp32 [L, 2, B] on the
        model's device, scales[i, 0] / scales[i, 1] multiplying the attention / MLP branch of block i per clip (0 drops it; a draw
        gives 0 or 1 / keep_i).  Used once; None withdraws them."""
        if scales is not None:
            if scales.dim() != 3 or tuple(scales.shape[:2]) != (len(self.blocks), 2) or scales.dtype != torch.float32:
                raise ValueError(f"set_drop_path_scales: expected float32 [{len(self.blocks)}, 2, B], got {scales.dtype} "
                                 f"{tuple(scales.shape)}")
            scales = scales.detach().contiguous()
        self.__dict__["_drop_scales_next"] = scales

    def _drop_path_entries(self, x, inp):
        """The per-block (s_attn, s_mlp) list of engine.layers for a grad-recording forward of the input x that `inp` describes, or
        None: nothing drops.  One torch.rand((L, 2, B)) on the device per forward, no host synchronisation; s = floor(keep + u) /
        keep.  A branch whose rate is 0 gets no scale and keeps the fused residual add.  `last_drop_path_scales` holds what the
        forward used."""
        self.__dict__["last_drop_path_scales"] = None
        if not self.training or not inp.drops:
            return None
        L, B = len(self.blocks), x.shape[0]
        s = self.__dict__.get("_drop_scales_next")
        if s is not None:
            if s.shape[2] != B or s.device != x.device:
                raise ValueError(f"set_drop_path_scales: scales {tuple(s.shape)} on {s.device} do not fit a batch of {B} clips on "
                                 f"{x.device}")
            self.__dict__["_drop_scales_next"] = None
            self.__dict__["last_drop_path_scales"] = s
            return [(s[i, 0], s[i, 1]) for i in range(L)]
        if self.drop_path_rate == 0.0:
            return None
        keep = self.__dict__.get("_drop_keep")
        if keep is None or keep.device != x.device:
            keep = self.__dict__["_drop_keep"] = (1.0 - torch.tensor(self.drop_path_rates, dtype=torch.float32)).view(L, 1, 1).to(x.device)
        u = torch.rand((L, 2, B), device=x.device, generator=self.drop_path_generator)
        s = torch.floor(keep + u).clamp_(max=1.0) / keep      # (the clamp: keep + u can round up to 2 at u = 1 - 2^-24)
        self.__dict__["last_drop_path_scales"] = s
        return [(s[i, 0], s[i, 1]) if self.drop_path_rates[i] > 0.0 else None for i in range(L)]

    def train_on_any_input(self, flag=True):
        """Opt in (per module, default off, not part of the state dict) to recording a backward for every input the frozen path
        takes: still images [B,C,H,W], whose backward sums the gradient over the temporal slices (vj_slice_sum) and takes the
        patch embedding's gradients from the B*gh*gw distinct rows, and clips of another size than the model's, whose interpolated
        position table is a constant.  Off, such inputs raise while gradients are enabled, as they always have.  The image model
        (num_frames=1) keeps raising either way."""
        self.any_input_trains = bool(flag)
        return self

    def set_activation_recompute(self, mode):
        """Opt in (per module, default off, not part of the state dict) to recomputing block activations in the backward of every
        forward that records one -- native clips, masks and, with train_on_any_input, still images and off-native clips -- instead of
        keeping them: "block" keeps each block's input alone and runs the block's forward again directly before its backward, "mlp"
        keeps all but the two [M, 4D] tensors of the MLP and refills them with one fc1 GEMM; None or "none" is off.  Outputs and
        gradients are the same bits in every mode (the forward kernels are run-to-run deterministic); what changes is the memory held
        between the forward and the backward, and the time of the backward.  The frozen / no-grad path keeps nothing and ignores it."""
        self.activation_recompute = recompute_mode(mode, "set_activation_recompute: mode")
        return self

    def no_weight_decay(self):
        return {}

    def _apply(self, fn, *args, **kwargs):
        self.__dict__.pop("_pos_interp_cache", None)    # .to() / .cuda() / .float(): interpolated tables follow pos_embed
        return super()._apply(fn, *args, **kwargs)

    def _describe(self, x, frames=False):
        """What kind of input x is, asked once per call (_Input): the (T, H, W) of the clip it stands for -- a video encoder's 4-D
        [B,C,H,W] still image is its repetition over num_frames frames, an image or a frame of the image model its own one-frame
        clip -- and whether that is the model's native size.  frames: x is the validated clip list of forward_frames."""
        if frames:
            T, H, W, still = 1, x[0].shape[3], x[0].shape[4], False
        elif not self.is_video:
            if x.dim() != 4:
                raise ValueError(f"the image model (num_frames=1) takes images [B,C,H,W], got {tuple(x.shape)}; frames of a clip "
                                 "go through FrameAggregation")
            T, H, W, still = 1, x.shape[2], x.shape[3], False
        elif x.dim() == 4:
            T, H, W, still = self.num_frames, x.shape[2], x.shape[3], True
        elif x.dim() == 5:
            T, H, W, still = x.shape[2], x.shape[3], x.shape[4], False
        else:
            raise ValueError(f"expected clips [B,C,T,H,W] or still images [B,C,H,W], got {tuple(x.shape)}")
        return _Input(T, H, W, still=still, native=(T, H, W) == (self.num_frames, self.input_size, self.input_size),
                      drops=self.is_video)

    def interpolate_pos_encoding(self, x, pos_embed):
        """The position table of x's token grid (reference: vision_transformer.py:197-228): the parameter itself at the native
        size, otherwise its trilinear interpolation [1, T'*H'*W', D] in fp32 (vj_pos_interp3d), computed once per (T, H, W) and
        kept until pos_embed is reloaded or moved.  Image model (vision_transformer.py:230-246): bicubic interpolation by
        scale_factor = sqrt(npatch / N) to the square grid of x (vj_pos_interp2d_bicubic)."""
        return self._interpolate(self._describe(x), pos_embed)

    def _interpolate(self, inp, pos_embed):
        if inp.native:
            return pos_embed
        if not self.is_video:
            return self._interpolate_image(inp.H, inp.W, pos_embed)
        T, H, W = inp.T, inp.H, inp.W
        if T % self.tubelet_size or H % self.patch_size or W % self.patch_size or min(T, H, W) <= 0:
            raise ValueError(f"input of {T}x{H}x{W} is not divisible into tubelets of {self.tubelet_size}x{self.patch_size}x"
                             f"{self.patch_size}")
        hipmodule.require_gpu(pos_embed, "VisionTransformer.interpolate_pos_encoding")
        grid = (T // self.tubelet_size, H // self.patch_size, W // self.patch_size)
        cache = self._interp_cache(pos_embed)
        table = cache.get(grid)
        if table is None:
            from ...hip import ops
            N_t = self.num_frames // self.tubelet_size
            N_h = N_w = self.input_size // self.patch_size
            dim = pos_embed.shape[-1]
            assert N_h * N_w * N_t == pos_embed.shape[1], 'Positional embedding initialized incorrectly'
            scale_factor = (grid[0] / N_t, grid[1] / N_h, grid[2] / N_w)
            src = pos_embed.detach().to(torch.float32).contiguous().view(N_t, N_h, N_w, dim)
            out = ops.pos_interp3d(src, scale_factor)
            if tuple(out.shape[:3]) != grid:
                raise ValueError(f"interpolated position table has grid {tuple(out.shape[:3])}, the input has {grid}")
            table = cache[grid] = out.view(1, -1, dim)
        return table

    def _interp_cache(self, pos_embed):
        stamp = (pos_embed.data_ptr(), pos_embed._version, pos_embed.device)
        cache = self.__dict__.setdefault("_pos_interp_cache", {})
        if cache.get("stamp") != stamp:     # load_state_dict bumps the version, .to() moves the storage
            cache.clear()
            cache["stamp"] = stamp
        return cache

    def _interpolate_image(self, H, W, pos_embed):
        p = self.patch_size
        if H % p or W % p or min(H, W) <= 0:
            raise ValueError(f"input of {H}x{W} is not divisible into patches of {p}x{p}")
        N, dim = pos_embed.shape[1], pos_embed.shape[-1]
        side_in = int(math.sqrt(N))
        npatch = (H // p) * (W // p)
        scale_factor = math.sqrt(npatch / N)                       # as the reference computes it
        side = int(math.floor(float(side_in) * scale_factor))      # F.interpolate's output extent for a given scale factor
        if side * side != npatch or H // p != W // p:
            # the reference adds its side x side table to the H/p x W/p tokens and fails there (or, when the counts happen to agree,
            # adds rows of another grid)
            raise ValueError(f"the interpolated position table is a square {side}x{side} grid, the input has {H // p}x{W // p} patches")
        hipmodule.require_gpu(pos_embed, "VisionTransformer.interpolate_pos_encoding")
        cache = self._interp_cache(pos_embed)
        table = cache.get((H, W))
        if table is None:
            from ...hip import ops
            src = pos_embed.detach().to(torch.float32).contiguous().view(side_in, side_in, dim)
            table = cache[(H, W)] = ops.pos_interp2d_bicubic(src, scale_factor).view(1, -1, dim)
        return table

    # ---- compute ------------------------------------------------------------------------------------------
    def _hip_views(self, train):
        from ...engine.weights import encoder_views
        arena, prefix = self._hip_arena(train)
        cache = self.__dict__.setdefault("_hip_view_cache", {})
        key = (id(arena), prefix, bool(train), len(arena.wT))
        v = cache.get(key)
        if v is None:   # the views (and the C descriptor array hanging off them) only change with the arena
            cache.clear()
            v = cache[key] = encoder_views(arena, prefix, self,
                                           arena.frozen[prefix + "pos_embed"].reshape(self.num_patches, -1), train)
        return v

    def forward_masks(self, x, masks):
        """All masks through one fused chain; returns a list with one [B, K_i, D] tensor per mask."""
        out, segs = self._run(x, masks, self._describe(x))
        B = x.shape[0]
        return [out[s.row0:s.row0 + s.rows].view(B, s.S, self.embed_dim) for s in segs]

    def _needs_grad(self):
        return torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())

    def _frozen_only(self, what, then=""):
        """Refuse `what` while a backward would be recorded: it is a feature of the frozen / no-grad path."""
        if self._needs_grad():
            raise NotImplementedError(f"{what} on the frozen / no-grad path only (torch.no_grad() or parameters with "
                                      f"requires_grad=False){then}")

    def _pos_table(self, inp):
        """None at the native size (the arena's table is used), otherwise the fp32 [N', D] table of the input's token grid.  The
        image model, and a video encoder's still images and off-native sizes, are frozen-path features: with gradients enabled
        the image model raises, and the video encoder does unless the module opted in (train_on_any_input)."""
        if not self.is_video:
            self._frozen_only("the image (num_frames=1) encoder runs")
        elif not self.any_input_trains and (inp.still or not inp.native):
            self._frozen_only("still-image [B,C,H,W] and off-native-size inputs run", "; with gradients enabled the encoder runs "
                              "at its native clip size, as the pretraining step does")
        pos = self._interpolate(inp, self.pos_embed)
        return None if pos is self.pos_embed else pos.view(-1, self.embed_dim)

    def forward_frames(self, x):
        """Image model only: fp32 clips [B,3,T,H,W] -> [B, T*N, D], every frame encoded on its own (what FrameAggregation's
        x.permute(0,2,1,3,4).reshape(B*T,C,H,W) feeds the model, utils.py:62-66, without that copy: vj_tubelet_pack with tubelet 1
        emits the patch rows of the clip in (b,t,h,w) order, which is frame-major, and the trunk runs on B*T sequences).  A list of
        clips of one frame size goes through ONE trunk call and comes back as a list of views of its output."""
        if self.is_video:
            raise ValueError("forward_frames belongs to the image (num_frames=1) model")
        parts = list(x) if isinstance(x, (list, tuple)) else [x]
        for c in parts:
            if c.dim() != 5 or c.shape[1:2] + c.shape[3:] != parts[0].shape[1:2] + parts[0].shape[3:]:    # the one shape check of the frames route
                raise ValueError(f"forward_frames expects clips [B,C,T,H,W] of one frame size, got {[tuple(q.shape) for q in parts]}")
        out, segs = self._run(parts if len(parts) > 1 else parts[0], None, self._describe(parts, frames=True))
        N, views, r = segs[0].S, [], 0
        for c in parts:
            rows = c.shape[0] * c.shape[2] * N
            views.append(out[r:r + rows].view(c.shape[0], c.shape[2] * N, self.embed_dim))
            r += rows
        return views if isinstance(x, (list, tuple)) else views[0]

    def forward(self, x, masks=None):
        """x: fp32 clips [B,3,T,H,W] on the GPU, or still images [B,3,H,W] standing for the clip of num_frames repetitions
        (the forward pre-hook of evals/image_classification_frozen/eval.py:452-455); masks: None, an index tensor, or a list
        of [B,K] index tensors addressing the input's token grid.  The image model (num_frames=1) takes fp32 images [B,3,H,W]."""
        if masks is not None and not isinstance(masks, list):
            masks = [masks]
        if masks is not None:
            return torch.cat(self.forward_masks(x, masks), dim=0)
        out, segs = self._run(x, None, self._describe(x))
        return out.view(x.shape[0], segs[0].S, self.embed_dim)

    def _run(self, x, masks, inp):
        pos = self._pos_table(inp)
        self.__dict__["last_drop_path_scales"] = None
        if isinstance(x, list):     # frames of the image model, clip by clip (forward_frames)
            for c in x:
                hipmodule.require_gpu(c, "VisionTransformer.forward_frames")
            x = [c.contiguous().float() for c in x]
        else:
            hipmodule.require_gpu(x, "VisionTransformer.forward")
            x = x.contiguous().float()
        if masks is not None:
            masks = [m.contiguous() for m in masks]
        if self._needs_grad():
            return hipmodule.run_with_autograd(self, _enc_fwd, _enc_bwd, (x, masks, self._drop_path_entries(x, inp), pos,
                                                                             self.activation_recompute))
        # inference: one C call per trunk (no saved activations, a private workspace) and, because nothing else shares the
        # GPU with this stream, the two-workgroups-per-CU GEMM (gemm4w.hip; see DESIGN.md section 6 for why training does not)
        ew = self._hip_views(train=False)
        # (ViT-L B=24 forward: 728.7 -> 761.1 clips/s; ViT-H, whose 1280 = 5 x 256 columns tile the big kernel exactly: 405.6 vs
        # 395.9, so the wide models keep the automatic selection -- tools/infer_bench.py)
        flags = INFER_GEMM_FLAGS if self.embed_dim <= 1024 else 0
        tag = f"infer{id(self)}:"
        if "_hip_ws_finalizer" not in self.__dict__:   # the workspace dies with the module
            self.__dict__["_hip_ws_finalizer"] = weakref.finalize(self, Workspace.release, tag)
        out, segs, _ = encoder_forward(ew, x, masks, save=False, ws_tag=tag, gemm_flags=flags, pos=pos)
        return out, segs


INFER_GEMM_FLAGS = 0x100


def _enc_fwd(module, ew, args, diff):
    x, masks, drop, pos, recompute = args     # pos: None (the arena's table) or the interpolated table of x's grid, a constant
    out, segs, saved = encoder_forward(ew, x, masks, save=True, drop=drop, pos=pos, recompute=recompute)
    return out, segs, (saved, segs)


def _enc_bwd(module, ew, ctx_saved, dout):
    saved, segs = ctx_saved
    reducer = module.grad_reducer
    if reducer is None:
        encoder_backward(dout, saved, ew, segs, alpha=1.0)
        return None
    # data parallel (engine.finetune.EncoderFineTuner on several ranks): a block's bucket of the gradient arena goes out as soon as
    # its backward is enqueued, waiting on the side stream the weight gradients run on; finish() reduces the small tensors and makes
    # this stream wait for every collective -- the pretraining step's walk (engine/step.py)
    side = side_stream(dout.device)
    reducer.begin(side.stream if side.enabled else None)
    encoder_backward(dout, saved, ew, segs, alpha=1.0, on_layer_done=reducer.layer_done)
    reducer.finish()
    return None


# name -> (embed_dim, depth, num_heads, mlp_ratio, default patch_size): the one table of the factories and of VIT_EMBED_DIMS
VIT_SIZES = {
    'vit_tiny': (192, 12, 3, 4, 16),
    'vit_small': (384, 12, 6, 4, 16),
    'vit_base': (768, 12, 12, 4, 16),
    'vit_large': (1024, 24, 16, 4, 16),
    'vit_huge': (1280, 32, 16, 4, 16),
    'vit_giant': (1408, 40, 16, 48 / 11, 16),
    # the reference passes a misspelt `mpl_ratio` here (vision_transformer.py:293), so its effective mlp_ratio is
    # the default 4.0; kept for checkpoint compatibility
    'vit_gigantic': (1664, 48, 16, 4.0, 14),
}


def _factory(name):
    embed_dim, depth, num_heads, mlp_ratio, patch = VIT_SIZES[name]

    def make(patch_size=patch, drop_path_rate=0.0, **kwargs):
        return VisionTransformer(patch_size=patch_size, embed_dim=embed_dim, depth=depth, num_heads=num_heads, mlp_ratio=mlp_ratio,
                                 qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), drop_path_rate=drop_path_rate, **kwargs)
    make.__name__ = make.__qualname__ = name
    return make


# module-level functions: the evals look them up by name (vit.__dict__[model_name])
vit_tiny = _factory('vit_tiny')
vit_small = _factory('vit_small')
vit_base = _factory('vit_base')
vit_large = _factory('vit_large')
vit_huge = _factory('vit_huge')
vit_giant = _factory('vit_giant')
vit_gigantic = _factory('vit_gigantic')

VIT_EMBED_DIMS = {name: size[0] for name, size in VIT_SIZES.items()}
