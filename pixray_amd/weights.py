"""Model configurations and parameter containers for the two frozen networks on the hot path.

No checkpoints exist offline (SURVEY.md §7 "No weights, no network"), so `synthetic_*` build
seeded random parameters with the REAL architectures' shapes (FLOPs and bytes identical to the
reference's `imagenet_f16_16384` VQGAN, vqgan.py:86, and OpenAI CLIP ViT-B/32).  Parameter names
and orders are the upstream state-dict ones, so a real checkpoint's state dict drops in
(`decoder.*` / `post_quant_conv.*` / `quantize.embedding.weight`; `visual.*`).
"""
from __future__ import annotations

import math
from collections import OrderedDict
from dataclasses import dataclass
from typing import Tuple

import torch


# --------------------------------------------------------------------------- VQGAN (taming) config
@dataclass
class VqganConfig:
    ch: int = 128
    ch_mult: Tuple[int, ...] = (1, 1, 2, 2, 4)
    num_res_blocks: int = 2
    attn_resolutions: Tuple[int, ...] = (16,)
    resolution: int = 256
    z_channels: int = 256
    embed_dim: int = 256
    n_embed: int = 16384
    out_ch: int = 3

    @property
    def num_resolutions(self) -> int:  # DrawingInterface.get_num_resolutions (vqgan.py:187-188)
        return len(self.ch_mult)

    def oracle_cfg(self) -> dict:
        return dict(ch=self.ch, ch_mult=self.ch_mult, num_res_blocks=self.num_res_blocks,
                    attn_resolutions=self.attn_resolutions, resolution=self.resolution,
                    z_channels=self.z_channels, out_ch=self.out_ch)


VQGAN_CONFIGS = {
    "imagenet_f16_16384": VqganConfig(),
    # reduced graph with the same operator mix, for fast parity tests
    "tiny_f4": VqganConfig(ch=128, ch_mult=(1, 2, 2), num_res_blocks=1, attn_resolutions=(16,), resolution=64,
                           z_channels=128, embed_dim=128, n_embed=512),
}


def vqgan_param_shapes(cfg: VqganConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """Ordered (name -> shape) list in the order the C ABI expects (include/prx.h, prx_vqgan_create)."""
    sh: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()

    def conv(name, cout, cin, k):
        sh[name + ".weight"] = (cout, cin, k, k)
        sh[name + ".bias"] = (cout,)

    def norm(name, c):
        sh[name + ".weight"] = (c,)
        sh[name + ".bias"] = (c,)

    def res(name, cin, cout):
        norm(name + ".norm1", cin); conv(name + ".conv1", cout, cin, 3)
        norm(name + ".norm2", cout); conv(name + ".conv2", cout, cout, 3)
        if cin != cout:
            conv(name + ".nin_shortcut", cout, cin, 1)

    def attn(name, c):
        norm(name + ".norm", c)
        for t in ("q", "k", "v", "proj_out"):
            conv(name + "." + t, c, c, 1)

    sh["quantize.embedding.weight"] = (cfg.n_embed, cfg.embed_dim)
    conv("post_quant_conv", cfg.z_channels, cfg.embed_dim, 1)
    nres = len(cfg.ch_mult)
    block_in = cfg.ch * cfg.ch_mult[-1]
    curr_res = cfg.resolution // 2 ** (nres - 1)
    conv("decoder.conv_in", block_in, cfg.z_channels, 3)
    res("decoder.mid.block_1", block_in, block_in)
    attn("decoder.mid.attn_1", block_in)
    res("decoder.mid.block_2", block_in, block_in)
    for lvl in reversed(range(nres)):
        block_out = cfg.ch * cfg.ch_mult[lvl]
        for b in range(cfg.num_res_blocks + 1):
            res(f"decoder.up.{lvl}.block.{b}", block_in, block_out)
            block_in = block_out
            if curr_res in cfg.attn_resolutions:
                attn(f"decoder.up.{lvl}.attn.{b}", block_in)
        if lvl != 0:
            conv(f"decoder.up.{lvl}.upsample.conv", block_in, block_in, 3)
            curr_res *= 2
    norm("decoder.norm_out", block_in)
    conv("decoder.conv_out", cfg.out_ch, block_in, 3)
    return sh


def vqgan_encoder_param_shapes(cfg: VqganConfig, in_channels: int = 3) -> "OrderedDict[str, Tuple[int, ...]]":
    """Ordered (name -> shape) list of taming's Encoder + quant_conv (+ the codebook), in the order the C ABI expects
    (include/prx.h, prx_vqgan_enc_create).  Names are the taming state-dict keys (`encoder.*`, `quant_conv.*`)."""
    sh: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()

    def conv(name, cout, cin, k):
        sh[name + ".weight"] = (cout, cin, k, k)
        sh[name + ".bias"] = (cout,)

    def norm(name, c):
        sh[name + ".weight"] = (c,)
        sh[name + ".bias"] = (c,)

    def res(name, cin, cout):
        norm(name + ".norm1", cin); conv(name + ".conv1", cout, cin, 3)
        norm(name + ".norm2", cout); conv(name + ".conv2", cout, cout, 3)
        if cin != cout:
            conv(name + ".nin_shortcut", cout, cin, 1)

    def attn(name, c):
        norm(name + ".norm", c)
        for t in ("q", "k", "v", "proj_out"):
            conv(name + "." + t, c, c, 1)

    sh["quantize.embedding.weight"] = (cfg.n_embed, cfg.embed_dim)
    conv("encoder.conv_in", cfg.ch, in_channels, 3)
    nres = len(cfg.ch_mult)
    block_in = cfg.ch
    curr_res = cfg.resolution
    for lvl in range(nres):
        block_out = cfg.ch * cfg.ch_mult[lvl]
        for b in range(cfg.num_res_blocks):
            res(f"encoder.down.{lvl}.block.{b}", block_in, block_out)
            block_in = block_out
            if curr_res in cfg.attn_resolutions:
                attn(f"encoder.down.{lvl}.attn.{b}", block_in)
        if lvl != nres - 1:
            conv(f"encoder.down.{lvl}.downsample.conv", block_in, block_in, 3)
            curr_res //= 2
    res("encoder.mid.block_1", block_in, block_in)
    attn("encoder.mid.attn_1", block_in)
    res("encoder.mid.block_2", block_in, block_in)
    norm("encoder.norm_out", block_in)
    conv("encoder.conv_out", cfg.z_channels, block_in, 3)
    conv("quant_conv", cfg.embed_dim, cfg.z_channels, 1)
    return sh


def _init_conv_like(name, shape, g):
    if name == "quantize.embedding.weight":
        return torch.randn(shape, generator=g)
    if name.endswith(".weight") and len(shape) == 1:      # GroupNorm gamma
        return 1.0 + 0.1 * torch.randn(shape, generator=g)
    if name.endswith(".bias") and (".norm" in name or "norm_out" in name):
        return 0.05 * torch.randn(shape, generator=g)
    if name.endswith(".bias"):
        return 0.02 * torch.randn(shape, generator=g)
    fan_in = shape[1] * shape[2] * shape[3]
    gain = 1.0
    if name.endswith("conv2.weight") or name.endswith("proj_out.weight"):
        gain = 0.5       # residual branches: keep the stream O(1) through 20 blocks
    if name.endswith("conv_out.weight"):
        gain = 0.7
    return torch.randn(shape, generator=g) * (gain / math.sqrt(fan_in))


def synthetic_vqgan_encoder_params(cfg: VqganConfig, seed: int = 0, codebook: torch.Tensor = None,
                                   in_channels: int = 3) -> "OrderedDict[str, torch.Tensor]":
    """Seeded random Encoder/quant_conv weights.  `codebook`: reuse the decoder's `quantize.embedding.weight` (a taming
    checkpoint has ONE codebook shared by encode and decode)."""
    g = torch.Generator().manual_seed(seed + 7919)
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape in vqgan_encoder_param_shapes(cfg, in_channels).items():
        if name == "quantize.embedding.weight" and codebook is not None:
            out[name] = codebook
            continue
        out[name] = _init_conv_like(name, shape, g)
    return out


def synthetic_vqgan_params(cfg: VqganConfig, seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    g = torch.Generator().manual_seed(seed)
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape in vqgan_param_shapes(cfg).items():
        if name == "quantize.embedding.weight":
            t = torch.randn(shape, generator=g)
        elif name.endswith(".weight") and len(shape) == 1:      # GroupNorm gamma
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif name.endswith(".bias") and (".norm" in name or "norm_out" in name):
            t = 0.05 * torch.randn(shape, generator=g)
        elif name.endswith(".bias"):
            t = 0.02 * torch.randn(shape, generator=g)
        else:
            fan_in = shape[1] * shape[2] * shape[3]
            gain = 1.0
            if name.endswith("conv2.weight") or name.endswith("proj_out.weight"):
                gain = 0.5       # residual branches: keep the stream O(1) through 20 blocks
            if name.endswith("conv_out.weight"):
                gain = 0.7
            t = torch.randn(shape, generator=g) * (gain / math.sqrt(fan_in))
        out[name] = t
    return out


# --------------------------------------------------------------------------- CLIP ViT config
@dataclass
class ClipVitConfig:
    name: str = "ViT-B/32"
    input_resolution: int = 224
    patch_size: int = 32
    width: int = 768
    layers: int = 12
    heads: int = 12
    output_dim: int = 512

    @property
    def tokens(self) -> int:
        return (self.input_resolution // self.patch_size) ** 2 + 1


CLIP_CONFIGS = {
    "ViT-B/32": ClipVitConfig(),
    "ViT-B/16": ClipVitConfig("ViT-B/16", 224, 16, 768, 12, 12, 512),
    "ViT-L/14": ClipVitConfig("ViT-L/14", 224, 14, 1024, 24, 16, 768),
    "ViT-L/14@336px": ClipVitConfig("ViT-L/14@336px", 336, 14, 1024, 24, 16, 768),       # 577 tokens
    # reduced tower (same operators, 2 layers) for fast parity tests
    "tiny-B/32": ClipVitConfig("tiny-B/32", 224, 32, 256, 2, 4, 128),
}


def clip_vit_param_shapes(cfg: ClipVitConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    w = cfg.width
    m = getattr(cfg, "mlp", 4 * w)          # hidden width of the MLP: 4 x width everywhere but OpenCLIP's ViT-g-14 / ViT-bigG-14
    sh: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    sh["conv1.weight"] = (w, 3, cfg.patch_size, cfg.patch_size)
    sh["class_embedding"] = (w,)
    sh["positional_embedding"] = (cfg.tokens, w)
    sh["ln_pre.weight"] = (w,); sh["ln_pre.bias"] = (w,)
    for i in range(cfg.layers):
        p = f"transformer.resblocks.{i}."
        sh[p + "ln_1.weight"] = (w,); sh[p + "ln_1.bias"] = (w,)
        sh[p + "attn.in_proj_weight"] = (3 * w, w); sh[p + "attn.in_proj_bias"] = (3 * w,)
        sh[p + "attn.out_proj.weight"] = (w, w); sh[p + "attn.out_proj.bias"] = (w,)
        sh[p + "ln_2.weight"] = (w,); sh[p + "ln_2.bias"] = (w,)
        sh[p + "mlp.c_fc.weight"] = (m, w); sh[p + "mlp.c_fc.bias"] = (m,)
        sh[p + "mlp.c_proj.weight"] = (w, m); sh[p + "mlp.c_proj.bias"] = (w,)
    sh["ln_post.weight"] = (w,); sh["ln_post.bias"] = (w,)
    sh["proj"] = (w, cfg.output_dim)
    return sh


def synthetic_clip_vit_params(cfg: ClipVitConfig, seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """OpenAI's initialisation scheme (clip/model.py CLIP.initialize_parameters) with seeded draws."""
    g = torch.Generator().manual_seed(seed)
    w = cfg.width
    proj_std = (w ** -0.5) * ((2 * cfg.layers) ** -0.5)
    attn_std = w ** -0.5
    fc_std = (2 * w) ** -0.5
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape in clip_vit_param_shapes(cfg).items():
        if name == "conv1.weight":
            t = torch.randn(shape, generator=g) / math.sqrt(3 * cfg.patch_size ** 2)
        elif name in ("class_embedding", "positional_embedding", "proj"):
            t = torch.randn(shape, generator=g) * (w ** -0.5)
        elif name.endswith("in_proj_weight"):
            t = torch.randn(shape, generator=g) * attn_std
        elif name.endswith("out_proj.weight") or name.endswith("c_proj.weight"):
            t = torch.randn(shape, generator=g) * proj_std
        elif name.endswith("c_fc.weight"):
            t = torch.randn(shape, generator=g) * fc_std
        elif name.endswith(".weight"):       # LayerNorm gamma
            t = 1.0 + 0.05 * torch.randn(shape, generator=g)
        else:                                # biases / LayerNorm beta
            t = 0.02 * torch.randn(shape, generator=g)
        out[name] = t
    return out


# --------------------------------------------------------------------------- OpenCLIP (LAION) ViT towers
# [UPSTREAM mlfoundations/open_clip src/open_clip/model_configs/{ViT-B-32,ViT-B-16,ViT-L-14,ViT-H-14,ViT-g-14,ViT-bigG-14}.json; the package is not
# installed, so the geometry is restated from the published configs, parity unpinned].  OpenCLIP spells its names with hyphens, which
# keeps them apart from OpenAI's towers of the same geometry.  Against those: the exact (erf) GELU instead of QuickGELU (the LAION
# checkpoints are trained without "quick_gelu"), on both the image and the text side; same tensors, same state-dict names, CLIP's
# preprocessing constants.  ViT-H-14 has 16 heads of 80 on width 1280: the runner pads them to 96 columns (csrc/attention.hip, the 96-wide instances).
# ViT-g-14 (width 1408 = 11 x 128, 16 heads of 88, MLP 6144) and ViT-bigG-14 (width 1664 = 13 x 128, 16 heads of 104, MLP 8192) are the
# two whose MLP is not 4 x width (mlp_ratio 4.3637 / 4.9231 in the configs): the hidden width is carried here.  Their widths run on
# the ragged LayerNorm instances (csrc/norms.hip, MAXV = 8); heads of 88 are padded to 96 columns, heads of 104 to 128 (the 128-wide
# instances of the same attention family).
@dataclass
class OpenClipVitConfig(ClipVitConfig):
    mlp_width: int = 0              # hidden width of the MLP; 0 = 4 x width

    @property
    def head_dim(self) -> int:
        return self.width // self.heads

    @property
    def mlp(self) -> int:
        return self.mlp_width or 4 * self.width


OPENCLIP_CONFIGS = {
    "ViT-B-32": OpenClipVitConfig("ViT-B-32", 224, 32, 768, 12, 12, 512),
    "ViT-B-16": OpenClipVitConfig("ViT-B-16", 224, 16, 768, 12, 12, 512),
    "ViT-L-14": OpenClipVitConfig("ViT-L-14", 224, 14, 1024, 24, 16, 768),
    "ViT-H-14": OpenClipVitConfig("ViT-H-14", 224, 14, 1280, 32, 16, 1024),            # 257 tokens, MLP 5120, heads of 80
    # reduced towers with heads of 80 (same operators, 2 layers; 640 is the smallest width that is a multiple of 80 and of 128)
    "tiny-H-32": OpenClipVitConfig("tiny-H-32", 224, 32, 640, 2, 8, 128),              # 50 tokens
    "tiny-H-14": OpenClipVitConfig("tiny-H-14", 224, 14, 640, 2, 8, 128),              # 257 tokens
    "ViT-g-14": OpenClipVitConfig("ViT-g-14", 224, 14, 1408, 40, 16, 1024, mlp_width=6144),        # 257 tokens, heads of 88
    "ViT-bigG-14": OpenClipVitConfig("ViT-bigG-14", 224, 14, 1664, 48, 16, 1280, mlp_width=8192),  # 257 tokens, heads of 104
    # reduced towers with heads of 88 / 104: lcm(88, 128) = 1408 and lcm(104, 128) = 1664, so the real width is the smallest width that
    # has these heads -- the depth is what is reduced (2 layers, the real MLP width)
    "tiny-g-32": OpenClipVitConfig("tiny-g-32", 224, 32, 1408, 2, 16, 128, mlp_width=6144),        # 50 tokens
    "tiny-g-14": OpenClipVitConfig("tiny-g-14", 224, 14, 1408, 2, 16, 128, mlp_width=6144),        # 257 tokens
    "tiny-bigG-32": OpenClipVitConfig("tiny-bigG-32", 224, 32, 1664, 2, 16, 128, mlp_width=8192),  # 50 tokens
    "tiny-bigG-14": OpenClipVitConfig("tiny-bigG-14", 224, 14, 1664, 2, 16, 128, mlp_width=8192),  # 257 tokens
}
OPENCLIP_SEED = 7919            # the synthetic weights of `ViT-B-32` are not those of `ViT-B/32`


# --------------------------------------------------------------------------- SLIP image towers (timm VisionTransformer)
# [UPSTREAM facebookresearch/SLIP models.py + timm vision_transformer.py; the SLIP/ submodule of the reference checkout is empty, so
# this is restated from the published sources, parity unpinned]: `timm.create_model(vit_*_patch16_224, num_classes=0)` followed by
# `@ image_projection`.  Against the CLIP tower: a patch-embed bias, no ln_pre, LayerNorm eps 1e-6, exact GELU, ImageNet Normalize.
@dataclass
class SlipVitConfig:
    name: str = "SLIP_VITB16"
    input_resolution: int = 224
    patch_size: int = 16
    width: int = 768
    layers: int = 12
    heads: int = 12
    output_dim: int = 512
    ln_eps: float = 1e-6
    seed_offset: int = 0            # the names that share a configuration keep their own synthetic weights
    checkpoint: str = ""            # file name under models/ (slip.py:90-107)

    @property
    def tokens(self) -> int:
        return (self.input_resolution // self.patch_size) ** 2 + 1

    @property
    def head_dim(self) -> int:
        return self.width // self.heads


IMAGENET_MEAN = (0.485, 0.456, 0.406)       # slip.py:120
IMAGENET_STD = (0.229, 0.224, 0.225)

SLIP_CONFIGS = {
    "SLIP_VITB16": SlipVitConfig("SLIP_VITB16", seed_offset=0, checkpoint="slip_base_100ep.pt"),
    # the same model on other training data (slip.py:133-135)
    "SLIP_CC3M": SlipVitConfig("SLIP_CC3M", seed_offset=1, checkpoint="slip_base_cc3m_40ep.pt"),
    "SLIP_CC12M": SlipVitConfig("SLIP_CC12M", seed_offset=2, checkpoint="slip_base_cc12m_35ep.pt"),
    "CLIP_VITB16": SlipVitConfig("CLIP_VITB16", seed_offset=3, checkpoint="clip_base_25ep.pt"),
    "SLIP_VITL16": SlipVitConfig("SLIP_VITL16", width=1024, layers=24, heads=16, seed_offset=4, checkpoint="slip_large_100ep.pt"),
    "CLIP_VITL16": SlipVitConfig("CLIP_VITL16", width=1024, layers=24, heads=16, seed_offset=5, checkpoint="clip_large_25ep.pt"),
    # SLIP's vit_small_mocov3_patch16_224: 12 heads of 32 on width 384; the runner pads the heads to 64 when it packs the weights
    "SLIP_VITS16": SlipVitConfig("SLIP_VITS16", width=384, layers=12, heads=12, seed_offset=6, checkpoint="slip_small_100ep.pt"),
    "CLIP_VITS16": SlipVitConfig("CLIP_VITS16", width=384, layers=12, heads=12, seed_offset=7, checkpoint="clip_small_25ep.pt"),
    # reduced 197-token tower (same operators, 2 layers) for fast parity tests
    "tiny-SLIP/16": SlipVitConfig("tiny-SLIP/16", width=256, layers=2, heads=4, output_dim=128, seed_offset=8),
    "tiny-SLIP32/16": SlipVitConfig("tiny-SLIP32/16", width=128, layers=2, heads=4, output_dim=128, seed_offset=9),    # heads of 32
}
SLIP_REFUSED = {"SIMCLR_VITS16": "SIMCLR_VITS16 has no text side (a SimCLR image encoder only): it cannot score prompts and is not provided"}


def slip_vit_param_shapes(cfg: SlipVitConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """timm state-dict names of the image side (`visual.` stripped) + SLIP's `image_projection`, in the order the C ABI expects
    (include/prx.h, prx_vit_tower_create)."""
    w = cfg.width
    sh: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    sh["patch_embed.proj.weight"] = (w, 3, cfg.patch_size, cfg.patch_size)
    sh["patch_embed.proj.bias"] = (w,)
    sh["cls_token"] = (1, 1, w)
    sh["pos_embed"] = (1, cfg.tokens, w)
    for i in range(cfg.layers):
        p = f"blocks.{i}."
        sh[p + "norm1.weight"] = (w,); sh[p + "norm1.bias"] = (w,)
        sh[p + "attn.qkv.weight"] = (3 * w, w); sh[p + "attn.qkv.bias"] = (3 * w,)
        sh[p + "attn.proj.weight"] = (w, w); sh[p + "attn.proj.bias"] = (w,)
        sh[p + "norm2.weight"] = (w,); sh[p + "norm2.bias"] = (w,)
        sh[p + "mlp.fc1.weight"] = (4 * w, w); sh[p + "mlp.fc1.bias"] = (4 * w,)
        sh[p + "mlp.fc2.weight"] = (w, 4 * w); sh[p + "mlp.fc2.bias"] = (w,)
    sh["norm.weight"] = (w,); sh["norm.bias"] = (w,)
    sh["image_projection"] = (w, cfg.output_dim)
    return sh


def synthetic_slip_vit_params(cfg: SlipVitConfig, seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """Seeded random weights of the real architecture, scaled as `synthetic_clip_vit_params` scales the CLIP tower's (the residual
    stream stays O(1) through every block)."""
    g = torch.Generator().manual_seed(seed + 15485863 + cfg.seed_offset)
    w = cfg.width
    proj_std = (w ** -0.5) * ((2 * cfg.layers) ** -0.5)
    attn_std = w ** -0.5
    fc_std = (2 * w) ** -0.5
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape in slip_vit_param_shapes(cfg).items():
        if name == "patch_embed.proj.weight":
            t = torch.randn(shape, generator=g) / math.sqrt(3 * cfg.patch_size ** 2)
        elif name in ("cls_token", "pos_embed", "image_projection"):
            t = torch.randn(shape, generator=g) * (w ** -0.5)
        elif name.endswith("attn.qkv.weight"):
            t = torch.randn(shape, generator=g) * attn_std
        elif name.endswith("attn.proj.weight") or name.endswith("fc2.weight"):
            t = torch.randn(shape, generator=g) * proj_std
        elif name.endswith("fc1.weight"):
            t = torch.randn(shape, generator=g) * fc_std
        elif name.endswith(".weight"):       # LayerNorm gamma
            t = 1.0 + 0.05 * torch.randn(shape, generator=g)
        else:                                # biases / LayerNorm beta
            t = 0.02 * torch.randn(shape, generator=g)
        out[name] = t
    return out


# --------------------------------------------------------------------------- CLIP text tower config
@dataclass
class ClipTextConfig:
    name: str = "ViT-B/32"
    vocab_size: int = 49408
    context_length: int = 77
    width: int = 512
    layers: int = 12
    heads: int = 8
    output_dim: int = 512


@dataclass
class OpenClipTextConfig(ClipTextConfig):
    """CLIP's text transformer with the exact GELU (the OpenCLIP towers); heads are 64 wide in every published config"""
    gelu: bool = True


# text-side hyper-parameters of the OpenAI checkpoints (clip/model.py `build_model`: heads = width // 64)
CLIP_TEXT_CONFIGS = {
    "ViT-B/32": ClipTextConfig(),
    "ViT-B/16": ClipTextConfig("ViT-B/16"),
    "ViT-L/14": ClipTextConfig("ViT-L/14", width=768, heads=12, output_dim=768),
    "ViT-L/14@336px": ClipTextConfig("ViT-L/14@336px", width=768, heads=12, output_dim=768),
    "tiny-B/32": ClipTextConfig("tiny-B/32", vocab_size=1000, context_length=77, width=256, layers=2, heads=4, output_dim=128),
    "RN50x4": ClipTextConfig("RN50x4", width=640, heads=10, output_dim=640),
    "RN50": ClipTextConfig("RN50", width=512, heads=8, output_dim=1024),
    "RN101": ClipTextConfig("RN101", width=512, heads=8, output_dim=512),
    "RN50x16": ClipTextConfig("RN50x16", width=768, heads=12, output_dim=768),
    "RN50x64": ClipTextConfig("RN50x64", width=1024, heads=16, output_dim=1024),
}
CLIP_TEXT_CONFIGS.update({
    "ViT-B-32": OpenClipTextConfig("ViT-B-32"),
    "ViT-B-16": OpenClipTextConfig("ViT-B-16"),
    "ViT-L-14": OpenClipTextConfig("ViT-L-14", width=768, heads=12, output_dim=768),
    "ViT-H-14": OpenClipTextConfig("ViT-H-14", width=1024, layers=24, heads=16, output_dim=1024),
    "tiny-H-32": OpenClipTextConfig("tiny-H-32", vocab_size=1000, context_length=77, width=256, layers=2, heads=4, output_dim=128),
    "tiny-H-14": OpenClipTextConfig("tiny-H-14", vocab_size=1000, context_length=77, width=256, layers=2, heads=4, output_dim=128),
    "ViT-g-14": OpenClipTextConfig("ViT-g-14", width=1024, layers=24, heads=16, output_dim=1024),         # ViT-H-14's text geometry
    "ViT-bigG-14": OpenClipTextConfig("ViT-bigG-14", width=1280, layers=32, heads=20, output_dim=1280),   # MLP 5120 = 4 x width
})
for _n in ("tiny-g-32", "tiny-g-14", "tiny-bigG-32", "tiny-bigG-14"):
    CLIP_TEXT_CONFIGS[_n] = OpenClipTextConfig(_n, vocab_size=1000, context_length=77, width=256, layers=2, heads=4, output_dim=128)
# every SLIP model size carries CLIP's text transformer at width 512 / 8 heads / 12 layers [UPSTREAM SLIP models.py]
CLIP_TEXT_CONFIGS.update({n: ClipTextConfig(n) for n in ("SLIP_VITS16", "SLIP_VITB16", "SLIP_VITL16", "SLIP_CC3M", "SLIP_CC12M",
                                                         "CLIP_VITS16", "CLIP_VITB16", "CLIP_VITL16")})
for _n in ("tiny-SLIP/16", "tiny-SLIP32/16"):
    CLIP_TEXT_CONFIGS[_n] = ClipTextConfig(_n, vocab_size=1000, context_length=77, width=256, layers=2, heads=4, output_dim=128)


def clip_text_param_shapes(cfg: ClipTextConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """OpenAI state-dict names of the text side, in the order the C ABI expects (include/prx.h, prx_clip_text_create)."""
    w = cfg.width
    sh: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    sh["token_embedding.weight"] = (cfg.vocab_size, w)
    sh["positional_embedding"] = (cfg.context_length, w)
    for i in range(cfg.layers):
        p = f"transformer.resblocks.{i}."
        sh[p + "ln_1.weight"] = (w,); sh[p + "ln_1.bias"] = (w,)
        sh[p + "attn.in_proj_weight"] = (3 * w, w); sh[p + "attn.in_proj_bias"] = (3 * w,)
        sh[p + "attn.out_proj.weight"] = (w, w); sh[p + "attn.out_proj.bias"] = (w,)
        sh[p + "ln_2.weight"] = (w,); sh[p + "ln_2.bias"] = (w,)
        sh[p + "mlp.c_fc.weight"] = (4 * w, w); sh[p + "mlp.c_fc.bias"] = (4 * w,)
        sh[p + "mlp.c_proj.weight"] = (w, 4 * w); sh[p + "mlp.c_proj.bias"] = (w,)
    sh["ln_final.weight"] = (w,); sh["ln_final.bias"] = (w,)
    sh["text_projection"] = (w, cfg.output_dim)
    return sh


def synthetic_clip_text_params(cfg: ClipTextConfig, seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """OpenAI's initialisation scheme (clip/model.py CLIP.initialize_parameters) with seeded draws."""
    g = torch.Generator().manual_seed(seed + 104729)
    w = cfg.width
    proj_std = (w ** -0.5) * ((2 * cfg.layers) ** -0.5)
    attn_std = w ** -0.5
    fc_std = (2 * w) ** -0.5
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape in clip_text_param_shapes(cfg).items():
        if name == "token_embedding.weight":
            t = torch.randn(shape, generator=g) * 0.02
        elif name == "positional_embedding":
            t = torch.randn(shape, generator=g) * 0.01
        elif name == "text_projection":
            t = torch.randn(shape, generator=g) * (w ** -0.5)
        elif name.endswith("in_proj_weight"):
            t = torch.randn(shape, generator=g) * attn_std
        elif name.endswith("out_proj.weight") or name.endswith("c_proj.weight"):
            t = torch.randn(shape, generator=g) * proj_std
        elif name.endswith("c_fc.weight"):
            t = torch.randn(shape, generator=g) * fc_std
        elif name.endswith(".weight"):       # LayerNorm gamma
            t = 1.0 + 0.05 * torch.randn(shape, generator=g)
        else:                                # biases / LayerNorm beta
            t = 0.02 * torch.randn(shape, generator=g)
        out[name] = t
    return out


# --------------------------------------------------------------------------- CLIP ModifiedResNet config (RN50x4, RN50x16, ...)
@dataclass
class ClipResNetConfig:
    name: str = "RN50x4"
    input_resolution: int = 288
    width: int = 80
    layers: Tuple[int, ...] = (4, 6, 10, 6)
    heads: int = 40                 # width * 32 // 64
    output_dim: int = 640

    @property
    def embed_dim(self) -> int:     # channels entering the attention pool
        return self.width * 32

    @property
    def final_grid(self) -> int:
        return self.input_resolution // 32


CLIP_RESNET_CONFIGS = {
    "RN50x4": ClipResNetConfig(),
    "RN50": ClipResNetConfig("RN50", 224, 64, (3, 4, 6, 3), 32, 1024),
    "RN101": ClipResNetConfig("RN101", 224, 64, (3, 4, 23, 3), 32, 512),      # quality `supreme` names it (pixray.py:1830)
    "RN50x16": ClipResNetConfig("RN50x16", 384, 96, (6, 8, 18, 8), 48, 768),           # 145 pool tokens, embed 3072
    "RN50x64": ClipResNetConfig("RN50x64", 448, 128, (3, 15, 36, 10), 64, 1024),      # 197 pool tokens, embed 4096
    # reduced tower with the same operator mix (stem, stride-1 and stride-2 bottlenecks, attention pool)
    "tiny-RN": ClipResNetConfig("tiny-RN", 96, 16, (1, 2, 1, 1), 8, 64),
}


def clip_resnet_param_shapes(cfg: ClipResNetConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """OpenAI `visual.*` state-dict names of a ModifiedResNet (prefix stripped), in definition order."""
    sh: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    w = cfg.width

    def bn(name, c):
        for k in ("weight", "bias", "running_mean", "running_var"):
            sh[f"{name}.{k}"] = (c,)

    sh["conv1.weight"] = (w // 2, 3, 3, 3); bn("bn1", w // 2)
    sh["conv2.weight"] = (w // 2, w // 2, 3, 3); bn("bn2", w // 2)
    sh["conv3.weight"] = (w, w // 2, 3, 3); bn("bn3", w)
    inplanes = w
    for li, nblocks in enumerate(cfg.layers):
        planes = w * 2 ** li
        for b in range(nblocks):
            stride = 2 if (li > 0 and b == 0) else 1
            pre = f"layer{li + 1}.{b}"
            sh[pre + ".conv1.weight"] = (planes, inplanes, 1, 1); bn(pre + ".bn1", planes)
            sh[pre + ".conv2.weight"] = (planes, planes, 3, 3); bn(pre + ".bn2", planes)
            sh[pre + ".conv3.weight"] = (planes * 4, planes, 1, 1); bn(pre + ".bn3", planes * 4)
            if stride > 1 or inplanes != planes * 4:
                sh[pre + ".downsample.0.weight"] = (planes * 4, inplanes, 1, 1); bn(pre + ".downsample.1", planes * 4)
            inplanes = planes * 4
    C = cfg.embed_dim
    sh["attnpool.positional_embedding"] = (cfg.final_grid ** 2 + 1, C)
    for n_ in ("k_proj", "q_proj", "v_proj"):
        sh[f"attnpool.{n_}.weight"] = (C, C); sh[f"attnpool.{n_}.bias"] = (C,)
    sh["attnpool.c_proj.weight"] = (cfg.output_dim, C); sh["attnpool.c_proj.bias"] = (cfg.output_dim,)
    return sh


def synthetic_clip_resnet_params(cfg: ClipResNetConfig, seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """Seeded random weights; BatchNorm running statistics are non-trivial so that the fold is exercised."""
    g = torch.Generator().manual_seed(seed + 31337)
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape in clip_resnet_param_shapes(cfg).items():
        if name.endswith("running_mean"):
            t = 0.1 * torch.randn(shape, generator=g)
        elif name.endswith("running_var"):
            t = 0.5 + torch.rand(shape, generator=g)
        elif ".bn" in name or name.startswith("bn") or "downsample.1" in name:
            t = (1.0 + 0.1 * torch.randn(shape, generator=g)) if name.endswith("weight") else 0.05 * torch.randn(shape, generator=g)
            if name.endswith("bn3.weight") and name.startswith("layer"):
                # residual-branch gain 0.2: with 26 bottlenecks the variance of the residual stream then grows 1.04^26 = 2.8x,
                # as in a BatchNorm-trained tower.  (Round 1 used 0.5: 1.25^26 = 330x, which saturated the attention pool's
                # softmax and made the random tower ill-conditioned -- rounding its WEIGHTS to bf16 alone moved the embedding by
                # 1.7-3 % depending on the seed, against 0.4 % now.)
                t = t * 0.2
        elif name == "attnpool.positional_embedding":
            t = torch.randn(shape, generator=g) * (shape[1] ** -0.5)
        elif name.endswith(".bias"):
            t = 0.02 * torch.randn(shape, generator=g)
        elif len(shape) == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            t = torch.randn(shape, generator=g) * math.sqrt(2.0 / fan_in)
        else:
            t = torch.randn(shape, generator=g) * (shape[1] ** -0.5)
        out[name] = t
    return out


def fold_clip_resnet_params(cfg: ClipResNetConfig, p) -> "OrderedDict[str, torch.Tensor]":
    """Frozen eval-mode BatchNorm folded into the preceding bias-free conv (w' = w * gamma / sqrt(var + eps), b' = beta -
    mean * gamma / sqrt(var + eps)); q/k/v projections of the attention pool concatenated.  Order = what
    prx_clip_resnet_create expects (include/prx.h)."""
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()

    def fold(conv, bn, key):
        w = p[conv + ".weight"].double()
        s = p[bn + ".weight"].double() / torch.sqrt(p[bn + ".running_var"].double() + 1e-5)
        out[key + ".weight"] = (w * s.view(-1, 1, 1, 1)).float()
        out[key + ".bias"] = (p[bn + ".bias"].double() - p[bn + ".running_mean"].double() * s).float()

    fold("conv1", "bn1", "stem1"); fold("conv2", "bn2", "stem2"); fold("conv3", "bn3", "stem3")
    inplanes = cfg.width
    for li, nblocks in enumerate(cfg.layers):
        planes = cfg.width * 2 ** li
        for b in range(nblocks):
            stride = 2 if (li > 0 and b == 0) else 1
            pre = f"layer{li + 1}.{b}"
            fold(pre + ".conv1", pre + ".bn1", pre + ".c1")
            fold(pre + ".conv2", pre + ".bn2", pre + ".c2")
            fold(pre + ".conv3", pre + ".bn3", pre + ".c3")
            if stride > 1 or inplanes != planes * 4:
                fold(pre + ".downsample.0", pre + ".downsample.1", pre + ".ds")
            inplanes = planes * 4
    out["attnpool.positional_embedding"] = p["attnpool.positional_embedding"].float()
    out["attnpool.in_proj_weight"] = torch.cat([p[f"attnpool.{n_}.weight"] for n_ in ("q_proj", "k_proj", "v_proj")], 0).float()
    out["attnpool.in_proj_bias"] = torch.cat([p[f"attnpool.{n_}.bias"] for n_ in ("q_proj", "k_proj", "v_proj")], 0).float()
    out["attnpool.c_proj.weight"] = p["attnpool.c_proj.weight"].float()
    out["attnpool.c_proj.bias"] = p["attnpool.c_proj.bias"].float()
    return out


# --------------------------------------------------------------------------- OpenCLIP ConvNeXt towers (LAION)
# [UPSTREAM mlfoundations/open_clip src/open_clip/model_configs/convnext_*.json and timm convnext.py (convnext_base, convnext_large,
# convnext_xxlarge); neither package is installed, so the geometry is restated from the published configs and sources, parity
# unpinned].  The trunk under `visual.trunk.`: stem.0 = Conv2d(3, d0, 4, stride 4) with a bias, stem.1 = LayerNorm over the channels;
# per stage i > 0 `stages.i.downsample.0` = LayerNorm, `.1` = Conv2d(d(i-1), d(i), 2, stride 2) with a bias; per block conv_dw
# (depthwise 7x7, padding 3, bias), norm (LayerNorm), mlp.fc1 (C -> 4C), the exact GELU, mlp.fc2 (4C -> C), a multiply by gamma[C] and
# the addition of the block input; then the mean over H x W, head.norm (LayerNorm) and, under `visual.head.`, the projection:
# `linear`: proj.weight [embed, d3] without a bias; `mlp`: mlp.fc1 {weight [2 embed, d3], bias}, GELU, mlp.fc2.weight [embed, 2 embed]
# without a bias.  Every LayerNorm has eps 1e-6 except convnext_xxlarge's 1e-5; CLIP's preprocessing constants; the text side is
# CLIP's transformer with the exact GELU (OpenClipTextConfig).
@dataclass
class ClipConvNextConfig:
    name: str = "convnext_base_w"
    input_resolution: int = 256
    depths: Tuple[int, ...] = (3, 3, 27, 3)
    dims: Tuple[int, ...] = (128, 256, 512, 1024)
    output_dim: int = 640
    proj: str = "linear"            # "linear" | "mlp"
    ln_eps: float = 1e-6


CLIP_CONVNEXT_CONFIGS = {
    "convnext_base": ClipConvNextConfig("convnext_base", 224, (3, 3, 27, 3), (128, 256, 512, 1024), 512, "linear"),
    "convnext_base_w": ClipConvNextConfig("convnext_base_w", 256, (3, 3, 27, 3), (128, 256, 512, 1024), 640, "linear"),
    "convnext_base_w_320": ClipConvNextConfig("convnext_base_w_320", 320, (3, 3, 27, 3), (128, 256, 512, 1024), 640, "linear"),
    "convnext_large_d": ClipConvNextConfig("convnext_large_d", 256, (3, 3, 27, 3), (192, 384, 768, 1536), 768, "mlp"),
    "convnext_large_d_320": ClipConvNextConfig("convnext_large_d_320", 320, (3, 3, 27, 3), (192, 384, 768, 1536), 768, "mlp"),
    "convnext_xxlarge": ClipConvNextConfig("convnext_xxlarge", 256, (3, 4, 30, 3), (384, 768, 1536, 3072), 1024, "linear", 1e-5),
    # reduced towers with the same operators: maps 16 / 8 / 4 / 2 and 24 / 12 / 6 / 3 -- the last ones smaller than the 7x7 filter
    "tiny-cnx": ClipConvNextConfig("tiny-cnx", 64, (1, 1, 2, 1), (64, 128, 256, 512), 128, "linear"),
    "tiny-cnx-d": ClipConvNextConfig("tiny-cnx-d", 96, (1, 1, 1, 1), (96, 192, 384, 768), 128, "mlp"),
}
CLIP_TEXT_CONFIGS.update({
    "convnext_base": OpenClipTextConfig("convnext_base"),
    "convnext_base_w": OpenClipTextConfig("convnext_base_w", width=640, heads=10, output_dim=640),
    "convnext_base_w_320": OpenClipTextConfig("convnext_base_w_320", width=640, heads=10, output_dim=640),
    "convnext_large_d": OpenClipTextConfig("convnext_large_d", width=768, layers=16, heads=12, output_dim=768),
    "convnext_large_d_320": OpenClipTextConfig("convnext_large_d_320", width=768, layers=16, heads=12, output_dim=768),
    "convnext_xxlarge": OpenClipTextConfig("convnext_xxlarge", width=1024, layers=24, heads=16, output_dim=1024),
    "tiny-cnx": OpenClipTextConfig("tiny-cnx", vocab_size=1000, context_length=77, width=256, layers=2, heads=4, output_dim=128),
    "tiny-cnx-d": OpenClipTextConfig("tiny-cnx-d", vocab_size=1000, context_length=77, width=256, layers=2, heads=4, output_dim=128),
})
CONVNEXT_SEED = 611953
# Synthetic-weight scales (no checkpoint exists offline).  The layer scale gamma is drawn with a spread of order 1 around
# CONVNEXT_GAMMA_MEAN -- not timm's 1e-6 initialisation, under which every block would be the identity and the tests blind.  With
# unit-variance LayerNorm outputs and fc1 at std 1/sqrt(C) the pre-activations are N(0, 1) and E[gelu^2] = 0.425; fc2 at std
# CONVNEXT_FC2_STD/sqrt(4C) and the layer scale then add 0.425 * CONVNEXT_FC2_STD^2 * (mean^2 + spread^2) = 0.053 of variance per
# block to a stream of variance about 1: x 6.5 in variance (x 2.5 in magnitude) over the 36 blocks of the deepest tower -- far inside
# IEEE half's range, and every block still moves the stream by a fifth of its size.
CONVNEXT_GAMMA_MEAN, CONVNEXT_GAMMA_SPREAD, CONVNEXT_FC2_STD = 0.5, 0.5, 0.5


def clip_convnext_param_shapes(cfg: ClipConvNextConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """open_clip `visual.*` state-dict names of a ConvNeXt tower (prefix stripped), in definition order"""
    sh: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    d = cfg.dims

    def pair(name, c):
        sh[name + ".weight"] = (c,); sh[name + ".bias"] = (c,)

    sh["trunk.stem.0.weight"] = (d[0], 3, 4, 4); sh["trunk.stem.0.bias"] = (d[0],)
    pair("trunk.stem.1", d[0])
    for i in range(4):
        if i > 0:
            pair(f"trunk.stages.{i}.downsample.0", d[i - 1])
            sh[f"trunk.stages.{i}.downsample.1.weight"] = (d[i], d[i - 1], 2, 2); sh[f"trunk.stages.{i}.downsample.1.bias"] = (d[i],)
        for b in range(cfg.depths[i]):
            p = f"trunk.stages.{i}.blocks.{b}."
            sh[p + "gamma"] = (d[i],)
            sh[p + "conv_dw.weight"] = (d[i], 1, 7, 7); sh[p + "conv_dw.bias"] = (d[i],)
            pair(p + "norm", d[i])
            sh[p + "mlp.fc1.weight"] = (4 * d[i], d[i]); sh[p + "mlp.fc1.bias"] = (4 * d[i],)
            sh[p + "mlp.fc2.weight"] = (d[i], 4 * d[i]); sh[p + "mlp.fc2.bias"] = (d[i],)
    pair("trunk.head.norm", d[3])
    if cfg.proj == "linear":
        sh["head.proj.weight"] = (cfg.output_dim, d[3])
    elif cfg.proj == "mlp":
        sh["head.mlp.fc1.weight"] = (2 * cfg.output_dim, d[3]); sh["head.mlp.fc1.bias"] = (2 * cfg.output_dim,)
        sh["head.mlp.fc2.weight"] = (cfg.output_dim, 2 * cfg.output_dim)
    else:
        raise ValueError(f"ConvNeXt projection {cfg.proj!r}: want 'linear' or 'mlp'")
    return sh


def synthetic_clip_convnext_params(cfg: ClipConvNextConfig, seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """Seeded random weights of the real architecture at the scales stated above (CONVNEXT_*)"""
    g = torch.Generator().manual_seed(seed + CONVNEXT_SEED)
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape in clip_convnext_param_shapes(cfg).items():
        if name.endswith("gamma"):
            t = CONVNEXT_GAMMA_MEAN + CONVNEXT_GAMMA_SPREAD * torch.randn(shape, generator=g)
        elif len(shape) == 4:                                    # stem, downsample, depthwise: fan-in scaled
            t = torch.randn(shape, generator=g) / math.sqrt(shape[1] * shape[2] * shape[3])
        elif name.endswith("fc2.weight") and ".blocks." in name:
            t = torch.randn(shape, generator=g) * (CONVNEXT_FC2_STD / math.sqrt(shape[1]))
        elif len(shape) == 2:                                    # fc1, head projections
            t = torch.randn(shape, generator=g) / math.sqrt(shape[1])
        elif name.endswith(".weight"):                           # LayerNorm gamma
            t = 1.0 + 0.05 * torch.randn(shape, generator=g)
        else:                                                    # biases / LayerNorm beta
            t = 0.02 * torch.randn(shape, generator=g)
        out[name] = t
    return out


def fold_clip_convnext_params(cfg: ClipConvNextConfig, p) -> "OrderedDict[str, torch.Tensor]":
    """The tensors prx_clip_convnext_create expects, in its order (include/prx.h).  The layer scale is folded into fc2 --
    W2' = diag(gamma) W2, b2' = gamma * b2: the weights are frozen, so the fold is exact for values and data gradients and the engine
    needs no per-column scale.  The convolutions become matrices: the stem [d0, 3*4*4] in patchify's column order (c, py, px), the
    downsamples [d(i), 4 d(i-1)] in space-to-depth's ((dy, dx), c), the depthwise filters [C, 49]."""
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    d = cfg.dims

    def keep(key, name):
        out[key] = p[name].float()

    out["stem.weight"] = p["trunk.stem.0.weight"].float().reshape(d[0], 48)
    keep("stem.bias", "trunk.stem.0.bias"); keep("stem.ln.weight", "trunk.stem.1.weight"); keep("stem.ln.bias", "trunk.stem.1.bias")
    for i in range(4):
        s = f"trunk.stages.{i}."
        if i > 0:
            keep(f"stages.{i}.ds.ln.weight", s + "downsample.0.weight"); keep(f"stages.{i}.ds.ln.bias", s + "downsample.0.bias")
            out[f"stages.{i}.ds.weight"] = p[s + "downsample.1.weight"].float().permute(0, 2, 3, 1).reshape(d[i], 4 * d[i - 1]).contiguous()
            keep(f"stages.{i}.ds.bias", s + "downsample.1.bias")
        for b in range(cfg.depths[i]):
            q, k = f"{s}blocks.{b}.", f"stages.{i}.blocks.{b}."
            out[k + "dw.weight"] = p[q + "conv_dw.weight"].float().reshape(d[i], 49)
            keep(k + "dw.bias", q + "conv_dw.bias"); keep(k + "ln.weight", q + "norm.weight"); keep(k + "ln.bias", q + "norm.bias")
            keep(k + "fc1.weight", q + "mlp.fc1.weight"); keep(k + "fc1.bias", q + "mlp.fc1.bias")
            gamma = p[q + "gamma"].double()
            out[k + "fc2.weight"] = (gamma.view(-1, 1) * p[q + "mlp.fc2.weight"].double()).float()
            out[k + "fc2.bias"] = (gamma * p[q + "mlp.fc2.bias"].double()).float()
    keep("head.ln.weight", "trunk.head.norm.weight"); keep("head.ln.bias", "trunk.head.norm.bias")
    if cfg.proj == "linear":
        keep("head.proj.weight", "head.proj.weight")
    else:
        keep("head.fc1.weight", "head.mlp.fc1.weight"); keep("head.fc1.bias", "head.mlp.fc1.bias"); keep("head.fc2.weight", "head.mlp.fc2.weight")
    return out


def clip_convnext_activation_bytes(cfg: ClipConvNextConfig, precision: str = "fp16") -> int:
    """Device bytes per cutout of `max_batch` that prx_clip_convnext_create allocates beside the packed weights (csrc/convnext.hip):
    per block the GELU pre-activation [pixels][4C] and the stencil output [pixels][C] in the operand format with two fp32 statistics
    per pixel; per stage two fp32 stream buffers (and two operand twins in the 16-bit modes) and the downsample's statistics; the
    stem's patch matrix, product and their gradients; the backward's workspace sized by the largest map."""
    f32 = precision == "f32"
    op = 4 if f32 else 2
    g0 = cfg.input_resolution // 4
    total, emax = 0, 0
    for i in range(4):
        m = (g0 >> i) ** 2
        e = m * cfg.dims[i]
        emax = max(emax, e)
        total += 2 * e * 4 + (0 if f32 else 2 * e * op)
        if i > 0:
            total += 2 * 4 * m * 4
        total += cfg.depths[i] * (5 * e * op + 2 * m * 4)
    t = g0 * g0 + 1
    total += t * 48 * op + t * cfg.dims[0] * 4 + t * 48 * 4 + t * cfg.dims[0] * op + 2 * t * 4
    total += emax * op * (1 + 4 + 4 + 1) + 3 * emax * 4 + (0 if f32 else emax * op)
    d3, e_ = cfg.dims[3], cfg.output_dim
    total += 3 * d3 * 4 + 2 * 4 + d3 * op + 3 * 2 * e_ * op + e_ * op + 2 * e_ * 4
    return total


# ------------------------------------------------------------------------------------------ VGG16 (StyleLoss plugin)
VGG16_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512)   # torchvision cfg "D" to relu5_3


def vgg16_param_shapes() -> "OrderedDict[str, tuple]":
    """torchvision `vgg16().features` state-dict names and shapes (conv layers 0,2,5,...,28)."""
    sh: "OrderedDict[str, tuple]" = OrderedDict()
    idx, cin = 0, 3
    for v in VGG16_CFG:
        if v == "M":
            idx += 1
            continue
        sh[f"features.{idx}.weight"] = (v, cin, 3, 3)
        sh[f"features.{idx}.bias"] = (v,)
        cin = v
        idx += 2
    return sh


def synthetic_vgg16_params(seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """Seeded He-initialised weights (no checkpoint exists offline): activations stay O(1) through the 13 ReLU layers."""
    g = torch.Generator().manual_seed(seed + 1616)
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape in vgg16_param_shapes().items():
        if name.endswith("bias"):
            out[name] = 0.05 * torch.randn(shape, generator=g)
        else:
            out[name] = torch.randn(shape, generator=g) * math.sqrt(2.0 / (shape[1] * 9))
    return out


# ------------------------------------------------------------------------------------------ RRDBNet (super_resolution drawer)
@dataclass
class RrdbNetConfig:
    """basicsr's RRDBNet(num_in_ch=3, num_out_ch=3, scale=4) as RealESRGAN_x4plus uses it (super_resolution.py:60-62)"""
    num_feat: int = 64
    num_grow_ch: int = 32
    num_block: int = 23
    name: str = "RealESRGAN_x4plus"


RRDBNET_CONFIGS = {
    "RealESRGAN_x4plus": RrdbNetConfig(),
    # reduced depth with the SAME channel geometry: the kernels are specialised on channels, not on depth
    "tiny-RRDB": RrdbNetConfig(num_block=1, name="tiny-RRDB"),
}


def rrdbnet_conv_names(cfg: RrdbNetConfig):
    names = ["conv_first"]
    for i in range(cfg.num_block):
        for r in (1, 2, 3):
            names += [f"body.{i}.rdb{r}.conv{k}" for k in range(1, 6)]
    return names + ["conv_body", "conv_up1", "conv_up2", "conv_hr", "conv_last"]


def rrdbnet_param_shapes(cfg: RrdbNetConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """basicsr state-dict names and shapes, in the order the C ABI takes them (include/prx.h prx_rrdbnet_create)"""
    f, g = cfg.num_feat, cfg.num_grow_ch
    sh: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    for name in rrdbnet_conv_names(cfg):
        if name == "conv_first":
            cin, cout = 3, f
        elif name == "conv_last":
            cin, cout = f, 3
        elif name.startswith("body."):
            k = int(name[-1])
            cin, cout = f + g * (k - 1), (f if k == 5 else g)
        else:
            cin, cout = f, f
        sh[name + ".weight"] = (cout, cin, 3, 3)
        sh[name + ".bias"] = (cout,)
    return sh


RRDBNET_LAST_STD = 0.35          # conv_last weight std * sqrt(fan_in): see synthetic_rrdbnet_params


def synthetic_rrdbnet_params(cfg: RrdbNetConfig, seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """Seeded weights of the real architecture (no checkpoint offline) under which a drawer does not start saturated.
    Kaiming-scaled convolutions with basicsr's x0.1 on the dense blocks put ~90 % of the pre-clamp output outside [0,1] at 23
    blocks, and the reason is the architecture's skips, not the convolutions: with small dense-block weights rdb3(rdb2(rdb1(x)))
    is close to x, so every RRDB returns about 0.2 x + x and the trunk grows like 1.2 ** num_block (x66 at 23 blocks).  The
    network is positively homogeneous in the trunk apart from its small biases, so conv_body is scaled by 1.2 ** -num_block:
    what it adds to the first features is then O(1) at any depth, and conv_last maps the O(1) features to 0.5 +- ~0.3
    (tests/test_super_resolution_host.py holds 2 % .. 30 % of the pre-clamp values outside [0,1] at 23 blocks, z ~ U[0,1]
    16 x 16).  Every bias is non-zero."""
    g = torch.Generator().manual_seed(seed + 2323)
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape in rrdbnet_param_shapes(cfg).items():
        base = name.rsplit(".", 1)[0]
        if name.endswith("bias"):
            out[name] = 0.02 * torch.randn(shape, generator=g) + (0.5 if base == "conv_last" else 0.0)
            continue
        std = math.sqrt(2.0 / (1.0 + 0.2 ** 2) / (shape[1] * 9))          # Kaiming for LeakyReLU(0.2)
        if base.startswith("body."):
            std *= 0.1                                                     # basicsr default_init_weights(scale=0.1)
        elif base == "conv_body":
            std *= 1.2 ** -cfg.num_block
        elif base == "conv_last":
            std = RRDBNET_LAST_STD / math.sqrt(shape[1] * 9)
        out[name] = torch.randn(shape, generator=g) * std
    return out
