"""State-dict adapters for real checkpoints.  No checkpoint can be downloaded offline, so these
are exercised in tests with randomly initialised upstream-format state dicts; the formats are:

* OpenAI CLIP (`clip.load(name)` state dict, slip.py:175): keys `visual.conv1.weight`, `visual.class_embedding`,
  `visual.positional_embedding`, `visual.ln_pre.*`, `visual.transformer.resblocks.{i}.*`, `visual.ln_post.*`,
  `visual.proj` -> strip the `visual.` prefix (weights may be fp16 on CUDA: cast to fp32).  The ModifiedResNet models (RN50 ...
  RN50x64) carry `visual.conv{1,2,3}`, `visual.bn{1,2,3}.*`, `visual.layer{1..4}.{b}.*` and `visual.attnpool.*` instead.
* OpenCLIP (`open_clip.create_model(name, pretrained=...).state_dict()`, the LAION towers): its native ViT models keep OpenAI's key
  names on both sides; the geometry comes from the named configuration (`clip_visual_from_openclip` / `clip_text_from_openclip`).
  Its ConvNeXt models wrap a timm trunk: `visual.trunk.stem.*`, `visual.trunk.stages.{i}.{downsample,blocks.{b}}.*`,
  `visual.trunk.head.norm.*`, `visual.head.{proj | mlp.fc1, mlp.fc2}.*` (`clip_convnext_from_openclip`).
* HF `CLIPVisionModelWithProjection` -> the same names (q/k/v projections are concatenated into `in_proj_*`).
* taming-transformers VQGAN Lightning checkpoint (`vqgan.py:124-140`): `state_dict` with `decoder.*`,
  `post_quant_conv.*`, `quantize.embedding.weight` for the decoder runner, plus `encoder.*` / `quant_conv.*` for the
  encoder runner when the checkpoint has them (`loss.*` is dropped, as `del model.loss` does at vqgan.py:139).
* facebookresearch/SLIP checkpoints (`models/slip_base_100ep.pt`, ..., slip.py:90-140): `load_slip`.
* torchvision `vgg16` (`models.vgg16(pretrained=True)`, Losses/StyleLoss.py:27): `features.{0,2,5,...,28}.{weight,bias}`;
  the `classifier.*` tensors are dropped (the StyleLoss extractor stops at relu5_3).
* RealESRGAN (`models/super_resolution_RealESRGAN_x4plus.ckpt`, super_resolution.py:47-61, real_esrganer.py:54-60): basicsr's
  RRDBNet state dict under `params_ema`, else `params`: `load_rrdbnet`.
"""
from collections import OrderedDict
from typing import Dict

import torch

from .weights import (ClipResNetConfig, ClipTextConfig, ClipVitConfig, VqganConfig, clip_resnet_param_shapes, clip_text_param_shapes,
                      clip_vit_param_shapes, slip_vit_param_shapes, vgg16_param_shapes, vqgan_encoder_param_shapes, vqgan_param_shapes)


def _check(params: Dict[str, torch.Tensor], shapes) -> "OrderedDict[str, torch.Tensor]":
    out = OrderedDict()
    for name, shape in shapes.items():
        if name not in params:
            raise KeyError(f"checkpoint is missing {name}")
        t = params[name].detach().float().contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: checkpoint has shape {tuple(t.shape)}, the configuration needs {tuple(shape)}")
        out[name] = t
    return out


def clip_visual_from_openai(state_dict: Dict[str, torch.Tensor], cfg):
    """visual side of an OpenAI CLIP state dict: the ViT towers' tensors in the order of `clip_vit_param_shapes`, or -- for a
    ClipResNetConfig (RN50 ... RN50x64) -- the ModifiedResNet's in the order of `clip_resnet_param_shapes` (BatchNorm un-folded, its
    `num_batches_tracked` counters dropped: ops.ClipResNetHandle folds)."""
    params = {k[len("visual."):]: v for k, v in state_dict.items() if k.startswith("visual.")}
    if isinstance(cfg, ClipResNetConfig):
        return _check(params, clip_resnet_param_shapes(cfg))
    return _check(params, clip_vit_param_shapes(cfg))


def _openclip_configs(name_or_cfg, text: bool):
    from .weights import CLIP_TEXT_CONFIGS, OPENCLIP_CONFIGS
    if not isinstance(name_or_cfg, str):
        return name_or_cfg
    if name_or_cfg not in OPENCLIP_CONFIGS:
        raise KeyError(f"unknown OpenCLIP model {name_or_cfg!r} (supported: {sorted(OPENCLIP_CONFIGS)})")
    return CLIP_TEXT_CONFIGS[name_or_cfg] if text else OPENCLIP_CONFIGS[name_or_cfg]


def clip_visual_from_openclip(state_dict: Dict[str, torch.Tensor], name_or_cfg):
    """visual side of an OpenCLIP state dict of a native ViT model (`visual.conv1.weight`, `visual.class_embedding`, ...: OpenAI's key
    names) for the named configuration (`ViT-B-32`, `ViT-B-16`, `ViT-L-14`, `ViT-H-14`, `ViT-g-14`, `ViT-bigG-14`) or an OpenClipVitConfig.  The geometry --
    the MLP width included, which is 6144 / 8192 and not 4 x width in the last two -- is the
    configuration's, never read off the tensors: `clip_config_from_state_dict` takes heads = width // 64 as `clip.model.build_model`
    does, which is wrong for ViT-H-14 (16 heads of 80 on width 1280).  A missing or mis-shaped tensor is named."""
    cfg = _openclip_configs(name_or_cfg, text=False)
    params = {k[len("visual."):]: v for k, v in state_dict.items() if k.startswith("visual.")}
    return _check(params, clip_vit_param_shapes(cfg))


def clip_text_from_openclip(state_dict: Dict[str, torch.Tensor], name_or_cfg):
    """text side of the same state dict: the un-prefixed entries under OpenAI's names, for the named configuration's geometry
    (`attn_mask` and `logit_scale` ride along in the file and are not read)"""
    return _check(dict(state_dict), clip_text_param_shapes(_openclip_configs(name_or_cfg, text=True)))


def clip_convnext_from_openclip(state_dict: Dict[str, torch.Tensor], name_or_cfg, text_cfg=None):
    """-> (params, text_params) of an OpenCLIP ConvNeXt model's state dict (`open_clip.create_model("convnext_base_w", ...)`): the
    visual side's `visual.trunk.*` and `visual.head.*` entries with the prefix stripped, in the order of `clip_convnext_param_shapes`
    (the layer scale `gamma` un-folded: ops.ClipConvNextHandle folds), and the un-prefixed text entries under OpenAI's names.  The
    geometry is the named configuration's (or a ClipConvNextConfig with its OpenClipTextConfig); a missing or mis-shaped tensor is
    named."""
    from .weights import CLIP_CONVNEXT_CONFIGS, CLIP_TEXT_CONFIGS, clip_convnext_param_shapes
    if isinstance(name_or_cfg, str):
        if name_or_cfg not in CLIP_CONVNEXT_CONFIGS:
            raise KeyError(f"unknown OpenCLIP ConvNeXt model {name_or_cfg!r} (supported: {sorted(CLIP_CONVNEXT_CONFIGS)})")
        cfg, text_cfg = CLIP_CONVNEXT_CONFIGS[name_or_cfg], CLIP_TEXT_CONFIGS[name_or_cfg]
    else:
        cfg = name_or_cfg
        if text_cfg is None:
            text_cfg = CLIP_TEXT_CONFIGS[cfg.name]
    visual = {k[len("visual."):]: v for k, v in state_dict.items() if k.startswith("visual.")}
    return _check(visual, clip_convnext_param_shapes(cfg)), _check(dict(state_dict), clip_text_param_shapes(text_cfg))


def clip_visual_from_hf(state_dict: Dict[str, torch.Tensor], cfg: ClipVitConfig):
    sd = state_dict
    p = {"class_embedding": sd["vision_model.embeddings.class_embedding"],
         "conv1.weight": sd["vision_model.embeddings.patch_embedding.weight"],
         "positional_embedding": sd["vision_model.embeddings.position_embedding.weight"],
         "ln_pre.weight": sd["vision_model.pre_layrnorm.weight"], "ln_pre.bias": sd["vision_model.pre_layrnorm.bias"],
         "ln_post.weight": sd["vision_model.post_layernorm.weight"], "ln_post.bias": sd["vision_model.post_layernorm.bias"],
         "proj": sd["visual_projection.weight"].T}
    for i in range(cfg.layers):
        a, b = f"transformer.resblocks.{i}.", f"vision_model.encoder.layers.{i}."
        p[a + "attn.in_proj_weight"] = torch.cat([sd[b + f"self_attn.{n}_proj.weight"] for n in "qkv"], 0)
        p[a + "attn.in_proj_bias"] = torch.cat([sd[b + f"self_attn.{n}_proj.bias"] for n in "qkv"], 0)
        p[a + "attn.out_proj.weight"] = sd[b + "self_attn.out_proj.weight"]
        p[a + "attn.out_proj.bias"] = sd[b + "self_attn.out_proj.bias"]
        for (x, y) in (("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"), ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
            p[a + x + ".weight"] = sd[b + y + ".weight"]
            p[a + x + ".bias"] = sd[b + y + ".bias"]
    return _check(p, clip_vit_param_shapes(cfg))


def clip_text_from_openai(state_dict: Dict[str, torch.Tensor], cfg: ClipTextConfig):
    """text side of an OpenAI CLIP state dict: the un-prefixed entries (`token_embedding.weight`, `positional_embedding`,
    `transformer.resblocks.*`, `ln_final.*`, `text_projection`)"""
    return _check(dict(state_dict), clip_text_param_shapes(cfg))


def clip_text_from_hf(state_dict: Dict[str, torch.Tensor], cfg: ClipTextConfig):
    sd = state_dict
    p = {"token_embedding.weight": sd["text_model.embeddings.token_embedding.weight"],
         "positional_embedding": sd["text_model.embeddings.position_embedding.weight"],
         "ln_final.weight": sd["text_model.final_layer_norm.weight"], "ln_final.bias": sd["text_model.final_layer_norm.bias"],
         "text_projection": sd["text_projection.weight"].T}
    for i in range(cfg.layers):
        a, b = f"transformer.resblocks.{i}.", f"text_model.encoder.layers.{i}."
        p[a + "attn.in_proj_weight"] = torch.cat([sd[b + f"self_attn.{n}_proj.weight"] for n in "qkv"], 0)
        p[a + "attn.in_proj_bias"] = torch.cat([sd[b + f"self_attn.{n}_proj.bias"] for n in "qkv"], 0)
        p[a + "attn.out_proj.weight"] = sd[b + "self_attn.out_proj.weight"]
        p[a + "attn.out_proj.bias"] = sd[b + "self_attn.out_proj.bias"]
        for (x, y) in (("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"), ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
            p[a + x + ".weight"] = sd[b + y + ".weight"]
            p[a + x + ".bias"] = sd[b + y + ".bias"]
    return _check(p, clip_text_param_shapes(cfg))


def vqgan_from_taming(state_dict: Dict[str, torch.Tensor], cfg: VqganConfig, with_encoder: bool = None):
    """-> one ordered dict usable as `settings.vqgan_state_dict`: the decoder entries, and the encoder entries when the
    checkpoint has them (`with_encoder=None`: if present; True: required; False: dropped)."""
    sd = dict(state_dict.get("state_dict", state_dict))
    out = _check(sd, vqgan_param_shapes(cfg))
    if with_encoder is None:
        with_encoder = any(k.startswith("encoder.") for k in sd)
    if with_encoder:
        out.update(_check(sd, vqgan_encoder_param_shapes(cfg)))
    return out


TAMING_TARGETS = {"taming.models.vqgan.VQModel": ("", False), "taming.models.vqgan.GumbelVQ": ("", True),
                  "taming.models.cond_transformer.Net2NetTransformer": ("first_stage_model.", False)}


def vqgan_config_from_taming_yaml(path_or_dict):
    """taming's model yaml (`model.target` + `model.params.{embed_dim, n_embed, ddconfig}`; what `OmegaConf.load` reads at
    vqgan.py:121) -> (VqganConfig, key prefix of the first-stage model inside the checkpoint, gumbel flag).  For a
    Net2NetTransformer config the first stage is `params.first_stage_config` (vqgan.py:131-135)."""
    import yaml
    doc = path_or_dict
    if not isinstance(doc, dict):
        with open(path_or_dict) as f:
            doc = yaml.safe_load(f)
    model = doc["model"]
    target = model["target"]
    if target not in TAMING_TARGETS:
        raise ValueError(f"unknown model type: {target}")                     # vqgan.py:136-137
    prefix, gumbel = TAMING_TARGETS[target]
    prm = model["params"]
    if prefix:                                                                # the transformer wraps a VQModel config
        prm = prm["first_stage_config"]["params"]
    dd = prm["ddconfig"]
    if dd.get("double_z", False):
        raise ValueError("ddconfig.double_z=True is a KL autoencoder, not a VQGAN")
    cfg = VqganConfig(ch=int(dd["ch"]), ch_mult=tuple(int(m) for m in dd["ch_mult"]), num_res_blocks=int(dd["num_res_blocks"]),
                      attn_resolutions=tuple(int(r) for r in dd["attn_resolutions"]), resolution=int(dd["resolution"]),
                      z_channels=int(dd["z_channels"]), embed_dim=int(prm["embed_dim"]), n_embed=int(prm["n_embed"]),
                      out_ch=int(dd.get("out_ch", 3)))
    if int(dd.get("in_channels", 3)) != 3 or cfg.out_ch != 3:
        raise ValueError("only RGB VQGANs are supported (ddconfig.in_channels / out_ch must be 3)")
    return cfg, prefix, gumbel


def load_taming(config_path: str, checkpoint_path: str, with_encoder: bool = None):
    """The reference's `load_model` (vqgan.py:96-140) without the download and without taming: yaml ddconfig -> VqganConfig,
    Lightning `.ckpt` (`{"state_dict": ...}` with `loss.*` discriminator entries that `del model.loss` drops) -> the ordered
    parameter dict of the HIP runner.  GumbelVQ keeps its codebook under `quantize.embed.weight` (vqgan.py:193): renamed to
    the runner's `quantize.embedding.weight`.  -> (cfg, params, gumbel)"""
    cfg, prefix, gumbel = vqgan_config_from_taming_yaml(config_path)
    blob = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
    sd = blob.get("state_dict", blob)
    if prefix:
        sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    sd = {k: v for k, v in sd.items() if not k.startswith("loss.")}
    if gumbel and "quantize.embed.weight" in sd:
        sd["quantize.embedding.weight"] = sd.pop("quantize.embed.weight")
    out = vqgan_from_taming(sd, cfg, with_encoder)
    if gumbel:
        # GumbelQuantize's logits projection (a 1x1 convolution z_channels -> n_embed): not on the decode path; kept so that
        # VqganDrawer can ENCODE an image the way GumbelVQ.encode does (init_image / overlay / z labels, vqgan.py:174-185)
        for k in ("quantize.proj.weight", "quantize.proj.bias"):
            if k in sd:
                out[k] = sd[k].detach().float().contiguous()
    return cfg, out, gumbel


def clip_state_dict_from_archive(path: str) -> Dict[str, torch.Tensor]:
    """What `clip.load(name, download_root="models")` reads (slip.py:175): OpenAI publishes every CLIP model as a TorchScript
    archive (`ViT-B-32.pt`, ...), and `clip.load` takes `torch.jit.load(path).state_dict()` from it; a plain pickled state dict
    (or `{"state_dict": ...}`) is accepted as well, as `clip.load` does when the file is not an archive.  The result feeds
    `clip_visual_from_openai` / `clip_text_from_openai` (fp16 tensors are cast to fp32 there)."""
    try:
        module = torch.jit.load(path, map_location="cpu")
        sd = module.state_dict()
    except RuntimeError:
        blob = torch.load(path, map_location="cpu", weights_only=False)
        sd = blob.get("state_dict", blob) if isinstance(blob, dict) else blob.state_dict()
    return {k: v.detach() for k, v in sd.items()}


def clip_config_from_state_dict(sd: Dict[str, torch.Tensor], name: str = "checkpoint"):
    """`clip.model.build_model` reads the geometry off the tensors' shapes; so does this: a ClipVitConfig when the state dict has
    `visual.proj`, else the ClipResNetConfig of a ModifiedResNet (width from `visual.layer1.0.conv1.weight`, blocks per layer counted,
    resolution from the attention pool's positional embedding, heads = width * 32 // 64)."""
    if "visual.proj" in sd:
        width = sd["visual.conv1.weight"].shape[0]
        patch = sd["visual.conv1.weight"].shape[-1]
        layers = len({k.split(".")[3] for k in sd if k.startswith("visual.transformer.resblocks.")})
        grid = round((sd["visual.positional_embedding"].shape[0] - 1) ** 0.5)
        return ClipVitConfig(name, patch * grid, patch, width, layers, width // 64, sd["visual.proj"].shape[1])
    for k in ("visual.layer1.0.conv1.weight", "visual.attnpool.positional_embedding", "visual.attnpool.c_proj.weight"):
        if k not in sd:
            raise KeyError(f"not a CLIP state dict: neither visual.proj (ViT) nor {k} (ModifiedResNet)")
    width = sd["visual.layer1.0.conv1.weight"].shape[0]
    layers = tuple(len({k.split(".")[2] for k in sd if k.startswith(f"visual.layer{b}.")}) for b in (1, 2, 3, 4))
    grid = round((sd["visual.attnpool.positional_embedding"].shape[0] - 1) ** 0.5)
    return ClipResNetConfig(name, grid * 32, width, layers, width * 32 // 64, sd["visual.attnpool.c_proj.weight"].shape[0])


def clip_text_config_from_state_dict(sd: Dict[str, torch.Tensor], name: str = "checkpoint") -> ClipTextConfig:
    """the text side of `clip.model.build_model`: width and heads (width // 64) from `ln_final`, layers counted"""
    for k in ("token_embedding.weight", "positional_embedding", "ln_final.weight", "text_projection"):
        if k not in sd:
            raise KeyError(f"checkpoint is missing {k}")
    width = sd["ln_final.weight"].shape[0]
    layers = len({k.split(".")[2] for k in sd if k.startswith("transformer.resblocks.")})
    return ClipTextConfig(name, sd["token_embedding.weight"].shape[0], sd["positional_embedding"].shape[0], width, layers, width // 64,
                          sd["text_projection"].shape[1])


def load_slip(path: str, cfg, text_cfg: ClipTextConfig):
    """A facebookresearch/SLIP checkpoint (`models/slip_*.pt` / `clip_*.pt`, slip.py:90-140): `{"state_dict": ..., "args":
    argparse.Namespace, ...}` saved from a DistributedDataParallel model, so every key carries `module.`.  -> (image-side
    parameters: the timm `visual.*` entries with the prefix stripped + `image_projection`; text-side parameters under the names
    of `clip_text_param_shapes`).  The SSL-only entries (`image_mlp.*`, SLIP's SimCLR head) and `logit_scale` are dropped: neither
    encode_image nor encode_text reads them.  Loaded with `weights_only=True`; the only non-tensor class admitted is the
    `argparse.Namespace` of `ckpt['args']`.  A missing or mis-shaped tensor is reported by name."""
    import argparse
    with torch.serialization.safe_globals([argparse.Namespace]):
        blob = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(blob, dict) or "state_dict" not in blob:
        raise ValueError(f"{path}: not a SLIP checkpoint (no 'state_dict' entry)")
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in blob["state_dict"].items()}
    image = {k[len("visual."):]: v for k, v in sd.items() if k.startswith("visual.")}
    if "image_projection" in sd:
        image["image_projection"] = sd["image_projection"]
    text_names = set(clip_text_param_shapes(text_cfg))
    text = {k: v for k, v in sd.items() if k in text_names}
    try:
        return _check(image, slip_vit_param_shapes(cfg)), _check(text, clip_text_param_shapes(text_cfg))
    except (KeyError, ValueError) as e:
        raise type(e)(f"{path}: {e.args[0]}") from None


def vgg16_from_torchvision(state_dict: Dict[str, torch.Tensor]):
    """torchvision VGG16 state dict (optionally wrapped as {"state_dict": ...} or prefixed `module.`) -> the 26 tensors the
    StyleLoss extractor needs (`pixray_amd.style_loss.Vgg16Extractor(params=...)`)"""
    sd = state_dict.get("state_dict", state_dict)
    params = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    return _check(params, vgg16_param_shapes())


def load_rrdbnet(path: str, cfg):
    """A RealESRGAN checkpoint file -> the RRDBNet runner's parameters (weights.rrdbnet_param_shapes order).  The file keeps
    basicsr's state dict under `params_ema`, else `params` (real_esrganer.py:54-60); names and shapes are checked strictly and
    the first missing or mismatching key is named.  Nothing is ever fetched: a file that is not there is an error."""
    from .weights import rrdbnet_param_shapes
    loadnet = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(loadnet, dict) and "params_ema" in loadnet:
        sd = loadnet["params_ema"]
    elif isinstance(loadnet, dict) and "params" in loadnet:
        sd = loadnet["params"]
    else:
        raise KeyError(f"{path}: no `params_ema` / `params` entry (not a RealESRGAN checkpoint)")
    shapes = rrdbnet_param_shapes(cfg)
    out = _check(sd, shapes)
    extra = [k for k in sd if k not in shapes]
    if extra:
        raise KeyError(f"{path}: unexpected entry {extra[0]} (the configuration has {cfg.num_block} blocks)")
    return out
