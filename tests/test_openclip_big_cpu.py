"""OpenCLIP ViT-g-14 and ViT-bigG-14 without a device: the configuration tables (MLP widths 6144 / 8192, heads of 88 / 104), the
shape lists, the synthetic weights, and the state-dict adapter on correct and mis-shaped tensors.

Every test here fails on a tree without the two names (`KeyError: unknown / unsupported perceptor 'ViT-g-14'`)."""
import dataclasses
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from pixray_amd import checkpoints, perceptor, weights  # noqa: E402

GEOMETRY = {       # [UPSTREAM open_clip model_configs ViT-g-14.json / ViT-bigG-14.json, restated]
    "ViT-g-14": dict(vision=(224, 14, 1408, 40, 16, 1024, 257), mlp=6144, head_dim=88, text=(1024, 16, 24, 1024)),
    "ViT-bigG-14": dict(vision=(224, 14, 1664, 48, 16, 1280, 257), mlp=8192, head_dim=104, text=(1280, 20, 32, 1280)),
}
TINY = {"tiny-g-32": ("ViT-g-14", 50), "tiny-g-14": ("ViT-g-14", 257), "tiny-bigG-32": ("ViT-bigG-14", 50), "tiny-bigG-14": ("ViT-bigG-14", 257)}


@pytest.mark.parametrize("name", sorted(GEOMETRY))
def test_the_names_resolve_to_the_published_geometry(name):
    v, t = perceptor.perceptor_config(name)
    want = GEOMETRY[name]
    assert isinstance(v, weights.OpenClipVitConfig) and name in weights.OPENCLIP_CONFIGS and name not in weights.CLIP_CONFIGS
    assert (v.input_resolution, v.patch_size, v.width, v.layers, v.heads, v.output_dim, v.tokens) == want["vision"]
    assert v.mlp == v.mlp_width == want["mlp"] and v.mlp != 4 * v.width and v.head_dim == want["head_dim"]
    assert v.width % 128 == 0 and v.width % 256 == 128 and v.width <= 2048        # the ragged LayerNorm's widths
    assert isinstance(t, weights.OpenClipTextConfig) and t.gelu
    assert (t.width, t.heads, t.layers, t.output_dim) == want["text"] and t.output_dim == v.output_dim
    assert t.width == 64 * t.heads and t.width % 256 == 0 and (t.context_length, t.vocab_size) == (77, 49408)


@pytest.mark.parametrize("name", sorted(TINY))
def test_the_reduced_configs_keep_width_heads_and_mlp(name):
    v, t = perceptor.perceptor_config(name)
    full = weights.OPENCLIP_CONFIGS[TINY[name][0]]
    assert (v.width, v.heads, v.mlp, v.head_dim) == (full.width, full.heads, full.mlp, full.head_dim)
    assert (v.layers, v.output_dim, v.tokens) == (2, 128, TINY[name][1])
    assert (t.width, t.heads, t.layers, t.output_dim, t.vocab_size) == (256, 4, 2, 128, 1000) and t.gelu


def test_the_other_configs_keep_four_times_width():
    for name, cfg in weights.OPENCLIP_CONFIGS.items():
        if name not in GEOMETRY and name not in TINY:
            assert cfg.mlp_width == 0 and cfg.mlp == 4 * cfg.width, name
    sh = weights.clip_vit_param_shapes(weights.CLIP_CONFIGS["ViT-B/32"])          # a config without the field
    assert sh["transformer.resblocks.0.mlp.c_fc.weight"] == (3072, 768)


def test_shape_lists_and_synthetic_weights():
    for name, want in GEOMETRY.items():
        v, t = perceptor.perceptor_config(name)
        w, m = v.width, want["mlp"]
        sh = weights.clip_vit_param_shapes(v)
        last = f"transformer.resblocks.{v.layers - 1}."
        assert sh["conv1.weight"] == (w, 3, 14, 14) and sh["positional_embedding"] == (257, w) and sh["proj"] == (w, v.output_dim)
        assert sh[last + "attn.in_proj_weight"] == (3 * w, w) and sh[last + "attn.out_proj.weight"] == (w, w)
        assert sh[last + "mlp.c_fc.weight"] == (m, w) and sh[last + "mlp.c_fc.bias"] == (m,)
        assert sh["transformer.resblocks.0.mlp.c_proj.weight"] == (w, m) and sh["transformer.resblocks.0.mlp.c_proj.bias"] == (w,)
        assert len(sh) == 5 + 12 * v.layers + 3
        tsh = weights.clip_text_param_shapes(t)
        assert tsh["transformer.resblocks.0.mlp.c_fc.weight"] == (4 * t.width, t.width) and tsh["text_projection"] == (t.width, t.output_dim)
    for name in ("tiny-g-32", "tiny-bigG-14"):
        cfg = weights.OPENCLIP_CONFIGS[name]
        p = weights.synthetic_clip_vit_params(cfg, 3)
        assert {k: tuple(x.shape) for k, x in p.items()} == dict(weights.clip_vit_param_shapes(cfg))
        assert all(x.dtype == torch.float32 and torch.isfinite(x).all() for x in p.values())
        assert torch.equal(p["transformer.resblocks.1.mlp.c_fc.weight"], weights.synthetic_clip_vit_params(cfg, 3)["transformer.resblocks.1.mlp.c_fc.weight"])


def test_the_state_dict_adapter_takes_the_configs_mlp_width_and_names_a_mis_shaped_tensor():
    cfg = weights.OPENCLIP_CONFIGS["tiny-bigG-32"]
    p = weights.synthetic_clip_vit_params(cfg, 1)
    sd = {"visual." + k: v.half() for k, v in p.items()}
    sd["logit_scale"] = torch.tensor(1.0)
    got = checkpoints.clip_visual_from_openclip(sd, "tiny-bigG-32")
    assert list(got) == list(weights.clip_vit_param_shapes(cfg)) and got["transformer.resblocks.0.mlp.c_fc.weight"].shape == (8192, 1664)
    assert all(t.dtype == torch.float32 for t in got.values())
    # a checkpoint with a 4 x width MLP handed to the same name
    wrong = {"visual." + k: v for k, v in weights.synthetic_clip_vit_params(dataclasses.replace(cfg, mlp_width=0), 1).items()}
    with pytest.raises(ValueError, match=r"transformer\.resblocks\.0\.mlp\.c_fc\.weight: checkpoint has shape \(6656, 1664\), the configuration needs \(8192, 1664\)"):
        checkpoints.clip_visual_from_openclip(wrong, "tiny-bigG-32")
    sd2 = dict(sd)
    sd2["visual.transformer.resblocks.1.mlp.c_proj.weight"] = torch.zeros(1664, 6656)
    with pytest.raises(ValueError, match=r"resblocks\.1\.mlp\.c_proj\.weight: checkpoint has shape \(1664, 6656\)"):
        checkpoints.clip_visual_from_openclip(sd2, cfg)
    del sd2["visual.transformer.resblocks.1.mlp.c_proj.weight"]
    with pytest.raises(KeyError, match=r"missing transformer\.resblocks\.1\.mlp\.c_proj\.weight"):
        checkpoints.clip_visual_from_openclip(sd2, cfg)
    for name in GEOMETRY:
        assert checkpoints._openclip_configs(name, text=True) is weights.CLIP_TEXT_CONFIGS[name]


def test_the_older_lookup_keeps_its_domain():
    """clip_perceptor_config served towers with a 4 x width MLP only; it refuses the names that carry an MLP width and names the other lookup"""
    for name in list(GEOMETRY) + list(TINY):
        with pytest.raises(KeyError, match="use perceptor_config"):
            perceptor.clip_perceptor_config(name)
    assert perceptor.clip_perceptor_config("ViT-H-14") == perceptor.perceptor_config("ViT-H-14")


def test_an_unknown_name_lists_the_two_new_ones():
    with pytest.raises(KeyError, match="unknown / unsupported perceptor") as e:
        perceptor.perceptor_config("ViT-G-14")
    for name in GEOMETRY:
        assert repr(name) in str(e.value), name
