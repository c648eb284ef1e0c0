"""The OpenCLIP (LAION) perceptors without a device: configuration tables, the shape lists of ViT-H-14, the state-dict adapters and
their error messages, the front end, and the head padding of the weight packs on the CPU emulation of the runner's own code.

Every test here fails on a tree without the OpenCLIP names (`KeyError: unknown / unsupported perceptor 'ViT-H-14'`)."""
import os
import shutil
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _emu  # noqa: E402
from pixray_amd import checkpoints, perceptor, weights  # noqa: E402

NAMES = ("ViT-B-32", "ViT-B-16", "ViT-L-14", "ViT-H-14")


# ------------------------------------------------------------------------------------------------ configurations
def test_config_tables():
    """the four names resolve to the published geometry [UPSTREAM open_clip model_configs]; the three that share a geometry with an
    OpenAI tower differ from it in the activation only"""
    for name, twin in (("ViT-B-32", "ViT-B/32"), ("ViT-B-16", "ViT-B/16"), ("ViT-L-14", "ViT-L/14")):
        v, t = perceptor.clip_perceptor_config(name)
        ov, ot = perceptor.clip_perceptor_config(twin)
        assert isinstance(v, weights.OpenClipVitConfig) and not isinstance(ov, weights.OpenClipVitConfig)
        assert (v.input_resolution, v.patch_size, v.width, v.layers, v.heads, v.output_dim) == \
               (ov.input_resolution, ov.patch_size, ov.width, ov.layers, ov.heads, ov.output_dim)
        assert (t.vocab_size, t.context_length, t.width, t.layers, t.heads, t.output_dim) == \
               (ot.vocab_size, ot.context_length, ot.width, ot.layers, ot.heads, ot.output_dim)
        assert t.gelu and not getattr(ot, "gelu", False) and v.head_dim == 64
    v, t = perceptor.clip_perceptor_config("ViT-H-14")
    assert isinstance(v, weights.OpenClipVitConfig)
    assert (v.input_resolution, v.patch_size, v.width, v.layers, v.heads, v.output_dim, v.tokens) == (224, 14, 1280, 32, 16, 1024, 257)
    assert v.head_dim == 80 and v.width % 256 == 0            # LayerNorm's width rule; the heads are padded to 96 by the runner
    assert (t.width, t.heads, t.layers, t.output_dim, t.context_length, t.vocab_size) == (1024, 16, 24, 1024, 77, 49408)
    assert t.gelu and t.width == 64 * t.heads
    for name in NAMES:
        assert name in weights.OPENCLIP_CONFIGS and name not in weights.CLIP_CONFIGS and name in weights.CLIP_TEXT_CONFIGS
    for refused in ("ViT-g-14", "ViT-bigG-14"):             # widths 1408 / 1664 are no multiple of 256
        with pytest.raises(KeyError, match="unknown / unsupported perceptor"):
            perceptor.clip_perceptor_config(refused)


def test_vit_h_14_shape_lists():
    v, t = perceptor.clip_perceptor_config("ViT-H-14")
    sh = weights.clip_vit_param_shapes(v)
    assert sh["conv1.weight"] == (1280, 3, 14, 14) and sh["positional_embedding"] == (257, 1280) and sh["proj"] == (1280, 1024)
    assert sh["transformer.resblocks.31.attn.in_proj_weight"] == (3840, 1280) and sh["transformer.resblocks.31.mlp.c_fc.weight"] == (5120, 1280)
    assert sh["transformer.resblocks.0.mlp.c_proj.weight"] == (1280, 5120) and "transformer.resblocks.32.ln_1.weight" not in sh
    assert len(sh) == 5 + 12 * 32 + 3
    tsh = weights.clip_text_param_shapes(t)
    assert tsh["token_embedding.weight"] == (49408, 1024) and tsh["positional_embedding"] == (77, 1024) and tsh["text_projection"] == (1024, 1024)
    assert tsh["transformer.resblocks.23.attn.in_proj_weight"] == (3072, 1024) and len(tsh) == 2 + 12 * 24 + 3


def test_an_unknown_name_lists_the_new_ones():
    with pytest.raises(KeyError, match="unknown / unsupported perceptor") as e:
        perceptor.clip_perceptor_config("ViT-H-15")
    for name in NAMES + ("ViT-B/32", "RN50", "SLIP_VITB16"):
        assert repr(name) in str(e.value), name


def test_the_synthetic_weights_of_a_hyphen_name_are_its_own(monkeypatch):
    """`ViT-B-32` without a file carries seeded synthetic weights, and not the ones of `ViT-B/32`; it is built by the OpenCLIP handle"""
    from pixray_amd import ops
    made = {}

    def stub(kind):
        def make(cfg, params, mb, dev, precision=None):
            made[cfg.name] = (kind, params)
            return object()
        return make
    monkeypatch.setattr(ops, "OpenClipVitHandle", stub("openclip"))
    monkeypatch.setattr(ops, "ClipVitHandle", stub("clip"))
    p = perceptor.get_clip_perceptor("ViT-B-32", "cpu")
    perceptor.get_clip_perceptor("ViT-B/32", "cpu")
    assert made["ViT-B-32"][0] == "openclip" and made["ViT-B/32"][0] == "clip"
    assert p.input_resolution == 224 and p.output_dim == 512 and p.text_cfg.gelu and p.CLIP_MEAN == (0.48145466, 0.4578275, 0.40821073)
    a, b = made["ViT-B-32"][1], made["ViT-B/32"][1]
    assert list(a) == list(b) and not torch.equal(a["proj"], b["proj"])


# ------------------------------------------------------------------------------------------------ checkpoint adapters
def _reduced(name):
    """ViT-H-14's widths, heads and embedding size at one image block, two text blocks and a 1000-entry vocabulary (the adapters have
    no depth- or vocabulary-dependent branch)"""
    v, t = perceptor.clip_perceptor_config(name)
    vcfg = weights.OpenClipVitConfig(name, v.input_resolution, v.patch_size, v.width, 1, v.heads, v.output_dim)
    tcfg = weights.OpenClipTextConfig(name, 1000, 77, t.width, 2, t.heads, t.output_dim)
    return vcfg, tcfg


def _state_dict(vcfg, tcfg, seed):
    vis = weights.synthetic_clip_vit_params(vcfg, seed)
    txt = weights.synthetic_clip_text_params(tcfg, seed)
    sd = {"visual." + k: v.half() for k, v in vis.items()}
    sd.update({k: v.half() for k, v in txt.items()})
    sd["logit_scale"] = torch.tensor(4.6)
    sd["attn_mask"] = torch.zeros(77, 77)
    return sd, vis, txt


def test_openclip_state_dict_through_the_adapters():
    vcfg, tcfg = _reduced("ViT-H-14")
    sd, vis, txt = _state_dict(vcfg, tcfg, seed=4)
    # what reading the geometry off the shapes would give: 20 heads of 64 -- the rule the adapters must not use
    assert checkpoints.clip_config_from_state_dict(sd, "ViT-H-14").heads == 20 and vcfg.heads == 16
    got = checkpoints.clip_visual_from_openclip(sd, vcfg)
    assert list(got) == list(weights.clip_vit_param_shapes(vcfg))
    for k, t in got.items():
        assert t.dtype == torch.float32 and t.is_contiguous() and torch.equal(t, vis[k].half().float()), k
    got_t = checkpoints.clip_text_from_openclip(sd, tcfg)
    assert list(got_t) == list(weights.clip_text_param_shapes(tcfg))
    assert all(torch.equal(t, txt[k].half().float()) for k, t in got_t.items())
    # by name: the full configuration's geometry, so the one-block state dict is short of block 1 -- and the adapter says so
    with pytest.raises(KeyError, match=r"transformer\.resblocks\.1\.ln_1\.weight"):
        checkpoints.clip_visual_from_openclip(sd, "ViT-H-14")
    with pytest.raises(ValueError, match=r"token_embedding\.weight"):
        checkpoints.clip_text_from_openclip(sd, "ViT-H-14")
    with pytest.raises(KeyError, match="unknown OpenCLIP model"):
        checkpoints.clip_visual_from_openclip(sd, "ViT-B/32")
    # a missing tensor and a mis-shaped one are named, on both sides
    with pytest.raises(KeyError, match="positional_embedding"):
        checkpoints.clip_visual_from_openclip({k: v for k, v in sd.items() if k != "visual.positional_embedding"}, vcfg)
    with pytest.raises(KeyError, match="text_projection"):
        checkpoints.clip_text_from_openclip({k: v for k, v in sd.items() if k != "text_projection"}, tcfg)
    bad = dict(sd)
    bad["visual.transformer.resblocks.0.attn.in_proj_weight"] = torch.zeros(3 * 1024, 1024)
    with pytest.raises(ValueError, match=r"attn\.in_proj_weight"):
        checkpoints.clip_visual_from_openclip(bad, vcfg)
    bad = dict(sd)
    bad["text_projection"] = torch.zeros(512, 512)
    with pytest.raises(ValueError, match="text_projection"):
        checkpoints.clip_text_from_openclip(bad, tcfg)


def test_full_depth_names_by_meta_tensors():
    """the full 32-block shape list through the adapter without its bytes"""
    v, _ = perceptor.clip_perceptor_config("ViT-H-14")
    sd = {"visual." + k: torch.empty(s, device="meta") for k, s in weights.clip_vit_param_shapes(v).items()}
    with pytest.raises(KeyError, match=r"transformer\.resblocks\.31\.mlp\.c_proj\.bias"):
        checkpoints.clip_visual_from_openclip({k: t for k, t in sd.items() if k != "visual.transformer.resblocks.31.mlp.c_proj.bias"}, "ViT-H-14")


# ------------------------------------------------------------------------------------------------ front end
def test_front_end_sizes_the_cutout_table_for_vit_h_14(tmp_path):
    """`--clip_models ViT-H-14` through apply_settings / do_init with CPU stand-ins whose geometry is the product's own lookup"""
    from test_frontend import _TextPerceptor, _factories
    from pixray_amd import frontend as fe
    made, sizes = [], []
    parts = _factories(2)
    tiny = weights.CLIP_CONFIGS["tiny-B/32"]

    def perceptor_factory(name, index):
        cfg, text_cfg = perceptor.clip_perceptor_config(name)        # KeyError for a name the package does not know
        assert text_cfg is not None and text_cfg.output_dim == cfg.output_dim
        p = _TextPerceptor(tiny, weights.synthetic_clip_vit_params(tiny, 1 + index))
        p.input_resolution = cfg.input_resolution
        made.append(name)
        return p

    def cutouts_factory(size, index):
        sizes.append(size)
        return parts["cutouts_factory"](size, index)

    run = fe.Run()
    s = fe.apply_settings(["--clip_models", "ViT-H-14,ViT-B-16", "--drawer", "fast_pixel", "--prompts", "a red square", "--size", "64", "48",
                           "--pixel_size", "8", "6", "--num_cuts", "2", "--iterations", "2", "--outdir", str(tmp_path / "out"),
                           "--vector_prompts", "none"], run=run)
    assert s.clip_models == ["ViT-H-14", "ViT-B-16"]
    session = fe.do_init(s, run, perceptor_factory=perceptor_factory, cutouts_factory=cutouts_factory,
                         prompt_factory=parts["prompt_factory"], device="cpu")
    assert made == ["ViT-H-14", "ViT-B-16"] and sizes == [224]
    assert session.cutoutSizeTable == {"ViT-H-14": 224, "ViT-B-16": 224}


def test_quality_presets_are_unchanged():
    from pixray_amd import frontend as fe
    for table in fe.PERCEPTOR_TABLES.values():
        for names in table.values():
            assert not set(names if not isinstance(names, str) else names.split(",")) & set(weights.OPENCLIP_CONFIGS)


# ------------------------------------------------------------------------------------------------ the weight packs' head padding
needs_emu = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") or shutil.which("make") is None,
                               reason="needs the ROCm host clang++ and make to build tools/hipemu")


def pad_heads_check(device, stream=0):
    """the runner's own padding code (prx_k_vit_pad_heads: what prx_vit_tower_create runs on every block) on a random in_proj / out_proj
    at width 640 with 8 heads of 80: the padded packs equal the unpadded ones on the 80 live rows (columns) of every head and are
    exactly 0 on the 16 pad rows (columns)"""
    from pixray_amd._lib import call
    W, heads, hd, hp = 640, 8, 80, 96
    g = torch.Generator().manual_seed(3)
    w_in = torch.randn(3 * W, W, generator=g).to(device)
    w_out = torch.randn(W, W, generator=g).to(device)
    p_in = torch.full((3 * heads * hp, W), float("nan"), device=device)
    p_out = torch.full((W, heads * hp), float("nan"), device=device)
    call("prx_k_vit_pad_heads", w_in, p_in, w_out, p_out, W, heads, hd, hp, stream)
    if device != "cpu":
        torch.cuda.synchronize()
    a = p_in.reshape(3, heads, hp, W).cpu()
    assert torch.equal(a[:, :, :hd], w_in.reshape(3, heads, hd, W).cpu()) and (a[:, :, hd:] == 0).all()
    b = p_out.reshape(W, heads, hp).cpu()
    assert torch.equal(b[:, :, :hd], w_out.reshape(W, heads, hd).cpu()) and (b[:, :, hd:] == 0).all()


@needs_emu
def test_padded_pack_equals_the_unpadded_one_on_live_rows_and_is_zero_on_pad_rows():
    with _emu.enable():
        pad_heads_check("cpu")
