"""The OpenCLIP ConvNeXt perceptors without a device: the configuration table, the shape lists, the host-side fold (layer scale into
fc2, the convolutions as matrices in the runner's column orders) against the float64 restatement, the state-dict adapter and its error
messages, the capacity arithmetic, and the front end.

Every test here fails on a tree without the ConvNeXt names (`KeyError: unknown / unsupported perceptor 'convnext_base_w'`)."""
import dataclasses
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _convnext_ref  # noqa: E402
from pixray_amd import checkpoints, perceptor, weights  # noqa: E402

NAMES = ("convnext_base", "convnext_base_w", "convnext_base_w_320", "convnext_large_d", "convnext_large_d_320", "convnext_xxlarge")


# ------------------------------------------------------------------------------------------------ configurations
def test_config_table():
    """the six names resolve to the published geometry [UPSTREAM open_clip model_configs/convnext_*.json, timm convnext.py]"""
    want = {
        "convnext_base": (224, (3, 3, 27, 3), (128, 256, 512, 1024), 512, "linear", 1e-6, (512, 8, 12)),
        "convnext_base_w": (256, (3, 3, 27, 3), (128, 256, 512, 1024), 640, "linear", 1e-6, (640, 10, 12)),
        "convnext_base_w_320": (320, (3, 3, 27, 3), (128, 256, 512, 1024), 640, "linear", 1e-6, (640, 10, 12)),
        "convnext_large_d": (256, (3, 3, 27, 3), (192, 384, 768, 1536), 768, "mlp", 1e-6, (768, 12, 16)),
        "convnext_large_d_320": (320, (3, 3, 27, 3), (192, 384, 768, 1536), 768, "mlp", 1e-6, (768, 12, 16)),
        "convnext_xxlarge": (256, (3, 4, 30, 3), (384, 768, 1536, 3072), 1024, "linear", 1e-5, (1024, 16, 24)),
    }
    assert set(want) == set(NAMES)
    for name, (res, depths, dims, embed, proj, eps, text) in want.items():
        v, t = perceptor.clip_perceptor_config(name)
        assert isinstance(v, weights.ClipConvNextConfig) and v.name == name
        assert (v.input_resolution, tuple(v.depths), tuple(v.dims), v.output_dim, v.proj, v.ln_eps) == (res, depths, dims, embed, proj, eps)
        assert v.input_resolution % 32 == 0 and all(d % 8 == 0 for d in v.dims)          # what the runner asks of a geometry
        assert isinstance(t, weights.OpenClipTextConfig) and t.gelu
        assert (t.width, t.heads, t.layers) == text and t.output_dim == embed and t.width == 64 * t.heads
        assert (t.vocab_size, t.context_length) == (49408, 77)
    for name in ("tiny-cnx", "tiny-cnx-d"):
        v, t = perceptor.clip_perceptor_config(name)
        assert isinstance(v, weights.ClipConvNextConfig) and t.output_dim == v.output_dim == 128
    tiny, tiny_d = weights.CLIP_CONVNEXT_CONFIGS["tiny-cnx"], weights.CLIP_CONVNEXT_CONFIGS["tiny-cnx-d"]
    assert (tiny.input_resolution, tuple(tiny.depths), tuple(tiny.dims), tiny.proj) == (64, (1, 1, 2, 1), (64, 128, 256, 512), "linear")
    assert (tiny_d.input_resolution, tuple(tiny_d.depths), tuple(tiny_d.dims), tiny_d.proj) == (96, (1, 1, 1, 1), (96, 192, 384, 768), "mlp")


def test_shape_lists_and_counts():
    v = weights.CLIP_CONVNEXT_CONFIGS["convnext_base_w"]
    sh = weights.clip_convnext_param_shapes(v)
    assert list(sh)[:4] == ["trunk.stem.0.weight", "trunk.stem.0.bias", "trunk.stem.1.weight", "trunk.stem.1.bias"]
    assert sh["trunk.stem.0.weight"] == (128, 3, 4, 4) and sh["trunk.stages.1.downsample.1.weight"] == (256, 128, 2, 2)
    assert sh["trunk.stages.1.downsample.0.weight"] == (128,) and "trunk.stages.0.downsample.0.weight" not in sh
    assert sh["trunk.stages.2.blocks.26.conv_dw.weight"] == (512, 1, 7, 7) and sh["trunk.stages.2.blocks.26.gamma"] == (512,)
    assert sh["trunk.stages.3.blocks.2.mlp.fc1.weight"] == (4096, 1024) and sh["trunk.stages.3.blocks.2.mlp.fc2.weight"] == (1024, 4096)
    assert "trunk.stages.2.blocks.27.gamma" not in sh and sh["trunk.head.norm.weight"] == (1024,)
    assert list(sh)[-1] == "head.proj.weight" and sh["head.proj.weight"] == (640, 1024)
    assert len(sh) == 4 + 3 * 4 + 9 * 36 + 2 + 1
    d = weights.CLIP_CONVNEXT_CONFIGS["convnext_large_d"]
    shd = weights.clip_convnext_param_shapes(d)
    assert list(shd)[-3:] == ["head.mlp.fc1.weight", "head.mlp.fc1.bias", "head.mlp.fc2.weight"]
    assert shd["head.mlp.fc1.weight"] == (1536, 1536) and shd["head.mlp.fc2.weight"] == (768, 1536) and len(shd) == len(sh) + 2
    x = weights.clip_convnext_param_shapes(weights.CLIP_CONVNEXT_CONFIGS["convnext_xxlarge"])
    assert len(x) == 4 + 3 * 4 + 9 * 40 + 2 + 1 and x["trunk.stages.3.blocks.0.mlp.fc1.weight"] == (12288, 3072)
    # what the C ABI is handed: the layer scale folded away, 8 tensors per block
    folded = weights.fold_clip_convnext_params(weights.CLIP_CONVNEXT_CONFIGS["tiny-cnx"],
                                               weights.synthetic_clip_convnext_params(weights.CLIP_CONVNEXT_CONFIGS["tiny-cnx"], 0))
    assert len(folded) == 4 + 3 * 4 + 8 * 5 + 2 + 1 and not any("gamma" in k for k in folded)
    assert folded["stem.weight"].shape == (64, 48) and folded["stages.1.ds.weight"].shape == (128, 256) and folded["stages.0.blocks.0.dw.weight"].shape == (64, 49)
    with pytest.raises(ValueError, match="'linear' or 'mlp'"):
        weights.clip_convnext_param_shapes(dataclasses.replace(v, proj="attn"))


def test_synthetic_weights_keep_every_block_alive_and_half_finite():
    """gamma has a spread of order 1 (not timm's 1e-6 initialisation), and the deepest tower's residual stream stays far inside IEEE
    half's range under the stated scales: a 36-block stack of the block at width 64 on an 8 x 8 map, float32"""
    cfg = dataclasses.replace(weights.CLIP_CONVNEXT_CONFIGS["tiny-cnx"], depths=(36, 1, 1, 1))
    p = weights.synthetic_clip_convnext_params(cfg, 3)
    gam = torch.stack([p[f"trunk.stages.0.blocks.{b}.gamma"] for b in range(36)])
    assert 0.3 < float(gam.std()) < 0.7 and 0.3 < float(gam.mean()) < 0.7
    x = torch.randn(1, 64, 8, 8, generator=torch.Generator().manual_seed(0))
    for b in range(36):
        y = _convnext_ref.block(p, f"trunk.stages.0.blocks.{b}.", x, 1e-6)
        assert float((y - x).norm() / x.norm()) > 0.02, b          # every block moves the stream
        x = y
    assert torch.isfinite(x).all() and float(x.abs().max()) < 65504 / 64


# ------------------------------------------------------------------------------------------------ the fold
def _folded_forward(f, cfg, imgs):
    """the runner's arithmetic on the FOLDED tensors, in float64: the stem and the downsamples as matrix products in patchify's and
    space-to-depth's column orders, the depthwise filter from its [C, 49] form, no layer scale"""
    eps = cfg.ln_eps
    x = _convnext_ref.normalize(_convnext_ref.adjust_range(imgs))
    n, _, r, _ = x.shape
    g = r // 4
    a = x.view(n, 3, g, 4, g, 4).permute(0, 2, 4, 1, 3, 5).reshape(n, g, g, 48)                   # column (c, py, px)
    x = F.layer_norm(a @ f["stem.weight"].t() + f["stem.bias"], (cfg.dims[0],), f["stem.ln.weight"], f["stem.ln.bias"], eps)
    for i in range(4):
        c = cfg.dims[i]
        if i > 0:
            cp = cfg.dims[i - 1]
            h = F.layer_norm(x, (cp,), f[f"stages.{i}.ds.ln.weight"], f[f"stages.{i}.ds.ln.bias"], eps)
            g //= 2
            h = h.view(n, g, 2, g, 2, cp).permute(0, 1, 3, 2, 4, 5).reshape(n, g, g, 4 * cp)      # column (dy * 2 + dx) * C + c
            x = h @ f[f"stages.{i}.ds.weight"].t() + f[f"stages.{i}.ds.bias"]
        for b in range(cfg.depths[i]):
            k = f"stages.{i}.blocks.{b}."
            y = F.conv2d(x.permute(0, 3, 1, 2), f[k + "dw.weight"].view(c, 1, 7, 7), f[k + "dw.bias"], padding=3, groups=c).permute(0, 2, 3, 1)
            h = F.layer_norm(y, (c,), f[k + "ln.weight"], f[k + "ln.bias"], eps)
            h = _convnext_ref.gelu(h @ f[k + "fc1.weight"].t() + f[k + "fc1.bias"])
            x = x + h @ f[k + "fc2.weight"].t() + f[k + "fc2.bias"]
    h = F.layer_norm(x.mean(dim=(1, 2)), (cfg.dims[3],), f["head.ln.weight"], f["head.ln.bias"], eps)
    if cfg.proj == "linear":
        e = h @ f["head.proj.weight"].t()
    else:
        e = _convnext_ref.gelu(h @ f["head.fc1.weight"].t() + f["head.fc1.bias"]) @ f["head.fc2.weight"].t()
    return e / e.norm(dim=-1, keepdim=True)


@pytest.mark.parametrize("proj", ["linear", "mlp"])
def test_fold_identity_in_float64(proj):
    """one block per stage: the folded tensors in the runner's layouts give the restatement's embedding on the unfolded ones"""
    cfg = dataclasses.replace(weights.CLIP_CONVNEXT_CONFIGS["tiny-cnx"], depths=(1, 1, 1, 1), proj=proj)
    p = _convnext_ref.cast(weights.synthetic_clip_convnext_params(cfg, 7), torch.float64)
    folded = weights.fold_clip_convnext_params(cfg, p)
    assert all(t.dtype == torch.float32 for t in folded.values())
    f64 = {k: v.double() for k, v in folded.items()}
    imgs = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 1.2 - 0.1
    ref = _convnext_ref.encode_image(p, cfg, imgs)
    got = _folded_forward(f64, cfg, imgs)
    # the synthetic parameters are fp32 numbers, so everything but gamma * fc2 (rounded to fp32 once, 2^-24 relative) is carried over
    # exactly: unit-norm embeddings agree to a few fp32 roundings, evaluated in float64
    assert float((got - ref).abs().max()) < 1e-6, float((got - ref).abs().max())
    # the layer scale is live in the restatement: without it the embedding is another one
    nog = dict(p)
    nog["trunk.stages.1.blocks.0.gamma"] = torch.ones_like(p["trunk.stages.1.blocks.0.gamma"])
    assert float((_convnext_ref.encode_image(nog, cfg, imgs) - ref).abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------ checkpoint adapter
def _state_dict(vcfg, tcfg, seed):
    vis = weights.synthetic_clip_convnext_params(vcfg, seed)
    txt = weights.synthetic_clip_text_params(tcfg, seed)
    sd = {"visual." + k: v.half() for k, v in vis.items()}
    sd.update({k: v.half() for k, v in txt.items()})
    sd["logit_scale"] = torch.tensor(4.6)
    sd["attn_mask"] = torch.zeros(77, 77)
    return sd, vis, txt


def test_openclip_state_dict_through_the_adapter():
    v, t = perceptor.clip_perceptor_config("convnext_large_d")
    vcfg = dataclasses.replace(v, depths=(1, 1, 1, 1))                     # the adapter has no depth-dependent branch
    tcfg = weights.OpenClipTextConfig(v.name, 1000, 77, t.width, 2, t.heads, t.output_dim)
    sd, vis, txt = _state_dict(vcfg, tcfg, seed=4)
    got, got_t = checkpoints.clip_convnext_from_openclip(sd, vcfg, tcfg)
    assert list(got) == list(weights.clip_convnext_param_shapes(vcfg)) and list(got_t) == list(weights.clip_text_param_shapes(tcfg))
    for k, x in got.items():
        assert x.dtype == torch.float32 and x.is_contiguous() and torch.equal(x, vis[k].half().float()), k
    assert all(torch.equal(x, txt[k].half().float()) for k, x in got_t.items())
    # by name: the full configuration's geometry, so the one-block state dict is short of block 1 -- and the adapter says so
    with pytest.raises(KeyError, match=r"trunk\.stages\.0\.blocks\.1\.gamma"):
        checkpoints.clip_convnext_from_openclip(sd, "convnext_large_d")
    with pytest.raises(KeyError, match="unknown OpenCLIP ConvNeXt model"):
        checkpoints.clip_convnext_from_openclip(sd, "ViT-B-32")
    with pytest.raises(KeyError, match=r"head\.mlp\.fc2\.weight"):
        checkpoints.clip_convnext_from_openclip({k: x for k, x in sd.items() if k != "visual.head.mlp.fc2.weight"}, vcfg, tcfg)
    with pytest.raises(KeyError, match="text_projection"):
        checkpoints.clip_convnext_from_openclip({k: x for k, x in sd.items() if k != "text_projection"}, vcfg, tcfg)
    bad = dict(sd)
    bad["visual.trunk.stages.2.blocks.0.conv_dw.weight"] = torch.zeros(768, 1, 3, 3)
    with pytest.raises(ValueError, match=r"conv_dw\.weight"):
        checkpoints.clip_convnext_from_openclip(bad, vcfg, tcfg)
    # a linear-head state dict against an mlp configuration
    with pytest.raises(KeyError, match=r"head\.proj\.weight"):
        checkpoints.clip_convnext_from_openclip(sd, dataclasses.replace(vcfg, proj="linear"), tcfg)


def test_full_depth_names_by_meta_tensors():
    """the full 40-block shape list of convnext_xxlarge through the adapter without its bytes"""
    v, t = perceptor.clip_perceptor_config("convnext_xxlarge")
    sd = {"visual." + k: torch.empty(s, device="meta") for k, s in weights.clip_convnext_param_shapes(v).items()}
    with pytest.raises(KeyError, match=r"trunk\.stages\.2\.blocks\.29\.mlp\.fc2\.bias"):
        checkpoints.clip_convnext_from_openclip({k: x for k, x in sd.items() if k != "visual.trunk.stages.2.blocks.29.mlp.fc2.bias"}, "convnext_xxlarge")


# ------------------------------------------------------------------------------------------------ capacity
def test_activation_bytes_per_cutout():
    """the figures include/prx.h states, and the GELU pre-activations' share of them"""
    v = weights.CLIP_CONVNEXT_CONFIGS["convnext_base_w"]
    pre = sum(v.depths[i] * 4 * (64 >> i) ** 2 * v.dims[i] * 2 for i in range(4))
    assert pre == 48758784                                                  # 46.5 MiB in 16 bits
    assert weights.clip_convnext_activation_bytes(v, "fp16") == weights.clip_convnext_activation_bytes(v, "bf16") == 95181104
    assert weights.clip_convnext_activation_bytes(v, "f32") == 163087760
    assert weights.clip_convnext_activation_bytes(weights.CLIP_CONVNEXT_CONFIGS["convnext_xxlarge"], "fp16") == 302327856


def test_convnext_kernels_have_no_scratch():
    """the depthwise kernel keeps 4 x 8 accumulators and a filter column's 7 x 8 taps in registers; with its filter-column loop unrolled
    hipcc hoisted every LDS read, took 256 registers and spilled 1.8 KB per lane with all parity tests green.  The compiler's resource
    figures are the guard (the helper of tests/test_host_logic.py): no kernel of convnext.hip may use scratch."""
    from test_host_logic import _kernel_scratch
    kernels = _kernel_scratch(os.path.join(os.path.dirname(HERE), "pixray_amd", "csrc", "convnext.hip"))
    assert len([n for n, _ in kernels if "cnx_dwconv_kernel" in n]) == 3 and len(kernels) >= 20, kernels
    bad = [(n, s) for n, s in kernels if s != 0]
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ names and the front end
def test_an_unknown_name_lists_the_new_ones():
    with pytest.raises(KeyError, match="unknown / unsupported perceptor") as e:
        perceptor.clip_perceptor_config("convnext_small")
    for name in NAMES + ("ViT-B/32", "ViT-H-14", "RN50", "SLIP_VITB16"):
        assert repr(name) in str(e.value), name


def test_the_perceptor_is_built_on_the_convnext_handle_with_synthetic_weights(monkeypatch, capsys):
    from pixray_amd import ops
    made = {}

    def make(cfg, params, mb, dev, precision=None):
        made[cfg.name] = params
        return object()
    monkeypatch.setattr(ops, "ClipConvNextHandle", make)
    p = perceptor.get_clip_perceptor("convnext_base_w", "cpu", seed=3)
    assert "synthetic" in capsys.readouterr().out
    assert p.input_resolution == 256 and p.output_dim == 640 and p.text_cfg.gelu and p.CLIP_MEAN == (0.48145466, 0.4578275, 0.40821073)
    assert list(made["convnext_base_w"]) == list(weights.clip_convnext_param_shapes(p.cfg))
    assert float(made["convnext_base_w"]["trunk.stages.2.blocks.26.gamma"].std()) > 0.2


def test_front_end_sizes_the_cutout_table_without_a_device(tmp_path):
    """`--clip_models convnext_base_w,convnext_large_d_320` through apply_settings / do_init with CPU stand-ins whose geometry is the
    product's own lookup: cutouts of 256 and 320"""
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
    s = fe.apply_settings(["--clip_models", "convnext_base_w,convnext_large_d_320", "--drawer", "fast_pixel", "--prompts", "a red square",
                           "--size", "64", "48", "--pixel_size", "8", "6", "--num_cuts", "2", "--iterations", "2", "--outdir", str(tmp_path / "out"),
                           "--vector_prompts", "none"], run=run)
    assert s.clip_models == ["convnext_base_w", "convnext_large_d_320"]
    session = fe.do_init(s, run, perceptor_factory=perceptor_factory, cutouts_factory=cutouts_factory,
                         prompt_factory=parts["prompt_factory"], device="cpu")
    assert made == ["convnext_base_w", "convnext_large_d_320"] and sorted(sizes) == [256, 320]
    assert session.cutoutSizeTable == {"convnext_base_w": 256, "convnext_large_d_320": 320}


def test_quality_presets_are_unchanged():
    from pixray_amd import frontend as fe
    for table in fe.PERCEPTOR_TABLES.values():
        for names in table.values():
            assert not set(names if not isinstance(names, str) else names.split(",")) & set(weights.CLIP_CONVNEXT_CONFIGS)
