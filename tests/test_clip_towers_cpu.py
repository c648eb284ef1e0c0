"""The three CLIP perceptors `clip.available_models()` lists beyond the first six -- RN50x16, RN50x64, ViT-L/14@336px -- without a
device: the names resolve to the published geometries, the parameter shape lists are the OpenAI state dicts', the checkpoint adapters
return the tensors in ABI order and name what is missing or mis-shaped, the front end sizes the cutout tables from the towers'
resolutions, and the GEMM planner takes every product of the two new ModifiedResNets at full batch without an error (the row-streaming
kernels only where an instance exists)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from pixray_amd import checkpoints, perceptor, weights  # noqa: E402

NEW = ("RN50x16", "RN50x64", "ViT-L/14@336px")


# ------------------------------------------------------------------------------------------------ names and shapes
def test_the_three_names_resolve_to_the_published_geometries():
    """the numbers of OpenAI's published models (clip/model.py build_model reads them off the checkpoints)"""
    r16, t16 = perceptor.clip_perceptor_config("RN50x16")
    assert isinstance(r16, weights.ClipResNetConfig)
    assert (r16.input_resolution, r16.width, tuple(r16.layers), r16.heads, r16.output_dim) == (384, 96, (6, 8, 18, 8), 48, 768)
    assert (r16.embed_dim, r16.final_grid) == (3072, 12)
    assert (t16.width, t16.heads, t16.layers, t16.output_dim, t16.context_length, t16.vocab_size) == (768, 12, 12, 768, 77, 49408)
    r64, t64 = perceptor.clip_perceptor_config("RN50x64")
    assert isinstance(r64, weights.ClipResNetConfig)
    assert (r64.input_resolution, r64.width, tuple(r64.layers), r64.heads, r64.output_dim) == (448, 128, (3, 15, 36, 10), 64, 1024)
    assert (r64.embed_dim, r64.final_grid) == (4096, 14)
    assert (t64.width, t64.heads, t64.layers, t64.output_dim, t64.context_length, t64.vocab_size) == (1024, 16, 12, 1024, 77, 49408)
    v, tv = perceptor.clip_perceptor_config("ViT-L/14@336px")
    assert isinstance(v, weights.ClipVitConfig)
    assert (v.input_resolution, v.patch_size, v.width, v.layers, v.heads, v.output_dim, v.tokens) == (336, 14, 1024, 24, 16, 768, 577)
    assert (tv.width, tv.heads, tv.layers, tv.output_dim, tv.context_length, tv.vocab_size) == (768, 12, 12, 768, 77, 49408)
    for name in NEW:      # the three tables the issue names
        assert name in weights.CLIP_TEXT_CONFIGS and (name in weights.CLIP_CONFIGS) != (name in weights.CLIP_RESNET_CONFIGS)
    # the attention pools and every ViT head have head dim 64 (the attention kernels' contract)
    assert r16.embed_dim == 64 * r16.heads and r64.embed_dim == 64 * r64.heads and v.width == 64 * v.heads


def test_an_unknown_name_lists_the_supported_ones():
    with pytest.raises(KeyError, match="unknown / unsupported perceptor") as e:
        perceptor.clip_perceptor_config("RN50x128")
    for name in NEW + ("RN50", "RN101", "RN50x4", "ViT-B/32", "ViT-B/16", "ViT-L/14"):
        assert repr(name) in str(e.value), name
    with pytest.raises(ValueError, match="no text side"):                 # the refusal stays a refusal
        perceptor.clip_perceptor_config("SIMCLR_VITS16")


def test_parameter_shape_lists():
    sh = weights.clip_vit_param_shapes(weights.CLIP_CONFIGS["ViT-L/14@336px"])
    assert sh["positional_embedding"] == (577, 1024) and sh["conv1.weight"] == (1024, 3, 14, 14) and sh["proj"] == (1024, 768)
    assert len(sh) == 5 + 12 * 24 + 3
    for name, pos, stem, cproj, blocks in (("RN50x16", (145, 3072), (48, 3, 3, 3), (768, 3072), 40),
                                           ("RN50x64", (197, 4096), (64, 3, 3, 3), (1024, 4096), 64)):
        cfg = weights.CLIP_RESNET_CONFIGS[name]
        sh = weights.clip_resnet_param_shapes(cfg)
        assert sh["attnpool.positional_embedding"] == pos and sh["conv1.weight"] == stem and sh["attnpool.c_proj.weight"] == cproj
        assert sum(cfg.layers) == blocks
        # 3 stem convs, 3 per block and one downsample per layer, each with 4 BatchNorm tensors; 9 attention-pool tensors
        assert len(sh) == 5 * (3 + 3 * blocks + 4) + 9
        w = cfg.width
        assert sh["layer1.0.conv1.weight"] == (w, w, 1, 1) and sh["layer1.0.downsample.0.weight"] == (4 * w, w, 1, 1)
        assert sh[f"layer4.{cfg.layers[3] - 1}.conv3.weight"] == (32 * w, 8 * w, 1, 1)
        assert sh["layer4.0.conv2.weight"] == (8 * w, 8 * w, 3, 3) and "layer4.1.downsample.0.weight" not in sh
    for name, proj in (("RN50x16", (768, 768)), ("RN50x64", (1024, 1024)), ("ViT-L/14@336px", (768, 768))):
        tsh = weights.clip_text_param_shapes(weights.CLIP_TEXT_CONFIGS[name])
        assert tsh["text_projection"] == proj and tsh["token_embedding.weight"] == (49408, proj[0]) and tsh["positional_embedding"] == (77, proj[0])


def _reduced(cfg):
    """the same architecture at depth (1, 1, 1, 1) / one block: every KIND of tensor, a fraction of the bytes"""
    if isinstance(cfg, weights.ClipResNetConfig):
        return weights.ClipResNetConfig(cfg.name, cfg.input_resolution, cfg.width, (1, 1, 1, 1), cfg.heads, cfg.output_dim)
    return weights.ClipVitConfig(cfg.name, cfg.input_resolution, cfg.patch_size, cfg.width, 1, cfg.heads, cfg.output_dim)


def test_synthesis_and_fold_work_at_the_new_widths():
    """synthetic weights, the shape list and the BatchNorm fold at widths 96 and 128 (one block per layer: the code has no
    depth-dependent branch beyond the loop).  The fold is checked against an explicit eval-mode BatchNorm on one convolution."""
    for name in ("RN50x16", "RN50x64"):
        cfg = _reduced(weights.CLIP_RESNET_CONFIGS[name])
        p = weights.synthetic_clip_resnet_params(cfg, seed=1)
        assert {k: tuple(v.shape) for k, v in p.items()} == dict(weights.clip_resnet_param_shapes(cfg))
        f = weights.fold_clip_resnet_params(cfg, p)
        w = cfg.width
        assert f["stem1.weight"].shape == (w // 2, 3, 3, 3) and f["layer4.0.c3.weight"].shape == (32 * w, 8 * w, 1, 1)
        assert f["attnpool.in_proj_weight"].shape == (3 * 32 * w, 32 * w) and f["attnpool.c_proj.weight"].shape == (cfg.output_dim, 32 * w)
        assert len(f) == 2 * (3 + 3 * 4 + 4) + 5
        x = torch.randn(2, w, 5, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
        y = torch.nn.functional.conv2d(x, p["layer1.0.conv1.weight"].double())
        y = torch.nn.functional.batch_norm(y, p["layer1.0.bn1.running_mean"].double(), p["layer1.0.bn1.running_var"].double(),
                                           p["layer1.0.bn1.weight"].double(), p["layer1.0.bn1.bias"].double(), False, 0.0, 1e-5)
        z = torch.nn.functional.conv2d(x, f["layer1.0.c1.weight"].double(), f["layer1.0.c1.bias"].double())
        assert float((y - z).abs().max()) < 1e-5 * float(y.abs().max())


# ------------------------------------------------------------------------------------------------ checkpoint adapters
def _openai_state_dict(vcfg, tcfg, seed):
    """an OpenAI-style state dict (clip.load(name).state_dict()): `visual.*` + the un-prefixed text side + the scalars that ride along;
    fp16 like the published archives, BatchNorm counters included"""
    resnet = isinstance(vcfg, weights.ClipResNetConfig)
    vis = weights.synthetic_clip_resnet_params(vcfg, seed) if resnet else weights.synthetic_clip_vit_params(vcfg, seed)
    sd = {"visual." + k: v.half() for k, v in vis.items()}
    if resnet:
        for k in list(vis):
            if k.endswith("running_var"):
                sd["visual." + k[:-len("running_var")] + "num_batches_tracked"] = torch.tensor(7)
    txt = weights.synthetic_clip_text_params(tcfg, seed)
    sd.update({k: v.half() for k, v in txt.items()})
    sd["logit_scale"] = torch.tensor(4.6)
    sd["input_resolution"] = torch.tensor(vcfg.input_resolution)
    sd["context_length"] = torch.tensor(tcfg.context_length)
    sd["vocab_size"] = torch.tensor(tcfg.vocab_size)
    return sd, vis, txt


@pytest.mark.parametrize("name", NEW)
def test_openai_state_dict_through_the_adapters(name, tmp_path):
    """a synthetic OpenAI-style state dict of each architecture (real widths, resolution, heads and embedding size; one block per
    ResNet layer / one ViT block and a two-block text side, a 1000-entry vocabulary: the adapters have no depth- or vocabulary-dependent
    branch) -> the geometry read off the shapes, the tensors in ABI order as fp32, the pickled file through the archive reader;
    one tensor removed -> KeyError naming it; one mis-shaped -> ValueError naming it"""
    full_v, full_t = perceptor.clip_perceptor_config(name)
    vcfg = _reduced(full_v)
    tcfg = weights.ClipTextConfig(name, 1000, 77, full_t.width, 2, full_t.heads, full_t.output_dim)
    sd, vis, txt = _openai_state_dict(vcfg, tcfg, seed=4)
    assert checkpoints.clip_config_from_state_dict(sd, name) == vcfg
    assert checkpoints.clip_text_config_from_state_dict(sd, name) == tcfg
    resnet = isinstance(vcfg, weights.ClipResNetConfig)
    shapes = weights.clip_resnet_param_shapes(vcfg) if resnet else weights.clip_vit_param_shapes(vcfg)
    got = checkpoints.clip_visual_from_openai(sd, vcfg)
    assert list(got) == list(shapes)
    for k, t in got.items():
        assert t.dtype == torch.float32 and t.is_contiguous() and torch.equal(t, vis[k].half().float()), k
    got_t = checkpoints.clip_text_from_openai(sd, tcfg)
    assert list(got_t) == list(weights.clip_text_param_shapes(tcfg))
    assert all(torch.equal(t, txt[k].half().float()) for k, t in got_t.items())
    if resnet:          # what the runner's handle does with them: the fold takes the adapter's output as it is
        assert len(weights.fold_clip_resnet_params(vcfg, got)) == 2 * (3 + 3 * 4 + 4) + 5
    # the file form (clip.load falls back to a pickled state dict when the file is no TorchScript archive)
    path = str(tmp_path / "model.pt")
    torch.save(sd, path)
    back = checkpoints.clip_state_dict_from_archive(path)
    assert set(back) == set(sd) and checkpoints.clip_config_from_state_dict(back, name) == vcfg
    # a missing tensor, visual and text side, is named
    gone_v = "visual." + ("attnpool.c_proj.weight" if resnet else "positional_embedding")
    with pytest.raises(KeyError, match=gone_v[len("visual."):].replace(".", r"\.")):
        checkpoints.clip_visual_from_openai({k: v for k, v in sd.items() if k != gone_v}, vcfg)
    if resnet:
        with pytest.raises(KeyError, match=r"layer3\.0\.bn2\.running_var"):
            checkpoints.clip_visual_from_openai({k: v for k, v in sd.items() if k != "visual.layer3.0.bn2.running_var"}, vcfg)
    with pytest.raises(KeyError, match="text_projection"):
        checkpoints.clip_text_from_openai({k: v for k, v in sd.items() if k != "text_projection"}, tcfg)
    # a mis-shaped one: the stem of the other width / the 257-token table of ViT-L/14
    bad = dict(sd)
    bad_key = "visual.conv1.weight" if resnet else "visual.positional_embedding"
    bad[bad_key] = torch.zeros(32, 3, 3, 3) if resnet else torch.zeros(257, 1024)
    with pytest.raises(ValueError, match=bad_key[len("visual."):].replace(".", r"\.")):
        checkpoints.clip_visual_from_openai(bad, vcfg)
    bad = dict(sd)
    bad["text_projection"] = torch.zeros(512, 512)
    with pytest.raises(ValueError, match="text_projection"):
        checkpoints.clip_text_from_openai(bad, tcfg)


def test_full_depth_shape_lists_are_checked_by_the_adapters():
    """the full-depth towers through `_check` without their bytes (meta tensors): names, order and count of RN50x16's 644 and RN50x64's
    1004 visual tensors, and the first missing block is named"""
    for name in ("RN50x16", "RN50x64"):
        cfg = weights.CLIP_RESNET_CONFIGS[name]
        shapes = weights.clip_resnet_param_shapes(cfg)
        sd = {"visual." + k: torch.empty(s, device="meta") for k, s in shapes.items()}
        assert checkpoints.clip_config_from_state_dict(sd, name) == cfg
        last = f"layer3.{cfg.layers[2] - 1}.conv2.weight"
        with pytest.raises(KeyError, match=last.replace(".", r"\.")):
            checkpoints.clip_visual_from_openai({k: v for k, v in sd.items() if k != "visual." + last}, cfg)
    assert len(weights.clip_resnet_param_shapes(weights.CLIP_RESNET_CONFIGS["RN50x16"])) == 644
    assert len(weights.clip_resnet_param_shapes(weights.CLIP_RESNET_CONFIGS["RN50x64"])) == 1004


# ------------------------------------------------------------------------------------------------ front end
def test_front_end_sizes_the_cutout_tables_from_the_new_towers(tmp_path):
    """`--clip_models "RN50x16,ViT-L/14@336px"` through apply_settings / do_init with CPU stand-ins whose geometry is the product's own
    lookup (perceptor.clip_perceptor_config): two cutout tables, 384 and 336"""
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
    run.settings = dict(drawer="fast_pixel", prompts="a red square", clip_models="RN50x16,ViT-L/14@336px", size=[64, 48], pixel_size=[8, 6],
                        num_cuts=2, iterations=2, outdir=str(tmp_path / "out"), seed="42", skip_args=True, vector_prompts="none")
    s = fe.apply_settings(run=run)
    assert s.clip_models == ["RN50x16", "ViT-L/14@336px"]
    session = fe.do_init(s, run, perceptor_factory=perceptor_factory, cutouts_factory=cutouts_factory,
                         prompt_factory=parts["prompt_factory"], device="cpu")
    assert made == ["RN50x16", "ViT-L/14@336px"] and set(sizes) == {384, 336} and len(sizes) == 2
    assert session.cutoutSizeTable == {"RN50x16": 384, "ViT-L/14@336px": 336}


def test_command_line_takes_the_names(tmp_path):
    """`python -m pixray_amd --clip_models RN50x16,ViT-L/14@336px ...` parses to the two names (the comma list of pixray.py:1898)"""
    from pixray_amd import frontend as fe
    run = fe.Run()
    s = fe.apply_settings(["--clip_models", "RN50x16,ViT-L/14@336px", "--drawer", "fast_pixel", "--size", "64", "48",
                           "--outdir", str(tmp_path / "out")], run=run)
    assert s.clip_models == ["RN50x16", "ViT-L/14@336px"] and s.size == [64, 48]
    for name in s.clip_models:
        perceptor.clip_perceptor_config(name)


# ------------------------------------------------------------------------------------------------ GEMM selection
def _resnet_products(cfg, n, lean):
    """every GEMM descriptor of the ModifiedResNet runner (csrc/resnet.hip forward and backward_a) for n cutouts, as
    (M, N, K, conv side or None, act, residual kind: 0 none / 1 fp32 / 2 the 16-bit stream)"""
    NONE, RELU, MULMASK, MASKPOST = 0, 3, 4, 5
    w, R = cfg.width, cfg.input_resolution
    res = 2 if lean else 1
    out = []
    S2 = R // 2
    out += [(n * S2 * S2, w // 2, 9 * (w // 2), S2, RELU, 0), (n * S2 * S2, w, 9 * (w // 2), S2, RELU, 0)]            # stem conv2, conv3
    out += [(n * S2 * S2, w // 2, 9 * w, S2, MULMASK, 0), (n * S2 * S2, w // 2, 9 * (w // 2), S2, MULMASK, 0)]       # ... their dgrads
    H, inpl = R // 4, w
    first = True
    for li, nb in enumerate(cfg.layers):
        p = w << li
        for b in range(nb):
            stride = 2 if (li > 0 and b == 0) else 1
            Ho = H // stride
            Min, Mout = n * H * H, n * Ho * Ho
            has_ds = stride > 1 or inpl != 4 * p
            out.append((Min, p, inpl, None, RELU, 0))                                     # conv1
            out.append((Min, p, 9 * p, H, RELU, 0))                                       # conv2
            if has_ds:
                out.append((Mout, 4 * p, inpl, None, NONE, 0))                            # downsample
            out.append((Mout, 4 * p, p, None, RELU, res))                                 # conv3 + identity
            out.append((Mout, p, 4 * p, None, NONE if stride > 1 else MULMASK, 0))        # conv3 dgrad
            out.append((Min, p, 9 * p, H, MULMASK, 0))                                    # conv2 dgrad
            if has_ds:
                out.append((Mout, inpl, 4 * p, None, NONE, 0))                            # downsample dgrad
            out.append((Min, inpl, p, None, NONE if first else MASKPOST, res))            # conv1 dgrad + identity gradient
            first = False
            inpl, H = 4 * p, Ho
    C, T = cfg.embed_dim, cfg.final_grid ** 2 + 1
    out += [(n * T, 3 * C, C, None, NONE, 0), (n, cfg.output_dim, C, None, NONE, 0), (n, C, cfg.output_dim, None, NONE, 0),
            (n * T, C, 3 * C, None, NONE, 0)]
    return out


@pytest.mark.parametrize("name", ["RN50x16", "RN50x64"])
def test_every_product_of_the_new_resnets_plans_onto_a_kernel_that_exists(name):
    """The launch planner (host code, no device) over every GEMM descriptor of RN50x16 / RN50x64 at 64 cutouts, half and bf16: each
    plans without an error.  The row-streaming kernels exist for slabs of 160 / 128 / 80 columns at K <= 320 (80 columns: K <= 640),
    with no activation or ReLU, the ReLU mask after a residual, or -- 80-column slabs only -- the mask without one; a row-streaming
    plan outside that list would meet no instance at launch.  Restated here from csrc/gemmrow_kernel.h, not read from it.  The
    row-streaming 3x3 convolutions have instances for RN50x4's channel counts only: none of these towers' convolutions may plan
    onto them."""
    import ctypes
    from pixray_amd import _lib
    lib = _lib.load()
    cfg = weights.CLIP_RESNET_CONFIGS[name]
    ROW, ROWCONV = 5, 6
    seen = set()
    for prec in ("fp16", "bf16"):
        for (M, N, K, side, act, res) in _resnet_products(cfg, 64, lean=(prec == "fp16")):
            g = _lib.GemmArgs(ctx=None)
            g.A, g.B, g.bias_n, g.out_bf16, g.aux, g.resid = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, (6 << 20 if res else None)
            g.M, g.N, g.K, g.lda, g.ldb, g.ldc_bf16, g.ldaux, g.ldr, g.alpha, g.act = M, N, K, K, K, N, N, N, 1.0, act
            g.f32 = {"bf16": 0, "fp16": 2}[prec]
            g.row16 = 1 if res == 2 else 0
            if side:
                g.a_mode, g.H, g.W, g.Cin, g.lda = 1, side, side, K // 9, K // 9
            plan = (ctypes.c_int * 9)()
            assert lib.prx_gemm_plan(None, ctypes.byref(g), 64 << 20, 256, plan) == 0, (M, N, K, side, act, res, _lib.last_error())
            for fam, bm, bn, splits in (tuple(plan[:4]), tuple(plan[5:9])):
                seen.add(fam)
                assert fam != ROWCONV, (M, N, K, side)
                if fam == ROW:
                    assert side is None and bn in (160, 128, 80) and N % bn == 0 and K % 8 == 0, (M, N, K, bn)
                    assert K <= 320 or (bn == 80 and K <= 640), (M, N, K, bn)
                    assert act in (0, 3) or (act == 5 and res) or (act == 4 and not res and bn == 80), (M, N, K, bn, act, res)
    assert ROW in seen or name == "RN50x16"      # RN50x64's 128-multiples take the 128-column slabs
