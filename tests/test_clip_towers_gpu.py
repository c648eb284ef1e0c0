"""RN50x16, RN50x64 and ViT-L/14@336px on the device: the ModifiedResNet runner at widths 96 and 128 (stem 48 / 64, the bottlenecks,
the attention pool) in all three operand modes against the oracle, the general-T attention at the pools' real token counts and at
512 < T <= 640 through both kernel families against float64 softmax attention, a reduced 577-token ViT tower against the oracle,
every new tower once at its real geometry, and one RN50x16 run through the settings front end.

The case functions and their gates are the existing ones -- tests/test_path_gpu.py (half / bf16 towers), tests/test_f32_mode_gpu.py
(exact mode), tests/test_kernels_half_gpu.py (attention) -- called on the new geometries.  Two of the reduced-ResNet cases restate their
comparison here and say why (_f32_case: a ReLU kink 2.1e-7 from zero in the test inputs; _bf16_case: the two min / max entries of the
renormalisation are checked by an identity instead of through the norm of the whole gradient)."""
import contextlib
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu

import test_f32_mode_gpu as tf  # noqa: E402
import test_kernels_half_gpu as th  # noqa: E402
import test_path_gpu as tp  # noqa: E402
from pixray_amd import _lib, ops, perceptor, weights  # noqa: E402

DEV = "cuda"

# reduced towers at the new widths: stem 48 / 64, planes 96 .. 768 / 128 .. 1024 (embed 3072 / 4096, 48 / 64 heads), a stride-1 and three
# stride-2 first blocks, a block without a downsample branch, a 3 x 3 final grid (10 pool tokens)
weights.CLIP_RESNET_CONFIGS.setdefault("test-RN96", weights.ClipResNetConfig("test-RN96", 96, 96, (1, 2, 1, 1), 48, 64))
weights.CLIP_RESNET_CONFIGS.setdefault("test-RN128", weights.ClipResNetConfig("test-RN128", 96, 128, (1, 2, 1, 1), 64, 64))
# the 577 tokens of ViT-L/14@336px on a 2-layer, 2-head tower
weights.CLIP_CONFIGS.setdefault("test-L/14@336", weights.ClipVitConfig("test-L/14@336", 336, 14, 128, 2, 2, 64))

ROUTE_BLK, ROUTE_TILES = 0, 1      # prx_mha_route (include/prx.h): the workgroup-per-(image, head) family / the 64-token tile kernels


@contextlib.contextmanager
def mha_route(route):
    """the attention family of the general-T calls inside the block (None: the default rule)"""
    lib = _lib.load()
    before = lib.prx_mha_route(-1 if route is None else route)
    try:
        yield
    finally:
        lib.prx_mha_route(before)


# ------------------------------------------------------------------------------------------------ reduced ResNets
def _resnet_inputs(cfg, n):
    """weights and inputs of the `tiny-RN` tests (weight seed 3, input seed 17, smooth cutouts + 5 % noise)"""
    p = weights.synthetic_clip_resnet_params(cfg, seed=3)
    g = torch.Generator().manual_seed(17)
    R = cfg.input_resolution
    low = torch.rand(n, 3, R // 8, R // 8, generator=g)
    cut = F.interpolate(low, size=(R, R), mode="bilinear", align_corners=False) + 0.05 * torch.randn(n, 3, R, R, generator=g)
    return p, cut, torch.randn(n, cfg.output_dim, generator=g)


class _KinkRelu(torch.autograd.Function):
    """ReLU whose backward mask is inverted on the listed units (flat indices of this call's input); records the units whose input lies
    within `tau` of zero"""
    @staticmethod
    def forward(ctx, x, call, flips, tau, near):
        mask = x > 0
        if tau > 0:
            for i in (x.abs() < tau).flatten().nonzero().flatten().tolist():
                near.append((abs(float(x.flatten()[i])), call, i))
        for (c, i) in flips:
            if c == call:
                mask.view(-1)[i] = ~mask.view(-1)[i]
        ctx.save_for_backward(mask)
        return x.clamp_min(0)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None, None, None


def _oracle_f64(cfg, p, cut, ge, flips=(), tau=0.0):
    """float64 oracle embeddings and d/dcutouts; `flips`: (ReLU call number, flat unit index) pairs whose mask is inverted; also returns
    the units within `tau` of a ReLU's kink, nearest first"""
    from oracle import clip_resnet_ref
    near, calls = [], [0]

    def relu(x):
        calls[0] += 1
        return _KinkRelu.apply(x, calls[0], tuple(flips), tau, near)
    pp = {k: v.double() for k, v in p.items()}
    cr = cut.double().clone().requires_grad_(True)
    orig = clip_resnet_ref.F.relu
    clip_resnet_ref.F.relu = relu
    try:
        e = clip_resnet_ref.encode_image(pp, cr, layers=cfg.layers, heads=cfg.heads)
        (g,) = torch.autograd.grad(e, cr, ge.double())
    finally:
        clip_resnet_ref.F.relu = orig
    return e.detach(), g.detach(), sorted(near)


KINK_TAU = 1e-6      # a ReLU input this close to zero (the inputs are O(1)) is on either side of the kink in fp32: the exact mode's embeddings
                     # themselves sit 5e-7 from the float64 oracle's (measured, both widths), i.e. its activations carry that much round-off


def _f32_case(name, n):
    """test_f32_mode_gpu.test_clip_resnet_f32_vs_oracle with its gates (embeddings 1e-4; gradient max(3 x the fp32 oracle's own distance
    from the float64 oracle, 1e-4)) and one mend.  The gradient of a ReLU network jumps where a pre-activation crosses zero, and on the
    `tiny-RN` tests' inputs the width-96 tower has one unit 2.1e-7 above zero (cutout 2, a 768-channel 12 x 12 map; the float64 oracle
    says so, no device involved): fp32 round-off puts it at or below zero, its mask flips, and d/dcutouts moves by 2.21e-4 of its norm
    around pixels (3, 61..67) of that cutout -- measured on the MI355X and bit for bit on the CPU emulation of the kernels, and
    reproduced in the float64 oracle by inverting that one mask (2.2101e-4, the same pixels).  So where the plain comparison misses
    the gate, the reference may take the other side of kinks that lie within KINK_TAU of zero (at most 6 of them: the masks are
    chosen by the additive effect of each flip, then the oracle is run again with the chosen masks and the SAME gate applies to it).
    A wrong kernel is not excused: a flip moves the gradient only inside one unit's receptive field of one cutout."""
    cfg = weights.CLIP_RESNET_CONFIGS[name]
    p, cut, ge = _resnet_inputs(cfg, n)
    h = ops.ClipResNetHandle(cfg, p, max_batch=4, device=DEV, precision="f32")
    cd = cut.to(DEV).requires_grad_(True)
    emb = ops.clip_encode_image(cd, h)
    (gd,) = torch.autograd.grad(emb, cd, ge.to(DEV))
    gd = gd.detach().cpu().double()
    e64, g64, near = _oracle_f64(cfg, p, cut, ge, tau=KINK_TAU)
    from oracle import clip_resnet_ref
    cr = cut.clone().requires_grad_(True)
    e32 = clip_resnet_ref.encode_image(p, cr, layers=cfg.layers, heads=cfg.heads)
    (g32,) = torch.autograd.grad(e32, cr, ge)
    floor = tf.rel_l2(g32, g64)
    gate = max(3.0 * floor, tf.F32_GATE)
    got = tf.rel_l2(gd, g64)
    print(f"[f32] {name}: embeds rel {tf.rel_l2(emb, e64):.2e}; d/dcutouts rel vs fp64 oracle {got:.2e} (fp32 oracle vs fp64 oracle {floor:.2e}); "
          f"ReLU inputs within {KINK_TAU:g} of zero: {[(f'{v:.1e}', c, i) for v, c, i in near]}")
    assert tf.rel_l2(emb, e64) < tf.F32_GATE
    if got >= gate:
        assert 1 <= len(near) <= 6, (got, gate, near)
        units = [(c, i) for _, c, i in near]
        deltas = [_oracle_f64(cfg, p, cut, ge, flips=[u])[1] - g64 for u in units]
        best = min(range(1, 2 ** len(units)), key=lambda m: float((gd - g64 - sum(d for k, d in enumerate(deltas) if m >> k & 1)).norm()))
        chosen = [u for k, u in enumerate(units) if best >> k & 1]
        g_alt = _oracle_f64(cfg, p, cut, ge, flips=chosen)[1]
        got = tf.rel_l2(gd, g_alt)
        print(f"[f32] {name}: with the masks of {chosen} inverted in the oracle: d/dcutouts rel {got:.2e}")
    assert got < gate, (got, gate)


def _bf16_case(name, n):
    """test_path_gpu.test_clip_resnet_vs_oracle's bf16 gates on the embeddings (2e-2, cosine 0.999) and on the bulk of d/dcutouts (2e-1 /
    0.98: `tiny-RN` measures 0.119 / 0.9929 there, these towers 0.116 / 0.9933 at both widths), and another treatment of the two
    entries that hold the batch minimum and maximum.  Through the renormalisation (slip.py:21-36) those two receive
    -sum_i g_i (1 - y_i) and -sum_i g_i y_i over ALL pixels i (g the gradient, y the renormalised cutouts in [0, 1]): sums of 83 000 terms
    that cancel to about the size of the bulk's norm.  Their error is the same weighted sum of the bulk's errors; with independent
    errors that is a random walk of length ||bulk error|| <= 0.2 ||bulk|| (the bulk gate), so it does not shrink with the sum, and where
    the sum happens to cancel further its relative error is anything: width 128 measures -0.0125 / -0.106 against -0.0318 / -0.153
    (errors 0.019 and 0.047 = 0.11 and 0.27 ||bulk||), which is 0.244 / 0.977 on the whole gradient, while `tiny-RN` (0.014 on the whole
    gradient) and width 96 (0.057) pass the existing 2e-1 / 0.999 because their sums are 3 x larger.  That gate on the whole gradient
    therefore tests the inputs' cancellation, not the kernels; in its place:
      (a) against the oracle, each of the two entries within 3 x 0.2 ||bulk|| (three standard deviations of the random walk at the
          bulk gate);
      (b) against the device's OWN bulk gradient, the identity above in float64 -- what the renormalisation backward has to compute,
          free of bf16 noise: within 2 max|g| + 1e-5 of sum_i |g_i| (fp32 products in the device's sums; the CPU emulation of the
          kernels meets the identity to 1e-8).
    fp16 and the exact mode keep the existing gates on the whole gradient."""
    from oracle import clip_resnet_ref
    cfg = weights.CLIP_RESNET_CONFIGS[name]
    p, cut, ge = _resnet_inputs(cfg, n)
    h = ops.ClipResNetHandle(cfg, p, max_batch=4, device=DEV, precision="bf16")
    cr = cut.clone().requires_grad_(True)
    ref = clip_resnet_ref.encode_image(p, cr, layers=cfg.layers, heads=cfg.heads)
    (gref,) = torch.autograd.grad(ref, cr, ge)
    cd = cut.to(DEV).requires_grad_(True)
    emb = ops.clip_encode_image(cd, h)
    (gd,) = torch.autograd.grad(emb, cd, ge.to(DEV))
    assert tp.rel_l2(emb, ref) < 2e-2, tp.rel_l2(emb, ref)
    assert all(tp.cosine(emb[i], ref[i]) > 0.999 for i in range(n))
    flat = cut.flatten().double()
    ext = torch.stack([flat.argmin(), flat.argmax()])
    bulk_d, bulk_r = gd.detach().cpu().flatten().double().clone(), gref.flatten().double().clone()
    ext_d, ext_r = bulk_d[ext].clone(), bulk_r[ext].clone()
    bulk_d[ext] = 0.0; bulk_r[ext] = 0.0
    print(name, "bf16 emb rel", tp.rel_l2(emb, ref), "| bulk rel", tp.rel_l2(bulk_d, bulk_r), "bulk cos", tp.cosine(bulk_d, bulk_r),
          "| min/max entries", ext_d.tolist(), ext_r.tolist(), "| whole gradient", tp.rel_l2(gd, gref), tp.cosine(gd, gref))
    assert tp.rel_l2(bulk_d, bulk_r) < 2e-1 and tp.cosine(bulk_d, bulk_r) > 0.98
    assert ((ext_d - ext_r).abs() <= 3 * 0.2 * bulk_r.norm()).all(), (ext_d, ext_r, bulk_r.norm())
    y = (flat - flat.min()) / (flat.max() - flat.min())
    own = torch.stack([-(bulk_d * (1 - y)).sum(), -(bulk_d * y).sum()])
    tol = 2 * bulk_d.abs().max() + 1e-5 * bulk_d.abs().sum()
    print("    renormalisation identity on the device's own gradient:", ext_d.tolist(), own.tolist(), "tolerance", float(tol))
    assert ((ext_d - own).abs() <= tol).all(), (ext_d, own, tol)
    # the bound has power: dropping the sum (leaving an entry its direct term only) would exceed it
    assert (own.abs() > tol).all(), (own, tol)


@pytest.mark.parametrize("precision", ["f32", "fp16", "bf16"])
@pytest.mark.parametrize("name", ["test-RN96", "test-RN128"])
def test_reduced_resnets_at_the_new_widths_vs_oracle(name, precision):
    """3 cutouts of 96 x 96 through stem, bottlenecks and attention pool at widths 96 / 128: embeddings and d/dcutouts against the
    oracle with the gates of the `tiny-RN` tests of each mode -- fp16: test_path_gpu.test_clip_resnet_vs_oracle itself (2e-2 on the
    embeddings, 2e-1 / 0.999 on the gradient, its bulk 7e-2 / 0.998); exact mode and bf16: see _f32_case and _bf16_case"""
    if precision == "f32":
        _f32_case(name, 3)
    elif precision == "bf16":
        _bf16_case(name, 3)
    else:
        tp.test_clip_resnet_vs_oracle(name, 3, precision)


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("h16", [0, 1], ids=["bf16", "half"])
@pytest.mark.parametrize("T,heads", [(145, 48), (197, 64)])
def test_attention_pool_token_counts_and_head_counts(T, heads, h16):
    """prx_k_mha_fwd_gen / bwd_gen at the attention pools' shapes (RN50x16: 145 tokens x 48 heads, RN50x64: 197 x 64), N = 2, against
    float64 softmax attention: out, lse, dq, dk, dv at test_kernels_half_gpu's gates (ATT_GATES, LSE_GATE, the elementwise bounds)"""
    print(th.attention_case(2, T, 64 * heads, heads, h16, general=True, seed=2)[0])


@pytest.mark.parametrize("h16", [0, 1], ids=["bf16", "half"])
@pytest.mark.parametrize("route", [ROUTE_TILES, ROUTE_BLK], ids=["tiles", "workgroups"])
@pytest.mark.parametrize("T", [513, 577, 640])
def test_attention_beyond_512_tokens_both_routes(T, route, h16):
    """512 < T <= 640 (one token past the old limit, ViT-L/14@336px's 577, the last length the workgroup family takes), 2 heads, N = 2:
    forward output, lse, dq, dk, dv against float64 at the same gates, through the tile kernels and through the workgroup family; a
    second run of each is bit-identical (no atomics in either)"""
    with mha_route(route):
        fig, out, dqkv, _, _ = th.attention_case(2, T, 128, 2, h16, general=True, seed=3)
        print(T, "tiles" if route else "workgroups", fig)
        _, out2, dqkv2, _, _ = th.attention_case(2, T, 128, 2, h16, general=True, seed=3)
    assert torch.equal(out, out2) and torch.equal(dqkv, dqkv2)


def test_route_switch_reaches_the_kernels_and_641_tokens_stay_on_the_tiles():
    """the two families sum in different orders: on the same operands their outputs agree to rounding but not bit for bit, which is
    what shows that the switch chose another kernel; T = 641 is beyond the workgroup family and takes the tiles under either setting"""
    outs = {}
    for T in (577, 641):
        for route in (ROUTE_TILES, ROUTE_BLK):
            with mha_route(route):
                outs[T, route] = th.attention_case(1, T, 64, 1, 1, general=True, seed=4)[1]
    assert not torch.equal(outs[577, ROUTE_TILES], outs[577, ROUTE_BLK])
    assert torch.equal(outs[641, ROUTE_TILES], outs[641, ROUTE_BLK])
    assert _lib.load().prx_mha_route(-1) == -1           # the context manager restored the default rule


# ------------------------------------------------------------------------------------------------ reduced 577-token tower
@pytest.mark.parametrize("route", [None, ROUTE_TILES, ROUTE_BLK], ids=["default", "tiles", "workgroups"])
@pytest.mark.parametrize("precision", ["f32", "fp16"])
def test_reduced_577_token_tower_vs_oracle(precision, route):
    """resolution 336, patch 14 (24 x 24 + 1 = 577 tokens, K = 588), width 128, 2 heads, 2 layers, n = 2 against oracle/clip_vit_ref with
    the gates of the `tiny-B/32` tower tests (5e-3 / 2e-2 and cosines 0.9999 half; 1e-4 exact mode, whose attention is the fp32 kernel
    under every route)"""
    with mha_route(route):
        if precision == "f32":
            if route is None:
                tf.test_clip_vit_f32_vs_oracle("test-L/14@336", 2)
        else:
            tp.test_clip_vit_vs_oracle("test-L/14@336", 2)


# ------------------------------------------------------------------------------------------------ real geometry
def _real_geometry(name, seed=0):
    p = perceptor.get_clip_perceptor(name, DEV, max_batch=1, seed=seed, precision="fp16")
    R = p.input_resolution
    g = torch.Generator().manual_seed(11)
    low = torch.rand(1, 3, R // 8, R // 8, generator=g)
    cut = torch.nn.functional.interpolate(low, size=(R, R), mode="bilinear", align_corners=False) + 0.05 * torch.randn(1, 3, R, R, generator=g)
    ge = torch.randn(1, p.output_dim, generator=g).to(DEV)
    runs = []
    for _ in range(2):
        cd = cut.to(DEV).requires_grad_(True)
        emb = p.encode_image(cd)
        (gd,) = torch.autograd.grad(emb, cd, ge)
        torch.cuda.synchronize()
        runs.append((emb.detach().clone(), gd.clone()))
    emb, gd = runs[0]
    cfg, _ = perceptor.clip_perceptor_config(name)
    assert emb.shape == (1, cfg.output_dim) and gd.shape == (1, 3, cfg.input_resolution, cfg.input_resolution)
    assert bool(torch.isfinite(emb).all()) and abs(float(emb.norm()) - 1.0) < 1e-3
    assert bool(torch.isfinite(gd).all()) and float(gd.abs().max()) > 0.0
    assert torch.equal(emb, runs[1][0]) and torch.equal(gd, runs[1][1])
    return p


@pytest.mark.parametrize("name,dim,res", [("RN50x16", 768, 384), ("ViT-L/14@336px", 768, 336), ("RN50x64", 1024, 448)])
def test_new_towers_at_their_real_geometry(name, dim, res):
    """synthetic weights of the published architecture, half operands, one cutout: the embedding has the tower's width and is a finite
    unit vector, d/dcutout is finite and not zero, a second forward + backward repeats both bit for bit"""
    p = _real_geometry(name)
    assert (p.output_dim, p.input_resolution) == (dim, res)


def test_an_allocation_that_cannot_be_met_is_an_error_with_the_figure():
    """the runner allocates one forward's activations for max_batch cutouts when it is created.  RN50x64's geometry at max_batch = 2^20:
    the first activation buffer alone (layer1.0's conv1 output, 2^20 x 112 x 112 x 128 half values) is 3.4 TB, so the very first
    activation request is refused by the runtime with only one block's weights held -- PrxError with the bytes asked for and the bytes
    held, no abort, and the next handle is created as usual.  (one block per layer keeps the weights small)"""
    from pixray_amd._lib import PrxError
    cfg = weights.ClipResNetConfig("RN50x64-shallow", 448, 128, (1, 1, 1, 1), 64, 1024)
    params = weights.synthetic_clip_resnet_params(cfg, 0)
    with pytest.raises(PrxError, match=r"device allocation of 3367254360064 bytes failed .* with \d+ bytes already held .*max_batch = 1048576"):
        ops.ClipResNetHandle(cfg, params, 1 << 20, torch.device(DEV), precision="fp16")
    torch.cuda.synchronize()
    h = ops.ClipResNetHandle(weights.CLIP_RESNET_CONFIGS["tiny-RN"], weights.synthetic_clip_resnet_params(weights.CLIP_RESNET_CONFIGS["tiny-RN"], 0),
                             1, torch.device(DEV), precision="fp16")
    emb = ops.clip_encode_image(torch.rand(1, 3, 96, 96, device=DEV), h)
    assert bool(torch.isfinite(emb).all())


# ------------------------------------------------------------------------------------------------ one run through the front end
def test_one_rn50x16_run_through_the_front_end(tmp_path):
    """`--drawer fast_pixel --clip_models RN50x16 --num_cuts 2 --size 64 48`, 2 iterations through do_init / do_run on the HIP parts:
    384-pixel cutouts, finite losses, a PNG that names the tower"""
    from PIL import Image
    from pixray_amd import frontend as fe
    run = fe.Run()
    run.settings = dict(drawer="fast_pixel", clip_models="RN50x16", num_cuts=2, size=[64, 48], iterations=2, save_every=1, display_every=2,
                        outdir=str(tmp_path / "out"), seed=5, skip_args=True, vector_prompts="none", noise_prompt_seeds=[1],
                        noise_prompt_weights=[1.0], learning_rate_drops=[])
    s = fe.apply_settings(run=run)
    sess = fe.do_init(s, run, device=None)
    assert sess.cutoutSizeTable == {"RN50x16": 384}
    z0 = sess.drawer.get_z_copy()
    while not fe.do_run(s, return_display=True, run=run):
        pass
    assert sess.cur_iteration == 2 and len(sess.last_losses) >= 1 and all(torch.isfinite(l).all() for l in sess.last_losses)
    assert float((sess.drawer.get_z().detach() - z0).abs().max()) > 0.0
    img = Image.open(os.path.join(s.outdir, "output.png"))
    assert img.size == (64, 48) and "RN50x16" in img.info["pixray_clip_models"]
