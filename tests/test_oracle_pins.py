"""CPU tests that pin the UNPINNED halves of the oracle without a second implementation of the missing libraries
(VERDICT round 2, item 6):

* kornia 0.6.2 warps (`oracle/cutouts_ref.py`): metamorphic properties that follow from kornia's own conventions -- an identity
  transform is an exact copy wherever the convention makes the map the exact pixel map, and is the documented half-pixel-class
  resampling (checked against a bilinear sampler written out by hand here) where it does not; the cached composed 3x3 of
  pixray.py:480-486 reproduces the live two-stage geometry exactly where both are exact pixel maps, and differs from it where
  the reference itself is inconsistent (live perspective: align_corners=False, cached: the function default True); f64
  gradcheck of the whole `make_cutouts`.
* CLIP ModifiedResNet (`oracle/clip_resnet_ref.py`): every block against `torch.nn` modules assembled here from the published
  class definitions (openai/CLIP clip/model.py: Bottleneck, AttentionPool2d) and loaded from the SAME state dict by OpenAI's
  parameter names -- `nn.BatchNorm2d(eval)`, `nn.AvgPool2d`, `nn.Conv2d`, `F.multi_head_attention_forward` (the function CLIP's
  attention pool calls).
"""
import math
import os
import sys
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from oracle import clip_resnet_ref, cutouts_ref  # noqa: E402
from pixray_amd import cutouts as pc  # noqa: E402
from pixray_amd import weights  # noqa: E402


# ------------------------------------------------------------------------------------------------ kornia conventions
def _bilinear_zeros(img, xs, ys):
    """hand-written bilinear sampling of img[C,H,W] (numpy, float64) at pixel coordinates (xs, ys), zeros outside"""
    C, H, W = img.shape
    x0, y0 = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
    out = np.zeros((C,) + xs.shape)
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            w = (1 - np.abs(xs - xi)) * (1 - np.abs(ys - yi))
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            out += np.where(ok, w, 0.0) * img[:, np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)]
    return out


def _img(h, w, seed=0, dtype=torch.float64):
    return torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(seed), dtype=dtype)


def test_identity_perspective_is_a_copy_only_under_align_corners_true():
    """warp_perspective normalises with [0, W-1] -> [-1, 1] and samples a linspace(-1, 1) grid: with align_corners=True the
    identity matrix is the exact pixel map (a copy); with False (what RandomPerspective passes) F.grid_sample reads
    x' = x * W / (W - 1) - 0.5 -- the half-pixel-class scale the reference really applies"""
    src = _img(9, 13)
    eye = torch.eye(3, dtype=torch.float64)[None]
    for pad in ("zeros", "border", "reflection"):
        out = cutouts_ref.warp_perspective(src, eye, (9, 13), pad, align_corners=True)
        assert (out - src).abs().max() < 1e-12, pad        # coordinates come back to whole pixels up to f64 rounding
    out = cutouts_ref.warp_perspective(src, eye, (9, 13), "zeros", align_corners=False)
    assert (out - src).abs().max() > 1e-2
    H, W = 9, 13
    xs, ys = np.meshgrid(np.arange(W) * W / (W - 1) - 0.5, np.arange(H) * H / (H - 1) - 0.5)
    want = _bilinear_zeros(src[0].numpy(), xs, ys)
    assert np.abs(out[0].numpy() - want).max() < 1e-12


def test_identity_affine_is_a_copy_under_both_flavours():
    """warp_affine builds its grid with F.affine_grid(theta, align_corners=flag) and samples with the same flag, so the
    normalised identity IS the pixel identity for either flag (RandomAffine: False; crop_by_transform_mat: True)"""
    src = _img(10, 7, seed=1)
    eye = torch.eye(3, dtype=torch.float64)[None, :2]
    for flag in (False, True):
        out = cutouts_ref.warp_affine(src, eye, (10, 7), "zeros", align_corners=flag)
        assert (out - src).abs().max() < 1e-12, flag
        fill = torch.tensor([0.3, 0.3, 0.3], dtype=torch.float64)
        out = cutouts_ref.warp_affine(src, eye, (10, 7), "fill", align_corners=flag, fill_value=fill)
        assert (out - src).abs().max() < 1e-12, flag


def test_integer_translation_is_an_exact_shift_under_align_corners_true():
    """under align_corners=True the matrix acts in pixel units (normalize_homography's convention): a translation by whole
    pixels moves the image by exactly that many pixels and fills the rest -- for warp_perspective and for warp_affine."""
    src = _img(8, 8, seed=2)
    M = torch.eye(3, dtype=torch.float64)[None].clone()
    M[0, 0, 2], M[0, 1, 2] = 2.0, -1.0                              # dst = src shifted right by 2, up by 1
    fill = torch.tensor([0.5, 0.5, 0.5], dtype=torch.float64)
    want = torch.full_like(src, 0.5)
    want[:, :, 0:7, 2:8] = src[:, :, 1:8, 0:6]
    a = cutouts_ref.warp_perspective(src, M, (8, 8), "fill", align_corners=True, fill_value=fill)
    b = cutouts_ref.warp_affine(src, M[:, :2], (8, 8), "fill", align_corners=True, fill_value=fill)
    assert (a - want).abs().max() < 1e-12 and (b - want).abs().max() < 1e-12


def _params(cutn, S, seed, **over):
    g = torch.Generator().manual_seed(seed)
    prm = pc.sample_cutout_params(cutn, S, g, iteration=0)
    prm.update(over)
    return prm


def test_cached_composed_transform_vs_the_live_geometry():
    """pixray.py:480-486 replays the composed 3x3 with ONE warp_perspective (function default align_corners=True) where the
    live path ran staged warps with each augmentation's own flag.  Where every live stage is the identity (perspective off,
    zero translation, unit scale, full-image crop window) both are plain copies of the pooled image.  A whole-pixel affine
    translation t separates the two conventions, and each side is checked against a bilinear sampler written out by hand:
    the cached warp (True) is the exact shift by t, the live RandomAffine (False) samples at x - t * W / (W - 1) -- the
    reference's own inconsistency, kept on both sides rather than repaired."""
    S, cutn = 16, 5
    img = _img(16, 16, seed=3, dtype=torch.float32)
    prm = _params(cutn, S, 4)
    nz = int(0.6 * cutn)
    nw = cutn - nz
    prm.update(dict(z_persp_apply=torch.zeros(nz, dtype=torch.bool), w_persp_apply=torch.zeros(nw, dtype=torch.bool),
                    z_jit_apply=torch.zeros(nz, dtype=torch.bool), w_jit_apply=torch.zeros(nw, dtype=torch.bool),
                    z_crop=torch.tensor([[0.0, 0.0, float(S), float(S)]] * nz), w_trans=torch.zeros(nw, 2),
                    w_scale=torch.ones(nw), noise=None))
    pooled = cutouts_ref.pooled_image(img, S)
    live = cutouts_ref.make_cutouts(img, prm, S)
    cached = cutouts_ref.make_cutouts_cached(img, prm, S)
    assert (live - pooled).abs().max() < 1e-5 and (cached - pooled).abs().max() < 1e-5
    # whole-pixel translations of the wide set
    t = torch.tensor([[1.0, -2.0], [0.0, 3.0]])[:nw]
    prm["w_trans"] = t
    live = cutouts_ref.make_cutouts(img, prm, S)
    cached = cutouts_ref.make_cutouts_cached(img, prm, S)
    assert (live[:nz] - cached[:nz]).abs().max() < 1e-5               # the zoom set is untouched
    fill = float(prm["fill"])
    src = pooled[0].double().numpy()
    ones = np.ones_like(src)
    xs, ys = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64))
    for i in range(nw):
        tx, ty = float(t[i, 0]), float(t[i, 1])
        for got, scale in ((cached[nz + i], 1.0), (live[nz + i], S / (S - 1.0))):
            sx, sy = xs - tx * scale, ys - ty * scale
            want = _bilinear_zeros(src, sx, sy) + fill * (1.0 - _bilinear_zeros(ones, sx, sy))
            assert np.abs(got.double().numpy() - want).max() < 1e-5, (i, scale)
    assert (live[nz:] - cached[nz:]).abs().max() > 1e-2
    # perspective on: live (align_corners=False) != cached (True) as well
    prm["w_trans"] = torch.zeros(nw, 2)
    prm["w_persp_apply"] = torch.ones(nw, dtype=torch.bool)
    live = cutouts_ref.make_cutouts(img, prm, S)
    cached = cutouts_ref.make_cutouts_cached(img, prm, S)
    assert (live[nz:] - cached[nz:]).abs().max() > 1e-2


def test_make_cutouts_gradcheck_f64():
    """the whole staged construction (pooling, perspective, crop, affine, fill padding, noise) is differentiable as written:
    float64 finite differences vs autograd, ColorJitter off (its HSV round trip is not differentiable where two channels
    tie, and is gradchecked on its own below)"""
    S, cutn = 6, 5
    nz = int(0.6 * cutn)
    prm = _params(cutn, S, 7, z_jit_apply=torch.zeros(nz, dtype=torch.bool), w_jit_apply=torch.zeros(cutn - nz, dtype=torch.bool))
    prm["noise"] = None
    img = _img(12, 12, seed=8).requires_grad_(True)
    # adaptive max pooling picks one element per window: keep the maxima well separated so finite differences stay on one branch
    with torch.no_grad():
        img += torch.linspace(0, 0.5, img.numel(), dtype=torch.float64).reshape(img.shape)[..., torch.randperm(12, generator=torch.Generator().manual_seed(1))]
    proj = torch.randn(cutn, 3, S, S, dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    assert torch.autograd.gradcheck(lambda x: (cutouts_ref.make_cutouts(x, prm, S) * proj).sum(), (img,), eps=1e-6, atol=1e-6, rtol=1e-4)


def test_color_jitter_gradcheck_f64_away_from_ties():
    g = torch.Generator().manual_seed(10)
    # channels kept apart (r > g > b by >= 0.1) so that max / min / argmax are locally constant
    x = torch.stack([0.7 + 0.2 * torch.rand(2, 4, 4, generator=g, dtype=torch.float64),
                     0.4 + 0.2 * torch.rand(2, 4, 4, generator=g, dtype=torch.float64),
                     0.1 + 0.2 * torch.rand(2, 4, 4, generator=g, dtype=torch.float64)], dim=1).requires_grad_(True)
    apply = torch.tensor([True, True])
    sat, hue = torch.tensor([1.07, 0.93], dtype=torch.float64), torch.tensor([0.03, -0.02], dtype=torch.float64)
    for sat_first in (True, False):
        assert torch.autograd.gradcheck(lambda t: cutouts_ref.color_jitter(t, apply, sat, hue, sat_first), (x,), eps=1e-7, atol=1e-6)
    # neutral factors: an identity (the rgb -> hsv -> rgb round trip is exact to rounding)
    y = cutouts_ref.color_jitter(x.detach(), apply, torch.ones(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64), True)
    assert (y - x.detach()).abs().max() < 1e-7           # kornia's eps = 1e-8 in the saturation denominator


# ------------------------------------------------------------------------------------------------ a second implementation, end to end
import pytest  # noqa: E402

import _independent_cutouts as indep  # noqa: E402

_E2E_CASES = [(40, 40, 12, 10, 0, 1.0, 0), (40, 40, 12, 10, 1, 1.0, 1), (36, 54, 12, 10, 0, 1.5, 2), (54, 36, 12, 10, 1, 36 / 54, 3),
              (33, 47, 9, 7, 2, 47 / 33, 4)]


def _e2e_inputs(H, W, S, cutn, it, aspect, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(1, 3, H, W, generator=g)
    prm = pc.sample_cutout_params(cutn, S, g, iteration=it, aspect=aspect)
    prm["noise"] = torch.randn(cutn, 3, S, S, generator=g)
    return img, prm


@pytest.mark.parametrize("case", _E2E_CASES)
def test_make_cutouts_vs_the_independent_scipy_colorsys_implementation(case):
    """`oracle/cutouts_ref.make_cutouts` END TO END (pooling, aspect rescale, perspective, resized crop, affine + fill, centre
    crop, padded perspective, ColorJitter in either order, noise; reflection and border iterations; square, wide and tall
    canvases; non-divisible pooling windows) against tests/_independent_cutouts.py: numpy float64 closed-form pixel maps +
    scipy.ndimage.map_coordinates + colorsys, no torch, no normalised grids (its module docstring has the side-by-side).
    fp32 round-off is the only difference allowed."""
    H, W, S, cutn, it, aspect, seed = case
    img, prm = _e2e_inputs(*case)
    ref = cutouts_ref.make_cutouts(img, prm, S).double().numpy()
    out = indep.make_cutouts(img[0].double().numpy(), indep.params_to_numpy(prm), S)
    assert ref.shape == out.shape == (cutn, 3, S, S)
    assert np.abs(ref - out).max() < 3e-6, np.abs(ref - out).max()
    # the cached-transform replay (pixray.py:480-486) through the same second implementation
    refc = cutouts_ref.make_cutouts_cached(img, prm, S).double().numpy()
    outc = indep.make_cutouts_cached(img[0].double().numpy(), indep.params_to_numpy(prm), S)
    assert np.abs(refc - outc).max() < 3e-6, np.abs(refc - outc).max()


@pytest.mark.parametrize("flag", ["perspective_align_corners", "affine_align_corners", "crop_align_corners"])
def test_each_align_corners_convention_moves_both_implementations_alike(flag):
    """flipping ONE kornia flag changes the oracle's output by 1e-2 ... 2e-1, and the independent implementation follows it
    to round-off: the closed-form reading of each flag (half-pixel-class scale / shift) is the one the oracle realises."""
    case = _E2E_CASES[3]
    S = case[2]
    img, prm = _e2e_inputs(*case)
    cv = {flag: not cutouts_ref.CONVENTIONS[flag]}
    base = cutouts_ref.make_cutouts(img, prm, S).double().numpy()
    ref = cutouts_ref.make_cutouts(img, prm, S, conventions=cv).double().numpy()
    out = indep.make_cutouts(img[0].double().numpy(), indep.params_to_numpy(prm), S, conventions=cv)
    assert np.abs(ref - base).max() > 5e-3
    assert np.abs(ref - out).max() < 3e-6


def test_oracle_image_gradient_vs_finite_differences_of_the_independent_implementation():
    """d(sum(cutouts * proj)) / d(image) from the ORACLE's autograd against central differences of the INDEPENDENT forward
    (float64, ColorJitter off, pooling maxima separated): the backward the HIP kernels are compared with is the derivative of a
    function that was not written by the same hand."""
    S, cutn, H, W = 6, 5, 12, 12
    nz = int(0.6 * cutn)
    g = torch.Generator().manual_seed(21)
    prm = pc.sample_cutout_params(cutn, S, g, iteration=0)
    prm["z_jit_apply"] = torch.zeros(nz, dtype=torch.bool)
    prm["w_jit_apply"] = torch.zeros(cutn - nz, dtype=torch.bool)
    img = torch.rand(1, 3, H, W, generator=g, dtype=torch.float64)
    img += torch.linspace(0, 0.5, img.numel(), dtype=torch.float64).reshape(img.shape)[..., torch.randperm(W, generator=g)]
    proj = torch.randn(cutn, 3, S, S, dtype=torch.float64, generator=g)
    x = img.clone().requires_grad_(True)
    (cutouts_ref.make_cutouts(x, prm, S) * proj).sum().backward()
    p_np, proj_np = indep.params_to_numpy(prm), proj.numpy()
    base = img[0].numpy()
    eps = 1e-6
    rng = np.random.default_rng(0)
    for _ in range(40):
        c, y, xx = rng.integers(3), rng.integers(H), rng.integers(W)
        hi, lo = base.copy(), base.copy()
        hi[c, y, xx] += eps
        lo[c, y, xx] -= eps
        fd = ((indep.make_cutouts(hi, p_np, S) - indep.make_cutouts(lo, p_np, S)) * proj_np).sum() / (2 * eps)
        assert abs(fd - float(x.grad[0, c, y, xx])) < 1e-6 + 1e-5 * abs(fd), (c, y, xx, fd, float(x.grad[0, c, y, xx]))


# ------------------------------------------------------------------------------------------------ CLIP ModifiedResNet blocks
class _Bottleneck(nn.Module):
    """openai/CLIP clip/model.py `Bottleneck` as published (expansion 4; all strides through AvgPool2d; the downsample branch
    is Sequential(OrderedDict([("-1", AvgPool2d(stride)), ("0", Conv2d 1x1), ("1", BatchNorm2d)])))"""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.avgpool = nn.AvgPool2d(stride) if stride > 1 else nn.Identity()
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None
        if stride > 1 or inplanes != planes * 4:
            self.downsample = nn.Sequential(OrderedDict([("-1", nn.AvgPool2d(stride)), ("0", nn.Conv2d(inplanes, planes * 4, 1, stride=1, bias=False)),
                                                         ("1", nn.BatchNorm2d(planes * 4))]))

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.avgpool(out)
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


def _block_state(p, pre):
    return {k[len(pre) + 1:]: v for k, v in p.items() if k.startswith(pre + ".")}


def test_resnet_oracle_bottlenecks_vs_torch_nn_modules():
    cfg = weights.CLIP_RESNET_CONFIGS["tiny-RN"]
    p = weights.synthetic_clip_resnet_params(cfg, seed=5)
    g = torch.Generator().manual_seed(6)
    w = cfg.width
    inplanes = w
    checked = 0
    for li, nblocks in enumerate(cfg.layers):
        planes = w * 2 ** li
        for b in range(nblocks):
            stride = 2 if (li > 0 and b == 0) else 1
            pre = f"layer{li + 1}.{b}"
            mod = _Bottleneck(inplanes, planes, stride).eval()
            missing = mod.load_state_dict(_block_state(p, pre), strict=False)
            assert not missing.unexpected_keys, missing
            assert all(k.endswith("num_batches_tracked") for k in missing.missing_keys), missing
            x = torch.randn(2, inplanes, 12, 12, generator=g).requires_grad_(True)
            want = mod(x)
            got = clip_resnet_ref._bottleneck(p, pre, x, stride)
            assert got.shape == want.shape and (got - want).abs().max() < 1e-5 * max(1.0, want.abs().max().item()), pre
            gw = torch.randn(want.shape, generator=g)
            (ga,) = torch.autograd.grad(want, x, gw, retain_graph=True)
            (gb,) = torch.autograd.grad(got, x, gw)
            assert (ga - gb).abs().max() < 1e-5 * max(1.0, ga.abs().max().item()), pre
            inplanes = planes * 4
            checked += 1
    assert checked == sum(cfg.layers)


def test_resnet_oracle_stem_and_batchnorm_vs_torch_nn():
    cfg = weights.CLIP_RESNET_CONFIGS["tiny-RN"]
    p = weights.synthetic_clip_resnet_params(cfg, seed=5)
    w = cfg.width
    stem = nn.Sequential(OrderedDict([
        ("conv1", nn.Conv2d(3, w // 2, 3, stride=2, padding=1, bias=False)), ("bn1", nn.BatchNorm2d(w // 2)), ("relu1", nn.ReLU()),
        ("conv2", nn.Conv2d(w // 2, w // 2, 3, padding=1, bias=False)), ("bn2", nn.BatchNorm2d(w // 2)), ("relu2", nn.ReLU()),
        ("conv3", nn.Conv2d(w // 2, w, 3, padding=1, bias=False)), ("bn3", nn.BatchNorm2d(w)), ("relu3", nn.ReLU()),
        ("avgpool", nn.AvgPool2d(2))])).eval()
    sd = {k: v for k, v in p.items() if k.split(".")[0] in ("conv1", "conv2", "conv3", "bn1", "bn2", "bn3")}
    r = stem.load_state_dict(sd, strict=False)
    assert not r.unexpected_keys and all(k.endswith("num_batches_tracked") for k in r.missing_keys), r
    x = torch.randn(2, 3, cfg.input_resolution, cfg.input_resolution, generator=torch.Generator().manual_seed(2))
    want = stem(x)
    # the oracle's stem is the first four statements of resnet_forward: run it with no layers and intercept before the pool
    y = F.relu(clip_resnet_ref._bn(p, "bn1", F.conv2d(x, p["conv1.weight"], stride=2, padding=1)))
    y = F.relu(clip_resnet_ref._bn(p, "bn2", F.conv2d(y, p["conv2.weight"], padding=1)))
    y = F.relu(clip_resnet_ref._bn(p, "bn3", F.conv2d(y, p["conv3.weight"], padding=1)))
    y = F.avg_pool2d(y, 2)
    assert (y - want).abs().max() < 1e-5 * max(1.0, want.abs().max().item())


def test_resnet_oracle_attention_pool_vs_torch_multi_head_attention():
    """CLIP's AttentionPool2d.forward calls F.multi_head_attention_forward(query=x[:1], key=x, value=x, ... ,
    use_separate_proj_weight=True, q/k/v_proj_weight, in_proj_bias=cat(q,k,v biases), out_proj = c_proj): that torch
    function against the oracle's explicit arithmetic, forward and gradient"""
    cfg = weights.CLIP_RESNET_CONFIGS["tiny-RN"]
    p = weights.synthetic_clip_resnet_params(cfg, seed=5)
    C = cfg.width * 32
    G = cfg.input_resolution // 32
    x = torch.randn(3, C, G, G, generator=torch.Generator().manual_seed(4)).requires_grad_(True)
    got = clip_resnet_ref.attention_pool(p, x, cfg.heads)
    t = x.flatten(2).permute(2, 0, 1)
    t = torch.cat([t.mean(dim=0, keepdim=True), t], dim=0)
    t = t + p["attnpool.positional_embedding"][:, None, :]
    want, _ = F.multi_head_attention_forward(
        query=t[:1], key=t, value=t, embed_dim_to_check=C, num_heads=cfg.heads,
        q_proj_weight=p["attnpool.q_proj.weight"], k_proj_weight=p["attnpool.k_proj.weight"], v_proj_weight=p["attnpool.v_proj.weight"],
        in_proj_weight=None, in_proj_bias=torch.cat([p["attnpool.q_proj.bias"], p["attnpool.k_proj.bias"], p["attnpool.v_proj.bias"]]),
        bias_k=None, bias_v=None, add_zero_attn=False, dropout_p=0.0, out_proj_weight=p["attnpool.c_proj.weight"],
        out_proj_bias=p["attnpool.c_proj.bias"], use_separate_proj_weight=True, training=False, need_weights=False)
    want = want.squeeze(0)
    assert got.shape == want.shape == (3, cfg.output_dim)
    assert (got - want).abs().max() < 1e-5 * max(1.0, want.abs().max().item())
    gw = torch.randn(want.shape, generator=torch.Generator().manual_seed(5))
    (ga,) = torch.autograd.grad(want, x, gw, retain_graph=True)
    (gb,) = torch.autograd.grad(got, x, gw)
    assert (ga - gb).abs().max() < 1e-5 * max(1.0, ga.abs().max().item())


def test_resnet_oracle_whole_tower_vs_torch_nn_assembly():
    """the blocks above chained as clip.model.ModifiedResNet.forward does (stem, layer1..4, attnpool) equal the oracle's tower"""
    cfg = weights.CLIP_RESNET_CONFIGS["tiny-RN"]
    p = weights.synthetic_clip_resnet_params(cfg, seed=9)
    x = torch.randn(2, 3, cfg.input_resolution, cfg.input_resolution, generator=torch.Generator().manual_seed(3))
    got = clip_resnet_ref.resnet_forward(p, x, layers=cfg.layers, heads=cfg.heads)
    w = cfg.width
    y = x
    for i, (co, st) in enumerate([(w // 2, 2), (w // 2, 1), (w, 1)], start=1):
        conv = nn.Conv2d(y.shape[1], co, 3, stride=st, padding=1, bias=False)
        bn = nn.BatchNorm2d(co).eval()
        conv.load_state_dict({"weight": p[f"conv{i}.weight"]})
        bn.load_state_dict({k: p[f"bn{i}.{k}"] for k in ("weight", "bias", "running_mean", "running_var")}, strict=False)
        y = F.relu(bn(conv(y)))
    y = nn.AvgPool2d(2)(y)
    inplanes = w
    for li, nblocks in enumerate(cfg.layers):
        planes = w * 2 ** li
        for b in range(nblocks):
            mod = _Bottleneck(inplanes, planes, 2 if (li > 0 and b == 0) else 1).eval()
            mod.load_state_dict(_block_state(p, f"layer{li + 1}.{b}"), strict=False)
            y = mod(y)
            inplanes = planes * 4
    want = clip_resnet_ref.attention_pool(p, y, cfg.heads)       # pinned on its own above
    assert (got - want).abs().max() < 1e-5 * max(1.0, want.abs().max().item())


# ------------------------------------------------------------------------------------------------ fft drawer (configs[3])
def test_fft_oracle_inverse_transform_is_the_definition_of_irfft2():
    """`oracle/fft_ref.inverse_real_dft2` against (a) the double sum written as python loops over a tiny spectrum -- including
    non-zero imaginary parts in the DC and Nyquist columns, which a complex-to-real transform must ignore -- and (b)
    numpy's pocketfft `irfft2` for even / odd widths and heights"""
    from oracle import fft_ref
    g = torch.Generator().manual_seed(0)
    for (h, w) in [(4, 6), (5, 7), (6, 5), (3, 4)]:
        wf = fft_ref.n_freq_columns(w)
        spec = torch.randn(2, h, wf, 2, generator=g, dtype=torch.float64)
        got = fft_ref.inverse_real_dft2(spec, h, w).numpy()
        S = spec[..., 0].numpy() + 1j * spec[..., 1].numpy()
        want = np.zeros((2, h, w))
        for n in range(2):
            for y in range(h):
                for x in range(w):
                    acc = 0.0
                    for v in range(w // 2 + 1):
                        col = sum(S[n, u, v] * np.exp(2j * math.pi * u * y / h) for u in range(h))
                        if v == 0 or (w % 2 == 0 and v == w // 2):
                            acc += (col * np.exp(2j * math.pi * v * x / w)).real
                        else:
                            acc += 2 * (col * np.exp(2j * math.pi * v * x / w)).real
                    want[n, y, x] = acc / math.sqrt(h * w)
        assert np.abs(got - want).max() < 1e-12, (h, w)
        lib = np.fft.irfft2(S[..., : w // 2 + 1], s=(h, w), norm="ortho")
        assert np.abs(got - lib).max() < 1e-12, (h, w)


@pytest.mark.parametrize("size", [(96, 64), (45, 32), (64, 33), (31, 17)])
def test_fft_drawer_plugin_on_the_cpu_vs_the_explicit_dft_oracle(size):
    """the product's `FftDrawer` (torch.fft + einsum; the same class runs on rocFFT on the GPU) against oracle/fft_ref.py
    (explicit DFT sums in float64, no FFT library): identical seeded start, image to fp32 round-off, gradient w.r.t. the spectrum
    to 1e-6 -- even and odd canvas sizes (the odd-width spectrum carries the surplus column of the lucid frequency helper)"""
    import types
    from oracle import fft_ref
    from pixray_amd.fft_drawer import FftDrawer
    st = types.SimpleNamespace(size=size, fft_use="fft", fft_decay=1.5, fft_lrate=0.3, weight_seed=3)
    dr = FftDrawer(st)
    dr.load_model(st, "cpu")
    dr.init_from_tensor(None)
    p = fft_ref.rand_init(size, 3)
    assert torch.equal(p.detach(), dr.params[0].detach())
    a, b = dr.synth(0), fft_ref.synth(p, size)
    assert a.shape == b.shape == (1, 3, size[1], size[0])
    assert float((a - b).detach().abs().max()) < 1e-6
    proj = torch.randn(a.shape, generator=torch.Generator().manual_seed(1))
    (ga,) = torch.autograd.grad((a * proj).sum(), dr.params[0])
    (gb,) = torch.autograd.grad((b * proj).sum(), p)
    assert float((ga - gb).norm() / gb.norm()) < 2e-6


# ------------------------------------------------------------------------------------------------ VGG16 extractor (StyleLoss)
def test_vgg_oracle_vs_the_reference_extractor_class_run_live():
    """`oracle/vgg_ref.forward` against the reference's OWN `Vgg16_Extractor.forward` (Losses/StyleLoss.py:24-47, pulled out by
    AST and run by tests/golden/make_golden.py) wrapped around an nn.Sequential laid out like torchvision's vgg16().features:
    the same ten maps in both input spaces -- shapes, float64 sums and sums of squares, and the values at 512 seeded positions
    of every map (reference_live_golden.npz) -- so the capture indices [1,3,6,8,11,13,15,22,29] and the ImageNet
    normalisation are the reference's, executed, not restated"""
    from oracle import vgg_ref
    d = np.load(os.path.join(HERE, "golden", "reference_live_golden.npz"))
    params = weights.synthetic_vgg16_params(0)
    x = torch.from_numpy(d["vgg_x"])
    for space in ("uniform", "vgg"):
        got = vgg_ref.forward(params, x.clone(), space)
        assert int(d[f"vgg_{space}_count"]) == len(got) == 10
        for i, o in enumerate(got):
            k = f"vgg_{space}_{i}"
            assert tuple(o.shape) == tuple(d[k + "_shape"]), (space, i)
            r_sum, r_sq, r_max = d[k + "_stats"]
            # map 0 is the normalised input; the reference's in-place ReLUs overwrite the captured conv outputs, as here
            tol = 1e-6 * max(1.0, float(r_max))
            sample = o.reshape(-1)[torch.from_numpy(d[k + "_index"])]
            assert float((sample - torch.from_numpy(d[k + "_sample"])).abs().max()) <= tol, (space, i)
            o64 = o.double()
            assert abs(float(o64.abs().max()) - r_max) <= tol, (space, i)
            assert abs(float(o64.sum()) - r_sum) <= tol * o.numel(), (space, i)
            assert abs(float((o64 * o64).sum()) - r_sq) <= 2 * tol * float(o64.abs().sum()) + 1e-9 * r_sq, (space, i)


# ------------------------------------------------------------------------------------------------ what the teacher-forced image rests on
def test_reference_image_gradient_is_discontinuous_at_clamp_ties():
    """`oracle/step_ref.compare_k_steps` evaluates the oracle's cutouts -> CLIP -> loss gradient AT THE HIP PATH'S IMAGE because
    the reference's dL/d(image) is not a continuous function of the image once pixels sit on the bounds of `clamp_with_grad`
    (vqgan.py:66-79): `MakeCutouts` adds an adaptive MAX pool (pixray.py:443,463) whose gradient goes to the first maximum of a
    window, and tied windows re-route gradient spikes.  The ORACLE ALONE shows it (tools/oracle_tie_sensitivity.py; the headline
    run is committed under profiles/): at its own state after three Adam steps on a 256 x 256 canvas (two-pixel pooling windows,
    as at the headline), 1e-6 of image noise moves dL/d(image) by tenths -- and by 1e-3 or less once the max pool is swapped for an
    average pool."""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import oracle_tie_sensitivity as ots
    r = ots.measure(vqgan_model="tiny_f4", clip_model="tiny-B/32", size=(256, 256), cutn=8, steps=3)
    assert r["pixels_on_a_clamp_bound"] > 0.01, r
    assert r["rel_max"] >= 0.3, r
    assert r["rel_avg"] <= 1e-3, r
