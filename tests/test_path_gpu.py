"""Path-level parity tests (GPU): each operator of the hot path, called through the C ABI
(pixray_amd.ops -> libprx_hip.so), against the CPU fp32 oracle on the same seeded inputs.

Tolerances (stated per check):
  * fp32 kernels (cutouts, prompt loss, Adam, VQ): 1e-4-class, only summation order / fused-multiply
    differences.
  * bf16-MFMA networks (CLIP tower, VQGAN decoder): GEMM operands are rounded to bf16 (2^-9 relative
    per element), residual streams stay fp32: outputs within 2e-2 rel-L2, gradients within 3e-2 rel-L2
    and cosine >= 0.999 (BASELINE.md §3 targets: 2e-2 / 0.999).
"""
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import clip_vit_ref, cutouts_ref, prompt_ref, vqgan_ref
from pixray_amd import cutouts as pc
from pixray_amd import ops, weights
from pixray_amd._lib import call

DEV = "cuda"


def rel_l2(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def cosine(a, b):
    a, b = a.detach().float().cpu().flatten(), b.detach().float().cpu().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


# ------------------------------------------------------------------------------------------ cutouts
def _test_image(kind, HW, g):
    if kind == "noise":                       # worst case for position rounding: |d img/d px| ~ 0.3
        return torch.rand(1, 3, HW, HW, generator=g)
    low = torch.rand(1, 3, max(HW // 8, 4), max(HW // 8, 4), generator=g)
    img = torch.nn.functional.interpolate(low, size=(HW, HW), mode="bicubic")
    if kind == "smooth":
        return img.clamp(0.02, 0.98)
    return (img * 1.6 - 0.3).clamp(0, 1)      # "clamped": what ClampWithGrad leaves, exact 0/1 plateaus


@pytest.mark.parametrize("cutn,S,HW,it,kind", [(10, 224, 256, 0, "noise"), (10, 224, 256, 1, "smooth"),
                                                (64, 224, 256, 2, "smooth"), (5, 64, 40, 3, "noise"),
                                                (10, 224, 256, 0, "clamped"), (64, 224, 256, 1, "clamped")])
def test_make_cutouts_vs_oracle(cutn, S, HW, it, kind):
    g = torch.Generator().manual_seed(100 + cutn + it)
    img = _test_image(kind, HW, g)
    prm = pc.sample_cutout_params(cutn, S, g, iteration=it)
    prm["noise"] = torch.randn(cutn, 3, S, S, generator=g)
    img_ref = img.clone().requires_grad_(True)
    ref = cutouts_ref.make_cutouts(img_ref, prm, S)
    gout = torch.randn(cutn, 3, S, S, generator=g)
    (gref,) = torch.autograd.grad(ref, img_ref, gout)

    mk = pc.MakeCutouts(S, cutn)
    mk.fixed_params = prm
    img_d = img.to(DEV).requires_grad_(True)
    out = mk(img_d)
    assert out.shape == (cutn, 3, S, S) and out.grad_fn is not None
    # forward: fp32 gathers whose tap positions round like the oracle's (fp64 homography -> fp32 grid):
    # 2e-5 abs on [0,1] data, 1e-5 rel-L2
    assert (out.detach().cpu() - ref.detach()).abs().max().item() < 1e-4
    assert rel_l2(out, ref) < 1e-5
    (gd,) = torch.autograd.grad(out, img_d, gout.to(DEV))
    if kind != "clamped":
        # backward: atomics reorder fp32 sums; the HSV Jacobian is smooth away from gray / pure colours
        assert rel_l2(gd, gref) < 3e-3, rel_l2(gd, gref)     # measured 1e-5 (smooth) .. 2e-3 (white noise)
        assert cosine(gd, gref) > 0.99999
    else:
        # On exact 0/1 plateaus two channels tie to within 1e-6, hue is ill-defined and kornia's rgb->hsv->rgb
        # Jacobian is discontinuous in the last ulp of its input (either implementation returns rounding noise
        # there, as CUDA-vs-CPU kornia would).  Everywhere else the gradients agree: require that <1.5% of the
        # image-gradient entries deviate and that the bulk agrees to 2e-2 rel-L2.
        d = (gd.cpu() - gref).abs()
        scale = gref.abs().mean().item()
        assert (d > 1e-2 * scale).float().mean().item() < 1.5e-2
        assert rel_l2(gd, gref) < 2e-2, rel_l2(gd, gref)      # measured 5e-3 .. 1.3e-2
        assert cosine(gd, gref) > 0.9998


def cutout_noise_checks():
    """pixray.py:508-510 (`batch + fac * randn_like(batch)`) without a noise tensor: the stage-B kernel draws N(0,1) itself
    (Philox4x32-10 keyed by descriptor word 32, counter = pixel index, Box-Muller).  Zero canvas, identity geometry, factor 1:
    the output IS the noise -- moments, independence of channels / neighbours / cutouts, same key -> same bits, and a shard of
    the batch sees the draws the whole batch sees.  Device-agnostic (DEV): the emulator suite calls it on CPU tensors.
    Returns the draws."""
    n, S = 6, 64
    desc = torch.zeros(n, pc.DESC_WORDS, dtype=torch.float64)
    desc[:, 0:9] = torch.eye(3, dtype=torch.float64).reshape(9); desc[:, 9:18] = desc[:, 0:9]
    desc[:, 18] = pc.MODE_IDENT; desc[:, 19] = pc.MODE_IDENT
    desc[:, 25] = 1.0
    desc[:, 28:32] = torch.tensor([0.0, 0.0, float(S), float(S)], dtype=torch.float64)
    desc[:, 32] = torch.tensor([11, 12, 13, 2 ** 52 + 12345, 15, 11], dtype=torch.float64)     # first and last cutout share a key; one key above 2^32
    desc = desc.to(DEV)
    img = torch.zeros(1, 3, S, S, device=DEV)
    z = ops.make_cutouts(img, desc, None, S)
    assert z.shape == (n, 3, S, S) and torch.isfinite(z).all()
    assert abs(float(z.mean())) < 0.02 and abs(float(z.std()) - 1.0) < 0.02
    assert abs(float((z ** 3).mean())) < 0.06 and abs(float((z ** 4).mean()) - 3.0) < 0.15
    assert torch.equal(z[0], z[5]) and not torch.equal(z[0], z[1])
    flat = z[:5].reshape(5, 3, -1)
    c = lambda a, b: abs(float(((a - a.mean()) * (b - b.mean())).mean() / (a.std() * b.std())))
    assert c(flat[:, 0], flat[:, 1]) < 0.02 and c(flat[:, 0], flat[:, 2]) < 0.02 and c(flat[:, 1], flat[:, 2]) < 0.02   # channels
    assert c(flat[:, :, 1:], flat[:, :, :-1]) < 0.02 and c(flat[0], flat[1]) < 0.03                                      # neighbours, cutouts
    assert torch.equal(ops.make_cutouts(img, desc, None, S), z)
    assert torch.equal(ops.make_cutouts(img, desc[2:4].contiguous(), None, S), z[2:4])                                   # a shard sees the whole batch's draws
    d0 = desc.clone(); d0[:, 32] = 0.0                                                          # no key, no tensor: no noise
    assert float(ops.make_cutouts(img, d0, None, S).abs().max()) == 0.0
    # the module draws one key per cutout and iteration from a stream of its own: the augmentation draws stay where they were
    mk = pc.MakeCutouts(S, 4, noise_fac=0.1, generator=torch.Generator().manual_seed(5))
    mk.prepare(iteration=0, fill=0.5)
    k0 = mk.last_params["noise_seed"].clone()
    ref = pc.sample_cutout_params(4, S, torch.Generator().manual_seed(5), 0, 0.1, fill=0.5)
    assert all(torch.equal(mk.last_params[k], v) for k, v in ref.items() if isinstance(v, torch.Tensor))
    mk(torch.rand(1, 3, S, S, device=DEV))
    mk.prepare(iteration=1, fill=0.5)
    assert not torch.equal(mk.last_params["noise_seed"], k0)
    assert int(mk.last_params["noise_seed"].max()) < 2 ** 53                                    # a key is one exact descriptor word (float64)
    # the noise has the reference's scale: fac * N(0, 1) on top of the cutouts (statistics of a larger batch)
    desc2 = desc.clone(); desc2[:, 25] = 0.1
    z2 = ops.make_cutouts(img, desc2, None, S)
    assert abs(float(z2.std()) - 0.1) < 0.003
    return z.detach().cpu()


def test_cutout_noise_drawn_in_the_kernel_on_the_device():
    """the branch of the stage-B kernel that bench.py and Session.train run (no noise tensor: in-kernel Philox) ON THE DEVICE --
    every parity harness hands an explicit noise tensor and takes the other branch.  Moments / independence / key and shard
    invariance as on the emulation, and the device's draws against the emulated kernel's for the same keys: the Philox integers are
    exact on both, so the normals agree to the rounding of logf / sincosf / sqrtf (a few ulps of values <= 6)."""
    z_dev = cutout_noise_checks()
    import _emu
    import shutil
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") or shutil.which("make") is None:
        pytest.skip("no host toolchain for tools/hipemu on this box: device-vs-emulator comparison not run")
    global DEV
    with _emu.enable():
        DEV = "cpu"
        try:
            z_emu = cutout_noise_checks()
        finally:
            DEV = "cuda"
    d = (z_dev - z_emu).abs()
    same = float((z_dev == z_emu).float().mean())
    print(f"device vs emulated Philox normals: max |diff| {float(d.max()):.3e}, bit-identical {100 * same:.2f} %")
    assert float(d.max()) < 4e-6 and same > 0.5


@pytest.mark.parametrize("flip", ["crop_align_corners", "perspective_align_corners", "affine_align_corners"])
def test_cutout_align_corners_convention_is_a_descriptor_field(flip):
    """which align_corners flag each kornia call passes (oracle/cutouts_ref.py table) is DATA in the descriptor, not an
    assumption baked into the kernel: flip one convention on both sides and the HIP kernel follows the oracle again, forward
    and backward, while the two conventions themselves give visibly different cutouts"""
    cutn, S, HW = 10, 224, 256
    g = torch.Generator().manual_seed(77)
    img = _test_image("smooth", HW, g)
    prm = pc.sample_cutout_params(cutn, S, g, iteration=0)
    prm["noise"] = torch.randn(cutn, 3, S, S, generator=g)
    prm["z_jit_apply"][:] = False          # geometry only: the jitter's Jacobian has its own (tie-break) noise
    prm["w_jit_apply"][:] = False
    gout = torch.randn(cutn, 3, S, S, generator=g)
    outs = {}
    for value in (pc.KORNIA_062_CONVENTIONS[flip], not pc.KORNIA_062_CONVENTIONS[flip]):
        cv = {flip: value}
        img_ref = img.clone().requires_grad_(True)
        ref = cutouts_ref.make_cutouts(img_ref, prm, S, conventions=cv)
        (gref,) = torch.autograd.grad(ref, img_ref, gout)
        mk = pc.MakeCutouts(S, cutn)
        mk.fixed_params = prm
        mk.conventions = cv
        img_d = img.to(DEV).requires_grad_(True)
        out = mk(img_d)
        (gd,) = torch.autograd.grad(out, img_d, gout.to(DEV))
        assert rel_l2(out, ref) < 1e-5, (flip, value, rel_l2(out, ref))
        assert rel_l2(gd, gref) < 1e-4, (flip, value, rel_l2(gd, gref))
        outs[value] = out.detach().cpu()
    assert rel_l2(outs[True], outs[False]) > 1e-3          # the convention matters: a half-pixel-class resampling difference


def test_make_cutouts_shard_matches_full():
    """cutout sharding: slices of the batch equal the same rows of the full batch"""
    cutn, S = 16, 224
    g = torch.Generator().manual_seed(7)
    img = torch.rand(1, 3, 256, 256, generator=g).to(DEV)
    prm = pc.sample_cutout_params(cutn, S, g, iteration=0)
    prm["noise"] = torch.randn(cutn, 3, S, S, generator=g)
    mk = pc.MakeCutouts(S, cutn)
    mk.fixed_params = prm
    full = mk(img)
    parts = []
    for r in range(4):
        mk.shard = (r * 4, r * 4 + 4)
        mk.transforms = None          # each rank's call is the first of its iteration (else: cached-transform path)
        parts.append(mk(img))
    assert torch.equal(torch.cat(parts), full)


# ------------------------------------------------------------------------------------------ prompt
@pytest.mark.parametrize("n,m,D,w,stop", [(64, 1, 512, 1.0, float("-inf")), (64, 3, 512, -0.5, float("-inf")),
                                           (16, 2, 128, 2.0, 0.9), (64, 1, 512, 0.1, float("-inf"))])
def test_prompt_loss_vs_oracle(n, m, D, w, stop):
    g = torch.Generator().manual_seed(n + m)
    x = torch.randn(n, D, generator=g)
    x = x / x.norm(dim=-1, keepdim=True)
    e = torch.randn(m, D, generator=g)
    xr = x.clone().requires_grad_(True)
    ref = prompt_ref.Prompt(e, w, stop)(xr)
    (gref,) = torch.autograd.grad(ref, xr)
    xd = x.to(DEV).requires_grad_(True)
    out = ops.prompt_loss(xd, e.to(DEV), w, stop)
    (gd,) = torch.autograd.grad(out, xd)
    assert abs(out.item() - ref.item()) < 1e-5 * max(1.0, abs(ref.item()))
    assert rel_l2(gd, gref) < 1e-4, rel_l2(gd, gref)


def test_adam_clamp_vs_torch():
    g = torch.Generator().manual_seed(3)
    z0 = torch.randn(1, 256, 16, 16, generator=g)
    zmin = -torch.rand(256, generator=g) - 0.5
    zmax = torch.rand(256, generator=g) + 0.5
    zr = z0.clone().requires_grad_(True)
    opt = torch.optim.Adam([zr], lr=0.2)
    zd = z0.to(DEV).clone()
    m = torch.zeros_like(zd)
    v = torch.zeros_like(zd)
    for step in range(1, 6):
        grad = torch.randn(1, 256, 16, 16, generator=g)
        zr.grad = grad.clone()
        opt.step()
        with torch.no_grad():
            zr.copy_(zr.maximum(zmin[None, :, None, None]).minimum(zmax[None, :, None, None]))
        ops.adam_clamp_step(zd, m, v, grad.to(DEV), zmin.to(DEV), zmax.to(DEV), 0.2, step)
    # fp32 Adam: identical formula up to fused-multiply rounding
    assert (zd.cpu() - zr.detach()).abs().max().item() < 2e-6


# ------------------------------------------------------------------------------------------ VQ
def test_vq_nearest_vs_oracle():
    g = torch.Generator().manual_seed(11)
    NC, D, P = 16384, 256, 256
    cb = torch.randn(NC, D, generator=g)
    z = torch.randn(1, D, 16, 16, generator=g)
    x = z.movedim(1, 3).reshape(P, D)
    idx_ref, d = vqgan_ref.vq_indices(x, cb)
    cbd, zd = cb.to(DEV), z.to(DEV)
    cn = torch.empty(NC, device=DEV)
    call("prx_k_sqnorm_rows", cbd, cn, NC, D, ops._stream())
    nt = (NC + 63) // 64
    pmin = torch.empty(P, nt, device=DEV)
    pidx = torch.empty(P, nt, device=DEV, dtype=torch.int32)
    idx = torch.empty(P, device=DEV, dtype=torch.int32)
    zq = torch.empty(P, D, device=DEV)
    call("prx_k_vq_nearest", zd, 1, P, cbd, cn, P, NC, D, pmin, pidx, idx, zq, ops._stream())
    idx = idx.cpu().long()
    # integer output: EXACT.  The only admissible deviation is a near-tie, defined without reference to either fp32
    # implementation (oracle/vqgan_ref.py vq_exactness): positions whose two smallest FLOAT64 distances differ by less than
    # the fp32 rounding of the distance expression.  Outside that set the kernel must pick the float64 argmin; inside it, one
    # of the tied codes.
    bad, near, differs = vqgan_ref.vq_exactness(x, cb, idx)
    bad_ref, _, differs_ref = vqgan_ref.vq_exactness(x, cb, idx_ref)
    assert near <= 4, near                                         # ties are rare: the test is about exactness
    assert bad == 0 and bad_ref == 0, (bad, bad_ref)               # the fp32 oracle obeys the same rule
    print("vq: near-tie positions", near, "kernel != f64 argmin at", differs, "oracle != f64 argmin at", differs_ref)
    assert torch.equal(zq.cpu(), cb[idx])


# ------------------------------------------------------------------------------------------ CLIP tower
def _clip_case(name, n, seed):
    cfg = weights.CLIP_CONFIGS[name]
    params = weights.synthetic_clip_vit_params(cfg, seed)
    g = torch.Generator().manual_seed(seed + 1)
    cut = torch.rand(n, 3, cfg.input_resolution, cfg.input_resolution, generator=g) * 1.2 - 0.1
    gout = torch.randn(n, cfg.output_dim, generator=g)
    cr = cut.clone().requires_grad_(True)
    ref = clip_vit_ref.encode_image(params, cr, patch=cfg.patch_size, heads=cfg.heads, layers=cfg.layers)
    (gref,) = torch.autograd.grad(ref, cr, gout)
    h = ops.ClipVitHandle(cfg, params, max_batch=n, device=DEV)
    cd = cut.to(DEV).requires_grad_(True)
    out = ops.clip_encode_image(cd, h)
    (gd,) = torch.autograd.grad(out, cd, gout.to(DEV))
    return ref, out, gref, gd


weights.CLIP_CONFIGS.setdefault("test-B/16", weights.ClipVitConfig("test-B/16", 224, 16, 256, 2, 4, 128))   # 197 tokens
weights.CLIP_CONFIGS.setdefault("test-L/14", weights.ClipVitConfig("test-L/14", 224, 14, 256, 2, 4, 128))   # 257 tokens, K=588


@pytest.mark.parametrize("name,n", [("tiny-B/32", 4), ("ViT-B/32", 8), ("test-B/16", 3), ("test-L/14", 2)])
def test_clip_vit_vs_oracle(name, n):
    ref, out, gref, gd = _clip_case(name, n, 5)
    # gates at the stated fast-mode figures or tighter (measured in round 6, IEEE-half operands and streams: embeddings 5.7e-4 ...
    # 1.1e-3, gradient 3.6e-4 ... 4.3e-3, cosines 1 - 1e-6)
    assert rel_l2(out, ref) < 5e-3, rel_l2(out, ref)
    assert cosine(out, ref) > 0.9999
    assert rel_l2(gd, gref) < 2e-2, rel_l2(gd, gref)
    assert cosine(gd, gref) > 0.9999


def perceptor_preprocess_checks():
    """CLIP_Base.preprocess / encode_image(apply_preprocess=False) (slip.py:58-66): preprocessing once and encoding without it gives
    the embeddings -- and the image gradient -- of the fused default path; a given input_range replaces the batch's min / max;
    a non-square, larger image is resized on its shorter side and centre-cropped"""
    from pixray_amd.perceptor import get_clip_perceptor
    perc = get_clip_perceptor("tiny-B/32", DEV, max_batch=4, precision="f32")
    R = perc.input_resolution
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(3, 3, R, R, generator=g) * 1.7 - 0.3).to(DEV).requires_grad_(True)
    gout = torch.randn(3, perc.output_dim, generator=g).to(DEV)
    e0 = perc.encode_image(x)
    (g0,) = torch.autograd.grad(e0, x, gout)
    p = perc.preprocess(x)
    lo, hi = float(x.detach().min()), float(x.detach().max())
    mean = torch.tensor(perc.CLIP_MEAN, device=DEV).view(1, 3, 1, 1); std = torch.tensor(perc.CLIP_STD, device=DEV).view(1, 3, 1, 1)
    assert torch.allclose(p, ((x - lo) / (hi - lo) - mean) / std, atol=1e-6)          # slip.py:21-42 + Normalize, literally
    e1 = perc.encode_image(p, apply_preprocess=False)
    (g1,) = torch.autograd.grad(e1, x, gout)
    assert rel_l2(e1, e0) < 1e-5, rel_l2(e1, e0)
    # gradient: the default path also differentiates the batch min / max (two pixels); through preprocess() autograd carries them
    assert rel_l2(g1, g0) < 1e-4, rel_l2(g1, g0)
    p2 = perc.preprocess(x.detach(), input_range=(-0.5, 2.0))
    assert torch.allclose(p2, ((x.detach() + 0.5) / 2.5 - mean) / std, atol=1e-6)
    big = torch.rand(2, 3, 2 * R, 3 * R, generator=g).to(DEV)
    pb = perc.preprocess(big)
    assert pb.shape == (2, 3, R, R) and torch.isfinite(perc.encode_image(pb, apply_preprocess=False)).all()


def test_perceptor_preprocess_and_apply_preprocess_false():
    perceptor_preprocess_checks()


def gumbel_vq_encode_checks():
    """VqganDrawer.init_from_tensor / get_z_from_tensor on a GumbelVQ checkpoint (vqgan.py:149-153, 174-185): taming's
    GumbelQuantize in eval mode = codebook[argmax(proj(h) + Gumbel noise)] with F.gumbel_softmax's own noise draw -- the same
    codes as that expression evaluated in torch on the runner's pre-quantisation latent under the same generator state"""
    import types
    from pixray_amd.vqgan_drawer import VqganDrawer
    cfg = weights.VQGAN_CONFIGS["tiny_f4"]
    sd = dict(weights.synthetic_vqgan_params(cfg, 2))
    sd.update(weights.synthetic_vqgan_encoder_params(cfg, 2, codebook=sd["quantize.embedding.weight"]))
    g = torch.Generator().manual_seed(8)
    sd["quantize.proj.weight"] = torch.randn(cfg.n_embed, cfg.embed_dim, 1, 1, generator=g) * 3.0
    sd["quantize.proj.bias"] = torch.randn(cfg.n_embed, generator=g)
    st = types.SimpleNamespace(vqgan_model="tiny_f4", size=(32, 32), vqgan_state_dict=sd, vqgan_gumbel=True, precision="f32")
    dr = VqganDrawer(st)
    dr.load_model(st, DEV)
    img = (torch.rand(1, 3, 32, 32, generator=g) * 2 - 1).to(DEV)
    torch.manual_seed(77)
    dr.init_from_tensor(img)
    z = dr.z.detach().clone()
    assert z.shape == (1, cfg.embed_dim, 8, 8) and dr.z.requires_grad
    # the reference expression on the same latent, same generator state
    _, _, pre = ops.vqgan_encode(img, dr._encoder(), return_pre=True)
    torch.manual_seed(77)
    logits = F.conv2d(pre, sd["quantize.proj.weight"].to(DEV), sd["quantize.proj.bias"].to(DEV))
    one_hot = F.gumbel_softmax(logits, tau=1.0, dim=1, hard=True)
    z_ref = torch.einsum("bnhw,nd->bdhw", one_hot, sd["quantize.embedding.weight"].to(DEV))
    assert torch.equal(dr.last_encode_indices.long().cpu(), one_hot.argmax(1).reshape(-1).cpu())
    assert torch.allclose(z, z_ref, atol=1e-6)
    out = dr.synth(0)                                   # ... and the drawer decodes from it
    assert out.shape == (1, 3, 32, 32) and torch.isfinite(out).all()
    st2 = types.SimpleNamespace(vqgan_model="tiny_f4", size=(32, 32), vqgan_gumbel=True,
                                vqgan_state_dict={k: v for k, v in sd.items() if not k.startswith("quantize.proj")})
    d2 = VqganDrawer(st2); d2.load_model(st2, DEV)
    with pytest.raises(KeyError, match="quantize.proj"):
        d2.init_from_tensor(img)


def test_gumbel_vq_checkpoints_encode_images():
    gumbel_vq_encode_checks()


def vit_switch_ab(env_name, precision, name="tiny-B/32", n=4):
    """one image tower (ViT, or ModifiedResNet for the "*RN*" configs) forward + gradient with a debug switch of the runner
    off and on (read at handle creation): (embeddings, gradient) of both runs"""
    resnet = name in weights.CLIP_RESNET_CONFIGS
    cfg = weights.CLIP_RESNET_CONFIGS[name] if resnet else weights.CLIP_CONFIGS[name]
    params = weights.synthetic_clip_resnet_params(cfg, 5) if resnet else weights.synthetic_clip_vit_params(cfg, 5)
    g = torch.Generator().manual_seed(6)
    cut = torch.rand(n, 3, cfg.input_resolution, cfg.input_resolution, generator=g)
    gout = torch.randn(n, cfg.output_dim, generator=g)
    res = []
    old = os.environ.get(env_name)
    try:
        for val in ("0", "1"):
            os.environ[env_name] = val
            h = (ops.ClipResNetHandle if resnet else ops.ClipVitHandle)(cfg, params, max_batch=n, device=DEV, precision=precision)
            cd = cut.to(DEV).requires_grad_(True)
            out = ops.clip_encode_image(cd, h)
            (gd,) = torch.autograd.grad(out, cd, gout.to(DEV))
            res.append((out.detach().float().cpu(), gd.detach().float().cpu()))
    finally:
        if old is None:
            os.environ.pop(env_name, None)
        else:
            os.environ[env_name] = old
    return res


def test_vit_class_token_tail_is_the_same_tower():
    """PRX_VIT_CLS_TAIL=0 runs the last block on every token row, the default only on the class-token rows that ln_post reads:
    the same embeddings and the same gradient, to fp32 round-off in the exact-f32 mode (other tile shapes sum K in another
    order) and to 16-bit operand rounding in the half mode"""
    (e0, g0), (e1, g1) = vit_switch_ab("PRX_VIT_CLS_TAIL", "f32")
    assert rel_l2(e1, e0) < 2e-6 and rel_l2(g1, g0) < 2e-5, (rel_l2(e1, e0), rel_l2(g1, g0))
    (e0, g0), (e1, g1) = vit_switch_ab("PRX_VIT_CLS_TAIL", "fp16")
    assert rel_l2(e1, e0) < 2e-3 and rel_l2(g1, g0) < 5e-3, (rel_l2(e1, e0), rel_l2(g1, g0))


def test_vit_lean_streams_ab():
    """PRX_LEAN=0 (fp32 residual / gradient streams with 16-bit twins) against the half mode's default (streams in IEEE half
    only): the bisection switch of the lean layout keeps working, and the two layouts differ by stream rounding only"""
    (e0, g0), (e1, g1) = vit_switch_ab("PRX_LEAN", "fp16")
    assert rel_l2(e1, e0) < 3e-3 and rel_l2(g1, g0) < 1e-2, (rel_l2(e1, e0), rel_l2(g1, g0))
    assert not torch.equal(e0, e1)


def test_resnet_lean_streams_ab():
    """PRX_RN_LEAN=0 (fp32 Bottleneck residual stream / gradient with 16-bit twins) against the half mode's default (both in
    IEEE half only, resnet.hip): the bisection switch keeps working and the layouts differ by stream rounding (plus the ReLU
    masks that rounding flips) only; the bf16 mode has no lean layout, so there the switch changes nothing at all"""
    (e0, g0), (e1, g1) = vit_switch_ab("PRX_RN_LEAN", "fp16", name="tiny-RN", n=3)
    assert rel_l2(e1, e0) < 3e-3 and rel_l2(g1, g0) < 3e-2 and cosine(g1, g0) > 0.9995, (rel_l2(e1, e0), rel_l2(g1, g0))
    assert not torch.equal(e0, e1)
    (e0, g0), (e1, g1) = vit_switch_ab("PRX_RN_LEAN", "bf16", name="tiny-RN", n=3)
    assert torch.equal(e0, e1) and torch.equal(g0, g1)


# ------------------------------------------------------------------------------------------ VQGAN
def _vqgan_case(name, hw, seed):
    cfg = weights.VQGAN_CONFIGS[name]
    params = weights.synthetic_vqgan_params(cfg, seed)
    g = torch.Generator().manual_seed(seed + 1)
    hh, ww = (hw, hw) if isinstance(hw, int) else hw
    z = torch.randn(1, cfg.z_channels, hh, ww, generator=g)
    f = 2 ** (len(cfg.ch_mult) - 1)
    gimg = torch.randn(1, 3, hh * f, ww * f, generator=g)
    zr = z.clone().requires_grad_(True)
    ref = vqgan_ref.synth(params, zr, cfg.oracle_cfg())
    (gref,) = torch.autograd.grad(ref, zr, gimg)
    h = ops.VqganHandle(cfg, params, (hh, ww), DEV)
    zd = z.to(DEV).requires_grad_(True)
    out = ops.vqgan_synth(zd, h)
    (gd,) = torch.autograd.grad(out, zd, gimg.to(DEV))
    idx_ref, _ = vqgan_ref.vq_indices(z.movedim(1, 3).reshape(hh * ww, -1), params["quantize.embedding.weight"])
    return ref, out, gref, gd, idx_ref, h.last_indices.cpu().long()


@pytest.mark.parametrize("name,hw", [("tiny_f4", 16), ("imagenet_f16_16384", 16),
                                     ("imagenet_f16_16384", 32),         # 32: the 512x512 decoder of BASELINE.json configs[2]
                                     ("tiny_f4", (12, 20)), ("imagenet_f16_16384", (14, 25))])   # pixray sizes are rarely square
def test_vqgan_synth_vs_oracle(name, hw):
    ref, out, gref, gd, idx_ref, idx = _vqgan_case(name, hw, 9)
    assert torch.equal(idx, idx_ref), "VQ code selection differs"
    assert out.shape == ref.shape
    # image in [0,1]: IEEE-half operand rounding through ~60 layers.  Gates at SURVEY 8(d)'s stated fast-mode figures or tighter
    # (measured in round 6: image rel-L2 4.8e-4 ... 5.6e-4, gradient 1.5e-3 ... 6.1e-3, cosine >= 0.99998)
    assert (out.cpu() - ref.detach()).abs().mean().item() < 1e-3
    assert rel_l2(out, ref) < 2e-3, rel_l2(out, ref)
    assert rel_l2(gd, gref) < 2e-2, rel_l2(gd, gref)
    assert cosine(gd, gref) > 0.9999


def test_a_latent_that_cannot_be_allocated_is_an_error_with_the_figure():
    """the decoder allocates one forward's activations for its latent size when it is created.  tiny_f4 at a 44300 x 44300 latent:
    1 962 490 000 positions (below 2^31, and create forms the product in size_t: `(size_t)rh * rw`), so the first stream request --
    the first ResBlock's h1, positions x 256 channels of 2-byte (lean half) elements -- is 1 004 794 880 000 bytes, over three times
    the card's memory: the runtime refuses it with only the codebook and three weight packs held.  PrxError with the bytes asked
    for and the bytes held, the partly built handle freed; the 4 x 4 handle made next runs forward and backward as usual."""
    import re
    from pixray_amd._lib import PrxError
    cfg = weights.VQGAN_CONFIGS["tiny_f4"]
    params = weights.synthetic_vqgan_params(cfg, 0)
    with pytest.raises(PrxError, match=r"device allocation of \d+ bytes failed .* with \d+ bytes already held") as ei:
        ops.VqganHandle(cfg, params, (44300, 44300), DEV)
    asked = int(re.search(r"device allocation of (\d+) bytes", str(ei.value)).group(1))
    assert asked >= 10 ** 12 and asked % (44300 * 44300 * 256) == 0, asked          # 2 bytes per element (4 with PRX_LEAN=0)
    if DEV == "cuda":
        torch.cuda.synchronize()
    h = ops.VqganHandle(cfg, params, (4, 4), DEV)
    z = torch.randn(1, cfg.z_channels, 4, 4, device=DEV).requires_grad_(True)
    img = ops.vqgan_synth(z, h)
    (dz,) = torch.autograd.grad(img.sum(), z)
    assert bool(torch.isfinite(img).all()) and bool(torch.isfinite(dz).all())


# ------------------------------------------------------------------------------------------ VQGAN encoder
@pytest.mark.parametrize("name,HW", [("tiny_f4", (64, 64)), ("tiny_f4", (32, 96)), ("tiny_f4", (40, 56)),   # 140 tokens: not a multiple of 8
                                     ("imagenet_f16_16384", (256, 256))])
def test_vqgan_encode_vs_oracle(name, HW):
    """VqganDrawer.init_from_tensor's `model.encode` (vqgan.py:174-176): taming Encoder -> quant_conv -> nearest code.
    bf16-operand engine vs the fp32 oracle: the pre-quantisation latent within 2e-2 rel-L2; the chosen codes are exact
    integer work GIVEN the latent, so wherever they differ from the oracle's the two candidates must be a near-tie in
    the oracle's own distances."""
    cfg = weights.VQGAN_CONFIGS[name]
    p = weights.synthetic_vqgan_encoder_params(cfg, seed=5)
    eh = ops.VqganEncHandle(cfg, p, HW, DEV)
    g = torch.Generator().manual_seed(11)
    low = torch.rand(1, 3, HW[0] // 8, HW[1] // 8, generator=g)
    img = (torch.nn.functional.interpolate(low, size=HW, mode="bilinear", align_corners=False)
           + 0.05 * torch.randn(1, 3, *HW, generator=g)).clamp(0, 1) * 2 - 1
    z, idx, pre = ops.vqgan_encode(img.to(DEV), eh, return_pre=True)
    with torch.no_grad():
        z_ref, idx_ref, pre_ref = vqgan_ref.encode(p, img, cfg.oracle_cfg())
    f = 2 ** (len(cfg.ch_mult) - 1)
    assert z.shape == (1, cfg.embed_dim, HW[0] // f, HW[1] // f)
    assert rel_l2(pre, pre_ref) < 2e-2, rel_l2(pre, pre_ref)
    cb = p["quantize.embedding.weight"]
    idx = idx.cpu().long()
    # the output IS codebook rows (bit-exact gather)
    assert torch.equal(z.cpu().movedim(1, 3).reshape(-1, cfg.embed_dim), cb[idx])
    # the kernel's argmin is exact for ITS latent (first-index ties, same distance formula as vqgan.py:60-64)
    own, _ = vqgan_ref.vq_indices(pre.cpu().movedim(1, 3), cb)
    assert (own.reshape(-1) == idx).float().mean().item() > 0.995
    agree = (idx == idx_ref).float().mean().item()
    d = (pre_ref.movedim(1, 3).reshape(-1, 1, cfg.embed_dim) - cb[None]).pow(2).sum(-1)       # oracle distances
    chosen = d.gather(1, idx[:, None])[:, 0]
    best = d.min(dim=1).values
    assert agree > 0.7, agree
    assert ((chosen - best) / best).max().item() < 3e-2, ((chosen - best) / best).max().item()


def test_vqgan_encoder_independent_golden():
    """the committed HF JanusVQVAEEncoder fixture (tests/golden/encoder_golden.npz) through the HIP encoder"""
    import os, sys
    import numpy as np
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "golden"))
    import make_golden as mg
    d = np.load(os.path.join(here, "golden", "encoder_golden.npz"))
    cfg = mg.GOLDEN_VQ
    p = dict(weights.synthetic_vqgan_encoder_params(cfg, int(d["seed"])))
    p["quant_conv.weight"] = torch.eye(cfg.z_channels).reshape(cfg.z_channels, cfg.z_channels, 1, 1)   # expose the encoder output
    p["quant_conv.bias"] = torch.zeros(cfg.z_channels)
    eh = ops.VqganEncHandle(cfg, p, (16, 16), DEV)
    _, _, pre = ops.vqgan_encode(torch.from_numpy(d["x"]).to(DEV), eh, return_pre=True)
    assert rel_l2(pre, torch.from_numpy(d["h"])) < 2e-2, rel_l2(pre, torch.from_numpy(d["h"]))


def test_vqgan_drawer_encoder_entry_points():
    """init_from_tensor / reapply_from_tensor / get_z_from_tensor (vqgan.py:174-185) on the drawer surface"""
    import types
    from pixray_amd.vqgan_drawer import VqganDrawer
    s = types.SimpleNamespace(vqgan_model="tiny_f4", size=(64, 64))
    dr = VqganDrawer(s)
    dr.load_model(s, DEV)
    g = torch.Generator().manual_seed(2)
    img = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1
    dr.init_from_tensor(img)
    z = dr.get_z()
    assert z.is_leaf and z.requires_grad and z.shape == (1, dr.cfg.z_channels, 16, 16)
    z_ref = dr.get_z_from_tensor(img)
    assert torch.equal(z.detach(), z_ref)                       # same image -> same codes
    out = dr.synth(0)                                           # an encoded z is a fixed point of the quantiser
    assert torch.equal(dr.handle.last_indices.cpu(), dr.last_encode_indices.cpu())
    out.sum().backward()
    assert z.grad is not None and torch.isfinite(z.grad).all()
    img2 = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1
    zid = id(dr.get_z())
    dr.reapply_from_tensor(img2)
    assert id(dr.get_z()) == zid and not torch.equal(dr.get_z().detach(), z_ref)     # in place, as `self.z.copy_(new_z)`
    with pytest.raises(ValueError):
        dr.init_from_tensor(torch.zeros(1, 4, 64, 64))


# ------------------------------------------------------------------------------------------ CLIP text tower
def _tokens(cfg, n, seed):
    g = torch.Generator().manual_seed(seed)
    tk = torch.zeros(n, cfg.context_length, dtype=torch.long)
    for i in range(n):
        L = int(torch.randint(1, cfg.context_length - 2, (1,), generator=g)) if i else cfg.context_length - 2   # row 0: full length
        tk[i, 0] = cfg.vocab_size - 2
        tk[i, 1:1 + L] = torch.randint(1, cfg.vocab_size - 2, (L,), generator=g)
        tk[i, 1 + L] = cfg.vocab_size - 1
    return tk


@pytest.mark.parametrize("name,n", [("tiny-B/32", 5), ("ViT-B/32", 3), ("ViT-L/14", 2)])
def test_clip_text_tower_vs_oracle(name, n):
    """CLIP_Base.encode_text (slip.py:68-70) on token ids: causal transformer, EOT pooling, projection.  bf16 operands vs
    the fp32 oracle: 2e-2 rel-L2 / cosine 0.999 per embedding (same tolerance as the image tower)."""
    import dataclasses
    from oracle import clip_text_ref
    cfg = weights.CLIP_TEXT_CONFIGS[name]
    if cfg.layers > 4:
        cfg = dataclasses.replace(cfg, layers=4)          # keep the CPU oracle's share short; same operators
    p = weights.synthetic_clip_text_params(cfg, seed=9)
    h = ops.ClipTextHandle(cfg, p, max_batch=8, device=DEV)
    tk = _tokens(cfg, n, 13)
    e = ops.clip_encode_text_tokens(tk, h)
    with torch.no_grad():
        ref = clip_text_ref.text_forward(p, tk, heads=cfg.heads, layers=cfg.layers)
    assert e.shape == (n, cfg.output_dim)
    assert rel_l2(e, ref) < 2e-2, rel_l2(e, ref)
    for i in range(n):
        assert cosine(e[i], ref[i]) > 0.999
    # causality: tokens after the EOT position cannot change the embedding
    tk2 = tk.clone()
    eot = int(tk2[1].argmax())
    tk2[1, eot + 1:] = 7
    e2 = ops.clip_encode_text_tokens(tk2, h)
    assert torch.equal(e2[1], e[1])
    with pytest.raises(ValueError):
        ops.clip_encode_text_tokens(torch.full((1, cfg.context_length), cfg.vocab_size), h)


def test_clip_text_independent_golden_and_perceptor_surface():
    """the committed HF CLIPTextModelWithProjection fixture through the HIP text tower, and the perceptor's
    encode_text / encode_texts entry points (slip.py:68-74)"""
    import os, sys
    import numpy as np
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "golden"))
    import make_golden as mg
    d = np.load(os.path.join(here, "golden", "clip_text_golden.npz"))
    cfg = mg.GOLDEN_TEXT
    p = weights.synthetic_clip_text_params(cfg, int(d["seed"]))
    h = ops.ClipTextHandle(cfg, p, max_batch=8, device=DEV)
    e = ops.clip_encode_text_tokens(torch.from_numpy(d["tokens"]), h)
    assert rel_l2(e, torch.from_numpy(d["emb"])) < 2e-2, rel_l2(e, torch.from_numpy(d["emb"]))

    from pixray_amd.perceptor import get_clip_perceptor
    from pixray_amd.prompt import Prompt
    from pixray_amd.tokenizer import BpeTokenizer
    tok = BpeTokenizer([("t", "h"), ("th", "e</w>"), ("c", "a"), ("ca", "t</w>")])
    tcfg = weights.ClipTextConfig("tiny-B/32", vocab_size=tok.vocab_size, width=256, layers=2, heads=4, output_dim=128)
    perc = get_clip_perceptor("tiny-B/32", DEV, max_batch=4, tokenizer=tok)
    perc.text_cfg = tcfg
    emb = perc.encode_text("the cat")
    assert emb.shape == (1, 128) and emb.dtype == torch.float32 and emb.is_cuda
    assert torch.equal(emb, perc.encode_text(tok.tokenize("The  CAT")))
    both = perc.encode_texts(["the cat", "cat the"])
    assert both.shape == (2, 1, 128) and torch.allclose(both.norm(dim=-1), torch.ones(2, 1, device=DEV), atol=1e-5)
    # the text embedding drives a Prompt against image embeddings of the same perceptor (pixray.py:873-877, 1297-1299)
    img = torch.rand(2, 3, 224, 224, device=DEV, requires_grad=True)
    loss = Prompt(emb, 1.0, float("-inf")).to(DEV)(perc.encode_image(img).float())
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(img.grad).all()


# ------------------------------------------------------------------------------------------ cached cutout transforms (a6)
@pytest.mark.parametrize("it", [0, 1])
def test_make_cutouts_cached_transform_path_vs_oracle(it):
    """pixray.py:480-486: a second MakeCutouts call inside one iteration (image prompts, pixray.py:1318-1333) re-uses the
    iteration's composed 3x3 transforms in ONE warp (kornia default align_corners=True), zoom set with the iteration's
    reflection (even) / border (odd) padding, wide set gray-filled, no ColorJitter.  fp32 gather: 1e-4-class."""
    cutn, S, HW = 10, 224, 256
    g = torch.Generator().manual_seed(40 + it)
    img = _test_image("smooth", HW, g)
    target = _test_image("smooth", HW, g)
    prm = pc.sample_cutout_params(cutn, S, g, iteration=it, noise_fac=0.0)
    mk = pc.MakeCutouts(S, cutn, noise_fac=0.0)
    mk.fixed_params = prm
    mk.iteration = it
    live = mk(img.to(DEV))
    assert mk.transforms is not None
    cached = mk(target.to(DEV))
    ref_live = cutouts_ref.make_cutouts(img, prm, S)
    ref_cached = cutouts_ref.make_cutouts_cached(target, prm, S)
    assert rel_l2(live, ref_live) < 1e-4
    assert rel_l2(cached, ref_cached) < 1e-4, rel_l2(cached, ref_cached)
    assert (cached.cpu() - ref_cached).abs().max().item() < 5e-3
    # and it is a different resampling from the live path of the same image (single warp, no jitter)
    assert rel_l2(mk(img.to(DEV)), ref_live) > 1e-3
    mk.transforms = None                                   # what the loop does at the end of every iteration
    assert rel_l2(mk(img.to(DEV)), ref_live) < 1e-4


# ------------------------------------------------------------------------------------------ CLIP ModifiedResNet
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("name,n", [("tiny-RN", 3), ("RN50x4", 2)])
def test_clip_resnet_vs_oracle(name, n, precision):
    """CLIP_Base.encode_image with a ModifiedResNet tower (RN50x4 = BASELINE.json configs[2]): preprocessing, stem,
    bottlenecks with folded BatchNorm, attention pool, forward and the gradient w.r.t. the cutouts.  bf16 operands vs
    the fp32 oracle (which is restated from the published architecture: parity unpinned)."""
    from oracle import clip_resnet_ref
    cfg = weights.CLIP_RESNET_CONFIGS[name]
    p = weights.synthetic_clip_resnet_params(cfg, seed=3)
    h = ops.ClipResNetHandle(cfg, p, max_batch=4, device=DEV, precision=precision)
    g = torch.Generator().manual_seed(17)
    R = cfg.input_resolution
    low = torch.rand(n, 3, R // 8, R // 8, generator=g)
    cut = (torch.nn.functional.interpolate(low, size=(R, R), mode="bilinear", align_corners=False)
           + 0.05 * torch.randn(n, 3, R, R, generator=g))
    ge = torch.randn(n, cfg.output_dim, generator=g)
    cr = cut.clone().requires_grad_(True)
    ref = clip_resnet_ref.encode_image(p, cr, layers=cfg.layers, heads=cfg.heads)
    (gref,) = torch.autograd.grad(ref, cr, ge)
    cd = cut.to(DEV).requires_grad_(True)
    emb = ops.clip_encode_image(cd, h)
    (gd,) = torch.autograd.grad(emb, cd, ge.to(DEV))
    assert emb.shape == (n, cfg.output_dim)
    assert rel_l2(emb, ref) < 2e-2, rel_l2(emb, ref)
    for i in range(n):
        assert cosine(emb[i], ref[i]) > 0.999
    # gradient: bf16 roundings through up to 80 layers, and every pre-activation that bf16 moves across zero flips a
    # ReLU mask (a discrete change of the gradient path; the reference's own fp16 CUDA tower behaves the same way).
    # The two elements that hold the batch-global min and max of the cutouts (slip.py:21-36) receive the SUMS of the whole
    # batch's gradient through the renormalisation -- two entries that can be a fifth of one cutout's gradient norm and carry
    # the few-% error of a bf16 sum over 5e5 terms; they are checked on their own, the other entries as the bulk
    # (tools/f32_error_budget.py; the exact-f32 mode agrees on all of them to 4e-5, tests/test_f32_mode_gpu.py).
    flat = cut.flatten()
    ext = torch.stack([flat.argmin(), flat.argmax()])
    bulk_d, bulk_r = gd.detach().cpu().flatten().clone(), gref.flatten().clone()
    ext_d, ext_r = bulk_d[ext].clone(), bulk_r[ext].clone()
    bulk_d[ext] = 0.0; bulk_r[ext] = 0.0
    print(name, precision, "emb rel", rel_l2(emb, ref), "grad rel", rel_l2(gd, gref), "grad cos", cosine(gd, gref),
          "| bulk rel", rel_l2(bulk_d, bulk_r), "bulk cos", cosine(bulk_d, bulk_r), "| min/max entries", ext_d.tolist(), ext_r.tolist())
    # gates = measured values + margin (tiny-RN: few channels, the bf16 noise of a product does not average out; RN50x4:
    # wide layers).  They are bf16-operand noise, not a modelling difference: the exact-f32 mode of the same code meets 1e-4
    # on every entry (tests/test_f32_mode_gpu.py::test_clip_resnet_f32_mode_vs_float64_oracle).
    # measured: tiny-RN bulk 0.119 / 0.9929, RN50x4 bulk 0.155 / 0.9880 (total incl. the min/max entries 0.014 / 0.177)
    # fp16 (the product default, the reference's own arithmetic for this tower on a GPU), measured: tiny-RN bulk 1.6e-2 / 0.99987,
    # RN50x4 bulk 5.2e-2 / 0.99865 (3x closer than bf16; what is left are ReLU-mask flips of ~80 layers, which a 16-bit
    # activation format cannot avoid).  The end-to-end gradient of configs[2] -- this tower + ViT-B/16 through the decoder --
    # meets the stated 2e-2 / 0.999 with room (5.9e-3 at 16 cutouts, 1.7e-3 at 128: tests/test_e2e_gpu.py, test_fullsize_gpu.py)
    tol_rel, tol_cos = (7e-2, 0.998) if precision == "fp16" else (2e-1, 0.98)
    assert rel_l2(gd, gref) < 2e-1 and cosine(gd, gref) > 0.999, (rel_l2(gd, gref), cosine(gd, gref))
    assert rel_l2(bulk_d, bulk_r) < tol_rel, rel_l2(bulk_d, bulk_r)
    assert cosine(bulk_d, bulk_r) > tol_cos, cosine(bulk_d, bulk_r)
    # heavily cancelling sums: a quarter of their value is the bf16 noise of the terms (f32 mode: 1e-4)
    assert ((ext_d - ext_r).abs() <= 0.3 * ext_r.abs() + 1e-3 * gref.abs().max()).all(), (ext_d, ext_r)


# ------------------------------------------------------------------------------------------ non-square canvases (a6)
@pytest.mark.parametrize("H,W,S,it", [(144, 256, 224, 0), (144, 256, 224, 1), (256, 144, 224, 0), (64, 112, 64, 1)])
def test_make_cutouts_non_square_canvas_vs_oracle(H, W, S, it):
    """pixray.py:420-431, 468-472: on a W != H canvas the pooled cutout is rescaled to the canvas aspect, the zoom set is
    warped / cropped inside that rectangle, and the wide set shrinks the whole rectangle (scale U(.9,1)/aspect, shift along
    the short axis), takes the centred S x S crop and then the padded perspective.  Live and cached paths, forward and the
    gradient w.r.t. the canvas."""
    cutn = 10
    aspect = W / H
    g = torch.Generator().manual_seed(300 + H + it)
    low = torch.rand(1, 3, max(H // 8, 4), max(W // 8, 4), generator=g)
    img = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    target = torch.rand(1, 3, H, W, generator=g)
    prm = pc.sample_cutout_params(cutn, S, g, iteration=it, aspect=aspect)
    prm["noise"] = torch.randn(cutn, 3, S, S, generator=g)
    Hb, Wb = pc.base_size(S, aspect)
    assert (Hb == S) != (Wb == S) and (Wb > S if aspect > 1 else Hb > S)
    img_ref = img.clone().requires_grad_(True)
    ref = cutouts_ref.make_cutouts(img_ref, prm, S)
    gout = torch.randn(cutn, 3, S, S, generator=g)
    (gref,) = torch.autograd.grad(ref, img_ref, gout)
    mk = pc.MakeCutouts(S, cutn, aspect_width=aspect)
    mk.fixed_params = prm
    mk.iteration = it
    img_d = img.to(DEV).requires_grad_(True)
    out = mk(img_d)
    assert out.shape == (cutn, 3, S, S)
    assert (out.detach().cpu() - ref.detach()).abs().max().item() < 2e-4
    assert rel_l2(out, ref) < 2e-5, rel_l2(out, ref)
    (gd,) = torch.autograd.grad(out, img_d, gout.to(DEV))
    assert rel_l2(gd, gref) < 3e-3, rel_l2(gd, gref)
    assert cosine(gd, gref) > 0.99999
    # cached-transform path on the same iteration's geometry (image prompts)
    mk.noise_fac = 0.0
    cached = mk(target.to(DEV))
    ref_cached = cutouts_ref.make_cutouts_cached(target, prm, S)
    assert rel_l2(cached, ref_cached) < 1e-4, rel_l2(cached, ref_cached)


def test_make_cutouts_spot_masks_vs_oracle():
    """spot prompts (pixray.py:453-466, 1270-1292): the pooled cutout is blanked inside (spot=1) or outside (spot=0) the
    spot mask before the augmentations; the calls come after the iteration's first MakeCutouts call, i.e. through the
    cached transforms"""
    cutn, S, HW = 10, 64, 96
    g = torch.Generator().manual_seed(77)
    img = torch.rand(1, 3, HW, HW, generator=g)
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    inside = (((yy - S / 2) ** 2 + (xx - S / 2) ** 2) < (S / 4) ** 2)[None].expand(3, S, S).contiguous()
    prm = pc.sample_cutout_params(cutn, S, g, iteration=1, noise_fac=0.0)
    mk = pc.MakeCutouts(S, cutn, noise_fac=0.0)
    mk.fixed_params = prm
    mk.iteration = 1
    mk.spot_masks = (inside, ~inside)
    img_d = img.to(DEV).requires_grad_(True)
    live = mk(img_d)
    on = mk(img_d, spot=1)
    off = mk(img_d, spot=0)
    assert rel_l2(live, cutouts_ref.make_cutouts(img, prm, S)) < 1e-5
    assert rel_l2(on, cutouts_ref.make_cutouts_cached(img, prm, S, spot_mask=inside)) < 1e-4
    assert rel_l2(off, cutouts_ref.make_cutouts_cached(img, prm, S, spot_mask=~inside)) < 1e-4
    # masked pooled pixels are constants: no gradient reaches the canvas through them
    (g_on,) = torch.autograd.grad(on.sum(), img_d, retain_graph=True)
    imr = img.clone().requires_grad_(True)
    (g_ref,) = torch.autograd.grad(cutouts_ref.make_cutouts_cached(imr, prm, S, spot_mask=inside).sum(), imr)
    assert rel_l2(g_on, g_ref) < 1e-3, rel_l2(g_on, g_ref)
    # a live call with a mask (first call of an iteration) works too
    mk.transforms = None
    assert rel_l2(mk(img_d, spot=0), cutouts_ref.make_cutouts(img, prm, S, spot_mask=~inside)) < 1e-5
    mk2 = pc.MakeCutouts(S, cutn)
    with pytest.raises(ValueError):
        mk2(img_d, spot=1)


# ------------------------------------------------------------------------------------------ VGG16 extractor (StyleLoss plugin)
# Gates of the VGG16 extractor and of the STROTSS loss on top of it, per operand precision (features rel-L2, input-gradient
# rel-L2 / cosine).  The exact-f32 mode is the parity statement: fp32 round-off against the oracle.  The 16-bit modes are gated
# at their MEASURED values (tools/vgg_precision_probe.py, log committed as profiles/r04_vgg_precision_probe.txt): this probe
# differentiates random cotangents through 13 conv+ReLU layers of a seeded random network, where a pre-activation rounded
# across zero flips a ReLU mask -- fp16 0.9979..0.9983 / 5.8e-2..6.6e-2, bf16 0.984..0.986 / 0.17..0.18; end to end (configs[3]
# at its 256 cutouts WITH the StyleLoss term, tests/test_fullsize_gpu.py) the stated 2e-2 / 0.999 gate applies.
VGG_GATES = {"f32": dict(feat=1e-5, grad_rel=1e-4, grad_cos=0.9999999, strotss_val=1e-5, strotss_rel=1e-3, strotss_cos=0.999999),
             "fp16": dict(feat=2e-3, grad_rel=9e-2, grad_cos=0.997, strotss_val=1e-3, strotss_rel=1.6e-1, strotss_cos=0.99),
             "bf16": dict(feat=1.5e-2, grad_rel=2.5e-1, grad_cos=0.975, strotss_val=5e-3, strotss_rel=3.5e-1, strotss_cos=0.94)}


@pytest.mark.parametrize("precision", ["f32", "fp16", "bf16"])
@pytest.mark.parametrize("H,W", [(64, 48), (50, 70), (128, 128)])
def test_vgg16_features_and_input_gradient_match_the_oracle(H, W, precision):
    """the nine captured ReLU maps (Losses/StyleLoss.py:31) and d(sum_k <feat_k, r_k>)/dx against the fp32 oracle in all three
    operand precisions; odd sizes exercise the floor of the 2x2 pools"""
    from oracle import vgg_ref
    gate = VGG_GATES[precision]
    params = weights.synthetic_vgg16_params(0)
    handle = ops.Vgg16Handle(params, (128, 128), torch.device(DEV), precision=precision)
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(1, 3, H, W, generator=g) * 2 - 1)
    xn = vgg_ref.normalise(x)
    xo = xn.clone().requires_grad_(True)
    ref = vgg_ref.forward_base(params, xo)[1:]
    xd = xn.to(DEV).requires_grad_(True)
    got = ops.vgg16_features(xd, handle)
    assert len(got) == 9
    rs = []
    for k, (f, r) in enumerate(zip(got, ref)):
        assert tuple(f.shape) == (1, r.shape[2], r.shape[3], r.shape[1]), (k, f.shape, r.shape)
        assert rel_l2(f.permute(0, 3, 1, 2).cpu(), r.detach()) < gate["feat"], (k, rel_l2(f.permute(0, 3, 1, 2).cpu(), r.detach()))
        rs.append(torch.randn(r.shape, generator=g) / math.sqrt(r.numel()))
    sum((r_ * f_).sum() for r_, f_ in zip(rs, ref)).backward()
    sum((r_.permute(0, 2, 3, 1).to(DEV) * f_).sum() for r_, f_ in zip(rs, got)).backward()
    cs, rl = cosine(xd.grad.cpu(), xo.grad), rel_l2(xd.grad.cpu(), xo.grad)
    assert cs > gate["grad_cos"] and rl < gate["grad_rel"], (precision, cs, rl)
    # a gradient on one early feature only: the layers above it are skipped
    xd2 = xn.to(DEV).requires_grad_(True)
    f2 = ops.vgg16_features(xd2, handle)
    (rs[1].permute(0, 2, 3, 1).to(DEV) * f2[1]).sum().backward()
    xo.grad = None
    ref2 = vgg_ref.forward_base(params, xo)[1:]
    (rs[1] * ref2[1]).sum().backward()
    cs, rl = cosine(xd2.grad.cpu(), xo.grad), rel_l2(xd2.grad.cpu(), xo.grad)
    assert cs > max(gate["grad_cos"], 0.995) and rl < min(gate["grad_rel"], 8e-2), (precision, cs, rl)       # two conv layers + the mask flips of relu1_1


@pytest.mark.parametrize("precision", ["f32", "fp16", "bf16"])
def test_style_loss_on_the_hip_extractor_tracks_the_oracle_extractor(precision):
    """the StyleLoss plugin's STROTSS loss (arithmetic pinned to the reference's own code on CPU, tests/test_style_loss.py)
    with the HIP VGG16 extractor against the same plugin on the CPU oracle's features, same numpy seed -> same sampled
    positions.  Exact-f32 extractor: the value to 1e-5 and the image gradient to 1e-3 (measured 1.5e-7 / 1.7e-4: a handful of
    nearest-neighbour choices of the relaxed EMD sit on fp32 ties); 16-bit extractors at their measured values (VGG_GATES)."""
    import warnings
    import numpy as np
    from oracle import vgg_ref
    from pixray_amd import style_loss as sl
    gate = VGG_GATES[precision]
    params = weights.synthetic_vgg16_params(0)

    class OracleExtractor:
        def __call__(self, x):
            return [f.permute(0, 2, 3, 1).contiguous() for f in vgg_ref.forward(params, x, "uniform")]

        def forward_samples_hypercolumn(self, X, samps=100):
            return sl.sample_hypercolumns(self(X), samps)

    g = torch.Generator().manual_seed(17)
    img = torch.rand(1, 3, 96, 80, generator=g)
    style = torch.rand(1, 3, 96, 80, generator=g)
    a = img.clone().requires_grad_(True)
    b = img.clone().to(DEV).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        np.random.seed(3)
        la = sl.strotss_loss(a, style, 16.0, extractor=OracleExtractor())
        np.random.seed(3)
        lb = sl.strotss_loss(b, style.to(DEV), 16.0, extractor=sl.Vgg16Extractor(params=params, device=DEV, max_hw=(96, 80), precision=precision))
    (ga,) = torch.autograd.grad(la, a)
    (gb,) = torch.autograd.grad(lb, b)
    assert abs(float(la.detach()) - float(lb.detach())) < gate["strotss_val"] * abs(float(la.detach())), (float(la.detach()), float(lb.detach()))
    assert cosine(gb.cpu(), ga) > gate["strotss_cos"] and rel_l2(gb.cpu(), ga) < gate["strotss_rel"], (cosine(gb.cpu(), ga), rel_l2(gb.cpu(), ga))
