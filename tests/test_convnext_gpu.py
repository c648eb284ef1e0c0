"""OpenCLIP ConvNeXt perceptors on the HIP depthwise-conv runner (csrc/convnext.hip): the depthwise 7x7 kernel and its data gradient,
the space-to-depth permutation, the global average pool and the channel LayerNorm against float64; reduced towers against the
plain-torch restatement (tests/_convnext_ref.py, float64, unfolded layer scale); real widths; graph replay; refusals; one run through
the front end.  The check functions take their device from `DEV`, so tests/test_emu_convnext.py runs a subset on the CPU emulation.

Every test here fails on a tree without the feature (no prx_k_cnx_*, no CLIP_CONVNEXT_CONFIGS, no prx_clip_convnext_create)."""
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
from pixray_amd import _lib, ops, weights  # noqa: E402
from pixray_amd._lib import call  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32_GATE = 1e-4          # tests/test_f32_mode_gpu.py: the stated gate of the exact mode
# precision -> (PRX_PREC_* code, torch dtype, unit roundoff of the format)
PREC = {"fp16": (2, torch.float16, 2.0 ** -11), "bf16": (0, torch.bfloat16, 2.0 ** -8), "f32": (1, torch.float32, 2.0 ** -24)}


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def cosine(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-300)).item()


def stream():
    return _lib.current_stream()


def sync():
    if DEV != "cpu":
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ depthwise 7x7
DW_SHAPES = [(2, 2, 2, 64), (1, 3, 3, 128), (1, 5, 9, 8), (2, 7, 7, 320), (2, 16, 16, 192), (1, 64, 64, 128)]


def _nchw64(t):
    return t.double().cpu().permute(0, 3, 1, 2)


def _dw_ref(x, w, bias, add, flip):
    """float64 depthwise convolution of the (rounded) operands, NHWC in and out, and the sum of the magnitudes of its terms"""
    C = x.shape[-1]
    k = w.double().cpu()
    if flip:
        k = k.flip(-1)
    k = k.view(C, 1, 7, 7)
    ref = F.conv2d(_nchw64(x), k, None, padding=3, groups=C)
    mag = F.conv2d(_nchw64(x).abs(), k.abs(), None, padding=3, groups=C)
    if bias is not None:
        ref = ref + bias.double().cpu().view(1, C, 1, 1)
        mag = mag + bias.double().cpu().abs().view(1, C, 1, 1)
    ref, mag = ref.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)
    if add is not None:
        ref = ref + add.double().cpu()
        mag = mag + add.double().cpu().abs()
    return ref, mag


def _dw_run(x, pack, bias, add, flip, code):
    """one launch with both outputs, each behind a NaN guard row"""
    N, H, W, C = x.shape
    nan = float("nan")
    out_op = torch.full((N * H * W + 1, C), nan, dtype=x.dtype, device=DEV)
    out_f32 = torch.full((N * H * W + 1, C), nan, device=DEV)
    call("prx_k_cnx_dwconv", x, pack, bias, add, out_op, out_f32, N, H, W, C, flip, code, stream())
    sync()
    assert torch.isnan(out_op[-1].float()).all() and torch.isnan(out_f32[-1]).all(), "wrote past the end of an output"
    return out_op[:-1].reshape(N, H, W, C), out_f32[:-1].reshape(N, H, W, C)


def dwconv_checks(shape, precision):
    """|got - float64| <= 2^-18 * sum |w x| (+ |bias|, |add|) + rho |float64| per output: 49 fp32 FMAs and the additions, then the
    output format's rounding (rho = 2^-24 for the fp32 output)"""
    N, H, W, C = shape
    code, dt, rho = PREC[precision]
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + C)
    x = torch.randn(N, H, W, C, generator=g).to(DEV).to(dt)
    gr = torch.randn(N, H, W, C, generator=g).to(DEV).to(dt)
    w = (torch.randn(C, 49, generator=g) / 7.0).to(dt).float().to(DEV)          # representable in the operand format: the pack is exact
    bias = torch.randn(C, generator=g).to(DEV)
    add = torch.randn(N, H, W, C, generator=g).to(DEV)
    pack = torch.full((2 * 49 * C + 8,), float("nan"), dtype=dt, device=DEV)
    call("prx_k_cnx_pack_dw", w, pack, C, code, stream())
    sync()
    assert torch.isnan(pack[2 * 49 * C:].float()).all()
    assert torch.equal(pack[:49 * C].float().view(49, C), w.t()) and torch.equal(pack[49 * C:2 * 49 * C].float().view(49, C), w.flip(-1).t())
    worst = 0.0
    bounds = {}
    for flip, inp, b_, a_ in ((0, x, bias, None), (1, gr, None, add), (0, x, None, add), (1, gr, bias, None), (0, x, None, None), (1, gr, None, None)):
        ref, mag = _dw_ref(inp, w, b_, a_, flip)
        got_op, got_f32 = _dw_run(inp, pack, b_, a_, flip, code)
        for got, r in ((got_op, rho), (got_f32, 2.0 ** -24)):
            bound = 2.0 ** -18 * mag + r * ref.abs()
            err = (got.double().cpu() - ref).abs()
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            assert (err <= bound).all(), (shape, precision, flip, float((err / bound.clamp_min(1e-300)).max()))
        if b_ is None and a_ is None:
            bounds[flip] = (got_f32.double().cpu(), 2.0 ** -18 * mag + 2.0 ** -24 * ref.abs())
            again_op, again_f32 = _dw_run(inp, pack, None, None, flip, code)
            assert torch.equal(again_op, got_op) and torch.equal(again_f32, got_f32), "two calls differ"
    # <dwconv(x), g> = <x, dwconv_flip(g)> on the kernel's fp32 outputs, to the per-output bounds summed
    (y, by), (z, bz) = bounds[0], bounds[1]
    x64, g64 = x.double().cpu(), gr.double().cpu()
    lhs, rhs = float((y * g64).sum()), float((x64 * z).sum())
    tol = float((by * g64.abs()).sum() + (bz * x64.abs()).sum())
    print(f"dwconv {shape} {precision}: worst error / bound {worst:.3f}; adjoint |lhs - rhs| {abs(lhs - rhs):.3e} (bound {tol:.3e})")
    assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)


@pytest.mark.parametrize("precision", ["fp16", "bf16", "f32"])
@pytest.mark.parametrize("shape", DW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_depthwise_7x7_forward_and_data_gradient_vs_float64(shape, precision):
    dwconv_checks(shape, precision)


# ------------------------------------------------------------------------------------------ permutation, pool, LayerNorm
PERM_SHAPES = [(2, 2, 2, 64), (1, 6, 10, 192), (2, 16, 16, 128)]


def layout_checks(shape, precision):
    """space-to-depth and its inverse equal the indexing restatement exactly; the pool pair within 2^-20 * sum |x| / HW"""
    N, H, W, C = shape
    code, dt, rho = PREC[precision]
    g = torch.Generator().manual_seed(H + 7 * W + C)
    x = torch.randn(N, H, W, C, generator=g).to(DEV).to(dt)
    want = x.view(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 4 * C)
    nan = float("nan")
    s2d = torch.full((N * H * W + 1, C), nan, dtype=dt, device=DEV)
    call("prx_k_cnx_space_to_depth", x, s2d, N, H, W, C, code, stream())
    back = torch.full((N * H * W + 1, C), nan, dtype=dt, device=DEV)
    call("prx_k_cnx_depth_to_space", s2d, back, N, H, W, C, code, stream())
    sync()
    assert torch.isnan(s2d[-1].float()).all() and torch.isnan(back[-1].float()).all()
    assert torch.equal(s2d[:-1].reshape(want.shape), want), "space-to-depth"
    assert torch.equal(back[:-1].reshape(x.shape), x), "depth-to-space"
    pooled = torch.full((N + 1, C), nan, device=DEV)
    call("prx_k_cnx_avgpool_fwd", x, pooled, N, H * W, C, code, stream())
    gp = torch.randn(N, C, generator=g).to(DEV)
    dx32 = torch.full((N * H * W + 1, C), nan, device=DEV)
    dx16 = torch.full((N * H * W + 1, C), nan, dtype=dt, device=DEV)
    call("prx_k_cnx_avgpool_bwd", gp, dx32, dx16, N, H * W, C, code, stream())
    sync()
    assert torch.isnan(pooled[-1]).all() and torch.isnan(dx32[-1]).all() and torch.isnan(dx16[-1].float()).all()
    x64 = x.double().cpu().view(N, H * W, C)
    err = (pooled[:-1].double().cpu() - x64.mean(1)).abs()
    assert (err <= 2.0 ** -20 * x64.abs().sum(1) / (H * W)).all(), float(err.max())
    ref = (gp.double().cpu() / (H * W)).view(N, 1, C).expand(N, H * W, C)
    e32 = (dx32[:-1].double().cpu().view(N, H * W, C) - ref).abs()
    e16 = (dx16[:-1].double().cpu().view(N, H * W, C) - ref).abs()
    sub = 2.0 ** -25 if precision == "fp16" else 0.0         # g / HW reaches half's subnormals (spacing 2^-24): half a step, absolute
    assert (e32 <= 2.0 ** -20 * ref.abs()).all() and (e16 <= (2.0 ** -20 + rho) * ref.abs() + sub).all()


@pytest.mark.parametrize("precision", ["fp16", "bf16", "f32"])
@pytest.mark.parametrize("shape", PERM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_space_to_depth_its_inverse_and_the_pool_pair(shape, precision):
    layout_checks(shape, precision)


def layernorm_checks(rows, C, precision, group=0):
    """the channel LayerNorm (any C % 8 == 0; `group`: the stem's layout with one unused row ahead of every `group` rows) against float64
    on the rounded input.  Forward: mean and rstd to 2^-20 relative (two fp32 reductions over C), the output to 2^-18 (|xhat gamma| +
    |beta|) + 2^-20 rstd mean|x| |gamma| (what the mean's error carries into every element) + rho |ref|.  Backward: linear in g, so the bound is 2^-17 * rstd * (|g gamma| + mean|g gamma| + |xhat| mean|g gamma xhat|)
    + rho |ref| -- the magnitudes of its three terms, each a reduction over C in fp32."""
    code, dt, rho = PREC[precision]
    g = torch.Generator().manual_seed(rows + C)
    phys = rows + rows // group + 1 if group else rows
    x = (torch.randn(phys, C, generator=g) * 1.5 + 0.3).to(DEV).to(dt)
    ga, be = (1 + 0.2 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    gr = torch.randn(rows, C, generator=g).to(DEV)
    idx = torch.arange(rows)
    idx = idx + idx // group + 1 if group else idx
    nan = float("nan")
    out = torch.full((rows + 1, C), nan, dtype=dt, device=DEV)
    out32 = torch.full((rows + 1, C), nan, device=DEV)
    mean, rstd = torch.full((rows + 1,), nan, device=DEV), torch.full((rows + 1,), nan, device=DEV)
    call("prx_k_cnx_layernorm_fwd", x, 0, ga, be, out, out32, mean, rstd, rows, C, 1e-6, group, code, stream())
    dx = torch.full((phys + 1, C), nan, dtype=dt, device=DEV)
    dx32 = torch.full((phys + 1, C), nan, device=DEV)
    call("prx_k_cnx_layernorm_bwd", gr, x, 0, ga, mean, rstd, dx, dx32, rows, C, group, code, stream())
    sync()
    for t in (out, out32, mean, rstd, dx, dx32):
        assert torch.isnan(t[-1].float()).all(), "wrote past the end of an output"
    x64, ga64, be64, g64 = x.double().cpu()[idx], ga.double().cpu(), be.double().cpu(), gr.double().cpu()
    m = x64.mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x64 - m) ** 2).mean(1, keepdim=True) + 1e-6)
    xh = (x64 - m) * rs
    assert ((mean[:-1].double().cpu() - m[:, 0]).abs() <= 2.0 ** -20 * x64.abs().mean(1)).all()
    assert ((rstd[:-1].double().cpu() - rs[:, 0]).abs() <= 2.0 ** -20 * rs[:, 0]).all()
    ref = xh * ga64 + be64
    carried = 2.0 ** -20 * rs * x64.abs().mean(1, keepdim=True) * ga64.abs()       # the mean's own error, through rstd * gamma
    for got, r in ((out, rho), (out32, 2.0 ** -24)):
        assert ((got[:-1].double().cpu() - ref).abs() <= 2.0 ** -18 * ((xh * ga64).abs() + be64.abs()) + carried + r * ref.abs()).all()
    gg = g64 * ga64
    dref = rs * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    mag = rs * (gg.abs() + gg.abs().mean(1, keepdim=True) + xh.abs() * (gg * xh).abs().mean(1, keepdim=True))
    for got, r in ((dx, rho), (dx32, 2.0 ** -24)):
        assert ((got[:-1].double().cpu()[idx] - dref).abs() <= 2.0 ** -17 * mag + r * dref.abs()).all()
    if group:       # the unused rows are not written
        hole = torch.ones(phys, dtype=torch.bool); hole[idx] = False
        assert torch.isnan(dx32[:-1].cpu()[hole]).all()


@pytest.mark.parametrize("precision", ["fp16", "bf16", "f32"])
@pytest.mark.parametrize("rows,C,group", [(5, 8, 0), (9, 64, 4), (7, 96, 0), (6, 192, 0), (5, 320, 0), (3, 3072, 0)])
def test_channel_layernorm_vs_float64(rows, C, group, precision):
    layernorm_checks(rows, C, precision, group)


# ------------------------------------------------------------------------------------------ reduced towers vs restatement
def tower_case(cfg, n, precision, seed=5, params=None):
    params = weights.synthetic_clip_convnext_params(cfg, seed) if params is None else params
    g = torch.Generator().manual_seed(seed + 1)
    cut = torch.rand(n, 3, cfg.input_resolution, cfg.input_resolution, generator=g) * 1.2 - 0.1
    gout = torch.randn(n, cfg.output_dim, generator=g)
    ref, gref = _convnext_ref.embed_and_grad(params, cfg, cut, gout, torch.float64)
    h = ops.ClipConvNextHandle(cfg, params, max_batch=n, device=DEV, precision=precision)
    cd = cut.to(DEV).requires_grad_(True)
    out = ops.clip_encode_image(cd, h)
    (gd,) = torch.autograd.grad(out, cd, gout.to(DEV))
    return h, ref, out, gref, gd


def tower_checks(name, n, precision):
    """embedding and d/d cutouts of the runner (folded layer scale) against the float64 restatement (unfolded) at the per-mode gates of
    the project's reduced towers (tests/test_openclip_gpu.py::tower_checks)"""
    cfg = weights.CLIP_CONVNEXT_CONFIGS[name]
    h, ref, out, gref, gd = tower_case(cfg, n, precision)
    figs = (rel_l2(out, ref), cosine(out, ref), rel_l2(gd, gref), cosine(gd, gref))
    print(f"ConvNeXt tower {name} n={n} {precision}: emb rel-L2 {figs[0]:.3e} cos {figs[1]:.8f}  grad rel-L2 {figs[2]:.3e} cos {figs[3]:.8f}")
    if precision == "f32":
        assert figs[0] < F32_GATE and figs[2] < F32_GATE, figs
    elif precision == "fp16":
        assert figs[0] < 5e-3 and figs[1] > 0.9999 and figs[2] < 2e-2 and figs[3] > 0.9999, figs
    else:       # bf16: 2^3 times coarser operand rounding than half
        assert figs[0] < 8 * 5e-3 and figs[1] > 1 - 64e-4 and figs[2] < 8 * 2e-2 and figs[3] > 1 - 64e-4, figs
    return figs


@pytest.mark.parametrize("precision", ["f32", "fp16", "bf16"])
@pytest.mark.parametrize("name,n", [("tiny-cnx", 3), ("tiny-cnx-d", 2)])
def test_reduced_towers_vs_restatement(name, n, precision):
    """tiny-cnx: R 64 (maps 16 / 8 / 4 / 2), dims 64..512, depths 1/1/2/1, linear head, N = 3; tiny-cnx-d: R 96 (maps 24 / 12 / 6 / 3),
    dims 96..768, one block per stage, mlp head, N = 2.

    Measured on an MI355X (embedding rel-L2 / cosine, gradient rel-L2 / cosine):
      tiny-cnx   n=3  f32  4.6e-7 / 1.00000000, 6.0e-7 / 1.00000000;  fp16 6.2e-4 / 0.99999981, 1.04e-3 / 0.99999947;
                      bf16 5.3e-3 / 0.99998571, 6.6e-3 / 0.99997849
      tiny-cnx-d n=2  f32  5.9e-7 / 1.00000000, 1.0e-6 / 1.00000000;  fp16 7.3e-4 / 0.99999974, 8.8e-4 / 0.99999962;
                      bf16 6.2e-3 / 0.99998093, 6.9e-3 / 0.99997633"""
    tower_checks(name, n, precision)


def test_switches_are_live():
    """f32: zeroing one block's layer scale moves the embedding by more than 10 x the f32 gate while the runner still follows the
    restatement of the same parameters; the linear and the mlp head on one trunk differ, each matching its own restatement"""
    cfg = weights.CLIP_CONVNEXT_CONFIGS["tiny-cnx"]
    base = weights.synthetic_clip_convnext_params(cfg, 5)
    _, ref, out, _, _ = tower_case(cfg, 2, "f32", params=base)
    zeroed = dict(base)
    zeroed["trunk.stages.2.blocks.1.gamma"] = torch.zeros_like(base["trunk.stages.2.blocks.1.gamma"])
    _, ref0, out0, _, _ = tower_case(cfg, 2, "f32", params=zeroed)
    assert rel_l2(out, ref) < F32_GATE and rel_l2(out0, ref0) < F32_GATE
    assert rel_l2(out0, ref) > 10 * F32_GATE and rel_l2(out0, out) > 10 * F32_GATE, rel_l2(out0, out)
    mcfg = dataclasses.replace(cfg, proj="mlp")
    mp = weights.synthetic_clip_convnext_params(mcfg, 5)
    assert torch.equal(mp["trunk.stages.3.blocks.0.mlp.fc2.weight"], base["trunk.stages.3.blocks.0.mlp.fc2.weight"])     # the same trunk
    _, mref, mout, _, _ = tower_case(mcfg, 2, "f32", params=mp)
    assert rel_l2(mout, mref) < F32_GATE and rel_l2(mout, out) > 10 * F32_GATE


# ------------------------------------------------------------------------------------------ real widths
@pytest.mark.parametrize("name,depths", [("convnext_base_w", (1, 1, 2, 1)), ("convnext_large_d", (1, 1, 1, 1))])
def test_real_widths_finite_and_repeatable(name, depths):
    """the real widths, resolution (256) and head of convnext_base_w / convnext_large_d with the depths overridden, N = 2: one forward
    and one backward, finite, unit rows, and a second handle repeats them bit for bit.  No 36-block weight set is materialised."""
    cfg = dataclasses.replace(weights.CLIP_CONVNEXT_CONFIGS[name], depths=depths)
    params = weights.synthetic_clip_convnext_params(cfg, 1)
    g = torch.Generator().manual_seed(2)
    cut = torch.rand(2, 3, cfg.input_resolution, cfg.input_resolution, generator=g).to(DEV)
    gout = torch.randn(2, cfg.output_dim, generator=g).to(DEV)
    res = []
    for _ in range(2):
        h = ops.ClipConvNextHandle(cfg, params, max_batch=2, device=DEV)
        cd = cut.clone().requires_grad_(True)
        out = ops.clip_encode_image(cd, h)
        (gd,) = torch.autograd.grad(out, cd, gout)
        assert torch.isfinite(out).all() and torch.isfinite(gd).all() and float(gd.abs().max()) > 0
        assert torch.allclose(out.norm(dim=-1), torch.ones(2, device=DEV), atol=1e-4)
        res.append((out.detach().cpu(), gd.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ------------------------------------------------------------------------------------------ graph replay
def test_graph_replay_matches_eager_session(tmp_path):
    """a `fast_pixel` session with tiny-cnx takes enable_graph() (the runner only launches on the given stream), and two replayed
    iterations equal two eager ones bit for bit; cutout noise is off (the device randn streams of capture and eager differ)"""
    from pixray_amd import frontend as fe
    from pixray_amd.engine import HipAdam

    def build(name):
        run = fe.Run()
        run.settings = dict(drawer="fast_pixel", clip_models="tiny-cnx", size=[64, 48], num_cuts=4, iterations=8, save_every=100,
                            display_every=100, outdir=str(tmp_path / name), seed=5, skip_args=True, vector_prompts="none",
                            noise_prompt_seeds=[1], noise_prompt_weights=[1.0], learning_rate_drops=[])
        sess = fe.do_init(fe.apply_settings(run=run), run)
        for mk in sess.cutoutsTable.values():
            mk.noise_fac = 0.0
        return sess
    a, b = build("eager"), build("graph")
    assert isinstance(a.perceptors["tiny-cnx"].handle, ops.ClipConvNextHandle)
    assert torch.equal(a.drawer.get_z(), b.drawer.get_z())
    a.opts = [HipAdam.from_adam(o) if not isinstance(o, HipAdam) else o for o in a.opts]
    assert b.enable_graph(warmup=2), b.graph_error
    assert b.graph_error is None and b._graph is not None
    for it in range(2):
        a.train(it)
    for it in range(2, 4):
        a.train(it)
        b.train(it)
        assert torch.equal(a.drawer.get_z(), b.drawer.get_z()), it
        assert all(torch.equal(x, y) for x, y in zip(a.last_losses, b.last_losses)), it
    assert b._graph is not None


# ------------------------------------------------------------------------------------------ refusals
def refusal_checks():
    x = torch.zeros(4 * 4 * 16, dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.PrxError, match="multiple of 8"):
        call("prx_k_cnx_dwconv", x, x, None, None, x, None, 1, 4, 4, 12, 0, 2, stream())
    with pytest.raises(_lib.PrxError, match="multiple of 8"):
        call("prx_k_cnx_space_to_depth", x, x, 1, 4, 4, 12, 2, stream())
    with pytest.raises(_lib.PrxError, match="32-bit index range"):
        call("prx_k_cnx_dwconv", x, x, None, None, x, None, 64, 1024, 1024, 64, 0, 2, stream())
    cfg = weights.CLIP_CONVNEXT_CONFIGS["tiny-cnx"]
    params = weights.synthetic_clip_convnext_params(cfg, 0)
    with pytest.raises(_lib.PrxError, match="multiple of 32"):
        ops.ClipConvNextHandle(dataclasses.replace(cfg, input_resolution=100), params, 1, DEV)
    bad = dataclasses.replace(cfg, dims=(12, 128, 256, 512))
    with pytest.raises(_lib.PrxError, match="multiple of 8"):
        ops.ClipConvNextHandle(bad, weights.synthetic_clip_convnext_params(bad, 0), 1, DEV)
    h = ops.ClipConvNextHandle(cfg, params, max_batch=1, device=DEV)
    with pytest.raises(_lib.PrxError, match="exceeds handle capacity"):
        ops.clip_encode_image(torch.rand(2, 3, 64, 64).to(DEV), h)
    with pytest.raises(KeyError, match=r"trunk\.stages\.2\.blocks\.1\.gamma"):
        ops.ClipConvNextHandle(cfg, {k: v for k, v in params.items() if k != "trunk.stages.2.blocks.1.gamma"}, 1, DEV)


def test_refusals_by_name():
    refusal_checks()


# ------------------------------------------------------------------------------------------ one run through the front end
def test_one_convnext_base_w_run_through_the_front_end(tmp_path):
    """`--drawer fast_pixel --clip_models convnext_base_w --num_cuts 2 --size 64 48`, 2 iterations through do_init / do_run on the HIP parts"""
    from PIL import Image
    from pixray_amd import frontend as fe
    run = fe.Run()
    run.settings = dict(drawer="fast_pixel", clip_models="convnext_base_w", num_cuts=2, size=[64, 48], iterations=2, save_every=1, display_every=2,
                        outdir=str(tmp_path / "out"), seed=5, skip_args=True, vector_prompts="none", noise_prompt_seeds=[1],
                        noise_prompt_weights=[1.0], learning_rate_drops=[])
    s = fe.apply_settings(run=run)
    sess = fe.do_init(s, run, device=None)
    assert sess.cutoutSizeTable == {"convnext_base_w": 256}
    perc = sess.perceptors["convnext_base_w"]
    assert isinstance(perc.handle, ops.ClipConvNextHandle) and perc.text_cfg.gelu and perc.output_dim == 640
    z0 = sess.drawer.get_z_copy()
    while not fe.do_run(s, return_display=True, run=run):
        pass
    assert sess.cur_iteration == 2 and len(sess.last_losses) >= 1 and all(torch.isfinite(l).all() for l in sess.last_losses)
    assert float((sess.drawer.get_z().detach() - z0).abs().max()) > 0.0
    img = Image.open(os.path.join(s.outdir, "output.png"))
    assert img.size == (64, 48) and "convnext_base_w" in img.info["pixray_clip_models"]
