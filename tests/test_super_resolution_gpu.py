"""The RRDBNet x4 runner (csrc/rrdbnet.hip) and the super_resolution drawer as a whole, on the GPU, against the float64
restatement of the network in tests/_rrdbnet_ref.py.

Gates, both computed here on the CPU at the test's own shapes (nothing is taken from the code under test):
  * "f32"  : rel-L2 <= 8 x the error of torch's own fp32 evaluation of the same network against float64;
  * "fp16" : rel-L2 <= 3 x the error of the float64 network with its weights, every convolution input and every gradient
             entering a data gradient rounded to IEEE half, against plain float64.
The runner keeps the residual stream and every gradient sum in fp32 in both modes (only MFMA operands are half), so in the half
mode it is expected to land below the yardstick, not at it.

The clamped path: conv_last of a 2-block network is rescaled (weight std 0.125 / sqrt(fan_in), bias + 0.5: with this package's
synthetic initialisation the features entering conv_last have a standard deviation of ~1.6, so 0.5 / sqrt(fan_in) would put
40 % outside) so that about 5 % of the float64 pre-clamp values lie outside [0,1] (asserted: 2 % .. 12 %).  The upstream gradient
is set to ZERO at every pixel whose float64 pre-clamp value lies within delta of 0 or 1, so a mask decision that rounding could
flip cannot reach dL/dz.  delta = 10 x the mode's absolute image error bound, and that bound is what the image gate allows as an
absolute RMS error: (8 or 3) x the yardstick's rel-L2 x the RMS of the float64 pre-clamp image -- a flipped decision outside delta
would take a single-pixel error of ten times the RMS error the gate permits.  The zeroed share is asserted <= 3 %.

Measured, rel-L2 image / dz (yardstick on the CPU -> kernels on an MI355X; `pytest -s` prints every figure):
  tiny-RRDB 8 x 12      f32 3.0e-7 / 4.5e-7 -> 5.9e-7 / 6.1e-7     fp16 4.5e-4 / 2.5e-2 -> 4.0e-4 / 2.4e-2
  23 blocks 16 x 16     f32 3.2e-7 / 5.2e-7 -> 7.0e-7 / 6.7e-7     fp16 4.7e-4 / 2.8e-2 -> 4.4e-4 / 2.8e-2
  clamped, 2 blocks     f32 2.3e-7 / 3.9e-7 -> 6.2e-7 / 5.9e-7     fp16 3.4e-4 / 2.6e-2 -> 2.7e-4 / 1.8e-2
  clamped: 7.05 % of the float64 pre-clamp values outside [0,1]; zeroed share 0 % (f32, delta 8.0e-6) and 0.56 % (fp16, delta 4.4e-3).
(An f32 yardstick that holds a flipped LeakyReLU sign -- torch's fp32 evaluation against float64 -- is refused by an assertion.)"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from pixray_amd import api, ops
from pixray_amd._lib import PrxError
from pixray_amd.weights import RRDBNET_CONFIGS, RrdbNetConfig, synthetic_rrdbnet_params

import _rrdbnet_ref as R

DEV = "cuda"          # tests/test_emu_super_resolution.py switches this to "cpu" for the emulated kernels
MODES = ["f32", "fp16"]
_REF = {}             # (case, ref mode) -> the float64 / yardstick evaluations, computed once and shared between the modes


def ref_mode(mode):
    return "f32" if mode == "f32" else "half"


def factor(mode):
    return 8.0 if mode == "f32" else 3.0


def inputs(hw, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.rand(1, 3, *hw, generator=g).double()                       # fp32-representable: the kernels see the same numbers
    gi = torch.randn(1, 3, 4 * hw[0], 4 * hw[1], generator=g).double()
    return z, gi


def network_case(model, hw, mode):
    cfg = RRDBNET_CONFIGS[model]
    params = synthetic_rrdbnet_params(cfg, 0)
    # the tiny case's input seed is one at which torch's fp32 evaluation flips no LeakyReLU sign against float64 (seed 17 flips
    # one: its f32 dz yardstick is 5.7e-4 instead of 4e-7, a gate a thousand times too loose); asserted below
    z, gi = inputs(hw, 18 if model == "tiny-RRDB" else 17)
    for m in ("f64", ref_mode(mode)):
        if (model, hw, m) not in _REF:
            _REF[(model, hw, m)] = R.run(params, z, cfg.num_block, gi, m)
    (img64, dz64), (img_y, dz_y) = _REF[(model, hw, "f64")], _REF[(model, hw, ref_mode(mode))]
    y_img, y_dz = R.rel_l2(img_y, img64), R.rel_l2(dz_y, dz64)
    handle = ops.RrdbNetHandle(cfg, params, hw, torch.device(DEV), precision=mode)
    zt = z.float().to(DEV).requires_grad_(True)
    img = ops.rrdbnet_synth(zt, handle, clamp=False)
    img.backward(gi.float().to(DEV))
    e_img, e_dz = R.rel_l2(img.detach().cpu(), img64), R.rel_l2(zt.grad.cpu(), dz64)
    print(f"[rrdb-fig] {model} {hw} {mode}: image yardstick {y_img:.3e} error {e_img:.3e} | dz yardstick {y_dz:.3e} error {e_dz:.3e}")
    assert y_img > 0 and y_dz > 0
    if mode == "f32":
        assert y_img < 5e-6 and y_dz < 5e-6, "the fp32 yardstick holds a flipped LeakyReLU sign: it would not gate anything"
    assert e_img <= factor(mode) * y_img and e_dz <= factor(mode) * y_dz


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("model,hw", [("tiny-RRDB", (8, 12)), ("RealESRGAN_x4plus", (16, 16))])
def test_network_and_gradient_against_float64(model, hw, mode):
    network_case(model, hw, mode)


def clamp_params():
    cfg = RrdbNetConfig(num_block=2, name="depth-2")
    p = synthetic_rrdbnet_params(cfg, 0)
    g = torch.Generator().manual_seed(41)
    p["conv_last.weight"] = torch.randn(3, 64, 3, 3, generator=g) * 0.125 / (64 * 9) ** 0.5
    p["conv_last.bias"] = 0.5 + 0.02 * torch.randn(3, generator=g)
    return cfg, p


@pytest.mark.parametrize("mode", MODES)
def test_clamped_path(mode):
    cfg, params = clamp_params()
    hw = (8, 12)
    z, gi = inputs(hw, 23)
    if ("clamp", "raw64") not in _REF:
        _REF[("clamp", "raw64")] = R.run(params, z, cfg.num_block, None, "f64")[0]
    raw64 = _REF[("clamp", "raw64")]
    outside = float(((raw64 < 0) | (raw64 > 1)).double().mean())
    if ("clamp", ref_mode(mode)) not in _REF:
        _REF[("clamp", ref_mode(mode))] = R.run(params, z, cfg.num_block, None, ref_mode(mode))[0]
    bound = factor(mode) * R.rel_l2(_REF[("clamp", ref_mode(mode))], raw64) * float(raw64.pow(2).mean().sqrt())
    delta = 10 * bound
    near = ((raw64.abs() < delta) | ((raw64 - 1).abs() < delta))
    share = float(near.double().mean())
    print(f"[rrdb-fig] clamp {mode}: outside {outside:.4f} image bound {bound:.3e} delta {delta:.3e} zeroed share {share:.4f}")
    assert 0.02 <= outside <= 0.12
    assert share <= 0.03
    g = gi.clone()
    g[near] = 0.0
    _, img64, dz64 = R.run_clamped(params, z, cfg.num_block, g, "f64")
    _, img_y, dz_y = R.run_clamped(params, z, cfg.num_block, g, ref_mode(mode))
    y_img, y_dz = R.rel_l2(img_y, img64), R.rel_l2(dz_y, dz64)
    handle = ops.RrdbNetHandle(cfg, params, hw, torch.device(DEV), precision=mode)
    zt = z.float().to(DEV).requires_grad_(True)
    img = ops.rrdbnet_synth(zt, handle, clamp=True)
    img.backward(g.float().to(DEV))
    assert float(img.detach().min()) >= 0.0 and float(img.detach().max()) <= 1.0
    e_img, e_dz = R.rel_l2(img.detach().cpu(), img64), R.rel_l2(zt.grad.cpu(), dz64)
    print(f"[rrdb-fig] clamp {mode}: image yardstick {y_img:.3e} error {e_img:.3e} | dz yardstick {y_dz:.3e} error {e_dz:.3e}")
    assert e_img <= factor(mode) * y_img and e_dz <= factor(mode) * y_dz


def tiny_handle(hw, mode="f32"):
    cfg = RRDBNET_CONFIGS["tiny-RRDB"]
    return ops.RrdbNetHandle(cfg, synthetic_rrdbnet_params(cfg, 0), hw, torch.device(DEV), precision=mode)


def test_stale_backward_fails_by_name():
    h = tiny_handle((5, 7))
    z = torch.rand(1, 3, 5, 7, device=DEV, requires_grad=True)
    first = ops.rrdbnet_synth(z, h)
    ops.rrdbnet_synth(z, h)
    with pytest.raises(PrxError, match="stale backward"):
        first.sum().backward()
    with pytest.raises(PrxError, match=r"z must be \[1,3,5,7\]"):
        ops.rrdbnet_synth(torch.rand(1, 3, 7, 5, device=DEV), h)


def test_refused_geometry_and_precision():
    cfg = RrdbNetConfig(num_feat=32, num_grow_ch=16, num_block=1, name="narrow")
    with pytest.raises(PrxError, match="num_feat = 64, num_grow = 32"):
        ops.RrdbNetHandle(cfg, synthetic_rrdbnet_params(cfg, 0), (5, 7), torch.device(DEV), precision="f32")
    with pytest.raises(PrxError, match="bf16"):
        tiny_handle((5, 7), "bf16")


def test_two_handles_do_not_share_state():
    a, b = tiny_handle((8, 12)), tiny_handle((5, 7))
    za = torch.rand(1, 3, 8, 12, device=DEV, requires_grad=True)
    zb = torch.rand(1, 3, 5, 7, device=DEV, requires_grad=True)
    ga = torch.randn(1, 3, 32, 48, device=DEV)
    alone = ops.rrdbnet_synth(za, a, False)
    alone.backward(ga)
    want_img, want_dz = alone.detach().clone(), za.grad.clone()
    za.grad = None
    ia = ops.rrdbnet_synth(za, a, False)
    ib = ops.rrdbnet_synth(zb, b, False)                 # b's forward and backward run between a's forward and a's backward
    ib.backward(torch.randn(1, 3, 20, 28, device=DEV))
    ia.backward(ga)
    assert torch.equal(ia.detach(), want_img) and torch.equal(za.grad, want_dz)
    assert bool(torch.isfinite(zb.grad).all()) and float(zb.grad.abs().sum()) > 0


def test_session_eager_graph_and_repeat_are_bit_identical():
    def build():
        sess = api.build_super_resolution_clip_session(size=(64, 48), model="tiny-RRDB", clip_model="ViT-B/32", num_cuts=8, seed=2, device=DEV)
        for mk in sess.cutoutsTable.values():
            mk.noise_fac = 0.0            # device randn streams differ between capture and eager; compare without noise
        return sess
    runs = []
    for kind in ("eager", "graph", "eager"):
        s = build()
        assert tuple(s.drawer.get_z().shape) == (1, 3, 12, 16)
        if kind == "graph":
            assert s.enable_graph(warmup=2) is True, s.graph_error       # iterations 0, 1 eagerly; iteration 2 is captured and replayed
            s.train(2)
        else:
            for it in range(3):
                s.train(it)
        z = s.drawer.get_z().detach().clone()
        assert bool(torch.isfinite(z).all()) and float(z.min()) >= 0.0 and float(z.max()) <= 1.0
        runs.append(z)
        del s
    assert torch.equal(runs[0], runs[2]), "the eager run does not repeat bit for bit"
    assert torch.equal(runs[0], runs[1]), "graph replay differs from eager launches"
    init = build().drawer.get_z()
    assert not torch.equal(runs[0], init.detach())


def test_front_end_settings_to_png(tmp_path):
    """`--drawer super_resolution` through the settings front end: canvas 66 x 50 rounded down to 64 x 48, an init image resized to
    z, four iterations, a PNG out"""
    from PIL import Image
    from pixray_amd import frontend as fe
    from pixray_amd.engine import HipAdam
    run = fe.Run()
    run.settings = dict(drawer="super_resolution", super_resolution_model="tiny-RRDB", clip_models="tiny-B/32", size=[66, 50], num_cuts=8,
                        iterations=4, save_every=2, display_every=4, outdir=str(tmp_path / "out"), seed=3, skip_args=True, init_noise="pixels",
                        vector_prompts="none", noise_prompt_seeds=[1], noise_prompt_weights=[1.0], precision="fp16", learning_rate_drops=[])
    s = fe.apply_settings(run=run)
    sess = fe.do_init(s, run, device=None)
    assert sess.drawer.size == (64, 48) and tuple(sess.drawer.get_z().shape) == (1, 3, 12, 16)
    assert sess.drawer.get_z().is_cuda and isinstance(sess.opts[0], HipAdam) and sess.opts[0].bounds is not None
    z0 = sess.drawer.get_z_copy()
    while not fe.do_run(s, return_display=True, run=run):
        pass
    z = sess.drawer.get_z().detach()
    assert float((z - z0).abs().max()) > 1e-3 and float(z.min()) >= 0.0 and float(z.max()) <= 1.0
    assert all(torch.isfinite(l).all() for l in sess.last_losses)
    assert Image.open(os.path.join(s.outdir, "output.png")).size == (64, 48)
