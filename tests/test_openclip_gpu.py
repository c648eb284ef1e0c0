"""OpenCLIP (LAION) perceptors on the HIP runners: the attention kernels for heads of 96 operand columns (head dim 80 zero-padded)
against float64, reduced towers with heads of 80 and the GELU text tower against the plain-torch restatement (tests/_openclip_ref.py,
float64), ViT-H-14's real width, and one run through the front end.  The check functions take their device from `DEV`, so
tests/test_emu_openclip.py runs a subset on the CPU emulation of the kernels.

Every test here fails on a tree without the feature (no prx_k_mha_*_hd_op, no OPENCLIP_CONFIGS, no prx_text_tower_create)."""
import dataclasses
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _openclip_ref  # noqa: E402
from pixray_amd import _lib, ops, weights  # noqa: E402
from pixray_amd._lib import call  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32_GATE = 1e-4          # tests/test_f32_mode_gpu.py: the stated gate of the exact mode


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


# ------------------------------------------------------------------------------------------ the 96-wide attention kernels
N_ATT, HEADS_ATT = 2, 2


def _att_ref(x, do, hd):
    """float64 attention of the (already rounded) operands x [N, T, 3, heads, hd], scale 1 / sqrt(hd): out, lse, d(qkv) for d(out) = do"""
    q, k, v = [x[:, :, i].permute(0, 2, 1, 3).double().requires_grad_(True) for i in range(3)]
    sc = q @ k.transpose(-1, -2) * hd ** -0.5
    out = (torch.softmax(sc, dim=-1) @ v).permute(0, 2, 1, 3)                       # [N, T, heads, hd]
    gq, gk, gv = torch.autograd.grad(out, (q, k, v), do.double())
    dqkv = torch.stack([g.permute(0, 2, 1, 3) for g in (gq, gk, gv)], dim=2)        # [N, T, 3, heads, hd]
    return out.detach(), torch.logsumexp(sc.detach(), dim=-1), dqkv


def _att_run(x, do, cols, h16, op_cols):
    """the kernels on x [N, T, 3, heads, hd] zero-padded to `cols` columns per head; op_cols: the head_cols argument, or None for the
    prx_k_mha_*_gen_op entry points"""
    N, T, _, heads, hd = x.shape
    C = heads * cols
    qkv = torch.zeros(N, T, 3, heads, cols, dtype=x.dtype, device=DEV)
    qkv[..., :hd] = x
    dout = torch.zeros(N, T, heads, cols, dtype=x.dtype, device=DEV)
    dout[..., :hd] = do
    nan = float("nan")
    out = torch.full((N * T + 1, C), nan, dtype=x.dtype, device=DEV)             # one guard row behind every output
    lse = torch.full((N * heads * T + 4,), nan, device=DEV)
    dqkv = torch.full((N * T + 1, 3 * C), nan, dtype=x.dtype, device=DEV)
    if op_cols is None:
        call("prx_k_mha_fwd_gen_op", qkv, out, lse, N, T, C, heads, h16, stream())
        call("prx_k_mha_bwd_gen_op", qkv, out, dout, lse, dqkv, N, T, C, heads, h16, stream())
    else:
        call("prx_k_mha_fwd_hd_op", qkv, out, lse, N, T, C, heads, h16, op_cols, stream())
        call("prx_k_mha_bwd_hd_op", qkv, out, dout, lse, dqkv, N, T, C, heads, h16, op_cols, stream())
    sync()
    assert torch.isnan(out[N * T].float()).all() and torch.isnan(dqkv[N * T].float()).all() and torch.isnan(lse[N * heads * T:]).all(), \
        "wrote past the end of an output"
    return (out[:N * T].reshape(N, T, heads, cols), lse[:N * heads * T].reshape(N, heads, T), dqkv[:N * T].reshape(N, T, 3, heads, cols))


def _max_err(got, ref):
    """max |got - ref| over max |ref|"""
    return float((got.double().cpu() - ref.cpu()).abs().max() / ref.abs().max().clamp_min(1e-300))


ATT_T = (1, 31, 33, 50, 257, 577)
# lengths for the 96-wide family only, outside the yardstick: 129 puts one key in the second 128-token LDS chunk and one live lane in
# the fifth wave; 640 is 20 full token blocks on 4 x 5 waves, no partial block anywhere, the last length before the refusal
ATT_T_EDGE = (129, 640)
ATT_KEYS = ("out", "lse", "dqkv")


def _att_operands(T, h16):
    dt = torch.float16 if h16 else torch.bfloat16
    g = torch.Generator().manual_seed(1000 * T)
    x = torch.randn(N_ATT, T, 3, HEADS_ATT, 80, generator=g).to(DEV).to(dt)
    do = torch.randn(N_ATT, T, HEADS_ATT, 80, generator=g).to(DEV).to(dt)
    return x, do


@functools.lru_cache(maxsize=None)
def att_yardstick(h16, dev):
    """the existing 64-wide kernels (prx_k_mha_*_gen_op) on the same tokens and seed -- the first 64 of the 80 columns -- against
    float64 at head dim 64: per quantity, their largest max |kernel - float64| / max |float64| over the six sequence lengths.
    One figure per operand format and quantity, computed once: per-length ratios mean nothing where both families are exact up to
    fp32 rounding (at T = 1 every probability is 1 and `out` is v itself; lse is an fp32 quantity at every length)."""
    worst = dict.fromkeys(ATT_KEYS, 0.0)
    for T in ATT_T:
        x, do = _att_operands(T, h16)
        x, do = x[..., :64].contiguous(), do[..., :64].contiguous()
        got, ref = _att_run(x, do, 64, h16, None), _att_ref(x, do, 64)
        e = {k: _max_err(a, b) for k, a, b in zip(ATT_KEYS, got, ref)}
        print(f"mha 64-wide T={T} {'fp16' if h16 else 'bf16'}: " + "  ".join(f"{k} {v:.3e}" for k, v in e.items()))
        worst = {k: max(worst[k], e[k]) for k in ATT_KEYS}
    return worst


def attention96_checks(T, h16):
    x, do = _att_operands(T, h16)
    o96, l96, d96 = _att_run(x, do, 96, h16, 96)
    assert (o96[..., 80:] == 0).all() and (d96[..., 80:] == 0).all(), "pad columns of out / dqkv are not exactly zero"
    ref = _att_ref(x, do, 80)
    e96 = {k: _max_err(a, b) for k, a, b in zip(ATT_KEYS, (o96[..., :80], l96, d96[..., :80]), ref)}
    yard = att_yardstick(h16, DEV)
    print(f"mha hd96 T={T} {'fp16' if h16 else 'bf16'}: " + "  ".join(f"{k} {e96[k]:.3e} (64-wide yardstick {yard[k]:.3e})" for k in ATT_KEYS))
    for k in ATT_KEYS:
        assert e96[k] <= 2.0 * yard[k], (T, h16, k, e96[k], yard[k])


@pytest.mark.parametrize("h16", [1, 0])
@pytest.mark.parametrize("T", ATT_T + ATT_T_EDGE)
def test_mha_96_columns_vs_float64(T, h16):
    """prx_k_mha_{fwd,bwd}_hd_op at 96 columns per head with the last 16 of each head zeroed, N = 2, 2 heads: out, lse and d(qkv)
    against float64 attention of the rounded operands at head dim 80, scale 1 / sqrt(80); pad columns of out and dqkv exactly 0;
    nothing written past the outputs.  The tolerance is measured: the existing 64-wide kernels on the same tokens and seed are the
    yardstick (att_yardstick), and the 96-wide ones get twice their max error (the dot products are 1.25 x longer, rounding is not
    worst-case).

    Measured on an MI355X, max |kernel - float64| / max |float64|, worst of the six lengths, 96-wide (64-wide yardstick):
      fp16: out 3.80e-04 (4.76e-04), lse 1.43e-07 (1.38e-07), d(qkv) 5.71e-04 (4.20e-04)
      bf16: out 3.29e-03 (3.24e-03), lse 1.51e-07 (1.50e-07), d(qkv) 4.32e-03 (4.10e-03)
    and at the two edge lengths (ATT_T_EDGE; same gate, not part of the yardstick):
      T = 129  fp16: out 3.87e-04, lse 1.24e-07, d(qkv) 4.06e-04   bf16: out 2.26e-03, lse 1.46e-07, d(qkv) 3.35e-03
      T = 640  fp16: out 2.86e-04, lse 1.28e-07, d(qkv) 3.61e-04   bf16: out 1.74e-03, lse 1.28e-07, d(qkv) 2.87e-03
    (per length: DESIGN.md section 6d)"""
    attention96_checks(T, h16)


@pytest.mark.parametrize("h16", [1, 0])
@pytest.mark.parametrize("T", [33, 257])
def test_mha_hd_op_at_64_columns_is_the_gen_op(T, h16):
    """head_cols = 64 gives the bits of prx_k_mha_{fwd,bwd}_gen_op"""
    dt = torch.float16 if h16 else torch.bfloat16
    g = torch.Generator().manual_seed(T)
    x = torch.randn(N_ATT, T, 3, HEADS_ATT, 64, generator=g).to(DEV).to(dt)
    do = torch.randn(N_ATT, T, HEADS_ATT, 64, generator=g).to(DEV).to(dt)
    a, b = _att_run(x, do, 64, h16, 64), _att_run(x, do, 64, h16, None)
    for s, t in zip(a, b):
        assert torch.equal(s, t)
    with pytest.raises(_lib.PrxError, match="columns per head"):
        call("prx_k_mha_fwd_hd_op", x, x, None, 1, 1, 80, 1, h16, 80, stream())


def test_mha_96_refuses_what_it_cannot_run():
    x = torch.zeros(641 * 3 * 96, dtype=torch.float16, device=DEV)
    lse = torch.zeros(641, device=DEV)
    with pytest.raises(_lib.PrxError, match="T <= 640"):
        call("prx_k_mha_fwd_hd_op", x, x, lse, 1, 641, 96, 1, 1, 96, stream())
    with pytest.raises(_lib.PrxError, match="96 columns per head"):
        call("prx_k_mha_fwd_hd_op", x, x, lse, 1, 33, 128, 2, 1, 96, stream())


# ------------------------------------------------------------------------------------------ reduced towers vs restatement
def tower_case(cfg, n, precision, seed=5):
    params = weights.synthetic_clip_vit_params(cfg, seed)
    g = torch.Generator().manual_seed(seed + 1)
    cut = torch.rand(n, 3, cfg.input_resolution, cfg.input_resolution, generator=g) * 1.2 - 0.1
    gout = torch.randn(n, cfg.output_dim, generator=g)
    ref, gref = _openclip_ref.embed_and_grad(params, cfg, cut, gout, torch.float64)
    h = ops.OpenClipVitHandle(cfg, params, max_batch=n, device=DEV, precision=precision)
    cd = cut.to(DEV).requires_grad_(True)
    out = ops.clip_encode_image(cd, h)
    (gd,) = torch.autograd.grad(out, cd, gout.to(DEV))
    return h, ref, out, gref, gd


def tower_checks(name, n, precision):
    """embedding and d/d cutouts against the float64 restatement at the per-mode gates of tests/test_slip_gpu.py's reduced towers (the
    same runner with the same switches), and exact zeros in the pad columns (80 .. 95 of every head of q, k and v) of block 0's d(qkv)"""
    cfg = weights.OPENCLIP_CONFIGS[name]
    assert cfg.head_dim == 80
    h, ref, out, gref, gd = tower_case(cfg, n, precision)
    figs = (rel_l2(out, ref), cosine(out, ref), rel_l2(gd, gref), cosine(gd, gref))
    print(f"OpenCLIP tower {name} n={n} {precision}: emb rel-L2 {figs[0]:.3e} cos {figs[1]:.8f}  grad rel-L2 {figs[2]:.3e} cos {figs[3]:.8f}")
    if precision == "f32":
        assert figs[0] < F32_GATE and figs[2] < F32_GATE, figs
    elif precision == "fp16":
        assert figs[0] < 5e-3 and figs[1] > 0.9999 and figs[2] < 2e-2 and figs[3] > 0.9999, figs
    else:       # bf16: 2^3 times coarser operand rounding than half (tests/test_slip_gpu.py tower_checks)
        assert figs[0] < 8 * 5e-3 and figs[1] > 1 - 64e-4 and figs[2] < 8 * 2e-2 and figs[3] > 1 - 64e-4, figs
    dt = {"f32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[precision]
    dqkv = torch.full((n * cfg.tokens, 3, cfg.heads, 96), float("nan"), dtype=dt, device=DEV)
    got = _lib.load().prx_vit_tower_debug_dqkv(h.h, dqkv.data_ptr(), dqkv.numel() * dqkv.element_size(), stream())
    sync()
    assert got == dqkv.numel() * dqkv.element_size()
    assert torch.isfinite(dqkv.float()).all() and dqkv[..., :80].float().abs().max() > 0
    assert (dqkv[..., 80:] == 0).all(), "pad columns of dqkv are not exactly zero"


@pytest.mark.parametrize("precision", ["f32", "fp16", "bf16"])
@pytest.mark.parametrize("name,n", [("tiny-H-32", 3), ("tiny-H-14", 2)])
def test_reduced_towers_with_heads_of_80_vs_restatement(name, n, precision):
    """width 640, 8 heads of 80, 2 layers: 50 tokens (patch 32, N = 3) and 257 tokens (patch 14, N = 2)"""
    tower_checks(name, n, precision)


def test_the_exact_gelu_switch_of_the_vision_tower_is_live():
    """the same weights through the OpenAI creator (QuickGELU) give another embedding"""
    cfg = weights.OPENCLIP_CONFIGS["ViT-B-32"]
    cfg = dataclasses.replace(cfg, layers=2)
    params = weights.synthetic_clip_vit_params(cfg, 2)
    cut = torch.rand(2, 3, 224, 224, generator=torch.Generator().manual_seed(3)).to(DEV)
    a = ops.clip_encode_image(cut, ops.OpenClipVitHandle(cfg, params, 2, DEV, precision="f32"))
    b = ops.clip_encode_image(cut, ops.ClipVitHandle(cfg, params, 2, DEV, precision="f32"))
    ref = _openclip_ref.encode_image(_openclip_ref.cast(params, torch.float64), cfg, cut.cpu().double())
    assert rel_l2(a, ref) < F32_GATE and rel_l2(b, ref) > 10 * F32_GATE, (rel_l2(a, ref), rel_l2(b, ref))


def _tokens(cfg, n, seed):
    g = torch.Generator().manual_seed(seed)
    tk = torch.zeros(n, cfg.context_length, dtype=torch.long)
    for i in range(n):
        L = int(torch.randint(1, cfg.context_length - 2, (1,), generator=g)) if i else cfg.context_length - 2   # row 0: full length
        tk[i, 0] = cfg.vocab_size - 2
        tk[i, 1:1 + L] = torch.randint(1, cfg.vocab_size - 2, (L,), generator=g)
        tk[i, 1 + L] = cfg.vocab_size - 1
    return tk


def text_checks(n=4):
    """width 256, 4 heads, 2 layers, GELU (prx_text_tower_create) against the restatement at the CLIP text tower's gates
    (tests/test_path_gpu.py::test_clip_text_tower_vs_oracle: bf16 operands, rel-L2 2e-2, cosine 0.999 per row); the same weights
    through the QuickGELU creator (prx_clip_text_create) must give another result, the restatement's with QuickGELU"""
    cfg = weights.CLIP_TEXT_CONFIGS["tiny-H-32"]
    assert isinstance(cfg, weights.OpenClipTextConfig) and cfg.gelu and (cfg.width, cfg.heads, cfg.layers) == (256, 4, 2)
    p = weights.synthetic_clip_text_params(cfg, seed=9)
    tk = _tokens(cfg, n, 13)
    e = ops.clip_encode_text_tokens(tk, ops.ClipTextHandle(cfg, p, max_batch=8, device=DEV))
    quick_cfg = weights.ClipTextConfig(cfg.name, cfg.vocab_size, cfg.context_length, cfg.width, cfg.layers, cfg.heads, cfg.output_dim)
    eq = ops.clip_encode_text_tokens(tk, ops.ClipTextHandle(quick_cfg, p, max_batch=8, device=DEV))
    p64 = _openclip_ref.cast(p, torch.float64)
    ref = _openclip_ref.encode_text(p64, cfg, tk)
    refq = _openclip_ref.encode_text(p64, cfg, tk, act=_openclip_ref.quick_gelu)
    figs = (rel_l2(e, ref), rel_l2(eq, refq), rel_l2(e, eq), rel_l2(ref, refq))
    print(f"text tower GELU {figs[0]:.3e}  QuickGELU {figs[1]:.3e}  GELU vs QuickGELU: kernels {figs[2]:.3e} float64 {figs[3]:.3e}")
    assert e.shape == (n, cfg.output_dim)
    assert figs[0] < 2e-2 and figs[1] < 2e-2, figs
    for i in range(n):
        assert cosine(e[i], ref[i]) > 0.999
    assert not torch.equal(e, eq) and figs[2] > 0.5 * figs[3] > 0, figs       # the switch is live: the two activations' own distance


def test_text_tower_with_gelu_vs_restatement_and_the_switch_is_live():
    text_checks()


# ------------------------------------------------------------------------------------------ real width
def test_vit_h_14_width_two_layers_finite_and_repeatable():
    """ViT-H-14's width (1280, 16 heads of 80, MLP 5120, 257 tokens, embedding 1024) with layers = 2 overridden, N = 2: one forward and
    one backward, finite, and a second run on a second handle repeats bit for bit.  No 32-layer weight set is materialised."""
    cfg = dataclasses.replace(weights.OPENCLIP_CONFIGS["ViT-H-14"], layers=2)
    params = weights.synthetic_clip_vit_params(cfg, 1)
    g = torch.Generator().manual_seed(2)
    cut = torch.rand(2, 3, 224, 224, generator=g).to(DEV)
    gout = torch.randn(2, cfg.output_dim, generator=g).to(DEV)
    res = []
    for _ in range(2):
        h = ops.OpenClipVitHandle(cfg, params, max_batch=2, device=DEV)
        cd = cut.clone().requires_grad_(True)
        out = ops.clip_encode_image(cd, h)
        (gd,) = torch.autograd.grad(out, cd, gout)
        assert torch.isfinite(out).all() and torch.isfinite(gd).all() and float(gd.abs().max()) > 0
        assert torch.allclose(out.norm(dim=-1), torch.ones(2, device=DEV), atol=1e-4)
        res.append((out.detach().cpu(), gd.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ------------------------------------------------------------------------------------------ one run through the front end
def test_one_vit_b_16_openclip_run_through_the_front_end(tmp_path):
    """`--drawer fast_pixel --clip_models ViT-B-16 --num_cuts 2 --size 64 48`, 2 iterations through do_init / do_run on the HIP parts"""
    from PIL import Image
    from pixray_amd import frontend as fe
    run = fe.Run()
    run.settings = dict(drawer="fast_pixel", clip_models="ViT-B-16", num_cuts=2, size=[64, 48], iterations=2, save_every=1, display_every=2,
                        outdir=str(tmp_path / "out"), seed=5, skip_args=True, vector_prompts="none", noise_prompt_seeds=[1],
                        noise_prompt_weights=[1.0], learning_rate_drops=[])
    s = fe.apply_settings(run=run)
    sess = fe.do_init(s, run, device=None)
    assert sess.cutoutSizeTable == {"ViT-B-16": 224}
    perc = sess.perceptors["ViT-B-16"]
    assert isinstance(perc.handle, ops.OpenClipVitHandle) and perc.text_cfg.gelu
    z0 = sess.drawer.get_z_copy()
    while not fe.do_run(s, return_display=True, run=run):
        pass
    assert sess.cur_iteration == 2 and len(sess.last_losses) >= 1 and all(torch.isfinite(l).all() for l in sess.last_losses)
    assert float((sess.drawer.get_z().detach() - z0).abs().max()) > 0.0
    img = Image.open(os.path.join(s.outdir, "output.png"))
    assert img.size == (64, 48) and "ViT-B-16" in img.info["pixray_clip_models"]
