"""OpenCLIP ViT-g-14 and ViT-bigG-14 on the HIP runners: the ragged LayerNorm at MAXV = 8 (widths 1152, 1408, 1664) against float64, the
128-wide attention instances (heads of 104 zero-padded) and heads of 88 on the 96-wide ones against float64 with the 96-wide kernels
on heads of 80 as the yardstick, reduced towers (2 layers at the real widths and MLP widths) and the two text geometries against the
plain-torch restatement (tests/_openclip_ref.py takes the MLP width from the tensors), the real geometry at 2 layers, the refusals, and
one run through the front end.  The check functions take their device from `DEV`, so tests/test_emu_openclip_big.py runs a subset on the
CPU emulation of the kernels.

Every test here fails on a tree without the feature (no prx_k_layernorm_*_rag_op, no prx_k_mha_*_hdim_op, no `ViT-g-14` in
OPENCLIP_CONFIGS, no prx_vit_tower_create_mlp)."""
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
import test_kernels_half_gpu as kh  # noqa: E402   (layernorm_case: the LayerNorm kernel tests' own check and bounds)
import test_openclip_gpu as og  # noqa: E402       (_att_ref, _max_err, _tokens, the towers' gates)
from pixray_amd import _lib, checkpoints, ops, weights  # noqa: E402
from pixray_amd._lib import call  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def stream():
    return _lib.current_stream()


def sync():
    if DEV != "cpu":
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ ragged LayerNorm, MAXV = 8
_RAG = {"prx_k_layernorm_fwd_op": "prx_k_layernorm_fwd_rag_op", "prx_k_layernorm_bwd_op": "prx_k_layernorm_bwd_rag_op"}


def layernorm_rag_checks(C, rows, s16, h16, fp32_out):
    """tests/test_kernels_half_gpu.py::layernorm_case -- the check the C = 1280 cases of test_layernorm_variants run, bounds and all
    (fp32 outputs at min(4 x the fp32 reference's own error, 1e-5) rel-L2; 16-bit outputs within one ulp + the fp32 chain; mean / rstd
    by their summation depth; NaN guards beyond column C and beyond the last row of every output) -- through the ragged entry points"""
    saved = kh.call, kh.DEV
    kh.call, kh.DEV = (lambda name, *a: call(_RAG.get(name, name), *a)), DEV
    try:
        for with_add in (True, False):
            for add_every in (0, 2):
                kh.layernorm_case(rows, C, h16, s16, add_every=add_every, fp32_out=fp32_out, with_add=with_add, seed=rows)
    finally:
        kh.call, kh.DEV = saved


@pytest.mark.parametrize("h16", [0, 1], ids=["bf16", "half"])
@pytest.mark.parametrize("s16", [0, 1, 2, 7])
@pytest.mark.parametrize("C", [1152, 1408, 1664])
def test_ragged_layernorm_at_eight_vectors_vs_float64(C, s16, h16):
    """ln_fwd_kernel<8, S16, true> / ln_bwd_kernel<8, 0 | 1 | 2 | 7, true> at C = 1408 (11 x 128, ViT-g-14), 1664 (13 x 128,
    ViT-bigG-14) and 1152 (9 x 128: the first width past the old cap, lanes 32 .. 63 of vector 4 must stay silent); rows 1, 3, 4, 5 (four
    rows per workgroup: 5 leaves a part-filled last one); with and without `add`, add_every 0 and 2, with the fp32 output and 16-bit only"""
    for rows in (1, 3, 4, 5):
        for fp32_out in (True, False):
            layernorm_rag_checks(C, rows, s16, h16, fp32_out)


def test_ragged_layernorm_keeps_the_plain_entry_points_and_the_cap():
    """the plain entry points still refuse a width that is no multiple of 256; the ragged ones refuse 2176 (> 2048) and 1400"""
    rows = 4
    for name_f, name_b, C in (("prx_k_layernorm_fwd_op", "prx_k_layernorm_bwd_op", 1408),
                              ("prx_k_layernorm_fwd_rag_op", "prx_k_layernorm_bwd_rag_op", 2176),
                              ("prx_k_layernorm_fwd_rag_op", "prx_k_layernorm_bwd_rag_op", 1400)):
        x = torch.randn(rows, C, device=DEV)
        ga = torch.ones(C, device=DEV)
        o = torch.full((rows, C), float("nan"), dtype=torch.float16, device=DEV)
        mr = torch.zeros(rows, device=DEV)
        with pytest.raises(_lib.PrxError, match="multiple of 256"):
            call(name_f, x, C, ga, ga, o, None, mr, mr.clone(), rows, C, 1e-5, 1, 0, stream())
        with pytest.raises(_lib.PrxError, match="multiple of 256"):
            call(name_b, x, C, x, C, ga, mr, mr, None, C, None, C, o, C, rows, C, 1, 0, 0, stream())
        sync()
        assert bool(torch.isnan(o).all())


# ------------------------------------------------------------------------------------------ 128-wide attention, heads of 88 at 96
ATT_T = (1, 2, 31, 32, 33, 127, 128, 129, 257)      # the 32-token MFMA block and the 128-token LDS chunk, each -1 / 0 / +1; 257 tokens
HEAD_COLS = {80: 96, 88: 96, 104: 128}


def _operands(T, N, heads, hd, h16, draw=0):
    """operands of head dim hd: the first hd columns of one 128-column draw per (T, N, heads, draw), so that every head dim sees the
    same tokens, seed and value scale"""
    dt = torch.float16 if h16 else torch.bfloat16
    g = torch.Generator().manual_seed(100000 * draw + 1000 * T + 10 * N + heads)
    x = torch.randn(N, T, 3, heads, 128, generator=g)[..., :hd].contiguous().to(DEV).to(dt)
    do = torch.randn(N, T, heads, 128, generator=g)[..., :hd].contiguous().to(DEV).to(dt)
    return x, do


def _att_run(x, do, h16):
    """prx_k_mha_{fwd,bwd}_hdim_op on x [N, T, 3, heads, hd] zero-padded to the head dim's columns; NaN guards behind every output"""
    N, T, _, heads, hd = x.shape
    cols = HEAD_COLS[hd]
    C = heads * cols
    qkv = torch.zeros(N, T, 3, heads, cols, dtype=x.dtype, device=DEV)
    qkv[..., :hd] = x
    dout = torch.zeros(N, T, heads, cols, dtype=x.dtype, device=DEV)
    dout[..., :hd] = do
    nan = float("nan")
    out = torch.full((N * T + 1, C), nan, dtype=x.dtype, device=DEV)
    lse = torch.full((N * heads * T + 4,), nan, device=DEV)
    dqkv = torch.full((N * T + 1, 3 * C), nan, dtype=x.dtype, device=DEV)
    call("prx_k_mha_fwd_hdim_op", qkv, out, lse, N, T, C, heads, h16, cols, hd, stream())
    call("prx_k_mha_bwd_hdim_op", qkv, out, dout, lse, dqkv, N, T, C, heads, h16, cols, hd, stream())
    sync()
    assert torch.isnan(out[N * T].float()).all() and torch.isnan(dqkv[N * T].float()).all() and torch.isnan(lse[N * heads * T:]).all(), \
        "wrote past the end of an output"
    return (out[:N * T].reshape(N, T, heads, cols), lse[:N * heads * T].reshape(N, heads, T), dqkv[:N * T].reshape(N, T, 3, heads, cols))


def _draws(T, N, heads):
    """One draw of a small case holds a handful of 16-bit roundings (at two tokens and one head: four probabilities), and the ratio of
    two such errors is a coin toss -- heads of 88 against heads of 80 ON THE SAME KERNEL came out between 0.5 and 2.2.  A case therefore
    pools as many draws (launches of the same shape, seeds draw = 0, 1, ...) as give it 64 (image, head, token) rows, the new instance
    and the yardstick alike."""
    return max(1, -(-64 // (N * heads * T)))


def _errors(hd, T, N, heads, h16, checks=False):
    """rel-L2 error against float64 of out, dQ, dK and dV on the live columns, pooled over the case's draws (sqrt(sum |kernel -
    float64|^2 / sum |float64|^2)); then the two quantities that carry no 16-bit rounding, each as the largest (value / its own fp32
    bound) over the draws: `lse` (max |kernel - float64|) and, at one token, where dQ and dK are exactly 0 in float64, max |dQ|, |dK|.
    With `checks`: the pad columns of out and dqkv are exactly 0 and a repeat of the launches gives the same bits."""
    num, den = dict.fromkeys(("out", "dq", "dk", "dv"), 0.0), dict.fromkeys(("out", "dq", "dk", "dv"), 0.0)
    lse_err, dqk0 = 0.0, 0.0
    for draw in range(_draws(T, N, heads)):
        x, do = _operands(T, N, heads, hd, h16, draw)
        got = _att_run(x, do, h16)
        o, l, d = got
        if checks:
            assert (o[..., hd:] == 0).all() and (d[..., hd:] == 0).all(), "pad columns of out / dqkv are not exactly zero"
            assert all(torch.equal(a, b) for a, b in zip(got, _att_run(x, do, h16))), "a repeat differs"
        ro, rl, rd = og._att_ref(x, do, hd)
        pairs = {"out": (o[..., :hd], ro), "dq": (d[:, :, 0, :, :hd], rd[:, :, 0]), "dk": (d[:, :, 1, :, :hd], rd[:, :, 1]),
                 "dv": (d[:, :, 2, :, :hd], rd[:, :, 2])}
        for k, (a, b) in pairs.items():
            num[k] += float((a.double().cpu() - b.cpu()).pow(2).sum())
            den[k] += float(b.cpu().pow(2).sum())
        # fp32 bounds (classical: a sum of n products is off by at most n eps sum |terms|).  lse = log sum exp(scale q.k): the dot
        # product, eight operations on the result (scale multiply, max, exp2, log, the base change), and a T-term sum of the exponentials
        xd = x.double().cpu()
        q, kk, v = xd[:, :, 0], xd[:, :, 1], xd[:, :, 2]
        qk = float(torch.einsum("nihd,njhd->nhij", q.abs(), kk.abs()).max()) * hd ** -0.5
        lse_err = max(lse_err, float((l.double().cpu() - rl.cpu()).abs().max()) / (EPS32 * (hd * qk + 8 * max(1.0, float(rl.abs().max())) + T)))
        if T == 1:
            # dS = scale p (dP - D): dP (an MFMA sum) and D (a lane sum) are the same hd products v.dO in two orders, each within
            # hd eps sum |v dO| of the exact sum; times scale, times the largest |k| (dQ) or |q| (dK); one 16-bit rounding of dS and one
            # of the result (2^-8 each, relative)
            vdo = float((v.abs() * do.double().cpu().abs()).sum(-1).max())
            bound = 2 * hd * EPS32 * vdo * hd ** -0.5 * float(torch.maximum(q.abs().max(), kk.abs().max())) * (1 + 2.0 ** -7)
            dqk0 = max(dqk0, float(d[:, :, :2, :, :hd].double().abs().max()) / bound)
    e = {k: (num[k] / max(den[k], 1e-300)) ** 0.5 for k in num if not (T == 1 and k in ("dq", "dk"))}
    return e, lse_err, dqk0


@functools.lru_cache(maxsize=None)
def yardstick(T, N, heads, h16, dev):
    """the existing 96-wide instance on heads of 80 -- the first 80 columns of the same draws -- at the same T, N, heads, seeds and
    value scale, in the same run"""
    return _errors(80, T, N, heads, h16)[0]


# Quantities that carry no 16-bit rounding have no ratio to hold: lse at every length (an fp32 quantity in both families: 1.3e-7 here
# and there, tests/test_openclip_gpu.py's note), and dQ / dK at one token (exactly 0 in float64; in the kernels the difference of two
# fp32 sums of the same products in two orders, times one 16-bit operand).  They face the worst-case fp32 bounds written out in _errors.
EPS32 = 2.0 ** -24


def attention_checks(hd, T, N, heads, h16):
    (e, lse_err, dqk0), y = _errors(hd, T, N, heads, h16, checks=True), yardstick(T, N, heads, h16, DEV)
    print(f"mha head dim {hd} at {HEAD_COLS[hd]} columns T={T} N={N} heads={heads} {'fp16' if h16 else 'bf16'} ({_draws(T, N, heads)} draws): " +
          "  ".join(f"{k} {e[k]:.3e} / hd 80 {y[k]:.3e} = {e[k] / max(y[k], 1e-300):.2f}" for k in e) +
          f"  of their fp32 bounds: lse {lse_err:.3f}  dq, dk at T = 1 {dqk0:.3f}")
    assert lse_err <= 1.0 and dqk0 <= 1.0, (hd, T, N, heads, h16, lse_err, dqk0)
    for k in e:
        assert e[k] <= 2.0 * y[k], (hd, T, N, heads, h16, k, e[k], y[k])


@pytest.mark.parametrize("h16", [1, 0], ids=["half", "bf16"])
@pytest.mark.parametrize("N,heads", [(1, 1), (2, 16)])
@pytest.mark.parametrize("T", ATT_T)
@pytest.mark.parametrize("hd", [104, 88])
def test_mha_heads_of_104_and_88_vs_float64(hd, T, N, heads, h16):
    """prx_k_mha_{fwd,bwd}_hdim_op: heads of 104 on the 128-wide instances (scale 1 / sqrt(104)) and heads of 88 on the 96-wide ones
    (1 / sqrt(88)): out, dQ, dK, dV (rel-L2) and lse against float64 attention of the rounded operands; the pad columns of out and dqkv
    exactly 0; nothing written past the outputs; a repeat gives the same bits.  Yardstick: the 96-wide instance on heads of 80 of the
    same draws in the same run; the gate is twice its error (dot products 1.3 x longer, sqrt(104 / 80) = 1.14 in the rounding-noise
    model, with room for the accumulation order).  lse, and dQ / dK at one token, carry no 16-bit rounding and face fp32 bounds instead.

    Measured on an MI355X, rel-L2 of the new instance over that of the yardstick, smallest .. largest of the 18 cases (T, N, heads):
      104 fp16: out 0.97 .. 1.02  dQ 0.84 .. 1.15  dK 0.87 .. 1.20  dV 0.94 .. 1.02     bf16: 0.97 .. 1.02, 0.96 .. 1.27, 0.95 .. 1.20, 0.99 .. 1.07
       88 fp16: out 0.96 .. 1.02  dQ 0.86 .. 1.19  dK 0.86 .. 1.27  dV 0.95 .. 1.05     bf16: 0.96 .. 1.02, 0.94 .. 1.13, 0.93 .. 1.05, 0.91 .. 1.08
    (the largest at T = 2; 0.99 .. 1.00 at 257 tokens, 2 images, 16 heads); lse uses 1.5 % of its fp32 bound, dQ / dK at one token 0.6 %.
    Errors themselves: DESIGN.md section 6d."""
    attention_checks(hd, T, N, heads, h16)


def test_mha_hdim_refuses_what_it_has_no_instance_for():
    x = torch.zeros(641 * 3 * 128, dtype=torch.float16, device=DEV)
    lse = torch.zeros(641, device=DEV)
    for cols, hd in ((96, 96), (128, 112), (128, 88), (96, 104)):
        with pytest.raises(_lib.PrxError, match=f"head dim {hd} at {cols} columns"):
            call("prx_k_mha_fwd_hdim_op", x, x, lse, 1, 33, cols, 1, 1, cols, hd, stream())
        with pytest.raises(_lib.PrxError, match=f"head dim {hd} at {cols} columns"):
            call("prx_k_mha_bwd_hdim_op", x, x, x, lse, x, 1, 33, cols, 1, 1, cols, hd, stream())
    with pytest.raises(_lib.PrxError, match="T <= 640"):
        call("prx_k_mha_fwd_hdim_op", x, x, lse, 1, 641, 128, 1, 1, 128, 104, stream())
    with pytest.raises(_lib.PrxError, match="128 columns per head"):
        call("prx_k_mha_fwd_hdim_op", x, x, lse, 1, 33, 96, 1, 1, 128, 104, stream())


# ------------------------------------------------------------------------------------------ reduced towers vs restatement
def tower_checks(name, n, precision):
    """embedding and d/d cutouts against the float64 restatement at the gates tests/test_openclip_gpu.py applies to tiny-H-32 /
    tiny-H-14 (the same runner with the same switches), and exact zeros in the pad columns of block 0's d(qkv)"""
    cfg = weights.OPENCLIP_CONFIGS[name]
    hd, hp = cfg.head_dim, HEAD_COLS[cfg.head_dim]
    assert hd in (88, 104) and cfg.mlp != 4 * cfg.width
    saved = og.DEV
    og.DEV = DEV
    try:
        h, ref, out, gref, gd = og.tower_case(cfg, n, precision)
    finally:
        og.DEV = saved
    figs = (og.rel_l2(out, ref), og.cosine(out, ref), og.rel_l2(gd, gref), og.cosine(gd, gref))
    print(f"OpenCLIP tower {name} n={n} {precision}: emb rel-L2 {figs[0]:.3e} cos {figs[1]:.8f}  grad rel-L2 {figs[2]:.3e} cos {figs[3]:.8f}")
    if precision == "f32":
        assert figs[0] < og.F32_GATE and figs[2] < og.F32_GATE, figs
    elif precision == "fp16":
        assert figs[0] < 5e-3 and figs[1] > 0.9999 and figs[2] < 2e-2 and figs[3] > 0.9999, figs
    else:
        assert figs[0] < 8 * 5e-3 and figs[1] > 1 - 64e-4 and figs[2] < 8 * 2e-2 and figs[3] > 1 - 64e-4, figs
    dt = {"f32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[precision]
    dqkv = torch.full((n * cfg.tokens, 3, cfg.heads, hp), float("nan"), dtype=dt, device=DEV)
    got = _lib.load().prx_vit_tower_debug_dqkv(h.h, dqkv.data_ptr(), dqkv.numel() * dqkv.element_size(), stream())
    sync()
    assert got == dqkv.numel() * dqkv.element_size()
    assert torch.isfinite(dqkv.float()).all() and dqkv[..., :hd].float().abs().max() > 0
    assert (dqkv[..., hd:] == 0).all(), "pad columns of dqkv are not exactly zero"


@pytest.mark.parametrize("precision", ["f32", "fp16", "bf16"])
@pytest.mark.parametrize("name", ["tiny-g-32", "tiny-bigG-32", "tiny-bigG-14"])
def test_reduced_towers_with_heads_of_88_and_104_vs_restatement(name, precision):
    """widths 1408 / 1664, 16 heads of 88 / 104, MLP 6144 / 8192, 2 layers, 2 cutouts: 50 tokens (patch 32) and 257 tokens (patch 14)"""
    tower_checks(name, 2, precision)


def text_checks(name, layers=2, n=3):
    """the text geometry of `name` (ViT-g-14: width 1024, 16 heads; ViT-bigG-14: width 1280, 20 heads) at 2 layers and a 1000-token
    vocabulary, GELU, against the restatement at the CLIP text tower's gates (tests/test_openclip_gpu.py text_checks)"""
    cfg = dataclasses.replace(weights.CLIP_TEXT_CONFIGS[name], layers=layers, vocab_size=1000)
    assert isinstance(cfg, weights.OpenClipTextConfig) and cfg.gelu and cfg.width == 64 * cfg.heads
    p = weights.synthetic_clip_text_params(cfg, seed=9)
    tk = og._tokens(cfg, n, 13)
    e = ops.clip_encode_text_tokens(tk, ops.ClipTextHandle(cfg, p, max_batch=4, device=DEV))
    ref = _openclip_ref.encode_text(_openclip_ref.cast(p, torch.float64), cfg, tk)
    fig = og.rel_l2(e, ref)
    print(f"text tower {name} at {layers} layers: rel-L2 {fig:.3e}")
    assert e.shape == (n, cfg.output_dim) and fig < 2e-2, fig
    for i in range(n):
        assert og.cosine(e[i], ref[i]) > 0.999


@pytest.mark.parametrize("name", ["ViT-g-14", "ViT-bigG-14"])
def test_the_two_text_geometries_at_two_layers_vs_restatement(name):
    text_checks(name)


# ------------------------------------------------------------------------------------------ prompt loss at 1280
@pytest.mark.parametrize("n,m,D,w,stop", [(5, 1, 1280, 1.0, float("-inf")), (64, 3, 1280, -0.5, float("-inf")), (3, 2, 1088, 2.0, 0.9),
                                           (9, 2, 2048, 0.3, float("-inf"))])
def test_prompt_loss_beyond_1024_columns_vs_oracle(n, m, D, w, stop):
    """ViT-bigG-14 embeds into 1280 columns: the prompt loss holds a row in registers, 16 steps of 64 up to 1024 and 32 steps beyond
    (1088: the first width of the second instance; 2048: its last).  tests/test_path_gpu.py::test_prompt_loss_vs_oracle with its gates;
    n = 5, 3, 9 leave a part-filled last workgroup of four rows"""
    from oracle import prompt_ref
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
    assert og.rel_l2(gd, gref) < 1e-4, og.rel_l2(gd, gref)
    with pytest.raises(_lib.PrxError, match="<= 2048"):
        ops.prompt_loss(torch.zeros(2, 2112, device=DEV), torch.zeros(1, 2112, device=DEV), 1.0, float("-inf"))


# ------------------------------------------------------------------------------------------ real geometry
@pytest.mark.parametrize("name", ["ViT-g-14", "ViT-bigG-14"])
def test_real_geometry_two_layers_finite_and_repeatable(name):
    """the full width, heads, MLP width, 257 tokens and embedding size with layers = 2 overridden, 1 cutout: create, forward, backward;
    finite, the right shapes, and a second handle repeats bit for bit"""
    cfg = dataclasses.replace(weights.OPENCLIP_CONFIGS[name], layers=2)
    params = weights.synthetic_clip_vit_params(cfg, 1)
    g = torch.Generator().manual_seed(2)
    cut = torch.rand(1, 3, 224, 224, generator=g).to(DEV)
    gout = torch.randn(1, cfg.output_dim, generator=g).to(DEV)
    res = []
    for _ in range(2):
        h = ops.OpenClipVitHandle(cfg, params, max_batch=1, device=DEV)
        cd = cut.clone().requires_grad_(True)
        out = ops.clip_encode_image(cd, h)
        (gd,) = torch.autograd.grad(out, cd, gout)
        assert out.shape == (1, cfg.output_dim) and gd.shape == cut.shape
        assert torch.isfinite(out).all() and torch.isfinite(gd).all() and float(gd.abs().max()) > 0
        assert torch.allclose(out.norm(dim=-1), torch.ones(1, device=DEV), atol=1e-4)
        res.append((out.detach().clone(), gd.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def _two_layers(monkeypatch, name):
    monkeypatch.setitem(weights.OPENCLIP_CONFIGS, name, dataclasses.replace(weights.OPENCLIP_CONFIGS[name], layers=2))
    monkeypatch.setitem(weights.CLIP_TEXT_CONFIGS, name, dataclasses.replace(weights.CLIP_TEXT_CONFIGS[name], layers=2))


@pytest.mark.parametrize("name", ["ViT-g-14", "ViT-bigG-14"])
def test_real_geometry_graph_replay_matches_eager_session(tmp_path, monkeypatch, name):
    """a `fast_pixel` session on the tower's real geometry at 2 layers takes enable_graph(), and two replayed iterations equal two eager
    ones bit for bit; cutout noise is off (the device randn streams of capture and eager differ)"""
    from pixray_amd import frontend as fe
    from pixray_amd.engine import HipAdam
    _two_layers(monkeypatch, name)

    def build(tag):
        run = fe.Run()
        run.settings = dict(drawer="fast_pixel", clip_models=name, size=[64, 48], num_cuts=1, iterations=8, save_every=100,
                            display_every=100, outdir=str(tmp_path / tag), seed=5, skip_args=True, vector_prompts="none",
                            noise_prompt_seeds=[1], noise_prompt_weights=[1.0], learning_rate_drops=[])
        sess = fe.do_init(fe.apply_settings(run=run), run)
        for mk in sess.cutoutsTable.values():
            mk.noise_fac = 0.0
        return sess
    a, b = build("eager"), build("graph")
    assert isinstance(a.perceptors[name].handle, ops.OpenClipVitHandle) and a.perceptors[name].handle.cfg.layers == 2
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
@pytest.mark.parametrize("hd", [96, 112])
def test_a_head_dim_without_a_kernel_is_refused_by_name(hd):
    cfg = weights.OpenClipVitConfig(f"heads-of-{hd}", 224, 32, 8 * hd, 1, 8, 128)       # 768 / 896: multiples of 128
    params = weights.synthetic_clip_vit_params(cfg, 0)
    with pytest.raises(_lib.PrxError, match=f"head dim {hd}"):
        ops.OpenClipVitHandle(cfg, params, max_batch=1, device=DEV)


def test_more_than_640_tokens_at_128_columns_is_refused_by_name():
    cfg = weights.OpenClipVitConfig("bigG-heads-at-700-tokens", 14 * 27, 14, 1664, 1, 16, 128, mlp_width=256)     # 27 x 27 + 1 = 730 tokens
    params = weights.synthetic_clip_vit_params(cfg, 0)
    with pytest.raises(_lib.PrxError, match="heads of 104 run on the 128-wide attention kernels, which take at most 640 tokens"):
        ops.OpenClipVitHandle(cfg, params, max_batch=1, device=DEV)


def test_a_checkpoint_with_a_four_times_width_mlp_names_the_tensor():
    cfg = dataclasses.replace(weights.OPENCLIP_CONFIGS["ViT-bigG-14"], layers=1)
    wrong = weights.synthetic_clip_vit_params(dataclasses.replace(cfg, mlp_width=0), 0)          # c_fc [6656, 1664]
    sd = {"visual." + k: v for k, v in wrong.items()}
    with pytest.raises(ValueError, match=r"transformer\.resblocks\.0\.mlp\.c_fc\.weight: checkpoint has shape \(6656, 1664\), the configuration needs \(8192, 1664\)"):
        checkpoints.clip_visual_from_openclip(sd, cfg)
    with pytest.raises(ValueError, match=r"c_fc\.weight has shape \(6656, 1664\)"):          # ... and so does the handle, given the tensors directly
        ops.OpenClipVitHandle(cfg, wrong, max_batch=1, device=DEV)


# ------------------------------------------------------------------------------------------ one run through the front end
def test_one_vit_g_14_run_through_the_front_end(tmp_path, monkeypatch):
    """`--drawer fast_pixel --clip_models ViT-g-14 --quality draft --num_cuts 2 --size 64 48`, 2 iterations through do_init / do_run on
    the HIP parts, with both towers' configurations cut to 2 layers (the front end builds synthetic weights for what the tables say)"""
    from PIL import Image
    from pixray_amd import frontend as fe
    _two_layers(monkeypatch, "ViT-g-14")
    run = fe.Run()
    run.settings = dict(drawer="fast_pixel", clip_models="ViT-g-14", quality="draft", num_cuts=2, size=[64, 48], iterations=2, save_every=1,
                        display_every=2, outdir=str(tmp_path / "out"), seed=5, skip_args=True, vector_prompts="none", noise_prompt_seeds=[1],
                        noise_prompt_weights=[1.0], learning_rate_drops=[])
    s = fe.apply_settings(run=run)
    sess = fe.do_init(s, run, device=None)
    assert sess.cutoutSizeTable == {"ViT-g-14": 224}
    perc = sess.perceptors["ViT-g-14"]
    assert isinstance(perc.handle, ops.OpenClipVitHandle) and perc.handle.cfg.mlp == 6144 and perc.handle.cfg.head_dim == 88 and perc.text_cfg.gelu
    z0 = sess.drawer.get_z_copy()
    while not fe.do_run(s, return_display=True, run=run):
        pass
    assert sess.cur_iteration == 2 and len(sess.last_losses) >= 1 and all(torch.isfinite(l).all() for l in sess.last_losses)
    assert float((sess.drawer.get_z().detach() - z0).abs().max()) > 0.0
    img = Image.open(os.path.join(s.outdir, "output.png"))
    assert img.size == (64, 48) and "ViT-g-14" in img.info["pixray_clip_models"]
