"""Kernel-level parity tests (GPU) of the runners' PRIVATE kernels: the CLIP-ResNet stem, pools and attention-pool token kernels
(resnet.hip), batch min / max, patchify and the min/max renormalisation backward (cutouts.hip), the VGG pools and gradient routing
(vgg.hip), the ViT / text embedding kernels (vit.hip, clip_text.hip), l2norm / sqnorm_rows (prompt_vq.hip) and the weight packers.
Each is reached through `prx_k_*` -> the host launcher its runner itself calls (grid computation, operand type / CO dispatch), so
the launch code under test is the product's.

The method is tests/test_kernels_half_gpu.py's (its helpers are imported, not copied): inputs are rounded to the format the kernel
reads, a plain torch expression is evaluated in FLOAT64 on those rounded inputs, outputs are pre-filled with NaN and carry spare
rows that must come back untouched, and every kernel templated on the operand type runs at bf16, fp16 and f32.  Tolerances -- three
rules, none tuned against a kernel's output:

* R1, data movement and conversion: bit equality with torch's round-to-nearest-even conversion (half saturating at +-65504);
* R2, short fp32 chains: |out - ref64| <= [ulp16(ref64) if the output is 16-bit] + k * 2^-24 * A, A = the sum of the absolute values
  of the float64 terms at that element, k = the fp32 roundings of the kernel's chain, counted in a comment beside each use;
* R3, behind a reduction or a library erff / expf (l2norm, sqnorm_rows, gelu_f32): rel-L2 gate = 4 x the rel-L2 error of torch's own
  fp32 evaluation of the same op against the float64 reference (reference against reference), never above 1e-5."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from pixray_amd import _lib
from pixray_amd._lib import PrxError, call, PREC_BF16, PREC_F32, PREC_F16

import test_kernels_half_gpu as th
from test_kernels_half_gpu import guarded, untouched, within, check16, ulp16, to16, bits, EXPF_REL  # noqa: F401

DEV = "cuda"          # tests/test_emu_cpu.py switches this (and the helper module's) to "cpu" for the emulated kernels
EPS32 = 2.0 ** -24
NAN = float("nan")
PRECS = [PREC_BF16, PREC_F16, PREC_F32]
PREC_IDS = ["bf16", "fp16", "f32"]
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
IMNET_MEAN, IMNET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)                # slip.py's ImageNet set
prec_all = pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)


def stream():
    return _lib.current_stream()


def sync():
    torch.cuda.synchronize()


def odt(prec):
    return {PREC_BF16: torch.bfloat16, PREC_F16: torch.float16, PREC_F32: torch.float32}[prec]


def cvt(x, prec):
    """the operand-format conversion of an fp32 tensor (R1): round to nearest even, half saturates"""
    return x.float() if prec == PREC_F32 else to16(x.float(), prec == PREC_F16)


def rnd(shape, prec, scale=1.0, shift=0.0):
    """random values already rounded to the operand format of `prec`"""
    return cvt(torch.randn(*shape, device=DEV) * scale + shift, prec)


def f32c(vals):
    """fp32 constants as the kernel holds them, in float64"""
    return torch.tensor(vals, dtype=torch.float32, device=DEV).double()


def flat(n, dtype):
    """a NaN-filled flat buffer of n elements with spare rows of n behind it"""
    full, win = guarded(1, n, dtype)
    return full, win[0]


def check_op(out, ref64, prec, k, A):
    """R2 for an output in the operand format of `prec`"""
    if prec == PREC_F32:
        ok, worst = within(out, ref64, k * EPS32 * A)
        assert ok, ("fp32 output off by more than the counted chain", worst)
    else:
        check16(out, ref64, prec == PREC_F16, k * EPS32, A)


def check_f32(out, ref64, k, A):
    ok, worst = within(out, ref64, k * EPS32 * A)
    assert ok, ("fp32 output off by more than the counted chain", worst)


def same_bits(out, ref):
    assert out.dtype == ref.dtype and out.shape == ref.shape, (out.dtype, ref.dtype, out.shape, ref.shape)
    assert torch.equal(bits(out), bits(ref)), ("bits differ at", int((bits(out) != bits(ref)).flatten().nonzero()[0]))


def rel_l2(a, b):
    return th.rel_l2(a, b)


# ================================================================================================ weight packers (R1)
def _pack_weights(Cout, Cin):
    w = torch.randn(Cout, Cin, 3, 3, device=DEV)
    w.view(-1)[0] = 1e6                     # beyond the half range: saturates
    w.view(-1)[-1] = -7e4
    return w


@prec_all
@pytest.mark.parametrize("Cout,Cin", [(5, 3), (16, 8)])
def test_rn_pack_conv3x3(Cout, Cin, prec):
    """Wf[co][tap*Cin + ci] = w[co][ci][ky][kx];  Wd[ci][tap'*Cout + co] = w[co][ci][2-ky][2-kx]"""
    torch.manual_seed(Cout)
    w = _pack_weights(Cout, Cin)
    ff, Wf = guarded(Cout, 9 * Cin, odt(prec))
    fd, Wd = guarded(Cin, 9 * Cout, odt(prec))
    call("prx_k_rn_pack_conv3x3", w, ff, fd, Cout, Cin, prec, stream())
    sync()
    same_bits(Wf, cvt(w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin), prec))
    same_bits(Wd, cvt(w.flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, 9 * Cout), prec))
    assert untouched(ff, Cout, 9 * Cin) and untouched(fd, Cin, 9 * Cout)


@prec_all
@pytest.mark.parametrize("Cout,Cin,CiP", [(5, 3, 8), (8, 8, 8)])
def test_vgg_pack(Cout, Cin, CiP, prec):
    """as above with the input channels zero-padded to CiP in both packs"""
    torch.manual_seed(Cout)
    w = _pack_weights(Cout, Cin)
    wp = F.pad(w, (0, 0, 0, 0, 0, CiP - Cin))
    ff, Wf = guarded(Cout, 9 * CiP, odt(prec))
    fd, Wd = guarded(CiP, 9 * Cout, odt(prec))
    call("prx_k_vgg_pack", w, ff, fd, Cout, Cin, CiP, prec, stream())
    sync()
    same_bits(Wf, cvt(wp.permute(0, 2, 3, 1).reshape(Cout, 9 * CiP), prec))
    same_bits(Wd, cvt(wp.flip(2, 3).permute(1, 2, 3, 0).reshape(CiP, 9 * Cout), prec))
    assert untouched(ff, Cout, 9 * CiP) and untouched(fd, CiP, 9 * Cout)


@prec_all
@pytest.mark.parametrize("Cout,Cin,CoP", [(3, 8, 8), (8, 5, 8)])
def test_vqgan_pack_conv3x3(Cout, Cin, CoP, prec):
    """the decoder's pack: Wd's OUTPUT channels zero-padded to CoP; Wf gets Cout rows (the runner zeroes the rest itself)"""
    torch.manual_seed(Cout)
    w = _pack_weights(Cout, Cin)
    wp = F.pad(w, (0, 0, 0, 0, 0, 0, 0, CoP - Cout))
    ff, Wf = guarded(Cout, 9 * Cin, odt(prec))
    fd, Wd = guarded(Cin, 9 * CoP, odt(prec))
    call("prx_k_vqgan_pack_conv3x3", w, ff, fd, Cout, Cin, CoP, prec, stream())
    sync()
    same_bits(Wf, cvt(w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin), prec))
    same_bits(Wd, cvt(wp.flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, 9 * CoP), prec))
    assert untouched(ff, Cout, 9 * Cin) and untouched(fd, Cin, 9 * CoP)


@pytest.mark.parametrize("Cout,Cin,CiP", [(5, 3, 8), (4, 16, 16)])
def test_vqgan_enc_pack_conv3x3(Cout, Cin, CiP):
    """the encoder's forward pack (bf16 only), input channels zero-padded to CiP"""
    torch.manual_seed(Cout)
    w = _pack_weights(Cout, Cin)
    wp = F.pad(w, (0, 0, 0, 0, 0, CiP - Cin))
    ff, Wf = guarded(Cout, 9 * CiP, torch.bfloat16)
    call("prx_k_vqgan_enc_pack_conv3x3", w, ff, Cout, Cin, CiP, stream())
    sync()
    same_bits(Wf, wp.permute(0, 2, 3, 1).reshape(Cout, 9 * CiP).to(torch.bfloat16))
    assert untouched(ff, Cout, 9 * CiP)


@prec_all
@pytest.mark.parametrize("Cout,Cin,CiP,CoP,sides", [(5, 3, 8, 8, "fd"), (8, 8, 8, 8, "fd"), (5, 3, 8, 8, "f"), (5, 3, 8, 8, "d")])
def test_pack_conv3x3(Cout, Cin, CiP, CoP, sides, prec):
    """the one pack kernel behind the four entries above: input channels zero-padded to CiP and output channels to CoP at once;
    Wf gets Cout rows; a null pack is not written (`sides`: f = Wf, d = Wd)"""
    torch.manual_seed(Cout)
    w = _pack_weights(Cout, Cin)
    wi = F.pad(w, (0, 0, 0, 0, 0, CiP - Cin))
    wp = F.pad(wi, (0, 0, 0, 0, 0, 0, 0, CoP - Cout))
    ff, Wf = guarded(Cout, 9 * CiP, odt(prec))
    fd, Wd = guarded(CiP, 9 * CoP, odt(prec))
    call("prx_k_pack_conv3x3", w, ff if "f" in sides else None, fd if "d" in sides else None, Cout, Cin, CiP, CoP, prec, stream())
    sync()
    if "f" in sides:
        same_bits(Wf, cvt(wi.permute(0, 2, 3, 1).reshape(Cout, 9 * CiP), prec))
        assert untouched(ff, Cout, 9 * CiP)
    else:
        assert bool(torch.isnan(ff).all())
    if "d" in sides:
        same_bits(Wd, cvt(wp.flip(2, 3).permute(1, 2, 3, 0).reshape(CiP, 9 * CoP), prec))
        assert untouched(fd, CiP, 9 * CoP)
    else:
        assert bool(torch.isnan(fd).all())


def test_pack_conv3x3_refuses_no_pack_and_a_padded_size_below_the_channels():
    w = _pack_weights(5, 3)
    ff, _ = guarded(5, 9 * 8, torch.float16)
    fd, _ = guarded(8, 9 * 8, torch.float16)
    with pytest.raises(PrxError, match="neither pack"):
        call("prx_k_pack_conv3x3", w, None, None, 5, 3, 8, 8, PREC_F16, stream())
    with pytest.raises(PrxError, match="do not fit"):
        call("prx_k_pack_conv3x3", w, ff, fd, 5, 3, 2, 8, PREC_F16, stream())
    sync()
    assert bool(torch.isnan(ff).all()) and bool(torch.isnan(fd).all())          # no launch


@pytest.mark.parametrize("rows,D", [(7, 1), (5, 300)])
def test_colminmax(rows, D):
    """per-column minimum / maximum (exact); D = 300: a second, partial workgroup"""
    torch.manual_seed(D)
    w = torch.randn(rows, D, device=DEV)
    fmn, mn = flat(D, torch.float32)
    fmx, mx = flat(D, torch.float32)
    call("prx_k_colminmax", w, fmn, fmx, rows, D, stream())
    sync()
    same_bits(mn, w.min(dim=0).values)
    same_bits(mx, w.max(dim=0).values)
    assert untouched(fmn, 1, D) and untouched(fmx, 1, D)


@prec_all
@pytest.mark.parametrize("R,C", [(33, 70), (1, 1)])
def test_pack_transpose(R, C, prec):
    """out[c][r] = convert(in[r][c]); 33 x 70: ragged against the 32 x 32 tile in both directions"""
    torch.manual_seed(R)
    x = torch.randn(R, C, device=DEV) * 3
    x[0, 0] = 1e6
    full, out = guarded(C, R, odt(prec))
    call("prx_k_pack_transpose_op", x, full, R, C, prec, stream())
    sync()
    same_bits(out, cvt(x.t().contiguous(), prec))
    assert untouched(full, C, R)


# ================================================================================================ ResNet stem
STEM_CO = [8, 16, 32, 40, 48, 64]
# (N, S): 243 output pixels = one partial 256-pixel tile; 405 = a full tile + a partial tile of 149 (the staged store's tail);
# a single output pixel with every tap but four outside the image
STEM_SHAPES = [(3, 18), (5, 18), (1, 2)]


def _stem_inputs(N, S, CO, constant=False):
    torch.manual_seed(100 * N + S + CO)
    cut = torch.full((N, 3, S, S), 0.375, device=DEV) if constant else torch.rand(N, 3, S, S, device=DEV)
    mm = torch.stack([cut.min(), cut.max()])                     # the true min / max
    w = torch.randn(CO, 3, 3, 3, device=DEV) * 0.3
    b = torch.randn(CO, device=DEV) * 0.2
    return cut, mm, w, b


def _normalise64(cut, mm, mean, std):
    """slip.py:21-42 in float64 on the kernel's fp32 inputs: (xn, A) with A = the sum of the absolute terms of xn"""
    x, mn, mx = cut.double(), mm[0].double(), mm[1].double()
    inv = 1.0 / (mx - mn) if float(mx - mn) != 0.0 else 1.0            # range == 0: the kernels take inv = 1
    m, s = f32c(mean).view(1, 3, 1, 1), f32c(std).view(1, 3, 1, 1)
    return ((x - mn) * inv - m) / s, ((x.abs() + mn.abs()) * inv + m) / s


def stem_fwd_case(N, S, CO, prec, constant=False):
    cut, mm, w, b = _stem_inputs(N, S, CO, constant)
    So = S // 2
    rows = N * So * So
    full, out = guarded(rows, CO, odt(prec))
    call("prx_k_stem1_fwd", cut, mm, w, b, full, N, S, CO, prec, stream())
    sync()
    xn, An = _normalise64(cut, mm, CLIP_MEAN, CLIP_STD)
    ref = F.relu(F.conv2d(xn, w.double(), b.double(), stride=2, padding=1)).permute(0, 2, 3, 1).reshape(rows, CO)
    A = (F.conv2d(An, w.double().abs(), b.double().abs(), stride=2, padding=1)).permute(0, 2, 3, 1).reshape(rows, CO)
    # k = 4 (the normalisation: sub, mul, sub, mul) + 27 (bias + 27 multiply-adds, one rounding each); ReLU is 1-Lipschitz
    check_op(out, ref, prec, 4 + 27, A)
    assert untouched(full, rows, CO)


@prec_all
@pytest.mark.parametrize("CO", STEM_CO)
def test_stem1_fwd(CO, prec):
    """stem1_fwd_kernel<TOp, CO>: every CO case of the dispatch at every operand type; the 16-bit builds stage an LDS tile and write it
    out in 16-byte pieces (partial last tile: npix * CO * sizeof(TOp) / 16 pieces), the fp32 build stores directly"""
    for N, S in STEM_SHAPES:
        stem_fwd_case(N, S, CO, prec)
    stem_fwd_case(2, 6, CO, prec, constant=True)            # range == 0 -> inv = 1


def stem_bwd_case(N, S, CO, prec, oscale):
    torch.manual_seed(N + S + CO)
    So = S // 2
    g = rnd((N, So, So, CO), prec)
    w = torch.randn(CO, 3, 3, 3, device=DEV) * 0.3
    osc = None if oscale is None else torch.tensor([oscale], device=DEV)
    full, dY = guarded(N * 3 * S, S, torch.float32)
    call("prx_k_stem1_bwd", g, w, full, N, S, CO, osc, prec, stream())
    sync()
    o = 1.0 if oscale is None else oscale
    g64 = g.double().permute(0, 3, 1, 2)
    # = the float64 autograd gradient of the stem convolution w.r.t. its (normalised) input
    ref = F.conv_transpose2d(g64, w.double(), stride=2, padding=1, output_padding=1) * o
    A = F.conv_transpose2d(g64.abs(), w.double().abs(), stride=2, padding=1, output_padding=1) * o
    assert ref.shape == (N, 3, S, S)
    # k: at most 4 taps x CO multiply-adds reach a pixel, + the oscale multiply
    check_f32(dY, ref.reshape(N * 3 * S, S), 4 * CO + 1, A.reshape(N * 3 * S, S))
    assert untouched(full, N * 3 * S, S)


@prec_all
@pytest.mark.parametrize("CO", STEM_CO)
def test_stem1_bwd(CO, prec):
    """stem1_bwd_kernel<TOp, CO> against conv_transpose2d in float64; with oscale_dev null and 2^-5 (the half mode's unscale)"""
    for N, S in STEM_SHAPES:
        for oscale in (None, 2.0 ** -5):
            stem_bwd_case(N, S, CO, prec, oscale)


def test_stem_refuses_a_width_it_has_no_kernel_for():
    cut, mm, w, b = _stem_inputs(1, 4, 24)
    full, _ = guarded(4, 24, torch.float16)
    with pytest.raises(PrxError, match="not one of 8, 16, 32, 40, 48, 64"):
        call("prx_k_stem1_fwd", cut, mm, w, b, full, 1, 4, 24, PREC_F16, stream())
    fdy, _ = guarded(3 * 4, 4, torch.float32)
    with pytest.raises(PrxError, match="not one of 8, 16, 32, 40, 48, 64"):
        call("prx_k_stem1_bwd", torch.zeros(4, 24, dtype=torch.float16, device=DEV), w, fdy, 1, 4, 24, None, PREC_F16, stream())
    sync()
    assert bool(torch.isnan(full).all()) and bool(torch.isnan(fdy).all())          # no launch


# ================================================================================================ 2x2 average pool, ReLU mask
POOL_SHAPES = [(2, 6, 10, 4), (1, 2, 2, 40), (3, 4, 4, 64)]


@prec_all
@pytest.mark.parametrize("N,H,W,C", POOL_SHAPES)
def test_avgpool2_fwd(N, H, W, C, prec):
    torch.manual_seed(H * W + C)
    x = rnd((N, H, W, C), prec)
    rows = N * (H // 2) * (W // 2)
    full, out = guarded(rows, C, odt(prec))
    call("prx_k_avgpool2_fwd", x, full, N, H, W, C, prec, stream())
    sync()
    x64 = x.double().permute(0, 3, 1, 2)
    ref = F.avg_pool2d(x64, 2).permute(0, 2, 3, 1).reshape(rows, C)
    A = F.avg_pool2d(x64.abs(), 2).permute(0, 2, 3, 1).reshape(rows, C)
    check_op(out, ref, prec, 3, A)                 # k = 3: three additions (the multiplication by 0.25 is exact)
    assert untouched(full, rows, C)


@prec_all
@pytest.mark.parametrize("outs", ["op", "f32", "both"])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("N,H,W,C", POOL_SHAPES)
def test_avgpool2_bwd(N, H, W, C, masked, outs, prec):
    """dx = 0.25 * g (exact) where the mask is > 0: +0.0, -0.0 and negative mask entries all block the gradient (R1)"""
    torch.manual_seed(H * W + C)
    g = torch.randn(N, H // 2, W // 2, C, device=DEV)
    mask = None
    if masked:
        mask = rnd((N, H, W, C), prec)
        mf = mask.view(-1)
        mf[0::5] = 0.0
        mf[1::5] = -0.0
        assert bool((mask < 0).any()) and bool((mask > 0).any())
    rows = N * H * W
    f32_full, d32 = guarded(rows, C, torch.float32) if outs in ("f32", "both") else (None, None)
    op_full, dop = guarded(rows, C, odt(prec)) if outs in ("op", "both") else (None, None)
    call("prx_k_avgpool2_bwd", g, mask, f32_full, op_full, N, H, W, C, prec, stream())
    sync()
    up = (0.25 * g).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    ref = torch.where(mask.float() > 0, up, torch.zeros_like(up)) if masked else up
    ref = ref.reshape(rows, C)
    if d32 is not None:
        same_bits(d32, ref)
        assert untouched(f32_full, rows, C)
    if dop is not None:
        same_bits(dop, cvt(ref, prec))
        assert untouched(op_full, rows, C)


@prec_all
def test_relu_mask(prec):
    """g <- g * [out > 0] in place, and its operand-format twin (R1); 1000 elements: four workgroups, the last one partial"""
    torch.manual_seed(5)
    n = 1000
    o = rnd((n,), prec)
    o[0::7] = 0.0
    o[1::7] = -0.0
    g0 = torch.randn(n, device=DEV) * 300
    g0[3] = 1e6
    gfull, g = flat(n, torch.float32)
    g.copy_(g0)
    tfull, twin = flat(n, odt(prec))
    call("prx_k_relu_mask", gfull, o, tfull, n, prec, stream())
    sync()
    ref = torch.where(o.float() > 0, g0, torch.zeros_like(g0))
    same_bits(g, ref)
    same_bits(twin, cvt(ref, prec))
    assert untouched(gfull, 1, n) and untouched(tfull, 1, n)


# ================================================================================================ attention-pool tokens
TOKEN_SHAPES = [(3, 9, 24), (1, 49, 64)]


@prec_all
@pytest.mark.parametrize("N,P,C", TOKEN_SHAPES)
def test_tokens_fwd(N, P, C, prec):
    """t[n][0] = mean_p x[n][p] + pos[0];  t[n][1 + p] = x[n][p] + pos[1 + p]"""
    torch.manual_seed(P)
    x = torch.randn(N, P, C, device=DEV) + 0.5
    pos = torch.randn(P + 1, C, device=DEV)
    full, t = guarded(N * (P + 1), C, odt(prec))
    call("prx_k_tokens_fwd", x, pos, full, N, P, C, prec, stream())
    sync()
    x64, p64 = x.double(), pos.double()
    t = t.reshape(N, P + 1, C)
    check_op(t[:, 1:], x64 + p64[1:], prec, 1, x64.abs() + p64[1:].abs())                            # k = 1: one addition
    # k = P + 2: P additions, the division, the addition of pos[0]
    check_op(t[:, 0], x64.mean(dim=1) + p64[0], prec, P + 2, x64.abs().mean(dim=1) + p64[0].abs())
    assert untouched(full, N * (P + 1), C)


@prec_all
@pytest.mark.parametrize("N,P,C", TOKEN_SHAPES)
def test_tokens_bwd(N, P, C, prec):
    """dx[n][p] = dt[n][1 + p] + dt[n][0] / P"""
    torch.manual_seed(P + 1)
    dt = torch.randn(N, P + 1, C, device=DEV)
    full, dx = guarded(N * P, C, torch.float32)
    call("prx_k_tokens_bwd", dt, full, N, P, C, prec, stream())
    sync()
    d64 = dt.double()
    ref = d64[:, 1:] + d64[:, :1] / P
    A = d64[:, 1:].abs() + d64[:, :1].abs() / P
    check_f32(dx.reshape(N, P, C), ref, 3, A)        # k = 3: 1 / P, the multiplication by it, the addition
    assert untouched(full, N * P, C)


@prec_all
def test_tok0_gather_and_scatter(prec):
    """row 0 of every image's tokens out, and back into exact zeros everywhere else (R1)"""
    torch.manual_seed(2)
    N, T, C = 3, 10, 24
    t = rnd((N, T, C), prec)
    gfull, out = guarded(N, C, odt(prec))
    call("prx_k_tok0_gather", t, gfull, N, T, C, prec, stream())
    sfull, dt = guarded(N * T, C, odt(prec))
    g0 = rnd((N, C), prec)
    call("prx_k_tok0_scatter", g0, sfull, N, T, C, prec, stream())
    sync()
    same_bits(out, t[:, 0].contiguous())
    ref = torch.zeros(N, T, C, dtype=odt(prec), device=DEV)
    ref[:, 0] = g0
    same_bits(dt, ref.reshape(N * T, C))              # bit equality: the other rows are +0.0
    assert untouched(gfull, N, C) and untouched(sfull, N * T, C)


# ================================================================================================ batch min / max
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset-by-one-float"])
@pytest.mark.parametrize("nparts", [1, 64])
@pytest.mark.parametrize("n", [1, 3, 4, 7, 1023, 4099])
def test_minmax(n, nparts, offset):
    """minmax_partial_kernel + minmax_final_kernel: exact.  A 16-byte aligned base takes the float4 path (+ its scalar tail of n % 4),
    a base offset by one float the scalar path; all-negative data; the extrema placed in the last n % 4 elements"""
    torch.manual_seed(n + nparts)
    buf = torch.empty(n + 9, device=DEV)
    assert buf.data_ptr() % 16 == 0
    for variant in ("random", "negative", "tail"):
        x = buf[offset:offset + n]
        x.copy_(torch.randn(n, device=DEV))
        if variant == "negative":
            x.copy_(-x.abs() - 1.0)
        if variant == "tail":
            x[n - 1] = 50.0                               # inside the scalar tail of n % 4 elements whenever there is one
            if n > 1:
                x[n - n % 4 if n % 4 >= 2 else n - 2] = -60.0         # the first tail element when the tail holds two or more
        pfull, part = flat(2 * nparts, torch.float32)
        mfull, mm = flat(2, torch.float32)
        call("prx_k_minmax", x, n, pfull, nparts, mfull, stream())
        sync()
        assert mm.tolist() == [float(x.min()), float(x.max())], (variant, mm.tolist())
        assert not bool(torch.isnan(part).any()) and untouched(pfull, 1, 2 * nparts) and untouched(mfull, 1, 2)


# ================================================================================================ patchify and the renormalisation backward
PATCH_SHAPES = [(32, 16), (28, 14), (8, 4)]        # fast path (P % 8 == 0); slow path with K = 588 padded to 592; slow path, small K
NORMS = {"clip": (CLIP_MEAN, CLIP_STD), "imagenet": (IMNET_MEAN, IMNET_STD)}


def _to_rows(img, N, S, P):
    """[N][3][S][S] -> [N][G*G][3*P*P]: row gy*G + gx, column c*P*P + py*P + px"""
    G = S // P
    return img.reshape(N, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(N, G * G, 3 * P * P)


def _to_image(rows, N, S, P):
    G = S // P
    return rows.reshape(N, G, G, 3, P, P).permute(0, 3, 1, 4, 2, 5).reshape(N, 3, S, S)


def _kp(P):
    return (3 * P * P + 7) // 8 * 8


@prec_all
@pytest.mark.parametrize("norm", ["clip", "imagenet"])
@pytest.mark.parametrize("S,P", PATCH_SHAPES)
def test_patchify_fwd(S, P, norm, prec):
    torch.manual_seed(S)
    N, G = 3, S // P
    T, K, Kp = G * G + 1, 3 * P * P, _kp(P)
    mean, std = NORMS[norm]
    cut = torch.rand(N, 3, S, S, device=DEV)
    mm = torch.stack([cut.min(), cut.max()])
    full, A_ = guarded(N * T, Kp, odt(prec))
    call("prx_k_patchify_fwd", cut, mm, full, prec, N, S, P, T, *mean, *std, stream())
    sync()
    xn, An = _normalise64(cut, mm, mean, std)
    out = A_.reshape(N, T, Kp)
    # k = 7: x - mn, mx - mn, 1 / range, the product, - mean, 1 / std, the product (the slow path divides by std instead: 6)
    check_op(out[:, 1:, :K], _to_rows(xn, N, S, P), prec, 7, _to_rows(An, N, S, P))
    assert bool((bits(out[:, 0]) == 0).all()) and bool((bits(out[:, :, K:]) == 0).all())        # class-token rows, padding columns: +0.0
    assert untouched(full, N * T, Kp)


def _renorm_case(N, S, constant=False):
    """cutouts whose minimum occurs three times and whose maximum twice (or constant cutouts: range == 0)"""
    cut = torch.rand(N, 3, S, S, device=DEV) * 0.8 + 0.1
    if constant:
        cut.fill_(0.625)
    else:
        f = cut.view(-1)
        n = f.numel()
        f[[5, n // 2, n - 3]] = 0.03125
        f[[17, n - 1]] = 0.96875
    mm = torch.stack([cut.min(), cut.max()])
    return cut, mm


def _renorm_bwd_ref(cut, mm, gimg64, std):
    """float64: (gy, y, acc, gcut); the gradient of a tied extremum is shared 1 / count (the kernel's documented split)"""
    x, mn, mx = cut.double(), mm[0].double(), mm[1].double()
    live = float(mx - mn) != 0.0
    inv = 1.0 / (mx - mn) if live else 1.0
    gy = gimg64 / f32c(std).view(1, 3, 1, 1)
    y = (x - mn) * inv
    ismin, ismax = (x == mn), (x == mx)
    acc = torch.stack([gy.sum(), (gy * y).sum(), ismin.sum().double(), ismax.sum().double()])
    gmin = (acc[1] - acc[0]) * inv / acc[2] if live else 0.0             # d y / d min = (y - 1) / range
    gmax = -acc[1] * inv / acc[3] if live else 0.0                       # d y / d max = -y / range
    gcut = gy * inv + ismin * gmin + ismax * gmax
    A = (gy * inv).abs() + ismin * abs(gmin) + ismax * abs(gmax)
    return gy, y, acc, gcut, A, inv


def _check_reduce(acc, cut, mm, gimg64, std):
    gy, y, ref, _, _, inv = _renorm_bwd_ref(cut, mm, gimg64, std)
    x, mn = cut.double(), mm[0].double()
    # the sums run in double over fp32 terms.  k = 1 for sum gy (the division by std); k = 6 for sum gy * y: the division, x - mn,
    # mx - mn, 1 / range, the product y, the product gy * y.  The two counts are exact.
    A0 = gy.abs().sum()
    A1 = (gy.abs() * (x.abs() + mn.abs()) * inv).sum()
    ok, worst = within(acc[:2], ref[:2], torch.stack([1 * EPS32 * A0, 6 * EPS32 * A1]))
    assert ok, ("renormalisation sums", worst)
    assert acc[2:4].tolist() == ref[2:].tolist(), (acc.tolist(), ref.tolist())
    return ref


def _autograd_check(cut, gimg64, mean, std, gcut_ref):
    """the explicit float64 formula above IS the autograd gradient of ((x - min) / (max - min) - mean) / std (amin / amax share a tied
    extremum's gradient evenly, as the kernel does) -- a check of this test's own algebra"""
    x = cut.double().requires_grad_(True)
    m, s = f32c(mean).view(1, 3, 1, 1), f32c(std).view(1, 3, 1, 1)
    f = ((x - x.amin()) / (x.amax() - x.amin()) - m) / s
    (gx,) = torch.autograd.grad(f, x, gimg64)
    assert rel_l2(gx, gcut_ref) < 1e-12


def patchify_bwd_case(S, P, norm, constant=False, N=3):
    torch.manual_seed(S + P)
    G = S // P
    T, K, Kp = G * G + 1, 3 * P * P, _kp(P)
    mean, std = NORMS[norm]
    cut, mm = _renorm_case(N, S, constant)
    dA = torch.randn(N * T, Kp, device=DEV)
    gimg64 = _to_image(dA.reshape(N, T, Kp)[:, 1:, :K].double(), N, S, P)
    afull, acc = flat(4, torch.float64)
    call("prx_k_patchify_bwd_reduce", cut, mm, dA, afull, N, S, P, T, *mean, *std, stream())
    sync()
    ref_acc = _check_reduce(acc, cut, mm, gimg64, std)
    assert untouched(afull, 1, 4)
    _, _, _, gref, A, _ = _renorm_bwd_ref(cut, mm, gimg64, std)
    if not constant:
        _autograd_check(cut, gimg64, mean, std, gref)
    gfull, gcut = guarded(N * 3 * S, S, torch.float32)
    call("prx_k_patchify_bwd_apply", cut, mm, dA, ref_acc.contiguous(), gfull, N, S, P, T, *mean, *std, stream())      # the float64 sums: apply alone
    sync()
    # k = 8: gy (1), inv (2), gy * inv (1); at an extremum gmin / gmax (inv: 2, the conversion to fp32: 1) and its addition (1)
    check_f32(gcut, gref.reshape(N * 3 * S, S), 8, A.reshape(N * 3 * S, S))
    assert untouched(gfull, N * 3 * S, S)
    return acc.clone()


@pytest.mark.parametrize("norm", ["clip", "imagenet"])
@pytest.mark.parametrize("S,P", PATCH_SHAPES)
def test_patchify_bwd_reduce_and_apply(S, P, norm):
    """min three times, max twice: the extrema's gradient is shared by the counts; a wrong sign on gmax, a dropped count or a
    swapped px / py would each show here"""
    patchify_bwd_case(S, P, norm)


def test_patchify_bwd_constant_cutouts():
    """range == 0: inv = 1 and the extrema terms vanish"""
    patchify_bwd_case(8, 4, "clip", constant=True)


@pytest.mark.parametrize("constant", [False, True])
def test_preproc_bwd_reduce_and_apply(constant):
    """the same two kernels on an image-layout gradient dY[N][3][S][S] (one `patch` = the image, T = 1, the pointer shifted back by one
    row of K): pins the `dY - K` row trick"""
    torch.manual_seed(12)
    N, S = 3, 12
    cut, mm = _renorm_case(N, S, constant)
    dY = torch.randn(N, 3, S, S, device=DEV)
    afull, acc = flat(4, torch.float64)
    call("prx_k_preproc_bwd_reduce", cut, mm, dY, afull, N, S, stream())
    sync()
    ref_acc = _check_reduce(acc, cut, mm, dY.double(), CLIP_STD)
    _, _, _, gref, A, _ = _renorm_bwd_ref(cut, mm, dY.double(), CLIP_STD)
    if not constant:
        _autograd_check(cut, dY.double(), CLIP_MEAN, CLIP_STD, gref)
    gfull, gcut = guarded(N * 3 * S, S, torch.float32)
    call("prx_k_preproc_bwd_apply", cut, mm, dY, ref_acc.contiguous(), gfull, N, S, stream())
    sync()
    check_f32(gcut, gref.reshape(N * 3 * S, S), 8, A.reshape(N * 3 * S, S))          # k = 8: as in patchify_bwd_case
    assert untouched(afull, 1, 4) and untouched(gfull, N * 3 * S, S)


# ================================================================================================ VGG16 pools and gradient routing
VGG_SHAPES = [(7, 9, 8), (4, 4, 64)]        # both sides odd: the last row and column are outside every window


def _pool_ref(x):
    """2 x 2 stride-2 max pool of [H][W][C], written out: scan (0,0), (0,1), (1,0), (1,1), a later tap wins only when strictly greater"""
    H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    xf = x.float()
    best = xf[0:2 * Ho:2, 0:2 * Wo:2].clone()
    arg = torch.zeros(Ho, Wo, C, dtype=torch.uint8, device=x.device)
    for a, (dy, dx) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        if a == 0:
            continue
        v = xf[dy:2 * Ho:2, dx:2 * Wo:2]
        win = v > best
        best = torch.where(win, v, best)
        arg = torch.where(win, torch.full_like(arg, a), arg)
    return best, arg


def _tied_map(H, W, C, prec):
    """small integers (exact in every format): most windows hold a 2-way tie, many a 3- or 4-way one"""
    x = torch.randint(-2, 3, (H, W, C), device=DEV).float()
    x[0:2, 0:2, 0] = 1.0                     # a 4-way tie
    x[0:2, 2:4, 0] = torch.tensor([[0.0, 2.0], [2.0, 1.0]], device=DEV)     # a 2-way tie of taps 1 and 2
    return cvt(x * 0.5, prec)


@prec_all
@pytest.mark.parametrize("H,W,C", VGG_SHAPES)
def test_vgg_maxpool(H, W, C, prec):
    """value and argument, bit for bit (R1); the first maximum in scan order wins a tie"""
    torch.manual_seed(H)
    x = _tied_map(H, W, C, prec)
    Ho, Wo = H // 2, W // 2
    ofull, out = guarded(Ho * Wo, C, odt(prec))
    afull = torch.full((Ho * Wo + 3, C), 255, dtype=torch.uint8, device=DEV)
    call("prx_k_vgg_maxpool", x, ofull, afull, H, W, C, prec, stream())
    sync()
    best, arg = _pool_ref(x)
    same_bits(out, cvt(best, prec).reshape(Ho * Wo, C))
    assert torch.equal(afull[:Ho * Wo], arg.reshape(Ho * Wo, C)) and bool((afull[Ho * Wo:] == 255).all())
    assert int((arg == 0).sum()) > 0 and int((arg == 3).sum()) > 0
    assert untouched(ofull, Ho * Wo, C)


@prec_all
@pytest.mark.parametrize("gscale", [None, 2.0 ** 6])
@pytest.mark.parametrize("mode", ["none", "gcap", "above", "above+gcap", "routed", "routed+gcap"])
@pytest.mark.parametrize("H,W,C", VGG_SHAPES)
def test_vgg_combine(H, W, C, mode, gscale, prec):
    """gpre = [act > 0] * (above routed through the pool argument + S * gcap): every null / non-null combination; S multiplies the
    captured gradient only (`above` already carries it)"""
    torch.manual_seed(H + len(mode))
    Ho, Wo = H // 2, W // 2
    act = rnd((H, W, C), prec)
    act.view(-1)[0::3] = 0.0
    routed = mode.startswith("routed")
    above = arg = gcap = None
    ab64 = torch.zeros(H, W, C, dtype=torch.float64, device=DEV)
    if routed:
        _, arg = _pool_ref(_tied_map(H, W, C, prec))
        above = torch.randn(Ho, Wo, C, device=DEV)
        for a, (dy, dx) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
            ab64[dy:2 * Ho:2, dx:2 * Wo:2] = torch.where(arg == a, above.double(), torch.zeros_like(above, dtype=torch.float64))
    elif mode.startswith("above"):
        above = torch.randn(H, W, C, device=DEV)
        ab64 = above.double()
    if mode.endswith("gcap"):
        gcap = torch.randn(H, W, C, device=DEV)
    S = 1.0 if gscale is None else gscale
    gs = None if gscale is None else torch.tensor([gscale, 1.0 / gscale], device=DEV)
    full, gpre = guarded(H * W, C, odt(prec))
    call("prx_k_vgg_combine", above, arg, gcap, act, full, H, W, C, gs, prec, stream())
    sync()
    gc64 = gcap.double() * S if gcap is not None else torch.zeros_like(ab64)
    live = act.double() > 0
    ref = torch.where(live, ab64 + gc64, torch.zeros_like(ab64)).reshape(H * W, C)
    A = torch.where(live, ab64.abs() + gc64.abs(), torch.zeros_like(ab64)).reshape(H * W, C)
    check_op(gpre, ref, prec, 2, A)                  # k = 2: S * gcap, the addition
    if routed and (H % 2 or W % 2):
        assert bool((ab64[2 * Ho:] == 0).all()) and bool((ab64[:, 2 * Wo:] == 0).all())       # outside every window: no routed gradient
    assert untouched(full, H * W, C)


@prec_all
def test_vgg_input_and_input_grad(prec):
    """[3][HW] fp32 -> NHWC with 8 channels (5 zeros) in the operand format (R1); and the first three channels back, times 1 / S"""
    torch.manual_seed(9)
    HW = 301
    x = torch.randn(3, HW, device=DEV) * 4
    x[1, 7] = 1e6
    full, out = guarded(HW, 8, odt(prec))
    call("prx_k_vgg_input", x, full, HW, prec, stream())
    ref = torch.zeros(HW, 8, device=DEV)
    ref[:, :3] = x.t()
    d = torch.randn(HW, 8, device=DEV)
    outs = []
    for u in (None, 2.0 ** -6):
        gfull, gx = guarded(3, HW, torch.float32)
        call("prx_k_vgg_input_grad", d, gfull, HW, None if u is None else torch.tensor([u], device=DEV), stream())
        outs.append((u, gfull, gx))
    sync()
    same_bits(out, cvt(ref, prec))
    assert untouched(full, HW, 8)
    for u, gfull, gx in outs:
        r = d[:, :3].t().double() * (1.0 if u is None else u)
        check_f32(gx, r, 1, r.abs())                 # k = 1: the multiplication by 1 / S
        assert untouched(gfull, 3, HW)


# ================================================================================================ l2norm, sqnorm_rows (R3)
def _norm_rows(n, D):
    torch.manual_seed(n * 7 + D)
    e = torch.randn(n, D, device=DEV)
    e[n // 2] *= 2.0 ** 10                 # one row 2^10 times larger than the others
    return e


def _gate(ref32, ref64):
    return min(4 * rel_l2(ref32, ref64), 1e-5)


def _l2norm_bwd_expr(e, g):
    eh = e / e.norm(dim=1, keepdim=True)
    return (g - eh * (eh * g).sum(dim=1, keepdim=True)) / e.norm(dim=1, keepdim=True)


@pytest.mark.parametrize("D", [1, 512, 640, 1024])
@pytest.mark.parametrize("n", [1, 3, 5])
def test_l2norm_and_sqnorm_rows(n, D):
    """one wave per row, four rows per workgroup: n = 1, 3, 5 leave a ragged last workgroup.  D = 1 is the smallest row the kernels
    take; there nothing is reduced -- every output is a short chain on one element, torch's own fp32 result is exact (gate 0) and
    the backward's float64 reference is identically zero (a relative gate is undefined) -- so the counted rule R2 applies instead."""
    e = _norm_rows(n, D)
    g = torch.randn(n, D, device=DEV)
    e64, g64 = e.double(), g.double()
    ofull, out = guarded(n, D, torch.float32)
    bfull, de = guarded(n, D, torch.float32)
    sfull, sq = flat(n, torch.float32)
    call("prx_k_l2norm_fwd", e, ofull, n, D, stream())
    call("prx_k_l2norm_bwd", e, g, bfull, n, D, stream())
    call("prx_k_sqnorm_rows", e, sfull, n, D, stream())
    sync()
    assert untouched(ofull, n, D) and untouched(bfull, n, D) and untouched(sfull, 1, n)
    ref = e64 / e64.norm(dim=1, keepdim=True)
    refb = _l2norm_bwd_expr(e64, g64)
    fig = {}
    if D == 1:
        check_f32(out, ref, 4, ref.abs())                          # k = 4: v * v, the root, the reciprocal, the product
        check_f32(sq, (e64 * e64).sum(dim=1), 1, (e64 * e64).sum(dim=1))       # k = 1: v * v
        # k = 7: v * v, v * g, v * dot, / ss, the subtraction, 1 / sqrt (2: the root, the reciprocal) -- and the product with inv
        # scales both sides.  A = (|g| + |v dot / ss|) / |e| = 2 |g| / |e|
        check_f32(de, refb, 7, 2 * g64.abs() / e64.abs())
    else:
        fig = {"fwd": (rel_l2(out, ref), _gate(e / e.norm(dim=1, keepdim=True), ref)),
               "sq": (rel_l2(sq, (e64 * e64).sum(dim=1)), _gate((e * e).sum(dim=1), (e64 * e64).sum(dim=1))),
               "bwd": (rel_l2(de, refb), _gate(_l2norm_bwd_expr(e, g), refb))}
    print(n, D, fig)
    for name, (err, gate) in fig.items():
        assert err <= gate, (name, err, gate)


# ================================================================================================ ViT / text embedding kernels
def test_vit_add_cls_pos_and_embed_tokens():
    """x[n][t] += pos[t] (+ cls at t = 0) in place; and the ln_pre-free family's tokens: cls + pos[0] | x + pos[t], fp32 or half out"""
    torch.manual_seed(4)
    N, T, W = 2, 5, 24
    x = torch.randn(N, T, W, device=DEV)
    cls, pos = torch.randn(W, device=DEV), torch.randn(T, W, device=DEV)
    x64, c64, p64 = x.double(), cls.double(), pos.double()
    xfull, xw = guarded(N * T, W, torch.float32)
    xw.copy_(x.reshape(N * T, W))
    call("prx_k_vit_add_cls_pos", xfull, cls, pos, N, T, W, stream())
    ffull, o32 = guarded(N * T, W, torch.float32)
    hfull, o16 = guarded(N * T, W, torch.float16)
    call("prx_k_vit_embed_tokens", x, cls, pos, ffull, 0, N, T, W, stream())
    call("prx_k_vit_embed_tokens", x, cls, pos, hfull, 1, N, T, W, stream())
    sync()
    first = torch.zeros(1, T, 1, dtype=torch.float64, device=DEV)
    first[0, 0, 0] = 1.0
    ref = x64 + p64 + first * c64
    check_f32(xw.reshape(N, T, W), ref, 2, x64.abs() + p64.abs() + first * c64.abs())                # k = 2: two additions
    ref = torch.where(first.bool(), c64 + p64, x64 + p64)
    A = torch.where(first.bool(), c64.abs() + p64.abs(), x64.abs() + p64.abs())
    check_f32(o32.reshape(N, T, W), ref, 1, A)                                                     # k = 1: one addition
    check16(o16.reshape(N, T, W), ref, 1, 1 * EPS32, A)
    assert untouched(xfull, N * T, W) and untouched(ffull, N * T, W) and untouched(hfull, N * T, W)


@pytest.mark.parametrize("blocks", [1, 256])
def test_vit_scale_f32(blocks):
    torch.manual_seed(blocks)
    n = 1031
    x = torch.randn(n, device=DEV)
    full, w = flat(n, torch.float32)
    w.copy_(x)
    call("prx_k_vit_scale_f32", full, n, 0.125 ** 0.5, blocks, stream())
    sync()
    s64 = float(torch.tensor(0.125 ** 0.5, dtype=torch.float32))
    check_f32(w, x.double() * s64, 1, x.double().abs() * s64)            # k = 1: one multiplication
    assert untouched(full, 1, n)


def _gelu64(x):
    return x * 0.5 * (1 + torch.erf(x * 0.5 ** 0.5))


def test_vit_gelu_f32():
    """the exact mode's own GELU pass, |x| <= 6 with 0 and +-0 (R3): out = gelu(t) and io *= gelu'(t)"""
    torch.manual_seed(6)
    n = 4099
    t = (torch.rand(n, device=DEV) * 12 - 6)
    t[0], t[1], t[2], t[3], t[4] = 0.0, -0.0, 6.0, -6.0, 1e-20
    t64 = t.double()
    ffull, fo = flat(n, torch.float32)
    call("prx_k_vit_gelu_f32", t, ffull, n, 0, stream())
    io0 = torch.randn(n, device=DEV)
    bfull, bo = flat(n, torch.float32)
    bo.copy_(io0)
    call("prx_k_vit_gelu_f32", t, bfull, n, 1, stream())
    sync()
    ref = _gelu64(t64)
    t64g = t64.clone().requires_grad_(True)
    (refb,) = torch.autograd.grad(_gelu64(t64g), t64g, io0.double())
    t32g = t.clone().requires_grad_(True)
    (b32,) = torch.autograd.grad(F.gelu(t32g), t32g, io0)
    fig = {"fwd": (rel_l2(fo, ref), _gate(F.gelu(t), ref)), "bwd": (rel_l2(bo, refb), _gate(b32, refb))}
    print(fig)
    assert untouched(ffull, 1, n) and untouched(bfull, 1, n)
    assert float(fo[0]) == 0.0 and float(fo[1]) == 0.0
    for name, (err, gate) in fig.items():
        assert err <= gate, (name, err, gate)


def _first_argmax(tk):
    """first index of the largest token id, written out"""
    res = []
    for row in tk.tolist():
        best, bj = row[0], 0
        for j in range(1, len(row)):
            if row[j] > best:
                best, bj = row[j], j
        res.append(bj)
    return res


def test_text_embed_and_gather_rows():
    """x = emb[token] + pos (a gather and one addition: the correctly rounded fp32 sum, R1) with repeated tokens; eot = the FIRST index
    of the largest id -- the largest id first, last, and tied; gather_rows copies row eot"""
    torch.manual_seed(8)
    n, ctx, W, vocab = 4, 7, 40, 50
    tk = torch.randint(0, 30, (n, ctx), dtype=torch.int32, device=DEV)
    tk[0, 0] = 49                      # first
    tk[1, ctx - 1] = 49                # last
    tk[2, 2] = tk[2, 5] = 49           # tied: index 2
    tk[3, :] = 3                       # all equal: index 0
    tk[0, 1] = tk[0, 2] = 11           # repeated tokens
    emb, pos = torch.randn(vocab, W, device=DEV), torch.randn(ctx, W, device=DEV)
    xfull, x = guarded(n * ctx, W, torch.float32)
    efull = torch.full((n + 3,), -77, dtype=torch.int32, device=DEV)
    call("prx_k_text_embed", tk, emb, pos, xfull, efull, n, ctx, W, vocab, stream())
    sync()
    ref = (emb.double()[tk.long()] + pos.double()).float()
    same_bits(x, ref.reshape(n * ctx, W))
    want = _first_argmax(tk)
    assert want == [0, ctx - 1, 2, 0] and efull[:n].tolist() == want and efull[n:].tolist() == [-77] * 3
    assert untouched(xfull, n * ctx, W)
    ofull, out = guarded(n, W, torch.float32)
    call("prx_k_gather_rows", x, efull, ofull, n, ctx, W, stream())
    sync()
    same_bits(out, torch.stack([ref[i, want[i]] for i in range(n)]))
    assert untouched(ofull, n, W)


# ================================================================================================ the tower boundary (csrc/runner_core.h)
def tower_handle(model, max_batch, precision, dev=None):
    """(handle, cutout side) of a reduced tower of every kind behind clip_encode_image"""
    from pixray_amd import ops, weights as W
    dev = torch.device(dev or DEV)
    if model in W.CLIP_CONFIGS:
        cfg = W.CLIP_CONFIGS[model]
        h = ops.ClipVitHandle(cfg, W.synthetic_clip_vit_params(cfg, 0), max_batch, dev, precision)
    elif model in W.SLIP_CONFIGS:
        cfg = W.SLIP_CONFIGS[model]
        h = ops.SlipVitHandle(cfg, W.synthetic_slip_vit_params(cfg, 0), max_batch, dev, precision)
    elif model in W.OPENCLIP_CONFIGS:
        cfg = W.OPENCLIP_CONFIGS[model]
        h = ops.OpenClipVitHandle(cfg, W.synthetic_clip_vit_params(cfg, 0), max_batch, dev, precision)
    elif model in W.CLIP_RESNET_CONFIGS:
        cfg = W.CLIP_RESNET_CONFIGS[model]
        h = ops.ClipResNetHandle(cfg, W.synthetic_clip_resnet_params(cfg, 0), max_batch, dev, precision)
    else:
        cfg = W.CLIP_CONVNEXT_CONFIGS[model]
        h = ops.ClipConvNextHandle(cfg, W.synthetic_clip_convnext_params(cfg, 0), max_batch, dev, precision)
    return h, cfg.input_resolution


def shared_handle_case(model, precision):
    """A handle made for two cutouts runs two, then one; a fresh handle made for one runs the same one.  Embeddings and cutout gradient
    of the two one-cutout runs must agree bit for bit: nothing of a tower may depend on the capacity of its handle (buffer strides,
    the batch the backward differentiates, what the larger batch left behind in the activations)."""
    from pixray_amd import ops
    big, R = tower_handle(model, 2, precision)
    one, _ = tower_handle(model, 1, precision)
    gen = torch.Generator().manual_seed(11)
    cut = torch.rand(2, 3, R, R, generator=gen).to(DEV)
    g = (torch.randn(2, big.cfg.output_dim, generator=gen) * 1e-3).to(DEV)

    def run(h, c, gg):
        c = c.clone().requires_grad_(True)
        e = ops.clip_encode_image(c, h)
        e.backward(gg)
        sync()
        return e.detach(), c.grad

    e_two, g_two = run(big, cut, g)
    e_big, g_big = run(big, cut[1:], g[1:])
    e_one, g_one = run(one, cut[1:], g[1:])
    for t in (e_two, g_two, e_big, g_big):
        assert bool(torch.isfinite(t).all())
    assert float(g_big.abs().max()) > 0
    same_bits(e_big, e_one)
    same_bits(g_big, g_one)


@pytest.mark.parametrize("precision", ["fp16", "bf16", "f32"])
@pytest.mark.parametrize("model", ["tiny-B/32", "tiny-RN", "tiny-cnx-d"])
def test_tower_results_do_not_depend_on_the_handle_capacity(model, precision):
    shared_handle_case(model, precision)


# ================================================================================================ a CPU-sized subset (tests/test_emu_cpu.py)
def emu_subset(lib=None):
    """one small case per kernel on the emulated kernels (DEV = "cpu").  With the emulator's library handle: the renormalisation sums
    once more under the reversed workgroup order -- they end in cross-workgroup atomic additions of doubles and must not change
    by a bit (the gradients are claimed bit-reproducible)."""
    for prec in PRECS:
        test_rn_pack_conv3x3(5, 3, prec)
        test_vgg_pack(5, 3, 8, prec)
        test_vqgan_pack_conv3x3(3, 8, 8, prec)
        test_pack_conv3x3(5, 3, 8, 8, "fd", prec)
        test_pack_transpose(33, 70, prec)
        for CO in STEM_CO:
            stem_fwd_case(5, 18, CO, prec)
            stem_bwd_case(5, 18, CO, prec, 2.0 ** -5)
        stem_fwd_case(1, 2, 40, prec)
        stem_fwd_case(2, 6, 8, prec, constant=True)
        stem_bwd_case(1, 2, 40, prec, None)
        test_avgpool2_fwd(2, 6, 10, 4, prec)
        for outs in ("op", "f32", "both"):
            test_avgpool2_bwd(2, 6, 10, 4, True, outs, prec)
        test_avgpool2_bwd(1, 2, 2, 40, False, "both", prec)
        test_relu_mask(prec)
        test_tokens_fwd(3, 9, 24, prec)
        test_tokens_bwd(3, 9, 24, prec)
        test_tok0_gather_and_scatter(prec)
        test_patchify_fwd(32, 16, "clip", prec)
        test_patchify_fwd(28, 14, "imagenet", prec)
        test_vgg_maxpool(7, 9, 8, prec)
        for mode in ("none", "gcap", "above", "above+gcap", "routed", "routed+gcap"):
            test_vgg_combine(7, 9, 8, mode, 2.0 ** 6, prec)
        test_vgg_combine(4, 4, 64, "routed+gcap", None, prec)
        test_vgg_input_and_input_grad(prec)
    test_stem_refuses_a_width_it_has_no_kernel_for()
    test_pack_conv3x3_refuses_no_pack_and_a_padded_size_below_the_channels()
    test_vqgan_enc_pack_conv3x3(5, 3, 8)
    test_colminmax(5, 300)
    for n in (1, 7, 4099):
        for offset in (0, 1):
            test_minmax(n, 64, offset)
    for S, P in PATCH_SHAPES:
        patchify_bwd_case(S, P, "imagenet" if P == 4 else "clip")
    test_patchify_bwd_constant_cutouts()
    test_preproc_bwd_reduce_and_apply(False)
    test_preproc_bwd_reduce_and_apply(True)
    for n, D in [(1, 1), (5, 1), (3, 512), (5, 640), (1, 1024)]:
        test_l2norm_and_sqnorm_rows(n, D)
    test_vit_add_cls_pos_and_embed_tokens()
    test_vit_scale_f32(1)
    test_vit_scale_f32(256)
    test_vit_gelu_f32()
    test_text_embed_and_gather_rows()
    if lib is not None:
        a = patchify_bwd_case(32, 16, "clip", N=5)          # 15360 elements: 60 workgroups
        lib.hipemu_set_reverse_order(1)
        try:
            b = patchify_bwd_case(32, 16, "clip", N=5)
        finally:
            lib.hipemu_set_reverse_order(0)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)), ("the renormalisation sums depend on the workgroup order", a.tolist(), b.tolist())
