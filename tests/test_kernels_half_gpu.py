"""Kernel-level parity tests (GPU) of the variants the product's default runs: IEEE-half operands (`h16 = 1`) and the lean layout
(`s16`: residual streams, feature maps and their gradients in 16 bits only), next to their bf16 / fp32-stream twins, through the
`prx_k_*_op` entry points that forward every argument of the internal functions (csrc/api_kernels.hip).

Every test rounds its inputs to the format the kernel consumes, evaluates a plain torch expression of the operation in FLOAT64 on
those rounded inputs, and compares.  Output buffers are pre-filled with NaN and carry spare rows / columns behind the leading
dimension, which must come back untouched.  Where the tolerances come from (none is tuned against a kernel's output):

* data movement and conversions: bit equality with torch's round-to-nearest-even conversion (after clamp(+-65504) for half);
* short fp32 chains rounded once to 16 bits: |out - ref64| <= ulp16(ref64) + k * 2^-24 * A, A = sum of the absolute values of the
  terms of the float64 expression at that element, k = the fp32 roundings of the kernel's chain, counted beside each use;
* fp32 quantities behind a reduction: rel-L2 gate = 4 x the rel-L2 error of torch's own fp32 evaluation of the same op against
  the float64 reference (computed here, reference against reference), never above the fp32 gates of test_kernels_gpu.py
  (1e-5, GroupNorm backward 2e-5); the swish / softmax paths add the error of the fast `__expf` (derived at `EXPF_REL`);
  the 16-bit outputs of those kernels: the elementwise bound above with that gate added to k * 2^-24;
* attention: the project's bf16 gates; the half instantiation's gates are 2 x the largest error measured over this file's
  parametrisation on an MI355X, and never looser than the bf16 gate of the same check (figures beside the asserts)."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from pixray_amd import _lib
from pixray_amd._lib import PrxError, call

DEV = "cuda"
EPS32 = 2.0 ** -24          # unit round-off of fp32
NAN = float("nan")
F16_MAX = 65504.0


def stream():
    return _lib.current_stream()


def sync():
    torch.cuda.synchronize()


def fmt(h16):
    return torch.float16 if h16 else torch.bfloat16


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-300)).item()


def ulp16(ref, h16):
    """spacing of the 16-bit format at |ref| (the subnormal spacing below the smallest normal number); half saturates at 65504"""
    pbits, emin = (10, -14) if h16 else (7, -126)
    a = ref.double().abs()
    if h16:
        a = a.clamp(max=F16_MAX)
    e = torch.frexp(a.clamp_min(2.0 ** -140))[1] - 1           # floor(log2 |ref|)
    return torch.ldexp(torch.ones_like(a), e.clamp_min(emin) - pbits)


def to16(x, h16):
    """torch's round-to-nearest-even conversion; the half path saturates instead of overflowing (common.h f32_to_f16_sat)"""
    return x.clamp(-F16_MAX, F16_MAX).to(torch.float16) if h16 else x.to(torch.bfloat16)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def guarded(rows, cols, dtype, ld=None, spare_rows=3):
    """a NaN-filled [rows + spare_rows][ld] buffer and its [rows][cols] window"""
    ld = cols if ld is None else ld
    full = torch.full((rows + spare_rows, ld), NAN, dtype=dtype, device=DEV)
    return full, full[:rows, :cols]


def untouched(full, rows, cols):
    """everything outside the window is still NaN"""
    return bool(torch.isnan(full[rows:]).all()) and bool(torch.isnan(full[:rows, cols:]).all())


def within(out, ref, tol):
    """elementwise |out - ref| <= tol; NaN anywhere fails"""
    err = (out.double() - ref.double()).abs()
    ok = err <= tol
    if not bool(ok.all()):
        i = int((err - tol).nan_to_num(nan=float("inf")).argmax())
        return False, (i, float(err.flatten()[i]), float(tol.flatten()[i]), float(ref.flatten()[i]))
    return True, None


def check16(out16, ref64, h16, k_rel, A):
    """the 16-bit rule: |out - ref64| <= ulp16(ref64) + k_rel * A"""
    r = ref64.clamp(-F16_MAX, F16_MAX) if h16 else ref64
    ok, worst = within(out16, r, ulp16(r, h16) + k_rel * A)
    assert ok, ("16-bit output off by more than one ulp + fp32 chain", worst)


# `__expf(x)` is exp2(x * log2(e)): the argument scaling rounds x * log2(e) to fp32, a relative error of |x| * log2(e) * ln(2) * 2^-24
# = |x| * 2^-24 in the result, plus two units for the multiplication and the hardware exp2 (1 ulp)
def EXPF_REL(xmax):
    return (xmax + 2.0) * EPS32


def swish64(y):
    return y * torch.sigmoid(y)


# ================================================================================================ GroupNorm
def _gn_ref(x64, gamma, beta, swish):
    y = F.group_norm(x64.permute(0, 2, 1), 32, gamma, beta, eps=1e-6).permute(0, 2, 1)
    return y, (swish64(y) if swish else y)


def _gn_terms(x64, gamma, beta, C):
    """per-group mean / rstd of the float64 reference, broadcast to [NB][P][C]"""
    NB, P, _ = x64.shape
    xg = x64.reshape(NB, P, 32, C // 32)
    m = xg.mean(dim=(1, 3), keepdim=True)
    var = xg.var(dim=(1, 3), keepdim=True, unbiased=False)
    rstd = (var + 1e-6).rsqrt()
    return m.expand_as(xg).reshape(NB, P, C), rstd.expand_as(xg).reshape(NB, P, C)


def groupnorm_case(NB, P, C, swish, with_add, s16, h16, *, stats_ready=0, fp32_out=True, mean=0.3, sigma=1.5, seed=0):
    """forward and backward of one shape.  Returns the measured figures (for the docstrings / the description)."""
    torch.manual_seed(1000 * seed + P + C + NB)
    sdt = fmt(h16) if s16 else torch.float32                                 # element type of the streams x, g, add
    x = (torch.randn(NB, P, C, device=DEV) * sigma + mean).to(sdt)
    gamma = torch.randn(C, device=DEV) * 0.2 + 1.0
    beta = torch.randn(C, device=DEV) * 0.1
    x64 = x.double().requires_grad_(True)
    ga64, be64 = gamma.double(), beta.double()
    y64, ref = _gn_ref(x64, ga64, be64, swish)
    m64, r64 = _gn_terms(x64.detach(), ga64, be64, C)
    # the yardstick of the reduction: torch's fp32 evaluation of the same op on the same inputs
    y32, ref32 = _gn_ref(x.float().requires_grad_(True), gamma, beta, swish)
    ymax = float(y64.detach().abs().max())
    intr = EXPF_REL(ymax) if swish else 0.0
    gate_f = min(4 * rel_l2(ref32, ref) + intr, 1e-5)

    stats = torch.full((NB * 64 + 8,), NAN, dtype=torch.float64, device=DEV)
    if stats_ready:                                                           # exact float64 sums: what a producing GEMM's epilogue supplies
        xg = x64.detach().reshape(NB, P, 32, C // 32)
        stats[:NB * 64] = torch.stack([xg.sum(dim=(1, 3)), (xg * xg).sum(dim=(1, 3))], dim=-1).reshape(-1)
    rows = NB * P
    o16_full, o16 = guarded(rows, C, fmt(h16))
    o32_full, o32 = guarded(rows, C, torch.float32) if fp32_out else (None, None)
    call("prx_k_groupnorm_fwd_op", x, gamma, beta, stats, o16_full, o32_full, NB, P, C, swish, 1e-6, 0 if stats_ready else 1, stats_ready,
         h16, s16, stream())
    sync()
    refd = ref.detach().reshape(rows, C)
    # A: y = (x - m) * rstd * gamma + beta; the swish multiplies by at most 1.1 (max of d/dy y sigmoid(y)) and adds its own result
    A = ((x64.detach().abs() + m64.abs()) * r64 * ga64.abs() + be64.abs()).reshape(rows, C)
    if swish:
        A = 1.1 * A + refd.abs()
    k_fwd = (4 + (4 if swish else 0)) * EPS32 + intr                           # sub, mul, mul, add (+ exp scale, add, div, mul)
    fig = {}
    assert untouched(o16_full, rows, C) and bool(torch.isnan(stats[NB * 64:]).all())
    if fp32_out:
        assert untouched(o32_full, rows, C)
        fig["fwd_f32"] = rel_l2(o32, refd)
        assert fig["fwd_f32"] <= gate_f, (fig, gate_f)
        assert torch.equal(bits(o16), bits(to16(o32, h16))), "the 16-bit twin is not the rounded fp32 output"
    check16(o16, refd, h16, k_fwd + gate_f, A)
    if not stats_ready:                                                         # the sums themselves, against float64
        xg = x64.detach().reshape(NB, P, 32, C // 32)
        s64 = torch.stack([xg.sum(dim=(1, 3)), (xg * xg).sum(dim=(1, 3))], dim=-1).reshape(-1)
        a64 = torch.stack([xg.abs().sum(dim=(1, 3)), (xg * xg).sum(dim=(1, 3))], dim=-1).reshape(-1)
        # a thread owns every (blocks * ppb)-th pixel: it adds that many quads (4 additions and a squaring each) in fp32, everything
        # behind it is float64 -- depth * 2^-24 * sum |terms|
        ppb = 1024 // C
        blocks = min((P + 4 * ppb - 1) // (4 * ppb), 256)
        depth = 5 * (P // (blocks * ppb) + 1)
        ok, worst = within(stats[:NB * 64], s64, depth * EPS32 * a64)
        assert ok, ("forward sums", worst)

    # ---- backward
    g = torch.randn(NB, P, C, device=DEV).to(sdt)
    add = torch.randn(NB, P, C, device=DEV).to(sdt) if with_add else None
    g64 = g.double()
    (gx,) = torch.autograd.grad(ref, x64, g64)
    refb = gx + (add.double() if with_add else 0.0)
    x32 = x.float().requires_grad_(True)
    (gx32,) = torch.autograd.grad(_gn_ref(x32, gamma, beta, swish)[1], x32, g.float())
    intr_b = 2 * intr                                                         # sigmoid enters swish_grad twice
    gate_b = min(4 * rel_l2(gx32, gx) + intr_b, 2e-5)
    fstats = stats[:NB * 64].clone()
    xh = (x64.detach() - m64) * r64
    yb = xh * ga64 + be64
    sg = torch.sigmoid(yb)
    dxh = g64 * ga64 * ((sg * (1 + yb * (1 - sg))) if swish else 1.0)
    dg = dxh.reshape(NB, P, 32, C // 32)
    m1 = dg.mean(dim=(1, 3), keepdim=True).expand_as(dg).reshape(NB, P, C)
    m2 = (dg * xh.reshape(NB, P, 32, C // 32)).mean(dim=(1, 3), keepdim=True).expand_as(dg).reshape(NB, P, C)
    # the float64 expression written out once more must be the autograd result (a check of this test's own algebra)
    assert rel_l2(r64 * (dxh - m1 - xh * m2), gx) < 1e-10
    # |dxhat|'s own terms: swish'(y) = s + y s (1 - s) is a sum of two terms of opposite sign for y < 0 (it crosses zero at
    # y = -1.28), and the fp32 round-off of y = xhat gamma + beta reaches it through |swish''| <= 0.5
    adxh = (g64 * ga64).abs() * ((sg + yb.abs() * sg * (1 - sg) + 0.5 * ((xh * ga64).abs() + be64.abs())) if swish else 1.0)
    Ab = (r64 * (adxh + m1.abs() + (xh * m2).abs()) + (add.double().abs() if with_add else 0.0)).reshape(rows, C)
    # xhat (2), y (2), swish_grad (exp scale, add, div, sub, mul, add, mul = 7), g * (.) * gamma (2), sub, mul, sub, mul, add (5)
    k_bwd = ((18 if swish else 9)) * EPS32 + intr_b
    bstats = torch.full((NB * 64 + 8,), NAN, dtype=torch.float64, device=DEV)
    if stats_ready:
        bstats[:NB * 64] = torch.stack([dg.sum(dim=(1, 3)), (dg * xh.reshape(NB, P, 32, C // 32)).sum(dim=(1, 3))], dim=-1).reshape(-1)
    d16_full, d16 = guarded(rows, C, fmt(h16))
    d32_full, d32 = guarded(rows, C, torch.float32) if fp32_out else (None, None)
    call("prx_k_groupnorm_bwd_op", g, x, gamma, beta, fstats, bstats, add, d32_full, d16_full, NB, P, C, swish, 1e-6,
         0 if stats_ready else 1, stats_ready, h16, s16, stream())
    sync()
    refb = refb.reshape(rows, C)
    assert untouched(d16_full, rows, C) and bool(torch.isnan(bstats[NB * 64:]).all())
    if fp32_out:
        assert untouched(d32_full, rows, C)
        fig["bwd_f32"] = rel_l2(d32 - (add.float().reshape(rows, C) if with_add else 0.0), gx.reshape(rows, C))
        assert rel_l2(d32, refb) <= gate_b, (rel_l2(d32, refb), gate_b)
        assert torch.equal(bits(d16), bits(to16(d32, h16))), "the 16-bit twin is not the rounded fp32 gradient"
    check16(d16, refb, h16, k_bwd + gate_b, Ab)
    fig["gates"] = (gate_f, gate_b)
    return fig


# (NB, P, C, swish, add): P below one block step (1, 3), odd P for the 4-way unrolled statistics loop and its tail (3, 255), non-square
# decoder maps (12 x 20, 15 x 17), every C the PRX_REQUIRE admits.  NB > 1: (3, 255, 512) makes 255 * 128 = 32640 quads per
# image = 127.5 workgroup slices of 256, so a slice and a thread's second element cross into the next image; (3, 4096, 512) has
# slices of 768 quads against 524288 per image (682.67 slices): a thread's stride crosses the boundary inside its loop; (3, 700, 1024)
# is the smallest such case (537600 quads > 2048 workgroups x 256: slices of 263, the first 7 threads of a slice take a second quad
# 256 further on, 179200 quads per image = 681.37 slices) -- the one the CPU emulation runs
GN_SHAPES = [(1, 1, 128, 1, True), (2, 1, 1024, 0, False), (1, 3, 1024, 1, True), (3, 3, 512, 0, True), (2, 240, 256, 1, True),
             (3, 240, 1024, 1, False), (1, 255, 128, 0, True), (3, 255, 512, 1, True), (2, 255, 256, 1, False), (1, 4096, 128, 1, True),
             (2, 4096, 256, 0, True), (3, 4096, 512, 1, True), (1, 4096, 1024, 1, False), (1, 65536, 128, 1, True), (3, 700, 1024, 1, True)]


@pytest.mark.parametrize("s16,h16", [(0, 0), (0, 1), (1, 0), (1, 1)], ids=["f32stream-bf16", "f32stream-half", "lean-bf16", "lean-half"])
@pytest.mark.parametrize("NB,P,C,swish,with_add", GN_SHAPES)
def test_groupnorm_variants(NB, P, C, swish, with_add, s16, h16):
    """gn_stats_kernel<0/1, S16>, gn_apply_fwd/bwd_kernel<S16>, both 16-bit formats, fp32 + 16-bit outputs"""
    print(groupnorm_case(NB, P, C, swish, with_add, s16, h16))


@pytest.mark.parametrize("s16,h16", [(0, 0), (1, 1)], ids=["f32stream-bf16", "lean-half"])
@pytest.mark.parametrize("NB,P,C,swish,with_add", [(2, 255, 256, 1, True), (3, 240, 512, 1, False), (1, 4096, 128, 0, True), (2, 3, 1024, 1, True)])
def test_groupnorm_16bit_output_only(NB, P, C, swish, with_add, s16, h16):
    """dx == nullptr / out_f32 == nullptr: what the lean layout launches"""
    print(groupnorm_case(NB, P, C, swish, with_add, s16, h16, fp32_out=False, seed=1))


@pytest.mark.parametrize("s16,h16", [(0, 0), (1, 1)], ids=["f32stream-bf16", "lean-half"])
@pytest.mark.parametrize("NB,P,C,swish,with_add", [(2, 255, 256, 1, True), (3, 3, 128, 0, False), (1, 4096, 512, 1, True)])
def test_groupnorm_stats_supplied_by_the_caller(NB, P, C, swish, with_add, s16, h16):
    """stats_ready = 1, zero_stats = 0: float64 sums as a producing GEMM's epilogue leaves them; the statistics pass must not run
    (the NaN behind the sums stays, the sums are not accumulated a second time)"""
    print(groupnorm_case(NB, P, C, swish, with_add, s16, h16, stats_ready=1, seed=2))


@pytest.mark.parametrize("s16,h16", [(0, 0), (0, 1)], ids=["f32stream-bf16", "f32stream-half"])
def test_groupnorm_group_mean_far_from_zero(s16, h16):
    """the statistics are sum x, sum x^2 in fp32 per thread and var = E[x^2] - m^2: a per-group mean 32 standard deviations from zero.
    The ratio 32 is the largest power of two at which torch's own fp32 F.group_norm on the CPU keeps 4 x room under the 1e-5
    ceiling (its rel-L2 error against float64 at [2][240][256]: 2.4e-7, 4.9e-7, 9.1e-7, 2.1e-6, 3.8e-6 at ratios 4, 8, 16, 32, 64),
    which is asserted here.  fp32 streams: a 16-bit stream cannot hold such a tensor (its rounding alone is sigma / 8 at half).


    Found by this test (backward without swish, [2][240][256] and [3][255][512]: rel-L2 3.1e-6 on the MI355X against a gate of
    5.8e-7): gn_stats_kernel<0> rounded every x^2 and its running sums to fp32, so rstd carried mean^2 / var = 1024 units of fp32
    round-off.  Threads whose values lie far from zero now hand on float64 sums (csrc/norms.hip); measured after: 7.5e-8 on the CPU emulation."""
    torch.manual_seed(0)
    x = torch.randn(2, 240, 256) + 32.0
    ga, be = torch.randn(256) * 0.2 + 1.0, torch.randn(256) * 0.1
    e_cpu = rel_l2(_gn_ref(x, ga, be, 0)[1], _gn_ref(x.double(), ga.double(), be.double(), 0)[1])
    assert e_cpu <= 1e-5 / 4, e_cpu
    for shape in [(2, 240, 256, 0, True), (1, 4096, 128, 1, True), (3, 255, 512, 0, False)]:
        print(groupnorm_case(*shape, s16, h16, mean=32.0, sigma=1.0, seed=3))


@pytest.mark.parametrize("C", [64, 96])
def test_groupnorm_refuses_channel_counts_it_cannot_tile(C):
    x = torch.randn(1, 16, C, device=DEV)
    ga, be = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    stats = torch.zeros(64, dtype=torch.float64, device=DEV)
    o16_full, _ = guarded(16, C, torch.float16)
    with pytest.raises(PrxError, match="unsupported C"):
        call("prx_k_groupnorm_fwd_op", x, ga, be, stats, o16_full, None, 1, 16, C, 0, 1e-6, 1, 0, 1, 0, stream())
    with pytest.raises(PrxError, match="unsupported C"):
        call("prx_k_groupnorm_bwd_op", x, x, ga, be, stats, stats.clone(), None, None, o16_full, 1, 16, C, 0, 1e-6, 1, 0, 1, 0, stream())
    sync()
    assert bool(torch.isnan(o16_full).all())


# ================================================================================================ LayerNorm
def layernorm_case(rows, C, h16, s16, add_every=0, fp32_out=True, with_add=True, seed=0):
    """forward (x a 16-bit stream when s16 & 1) and backward (s16 bits: 1 = x, 2 = g, 4 = add) of one shape; x and g are the middle
    column blocks of [rows][3C] matrices, every other leading dimension differs from C too"""
    torch.manual_seed(77 * seed + rows + C)
    f16 = fmt(h16)
    xdt = f16 if s16 & 1 else torch.float32
    gdt = f16 if s16 & 2 else torch.float32
    adt = f16 if s16 & 4 else torch.float32
    X = (torch.randn(rows + 1, 3 * C, device=DEV) * 2 + 0.5).to(xdt)
    x = X[:rows, C:2 * C]
    gamma = torch.randn(C, device=DEV) * 0.2 + 1.0
    beta = torch.randn(C, device=DEV) * 0.1
    x64 = x.double().requires_grad_(True)
    ga64, be64 = gamma.double(), beta.double()
    ref = F.layer_norm(x64, (C,), ga64, be64, eps=1e-5)
    x32 = x.float().requires_grad_(True)
    ref32 = F.layer_norm(x32, (C,), gamma, beta, eps=1e-5)
    gate_f = min(4 * rel_l2(ref32, ref), 1e-5)
    m64 = x64.detach().mean(dim=1, keepdim=True)
    r64 = (x64.detach().var(dim=1, keepdim=True, unbiased=False) + 1e-5).rsqrt()
    o16_full, o16 = guarded(rows, C, f16)
    o32_full, o32 = guarded(rows, C, torch.float32) if fp32_out else (None, None)
    mean = torch.full((rows + 3,), NAN, device=DEV)
    rstd = torch.full((rows + 3,), NAN, device=DEV)
    call("prx_k_layernorm_fwd_op", x, 3 * C, gamma, beta, o16_full, o32_full, mean, rstd, rows, C, 1e-5, h16, s16 & 1, stream())
    sync()
    refd = ref.detach()
    A = (x64.detach().abs() + m64.abs()) * r64 * ga64.abs() + be64.abs()
    k_fwd = 4 * EPS32                                                         # sub, mul, mul, add
    assert untouched(o16_full, rows, C) and bool(torch.isnan(mean[rows:]).all()) and bool(torch.isnan(rstd[rows:]).all())
    fig = {}
    if fp32_out:
        assert untouched(o32_full, rows, C)
        fig["fwd_f32"] = rel_l2(o32, refd)
        assert fig["fwd_f32"] <= gate_f, (fig, gate_f)
        assert torch.equal(bits(o16), bits(to16(o32, h16)))
    check16(o16, refd, h16, k_fwd + gate_f, A)
    # mean: C fp32 additions (4 per lane step, 6 shuffle levels) and one division; rstd: the same for the variance, rsqrt (1 ulp)
    depth = (C // 64 + 6 + 2) * EPS32
    ok, worst = within(mean[:rows], m64[:, 0], depth * x64.detach().abs().mean(dim=1) + EPS32 * m64[:, 0].abs())
    assert ok, ("mean", worst)
    ok, worst = within(rstd[:rows], r64[:, 0], (2 * depth + 4 * EPS32) * r64[:, 0])
    assert ok, ("rstd", worst)

    # ---- backward; mean / rstd come from the float64 reference (rounded to fp32), not from the kernel under test
    mean_in, rstd_in = m64[:, 0].float().contiguous(), r64[:, 0].float().contiguous()
    G = torch.randn(rows + 1, 3 * C, device=DEV).to(gdt)
    g = G[:rows, C:2 * C]
    ldadd, lddx, lddxb = C + 8, C + 4, C + 16
    addf = torch.randn(rows + 1, ldadd, device=DEV).to(adt)
    sel = torch.ones(rows, dtype=torch.bool, device=DEV)
    if add_every:
        sel = (torch.arange(rows, device=DEV) % add_every) == 0
        addf[:rows][~sel] = NAN                                               # proves the other rows are never read
    add64 = torch.where(sel[:, None], addf[:rows, :C].double(), torch.zeros((), dtype=torch.float64, device=DEV))
    if not with_add:
        addf, add64 = None, torch.zeros_like(add64)
    g64 = g.double()
    (gx,) = torch.autograd.grad(ref, x64, g64)
    (gx32,) = torch.autograd.grad(ref32, x32, g.float())
    gate_b = min(4 * rel_l2(gx32, gx), 1e-5)
    refb = gx + add64
    xh = (x64.detach() - m64) * r64
    dxh = g64 * ga64
    m1, m2 = dxh.mean(dim=1, keepdim=True), (dxh * xh).mean(dim=1, keepdim=True)
    assert rel_l2(r64 * (dxh - m1 - xh * m2), gx) < 1e-10
    # the fp32-rounded mean / rstd inputs perturb xhat by 2^-24 (|m| + |x - m|) rstd: inside the |x| + |m| term of Ab
    Ab = r64 * (dxh.abs() + m1.abs() + (xh.abs() + (x64.detach().abs() + m64.abs()) * r64) * m2.abs()) + add64.abs()
    k_bwd = 10 * EPS32                                                        # xhat (2), g * gamma, sub, mul, sub, mul, add, the rounded mean / rstd (2)
    d16_full, d16 = guarded(rows, C, f16, ld=lddxb)
    d32_full, d32 = guarded(rows, C, torch.float32, ld=lddx) if fp32_out else (None, None)
    call("prx_k_layernorm_bwd_op", g, 3 * C, x, 3 * C, gamma, mean_in, rstd_in, addf, ldadd, d32_full, lddx, d16_full, lddxb, rows, C, h16,
         add_every, s16, stream())
    sync()
    assert untouched(d16_full, rows, C)
    if fp32_out:
        assert untouched(d32_full, rows, C)
        fig["bwd_f32"] = rel_l2(d32, refb)
        assert fig["bwd_f32"] <= gate_b, (fig, gate_b)
        assert torch.equal(bits(d16), bits(to16(d32, h16)))
    check16(d16, refb, h16, k_bwd + gate_b, Ab)
    fig["gates"] = (gate_f, gate_b)
    return fig


@pytest.mark.parametrize("h16", [0, 1], ids=["bf16", "half"])
@pytest.mark.parametrize("s16", [0, 1, 2, 7])
@pytest.mark.parametrize("rows,C", [(1, 256), (5, 512), (257, 768), (3200, 768), (257, 1024), (5, 1280), (257, 1280), (1, 2048), (3200, 2048),
                                    (3200, 256), (5, 1024)])
def test_layernorm_variants(rows, C, s16, h16):
    """ln_fwd_kernel<4 / 8, S16>, ln_bwd_kernel<4 / 8, 0 / 1 / 2 / 7> (MAXV = 4 up to C = 1024, 8 beyond), ld != C everywhere"""
    print(layernorm_case(rows, C, h16, s16))


@pytest.mark.parametrize("h16", [0, 1], ids=["bf16", "half"])
@pytest.mark.parametrize("s16", [0, 7])
@pytest.mark.parametrize("n,T,C", [(3, 50, 768), (64, 50, 768), (2, 197, 768), (2, 197, 1280), (1, 50, 256)])
def test_layernorm_bwd_adds_the_class_token_gradient_on_every_Tth_row(n, T, C, s16, h16):
    """add_every = T: `add` enters on rows = 0 (mod T) only and holds NaN on every other row; with and without the fp32 output"""
    print(layernorm_case(n * T, C, h16, s16, add_every=T, seed=1))
    print(layernorm_case(n * T, C, h16, s16, add_every=T, fp32_out=False, seed=2))


@pytest.mark.parametrize("h16", [0, 1], ids=["bf16", "half"])
@pytest.mark.parametrize("rows,C,s16", [(257, 768, 7), (5, 2048, 1), (3200, 1024, 7)])
def test_layernorm_16bit_output_only(rows, C, s16, h16):
    print(layernorm_case(rows, C, h16, s16, fp32_out=False, seed=3))
    print(layernorm_case(rows, C, h16, s16, fp32_out=False, with_add=False, seed=4))


def test_layernorm_refuses_what_it_has_no_kernel_for():
    rows = 4
    for C, s16, msg in [(384, 0, "multiple of 256"), (768, 3, "stream layouts"), (2304, 0, "multiple of 256")]:
        x = torch.randn(rows, C, device=DEV)
        ga = torch.ones(C, device=DEV)
        o_full, _ = guarded(rows, C, torch.float16)
        mr = torch.zeros(rows, device=DEV)
        if s16 == 0:
            with pytest.raises(PrxError, match=msg):
                call("prx_k_layernorm_fwd_op", x, C, ga, ga, o_full, None, mr, mr.clone(), rows, C, 1e-5, 1, 0, stream())
        with pytest.raises(PrxError, match=msg):
            call("prx_k_layernorm_bwd_op", x, C, x, C, ga, mr, mr, None, C, None, C, o_full, C, rows, C, 1, 0, s16, stream())
        sync()
        assert bool(torch.isnan(o_full).all())


# ================================================================================================ attention
# rel-L2 gates.  bf16: the project's (tests/test_kernels_gpu.py).  half: 2 x the largest error measured over this file's
# parametrisation (MI355X and CPU emulation, whichever is larger), never above bf16's.  The half instantiation rounds P, dS and
# the results to 11 significant bits instead of 8: the measured errors are 1/8 of bf16's, as expected.
ATT_GATES = {
    # check: (bf16 gate, half gate)      largest measured: MI355X bf16 / half; emulation subset half
    "fwd": (8e-3, 5.9e-4),             # 2.36e-3 / 2.93e-4; 2.95e-4
    "bwd": (1.2e-2, 6.0e-4),           # 2.43e-3 / 2.99e-4; 2.97e-4
    "bwd_gen": (1.5e-2, 1.23e-3),      # 4.36e-3 / 5.57e-4; 6.13e-4 (queries scaled by 6, T = 130)
    "causal": (8e-3, 4.7e-4),          # 1.87e-3 / 2.35e-4; 2.31e-4
}
assert all(h <= b for b, h in ATT_GATES.values())
LSE_GATE = 1e-5


def _unit(h16):
    return 2.0 ** -12 if h16 else 2.0 ** -9          # half an ulp, relative: the unit round-off of the 16-bit format


def _att_ref(qkv16, N, T, C, heads, causal=False):
    q, k, v = [t.reshape(N, T, heads, 64).permute(0, 2, 1, 3).double().requires_grad_(True) for t in qkv16.double().split(C, dim=1)]
    sc = q @ k.transpose(-1, -2) * 0.125
    if causal:
        sc = sc.masked_fill(torch.ones(T, T, dtype=torch.bool, device=qkv16.device).triu(1), float("-inf"))
    att = torch.softmax(sc, dim=-1)
    ref = (att @ v).permute(0, 2, 1, 3).reshape(N * T, C)
    return q, k, v, sc, att, ref


def _rows_back(t, N, T, C):
    return t.permute(0, 2, 1, 3).reshape(N * T, C)


def _median_row_zeroed_fails(ref, tol_abs):
    """the elementwise guard's own power, on the reference alone: replacing one token row (the one of median magnitude) by zeros
    must exceed the bound"""
    rowmax = ref.abs().amax(dim=1)
    r = int(rowmax.argsort()[rowmax.numel() // 2])
    broken = ref.clone()
    broken[r] = 0
    return float((broken - ref).abs().max()) > tol_abs


def attention_case(N, T, C, heads, h16, qs=1.0, general=False, grid=False, seed=0, figures=None):
    """forward + backward of the T <= 64 kernels, or of the general kernels (with lse)"""
    torch.manual_seed(N * T + seed)
    dt = fmt(h16)
    u = _unit(h16)
    if grid:      # 8 significant bits, exponents within half's normal range: the same operands in both formats
        qkv = torch.randn(N * T, 3 * C, device=DEV).clamp(-4, 4)
        qkv = torch.where(qkv.abs() < 2.0 ** -10, torch.full_like(qkv, 2.0 ** -10), qkv).to(torch.bfloat16).to(dt)
        assert torch.equal(qkv.float(), qkv.to(torch.bfloat16).float()) and torch.equal(qkv.float(), qkv.to(torch.float16).float())
    else:
        qkv = torch.randn(N * T, 3 * C, device=DEV)
        qkv[:, :C] *= qs
        qkv = qkv.to(dt)
    q, k, v, sc, att, ref = _att_ref(qkv, N, T, C, heads)
    out_full, out = guarded(N * T, C, dt)
    lse = torch.full((N * heads * T + 5,), NAN, device=DEV)
    if general:
        call("prx_k_mha_fwd_gen_op", qkv, out_full, lse, N, T, C, heads, h16, stream())
    else:
        call("prx_k_mha_fwd_op", qkv, out_full, N, T, C, heads, h16, stream())
    sync()
    refd = ref.detach()
    fig = {"fwd": rel_l2(out, refd)}
    gate = ATT_GATES["fwd"][h16]
    assert untouched(out_full, N * T, C)
    assert fig["fwd"] < gate, (fig, gate)
    # elementwise: out = sum_j P_j v_j with P rounded to 16 bits (<= u sum_j P_j |v_j|) and the result rounded once (u |out|); x 2
    Af = _rows_back(att.detach() @ v.detach().abs(), N, T, C)
    tol_f = 2 * u * float((Af + refd.abs()).max())
    fig["fwd_el"] = float((out.double() - refd).abs().max())
    assert fig["fwd_el"] <= tol_f, (fig, tol_f)
    assert _median_row_zeroed_fails(refd, tol_f)
    if general:
        assert bool(torch.isnan(lse[N * heads * T:]).all())
        lse64 = torch.logsumexp(sc.detach(), dim=-1)
        fig["lse"] = rel_l2(lse[:N * heads * T].reshape(N, heads, T), lse64)
        assert fig["lse"] < LSE_GATE, fig
    do = torch.randn(N * T, C, device=DEV)
    if grid:
        do = torch.where(do.abs() < 2.0 ** -10, torch.full_like(do, 2.0 ** -10), do.clamp(-4, 4)).to(torch.bfloat16)
    do = do.to(dt)
    dq_full, dqkv = guarded(N * T, 3 * C, dt)
    if general:
        call("prx_k_mha_bwd_gen_op", qkv, out_full, do, lse, dq_full, N, T, C, heads, h16, stream())
    else:
        call("prx_k_mha_bwd_op", qkv, do, dq_full, N, T, C, heads, h16, stream())
    sync()
    gq, gk, gv = torch.autograd.grad(ref, (q, k, v), do.double())
    assert untouched(dq_full, N * T, 3 * C)
    # the float64 intermediates the kernel keeps in 16 bits: P, dS = P o (dP - D) and its scaled form, the results
    do4 = do.double().reshape(N, T, heads, 64).permute(0, 2, 1, 3)
    dP = do4 @ v.detach().transpose(-1, -2)
    D = (dP * att.detach()).sum(dim=-1, keepdim=True)
    dS = att.detach() * (dP - D)
    for t in (dS, gq, gk, gv, refd, dP):
        assert float(t.abs().max()) < F16_MAX
    # sums of absolute values of the terms of dq = 0.125 dS k, dk = 0.125 dS^T q, dv = P^T dO; the chain rounds P, dS (whose own
    # terms are P |dP| and P |D|), O (inside D, general kernels) and the result: 4 roundings, x 2
    aS = att.detach() * (dP.abs() + D.abs())
    Aq = _rows_back(0.125 * aS @ k.detach().abs(), N, T, C)
    Ak = _rows_back(0.125 * aS.transpose(-1, -2) @ q.detach().abs(), N, T, C)
    Av = _rows_back(att.detach().transpose(-1, -2) @ do4.abs(), N, T, C)
    gate_b = ATT_GATES["bwd_gen" if general else "bwd"][h16]
    for i, (nm, gref, Ab) in enumerate(zip("qkv", (gq, gk, gv), (Aq, Ak, Av))):
        got = dqkv[:, i * C:(i + 1) * C]
        r = _rows_back(gref, N, T, C)
        fig["d" + nm] = rel_l2(got, r)
        assert fig["d" + nm] < gate_b, (nm, fig, gate_b)
        tol = 8 * u * float(Ab.max())
        fig["d" + nm + "_el"] = float((got.double() - r).abs().max())
        assert fig["d" + nm + "_el"] <= tol, (nm, fig, tol)
        if T > 1:
            assert _median_row_zeroed_fails(r, tol), nm
    if figures is not None:
        figures.append(fig)
    return fig, out.clone(), dqkv.clone(), refd, torch.cat([_rows_back(t, N, T, C) for t in (gq, gk, gv)], dim=1)


@pytest.mark.parametrize("h16", [0, 1], ids=["bf16", "half"])
@pytest.mark.parametrize("N,T", [(64, 50), (3, 64), (2, 17), (2, 1)])
def test_mha_both_formats(N, T, h16):
    """mha_fwd_kernel, mha_bwd_kernel <FmtBf16 | FmtF16> (T <= 64); measured figures and gates: ATT_GATES"""
    print(attention_case(N, T, 768, 12, h16)[0])


@pytest.mark.parametrize("h16", [0, 1], ids=["bf16", "half"])
@pytest.mark.parametrize("N,T,qs", [(2, 65, 1.0), (3, 197, 1.0), (2, 257, 1.0), (4, 50, 1.0), (2, 82, 1.0), (1, 130, 1.0), (1, 300, 1.0),
                                    (1, 512, 1.0), (1, 577, 1.0), (2, 257, 6.0), (1, 197, 6.0)])
def test_mha_general_both_formats(N, T, qs, h16):
    """<FmtBf16 | FmtF16> of mha_fwd_blk_kernel<F, 64>, mha_bwd_dq/dkv_blk_kernel<F, 64> (T <= 512), mha_fwd_gen_kernel<F, false>, mha_bwd_dq/dkv_gen_kernel<F>
    (T = 577); `qs` scales the queries so that the running maximum of the online softmax moves between key blocks"""
    print(attention_case(N, T, 256, 4, h16, qs=qs, general=True, seed=1)[0])


@pytest.mark.parametrize("h16", [0, 1], ids=["bf16", "half"])
def test_mha_causal_forward(h16):
    """mha_fwd_gen_kernel<true> (the CLIP text transformer: context 77, width 512, 8 heads) against a masked float64 softmax"""
    N, T, C, heads = 3, 77, 512, 8
    torch.manual_seed(77)
    dt, u = fmt(h16), _unit(h16)
    qkv = torch.randn(N * T, 3 * C, device=DEV).to(dt)
    q, k, v, sc, att, ref = _att_ref(qkv, N, T, C, heads, causal=True)
    out_full, out = guarded(N * T, C, dt)
    call("prx_k_mha_fwd_causal_op", qkv, out_full, N, T, C, heads, h16, stream())
    sync()
    refd = ref.detach()
    e = rel_l2(out, refd)
    print({"causal": e})
    assert untouched(out_full, N * T, C)
    assert e < ATT_GATES["causal"][h16], e
    Af = _rows_back(att.detach() @ v.detach().abs(), N, T, C)
    # per element here (not the global maximum): token 0 attends to itself alone, so out[0] = v[0] to one rounding, and an
    # off-by-one mask (token t also seeing t + 1, or not seeing itself) moves the early rows by O(1)
    ok, worst = within(out, refd, 2 * u * (Af + refd.abs()) + 16 * EPS32 * Af)
    assert ok, worst
    assert _median_row_zeroed_fails(refd, 2 * u * float((Af + refd.abs()).max()))


@pytest.mark.parametrize("general,N,T", [(False, 3, 50), (True, 2, 197)])
def test_mha_half_is_the_more_accurate_instantiation_on_identical_operands(general, N, T):
    """inputs on a grid both formats hold exactly (8 significant bits, |x| in [2^-10, 4]): the two instantiations see the same
    operands, and the one that rounds P / dS / the results to 11 significant bits instead of 8 must be the closer one everywhere"""
    C, heads = (256, 4) if general else (768, 12)
    fb, ob, db, ref, refd = attention_case(N, T, C, heads, 0, general=general, grid=True, seed=5)
    fh, oh, dh, ref2, refd2 = attention_case(N, T, C, heads, 1, general=general, grid=True, seed=5)
    assert torch.equal(ref, ref2) and torch.equal(refd, refd2)              # same operands, same float64 reference
    print(fb, fh)
    for key in ("fwd", "dq", "dk", "dv"):
        assert fh[key] < 0.5 * fb[key], (key, fh[key], fb[key])


def test_mha_refuses_what_it_has_no_kernel_for():
    qkv = torch.zeros(2 * 65, 3 * 128, dtype=torch.float16, device=DEV)
    out_full, _ = guarded(2 * 65, 128, torch.float16)
    with pytest.raises(PrxError, match="T <= 64"):
        call("prx_k_mha_fwd_op", qkv, out_full, 2, 65, 128, 2, 1, stream())
    with pytest.raises(PrxError, match="head dim 64"):
        call("prx_k_mha_fwd_causal_op", qkv, out_full, 2, 65, 128, 3, 1, stream())
    sync()
    assert bool(torch.isnan(out_full).all())


# ================================================================================================ elementwise
PREC = {"bf16": (0, torch.bfloat16, 0), "f32": (1, torch.float32, None), "fp16": (2, torch.float16, 1)}


@pytest.mark.parametrize("prec", ["bf16", "f32", "fp16"])
@pytest.mark.parametrize("rows,cols", [(256, 256), (240, 240), (64, 1024), (1, 16)])
def test_softmax_rows_every_precision(rows, cols, prec):
    """softmax_rows_kernel<T> / softmax_rows_bwd_kernel<T> for T = bf16, half, float; the transposed copy bit for bit"""
    code, dt, h16 = PREC[prec]
    torch.manual_seed(rows + cols)
    ldS, ldp, ldpt = cols + 4, cols + 8, rows + 2
    Sfull = torch.randn(rows, ldS, device=DEV) * 20
    S = Sfull[:, :cols]
    scale = 512 ** -0.5
    P_full, P = guarded(rows, cols, dt, ld=ldp)
    PT_full, PT = guarded(cols, rows, dt, ld=ldpt)
    call("prx_k_softmax_rows_op", Sfull, ldS, scale, P_full, ldp, PT_full, ldpt, rows, cols, code, stream())
    sync()
    z = S.double() * scale
    ref = torch.softmax(z, dim=-1)
    ref32 = torch.softmax(S * scale, dim=-1)
    xmax = float((z - z.amax(dim=-1, keepdim=True)).abs().max())
    # __expf enters the numerator and the row sum: 2 x EXPF_REL; scale * s, the subtraction of the maximum (times the exponent's
    # sensitivity, |x| <= xmax: inside EXPF_REL's |x| term, once more), the reciprocal and the product: 4 roundings
    intr = 3 * EXPF_REL(xmax) + 4 * EPS32
    gate = 4 * rel_l2(ref32, ref) + intr                                      # rel-L2
    gate_el = 4 * float(((ref32.double() - ref).abs() / ref).max()) + intr    # the same yardstick per element, relative
    assert gate < 1e-5 and gate_el < 1e-5
    assert untouched(P_full, rows, cols) and untouched(PT_full, cols, rows)
    assert torch.equal(bits(P.T), bits(PT)), "P^T is not P transposed bit for bit"
    e = rel_l2(P, ref)
    print({"softmax": e, "gate": gate})
    if prec == "f32":
        assert e <= gate, (e, gate)
        ok, worst = within(P, ref, gate_el * ref)
    else:
        ok, worst = within(P, ref, ulp16(ref, h16) + gate_el * ref)
    assert ok, worst
    # backward, from the kernel's own (rounded) P: dS = scale * P o (dP - rowsum(dP o P))
    lddp, ldds, lddst = cols + 12, cols + 16, rows + 6
    dPfull = torch.randn(rows, lddp, device=DEV)
    dP = dPfull[:, :cols]
    dS_full, dS = guarded(rows, cols, dt, ld=ldds)
    dST_full, dST = guarded(cols, rows, dt, ld=lddst)
    call("prx_k_softmax_rows_bwd_op", P_full, ldp, dPfull, lddp, scale, dS_full, ldds, dST_full, lddst, rows, cols, code, stream())
    sync()
    p64, dp64 = P.double(), dP.double()
    dot = (p64 * dp64).sum(dim=-1, keepdim=True)
    refd = scale * p64 * (dp64 - dot)
    pf = P.float()
    refd32 = scale * pf * (dP - (pf * dP).sum(dim=-1, keepdim=True))
    Ad = scale * p64 * (dp64.abs() + (p64 * dp64).abs().sum(dim=-1, keepdim=True))
    yard = float(((refd32.double() - refd).abs() / Ad.clamp_min(1e-300)).max())          # torch's fp32 evaluation, relative to the terms
    k_rel = 4 * yard + 4 * EPS32                                                          # product, subtraction, two multiplications
    assert k_rel < 1e-5
    assert untouched(dS_full, rows, cols) and untouched(dST_full, cols, rows)
    assert torch.equal(bits(dS.T), bits(dST)), "dS^T is not dS transposed bit for bit"
    if prec == "f32":
        ok, worst = within(dS, refd, k_rel * Ad)
    else:
        ok, worst = within(dS, refd, ulp16(refd, h16) + k_rel * Ad)
    assert ok, worst


def test_softmax_rows_refuses_an_unknown_precision():
    S = torch.zeros(4, 16, device=DEV)
    P_full, _ = guarded(4, 16, torch.float32)
    with pytest.raises(PrxError, match="unknown precision"):
        call("prx_k_softmax_rows_op", S, 16, 1.0, P_full, 16, None, 0, 4, 16, 3, stream())
    with pytest.raises(PrxError, match="unknown precision"):
        call("prx_k_softmax_rows_bwd_op", P_full, 16, S, 16, 1.0, P_full, 16, None, 0, 4, 16, -1, stream())


@pytest.mark.parametrize("f32", [0, 1], ids=["16bit", "fp32"])
@pytest.mark.parametrize("R,C", [(33, 70), (1, 1), (100, 31), (257, 129), (64, 96)])
def test_transpose_ragged(R, C, f32):
    """transpose_op_kernel<bf16_t> / <float>: R, C not multiples of the 32 x 32 tile, both leading dimensions wider than the rows"""
    torch.manual_seed(R * C)
    dt = torch.float32 if f32 else torch.float16           # 16-bit data movement does not depend on the format
    ldin, ldout = C + 5, R + 3
    a = (torch.randn(R, ldin, device=DEV) * 100).to(dt)
    o_full, o = guarded(C, R, dt, ld=ldout)
    call("prx_k_transpose_op", a, ldin, o_full, ldout, R, C, f32, stream())
    sync()
    assert torch.equal(bits(o), bits(a[:, :C].T)) and untouched(o_full, C, R)


@pytest.mark.parametrize("h16", [0, 1], ids=["bf16", "half"])
@pytest.mark.parametrize("s16", [0, 1])
@pytest.mark.parametrize("NB,Hl,Wl,C", [(1, 5, 7, 128), (2, 3, 9, 64), (2, 1, 1, 4), (1, 16, 16, 256)])
def test_upsample2x_bwd_variants(NB, Hl, Wl, C, s16, h16):
    """upsample2x_bwd_kernel<false / true>: odd maps, two images, the 16-bit output alone (low == nullptr)"""
    torch.manual_seed(Hl * Wl + C)
    sdt = fmt(h16) if s16 else torch.float32
    hi = (torch.randn(NB, 2 * Hl, 2 * Wl, C, device=DEV) * 3).to(sdt)
    rows = NB * Hl * Wl
    h64 = hi.double().view(NB, Hl, 2, Wl, 2, C)
    ref = h64.sum(dim=(2, 4)).reshape(rows, C)
    A = h64.abs().sum(dim=(2, 4)).reshape(rows, C)
    k = 3 * EPS32                                                             # three additions
    for both in (True, False):
        l16_full, l16 = guarded(rows, C, fmt(h16))
        l32_full, l32 = guarded(rows, C, torch.float32) if both else (None, None)
        call("prx_k_upsample2x_bwd_op", hi, l32_full, l16_full, NB, Hl, Wl, C, h16, s16, stream())
        sync()
        assert untouched(l16_full, rows, C)
        if both:
            assert untouched(l32_full, rows, C)
            ok, worst = within(l32, ref, k * A)
            assert ok, worst
            assert torch.equal(bits(l16), bits(to16(l32, h16)))
        check16(l16, ref, h16, k, A)
    with pytest.raises(PrxError, match="no output"):
        call("prx_k_upsample2x_bwd_op", hi, None, None, NB, Hl, Wl, C, h16, s16, stream())


def _edge_values(h16):
    """+-0, subnormals of the target format, its largest finite value, values just above it, a tie, inf; ragged length"""
    if h16:
        sub, big = [2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -26], F16_MAX
        above = [65505.0, 65519.996, 65520.0, 65536.0, 1e6, 3e38]
    else:
        sub, big = [2.0 ** -133, 3 * 2.0 ** -133, 2.0 ** -134, 2.0 ** -127, 2.0 ** -126 - 2.0 ** -133], 3.3895313892515355e38
        above = [3.39e38, 3.3961775292304602e38, 3.4028234663852886e38]
    vals = [0.0, -0.0, 1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, big, float("inf")] + sub + above
    v = torch.tensor(vals + [-t for t in vals], dtype=torch.float32)
    torch.manual_seed(9)
    return torch.cat([v, torch.randn(1031 - v.numel()) * 300]).to(DEV)


@pytest.mark.parametrize("h16", [0, 1], ids=["bf16", "half"])
def test_f32_to_op16_and_scale_dev_conversions(h16):
    """f32_to_bf16_kernel, scale_dev_kernel: round-to-nearest-even, half saturates to +-65504 (inf included), bf16 does not"""
    v = _edge_values(h16)
    n = v.numel()
    assert n == 1031
    o_full = torch.full((n + 9,), NAN, dtype=fmt(h16), device=DEV)
    call("prx_k_f32_to_op16", v, o_full, n, h16, stream())
    sync()
    want = to16(v, h16)
    assert torch.equal(bits(o_full[:n]), bits(want)) and bool(torch.isnan(o_full[n:]).all())
    if h16:
        assert float(o_full[:n].float().abs().max()) == F16_MAX and bool(torch.isfinite(o_full[:n]).all())
    else:
        assert bool(torch.isinf(o_full[:n].float()).any()) and bool(torch.isinf(want[torch.isfinite(v)].float()).any())
    for sc in (1.0, 2.0 ** -3, 2.0 ** 7, 2.0 ** -20):
        x_full = torch.full((n + 9,), NAN, device=DEV)
        x_full[:n] = v
        scale = torch.tensor([sc, NAN], device=DEV)
        o_full = torch.full((n + 9,), NAN, dtype=fmt(h16), device=DEV)
        call("prx_k_scale_dev", x_full, n, scale, o_full, h16, stream())
        sync()
        want32 = v * sc                                                       # a power of two: exact up to overflow / fp32 subnormals
        assert torch.equal(bits(x_full[:n]), bits(want32)) and bool(torch.isnan(x_full[n:]).all())
        assert torch.equal(bits(o_full[:n]), bits(to16(want32, h16))) and bool(torch.isnan(o_full[n:]).all())
    x2 = v.clone()
    call("prx_k_scale_dev", x2, n, torch.tensor([0.5], device=DEV), None, h16, stream())     # out16 is optional
    sync()
    assert torch.equal(bits(x2), bits(v * 0.5))
    a, b = v, v.flip(0).contiguous()
    s_full = torch.full((n + 9,), NAN, device=DEV)
    call("prx_k_add_f32", a, b, s_full, n, stream())
    sync()
    ok = torch.equal(bits((a + b).nan_to_num(nan=7.0)), bits(s_full[:n].nan_to_num(nan=7.0)))      # inf - inf = NaN on both sides
    assert ok and bool(torch.isnan(s_full[n:]).all())


@pytest.mark.parametrize("h16", [0, 1], ids=["bf16", "half"])
def test_nchw_to_nhwc_both_formats(h16):
    torch.manual_seed(3)
    NB, C, HW, Cpad = 2, 3, 50, 8
    x = torch.randn(NB, C, HW, device=DEV) * 100
    x[0, 0, :4] = torch.tensor([70000.0, -70000.0, 2.0 ** -25, -0.0], device=DEV)
    o32_full, o32 = guarded(NB * HW, Cpad, torch.float32)
    o16_full, o16 = guarded(NB * HW, Cpad, fmt(h16))
    call("prx_k_nchw_to_nhwc_op", x, o32_full, o16_full, NB, C, HW, Cpad, h16, stream())
    sync()
    want = torch.zeros(NB, HW, Cpad, device=DEV)
    want[..., :C] = x.permute(0, 2, 1)
    want = want.reshape(NB * HW, Cpad)
    assert torch.equal(bits(o32), bits(want)) and torch.equal(bits(o16), bits(to16(want, h16)))
    assert untouched(o32_full, NB * HW, Cpad) and untouched(o16_full, NB * HW, Cpad)
    o16b_full, o16b = guarded(NB * HW, Cpad, fmt(h16))
    call("prx_k_nchw_to_nhwc_op", x, None, o16b_full, NB, C, HW, Cpad, h16, stream())
    sync()
    assert torch.equal(bits(o16b), bits(o16))


def _image_head_inputs(NB, C, H, W, ld):
    torch.manual_seed(H * W + C)
    HW = H * W
    x = torch.randn(NB, HW, ld, device=DEV) * 1.5
    # exactly at u = 0 and u = 1, one fp32 step to either side of both, far out on both sides
    edge = torch.tensor([-1.0, 1.0, -1.0 - 2.0 ** -23, -1.0 + 2.0 ** -24, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, -3.0, 3.0], device=DEV)
    x[:, :16, :C] = edge.repeat(2)[None, :, None]
    g = torch.randn(NB, C, HW, device=DEV)
    g[:, :, 8:16] = -g[:, :, :8]                                              # every edge with both gradient signs
    g[:, :, 16] = 0.0
    g[:, :, 17] = 60000.0                                                     # x 2^7 x 0.5: beyond the half range -> saturates
    g[:, :, 18] = 2.0 ** -20                                                  # x 2^-3 x 0.5: a half subnormal
    return x, g


def _image_head_ref(x, g, C, gs):
    """ClampWithGrad.backward (the gradient passes where g * (u - clamp(u)) >= 0, u = (x + 1) / 2 in fp32 as the forward computes it),
    then d/dx of (x + 1) / 2 and the power-of-two scale: exact in fp32 -- bit equality"""
    u = (x[..., :C].permute(0, 2, 1) + 1) / 2
    return torch.where(g * (u - u.clamp(0, 1)) >= 0, g * (0.5 * gs), torch.zeros_like(g)).permute(0, 2, 1)           # [NB][HW][C]


@pytest.mark.parametrize("h16", [0, 1], ids=["bf16", "half"])
@pytest.mark.parametrize("gs", [None, 2.0 ** -3, 2.0 ** 7])
def test_image_head_bwd_with_device_scale(gs, h16):
    """image_head_bwd_kernel with h16 and a device gscale: the scale multiplies the gradient, not the sign test"""
    NB, C, H, W, ld, ldo = 2, 3, 9, 7, 4, 8
    HW = H * W
    x, g = _image_head_inputs(NB, C, H, W, ld)
    gsd = None if gs is None else torch.tensor([gs, NAN], device=DEV)
    want = torch.zeros(NB * HW, ldo, device=DEV)
    want[:, :C] = _image_head_ref(x, g, C, 1.0 if gs is None else gs).reshape(NB * HW, C)
    dx_full, dx = guarded(NB * HW, ldo, torch.float32)
    d16_full, d16 = guarded(NB * HW, ldo, fmt(h16))
    call("prx_k_image_head_bwd_op", x, ld, g, dx_full, d16_full, ldo, NB, C, HW, h16, gsd, stream())
    sync()
    assert torch.equal(bits(dx), bits(want)) and untouched(dx_full, NB * HW, ldo)
    assert torch.equal(bits(d16), bits(to16(want, h16))) and untouched(d16_full, NB * HW, ldo)
    assert float(want.abs().max()) > 0 and bool((want[:16, :C] == 0).any()) and bool((want[:16, :C] != 0).any())
    d16b_full, d16b = guarded(NB * HW, ldo, fmt(h16))
    call("prx_k_image_head_bwd_op", x, ld, g, None, d16b_full, ldo, NB, C, HW, h16, gsd, stream())
    sync()
    assert torch.equal(bits(d16b), bits(d16))


@pytest.mark.parametrize("h16", [0, 1], ids=["bf16", "half"])
@pytest.mark.parametrize("gs", [None, 2.0 ** -3, 2.0 ** 7])
@pytest.mark.parametrize("H,W,ldk", [(9, 7, 72), (5, 11, 96), (1, 1, 80), (16, 16, 128)])
def test_image_head_bwd_im2col_is_unfold_of_the_plain_backward(H, W, ldk, gs, h16):
    """image_head_bwd_im2col_kernel: col[p][tap * 8 + c] = dy[(y + ky - 1, x + kx - 1)][c], zero outside the image, zero in the
    padding channels 3 .. 7 of every tap and in the columns 72 .. ldk - 1"""
    C, ld = 3, 4
    HW = H * W
    x, g = _image_head_inputs(1, C, H, W, ld) if HW >= 19 else (torch.full((1, 1, ld), 0.25, device=DEV), torch.full((1, C, 1), -1.5, device=DEV))
    gsd = None if gs is None else torch.tensor([gs, NAN], device=DEV)
    dy = torch.zeros(1, 8, H, W, device=DEV)
    dy[0, :C] = _image_head_ref(x, g, C, 1.0 if gs is None else gs)[0].T.reshape(C, H, W)
    dy16 = to16(dy, h16).float()                                              # exactly representable in fp32: unfold only moves it
    want = torch.zeros(HW, ldk, device=DEV)
    want[:, :72] = F.unfold(dy16, 3, padding=1).reshape(8, 9, HW).permute(2, 1, 0).reshape(HW, 72)
    col_full, col = guarded(HW, ldk, fmt(h16))
    call("prx_k_image_head_bwd_im2col", x, ld, g, col_full, ldk, C, H, W, h16, gsd, stream())
    sync()
    assert torch.equal(bits(col), bits(want.to(fmt(h16)))) and bool(torch.isnan(col_full[HW:]).all())
    with pytest.raises(PrxError, match="im2col"):
        call("prx_k_image_head_bwd_im2col", x, ld, g, col_full, 76, C, H, W, h16, gsd, stream())


def _expected_scale(g, target):
    """elementwise.h: S * max|g| in [2^(T-1), 2^T); S = 1 for an all-zero gradient or one that holds an inf or a NaN"""
    if not bool(torch.isfinite(g).all()):
        return 1.0
    m = float(g.abs().max())
    if m == 0.0:
        return 1.0
    _, e = math.frexp(m)                                                      # m = f * 2^e, f in [0.5, 1)
    return math.ldexp(1.0, max(-40, min(60, target - e)))


def _grad_scale_vectors():
    torch.manual_seed(4)
    base = torch.randn(1025) * 0.01
    out = {}
    v = base.clone(); v[517] = -0.25; out["power_of_two"] = v                 # max|g| = 2^-2 exactly
    v = base.clone(); v[1024] = 1.0 - 2.0 ** -24; out["just_below_one"] = v
    v = base.clone(); v[0] = 1.0; out["one"] = v
    out["all_zero"] = torch.zeros(1025)
    v = base.clone(); v[700] = float("inf"); out["inf"] = v
    v = base.clone(); v[3] = float("-inf"); out["neg_inf"] = v
    v = base.clone(); v[300] = NAN; out["one_nan_among_finite"] = v
    v = base.clone(); v[1024] = NAN; out["nan_in_the_last_entry"] = v
    out["n1"] = torch.tensor([-3.0])
    out["n1_nan"] = torch.tensor([NAN])
    out["tiny"] = base * 2.0 ** -100                                          # the exponent clamp k <= 60
    out["huge"] = base * 2.0 ** 100                                           # ... and k >= -40
    out["subnormal_max"] = torch.full((1025,), 2.0 ** -140)
    return out


@pytest.mark.parametrize("target", [4, 0, 12])
def test_grad_scale_is_the_documented_power_of_two(target):
    """amax_partial_kernel + grad_scale_final_kernel (prx_grad_scale, prx_grad_scale_multi) against math.frexp on the host.
    Found by the `one_nan_among_finite` case: the partial maximum was taken with fmaxf, which drops a NaN operand, so a gradient
    with a NaN among finite values got an ordinary S although elementwise.h documents S = 1 for a non-finite gradient"""
    nparts = 64
    for name, v in _grad_scale_vectors().items():
        g = v.to(DEV)
        n = g.numel()
        part = torch.full((nparts + 4,), NAN, device=DEV)
        sc = torch.full((2 + 3,), NAN, device=DEV)
        call("prx_k_grad_scale", g, n, part, nparts, target, sc, stream())
        sync()
        S = _expected_scale(v, target)
        assert sc[:2].tolist() == [S, 1.0 / S], (name, sc.tolist(), S)
        assert bool(torch.isnan(sc[2:]).all()) and bool(torch.isnan(part[nparts:]).all()), name
        m = float(v.abs().max())
        if math.isfinite(m) and m > 0 and -40 < target - math.frexp(m)[1] < 60:
            assert 2.0 ** (target - 1) <= S * m < 2.0 ** target, (name, S * m)
    # several tensors, one common S: a null / empty entry is skipped, the NaN of one tensor decides for all
    vs = _grad_scale_vectors()
    for names in (["power_of_two", "just_below_one"], ["all_zero", "n1", "tiny"], ["power_of_two", "one_nan_among_finite"], ["all_zero", "all_zero"],
                  ["huge", "inf"]):
        ts = [vs[k].to(DEV) for k in names]
        ptrs = (ctypes.c_void_p * (len(ts) + 1))(*([t.data_ptr() for t in ts] + [None]))
        ns = (ctypes.c_size_t * (len(ts) + 1))(*([t.numel() for t in ts] + [5]))
        part = torch.full(((len(ts) + 1) * nparts + 4,), NAN, device=DEV)
        sc = torch.full((5,), NAN, device=DEV)
        call("prx_k_grad_scale_multi", ctypes.addressof(ptrs), ctypes.addressof(ns), len(ts) + 1, part, nparts, target, sc, stream())
        sync()
        S = _expected_scale(torch.cat([vs[k] for k in names]), target)
        assert sc[:2].tolist() == [S, 1.0 / S], (names, sc.tolist(), S)
        assert bool(torch.isnan(sc[2:]).all()) and bool(torch.isnan(part[(len(ts) + 1) * nparts:]).all())
    with pytest.raises(PrxError, match="partials"):
        call("prx_k_grad_scale", vs["one"].to(DEV), 1025, part, 0, target, sc, stream())


# ================================================================================================ a CPU-sized subset (tests/test_emu_cpu.py)
def emu_subset():
    """every variant flag at least once at sizes the CPU emulation runs in seconds; returns the attention figures"""
    for s16, h16 in [(0, 0), (0, 1), (1, 0), (1, 1)]:
        groupnorm_case(2, 3, 128, 1, True, s16, h16)
        groupnorm_case(3, 255, 512, 1, True, s16, h16)                     # slices and strides that cross the image boundary
        groupnorm_case(2, 240, 256, 0, False, s16, h16)
    groupnorm_case(1, 21, 1024, 1, True, 1, 1, fp32_out=False)
    groupnorm_case(3, 700, 1024, 1, True, 1, 1)                            # a thread's second quad lies in the next image (gn_lane_load reload)
    groupnorm_case(2, 255, 256, 1, True, 1, 1, stats_ready=1)
    groupnorm_case(2, 240, 256, 0, True, 0, 1, mean=32.0, sigma=1.0)         # a group mean 32 standard deviations from zero
    test_groupnorm_refuses_channel_counts_it_cannot_tile(64)
    test_groupnorm_refuses_channel_counts_it_cannot_tile(96)
    for h16 in (0, 1):
        for s16 in (0, 1, 2, 7):
            layernorm_case(5, 256, h16, s16)
            layernorm_case(9, 1280, h16, s16)
        layernorm_case(2 * 50, 768, h16, 7, add_every=50)
        layernorm_case(2 * 50, 1024, h16, 0, add_every=50, fp32_out=False)
        layernorm_case(1, 2048, h16, 1, fp32_out=False)
    test_layernorm_refuses_what_it_has_no_kernel_for()
    figs = {0: [], 1: []}
    for h16 in (0, 1):
        attention_case(2, 17, 128, 2, h16, figures=figs[h16])
        attention_case(1, 1, 64, 1, h16, figures=figs[h16])
        attention_case(2, 65, 128, 2, h16, general=True, figures=figs[h16])
        attention_case(1, 130, 64, 1, h16, qs=6.0, general=True, figures=figs[h16])
        test_mha_causal_forward(h16)
    test_mha_half_is_the_more_accurate_instantiation_on_identical_operands(False, 3, 50)
    test_mha_refuses_what_it_has_no_kernel_for()
    for prec in ("bf16", "f32", "fp16"):
        test_softmax_rows_every_precision(64, 80, prec)
        test_softmax_rows_every_precision(1, 16, prec)
    test_softmax_rows_refuses_an_unknown_precision()
    for f32 in (0, 1):
        test_transpose_ragged(33, 70, f32)
    for h16 in (0, 1):
        for s16 in (0, 1):
            test_upsample2x_bwd_variants(2, 3, 9, 64, s16, h16)
        test_f32_to_op16_and_scale_dev_conversions(h16)
        test_nchw_to_nhwc_both_formats(h16)
        for gs in (None, 2.0 ** -3, 2.0 ** 7):
            test_image_head_bwd_with_device_scale(gs, h16)
            test_image_head_bwd_im2col_is_unfold_of_the_plain_backward(5, 11, 96, gs, h16)
        test_image_head_bwd_im2col_is_unfold_of_the_plain_backward(1, 1, 80, None, h16)
    test_grad_scale_is_the_documented_power_of_two(4)
    return figs
