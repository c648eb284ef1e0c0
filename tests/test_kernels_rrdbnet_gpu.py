"""Kernel-level float64 tests (GPU) of csrc/rrdbnet.hip, one kernel at a time through `prx_k_rrdb_*`: the 3x3 convolution family
of the RRDBNet runner (forward and data gradient, every channel prefix, the nearest-2x read and its 2x2-sum backward, the fused
residuals, the LeakyReLU derivative from the stored activation) and the two edge convolutions with the fused clamp rule.

Method: every buffer a call may write is pre-filled with NaN, is wider than the slice the call owns (pixel stride 192, as the
runner's concat buffers) and carries spare rows; afterwards everything outside the slice is still NaN.  The channels beyond the
prefix a convolution may READ hold NaN too, so a kernel that reads past its Cin poisons its output.  References are plain torch
on the CPU in float64.

Gates (computed in the test from the float64 reference at the test's own shapes, never from the kernel's output):
  * "f32"  : rel-L2 <= 8 x the rel-L2 error of torch's own fp32 evaluation of the same convolution against float64 (both are
             fp32 sums over K <= 1728 in different orders; a wrong tap, offset or scale shows at 1e-2 or more);
  * "fp16" : rel-L2 <= 3 x the error of the float64 convolution with its weights and its input (or the gradient entering the
             data gradient) rounded to IEEE half, against plain float64.  This holds every output, half-typed or fp32, with one
             exception that is a property of the number format and not of a kernel: conv5 writes 0.2 v + x twice, as the fp32
             trunk stream and as the next block's half operand.  The residual x enters exactly, so the yardstick of that
             case is ~5e-5 (only the 0.2 v part carries operand rounding), while ANY half store of the sum is off by up to
             2^-11 relative (rel-L2 ~2e-4 > 3 x 5e-5).  There the fp32 stream carries the gate, and the half store must be
             BIT-EQUAL to the round-to-nearest-even half of the fp32 stream -- the tightest statement a half store admits.
             The same bit-equality is asserted wherever a kernel writes both forms.
LeakyReLU derivative: the stored activation a decides, a > 0 -> 1, else 0.2 -- exact zero takes the 0.2 side, as torch's
leaky_relu backward does (`x > 0`).

Measured on an MI355X (`pytest -s` prints `[rrdb-fig] name error gate`), worst error / gate over all cases: forward 0.21 (f32) /
0.42 (fp16: half operands, exact sums, a half store); data gradient 0.20 / 0.33; up backward 0.17 / 0.33; conv_first 0.13 / 0.27
and its backward 0.30; conv_last 0.28 / 0.25 and its backward 0.14.  Every half store was bit-equal to the rounding of its fp32
twin.  The fp16 data-gradient ratios sit at 1/3 because the kernels' roundings ARE the yardstick's."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from pixray_amd import _lib
from pixray_amd._lib import PrxError, call, precision_code

import _rrdbnet_ref as R

DEV = "cuda"          # tests/test_emu_super_resolution.py switches this to "cpu" for the emulated kernels
NAN = float("nan")
SIZES = [(5, 7), (17, 33)]      # all border-adjacent; 561 pixels: ragged last tile of 16, rows that straddle tiles
MODES = ["f32", "fp16"]
SPARE = 3


def tdt(mode):
    return torch.float32 if mode == "f32" else torch.float16


def sync():
    torch.cuda.synchronize()


def stream():
    return _lib.current_stream()


def nanbuf(rows, ld, dtype):
    return torch.full((rows + SPARE, ld), NAN, dtype=dtype, device=DEV)


def put(buf, rows, lo, values):
    buf[:rows, lo:lo + values.shape[1]] = values.to(buf.dtype).to(DEV)


def only_slice_written(buf, rows, lo, hi):
    """everything outside buf[:rows, lo:hi] is still NaN, everything inside is finite"""
    b = buf.detach().cpu().double()
    inside = b[:rows, lo:hi]
    mask = torch.ones_like(b, dtype=torch.bool)
    mask[:rows, lo:hi] = False
    return bool(torch.isfinite(inside).all()) and bool(torch.isnan(b[mask]).all())


def nhwc(t):          # [1,C,H,W] -> [H*W, C]
    return t[0].permute(1, 2, 0).reshape(-1, t.shape[1]).contiguous()


def nchw(t, H, W):    # [H*W, C] -> [1,C,H,W]
    return t.reshape(H, W, -1).permute(2, 0, 1)[None].contiguous()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def make_w(cout, cin, g):
    return torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) / (cin * 9) ** 0.5, 0.1 * torch.randn(cout, generator=g, dtype=torch.float64)


def check(name, got, ref, yard, mode):
    gate = (8.0 if mode == "f32" else 3.0) * yard
    err = R.rel_l2(got, ref)
    print(f"[rrdb-fig] {name} {mode} error {err:.3e} gate {gate:.3e}")
    assert yard > 0 and err <= gate, (name, mode, err, gate)


def slope(a):
    return torch.where(a > 0, torch.ones_like(a), torch.full_like(a, 0.2))


def conv_fwd_case(Cin, Cout, H, W, mode, resid=0, up=False, lrelu=True, seed=0):
    g = gen(seed + 7 * Cin + H)
    T = tdt(mode)
    h, w = (H // 2, W // 2) if up else (H, W)
    x = torch.randn(1, Cin, h, w, generator=g, dtype=torch.float64)
    wt, b = make_w(Cout, Cin, g)
    r1 = torch.randn(1, 64, H, W, generator=g, dtype=torch.float64) if resid >= 1 else None
    r2 = torch.randn(1, 64, H, W, generator=g, dtype=torch.float64) if resid >= 2 else None
    alpha, beta = (1.0, 1.0) if resid == 0 else ((0.2, 1.0) if resid == 1 else (0.04, 0.2))

    def ref(xx, ww, bb, dt):
        xi = F.interpolate(xx.to(dt), scale_factor=2, mode="nearest") if up else xx.to(dt)
        v = F.conv2d(xi, ww.to(dt), bb.to(dt), padding=1)
        if lrelu:
            v = F.leaky_relu(v, 0.2)
        v = alpha * v
        if r1 is not None:
            v = v + beta * r1.to(dt)
        if r2 is not None:
            v = v + r2.to(dt)
        return v.double()

    exact = ref(x, wt, b, torch.float64)
    yard = R.rel_l2(ref(x, wt, b, torch.float32), exact) if mode == "f32" else R.rel_l2(ref(R.q16(x), R.q16(wt), b, torch.float64), exact)
    P, p = H * W, h * w
    same = Cout == 32 and not up and Cin + 32 <= 192     # the runner's case: the output slice lies in the buffer the prefix is read from
    xin = nanbuf(p, 192, T)
    put(xin, p, 0, nhwc(x))
    out = xin if same else nanbuf(P, 192, T)
    out_off = Cin if same else 0
    of = None if same else nanbuf(P, 64, torch.float32)
    r1d = None if r1 is None else nhwc(r1).float().to(DEV)
    r2d = None if r2 is None else nhwc(r2).float().to(DEV)
    before = xin[:p, :Cin].clone()
    call("prx_k_rrdb_conv", 0, xin, 192, 0, None, 0, 0, wt.float().to(DEV).contiguous(), b.float().to(DEV), Cin, Cout, H, W, int(up), int(lrelu),
         alpha, beta, r1d, 64, r2d, 64, out, 192, out_off, of, 64, 0, 0, precision_code(mode), stream())
    sync()
    assert torch.equal(xin[:p, :Cin], before), "the input prefix was modified"
    if same:
        b2 = out.clone()
        b2[:p, :Cin] = NAN
        assert only_slice_written(b2, P, out_off, out_off + Cout)
    else:
        assert only_slice_written(out, P, 0, Cout) and only_slice_written(of, P, 0, Cout)
        assert only_slice_written(xin, p, 0, Cin)
        check(f"fwd{Cin}->{Cout} {H}x{W} r{resid} up{int(up)} f32copy", nchw(of[:P, :Cout].cpu().double(), H, W), exact, yard, mode)
        assert torch.equal(out[:P, :Cout], of[:P, :Cout].to(T)), "the T-typed output is not the rounding of the fp32 output"
    if resid == 0 or mode == "f32":
        # (conv5's half store next to a residual is held to the bit-equality above instead: see the module docstring)
        check(f"fwd{Cin}->{Cout} {H}x{W} r{resid} up{int(up)}", nchw(out[:P, out_off:out_off + Cout].cpu().double(), H, W), exact, yard, mode)


def hand_act(shape, g):
    """activations of both signs and exact zeros"""
    a = torch.randn(shape, generator=g, dtype=torch.float64)
    a[torch.rand(shape, generator=g) < 0.15] = 0.0
    return a


def conv_dgrad_case(Cin, Cout, H, W, mode, resid=0, seed=0):
    """the data gradient of a Cin -> Cout convolution: gradient slice [Cin, Cin + 32) (or a separate [.., 64] for Cout = 64), the
    result accumulated into the prefix [0, Cin) of the same gradient buffer, twice"""
    g = gen(seed + 11 * Cin + H)
    T = tdt(mode)
    P = H * W
    wt, _ = make_w(Cout, Cin, g)
    go = torch.randn(1, Cout, H, W, generator=g, dtype=torch.float64)
    act = hand_act((1, Cout, H, W), g) if Cout == 32 else None
    act_t = None if act is None else act.to(T).double()          # what the kernel sees decides the slope
    gin = go if act is None else go * slope(act_t)
    alpha, beta = (1.0, 1.0) if resid == 0 else ((0.2, 1.0) if resid == 1 else (0.04, 0.2))
    r2 = torch.randn(1, 64, H, W, generator=g, dtype=torch.float64) if resid >= 2 else None

    def ref(gg, ww, dt):          # the whole expression in `dt`, the final sum included (the kernel's output is an fp32 sum too)
        v = alpha * F.conv_transpose2d(gg.to(dt), ww.to(dt), padding=1)
        if resid >= 1:
            v[:, :64] += beta * go.to(dt)
        if r2 is not None:
            v[:, :64] += r2.to(dt)
        return v.double()

    exact = ref(gin, wt, torch.float64)
    yard = R.rel_l2(ref(gin, wt, torch.float32), exact) if mode == "f32" else R.rel_l2(ref(R.q16(gin), R.q16(wt), torch.float64), exact)
    G = nanbuf(P, 192, torch.float32)
    wd = wt.float().to(DEV).contiguous()
    if Cout == 32:
        sep = Cin + 32 > 192              # 192 -> 32 is not a runner case: its gradient slice needs a buffer of its own
        base = torch.randn(P, Cin, generator=g, dtype=torch.float64).float()
        put(G, P, 0, base)
        S = nanbuf(P, 64, torch.float32) if sep else G
        off, ld = (0, 64) if sep else (Cin, 192)
        put(S, P, off, nhwc(go))
        A = nanbuf(P, ld, T)
        put(A, P, off, nhwc(act))
        for rep in (1, 2):
            call("prx_k_rrdb_conv", 1, S, ld, off, A, ld, off, wd, None, Cin, Cout, H, W, 0, 0, 1.0, 1.0, None, 0, None, 0, None, 0, 0, G, 192, 0, 1,
                 precision_code(mode), stream())
            sync()
            chk = G.clone()
            if not sep:
                chk[:P, Cin:Cin + 32] = NAN
            assert only_slice_written(chk, P, 0, Cin), "wrote outside the prefix / read NaN from beyond the slice"
            assert torch.equal(S[:P, off:off + 32].cpu(), nhwc(go).float()), "the gradient slice was modified"
            got = (G[:P, :Cin].cpu().double() - base.double()) / rep
            check(f"dgrad{Cin}->{Cout} {H}x{W} x{rep}", nchw(got, H, W), exact, yard, mode)
    else:
        gsrc = nanbuf(P, 192, torch.float32)
        put(gsrc, P, 0, nhwc(go))
        r2d = None if r2 is None else nhwc(r2).float().to(DEV)
        call("prx_k_rrdb_conv", 1, gsrc, 192, 0, None, 0, 0, wd, None, Cin, Cout, H, W, 0, 0, alpha, beta, gsrc if resid else None, 192, r2d, 64,
             None, 0, 0, G, 192, 0, 0, precision_code(mode), stream())
        sync()
        assert only_slice_written(G, P, 0, Cin) and only_slice_written(gsrc, P, 0, 64)
        check(f"dgrad{Cin}->{Cout} {H}x{W} r{resid}", nchw(G[:P, :Cin].cpu().double(), H, W), exact, yard, mode)


# ------------------------------------------------------------------------------------------------ the convolution family
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("Cin", [64, 96, 128, 160])
def test_conv_forward_prefix_to_32(Cin, hw, mode):
    conv_fwd_case(Cin, 32, hw[0], hw[1], mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("resid", [0, 1, 2])
def test_conv_forward_192(resid, hw, mode):
    if resid == 0:
        conv_fwd_case(192, 32, hw[0], hw[1], mode)                    # 192 -> 32: the widest prefix on the 32-channel path
    else:
        conv_fwd_case(192, 64, hw[0], hw[1], mode, resid=resid, lrelu=False)    # conv5: 0.2 v + x, and the RRDB-level second residual


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("Cin", [64, 96, 128, 160, 192])
def test_conv_dgrad_accumulates_into_prefix(Cin, hw, mode):
    conv_dgrad_case(Cin, 32, hw[0], hw[1], mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("resid", [1, 2])
def test_conv_dgrad_192_to_64(resid, hw, mode):
    conv_dgrad_case(192, 64, hw[0], hw[1], mode, resid=resid)


@pytest.mark.parametrize("mode", MODES)
def test_conv_up_forward_and_backward(mode):
    conv_fwd_case(64, 64, 10, 14, mode, up=True)                      # 5 x 7 read nearest-2x -> 10 x 14
    # backward: the data gradient on the 10 x 14 grid, then the 2 x 2 sum back to 5 x 7
    g = gen(99)
    T = tdt(mode)
    H, W, h, w = 10, 14, 5, 7
    wt, _ = make_w(64, 64, g)
    go = torch.randn(1, 64, H, W, generator=g, dtype=torch.float64)
    act = hand_act((1, 64, H, W), g)
    gin = go * slope(act.to(T).double())

    def ref(gg, ww, dt):
        d = F.conv_transpose2d(gg.to(dt), ww.to(dt), padding=1)
        return (d[..., 0::2, 0::2] + d[..., 0::2, 1::2] + d[..., 1::2, 0::2] + d[..., 1::2, 1::2]).double()

    exact = ref(gin, wt, torch.float64)
    yard = R.rel_l2(ref(gin, wt, torch.float32), exact) if mode == "f32" else R.rel_l2(ref(R.q16(gin), R.q16(wt), torch.float64), exact)
    gb = nanbuf(H * W, 64, torch.float32)
    put(gb, H * W, 0, nhwc(go))
    A = nanbuf(H * W, 64, T)
    put(A, H * W, 0, nhwc(act))
    tmp = nanbuf(H * W, 64, torch.float32)
    out = nanbuf(h * w, 64, torch.float32)
    call("prx_k_rrdb_conv", 1, gb, 64, 0, A, 64, 0, wt.float().to(DEV).contiguous(), None, 64, 64, H, W, 0, 0, 1.0, 1.0, None, 0, None, 0, None, 0, 0,
         tmp, 64, 0, 0, precision_code(mode), stream())
    call("prx_k_rrdb_sum2x2", tmp, out, h, w, 64, stream())
    sync()
    assert only_slice_written(tmp, H * W, 0, 64) and only_slice_written(out, h * w, 0, 64)
    check("up backward 10x14 -> 5x7", nchw(out[:h * w].cpu().double(), h, w), exact, yard, mode)


def test_leaky_relu_derivative_zero_takes_the_small_slope():
    """an activation slice of exact zeros, a one-hot centre weight: the data gradient is exactly torch's own (0.2 g: `x > 0` gets 1), bit for bit"""
    H, W, P = 5, 7, 35
    wt = torch.zeros(32, 64, 3, 3)
    for c in range(32):
        wt[c, c, 1, 1] = 1.0
    x = torch.zeros(1, 32, H, W, requires_grad=True)
    gsl = torch.arange(P * 32, dtype=torch.float32).reshape(P, 32) / 64 - 5
    F.leaky_relu(x, 0.2).backward(nchw(gsl, H, W))
    for mode, a0 in (("f32", 0.0), ("f32", -0.0), ("f32", 1e-30), ("fp16", 0.0)):
        G = nanbuf(P, 192, torch.float32)
        put(G, P, 0, torch.zeros(P, 64))
        put(G, P, 64, gsl)
        A = nanbuf(P, 192, tdt(mode))
        put(A, P, 64, torch.full((P, 32), a0))
        call("prx_k_rrdb_conv", 1, G, 192, 64, A, 192, 64, wt.to(DEV), None, 64, 32, H, W, 0, 0, 1.0, 1.0, None, 0, None, 0, None, 0, 0, G, 192, 0, 1,
             precision_code(mode), stream())
        sync()
        want = nhwc(x.grad) if a0 <= 0 else gsl        # torch's own derivative at zero; a positive activation passes g
        got = G[:P, :32].cpu()
        if mode == "fp16":
            want = want.half().float()
        assert torch.equal(got, want), (mode, a0)
        assert bool((G[:P, 32:64] == 0).all())


# ------------------------------------------------------------------------------------------------ the edge convolutions
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hw", SIZES)
def test_conv_first_and_its_backward(hw, mode):
    h, w = hw
    P = h * w
    g = gen(3 + h)
    T = tdt(mode)
    z = torch.rand(1, 3, h, w, generator=g, dtype=torch.float64)
    wt, b = make_w(64, 3, g)
    exact = F.conv2d(z, wt, b, padding=1)
    yard = R.rel_l2(F.conv2d(z.float(), wt.float(), b.float(), padding=1), exact) if mode == "f32" else \
        R.rel_l2(F.conv2d(R.q16(z), R.q16(wt), b, padding=1), exact)
    out, of = nanbuf(P, 192, T), nanbuf(P, 64, torch.float32)
    wd, bd = wt.float().to(DEV).contiguous(), b.float().to(DEV)
    call("prx_k_rrdb_conv_first", z[0].float().to(DEV).contiguous(), wd, bd, h, w, out, 192, of, precision_code(mode), stream())
    sync()
    assert only_slice_written(out, P, 0, 64) and only_slice_written(of, P, 0, 64)
    check(f"conv_first {h}x{w}", nchw(out[:P, :64].cpu().double(), h, w), exact, yard, mode)
    assert torch.equal(out[:P, :64], of[:P].to(T))
    check(f"conv_first {h}x{w} f32copy", nchw(of[:P].cpu().double(), h, w), exact, yard, mode)
    # the backward sums two gradient streams (the trunk's and the feat + body skip's); it is fp32 in both modes
    g1 = torch.randn(1, 64, h, w, generator=g, dtype=torch.float64)
    g2 = torch.randn(1, 64, h, w, generator=g, dtype=torch.float64)
    ex = F.conv_transpose2d(g1 + g2, wt, padding=1)
    yb = R.rel_l2(F.conv_transpose2d((g1 + g2).float(), wt.float(), padding=1), ex)
    G1, G2 = nanbuf(P, 192, torch.float32), nanbuf(P, 64, torch.float32)
    put(G1, P, 0, nhwc(g1))
    put(G2, P, 0, nhwc(g2))
    dz = torch.full((3 * P + 5,), NAN, device=DEV)
    call("prx_k_rrdb_conv_first_bwd", G1, 192, G2, 64, wd, h, w, dz, stream())
    sync()
    assert bool(torch.isnan(dz[3 * P:]).all())
    check(f"conv_first backward {h}x{w}", dz[:3 * P].cpu().double().reshape(1, 3, h, w), ex, yb, "f32")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hw", SIZES)
def test_conv_last_forward_and_clamp(hw, mode):
    H, W = hw
    P = H * W
    g = gen(5 + H)
    T = tdt(mode)
    x = torch.randn(1, 64, H, W, generator=g, dtype=torch.float64)
    wt, b = make_w(3, 64, g)
    b = b + 0.5
    exact = F.conv2d(x, wt, b, padding=1)
    assert 0.05 < float(((exact < 0) | (exact > 1)).double().mean()) < 0.95        # both sides of the clamp occur
    yard = R.rel_l2(F.conv2d(x.float(), wt.float(), b.float(), padding=1), exact) if mode == "f32" else \
        R.rel_l2(F.conv2d(R.q16(x), R.q16(wt), b, padding=1), exact)
    xin = nanbuf(P, 64, T)
    put(xin, P, 0, nhwc(x))
    wd, bd = wt.float().to(DEV).contiguous(), b.float().to(DEV)
    for clamp in (0, 1):
        img = torch.full((3 * P + 5,), NAN, device=DEV)
        raw = torch.full((3 * P + 5,), NAN, device=DEV)
        call("prx_k_rrdb_conv_last", xin, wd, bd, H, W, clamp, img, raw, precision_code(mode), stream())
        sync()
        assert bool(torch.isnan(img[3 * P:]).all()) and bool(torch.isnan(raw[3 * P:]).all())
        check(f"conv_last {H}x{W} raw", raw[:3 * P].cpu().double().reshape(1, 3, H, W), exact, yard, mode)
        want = raw[:3 * P].clamp(0, 1) if clamp else raw[:3 * P]
        assert torch.equal(img[:3 * P], want)


@pytest.mark.parametrize("hw", SIZES)
def test_conv_last_backward_clamp_rule(hw):
    """hand-placed pre-clamp values at exactly 0 and 1, just inside and just outside, far out and mid-range, each met by upstream
    gradients of both signs and zero"""
    H, W = hw
    P = H * W
    g = gen(8 + H)
    vals = torch.tensor([0.0, 1.0, 1e-6, -1e-6, 1.0 - 1e-6, 1.0 + 1e-6, 0.5, -3.0, 4.0, -0.0], dtype=torch.float32)
    gs = torch.tensor([1.5, -0.75, 0.0], dtype=torch.float32)
    idx = torch.arange(3 * P)
    raw = vals[idx % len(vals)].reshape(1, 3, H, W)
    gi = (gs[(idx // len(vals)) % 3] * (1 + 0.01 * torch.randn(3 * P, generator=g))).reshape(1, 3, H, W)
    wt, _ = make_w(3, 64, g)
    wd = wt.float().to(DEV).contiguous()
    for clamp in (1, 0):
        gm = R.clamp_rule(gi.double(), raw.double()) if clamp else gi.double()
        ex = F.conv_transpose2d(gm, wt, padding=1)
        yb = R.rel_l2(F.conv_transpose2d(gm.float(), wt.float(), padding=1), ex)
        out = nanbuf(P, 64, torch.float32)
        call("prx_k_rrdb_conv_last_bwd", gi[0].contiguous().to(DEV), raw[0].contiguous().to(DEV), wd, H, W, clamp, out, stream())
        sync()
        assert only_slice_written(out, P, 0, 64)
        check(f"conv_last backward {H}x{W} clamp{clamp}", nchw(out[:P].cpu().double(), H, W), ex, yb, "f32")
    # the rule itself, isolated by a one-hot centre weight: bit for bit
    w1 = torch.zeros(3, 64, 3, 3)
    for c in range(3):
        w1[c, c, 1, 1] = 1.0
    out = nanbuf(P, 64, torch.float32)
    call("prx_k_rrdb_conv_last_bwd", gi[0].contiguous().to(DEV), raw[0].contiguous().to(DEV), w1.to(DEV), H, W, 1, out, stream())
    sync()
    assert torch.equal(out[:P, :3].cpu(), nhwc(R.clamp_rule(gi, raw)))


def test_refusals_by_name():
    G = nanbuf(35, 192, torch.float32)
    w = torch.zeros(32, 64, 3, 3, device=DEV)
    with pytest.raises(PrxError, match="bf16"):
        call("prx_k_rrdb_conv", 0, G, 192, 0, None, 0, 0, w, None, 64, 32, 5, 7, 0, 0, 1.0, 1.0, None, 0, None, 0, G, 192, 64, None, 0, 0, 0, 0, stream())
    with pytest.raises(PrxError, match="Cin"):
        call("prx_k_rrdb_conv", 0, G, 192, 0, None, 0, 0, w, None, 48, 32, 5, 7, 0, 0, 1.0, 1.0, None, 0, None, 0, G, 192, 64, None, 0, 0, 0, 1, stream())
