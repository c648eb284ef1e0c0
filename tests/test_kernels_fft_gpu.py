"""Kernel-level float64 tests (GPU) of the fft drawer, csrc/fft_drawer.hip: `fft_pack_kernel`, `fft_moments_kernel` +
`fft_moments_final_kernel`, `fft_tail_fwd_kernel`, `fft_tail_bwd_gy_kernel`, `fft_tail_bwd_dx_kernel`, `fft_unpack_kernel`, each through
`prx_k_fft_*` -> the host launcher `prx_fft_drawer_synth` / `_backward` themselves call (csrc/fft_drawer.h); the drawer's tables through
`prx_fft_drawer_table`; its four exact-f32 GEMM calls replayed through `prx_k_gemm` at the drawer's own strides and offsets; and the
whole spectrum -> image map and d/d(spectrum) through ops.fft_synth.

Method (helpers and the rules R1 / R2 of tests/test_kernels_runner_gpu.py and tests/test_kernels_plugins_gpu.py, imported): inputs are
drawn on the CPU from seeded generators, outputs are pre-filled with NaN and carry spare rows that must come back untouched, references
are plain torch in FLOAT64 on the fp32 inputs, written from the expressions of the header comment of fft_drawer.hip (restated below,
nothing imported from oracle/), with autograd for the backward kernels.  Canvases are (W, H).

Gates, none tuned against a kernel's output:
* tables: |t - ref64| <= 2^-24 |ref64| + TAB * magnitude, TAB = 64 * 2^-53 for the double cos / sin / pow / sqrt of the builder and of this
  reference (argument 2 pi k / W: two roundings on at most 2 pi, the function itself an ulp, two products; pow carries the relative
  error of |f| decay-fold: under 16 units of 2^-53 a side); padding exact zeros, A1T / T2T bit-equal transposes.
* pack: R1, bit-equal to the single fp32 product; padding exact zeros.
* unpack: R2, k = 2 (one sum, one product) on (|p0| + |p1|) |scale|; <pack(p), D> == <p, unpack(D)> in float64 within
  (1 + 2) * 2^-24 * sum |p| A (pack's one rounding, unpack's two).
* moments: the float -> double conversions and the products of two floats are exact in double, only the additions round:
  |acc - exact| <= depth * 2^-53 * sum |terms|, the exact sum taken with math.fsum; depth counted in `mom_depth`.
* tail: fed FLOAT64-computed sums; R2 with the chain counted beside each use, plus EXPF_REL(max |z|) for the sigmoid's `__expf`.
* the f32 engine: |c - ref64| <= (K + 1 + split-K parts) * 2^-24 * sum |a| |b| per element.
* whole map: image max-abs and gradient rel-L2 against the float64 explicit DFT; the gate is 4 x the error of an fp32 restatement of the
  same explicit DFT (the same matrix products in torch fp32, twiddles rounded from float64) against the same float64 reference --
  reference against reference, the worst of four seeds per case --, never above 5e-6 (image) and 2e-5 (gradient).  The kernels run on
  all four seeds.

Measured (`python -m pytest -s` prints every figure as an `[fft-fig]` line: name, kernel error, gate; no gate was moved after a run).
Worst kernel error / gate per family on an MI355X (on the CPU emulation in brackets): tables 0.98 (0.98: the scale table at 64 x 33, a half
ulp of fp32 among 2112 entries); pack bit-equal everywhere; unpack 0.91 (0.91) at the small canvases and 0.99 one trip past the grid cap,
both at k = 2; pack / unpack adjointness 0.06 (0.06); moments 0.095 (0.095); tail forward 0.73 (0.73), past the cap 0.71; gy pass 0.26
(0.25), past the cap 0.42; dx pass 0.36 (0.36), past the cap 0.24; the f32 engine at the drawer's geometry 0.23 (0.23); whole map: image
0.35 (0.34) and gradient 0.62 (0.47) of their gates, i.e. the kernels' error was 0.48 .. 1.41 (0.37 .. 1.36) x the fp32 yardstick's
worst-of-four on the image and 0.03 .. 2.46 (0.02 .. 1.87) x on the gradient, against the factor 4 (the yardstick is torch's fp32 matmul
on the host that runs the test, so the two columns do not share it).  All 198 tests of the file take 4.5 s on the device, the largest (tail forward + gy past the cap) 1.9 s.

Found and fixed: `fft_tail_bwd_gy_kernel` took 1 - s by subtraction, which leaves it with the absolute rounding 2^-24 s of s.  A DC-heavy
spectrum (test_whole_map_dc_heavy_spectrum[0.5]: every z between 4.5 and 17) came out at a gradient rel-L2 of 4.5e-5 -- exactly the
fp32 yardstick's 4.6e-5, and over the 2e-5 cap; the kernel now takes 1 - s = e s above z = 0 and reaches 3.9e-6 there.  The gy bound
below is the tighter one that goes with that (it fails on the subtraction in 27 of the 40 gy cases).  The other six kernels compile to
the instructions they had before.  The product's two Python defects (image init on an odd width, a stale backward) have their tests in
tests/test_host_logic.py and here (test_drawer_starts_from_an_image_on_an_odd_width_canvas_hip_path, test_a_stale_backward_is_refused).

Mutation check on the emulated kernels (sources and tools/hipemu copied aside, one line changed, the library rebuilt, every check of this
file below the grid cap run one by one -- 194 checks; the unchanged copy passes all, each of the twelve mutants is caught; failing checks
counted in brackets):
g_v = 2 at the Nyquist column of an even width: test_tables and all four test_whole_map settings at 2x2, 2x3, 8x6, 64x33, both
test_tables_at_other_settings, both DC-heavy cases, the gradient check of the stale-backward test (25); `W % 2 == 0` dropped: the same
two at the odd widths 3x2, 5x7, 13x4, 45x32, test_tables_at_other_settings, every surplus-column and image-init case (28); the sign of
`-p[1]` in pack: test_pack and test_unpack (its adjointness) at every canvas, test_whole_map at every canvas with H > 2 and every later
whole-map test (48); `p0[1] - p1[0]` -> `+`: test_unpack at every canvas, the same whole-map tests (40); `(n - 1)` -> `n` in fft_std:
every tail forward, gy and dx case and every whole-map test (145); `st.mean` dropped: every test_tail_bwd_dx case and every whole-map
test (65); the `h < H` guard removed: test_tail_bwd_dx at the six canvases with H % 4 != 0 (18; the whole map cannot see it: T2T's
padding columns are zero); `v < Wh` removed in unpack: test_unpack at the four odd widths, test_whole_map and the surplus-column test at
3x2, the image-init test at 7x5 (10); `Wf` -> `Wh` in the pack index: test_pack, test_unpack, test_whole_map, the surplus-column and
image-init tests at every odd width (30); the final kernel's `b += 256` -> `b += 255`: test_moments at 262143, 262144, 262145 and
524289 elements, with and without y, and the offset case at 262145 (9); `m[3 * c + d]` transposed in the gy pass: every
test_tail_bwd_gy case and every whole-map test (81); `1 - s` by subtraction again: 27 of the 40 test_tail_bwd_gy cases and
test_whole_map_dc_heavy_spectrum[0.5] (28).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from pixray_amd import _lib, ops
from pixray_amd._lib import GemmArgs, PrxError, call

import test_kernels_half_gpu as th  # noqa: F401
from test_kernels_half_gpu import guarded, untouched, bits, rel_l2, EXPF_REL
from test_kernels_runner_gpu import stream, sync, flat, check_f32, same_bits
from test_kernels_plugins_gpu import f32v, all_nan

DEV = "cuda"          # tests/test_emu_cpu.py switches this (and the helper modules') to "cpu" for the emulated kernels
EPS32 = 2.0 ** -24
EPS64 = 2.0 ** -53
TAB = 64 * EPS64      # the double library functions of the table builder and of this reference (module docstring)
NAN = float("nan")
F32 = torch.float32
F64 = torch.float64
FIGURES = {}          # name -> (worst kernel error, its gate), printed by the tests (`pytest -s`)
CAP = 8192 * 256      # elements of a full grid of the elementwise kernels: one more and the grid-stride loop takes a second trip
TABLES = {"scale": 0, "A1": 1, "A1T": 2, "T2": 3, "T2T": 4, "cm": 5}
SMALL = [(2, 2), (3, 2), (2, 3), (5, 7), (8, 6), (13, 4), (45, 32), (64, 33)]
small = pytest.mark.parametrize("W,H", SMALL)


def dev(t):
    return t.to(DEV)


def fig(name, err, gate):
    err, gate = float(err), float(gate)
    old = FIGURES.get(name)
    if old is None or err / max(gate, 1e-300) >= old[0] / max(old[1], 1e-300):
        FIGURES[name] = (err, gate)
    print(f"[fft-fig] {name} {err:.3e} {gate:.3e}")


def r2(name, out, ref64, tol):
    """elementwise |out - ref64| <= tol (a tensor): prints the element that comes closest to its gate, then asserts every element"""
    out, ref64 = out.detach().double().cpu(), ref64.detach().double().cpu()
    tol = tol.detach().double().cpu().expand_as(ref64)
    err = (out - ref64).abs()
    ratio = (err / tol.clamp_min(1e-300)).nan_to_num(nan=float("inf")).flatten()
    i = int(ratio.argmax())
    fig(name, err.flatten()[i], tol.flatten()[i])
    check_f32(out, ref64, 1, tol / EPS32)


class Geom:
    """the padded geometry of a W x H canvas (fft_geom of csrc/fft_drawer.h, restated)"""

    def __init__(self, W, H):
        up4 = lambda v: (v + 3) & ~3
        self.W, self.H = W, H
        self.Wh = W // 2 + 1
        self.Wf = W // 2 + (2 if W % 2 else 1)
        self.HP, self.HP2, self.WP, self.K1p = up4(H), up4(2 * H), up4(W), up4(2 * self.Wh)


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ================================================================================================ 1. the tables
def tables64(W, H, decay, colors):
    """the header comment's tables in float64, padded as the drawer pads them:
    scale[u][v] = sqrt(W H) / max(|f|, 1 / max(W, H)) ^ decay;  A1[w][(v, 0)] = g_v cos th / sqrt(HW), A1[w][(v, 1)] = -g_v sin th / sqrt(HW),
    th = 2 pi v w / W, g_v = 1 (v = 0, and v = W / 2 when W is even) else 2;  T2 = [cos ph | sin ph], ph = 2 pi u h / H;  A1T, T2T their
    transposes;  cm[c][d] = M[d][c] / (largest column norm of M), M = colour correlation / (colors, 1, 1)"""
    g = Geom(W, H)
    u = torch.arange(H, dtype=F64)
    v = torch.arange(g.Wh, dtype=F64)
    fy = torch.where(u < (H + 1) // 2, u, u - H) / H
    fx = torch.where(v < (W + 1) // 2, v, v - W) / W
    f = torch.sqrt(fx[None] ** 2 + fy[:, None] ** 2).clamp_min(1.0 / max(W, H))
    scale = math.sqrt(W * H) / f ** decay
    gv = torch.full((g.Wh,), 2.0, dtype=F64)
    gv[0] = 1.0
    if W % 2 == 0:
        gv[W // 2] = 1.0
    nrm = 1.0 / math.sqrt(W * H)
    kw = torch.outer(torch.arange(W), torch.arange(g.Wh)) % W                      # the angle reduced exactly, in integers
    thw = 2 * math.pi * kw.double() / W
    A1 = torch.zeros(W, g.K1p, dtype=F64)
    A1[:, 0:2 * g.Wh:2] = gv * torch.cos(thw) * nrm
    A1[:, 1:2 * g.Wh:2] = -gv * torch.sin(thw) * nrm
    ph = 2 * math.pi * (torch.outer(torch.arange(H), torch.arange(H)) % H).double() / H
    T2 = torch.zeros(H, g.HP2, dtype=F64)
    T2[:, :H] = torch.cos(ph)
    T2[:, H:2 * H] = torch.sin(ph)
    A1T = torch.zeros(g.K1p, g.WP, dtype=F64)
    A1T[:, :W] = A1.T
    T2T = torch.zeros(g.HP2, g.HP, dtype=F64)
    T2T[:, :H] = T2.T
    M = torch.tensor([[0.26, 0.09, 0.02], [0.27, 0.00, -0.05], [0.27, -0.09, 0.03]], dtype=F64) / torch.tensor([colors, 1.0, 1.0], dtype=F64)
    cm = (M / M.norm(dim=0).max()).T.contiguous()
    mag = {"scale": scale, "A1": torch.tensor(2 * nrm, dtype=F64), "A1T": torch.tensor(2 * nrm, dtype=F64), "T2": torch.tensor(1.0, dtype=F64),
           "T2T": torch.tensor(1.0, dtype=F64), "cm": torch.tensor(1.0, dtype=F64)}
    return {"scale": scale, "A1": A1, "A1T": A1T, "T2": T2, "T2T": T2T, "cm": cm}, mag, gv


def table(handle, name, rows, cols):
    full, win = guarded(rows, cols, F32)
    call("prx_fft_drawer_table", handle.h, TABLES[name], full, rows * cols, stream())
    sync()
    assert untouched(full, rows, cols)
    return win.clone()


def table_shapes(g):
    return {"scale": (g.H, g.Wh), "A1": (g.W, g.K1p), "A1T": (g.K1p, g.WP), "T2": (g.H, g.HP2), "T2T": (g.HP2, g.HP), "cm": (3, 3)}


def all_tables(handle, g):
    return {name: table(handle, name, *shape) for name, shape in table_shapes(g).items()}


def check_tables(W, H, decay=1.5, colors=1.5):
    g = Geom(W, H)
    handle = ops.FftDrawerHandle(W, H, decay=decay, colors=colors)
    assert handle.freq_columns == g.Wf
    got = all_tables(handle, g)
    ref, mag, gv = tables64(W, H, f32v(decay), f32v(colors))
    for name, t in got.items():
        t = t.cpu()
        # each entry is the fp32 rounding (2^-24 |ref|) of its float64 definition, TAB for the double functions on both sides
        r2(f"tab/{W}x{H}-d{decay}-c{colors}/{name}", t, ref[name], EPS32 * ref[name].abs() + TAB * mag[name])
        assert bool((t[ref[name] == 0] == 0).all()), f"{name}: an entry that is zero by definition"
    A1, A1T, T2, T2T = (got[k].cpu() for k in ("A1", "A1T", "T2", "T2T"))
    # g_v read off row w = 0 (th = 0: the entry is g_v / sqrt(HW), one rounding): 1 at v = 0 and at v = W / 2 of an even W only
    gv_got = A1[0, 0:2 * g.Wh:2].double() * math.sqrt(W * H)
    assert bool(((gv_got - gv).abs() <= 4 * EPS32).all()), ("g_v", gv_got, gv)
    assert bool((A1[:, 2 * g.Wh:] == 0).all()) and bool((A1T[2 * g.Wh:] == 0).all()) and bool((A1T[:, W:] == 0).all()), "A1 / A1T padding"
    assert bool((T2[:, 2 * H:] == 0).all()) and bool((T2T[2 * H:] == 0).all()) and bool((T2T[:, H:] == 0).all()), "T2 / T2T padding"
    same_bits(A1T[:, :W].contiguous(), A1.T.contiguous())
    same_bits(T2T[:, :H].contiguous(), T2.T.contiguous())
    return got


@small
def test_tables(W, H):
    check_tables(W, H)


@pytest.mark.parametrize("decay,colors", [(0.0, 1.0), (3.0, 2.0)])
def test_tables_at_other_settings(decay, colors):
    """scale at decay 0 (all sqrt(W H)), 1.5 (above) and 3; the colour matrix at colours 1.0, 1.5 (above) and 2.0"""
    got = check_tables(13, 4, decay, colors)
    check_tables(8, 6, decay, colors)
    if decay == 0.0:
        assert bool((got["scale"].cpu() == f32v(math.sqrt(13 * 4))).all())


# ================================================================================================ 2. pack (R1), 3. unpack
def pack_ref(p, scale, g):
    """Bt1[(c, part', u)][(v, part)]: part' = 0: (re, im) * scale[u, v]; part' = 1: (-im, re) * scale[u, v]; the single fp32 product"""
    H, Wh = g.H, g.Wh
    bt = torch.zeros(3, g.HP2, g.K1p, dtype=F32)
    re, im = p[:, :, :Wh, 0] * scale, p[:, :, :Wh, 1] * scale
    bt[:, :H, 0:2 * Wh:2], bt[:, :H, 1:2 * Wh:2] = re, im
    bt[:, H:2 * H, 0:2 * Wh:2], bt[:, H:2 * H, 1:2 * Wh:2] = -im, re
    return bt.reshape(3 * g.HP2, g.K1p)


def run_pack(p, scale, g):
    full, win = guarded(3 * g.HP2, g.K1p, F32)
    call("prx_k_fft_pack", dev(p), dev(scale), full, g.W, g.H, stream())
    sync()
    assert untouched(full, 3 * g.HP2, g.K1p)
    return win.cpu()


def pack_inputs(W, H):
    g = Geom(W, H)
    p = rnd(W * 100 + H, 3, H, g.Wf, 2)
    scale = 0.5 + torch.rand(H, g.Wh, generator=torch.Generator().manual_seed(W + H))
    return g, p, scale


def check_pack(W, H):
    g, p, scale = pack_inputs(W, H)
    got = run_pack(p, scale, g)
    same_bits(got, pack_ref(p, scale, g))                               # R1, the zero padding rows k >= 2 H and columns >= 2 Wh included
    if W % 2:                                                           # the surplus column is never read
        q = p.clone()
        q[:, :, g.Wf - 1, :] = NAN
        again = run_pack(q, scale, g)
        assert bool(torch.isfinite(again).all())
        same_bits(again, got)
    fig(f"pack/{W}x{H}", 0.0, 0.0)


@small
def test_pack(W, H):
    check_pack(W, H)


def run_unpack(D, scale, g):
    full, win = guarded(3 * g.H, g.Wf * 2, F32)
    call("prx_k_fft_unpack", dev(D), dev(scale), full, g.W, g.H, stream())
    sync()
    assert untouched(full, 3 * g.H, g.Wf * 2)
    return win.cpu().reshape(3, g.H, g.Wf, 2)


def unpack_inputs(W, H):
    """dP with NaN planted in its padding rows k >= 2 H and columns >= 2 Wh"""
    g, p, scale = pack_inputs(W, H)
    D = rnd(W * 7 + H, 3, g.HP2, g.K1p)
    D[:, 2 * H:, :] = NAN
    D[:, :, 2 * g.Wh:] = NAN
    return g, p, scale, D


def unpack_ref(D, scale, g):
    """gre = (p0[0] + p1[1]) * s, gim = (p0[1] - p1[0]) * s, p0 / p1 the part' = 0 / 1 rows: float64, and the R2 terms A"""
    H, Wh = g.H, g.Wh
    D, s = D.double(), scale.double()
    p0, p1 = D[:, :H, :2 * Wh].reshape(3, H, Wh, 2), D[:, H:2 * H, :2 * Wh].reshape(3, H, Wh, 2)
    ref = torch.zeros(3, H, g.Wf, 2, dtype=F64)
    A = torch.zeros(3, H, g.Wf, 2, dtype=F64)
    ref[:, :, :Wh, 0] = (p0[..., 0] + p1[..., 1]) * s
    ref[:, :, :Wh, 1] = (p0[..., 1] - p1[..., 0]) * s
    A[:, :, :Wh, 0] = (p0[..., 0].abs() + p1[..., 1].abs()) * s
    A[:, :, :Wh, 1] = (p0[..., 1].abs() + p1[..., 0].abs()) * s
    return ref, A


def check_unpack(W, H):
    g, p, scale, D = unpack_inputs(W, H)
    got = run_unpack(D, scale, g)
    ref, A = unpack_ref(D, scale, g)
    r2(f"unpack/{W}x{H}", got, ref, 2 * EPS32 * A)                      # one sum, one product: k = 2
    assert bool(torch.isfinite(got).all()), "NaN of the padding of dP came through"
    if W % 2:
        assert bool((got[:, :, g.Wf - 1, :] == 0).all()), "the surplus column's gradient is exactly zero"
    # adjointness with pack in float64: pack rounds each product once, unpack its sum and its product
    packed = run_pack(p, scale, g).double().reshape(3, g.HP2, g.K1p)
    lhs = float((packed * D.double().nan_to_num(nan=0.0)).sum())        # pack's padding is exact zeros
    rhs = float((p.double() * got.double()).sum())
    gate = 3 * EPS32 * float((p.double().abs() * A).sum())
    fig(f"unpack-adjoint/{W}x{H}", abs(lhs - rhs), gate)
    assert abs(lhs - rhs) <= gate, (lhs, rhs, gate)


@small
def test_unpack(W, H):
    check_unpack(W, H)


# ================================================================================================ 4. moments
MOM_N = [12, 255, 256, 257, 262143, 262144, 262145, 2 * 262144 + 1]


def mom_blocks(n):
    return min((n + 255) // 256, 1024)


def mom_depth(n):
    """additions a term goes through: its thread's grid-stride trips, the wave butterfly (6), the four waves (2); then the final
    kernel's strided sum over the block partials (ceil(blocks / 256)), its butterfly (6) and its four waves (2)"""
    mb = mom_blocks(n)
    trips = -(-n // (mb * 256))
    return trips + 6 + 2 + -(-mb // 256) + 6 + 2


def run_moments(x, y, n):
    mb = mom_blocks(n)
    pfull, part = flat(3 * mb, F64)
    afull, acc = flat(3, F64)
    call("prx_k_fft_moments", x, y, n, pfull, afull, stream())
    sync()
    assert untouched(pfull, 1, 3 * mb), "`part` beyond 3 * blocks was written"
    assert untouched(afull, 1, 3)
    return acc.cpu(), part.cpu()


def check_moments(n, with_y, offset=0.0):
    x = offset + rnd(n, n)
    y = rnd(n + 1, n) if with_y else None
    xd, yd = dev(x), None if y is None else dev(y)
    acc, part = run_moments(xd, yd, n)
    acc2, part2 = run_moments(xd, yd, n)
    assert torch.equal(bits64(acc), bits64(acc2)) and torch.equal(bits64(part), bits64(part2)), "two runs differ"
    x64 = x.double()
    terms = [x64, x64 * x64] + ([x64 * y.double()] if with_y else [])   # exact in double: 24- and 48-bit significands
    name = f"mom/{n}{'-y' if with_y else ''}{'-offset' if offset else ''}"
    for k, t in enumerate(terms):
        exact = math.fsum(t.tolist())
        gate = mom_depth(n) * EPS64 * float(t.abs().sum())
        fig(f"{name}/s{k}", abs(float(acc[k]) - exact), gate)
        assert abs(float(acc[k]) - exact) <= gate, (name, k, float(acc[k]), exact, gate)
    if not with_y:
        assert float(acc[2]) == 0.0 and bool((part.reshape(-1, 3)[:, 2] == 0).all()), "without y the third sum is exactly 0"


def bits64(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("with_y", [False, True], ids=["x", "xy"])
@pytest.mark.parametrize("n", MOM_N)
def test_moments(n, with_y):
    check_moments(n, with_y)


@pytest.mark.parametrize("n", [257, 262145])
def test_moments_of_a_mean_far_from_zero(n):
    """1e3 + noise: the sums themselves stay exact to the same gate (the cancellation is fft_std's, checked with the tail kernels)"""
    check_moments(n, True, offset=1e3)


# ================================================================================================ 5. the tail, forward and backward pair
def sums64(x, y=None):
    x = x.double().flatten()
    return torch.tensor([math.fsum(x.tolist()), math.fsum((x * x).tolist()), 0.0 if y is None else math.fsum((x * y.double().flatten()).tolist())],
                        dtype=F64)


def sigma_extra(x):
    """fft_std takes var = (acc[1] - n mean^2) / (n - 1) in double: the subtraction cancels, the relative error of var is about
    4 * 2^-53 * acc[1] / ((n - 1) var) and sigma's half of it -- in units of 2^-24, to be added to a counted k"""
    x = x.double()
    return 2 * EPS64 * float((x * x).sum() / ((x.numel() - 1) * x.var())) / EPS32


def tail_inputs(W, H, contrast, mean_sigmas, zmax, seed=0):
    """x [3][P] = noise + mean_sigmas standard deviations; a random 3 x 3 colour matrix (not symmetric: a transposed index shows),
    scaled so that the largest |z| is zmax"""
    P = W * H
    x = (0.3 * (rnd(seed + W * 31 + H, 3, P) + mean_sigmas)).contiguous()
    x64 = x.double()
    a = f32v(contrast) / float(x64.std())
    R = rnd(seed + 5, 3, 3)
    z = torch.einsum("cp,cd->dp", a * x64, R.double())
    cm = (R * (zmax / float(z.abs().max()))).contiguous()
    return x, cm


def tail_fwd_ref(x, cm, contrast):
    """a = contrast / std (unbiased, over all 3 H W values), y = a x, z_d = sum_c y_c M[c][d], rgb = sigmoid(z); float64.
    Returns rgb, z, A_z = sum_c |a x_c M[c][d]|"""
    x64, m = x.double(), cm.double()
    a = contrast / x64.std()
    z = torch.einsum("cp,cd->dp", a * x64, m)
    Az = torch.einsum("cp,cd->dp", (a * x64).abs(), m.abs())
    return torch.sigmoid(z), z, Az


def s_error(s, z, Az, kz):
    """the fp32 sigmoid's absolute error.  z carries kz roundings on A_z; e = __expf(-z) a relative EXPF_REL(max |z|); s = 1 / (1 + e)
    moves by s (1 - s) per unit of either; the addition and the division round s itself (2)"""
    return s * (1 - s) * (kz * EPS32 * Az + EXPF_REL(float(z.abs().max()))) + 2 * EPS32 * s


def check_tail_fwd(W, H, contrast, mean_sigmas, zmax, name=None):
    P = W * H
    x, cm = tail_inputs(W, H, contrast, mean_sigmas, zmax)
    c32 = f32v(contrast)
    full, win = guarded(3, P, F32)
    call("prx_k_fft_tail_fwd", dev(x), dev(sums64(x)), c32, dev(cm), full, W, H, stream())
    sync()
    assert untouched(full, 3, P)
    s, z, Az = tail_fwd_ref(x, cm, c32)
    # z: sigma (the conversion of the double root: 1), a = contrast / sigma (1), y = a x (1), the product with m (1), two additions (2):
    # k = 6 on A_z, + the cancellation of fft_std
    kz = 6 + sigma_extra(x)
    r2(name or f"tail-fwd/{W}x{H}-c{contrast}-m{mean_sigmas}-z{zmax}", win, s, s_error(s, z, Az, kz))
    assert bool(torch.isfinite(win).all())


def check_tail_gy(W, H, contrast, mean_sigmas, zmax, name=None):
    P = W * H
    x, cm = tail_inputs(W, H, contrast, mean_sigmas, zmax)
    g = rnd(W * 3 + H, 3, P)
    c32 = f32v(contrast)
    full, win = guarded(3, P, F32)
    call("prx_k_fft_tail_bwd_gy", dev(x), dev(g), dev(sums64(x)), c32, dev(cm), full, W, H, stream())
    sync()
    assert untouched(full, 3, P)
    x64, m = x.double(), cm.double()
    y = (c32 / x64.std() * x64).requires_grad_(True)
    (gy64,) = torch.autograd.grad((torch.sigmoid(torch.einsum("cp,cd->dp", y, m)) * g.double()).sum(), y)
    s, z, Az = tail_fwd_ref(x, cm, c32)
    kz = 6 + sigma_extra(x)
    es = s_error(s, z, Az, kz)
    # gz = g s (1 - s).  z <= 0 (1 - s >= 1 / 2 is taken by subtraction): s carries es, 1 - s inherits it absolutely and rounds once
    # more (2^-24 (1 - s)); two products: |g| (|1 - 2 s| es + 3 * 2^-24 s (1 - s)).  z > 0 (1 - s is taken as e s, e = __expf(-z), so
    # that it keeps its RELATIVE accuracy where s -> 1: before this file the kernel subtracted there too, and 1 - s was left with the
    # absolute rounding 2^-24 s of s -- nothing of it at z = 17; test_whole_map_dc_heavy_spectrum found that): e carries the error of z
    # and EXPF_REL relatively (D), s carries es / s, three products: |g| s (1 - s) (D + 2 es / s + 3 * 2^-24).  Around z = 0 the
    # kernel's own z decides the branch: within its error D of zero the larger of the two bounds is taken.
    # gy_c = sum_d gz_d m[c][d]: three products, two additions: 5 * 2^-24 on sum |gz m|, + the errors of gz carried through |m|
    t = s * (1 - s)
    D = kz * EPS32 * Az + EXPF_REL(float(z.abs().max()))
    e_sub = (1 - 2 * s).abs() * es + 3 * EPS32 * t
    e_mul = t * (D + 2 * es / s + 3 * EPS32)
    egz = g.double().abs() * torch.where(z.abs() <= D, torch.maximum(e_sub, e_mul), torch.where(z > 0, e_mul, e_sub))
    tol = torch.einsum("dp,cd->cp", egz + 5 * EPS32 * (g.double() * t).abs(), m.abs())
    r2(name or f"tail-gy/{W}x{H}-c{contrast}-m{mean_sigmas}-z{zmax}", win, gy64, tol)
    assert bool(torch.isfinite(win).all())


def check_tail_dx(W, H, contrast, mean_sigmas, name=None):
    g = Geom(W, H)
    P = W * H
    x, _ = tail_inputs(W, H, contrast, mean_sigmas, 1.0)
    gy = rnd(W * 5 + H, 3, P)
    c32 = f32v(contrast)
    full, win = guarded(3 * W, g.HP, F32)
    call("prx_k_fft_tail_bwd_dx", dev(x), dev(gy), dev(sums64(x)), dev(sums64(gy, x)), c32, full, W, H, stream())
    sync()
    assert untouched(full, 3 * W, g.HP)
    got = win.cpu().reshape(3, W, g.HP)
    assert bool((got[:, :, H:] == 0).all()), "padding entries h >= H of dxT are exact zeros"
    xr = x.double().requires_grad_(True)
    (dx64,) = torch.autograd.grad((c32 * xr / xr.std() * gy.double()).sum(), xr)
    # dx = a gy - k (x - mean), k = a S / (sigma^2 (n - 1)).  a: sigma (1), the division (1); a gy: the product (1), the final
    # subtraction (1): 4 on |a gy|.  k: a (2) and sigma squared (2) enter a double expression, its conversion (1): 5; x - mean: mean's
    # conversion (1) and the subtraction (1), on |x| + |mean|; the product (1) and the final subtraction (1): 9 on |k| (|x| + |mean|).
    # k = 9 on the whole of A, + the cancellation of fft_std, which enters a once and k three times
    x64 = x.double()
    n = 3 * P
    a = c32 / float(x64.std())
    kk = a * float((gy.double() * x64).sum()) / (float(x64.var()) * (n - 1))
    A = abs(a) * gy.double().abs() + abs(kk) * (x64.abs() + abs(float(x64.mean())))
    tol = (9 + 3 * sigma_extra(x)) * EPS32 * A
    transposed = lambda t: t.reshape(3, H, W).permute(0, 2, 1)                    # the layout is dxT[c][w][h], row stride HP
    r2(name or f"tail-dx/{W}x{H}-c{contrast}-m{mean_sigmas}", got[:, :, :H], transposed(dx64), transposed(tol))


TAIL_SETTINGS = [(0.9, 0, 8.0), (0.1, 10, 8.0), (2.5, 100, 8.0), (0.9, 10, 3.0), (0.9, 0, 20.0)]     # contrast, mean / sigma, max |z| (20: saturated)
TAIL_IDS = ["c0.9-m0-z8", "c0.1-m10-z8", "c2.5-m100-z8", "c0.9-m10-z3", "c0.9-m0-z20-saturated"]


@pytest.mark.parametrize("contrast,mean_sigmas,zmax", TAIL_SETTINGS, ids=TAIL_IDS)
@small
def test_tail_fwd(W, H, contrast, mean_sigmas, zmax):
    check_tail_fwd(W, H, contrast, mean_sigmas, zmax)


@pytest.mark.parametrize("contrast,mean_sigmas,zmax", TAIL_SETTINGS, ids=TAIL_IDS)
@small
def test_tail_bwd_gy(W, H, contrast, mean_sigmas, zmax):
    check_tail_gy(W, H, contrast, mean_sigmas, zmax)


@pytest.mark.parametrize("contrast,mean_sigmas", [(0.9, 0), (0.1, 10), (2.5, 100)], ids=["c0.9-m0", "c0.1-m10", "c2.5-m100"])
@small
def test_tail_bwd_dx(W, H, contrast, mean_sigmas):
    check_tail_dx(W, H, contrast, mean_sigmas)


# ================================================================================================ 6. one trip past the grid cap
def test_pack_past_the_grid_cap():
    W, H = 836, 418
    g = Geom(W, H)
    assert 3 * g.HP2 * g.K1p > CAP >= 3 * Geom(W - 2, H - 1).HP2 * Geom(W - 2, H - 1).K1p
    check_pack(W, H)


def test_unpack_past_the_grid_cap():
    W, H = 1672, 836
    assert 3 * H * Geom(W, H).Wf > CAP >= 3 * (H - 1) * Geom(W - 2, H - 1).Wf
    check_unpack(W, H)


def test_tail_fwd_and_gy_past_the_grid_cap():
    W, H = 2049, 1024
    assert W * H > CAP >= (W - 1) * H
    check_tail_fwd(W, H, 0.9, 0, 8.0, name="cap/tail-fwd")
    check_tail_gy(W, H, 0.9, 0, 8.0, name="cap/tail-gy")


def test_tail_dx_past_the_grid_cap():
    W, H = 837, 836
    assert 3 * W * Geom(W, H).HP > CAP >= 3 * (W - 1) * Geom(W, H).HP
    check_tail_dx(W, H, 0.9, 10, name="cap/tail-dx")


# ================================================================================================ 7. the f32 engine at the drawer's geometry
def gemm_at(name, A, a_off, lda, B, b_off, ldb, M, N, K, out, c_off, ldc):
    """one exact-f32 product C[M][N] = A[M][K] Bt[N][K]^T through prx_k_gemm, at element offsets into flat device buffers, checked
    against float64 on the same fp32 operands; returns the float64 reference"""
    ga = GemmArgs()
    ga.f32 = 1
    ga.A = A.data_ptr() + 4 * a_off; ga.a_mode = 0; ga.lda = lda
    ga.B = B.data_ptr() + 4 * b_off; ga.ldb = ldb
    ga.M, ga.N, ga.K = M, N, K
    ga.alpha = 1.0
    ga.out_f32 = out.data_ptr() + 4 * c_off; ga.ldc_f32 = ldc
    ws = torch.empty(32 << 20, dtype=torch.uint8, device=DEV)
    plan = torch.zeros(9, dtype=torch.int32)
    call("prx_gemm_plan", None, ga, ws.numel(), 0, plan)
    splits = max(int(plan[3]), 1)
    before = out.clone()
    call("prx_k_gemm", ga, ws, ws.numel(), stream())
    sync()
    a = torch.as_strided(A.cpu().flatten(), (M, K), (lda, 1), a_off).double()
    b = torch.as_strided(B.cpu().flatten(), (N, K), (ldb, 1), b_off).double()
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    ref = a @ b.T
    got = torch.as_strided(out.cpu(), (M, N), (ldc, 1), c_off)
    # an fmaf chain of K terms (K roundings), the conversion / split-K additions: k = K + 1 + split-K parts on sum |a| |b|
    r2(name, got, ref, (K + 1 + splits) * EPS32 * (a.abs() @ b.abs().T))
    mask = torch.zeros(out.numel(), dtype=torch.bool)
    torch.as_strided(mask, (M, N), (ldc, 1), c_off).fill_(True)
    same = bits(out.cpu().flatten()) == bits(before.cpu().flatten())
    assert bool(same[~mask].all()), f"{name}: wrote outside its M x N window (columns N .. ldc - 1 or rows beyond M)"
    return ref


def check_engine(W, H):
    g = Geom(W, H)
    handle = ops.FftDrawerHandle(W, H)
    tabs = all_tables(handle, g)
    _, p, _ = pack_inputs(W, H)
    nanbuf = lambda n: torch.full((n + 64,), NAN, dtype=F32, device=DEV)
    bt1 = nanbuf(3 * g.HP2 * g.K1p)
    call("prx_k_fft_pack", dev(p), tabs["scale"].contiguous(), bt1, W, H, stream())
    sync()
    P = W * H
    tag = f"engine/{W}x{H}"
    # GEMM 1: C1[w][(c, part', u)], N == ldc
    c1 = nanbuf(W * 3 * g.HP2)
    gemm_at(tag + "/gemm1", tabs["A1"].contiguous(), 0, g.K1p, bt1, 0, g.K1p, W, 3 * g.HP2, g.K1p, c1, 0, 3 * g.HP2)
    # GEMM 2, per channel: B is the strided sub-matrix c1 + c * HP2 of row stride 3 * HP2
    x = nanbuf(3 * P)
    for c in range(3):
        gemm_at(f"{tag}/gemm2-c{c}", tabs["T2"].contiguous(), 0, g.HP2, c1, c * g.HP2, 3 * g.HP2, H, W, g.HP2, x, c * P, W)
    # GEMM 2', per channel: M = 2 H < HP2 rows and N = W < ldc = WP columns of dC1T
    dxT = torch.zeros(3, W, g.HP)
    dxT[:, :, :H] = rnd(W + H, 3, W, H)
    dxT = dev(dxT.flatten())
    dc1t = nanbuf(3 * g.HP2 * g.WP)
    for c in range(3):
        gemm_at(f"{tag}/gemm2T-c{c}", tabs["T2T"].contiguous(), 0, g.HP, dxT, c * W * g.HP, g.HP, 2 * H, W, g.HP, dc1t, c * g.HP2 * g.WP, g.WP)
    got = dc1t.cpu()
    clean = torch.where(torch.isnan(got), torch.zeros_like(got), got)   # the drawer's dC1T is zeroed once: padding rows and columns 0
    # GEMM 1': dBt1[n][(v, part)] = sum_w dC1T[n][w] A1T[(v, part)][w]
    dP = nanbuf(3 * g.HP2 * g.K1p)
    gemm_at(tag + "/gemm1T", dev(clean), 0, g.WP, tabs["A1T"].contiguous(), 0, g.WP, 3 * g.HP2, g.K1p, g.WP, dP, 0, g.K1p)


@pytest.mark.parametrize("W,H", [(2, 2), (3, 2), (5, 7), (64, 33)])
def test_f32_engine_at_the_drawers_operand_geometry(W, H):
    check_engine(W, H)


# ================================================================================================ 8. the whole map
def dft_synth(p, W, H, decay, contrast, colors, dtype):
    """the header comment's map as explicit DFT matrix products in `dtype`, twiddles and tables rounded from float64:
    x[c,h,w] = Re sum_v g_v e^{i th(v,w)} sum_u S[c,u,v] e^{i ph(u,h)} / sqrt(HW), S = scale * spectrum; a = contrast / std;
    rgb = sigmoid(sum_c a x_c M[c][d]).  p [1][3][H][Wf][2] (requires grad) -> [1][3][H][W]"""
    g = Geom(W, H)
    tabs, _, gv = tables64(W, H, decay, colors)
    scale = tabs["scale"].to(dtype)
    ph = 2 * math.pi * (torch.outer(torch.arange(H), torch.arange(H)) % H).double() / H
    thw = 2 * math.pi * (torch.outer(torch.arange(g.Wh), torch.arange(W)) % W).double() / W
    nrm = 1.0 / math.sqrt(W * H)
    ch, sh = torch.cos(ph).to(dtype), torch.sin(ph).to(dtype)
    cw, sw = (gv[:, None] * torch.cos(thw) * nrm).to(dtype), (gv[:, None] * torch.sin(thw) * nrm).to(dtype)
    q = p[0].to(dtype)
    re, im = q[:, :, :g.Wh, 0] * scale, q[:, :, :g.Wh, 1] * scale
    yr, yi = ch @ re - sh @ im, sh @ re + ch @ im
    x = yr @ cw - yi @ sw
    a = torch.tensor(contrast, dtype=dtype) / x.std()
    z = torch.einsum("chw,cd->dhw", a * x, tabs["cm"].to(dtype))
    return torch.sigmoid(z)[None]


def map_errors(fn, p, proj, ref, gref):
    q = p.clone().requires_grad_(True)
    img = fn(q)
    (gq,) = torch.autograd.grad((img * proj.to(img.dtype).to(img.device)).sum(), q)
    return float((img.detach().double().cpu() - ref).abs().max()), rel_l2(gq.detach().cpu(), gref), img.detach().cpu(), gq.detach().cpu()


def check_map(name, W, H, decay, contrast, colors, spectra):
    """`spectra`: the seeds' spectra [1][3][H][Wf][2] of one case.  Yardstick first (reference against reference, worst of the seeds),
    then the kernels on every seed against gates fixed by it"""
    g = Geom(W, H)
    d32, c32, k32 = f32v(decay), f32v(contrast), f32v(colors)
    refs, yard_img, yard_grad = [], 0.0, 0.0
    for i, p in enumerate(spectra):
        proj = rnd(1000 + i, 1, 3, H, W)
        q = p.clone().requires_grad_(True)
        ref = dft_synth(q, W, H, d32, c32, k32, F64)
        (gref,) = torch.autograd.grad((ref * proj.double()).sum(), q)
        ref, gref = ref.detach(), gref.detach().double()
        e_img, e_grad, _, _ = map_errors(lambda t: dft_synth(t, W, H, d32, c32, k32, F32), p, proj, ref, gref)
        yard_img, yard_grad = max(yard_img, e_img), max(yard_grad, e_grad)
        refs.append((proj, ref, gref))
    gate_img, gate_grad = min(4 * yard_img, 5e-6), min(4 * yard_grad, 2e-5)
    handle = ops.FftDrawerHandle(W, H, decay=decay, colors=colors)
    outs = []
    for i, (p, (proj, ref, gref)) in enumerate(zip(spectra, refs)):
        e_img, e_grad, img, gq = map_errors(lambda t: ops.fft_synth(t, handle, contrast), dev(p), proj, ref, gref)
        fig(f"map-img/{name}/s{i}", e_img, gate_img)
        fig(f"map-grad/{name}/s{i}", e_grad, gate_grad)
        print(f"[fft-fig] map-ratio/{name}/s{i} image {e_img / max(yard_img, 1e-300):.2f} gradient {e_grad / max(yard_grad, 1e-300):.2f} x yardstick")
        assert e_img <= gate_img, (name, i, e_img, gate_img)
        assert e_grad <= gate_grad, (name, i, e_grad, gate_grad)
        if W % 2:
            assert bool((gq[..., g.Wf - 1, :] == 0).all()), "the surplus column's gradient is exactly zero"
        outs.append((img, gq))
    return handle, outs


def spectra_of(W, H, n=4, dc=0.0):
    out = []
    for i in range(n):
        p = 0.01 * rnd(W * 1000 + H * 10 + i, 1, 3, H, Geom(W, H).Wf, 2)
        p[..., 0, 0, 0] += dc
        out.append(p)
    return out


MAP_SETTINGS = [(1.5, 0.9, 1.5), (0.0, 0.9, 1.5), (3.0, 2.5, 1.0), (1.0, 0.1, 2.0)]      # decay, contrast, colours


@pytest.mark.parametrize("decay,contrast,colors", MAP_SETTINGS, ids=["d1.5-c0.9-k1.5", "d0-c0.9-k1.5", "d3-c2.5-k1", "d1-c0.1-k2"])
@small
def test_whole_map(W, H, decay, contrast, colors):
    check_map(f"{W}x{H}-d{decay}-c{contrast}-k{colors}", W, H, decay, contrast, colors, spectra_of(W, H))


@pytest.mark.parametrize("dc", [0.05, 0.5])
def test_whole_map_dc_heavy_spectrum(dc):
    """a mean far from zero in the un-normalised image: the cancellation in x - mean and in acc[1] - n mean^2, in the product's flow"""
    check_map(f"20x12-dc{dc}", 20, 12, 1.5, 0.9, 1.5, spectra_of(20, 12, dc=dc))


@pytest.mark.parametrize("W,H", [(3, 2), (5, 7), (13, 4), (45, 32)])
def test_whole_map_never_reads_the_surplus_column(W, H):
    spectra = spectra_of(W, H, n=1)
    handle, outs = check_map(f"{W}x{H}-surplus", W, H, 1.5, 0.9, 1.5, spectra)
    q = spectra[0].clone()
    q[..., Geom(W, H).Wf - 1, :] = NAN
    img = ops.fft_synth(dev(q), handle, 0.9).cpu()
    assert bool(torch.isfinite(img).all())
    same_bits(img, outs[0][0])


@pytest.mark.parametrize("W,H", [(45, 32), (7, 5)])
def test_drawer_starts_from_an_image_on_an_odd_width_canvas_hip_path(W, H):
    """FftDrawer.init_from_tensor on the HIP path at an odd width: the synth of the initialised spectrum is the float64 map of that same
    spectrum (four images: the yardstick's four seeds)"""
    import types
    from pixray_amd.fft_drawer import FftDrawer
    st = types.SimpleNamespace(size=(W, H), fft_use="fft", fft_decay=1.5, fft_lrate=0.3, weight_seed=2, fft_hip_force=True)
    spectra, imgs = [], []
    for i in range(4):
        dr = FftDrawer(st)
        dr.load_model(st, DEV)
        dr.init_from_tensor(torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(i)) * 2 - 1)
        assert dr.hip and dr.params[0].shape == (1, 3, H, W // 2 + 2, 2)
        spectra.append(dr.params[0].detach().cpu().clone())
        imgs.append(dr.synth(0).detach().cpu())
    handle, outs = check_map(f"{W}x{H}-from-image", W, H, 1.5, 0.9, 1.5, spectra)
    for a, (b, _) in zip(imgs, outs):
        same_bits(a, b)                                                  # the drawer's own synth is that map


# ================================================================================================ 9. stale backward, refusals
def check_stale_backward():
    W, H = 20, 12
    handle = ops.FftDrawerHandle(W, H)
    p1, p2 = (dev(p).requires_grad_(True) for p in spectra_of(W, H, n=2))
    a = ops.fft_synth(p1, handle, 0.9)
    b = ops.fft_synth(p2, handle, 0.9)
    p1.grad = torch.full_like(p1, NAN)
    with pytest.raises(PrxError, match="stale backward -- this is the backward of synth 1 of its handle, which now holds the state of synth 2"):
        a.sum().backward()
    sync()
    assert all_nan(p1.grad), "the refused backward wrote the gradient"
    proj = dev(rnd(3, 1, 3, H, W))
    (g1,) = torch.autograd.grad((b * proj).sum(), p2, retain_graph=True)          # repeated backwards of the latest synth stay legal
    (g2,) = torch.autograd.grad((b * proj).sum(), p2)
    same_bits(g1.cpu(), g2.cpu())
    q = p2.detach().cpu().clone().requires_grad_(True)                            # and they are the gradient of THAT synth
    (gref,) = torch.autograd.grad((dft_synth(q, W, H, 1.5, f32v(0.9), 1.5, F64) * proj.cpu().double()).sum(), q)
    assert rel_l2(g1.cpu(), gref) < 2e-5


def test_a_stale_backward_is_refused():
    check_stale_backward()


def check_refusals():
    nan = lambda n, dtype=F32: torch.full((n,), NAN, dtype=dtype, device=DEV)
    x = torch.rand(4096, device=DEV)
    acc = torch.ones(3, dtype=F64, device=DEV)
    out, part, oacc = nan(4096), nan(64, F64), nan(3, F64)
    s = stream()
    bad = [
        ("fft pack: canvas 1 x 8 too small", "prx_k_fft_pack", (x, x, out, 1, 8, s)),
        ("fft pack: canvas 8 x 1 too small", "prx_k_fft_pack", (x, x, out, 8, 1, s)),
        ("fft pack: null argument", "prx_k_fft_pack", (None, x, out, 8, 6, s)),
        ("fft pack: null argument", "prx_k_fft_pack", (x, None, out, 8, 6, s)),
        ("fft unpack: canvas 0 x 8 too small", "prx_k_fft_unpack", (x, x, out, 0, 8, s)),
        ("fft unpack: null argument", "prx_k_fft_unpack", (x, None, out, 8, 6, s)),
        ("fft moments: null argument", "prx_k_fft_moments", (None, None, 12, part, oacc, s)),
        ("fft moments: no elements", "prx_k_fft_moments", (x, None, 0, part, oacc, s)),
        ("fft tail forward: canvas 8 x 1 too small", "prx_k_fft_tail_fwd", (x, acc, 0.9, x, out, 8, 1, s)),
        ("fft tail forward: null argument", "prx_k_fft_tail_fwd", (x, None, 0.9, x, out, 8, 6, s)),
        (r"fft tail backward \(gy\): canvas 1 x 1 too small", "prx_k_fft_tail_bwd_gy", (x, x, acc, 0.9, x, out, 1, 1, s)),
        (r"fft tail backward \(gy\): null argument", "prx_k_fft_tail_bwd_gy", (x, x, acc, 0.9, None, out, 8, 6, s)),
        (r"fft tail backward \(dx\): canvas -3 x 6 too small", "prx_k_fft_tail_bwd_dx", (x, x, acc, acc, 0.9, out, -3, 6, s)),
        (r"fft tail backward \(dx\): null argument", "prx_k_fft_tail_bwd_dx", (x, x, acc, None, 0.9, out, 8, 6, s)),
    ]
    for msg, entry, args in bad:
        with pytest.raises(PrxError, match=msg):
            call(entry, *args)
    for entry, args in (("prx_k_fft_pack", (x, x, None, 8, 6, s)), ("prx_k_fft_moments", (x, None, 12, None, oacc, s))):
        with pytest.raises(PrxError, match="null argument"):
            call(entry, *args)
    for W, H in ((1, 8), (8, 1)):
        with pytest.raises(PrxError, match=f"fft drawer: canvas {W} x {H} too small"):
            ops.FftDrawerHandle(W, H)
    handle = ops.FftDrawerHandle(45, 32)
    with pytest.raises(PrxError, match="fft drawer table: no table 6"):
        call("prx_fft_drawer_table", handle.h, 6, out, 9, s)
    with pytest.raises(PrxError, match="fft drawer table 5: 9 elements, not 8"):
        call("prx_fft_drawer_table", handle.h, 5, out, 8, s)
    with pytest.raises(PrxError, match="fft drawer table: null argument"):
        call("prx_fft_drawer_table", handle.h, 5, None, 9, s)
    # a spectrum with rfftn's column count, not the drawer's (an odd width has one more)
    with pytest.raises(PrxError, match=r"spectrum \(1, 3, 32, 23, 2\) does not fit a 45 x 32 canvas"):
        ops.fft_synth(torch.zeros(1, 3, 32, 23, 2, device=DEV), handle, 0.9)
    for entry, args in (("prx_fft_drawer_synth", (handle.h, None, 0.9, out, s)), ("prx_fft_drawer_backward", (handle.h, x, None, s))):
        with pytest.raises(PrxError, match="null argument"):
            call(entry, *args)
    sync()
    assert all_nan(out, part, oacc)


def test_refusals_leave_the_outputs_untouched():
    check_refusals()


# ================================================================================================ the CPU subset
def emu_subset():
    """every check of this file on the emulated kernels, except the cases one trip past the grid cap; returns the figures"""
    for W, H in SMALL:
        check_tables(W, H)
        check_pack(W, H)
        check_unpack(W, H)
        for contrast, mean_sigmas, zmax in TAIL_SETTINGS:
            check_tail_fwd(W, H, contrast, mean_sigmas, zmax)
            check_tail_gy(W, H, contrast, mean_sigmas, zmax)
        for contrast, mean_sigmas in ((0.9, 0), (0.1, 10), (2.5, 100)):
            check_tail_dx(W, H, contrast, mean_sigmas)
        for decay, contrast, colors in MAP_SETTINGS:
            test_whole_map(W, H, decay, contrast, colors)
    for decay, colors in ((0.0, 1.0), (3.0, 2.0)):
        test_tables_at_other_settings(decay, colors)
    for n in MOM_N:
        check_moments(n, False)
        check_moments(n, True)
    for n in (257, 262145):
        test_moments_of_a_mean_far_from_zero(n)
    for W, H in ((2, 2), (3, 2), (5, 7), (64, 33)):
        check_engine(W, H)
    for dc in (0.05, 0.5):
        test_whole_map_dc_heavy_spectrum(dc)
    for W, H in ((3, 2), (5, 7), (13, 4), (45, 32)):
        test_whole_map_never_reads_the_surplus_column(W, H)
    for W, H in ((45, 32), (7, 5)):
        test_drawer_starts_from_an_image_on_an_odd_width_canvas_hip_path(W, H)
    check_stale_backward()
    check_refusals()
    return FIGURES
