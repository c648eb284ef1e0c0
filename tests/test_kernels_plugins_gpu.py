"""Kernel-level float64 tests (GPU) of the built-in loss, blur and wallpaper kernels of csrc/plugin_losses.hip and csrc/plugin_filters.hip:
`saturation_fwd_kernel` / `saturation_bwd_kernel`, `symmetry_kernel`, `edge_kernel`, `edge_target_kernel`, `gaussian_kernel`,
`aesthetic_kernel`, `blur_fwd_kernel` / `blur_bwd_kernel`, `wallpaper_fwd_kernel` / `wallpaper_bwd_kernel`, each through the C entry the
product calls (`prx_saturation_fwd` / `_bwd`, `prx_symmetry_fwd_bwd`, `prx_edge_fwd_bwd`, `prx_edge_target_fwd_bwd`, `prx_gaussian_fwd_bwd`,
`prx_aesthetic_fwd_bwd`, `prx_blur_fwd` / `_bwd`, `prx_wallpaper_fwd` / `_bwd`), never through ops.py or the plugin classes.

Method (that of tests/test_kernels_select_gpu.py; helpers and the rules R1 / R2 / R3 of tests/test_kernels_runner_gpu.py, imported): every
input is drawn on the CPU from a seeded generator, outputs are pre-filled with NaN and carry spare rows that must come back untouched,
every reducing call gets its own zeroed ticket word (read back: zero again) and its own 4 * 1024 doubles of partials, and every reducer is
also run twice on ONE ticket word (bit-identical results).  References are plain torch in FLOAT64 on the fp32 inputs, written from the
pixray expression each kernel's comment cites (restated below, not imported), with autograd for the gradients.

Tolerances: R1 (bit equality) for the wallpaper image, for every gradient that is a pure gather (wallpaper backward with em == 0, or with a
null seam-loss gradient), for the blur adjoint of a one-hot (the tap table itself) and for entries that must be exactly zero; R2
(|out - ref64| <= k * 2^-24 * A, A the sum of the absolute float64 terms at the element, k the counted fp32 roundings, host-side `float`
arguments included, counted in a comment beside each use) for everything else.  R3 is not used: saturation's root-derived values are
bounded by propagating the counted roundings of rg and yb through variance, root and norm (`sat_stat_gates`), and its backward kernel is
fed the float64 statistics, so that its own chain is counted on its own.  The loss scalars are double sums with one final conversion:
k = (roundings per term) + 1 on the sum of the absolute terms; `aesthetic_kernel` works in double end to end: k = 1 for both outputs.

Measured (`python -m pytest -s` prints every figure as a `[plugin-fig]` line: name, kernel error, gate; no gate was moved after a run).
Worst kernel error / gate per family on an MI355X (on the CPU emulation in brackets): saturation statistics 0.27 (0.27), loss 0.14 (0.14),
gradient 0.40 (0.40); symmetry gradient 0.74 (0.74), loss 0.28 (0.28); edge gradient 0.22 (0.22), loss 0.16 (0.16); edge with target /
mask gradient 0.22 (0.22), loss 0.29 (0.29); gaussian gradient 0.50 (0.50), loss 0.05 (0.05); aesthetic gradient 0.997 (0.997), loss 0.85
(0.85) -- k = 1 is the conversion's own half ulp, which the worst of 12300 elements nearly reaches; blur forward 0.92 (0.92) and
backward 0.89 (0.89), both at k = 1 (one product: again a half ulp), 0.07 and 0.09 at k = 4, 1e-3 and 2e-3 at k = 33; wallpaper loss
0.26 (0.26), gradient 0.99 (0.99) in shift mode (one addition), 0.39 (0.39) with seams; every R1 comparison bit-equal.  Of the 260
figures the device's and the emulation's agree in every printed digit but one (a mean_rg of 2.3e-18 against 6.9e-18, the last bit of a
double sum).  No defect was found: the hipcc build's division and root land where the host build's do at all of these points.

Mutation check on the emulated kernels (sources and tools/hipemu copied aside, one line changed, the two plugin objects rebuilt, every
test of this file below the workgroup cap run; all sixteen caught):
`t[a * k + b]` -> `t[b * k + a]` in blur_bwd_kernel: test_blur_asymmetric_taps at k = 4, 5, 33 and the one-hot test at k = 4, 33 fail;
the same in blur_fwd_kernel: test_blur_asymmetric_taps at k = 4, 5, 33; `w / 2` -> `(w + 1) / 2` in both wallpaper kernels:
test_wallpaper shift mode at w = 7 and w = 5 and test_wallpaper_shift_mode_ignores_edge_match (even w and w = 1 pass); `em / 2` ->
`(em + 1) / 2` in WallGeom: every em = 3 and em = 5 case of test_wallpaper and the sweep (even em passes); `vc0 = 0; vc1 = w`: the seam
loss of every mode-`both` case with em > 0 (2e-4 .. 0.25 off); pmod as a plain `%`: every test_wallpaper case with a negative word, the
staged-shifts test, the sweep; the `c >= left && c < w - right` condition dropped in edge_kernel: the seven test_edge_bands cases with a
side band and an upper or lower band; `pl % 3` -> `pl % 2`: every test_edge_bands case, test_edge_colour_channel_is_the_plane_modulo_three,
the target / mask test and test_gaussian; `mask[rem] <= 0.f` -> `< 0.f`: test_edge_target_image_and_mask_combinations (the planted
+0.0); `gy[y], gx[c]` -> `gy[c % h], gx[y % w]`: test_gaussian at 5 x 9, 9 x 5, 19 x 31; `d >= 0.f ? ... : ...`: test_gaussian (the
planted x == colour); `4.f * weight` -> `2.f * weight`: test_symmetry and its sweep wherever w > 1; `(Nd - 1.0)` -> `Nd`: S of
test_saturation_random and of the offset image; the `S > 0.0 ?` guard removed: test_saturation_constant_colour_S_is_zero (NaN) and the
grey image; `floor_ ? 0.0 :` removed: test_aesthetic at every shape with the planted rows (1e8 off); `atomicInc(ticket, gridDim.x - 1)`
-> `atomicAdd(ticket, 1)`: "the ticket word is not zero again on exit" in 66 of the 77 cases run (every reducing call).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from pixray_amd import _lib  # noqa: F401
from pixray_amd._lib import PrxError, call

import test_kernels_half_gpu as th  # noqa: F401
from test_kernels_half_gpu import guarded, untouched, within, rel_l2, bits  # noqa: F401  (within: behind check_f32)
from test_kernels_runner_gpu import stream, sync, flat, check_f32, same_bits

DEV = "cuda"          # tests/test_emu_cpu.py switches this (and the helper modules') to "cpu" for the emulated kernels
EPS32 = 2.0 ** -24
DBL = 64 * 2.0 ** -53   # a double sum of this file: under 40 additions deep (thread, wave, workgroup, 16 rows per lane, wave), each 2^-53
NAN = float("nan")
F32 = torch.float32
F64 = torch.float64
FIGURES = {}          # name -> (worst kernel error, its gate), printed by the tests (`pytest -s`)
CAP = 1024 * 256      # elements of a full grid: one more and the grid-stride loops take a second trip
BOTH, HORIZONTAL, VERTICAL, SHIFT = 0, 1, 2, 3          # PRX_WALL_* of include/prx.h


def dev(t):
    return t.to(DEV)


def f32v(v):
    """the fp32 value a C `float` argument takes"""
    return float(torch.tensor(v, dtype=F32))


def fig(name, err, gate):
    err, gate = float(err), float(gate)
    old = FIGURES.get(name)
    if old is None or err / max(gate, 1e-300) >= old[0] / max(old[1], 1e-300):
        FIGURES[name] = (err, gate)
    print(f"[plugin-fig] {name} {err:.3e} {gate:.3e}")


def scratch():
    """a zeroed ticket word and 4 * 1024 doubles of partials for ONE call"""
    return torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(4 * 1024, dtype=F64, device=DEV)


def r2(name, out, ref64, k, A):
    """R2 elementwise: prints the element that comes closest to its gate, then asserts every element"""
    out, ref64 = out.detach().double().cpu(), ref64.detach().double().cpu()
    tol = (k * EPS32 * A.detach().double().cpu()).expand_as(ref64)
    err = (out - ref64).abs()
    ratio = (err / tol.clamp_min(1e-300)).nan_to_num(nan=float("inf")).flatten()
    i = int(ratio.argmax())
    fig(name, err.flatten()[i], tol.flatten()[i])
    check_f32(out, ref64, k, A.detach().double().cpu().expand_as(ref64))


def scalar(name, got, ref64, gate):
    err = abs(float(got) - float(ref64))
    fig(name, err, gate)
    assert err <= gate, (name, float(got), float(ref64), err, gate)


def all_nan(*ts):
    return all(bool(torch.isnan(t).all()) for t in ts)


def zero_ticket(tk):
    assert int(tk.item()) == 0, "the ticket word is not zero again on exit"


# ================================================================================================ 1. saturation
def sat_ref(x, weight, mean_term_only=False):
    """SaturationLoss.py on one cutout batch, float64: x [n][3][hw] -> (loss, grad, (mean_rg, mean_yb, S, M))"""
    xr = x.double().requires_grad_(True)
    px = xr.permute(0, 2, 1).reshape(-1, 3)
    rg = px[:, 0] - px[:, 1]
    yb = 0.5 * (px[:, 0] + px[:, 1]) - px[:, 2]
    rg_std, rg_mean = torch.std_mean(rg)
    yb_std, yb_mean = torch.std_mean(yb)
    ss, mm = rg_std ** 2 + yb_std ** 2, rg_mean ** 2 + yb_mean ** 2
    std_rggb = torch.sqrt(ss)
    mean_rggb = torch.sqrt(mm)
    colorfullness = (0.0 if mean_term_only else std_rggb) + .3 * mean_rggb
    loss = -colorfullness * weight / 10.0
    (g,) = torch.autograd.grad(loss, xr) if float(mm.detach()) > 0 else (torch.zeros_like(xr),)
    full = -(std_rggb + .3 * mean_rggb) * weight / 10.0
    return full.detach(), g, torch.stack([rg_mean, yb_mean, std_rggb, mean_rggb]).detach()


def sat_terms(x):
    """float64 rg, yb per pixel and the bounds of their fp32 roundings: rg = r - g is one rounding on |r| + |g|; yb = 0.5f * (r + g) - bl
    is the sum (1, the halving is exact) and the subtraction (1): 2 on 0.5 (|r| + |g|) + |bl|"""
    px = x.double().permute(0, 2, 1).reshape(-1, 3)
    r, g, b = px[:, 0], px[:, 1], px[:, 2]
    a_rg, a_yb = r.abs() + g.abs(), 0.5 * (r.abs() + g.abs()) + b.abs()
    return r - g, 0.5 * (r + g) - b, a_rg, a_yb, 1 * EPS32 * a_rg, 2 * EPS32 * a_yb


def sat_stat_gates(x, st64):
    """R2 carried through the statistics.  With x_i' = x_i + d_i, |d_i| <= e_i (sat_terms):
      mean' - mean = mean(d): |.| <= mean(e)
      var' = var + 2 / (N - 1) sum (x_i - m) d_i + 1 / (N - 1) sum (d_i - mean d)^2, so S'^2 lies in [S^2 - 2 G - D, S^2 + 2 G + Q + D],
        G = sum |x_i - m| e_i / (N - 1), Q = sum e_i^2 / (N - 1) (both over rg and yb), D the double round-off of v1 - v0 * mean:
        DBL on sum x_i^2 and on v0 * mean <= sum x_i^2
      M = |(mean_rg, mean_yb)| is 1-Lipschitz in that vector: |M' - M| <= |(mean e_rg, mean e_yb)|"""
    rg, yb, a_rg, a_yb, e_rg, e_yb = sat_terms(x)
    N = rg.numel()
    mrg, myb, S, M = (float(v) for v in st64)
    g_mrg = float(e_rg.mean()) + DBL * float(rg.abs().mean())
    g_myb = float(e_yb.mean()) + DBL * float(yb.abs().mean())
    G = float(((rg - mrg).abs() * e_rg).sum() + ((yb - myb).abs() * e_yb).sum()) / (N - 1)
    Q = float((e_rg ** 2).sum() + (e_yb ** 2).sum()) / (N - 1)
    D = DBL * 2.0 * float((rg ** 2).sum() + (yb ** 2).sum()) / (N - 1)
    g_S = max((S * S + 2 * G + Q + D) ** 0.5 - S, S - max(S * S - 2 * G - D, 0.0) ** 0.5)
    g_M = (g_mrg ** 2 + g_myb ** 2) ** 0.5
    return g_mrg, g_myb, g_S, g_M


def sat_formula(x, st, weight, gout):
    """the gradient the comment above saturation_bwd_kernel states, in float64 at the statistics `st`, and the A of each element.
    R2 of the kernel's chain: a1, brg / byb, fmrg / fmyb are each one conversion (3); drg = a1 * ((r - g) - fmrg) + brg: r - g (1; yb: 2),
    the subtraction (1), the product (1), the sum (1); pg = drg + 0.5f * dyb (1): at most k = 3 + 2 + 3 + 1 = 9 on
    A_rg = |a1| (|r| + |g| + |mean_rg|) + |brg|, A_yb alike; r and g carry A_rg + 0.5 A_yb, b carries A_yb"""
    n, _, hw = x.shape
    rg, yb, a_rg, a_yb, _, _ = sat_terms(x)
    N = rg.numel()
    mrg, myb, S, M = (float(v) for v in st)
    c = -weight / 10.0 * gout
    a1 = c / ((N - 1) * S) if S > 0 else 0.0
    brg = c * 0.3 * mrg / (N * M) if M > 0 else 0.0
    byb = c * 0.3 * myb / (N * M) if M > 0 else 0.0
    drg, dyb = a1 * (rg - mrg) + brg, a1 * (yb - myb) + byb
    A_rg, A_yb = abs(a1) * (a_rg + abs(mrg)) + abs(brg), abs(a1) * (a_yb + abs(myb)) + abs(byb)
    grad = torch.stack([drg + 0.5 * dyb, -drg + 0.5 * dyb, -dyb], 1)
    A = torch.stack([A_rg + 0.5 * A_yb, A_rg + 0.5 * A_yb, A_yb], 1)
    back = lambda t: t.reshape(n, hw, 3).permute(0, 2, 1)
    return back(grad), back(A)


def sat_fwd(xd, n, hw, weight, ticket=None):
    tk, partials = scratch()
    tk = tk if ticket is None else ticket
    sfull, st = flat(4, F64)
    lfull, ls = flat(1, F32)
    call("prx_saturation_fwd", xd, n, hw, weight, partials, sfull, lfull, tk, stream())
    sync()
    assert untouched(sfull, 1, 4) and untouched(lfull, 1, 1)
    zero_ticket(tk)
    return st, ls


def sat_bwd(xd, n, hw, weight, st, gout):
    gfull, gr = guarded(n * 3, hw, F32)
    call("prx_saturation_bwd", xd, n, hw, weight, st, dev(torch.tensor([gout], dtype=F32)), gfull, stream())
    sync()
    assert untouched(gfull, n * 3, hw)
    return gr.reshape(n, 3, hw)


def sat_case(name, x, weight=0.37, gout=1.7):
    """forward: the four statistics and the loss against float64 under the propagated R2; backward twice: fed the FLOAT64 statistics
    against float64 autograd (the kernel's own chain, and its two guards), and fed the forward kernel's statistics against the kernel
    comment's formula in float64 at those statistics (the product's data flow)"""
    n, _, hw = x.shape
    weight, gout = f32v(weight), f32v(gout)
    xd = dev(x)
    st, ls = sat_fwd(xd, n, hw, weight)
    tk = torch.zeros(1, dtype=torch.int32, device=DEV)
    for _ in range(2):                                     # two calls on one ticket word: bit-identical
        st2, ls2 = sat_fwd(xd, n, hw, weight, ticket=tk)
        assert torch.equal(st2, st) and torch.equal(bits(ls2), bits(ls)), "two calls on one ticket differ"
    l64, g64, st64 = sat_ref(x, weight)
    gates = sat_stat_gates(x, st64)
    for i, what in enumerate(("mean_rg", "mean_yb", "S", "M")):
        scalar(f"sat/{name}/{what}", st[i], st64[i], gates[i])
    # loss = (float)(-(S + 0.3 M) * weight / 10): the statistics' bounds and the conversion (1)
    scalar(f"sat/{name}/loss", ls, l64, abs(weight) / 10.0 * (gates[2] + 0.3 * gates[3]) + 1 * EPS32 * abs(float(l64)))
    S64, M64 = float(st64[2]), float(st64[3])
    if S64 == 0.0:                                         # sqrt's derivative at 0: autograd (pixray's too) gives NaN; the mean term decides
        _, g64, _ = sat_ref(x, weight, mean_term_only=True)
    g64 = g64 * gout
    f64, A = sat_formula(x, st64, weight, gout)
    assert float((f64 - g64).abs().max()) <= 1e-9 * float(A.max()), "the kernel comment's formula is not autograd's gradient"
    r2(f"sat/{name}/grad-of-float64-stats", sat_bwd(xd, n, hw, weight, dev(st64), gout), g64, 9, A)
    own = st.detach().cpu().clone()
    fown, Aown = sat_formula(x, own, weight, gout)
    got = sat_bwd(xd, n, hw, weight, st, gout)
    r2(f"sat/{name}/grad-of-own-stats", got, fown, 9, Aown)
    return st, ls, got


SAT_SHAPES = [(1, 2), (2, 15), (1, 257), (3, 171), (1, CAP + 1)]     # N = 2; 2 x 3 x 3 x 5; N % 256 == 1 twice; one pixel past the cap


@pytest.mark.parametrize("n,hw", SAT_SHAPES)
def test_saturation_random(n, hw):
    g = torch.Generator().manual_seed(n * 1000 + hw)
    sat_case(f"rand-{n}x{hw}", torch.rand(n, 3, hw, generator=g))


def test_saturation_mean_large_against_spread():
    """channel offsets (0.9, 0.1, 0.3) + 1e-3 noise: rg = 0.8 +- 1e-3, each rounded at 2^-24 * 1.0 -- the deviations carry 6e-5 of
    themselves, which is what the propagated bound states and what v1 - v0 * mean must not make worse"""
    g = torch.Generator().manual_seed(5)
    x = torch.tensor([0.9, 0.1, 0.3])[None, :, None] + 1e-3 * torch.randn(2, 3, 300, generator=g)
    sat_case("offset", x)


def test_saturation_constant_colour_S_is_zero():
    """S = 0, M > 0: `S > 0 ? ... : 0`.  Fed S = 0 the backward must give the mean term's gradient alone (without the guard c / 0 = inf,
    inf * 0 = NaN); in the product's flow S may come out as the root of v1's double round-off, but (r - g) - fmrg is exactly 0 (the
    sum of N equal fp32 values is exact in double, and so is its division by N), so the gradient is the mean term's there too"""
    x = torch.tensor([0.8, 0.25, 0.4])[None, :, None].repeat(2, 1, 37).contiguous()
    weight, gout = f32v(0.37), f32v(1.7)
    st, ls, got = sat_case("constant", x)
    assert float(sat_ref(x, weight)[2][2]) == 0.0
    _, g64, st64 = sat_ref(x, weight, mean_term_only=True)
    _, A = sat_formula(x, torch.tensor([float(st64[0]), float(st64[1]), 0.0, float(st64[3])]), weight, gout)
    r2("sat/constant/own-stats-against-the-mean-term", got, g64 * gout, 9, A)
    assert bool(torch.isfinite(got).all())


def test_saturation_grey_image_is_zero_not_nan():
    """r = g = b: rg = yb = 0 exactly, S = 0 and M = 0.  pixray's expression gives NaN here (sqrt's derivative at 0 is inf, times 0); the
    zero loss and the zero gradient are this project's documented choice (the guards `S > 0` / `M > 0`)"""
    g = torch.Generator().manual_seed(9)
    x = torch.rand(2, 1, 41, generator=g).repeat(1, 3, 1).contiguous()
    xd = dev(x)
    st, ls = sat_fwd(xd, 2, 41, f32v(0.37))
    assert bool((st == 0).all()) and float(ls) == 0.0
    for stats in (st, torch.zeros(4, dtype=F64, device=DEV)):
        assert bool((sat_bwd(xd, 2, 41, f32v(0.37), stats, 1.7) == 0).all()), "the gradient of a grey image must be exactly zero"
    fig("sat/grey/loss", abs(float(ls)), 0.0)


# ================================================================================================ 2. symmetry
def sym_launch(xd, planes, h, w, weight, ticket=None):
    tk, partials = scratch()
    tk = tk if ticket is None else ticket
    gfull, gr = guarded(planes * h, w, F32)
    lfull, ls = flat(1, F32)
    call("prx_symmetry_fwd_bwd", xd, planes, h, w, weight, partials, gfull, lfull, tk, stream())
    sync()
    assert untouched(gfull, planes * h, w) and untouched(lfull, 1, 1)
    zero_ticket(tk)
    return gr.reshape(planes, h, w), ls


def sym_case(name, planes, h, w, weight=0.37, twice=True):
    g = torch.Generator().manual_seed(planes * 100 + h * 10 + w)
    x = torch.randn(1, planes, h, w, generator=g)
    weight = f32v(weight)
    xd = dev(x)
    gr, ls = sym_launch(xd, planes, h, w, weight)
    if twice:
        tk = torch.zeros(1, dtype=torch.int32, device=DEV)
        for _ in range(2):
            g2, l2 = sym_launch(xd, planes, h, w, weight, ticket=tk)
            assert torch.equal(bits(g2), bits(gr)) and torch.equal(bits(l2), bits(ls)), "two calls on one ticket differ"
    xr = x.double().requires_grad_(True)
    loss = F.mse_loss(xr, torch.flip(xr, [3])) * weight                 # SymmetryLoss.py
    (g64,) = torch.autograd.grad(loss, xr)
    loss = loss.detach()
    N = x.numel()
    # grad = gs * d: gs = 4.f * weight / (float)N (the division: 1), d = x - mirror (1), the product (1): k = 3 on 4 |w| (|x| + |mirror|) / N
    A = 4.0 * abs(weight) * (x.double().abs() + torch.flip(x, [3]).double().abs()) / N
    r2(f"sym/{name}/grad", gr, g64[0], 3, A[0])
    # loss: d (1, squared: 2), the sum, / N and * weight in double, the conversion (1): k = 3 on the sum of positive terms
    scalar(f"sym/{name}/loss", ls, loss, 3 * EPS32 * abs(float(loss)))
    if w % 2:
        assert bool((gr[:, :, w // 2] == 0).all()), "the centre column of an odd width mirrors onto itself: exactly zero"
    return gr, ls


SYM_SHAPES = [(6, 2, 8), (4, 1, 2), (3, 4, 1), (5, 3, 7), (1, 5, (CAP + 1) // 5)]     # 2 x 3 x 2 x 8; 1 x 4 x 1 x 2; w = 1; odd w; past the cap


@pytest.mark.parametrize("planes,h,w", SYM_SHAPES)
def test_symmetry(planes, h, w):
    gr, ls = sym_case(f"{planes}x{h}x{w}", planes, h, w)
    if w == 1:
        assert float(ls) == 0.0


SWEEP = [1, 255, 256, 257, 64 * 256 + 1, CAP + 1]          # 1 workgroup (ragged, full), 2, 65 (the last workgroup's sum strides), the cap + 1


@pytest.mark.parametrize("total", SWEEP)
def test_launch_shape_sweep_symmetry(total):
    sym_case(f"sweep-{total}", 1, 1, total)
    FIGURES[f"sweep/sym-{total}"] = FIGURES[f"sym/sweep-{total}/loss"]


# ================================================================================================ 3. edge, 4. edge with target / mask
def edge_ref(out, zers, margins, mask, edge_weight, global_weight):
    """EdgeLoss.py:77-108 with the margins already in pixels.  The right / lower bands start at max(size - margin, 0): the kernel
    documents them as [w - right, w) and [h - lower, h) (a margin past the size is the whole axis), where a negative python start would
    count from the other end"""
    mse = lambda a, b: ((a - b) ** 2).mean()
    cur = out.new_zeros(())
    lmax, rmax = out.shape[2], out.shape[3]
    if mask is None:
        left, right, upper, lower = margins
        r0, d0 = max(rmax - right, 0), max(lmax - lower, 0)
        if left != 0:
            cur = cur + mse(out[:, :, :, :left], zers[:, :, :, :left])
        if right != 0:
            cur = cur + mse(out[:, :, :, r0:], zers[:, :, :, r0:])
        if upper != 0:
            cur = cur + mse(out[:, :, :upper, left:r0], zers[:, :, :upper, left:r0])
        if lower != 0:
            cur = cur + mse(out[:, :, d0:, left:r0], zers[:, :, d0:, left:r0])
    else:
        maked_out = torch.where(mask > 0, zers, out)
        cur = cur + mse(maked_out, zers)
    if global_weight:
        cur = cur + mse(out, zers) * global_weight
    return cur * edge_weight


def edge_weights(shape, margins, masked, global_weight):
    """the five 1 / (band elements) in float64, from the sizes of the slices edge_ref takes (0 where a margin is 0), and the weight
    a64 of every element: the sum of the bands that hold it"""
    z = torch.zeros(shape, dtype=F64)
    w, h = shape[3], shape[2]
    left, right, upper, lower = margins
    r0, d0 = max(w - right, 0), max(h - lower, 0)
    views = [z[:, :, :, :left], z[:, :, :, r0:], z[:, :, :upper, left:r0], z[:, :, d0:, left:r0]]
    inv = [1.0 / v.numel() if m != 0 else 0.0 for v, m in zip(views, margins)]
    inv_all = global_weight / z.numel() if global_weight else 0.0
    if not masked:
        for v, i in zip(views, inv):
            v += i
    return inv, inv_all, z + inv_all


def edge_launch(entry, xd, planes, h, w, target, col, mask, margins, inv, inv_mask, inv_all, ew, ticket=None):
    tk, partials = scratch()
    tk = tk if ticket is None else ticket
    gfull, gr = guarded(planes * h, w, F32)
    lfull, ls = flat(1, F32)
    if entry == "prx_edge_fwd_bwd":
        call(entry, xd, planes, h, w, *col, *margins, *inv, inv_all, ew, partials, gfull, lfull, tk, stream())
    else:
        call(entry, xd, planes, h, w, target, *col, mask, *margins, *inv, inv_mask, inv_all, ew, partials, gfull, lfull, tk, stream())
    sync()
    assert untouched(gfull, planes * h, w) and untouched(lfull, 1, 1)
    zero_ticket(tk)
    return gr.reshape(planes // 3, 3, h, w), ls


EDGE_COLOUR = (0.9, 0.2, 0.55)


def edge_case(name, n, h, w, margins, global_weight, target=None, mask=None, entry="prx_edge_target_fwd_bwd", ew=0.37):
    """x [n][3][h][w] against the flat colour or `target` [3][h][w], with the margin bands or `mask` [h][w]"""
    g = torch.Generator().manual_seed(n * 1000 + h * 10 + w + sum(margins))
    x = torch.rand(n, 3, h, w, generator=g)
    ew = f32v(ew)
    col = tuple(f32v(c) for c in EDGE_COLOUR)
    inv64, inv_all64, a64 = edge_weights(x.shape, margins, mask is not None, global_weight)
    inv_mask64 = 1.0 / x.numel() if mask is not None else 0.0
    if mask is not None:
        a64 = a64 + inv_mask64 * (mask <= 0).double()[None, None]
    inv = [f32v(v) for v in inv64]                      # computed in float64, rounded to the fp32 the C arguments are
    args = (dev(x), n * 3, h, w, None if target is None else dev(target), col, None if mask is None else dev(mask), margins, inv,
            f32v(inv_mask64), f32v(inv_all64), ew)
    gr, ls = edge_launch(entry, *args)
    tk = torch.zeros(1, dtype=torch.int32, device=DEV)
    for _ in range(2):
        g2, l2 = edge_launch(entry, *args, ticket=tk)
        assert torch.equal(bits(g2), bits(gr)) and torch.equal(bits(l2), bits(ls)), "two calls on one ticket differ"
    zers = (torch.tensor(col, dtype=F64)[None, :, None, None].expand(n, 3, h, w) if target is None
            else target.double()[None].expand(n, 3, h, w))
    xr = x.double().requires_grad_(True)
    loss = edge_ref(xr, zers, margins, None if mask is None else mask.double()[None, None], ew, global_weight)
    (g64,) = torch.autograd.grad(loss, xr)
    loss = loss.detach()
    # a = inv_all + up to two band terms (corners: side bands only; with a mask: inv_mask): each a host conversion (3; mask: 2) and two
    # additions (mask: 1): ka = 5 (3).  grad = 2.f * edge_weight * a * d: d = x - tgt (1), two products (2): k = ka + 3 on
    # 2 |ew| a64 (|x| + |tgt|).  loss: a (ka), d squared (2), the conversion (1): k = ka + 3 on the sum of positive terms
    ka = 3 if mask is not None else 5
    A = 2.0 * abs(ew) * a64 * (x.double().abs() + zers.abs())
    r2(f"{name}/grad", gr, g64, ka + 3, A)
    scalar(f"{name}/loss", ls, loss, (ka + 3) * EPS32 * abs(float(loss)))
    return gr, ls, x


EDGE_CASES = [(2, 5, 7, (2, 3, 1, 2), 0.3),                   # batch 2, every band, the global term
              (1, 5, 7, (0, 3, 1, 2), 0.3), (1, 5, 7, (2, 0, 1, 2), 0.0), (1, 5, 7, (2, 3, 0, 2), 0.3), (1, 5, 7, (2, 3, 1, 0), 0.0),
              (1, 5, 7, (3, 4, 0, 0), 0.3),                   # left + right == w: inner width 0
              (1, 5, 7, (7, 9, 0, 0), 0.0),                   # both >= w: every column in both side bands
              (1, 5, 7, (1, 1, 6, 2), 0.3),                   # upper >= h
              (1, 5, 7, (1, 1, 3, 3), 0.0),                   # upper and lower meet and overlap
              (2, 4, 6, (0, 0, 0, 0), 0.7),                   # the global term alone
              (3, 3, 3, (0, 0, 0, 2), 0.0)]                   # batch 3, only `lower`


@pytest.mark.parametrize("n,h,w,margins,gw", EDGE_CASES)
def test_edge_bands(n, h, w, margins, gw):
    """edge_kernel, and edge_target_kernel with neither target nor mask: the same outputs bit for bit"""
    name = f"{n}x{h}x{w}-{'.'.join(map(str, margins))}-{gw}"
    gr, ls, _ = edge_case("edge/" + name, n, h, w, margins, gw, entry="prx_edge_fwd_bwd")
    gt, lt, _ = edge_case("edget/null-null-" + name, n, h, w, margins, gw)
    same_bits(gt, gr)
    same_bits(lt, ls)


def edge_target(h, w):
    return torch.rand(3, h, w, generator=torch.Generator().manual_seed(h * w))


def planted_mask(h, w):
    m = torch.rand(h, w, generator=torch.Generator().manual_seed(h + w)) - 0.5
    m.view(-1)[:6] = torch.tensor([0.0, -0.0, -1e-30, 1e-30, -1e-45, 1e-45])     # exact zeros of both signs, the smallest numbers around them
    return m


def test_edge_target_image_and_mask_combinations():
    """target / null x mask / null at batch 2 (both broadcast across the batch); with a mask the margins and their weights are ignored
    (they are passed non-zero here), `mask <= 0` counts exact zeros of both signs and the smallest negative numbers, `> 0` does not"""
    n, h, w = 2, 5, 7
    tgt, m = edge_target(h, w), planted_mask(h, w)
    assert int((m == 0).sum()) == 2 and int((m < 0).sum()) >= 2 and int((m > 0).sum()) >= 2
    edge_case("edget/target", n, h, w, (2, 3, 1, 2), 0.3, target=tgt)
    edge_case("edget/target-mask", n, h, w, (2, 3, 1, 2), 0.3, target=tgt, mask=m)
    edge_case("edget/mask", n, h, w, (2, 3, 1, 2), 0.0, mask=m)
    edge_case("edget/mask-all-positive", n, h, w, (0, 0, 0, 0), 0.3, mask=m.abs() + 0.1)          # only the global term remains
    edge_case("edget/mask-all-nonpositive", n, h, w, (0, 0, 0, 0), 0.0, target=tgt, mask=-m.abs())


def test_edge_colour_channel_is_the_plane_modulo_three():
    """a batch of 3 on a flat image equal to the colour: every element's d is exactly 0 only if plane p is compared with component p % 3"""
    n, h, w = 3, 4, 5
    col = tuple(f32v(c) for c in EDGE_COLOUR)
    x = torch.tensor(col)[None, :, None, None].expand(n, 3, h, w).contiguous()
    inv64, inv_all64, _ = edge_weights(x.shape, (1, 1, 1, 1), False, 0.5)
    for entry in ("prx_edge_fwd_bwd", "prx_edge_target_fwd_bwd"):
        gr, ls = edge_launch(entry, dev(x), n * 3, h, w, None, col, None, (1, 1, 1, 1), [f32v(v) for v in inv64], 0.0, f32v(inv_all64),
                             f32v(0.37))
        assert bool((gr == 0).all()) and float(ls) == 0.0


# ================================================================================================ 5. gaussian
def gauss_launch(xd, planes, h, w, gyd, gxd, col, scale, ticket=None):
    tk, partials = scratch()
    tk = tk if ticket is None else ticket
    gfull, gr = guarded(planes * h, w, F32)
    lfull, ls = flat(1, F32)
    call("prx_gaussian_fwd_bwd", xd, planes, h, w, gyd, gxd, *col, scale, partials, gfull, lfull, tk, stream())
    sync()
    assert untouched(gfull, planes * h, w) and untouched(lfull, 1, 1)
    zero_ticket(tk)
    return gr.reshape(planes // 3, 3, h, w), ls


GAUSS_SHAPES = [(2, 5, 9), (1, 9, 5), (1, 1, 1), (3, 19, 31)]


@pytest.mark.parametrize("n,h,w", GAUSS_SHAPES)
def test_gaussian(n, h, w):
    """h != w with gy and gx drawn independently in [0, 1.6) (no Gaussian tables: a swap shows; products above 1: |1 - .| folds),
    batch 2, x == colour bitwise at planted elements of one plane: gradient exactly zero there, not beside them"""
    g = torch.Generator().manual_seed(h * 100 + w)
    gy, gx = 1.6 * torch.rand(h, generator=g), 1.6 * torch.rand(w, generator=g)
    col = tuple(f32v(c) for c in EDGE_COLOUR)
    x = torch.rand(n, 3, h, w, generator=g)
    x[n - 1, 1, h // 2, :] = col[1]
    x[n - 1, 1, h // 2, w // 2] = col[1]
    weight = 0.37
    scale64 = weight / x.numel()
    args = (dev(x), n * 3, h, w, dev(gy), dev(gx), col, f32v(scale64))
    gr, ls = gauss_launch(*args)
    tk = torch.zeros(1, dtype=torch.int32, device=DEV)
    for _ in range(2):
        g2, l2 = gauss_launch(*args, ticket=tk)
        assert torch.equal(bits(g2), bits(gr)) and torch.equal(bits(l2), bits(ls)), "two calls on one ticket differ"
    gaus = torch.outer(gy, gx)                                          # GaussianLoss.py: the product in fp32, as torch.outer rounds it
    if h * w >= 45:
        assert float(gaus.max()) > 1.0 and float(gaus.min()) < 1.0
    color = torch.tensor(col, dtype=F64)[None, :, None, None].expand(n, 3, h, w)
    xr = x.double().requires_grad_(True)
    loss = (torch.abs(xr - color) * torch.abs(1 - gaus.double())).mean() * weight
    (g64,) = torch.autograd.grad(loss, xr)
    loss = loss.detach()
    # grad = +-(scale * a): scale (host conversion: 1), a = |1 - product| (1), the product (1): k = 3 on |scale| (1 + product)
    A = (abs(scale64) * (1.0 + gaus.double().abs()))[None, None].expand(n, 3, h, w)
    r2(f"gauss/{n}x{h}x{w}/grad", gr, g64, 3, A)
    # loss: a (1), d = x - colour (1), scale (1), the conversion (1): k = 4 on |scale| sum (1 + product) (|x| + |colour|)
    scalar(f"gauss/{n}x{h}x{w}/loss", ls, loss, 4 * EPS32 * float((A * (x.double().abs() + color.abs())).sum()))
    assert bool((gr[n - 1, 1, h // 2, :] == 0).all()), "x == colour: the zero subgradient"
    beside = gr[n - 1, 0, h // 2, :].cpu()                              # the same row of the plane before it: not planted
    assert bool((beside != 0)[gaus[h // 2] != 1].all()), "beside the planted elements the gradient is +-scale * a, not zero"


# ================================================================================================ 6. aesthetic
def aes_launch(ed, n, d, wd, bias, target, ticket=None):
    tk, partials = scratch()
    tk = tk if ticket is None else ticket
    gfull, gr = guarded(n, d, F32)
    lfull, ls = flat(1, F32)
    call("prx_aesthetic_fwd_bwd", ed, n, d, wd, bias, target, partials, gfull, lfull, tk, stream())
    sync()
    assert untouched(gfull, n, d) and untouched(lfull, 1, 1)
    zero_ticket(tk)
    return gr, ls


AES_SHAPES = [(1, 1), (3, 63), (5, 64), (2, 65), (9, 80), (4100, 3)]


@pytest.mark.parametrize("n,d", AES_SHAPES)
def test_aesthetic(n, d):
    """d < 64 (lanes without an element), d = 64, 65, 80, d = 1 (the gradient is pure cancellation: R2's A, no relative error), more than
    4096 rows (the wave loop strides); an all-zero row and a row of norm 1e-13, below F.normalize's floor of 1e-12: the divisor is the
    constant and only the first gradient term remains.  The kernel works in double: k = 1 (the conversion) for both outputs"""
    g = torch.Generator().manual_seed(n * 100 + d)
    e = torch.randn(n, d, generator=g)
    w = torch.randn(d, generator=g)
    if n >= 3 and d >= 2:
        e[1] = 0.0
        e[n - 1] = e[n - 1] / e[n - 1].double().norm() * 1e-13
        assert 0 < float(e[n - 1].double().norm()) < 1e-12
    bias, target = f32v(4.9), f32v(7.3)
    ed, wd = dev(e), dev(w)
    gr, ls = aes_launch(ed, n, d, wd, bias, target)
    tk = torch.zeros(1, dtype=torch.int32, device=DEV)
    for _ in range(2):
        g2, l2 = aes_launch(ed, n, d, wd, bias, target, ticket=tk)
        assert torch.equal(bits(g2), bits(gr)) and torch.equal(bits(l2), bits(ls)), "two calls on one ticket differ"
    er = e.double().requires_grad_(True)
    aes_rating = F.normalize(er, dim=-1) @ w.double()[:, None] + bias             # AestheticLoss.py: nn.Linear(d, 1) on the normalised rows
    loss = (aes_rating - target).square().mean() * 0.02
    (g64,) = torch.autograd.grad(loss, er)
    loss = loss.detach()
    nrm = e.double().norm(dim=1)
    floor_ = nrm <= 1e-12
    inv = 1.0 / torch.where(floor_, torch.full_like(nrm, 1e-12), nrm)
    dot = e.double() @ w.double()
    diff = dot * inv + bias - target
    ga = 0.04 / n * diff * inv
    gb = torch.where(floor_, torch.zeros_like(ga), 0.04 / n * diff * dot * inv ** 3)
    A = ga.abs()[:, None] * w.double().abs()[None] + gb.abs()[:, None] * e.double().abs()
    r2(f"aes/{n}x{d}/grad", gr, g64, 1, A)
    scalar(f"aes/{n}x{d}/loss", ls, loss, 1 * EPS32 * abs(float(loss)))


# ================================================================================================ 7. blur
def blur_fwd(x, taps):
    planes, h, w = x.shape
    k = taps.shape[0]
    yfull, y = guarded(planes * (h - k + 1), w - k + 1, F32)
    call("prx_blur_fwd", dev(x), planes, h, w, dev(taps), k, yfull, stream())
    sync()
    assert untouched(yfull, planes * (h - k + 1), w - k + 1)
    return y.reshape(planes, h - k + 1, w - k + 1)


def blur_bwd(gy, taps, h, w):
    planes = gy.shape[0]
    k = taps.shape[0]
    gfull, gx = guarded(planes * h, w, F32)
    call("prx_blur_bwd", dev(gy), planes, h, w, dev(taps), k, gfull, stream())
    sync()
    assert untouched(gfull, planes * h, w)
    return gx.reshape(planes, h, w)


def conv64(x, taps):
    """GaussianSmoothing's F.conv2d(groups = channels), valid padding, one k x k table for every plane"""
    planes = x.shape[0]
    return F.conv2d(x[None], taps[None, None].expand(planes, 1, *taps.shape).contiguous(), groups=planes)[0]


BLUR_CASES = [(6, 5, 7, 1), (3, 6, 9, 4), (3, 4, 9, 4), (3, 7, 4, 4), (6, 9, 8, 5), (3, 33, 36, 33), (3, 35, 33, 33)]


@pytest.mark.parametrize("planes,h,w,k", BLUR_CASES)
def test_blur_asymmetric_taps(planes, h, w, k):
    """taps drawn with randn: neither symmetric along an axis nor under transposition, so t[b * k + a] and a flipped adjoint show.
    k = 1, an even k, the maximum 33; h == k (one output row), w == k (one output column); planes = 6.
    R2: the loop is one fp32 multiply-add per tap into one accumulator; a term goes through its own product and every later addition,
    at most k * k roundings (the first addition, to 0, is exact; a fused multiply-add has fewer): k_r2 = k * k on sum |t| |x|"""
    g = torch.Generator().manual_seed(planes * 1000 + h * 40 + w + k)
    taps = torch.randn(k, k, generator=g)
    x = torch.randn(planes, h, w, generator=g)
    probe = torch.randn(planes, h - k + 1, w - k + 1, generator=g)
    xr = x.double().requires_grad_(True)
    y64 = conv64(xr, taps.double())
    (gx64,) = torch.autograd.grad(y64, xr, probe.double())
    name = f"blur/{planes}x{h}x{w}-k{k}"
    r2(name + "/fwd", blur_fwd(x, taps), y64, k * k, conv64(x.double().abs(), taps.double().abs()))
    xa = x.double().requires_grad_(True)
    (A,) = torch.autograd.grad(conv64(xa, taps.double().abs()), xa, probe.double().abs())
    r2(name + "/bwd", blur_bwd(probe, taps, h, w), gx64, k * k, A)


@pytest.mark.parametrize("k", [1, 4, 33])
def test_blur_bwd_of_a_one_hot_is_the_tap_table_unflipped(k):
    """R1: gy = 1 at (plane 1, oy, ox): gx[1][oy + a][ox + b] = t[a][b] * 1 + zeros, bit for bit; every other entry zero"""
    planes, h, w = 3, k + 5, k + 7
    oy, ox = 2, 5
    taps = torch.randn(k, k, generator=torch.Generator().manual_seed(k))
    gy = torch.zeros(planes, h - k + 1, w - k + 1)
    gy[1, oy, ox] = 1.0
    gx = blur_bwd(gy, taps, h, w).cpu()
    same_bits(gx[1, oy:oy + k, ox:ox + k], taps)
    rest = gx.clone()
    rest[1, oy:oy + k, ox:ox + k] = 0.0
    assert bool((rest == 0).all())
    fig(f"blur/one-hot-k{k}", 0.0, 0.0)


# ================================================================================================ 8. wallpaper
def wall_ref(imgs, mode, em, rand_h, rand_w):
    """WallpaperFilter.forward (filters/wallpaper.py:25-94) with the two draws handed in"""
    mse = lambda a, b: ((a - b) ** 2).mean()
    loss = imgs.new_zeros(())
    B, C, H, W = imgs.shape
    if mode == SHIFT:
        half_W = int(W / 2)
        row2 = torch.roll(imgs, shifts=(half_W,), dims=(3,))
        two_rows = torch.cat([imgs, row2], dim=2)
        imgs = torch.roll(two_rows, shifts=(rand_h, rand_w), dims=(2, 3))
    elif mode == HORIZONTAL:
        if em != 0:
            em2 = int(em / 2)
            loss = mse(imgs[:, :, :, :em], imgs[:, :, :, -em:]) / em
            imgs = imgs[:, :, :, em2:-em2]
        imgs = torch.roll(imgs, shifts=(rand_w,), dims=(3,))
    elif mode == VERTICAL:
        if em != 0:
            em2 = int(em / 2)
            loss = mse(imgs[:, :, :em, :], imgs[:, :, -em:, :]) / em
            imgs = imgs[:, :, em2:-em2, :]
        imgs = torch.roll(imgs, shifts=(rand_h,), dims=(2,))
    else:
        if em != 0:
            em2 = int(em / 2)
            loss1 = mse(imgs[:, :, :, :em], imgs[:, :, :, -em:]) / em
            imgs = imgs[:, :, :, em2:-em2]
            loss2 = mse(imgs[:, :, :em, :], imgs[:, :, -em:, :]) / em       # over the columns left after the horizontal trim
            imgs = imgs[:, :, em2:-em2, :]
            loss = loss1 + loss2
        imgs = torch.roll(imgs, shifts=(rand_h, rand_w), dims=(2, 3))
    return imgs, loss


def wall_fwd(xd, planes, h, w, mode, em, shifts, oshape, ticket=None):
    tk, partials = scratch()
    tk = tk if ticket is None else ticket
    ofull, out = guarded(planes * oshape[0], oshape[1], F32)
    lfull, ls = flat(1, F32)
    call("prx_wallpaper_fwd", xd, planes, h, w, mode, em, shifts, partials, ofull, lfull, tk, stream())
    sync()
    assert untouched(ofull, planes * oshape[0], oshape[1]) and untouched(lfull, 1, 1)
    zero_ticket(tk)
    return out.reshape(planes, *oshape), ls


def wall_bwd(xd, gout, planes, h, w, mode, em, shifts, gloss):
    gfull, gr = guarded(planes * h, w, F32)
    call("prx_wallpaper_bwd", xd, dev(gout), planes, h, w, mode, em, shifts, None if gloss is None else dev(torch.tensor([gloss], dtype=F32)),
         gfull, stream())
    sync()
    assert untouched(gfull, planes * h, w)
    return gr.reshape(planes, h, w)


def wall_case(name, mode, planes, h, w, em, sh, gloss=1.3, integer=False, twice=True):
    g = torch.Generator().manual_seed(planes * 1000 + h * 37 + w + (0 if mode == SHIFT else em))
    x = (torch.arange(planes * h * w, dtype=F32).reshape(planes, h, w) if integer else torch.randn(planes, h, w, generator=g))
    xd = dev(x)
    shifts = dev(torch.tensor(sh, dtype=torch.int32))
    em_ref = 0 if mode == SHIFT else em                                  # the reference's shift branch never looks at edge_match
    xr = x.double()[None].requires_grad_(True)
    o64, l64 = wall_ref(xr, mode, em_ref, sh[0], sh[1])
    oshape = tuple(o64.shape[2:])
    out, ls = wall_fwd(xd, planes, h, w, mode, em, shifts, oshape)
    if twice:
        tk = torch.zeros(1, dtype=torch.int32, device=DEV)
        for _ in range(2):
            o2, l2 = wall_fwd(xd, planes, h, w, mode, em, shifts, oshape, ticket=tk)
            assert torch.equal(bits(o2), bits(out)) and torch.equal(bits(l2), bits(ls)), "two calls on one ticket differ"
    same_bits(out.cpu(), wall_ref(x[None], mode, em_ref, sh[0], sh[1])[0][0].contiguous())       # R1: the image is a gather
    # loss = (float)(v0 * ch) + (float)(v1 * cv): d = x - x' (1, squared: 2), the double sums, a conversion each (1), their sum (1):
    # k = 4 on the sum of positive terms
    scalar(f"wall/{name}/loss", ls, l64.detach(), 4 * EPS32 * abs(float(l64.detach())))
    gout = torch.randn(planes, *oshape, generator=g)
    gl = f32v(gloss)
    (g64,) = torch.autograd.grad((o64[0] * gout.double()).sum() + gl * l64, xr)
    l64 = l64.detach()
    xa = x.double()[None].requires_grad_(True)
    (A,) = torch.autograd.grad((wall_ref(xa, mode, em_ref, sh[0], sh[1])[0][0] * gout.double().abs()).sum(), xa)   # sum of the |gout| gathered
    ax = x.double().abs()[None]
    if em_ref:                                                           # |2 c gl| (|x| + |x'|) on both bands of each seam
        A = A.clone()
        if mode in (BOTH, HORIZONTAL):
            s = 2.0 * abs(gl) / (planes * h * em * em) * (ax[..., :em] + ax[..., -em:])
            A[..., :em] += s
            A[..., -em:] += s
        if mode in (BOTH, VERTICAL):
            c0, c1 = (em // 2, w - em // 2) if mode == BOTH else (0, w)
            s = 2.0 * abs(gl) / (planes * em * (c1 - c0) * em) * (ax[:, :, :em, c0:c1] + ax[:, :, -em:, c0:c1])
            A[:, :, :em, c0:c1] += s
            A[:, :, -em:, c0:c1] += s
    gr = wall_bwd(xd, gout, planes, h, w, mode, em, shifts, gl)
    if em_ref == 0 and mode != SHIFT:
        same_bits(gr.cpu(), g64[0].float())                              # R1: a pure gather (kh = kv = 0)
        fig(f"wall/{name}/grad", 0.0, 0.0)
    else:
        # shift mode: the sum of two gathered values (1): k = 1.  seams: kh = (float)(2 c) * gl (2), d (1), the product (1), its addition
        # (1), the other seam's addition (1): k = 6 on |gout gathered| + the seam terms
        r2(f"wall/{name}/grad", gr, g64[0], 1 if mode == SHIFT else 6, A[0])
    if em_ref:                                                           # a null seam-loss gradient: the gather alone, R1
        (g0,) = torch.autograd.grad((wall_ref(xa, mode, em_ref, sh[0], sh[1])[0][0] * gout.double()).sum(), xa)
        same_bits(wall_bwd(xd, gout, planes, h, w, mode, em, shifts, None).cpu(), g0[0].float())
    return out, ls, gr


WALL_CASES = [(BOTH, 6, 5, 7, 0, (0, 0)), (BOTH, 3, 5, 7, 0, (-3, 16)), (BOTH, 3, 6, 9, 3, (-4, 23)), (BOTH, 3, 8, 10, 2, (9, -1)),
              (BOTH, 3, 11, 10, 5, (3, 4)), (BOTH, 3, 10, 13, 5, (-13, 30)), (BOTH, 6, 6, 6, 3, (1, 2)), (BOTH, 3, 4, 4, 2, (0, 0)),
              (HORIZONTAL, 3, 4, 7, 3, (5, -3)), (HORIZONTAL, 6, 3, 4, 2, (1, 9)), (HORIZONTAL, 3, 2, 11, 5, (0, 0)),
              (HORIZONTAL, 3, 4, 7, 0, (2, -8)),
              (VERTICAL, 3, 7, 4, 3, (-3, 5)), (VERTICAL, 3, 4, 5, 2, (6, 1)), (VERTICAL, 6, 10, 3, 5, (0, 0)), (VERTICAL, 3, 7, 4, 0, (-9, 2)),
              (SHIFT, 3, 4, 7, 0, (0, 0)), (SHIFT, 6, 3, 5, 0, (-5, 12)), (SHIFT, 3, 5, 1, 0, (11, 3)), (SHIFT, 3, 4, 8, 0, (7, -3))]


@pytest.mark.parametrize("mode,planes,h,w,em,sh", WALL_CASES)
def test_wallpaper(mode, planes, h, w, em, sh):
    """every mode; shifts {0, 0}, negative and >= the size, both words different (the unused word of `horizontal` / `vertical` too);
    em = 2, 3, 5 (odd: the trim is em // 2), 2 * em == w and 2 * em == h (the two seam bands tile the axis); mode `both` at h != w with
    em = 3 (the vertical seam over the trimmed columns only); `shift` at odd w (the second row rolled by w // 2) and at w = 1;
    planes = 6; once with integer-valued pixels (every gather shows its source), once random"""
    name = f"m{mode}-{planes}x{h}x{w}-em{em}-{sh[0]}.{sh[1]}"
    wall_case(name, mode, planes, h, w, em, sh)
    wall_case(name + "-int", mode, planes, h, w, em, sh, integer=True, twice=False)


def test_wallpaper_shift_mode_ignores_edge_match():
    a = wall_case("shift-em0", SHIFT, 3, 4, 7, 0, (2, 3))
    b = wall_case("shift-em3", SHIFT, 3, 4, 7, 3, (2, 3))
    for u, v in zip(a, b):
        same_bits(u, v)
    assert float(b[1]) == 0.0


def test_wallpaper_reads_the_staged_shifts_at_every_call():
    """the two words are read on the device at launch: rewriting the SAME buffer changes the next call (what a replayed graph relies on)"""
    planes, h, w = 3, 5, 7
    x = torch.arange(planes * h * w, dtype=F32).reshape(planes, h, w)
    shifts = dev(torch.tensor([1, 2], dtype=torch.int32))
    xd = dev(x)
    for sh in ((1, 2), (-2, 10), (0, 0)):
        shifts.copy_(torch.tensor(sh, dtype=torch.int32))
        out, ls = wall_fwd(xd, planes, h, w, BOTH, 0, shifts, (h, w))
        same_bits(out.cpu(), torch.roll(x, shifts=sh, dims=(1, 2)))


# total elements -> (mode, planes, h, w, em): wallpaper_fwd_kernel runs its three loops on the grid of planes * h * w
WALL_SWEEP = {1: (BOTH, 1, 1, 1, 0), 255: (BOTH, 1, 15, 17, 3), 256: (BOTH, 1, 16, 16, 3), 257: (HORIZONTAL, 1, 1, 257, 3),
              64 * 256 + 1: (BOTH, 1, 113, 145, 3), CAP + 1: (BOTH, 1, 481, 545, 3)}


@pytest.mark.parametrize("total", SWEEP)
def test_launch_shape_sweep_wallpaper_fwd(total):
    mode, planes, h, w, em = WALL_SWEEP[total]
    assert planes * h * w == total
    wall_case(f"sweep-{total}", mode, planes, h, w, em, (-1, 3), twice=total <= 64 * 256 + 1)
    FIGURES[f"sweep/wall-{total}"] = FIGURES[f"wall/sweep-{total}/loss"]


# ================================================================================================ refusals
def test_refusals_leave_the_outputs_untouched():
    nan = lambda *shape, dtype=F32: torch.full(shape, NAN, dtype=dtype, device=DEV)
    x = torch.rand(12 * 40 * 40, device=DEV)
    tk, partials = scratch()
    sh = torch.zeros(2, dtype=torch.int32, device=DEV)
    one = torch.ones(1, device=DEV)
    grad, loss, stats = nan(12 * 40 * 40), nan(1), nan(4, dtype=F64)
    bad = [
        ("saturation: bad arguments", "prx_saturation_fwd", (x, 1, 1, 1.0, partials, stats, loss, tk, stream())),           # N = 1
        ("saturation: bad arguments", "prx_saturation_fwd", (x, 2, 3, 1.0, partials, None, loss, tk, stream())),
        ("saturation backward: bad arguments", "prx_saturation_bwd", (x, 2, 3, 1.0, None, one, grad, stream())),
        ("symmetry: bad arguments", "prx_symmetry_fwd_bwd", (x, 3, 4, 5, 1.0, partials, grad, loss, None, stream())),
        ("edge: bad arguments", "prx_edge_fwd_bwd", (x, 4, 5, 7, .1, .2, .3, 1, 1, 1, 1, .1, .1, .1, .1, .1, 1.0, partials, grad, loss, tk,
                                                    stream())),                                                             # planes % 3
        ("negative margins", "prx_edge_target_fwd_bwd", (x, 3, 5, 7, None, .1, .2, .3, None, 1, -1, 1, 1, .1, .1, .1, .1, 0.0, .1, 1.0,
                                                         partials, grad, loss, tk, stream())),
        ("gaussian: bad arguments", "prx_gaussian_fwd_bwd", (x, 3, 5, 7, None, x, .1, .2, .3, 1.0, partials, grad, loss, tk, stream())),
        ("aesthetic: bad arguments", "prx_aesthetic_fwd_bwd", (x, 0, 8, x, 0.0, 1.0, partials, grad, loss, tk, stream())),  # n = 0
        (r"blur: bad arguments \(k = 34\)", "prx_blur_fwd", (x, 3, 40, 40, x, 34, grad, stream())),
        (r"blur: bad arguments \(k = 5\)", "prx_blur_fwd", (x, 3, 4, 40, x, 5, grad, stream())),                            # h < k
        ("blur backward: bad arguments", "prx_blur_bwd", (x, 3, 40, 40, x, 34, grad, stream())),
        ("blur backward: bad arguments", "prx_blur_bwd", (x, 3, 4, 40, x, 5, grad, stream())),
        ("wallpaper: mode 0, edge match 1 on", "prx_wallpaper_fwd", (x, 3, 8, 8, BOTH, 1, sh, partials, grad, loss, tk, stream())),
        ("wallpaper: mode 1, edge match 5 on 8 x 9", "prx_wallpaper_fwd", (x, 3, 8, 9, HORIZONTAL, 5, sh, partials, grad, loss, tk, stream())),
        ("wallpaper: mode 4", "prx_wallpaper_fwd", (x, 3, 8, 8, 4, 0, sh, partials, grad, loss, tk, stream())),
        ("wallpaper: mode -1", "prx_wallpaper_fwd", (x, 3, 8, 8, -1, 0, sh, partials, grad, loss, tk, stream())),
        ("wallpaper: null argument", "prx_wallpaper_fwd", (x, 3, 8, 8, BOTH, 0, None, partials, grad, loss, tk, stream())),
        ("wallpaper backward: mode 2, edge match 5 on 9 x 8", "prx_wallpaper_bwd", (x, x, 3, 9, 8, VERTICAL, 5, sh, one, grad, stream())),
        ("wallpaper backward: null argument", "prx_wallpaper_bwd", (x, None, 3, 8, 8, BOTH, 0, sh, one, grad, stream())),
    ]
    for msg, entry, args in bad:
        with pytest.raises(PrxError, match=msg):
            call(entry, *args)
    sync()
    assert all_nan(grad, loss, stats) and int(tk.item()) == 0 and bool((partials == 0).all())


# ================================================================================================ the CPU subset
def emu_subset(past_the_cap=True):
    """every case of this file on the emulated kernels; returns the figures.  The four cases one element past the 1024-workgroup cap
    (saturation, symmetry and the two sweeps at 1024 * 256 + 1) are a quarter of a million fibers each: `past_the_cap=False` leaves
    them to the GPU"""
    small = lambda total: past_the_cap or total <= CAP
    for n, hw in SAT_SHAPES:
        if small(n * hw):
            test_saturation_random(n, hw)
    test_saturation_mean_large_against_spread()
    test_saturation_constant_colour_S_is_zero()
    test_saturation_grey_image_is_zero_not_nan()
    for planes, h, w in SYM_SHAPES:
        if small(planes * h * w):
            test_symmetry(planes, h, w)
    for total in SWEEP:
        if small(total):
            test_launch_shape_sweep_symmetry(total)
            test_launch_shape_sweep_wallpaper_fwd(total)
    for case in EDGE_CASES:
        test_edge_bands(*case)
    test_edge_target_image_and_mask_combinations()
    test_edge_colour_channel_is_the_plane_modulo_three()
    for shape in GAUSS_SHAPES:
        test_gaussian(*shape)
    for shape in AES_SHAPES:
        test_aesthetic(*shape)
    for case in BLUR_CASES:
        test_blur_asymmetric_taps(*case)
    for k in (1, 4, 33):
        test_blur_bwd_of_a_one_hot_is_the_tap_table_unflipped(k)
    for case in WALL_CASES:
        test_wallpaper(*case)
    test_wallpaper_shift_mode_ignores_edge_match()
    test_wallpaper_reads_the_staged_shifts_at_every_call()
    test_refusals_leave_the_outputs_untouched()
    return FIGURES
