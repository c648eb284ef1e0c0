"""The separable tile path of the warp backward's form 0 (csrc/cutouts.hip: separable_stage / separable_tile) and its process-wide
switch `prx_cutout_bwd_separable` (GPU; tests/test_cutout_separable_cpu.py runs all of it on the emulated kernels).

A block of form 0 takes the path when its cutout's stage is an affine flavour under zeros / fill padding, the matrix's off-diagonal
words pass the pre-filter, the tile's destination box has at most SEP_CAP = 80 columns and rows, and the per-axis coordinate tables
are bit-identical at both ends of the box.  Everything else runs the workgroup scatter as before.

What is checked, per case and for both stages:
1. `tc.run_stage(..., forms=[0, 2])` with the switch on: that file's float64 gates and its twice-run bit-identity, unchanged;
2. on every ELIGIBLE cutout form 0 (switch on) equals form 2 BIT FOR BIT: the separable sum is gather_pixel's arithmetic in
   gather_pixel's order.  Compared per cutout: stage A on the private planes, before they are summed over the cutouts;
3. with the switch off form 0 still passes the gates;
4. on the generic-weight cases the switch changes at least one bit of an eligible cutout (the scatter sums in another order): the
   path ran and the switch works;
5. where every weight is exactly 0 or 1 (integer shift at scale 1: one term per source pixel) on, off and form 2 are bit-identical;
6. cutouts that are NOT eligible (off-diagonals of 1e-6, a box beyond the cap, perspective / rotated / border / copy cutouts beside
   a separable one) are bit-identical with the switch on and off: the block-uniform branch does not leak.
8. the ORDER itself is restated in this file (scatter_order_frozen: a wave in lockstep, written out in numpy fp32): setting 2 must
   reproduce it bit for bit on the device AND on the emulated kernels, and on the device the scatter (setting 0) must too -- so a
   change of scatter_candidate / scatter_rect that alters the order fails on the device, and a change of the separable sum fails on
   the emulation as well;
7. with the switch at 2, the product default (the separable tiles summed in the SCATTER'S order: per-wave partial sums over the
   64-candidate blocks each wave owned, tap kind by tap kind, the four partial sums added in wave order), form 0 is bit-identical
   to the switch-off result on every cutout of every case here, eligible or not -- so the iteration keeps the bits it had.
The switch is restored in a `finally` everywhere.

Shapes are tc.SMALL's (sources 20x37, 9x9, 33x16; destinations 17x23 and 40x40, square on stage B), a 104x104 destination over a
20x20 source for the cap (tc.SPECIAL's magnify6 geometry), and a 17x17 destination over the 9x9 source for the integer shift on
both stages: with corner-aligned grids of 16 and 8 intervals every step of project() is exact there, which the test asserts on the
frozen copy of project() instead of assuming it."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from pixray_amd import _lib
from pixray_amd import cutouts as pc
from pixray_amd._lib import call

import test_kernels_half_gpu as th
import test_kernels_cutouts_gpu as tc
import test_cutout_passes_gpu as tpass
from test_kernels_half_gpu import guarded, untouched, rel_l2
from test_kernels_runner_gpu import stream, sync
from test_kernels_cutouts_gpu import (GRID_MESH, GRID_AFFINE, GRID_AFFINE_AC, M_COPY, M_ZEROS, M_BORDER, M_FILL, Cut, desc_words,
                                      desc_tensor, norm_matrix, pixel_map, run_stage)

from oracle import cutouts_ref


def dev(t):
    return tc.dev(t)       # follows tc.DEV ("cuda"; "cpu" on the emulated kernels)


SCATTER_ORDER = 2          # the product default: the separable tiles summed in the scatter's order
# The scatter's order is that of a wave running in lockstep: instruction by instruction, the lanes of one LDS add ascending.  The CPU
# emulation runs the lanes of a wave one after another between two synchronisation points, so ITS scatter sums lane by lane and has
# other bits than the device's; tests/test_cutout_separable_cpu.py clears this flag and holds setting 2 to value gates instead.
LOCKSTEP = True


@contextlib.contextmanager
def separable(on):
    """True / 1: the separable path in the gather's order; False / 0: off; SCATTER_ORDER: the separable path in the scatter's order"""
    lib = _lib.load()
    before = lib.prx_cutout_bwd_separable(int(on))
    try:
        yield
    finally:
        lib.prx_cutout_bwd_separable(before)


def same(a, b):
    return a.shape == b.shape and torch.equal(th.bits(a), th.bits(b))


def planes(stage, cuts, Hs, Ws, Hd, Wd, form, seed, edge_window=False):
    """per-cutout source-gradient planes of one backward launch with a randn gradient: stage 1 the PRIVATE planes [n,3,Hs,Ws] (before
    reduce_planes sums them), stage 2 `ga` [n,3,Hs+11,Ws+13] through run_stage's window"""
    torch.manual_seed(seed)
    n = len(cuts)
    g = dev(torch.randn(n, 3, Hd, Wd))
    if stage == 1:
        desc = desc_tensor([desc_words(m1=c.m, mode1=c.mode, grid1=c.gtype, fill=c.fill) for c in cuts])
        fuv, _ = guarded(1, n * Hd * Wd * 2, torch.float32)
        fpriv, priv = guarded(n * 3 * Hs, Ws, torch.float32)
        fg, _ = guarded(3 * Hs, Ws, torch.float32)
        call("prx_k_warp_a_bwd", g, Hs, Ws, desc, fuv, fpriv, fg, n, Hd, Wd, form, stream())
        sync()
        assert untouched(fg, 3 * Hs, Ws) and untouched(fpriv, n * 3 * Hs, Ws) and untouched(fuv, 1, n * Hd * Wd * 2)
        out = priv.view(n, 3, Hs, Ws).cpu().clone()
    else:
        assert Hd == Wd
        HA, WA = Hs + 11, Ws + 13
        ox, oy = (13, 11) if edge_window else (5, 3)
        desc = desc_tensor([desc_words(m2=c.m, mode2=c.mode, grid2=c.gtype, fill=c.fill, win=(ox, oy, Ws, Hs)) for c in cuts])
        src = dev(torch.rand(n, 3, HA, WA))
        fuv, _ = guarded(1, n * Hd * Hd * 2, torch.float32)
        frgb, _ = guarded(n * 3 * Hd, Hd, torch.float32)
        fg, gk = guarded(n * 3 * HA, WA, torch.float32)
        maps = dev(torch.zeros(n * 16))
        call("prx_k_warp_b_bwd", src, HA, WA, desc, g, frgb, fuv, fg, n, Hd, maps, maps.numel() * 4, form, stream())
        sync()
        assert untouched(fg, n * 3 * HA, WA) and untouched(fuv, 1, n * Hd * Hd * 2)
        out = gk.view(n, 3, HA, WA).cpu().clone()
    assert bool(torch.isfinite(out).all())
    return out


def scatter_order_frozen(cut, g, Hs, Ws, Hd, Wd, Ho, Wo, ox, oy):
    """What scatter_tile leaves in a zeros / fill cutout's plane [3,Ho,Wo], restated: a frozen copy of the ORDER, written here and never
    derived from a kernel's output.  Per 16 x 16 tile of the output image: the tile's single raw rectangle and its destination box
    (tile_intervals, preimage_box on the frozen stage map, fp32 operation by operation); candidate k = j * bw + i of the box belongs to
    wave (k >> 6) & 3, which takes its candidates 256 apart in ascending order and per candidate issues the north-west, north-east,
    south-west, south-east tap adds, the lanes of one add ascending (a wave in lockstep); every wave has its own plane, and the four
    are summed ((p0 + p1) + p2) + p3.  Coordinates are tpass.project_frozen's, weights make_taps' / sample_plane's fp32 products."""
    import numpy as np
    F = np.float32
    sm = tpass.stage_map_frozen(cut.m, cut.gtype, Wd, Hd, Ws, Hs).numpy()
    Pi, ulo, uhi, vlo, vhi = sm[:9], sm[9], sm[10], sm[11], sm[12]
    u, v = [t.numpy() for t in tpass.project_frozen(cut.m, cut.gtype, Wd, Hd, Ws, Hs)]
    fx, fy = np.floor(u), np.floor(v)
    wx, wy = (u - fx).astype(F), (v - fy).astype(F)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    e, s_ = (F(1) - wx).astype(F), (F(1) - wy).astype(F)
    wts = [(s_ * e).astype(F), (s_ * wx).astype(F), (wy * e).astype(F), (wy * wx).astype(F)]          # NW, NE, SW, SE
    gn = g.numpy()
    eps = F(2e-3)

    def interval(s0, s1, lo, hi):
        a, b = max(F(F(s0) - F(1)) - eps, lo), min(F(F(s1) + F(1)) + eps, hi)
        return (a, b) if b > a else None

    def box(ua, ub, va, vb):
        xs, ys, bad = [], [], False
        for k in range(4):
            uu, vv = (ub if k & 1 else ua), (vb if k & 2 else va)
            z = F(F(Pi[6] * uu) + F(Pi[7] * vv)) + Pi[8]
            if not z > F(0.05):
                bad = True
                continue
            iz = F(1) / z
            xs.append(F(F(F(Pi[0] * uu) + F(Pi[1] * vv)) + Pi[2]) * iz)
            ys.append(F(F(F(Pi[3] * uu) + F(Pi[4] * vv)) + Pi[5]) * iz)
        if bad:
            return 0, Wd - 1, 0, Hd - 1
        x0, x1 = max(int(np.floor(min(xs) - F(0.25))), 0), min(int(np.ceil(max(xs) + F(0.25))), Wd - 1)
        y0, y1 = max(int(np.floor(min(ys) - F(0.25))), 0), min(int(np.ceil(max(ys) + F(0.25))), Hd - 1)
        return (x0, x1, y0, y1) if x0 <= x1 and y0 <= y1 else None

    out = np.zeros((3, Ho, Wo), dtype=F)
    for ay0 in range(0, Ho, 16):
        for ax0 in range(0, Wo, 16):
            tx0, ty0 = ax0 - ox, ay0 - oy
            sx0, sx1, sy0, sy1 = max(tx0, 0), min(tx0 + 15, Ws - 1), max(ty0, 0), min(ty0 + 15, Hs - 1)
            if sx0 > sx1 or sy0 > sy1:
                continue
            xi, yi = interval(sx0, sx1, ulo, uhi), interval(sy0, sy1, vlo, vhi)
            bx = box(xi[0], xi[1], yi[0], yi[1]) if xi and yi else None
            if bx is None:
                continue
            x0, x1, y0, y1 = bx
            bw, cnt = x1 - x0 + 1, (x1 - x0 + 1) * (y1 - y0 + 1)
            acc = np.zeros((4, 3, 16, 16), dtype=F)
            for blk in range((cnt + 63) // 64):                      # the blocks of one wave come in ascending order: that is all that counts
                w = blk & 3
                ks = [k for k in range(blk * 64, min(blk * 64 + 64, cnt))]
                for kind in range(4):
                    for k in ks:
                        y, x = y0 + k // bw, x0 + k % bw
                        if not (xi[0] <= u[y, x] < xi[1] and yi[0] <= v[y, x] < yi[1]):
                            continue
                        px, py = ix[y, x] + (kind & 1), iy[y, x] + (kind >> 1)
                        if not (0 <= px < Ws and 0 <= py < Hs and 0 <= px - tx0 < 16 and 0 <= py - ty0 < 16):
                            continue
                        wt = wts[kind][y, x]
                        for c in range(3):
                            acc[w, c, py - ty0, px - tx0] = acc[w, c, py - ty0, px - tx0] + F(gn[c, y, x] * wt)
            tot = ((acc[0] + acc[1]) + acc[2]) + acc[3]
            for ly in range(16):
                for lx in range(16):
                    ax, ay = ax0 + lx, ay0 + ly
                    if ax < Wo and ay < Ho and 0 <= ax - ox < Ws and 0 <= ay - oy < Hs:
                        out[:, ay, ax] = tot[:, ly, lx]
    return torch.from_numpy(out)


def check_scatter_order(stage, cuts, which, Hs, Ws, Hd, Wd, seed, edge_window=False):
    """the cutouts `which` (eligible ones) of a launch against the frozen order: setting 2 everywhere -- on the emulated kernels too,
    this is what holds separable_sum_scatter_order there --, and on the device also the scatter itself (setting 0)"""
    torch.manual_seed(seed)
    g = torch.randn(len(cuts), 3, Hd, Wd)              # planes()' first draw
    if stage == 1:
        Ho, Wo, ox, oy = Hs, Ws, 0, 0
    else:
        Ho, Wo = Hs + 11, Ws + 13
        ox, oy = (13, 11) if edge_window else (5, 3)
    with separable(SCATTER_ORDER):
        keep = planes(stage, cuts, Hs, Ws, Hd, Wd, 0, seed, edge_window)
    with separable(False):
        off = planes(stage, cuts, Hs, Ws, Hd, Wd, 0, seed, edge_window)
    for i in which:
        want = scatter_order_frozen(cuts[i], g[i], Hs, Ws, Hd, Wd, Ho, Wo, ox, oy)
        assert same(keep[i], want), ("setting 2 is not the frozen scatter order", stage, i, int((th.bits(keep[i]) != th.bits(want)).sum()))
        if LOCKSTEP:
            assert same(off[i], want), ("the device's scatter is not the frozen scatter order", stage, i)


def three_ways(stage, cuts, Hs, Ws, Hd, Wd, seed, edge_window=False):
    """(form 0 switch on, form 0 switch off, form 2) per-cutout planes of the same launch"""
    with separable(True):
        on = planes(stage, cuts, Hs, Ws, Hd, Wd, 0, seed, edge_window)
        gather = planes(stage, cuts, Hs, Ws, Hd, Wd, 2, seed, edge_window)
    with separable(False):
        off = planes(stage, cuts, Hs, Ws, Hd, Wd, 0, seed, edge_window)
    with separable(SCATTER_ORDER):
        keep = planes(stage, cuts, Hs, Ws, Hd, Wd, 0, seed, edge_window)
    assert rel_l2(keep, off) < 1e-5 and bool(((keep == 0) == (off == 0)).all())
    for i in range(len(cuts) if LOCKSTEP else 0):          # assertion 7, in every case of this file, eligible cutout or not
        assert same(keep[i], off[i]), ("the scatter-order setting must keep the scatter's bits", stage, i, int((th.bits(keep[i]) != th.bits(off[i])).sum()))
    return on, off, gather


def gates(stage, cuts, Hs, Ws, Hd, Wd, seed, name, **kw):
    """assertions 1 and 3: tc.run_stage's gates for forms 0 and 2 with the switch on, for form 0 with the switch off"""
    with separable(True):
        _, _, res = run_stage(stage, cuts, Hs, Ws, Hd, Wd, seed=seed, forms=[0, 2], name=f"sep-{name}", **kw)
    with separable(False):
        run_stage(stage, cuts, Hs, Ws, Hd, Wd, seed=seed, forms=[0], name=f"sep-off-{name}", **kw)
    return res


# ================================================================================================ axis-aligned cutouts
# (source pixels per destination pixel (x, y), shift of the sampled region's centre as a fraction of the source size, flavour, mode)
GENERIC = [((1.3, 1.3), (0.10, -0.10), GRID_AFFINE, M_ZEROS),               # minify
           ((1 / 0.95, 1 / 0.95), (0.25, 0.20), GRID_AFFINE, M_FILL),       # RandomAffine's scale
           ((0.5, 0.5), (0.42, -0.40), GRID_AFFINE_AC, M_ZEROS),            # x2, the zoom set's upper end
           ((0.25, 0.25), (-0.47, 0.45), GRID_AFFINE_AC, M_FILL),           # x4
           ((-0.8, 0.9), (0.20, 0.15), GRID_AFFINE, M_FILL),                # flipped in x
           ((0.7, -1.1), (-0.15, -0.20), GRID_AFFINE_AC, M_ZEROS)]          # flipped in y


def axis_cut(Hs, Ws, Hd, Wd, scale, shift, gtype, mode, off=0.0, fill=0.4):
    """an axis-aligned affine cutout; the off-diagonal words are SET (+off in the u row, -off in the v row), not left to the inverse"""
    P = pixel_map(Hs, Ws, Hd, Wd, scale=scale, shift=(shift[0] * Ws, shift[1] * Hs))
    m = norm_matrix(P, gtype, Hs, Ws, Hd, Wd)
    m[1], m[3] = off, -off
    return Cut(m, gtype, mode, fill)


def generic_cuts(Hs, Ws, Hd, Wd, off):
    cuts = [axis_cut(Hs, Ws, Hd, Wd, sc, sh, g, m, off) for sc, sh, g, m in GENERIC]
    fr = [tc.outside_fraction(c, Hs, Ws, Hd, Wd) for c in cuts]
    assert all(f < 0.99 for f in fr) and sum(f > 0.1 for f in fr) >= 4, ("a visible share of the samples must fall outside the source", fr)
    return cuts


@pytest.mark.parametrize("stage", [1, 2])
@pytest.mark.parametrize("Hs,Ws,Hd,Wd", tc.SMALL)
@pytest.mark.parametrize("off", [0.0, 4e-19, 1e-16], ids=["exact", "4e-19", "1e-16"])
def test_axis_aligned_cutouts_take_the_separable_path_and_equal_the_gather(off, Hs, Ws, Hd, Wd, stage):
    """both affine flavours x zeros / fill, scales 1.3, 1 / 0.95, 0.5, 0.25 and a flip in either axis, shifted partly off the source;
    off-diagonal words exactly zero and +-4e-19 / +-1e-16, the noise the zoom set's resized crop really carries"""
    if stage == 2:
        Wd = Hd
    cuts = generic_cuts(Hs, Ws, Hd, Wd, off)
    res = gates(stage, cuts, Hs, Ws, Hd, Wd, seed=7 + Hs, name=f"generic-{Hs}x{Ws}-{off:g}")
    assert same(res[0], res[2]), "every cutout of the launch is eligible: the summed result of form 0 must equal form 2's too"
    on, off_, gather = three_ways(stage, cuts, Hs, Ws, Hd, Wd, seed=11 + Hs)
    for i in range(len(cuts)):
        assert same(on[i], gather[i]), ("separable path differs from form 2", stage, i, int((th.bits(on[i]) != th.bits(gather[i])).sum()))
    assert not same(on, off_), "the switch changed nothing: the separable path did not run"
    assert rel_l2(on, off_) < 1e-5            # the two orders of the same fp32 sum
    if off == 0.0:
        check_scatter_order(stage, cuts, range(len(cuts)), Hs, Ws, Hd, Wd, seed=11 + Hs)


@pytest.mark.parametrize("stage", [1, 2])
@pytest.mark.parametrize("Hs,Ws,Hd,Wd", tc.SMALL)
def test_off_diagonals_of_1e_6_stay_on_the_scatter(Hs, Ws, Hd, Wd, stage):
    """the same matrices with off-diagonal words of +-1e-6: not axis-aligned, refused by the pre-filter"""
    if stage == 2:
        Wd = Hd
    cuts = generic_cuts(Hs, Ws, Hd, Wd, 1e-6)
    gates(stage, cuts, Hs, Ws, Hd, Wd, seed=3 + Hs, name=f"offdiag-{Hs}x{Ws}")
    on, off_, _ = three_ways(stage, cuts, Hs, Ws, Hd, Wd, seed=5 + Hs)
    assert same(on, off_), "a cutout that is not axis-aligned must run the scatter whatever the switch says"


@pytest.mark.parametrize("stage", [1, 2])
def test_integer_shift_at_scale_one_is_bit_identical_on_every_path(stage):
    """u = x - 3, v = y + 2 on a corner-aligned grid (9x9 source, 17x17 destination: 8 and 16 intervals, every operation of
    project() exact): every weight is 0 or 1, one term per source pixel, so on, off and form 2 agree bit for bit; half of the
    destination samples outside"""
    Hs = Ws = 9
    Hd = Wd = 17
    kx, ky = -3.0, 2.0
    # x = 8 (xn + 1), gx = 2 (x + kx) / 8 - 1 = 2 xn + 1 + kx / 4
    m = [2.0, 0.0, 1.0 + kx / 4, 0.0, 2.0, 1.0 + ky / 4, 0.0, 0.0, 1.0]
    u, v = tpass.project_frozen(m, GRID_AFFINE_AC, Wd, Hd, Ws, Hs)
    assert torch.equal(u, torch.arange(Wd, dtype=torch.float32).expand(Hd, Wd) + kx)
    assert torch.equal(v, (torch.arange(Hd, dtype=torch.float32) + ky)[:, None].expand(Hd, Wd))
    cuts = [Cut(m, GRID_AFFINE_AC, M_ZEROS), Cut(m, GRID_AFFINE_AC, M_FILL, 0.4)]
    gates(stage, cuts, Hs, Ws, Hd, Wd, seed=2, name="integer-shift")
    on, off_, gather = three_ways(stage, cuts, Hs, Ws, Hd, Wd, seed=4)
    assert same(on, gather) and same(on, off_)
    assert float(on.abs().max()) > 0


@pytest.mark.parametrize("stage", [1, 2])
def test_box_beyond_the_table_cap_falls_back_and_x4_does_not(stage):
    """104x104 destination over a 20x20 source, the sampled region centred on source pixel (6, 6).  Scale 1/6: a tile whose raw
    rectangle spans 14 source pixels or more inside the sampled region has a box of 85+ columns or rows, beyond SEP_CAP -> scatter.
    Stage A (tiles at source 0..15): the tiles of rows 0..15 or columns 0..15, i.e. all that anything reaches.  Stage B (window at
    (5, 3) of the stage-A image, tiles of that image): the tiles of image rows 0..15 hold source rows 0..12, raw rectangle [-1, 13]:
    ~87 rows; its columns split 11 + 9, boxes below the cap.  Scale 1/4: ~70 -> the separable path"""
    Hs = Ws = 20
    Hd = Wd = 104
    six = [axis_cut(Hs, Ws, Hd, Wd, (1 / 6.0, 1 / 6.0), (-0.175, -0.175), GRID_AFFINE, M_ZEROS),
           axis_cut(Hs, Ws, Hd, Wd, (1 / 6.0, 1 / 6.0), (-0.175, -0.175), GRID_AFFINE_AC, M_FILL)]
    four = [axis_cut(Hs, Ws, Hd, Wd, (0.25, 0.25), (0.1, -0.1), GRID_AFFINE, M_FILL)]
    cuts = six + four
    gates(stage, cuts, Hs, Ws, Hd, Wd, seed=6, name="cap")
    on, off_, gather = three_ways(stage, cuts, Hs, Ws, Hd, Wd, seed=8)
    first = torch.zeros(on.shape[-2:], dtype=torch.bool)
    first[:16, :] = True                                # every source pixel of a tile whose box is beyond the cap
    if stage == 1:
        first[:, :16] = True
    for i in range(len(six)):
        assert same(on[i][:, first], off_[i][:, first]), ("a box beyond the cap must take the scatter", i)
        assert float(on[i][:, first].abs().max()) > 0
    assert same(on[2], gather[2]) and not same(on[2], off_[2]), "x4 magnification must stay on the separable path"
    check_scatter_order(stage, cuts, [2], Hs, Ws, Hd, Wd, seed=8)


@pytest.mark.parametrize("stage", [1, 2])
def test_mixed_launch_the_branch_does_not_leak_between_cutouts(stage):
    """a separable cutout, a perspective one, a rotated affine, an axis-aligned affine under border padding and an exact copy side by
    side (stage B: the window touches the right and the bottom image edge): the first equals form 2 and differs from the scatter, the
    others are the scatter's bits whatever the switch says"""
    Hs, Ws = 20, 37
    Hd, Wd = (20, 37) if stage == 1 else (17, 17)
    sc = ((Ws - 1) / (Wd - 1) * 1.06, (Hs - 1) / (Hd - 1) * 1.06)
    persp = pixel_map(Hs, Ws, Hd, Wd, scale=sc, shift=(1.5, -1.0), persp=(0.3 / (Wd - 1), 0.2 / (Hd - 1)))
    rot = pixel_map(Hs, Ws, Hd, Wd, scale=sc, rot_deg=5.0, shift=(-1.0, 1.5))
    cuts = [axis_cut(Hs, Ws, Hd, Wd, (0.6, 0.55), (0.1, -0.1), GRID_AFFINE, M_FILL),          # magnifying: several terms per source pixel
            Cut(norm_matrix(persp, GRID_MESH, Hs, Ws, Hd, Wd), GRID_MESH, M_ZEROS),
            Cut(norm_matrix(rot, GRID_AFFINE, Hs, Ws, Hd, Wd), GRID_AFFINE, M_ZEROS),
            axis_cut(Hs, Ws, Hd, Wd, (sc[0] * 1.1, sc[1] * 1.1), (-0.05, 0.04), GRID_AFFINE_AC, M_BORDER),
            Cut(desc_words()[:9], 0, M_COPY)]
    edge = stage == 2
    gates(stage, cuts, Hs, Ws, Hd, Wd, seed=9, name="mixed", positive_g=False, edge_window=edge)
    on, off_, gather = three_ways(stage, cuts, Hs, Ws, Hd, Wd, seed=10, edge_window=edge)
    assert same(on[0], gather[0]) and not same(on[0], off_[0])
    for i in range(1, len(cuts)):
        assert same(on[i], off_[i]), ("the switch changed a cutout that is not eligible", i)
    assert float(on[4].abs().max()) > 0
    check_scatter_order(stage, cuts, [0], Hs, Ws, Hd, Wd, seed=10, edge_window=edge)


def test_one_iteration_descriptor_table_with_the_switch_on_and_off():
    """sample_cutout_params(8, 32) + build_descriptors (4 zoom cutouts: resized crop with the 8x8 solve's off-diagonal noise on stage B;
    4 wide ones: RandomAffine on stage A) through MakeCutouts -> prx_cutouts_backward, switch on and off: both against the oracle at
    tests/test_path_gpu.py's make-cutouts gate, and against each other at the same gate"""
    gen = torch.Generator().manual_seed(31)
    cutn, S, HW = 8, 32, 40
    img = torch.rand(1, 3, HW, HW, generator=gen)
    prm = pc.sample_cutout_params(cutn, S, gen, iteration=2)
    prm["noise"] = torch.randn(cutn, 3, S, S, generator=gen)
    gout = torch.randn(cutn, 3, S, S, generator=gen)
    desc = pc.build_descriptors(prm, S)
    zoom_b = desc[:int(0.6 * cutn)]
    assert bool((zoom_b[:, 26 + 1] == GRID_AFFINE_AC).all()) and float(zoom_b[:, [9 + 1, 9 + 3]].abs().max()) < 1e-12
    img_ref = img.clone().requires_grad_(True)
    ref = cutouts_ref.make_cutouts(img_ref, prm, S)
    (gref,) = torch.autograd.grad(ref, img_ref, gout)
    grads = {}
    for on in (True, False):
        with separable(on):
            mk = pc.MakeCutouts(S, cutn)
            mk.fixed_params = prm
            x = dev(img).requires_grad_(True)
            out = mk(x)
            (gd,) = torch.autograd.grad(out, x, dev(gout))
            grads[on] = gd.detach().cpu().clone()
        assert rel_l2(grads[on], gref) < 3e-3 and tc_cosine(grads[on], gref) > 0.99999, (on, rel_l2(grads[on], gref))
    with separable(SCATTER_ORDER):
        mk = pc.MakeCutouts(S, cutn)
        mk.fixed_params = prm
        x = dev(img).requires_grad_(True)
        (gd,) = torch.autograd.grad(mk(x), x, dev(gout))
    assert rel_l2(gd.detach().cpu(), grads[False]) < 1e-5
    assert not LOCKSTEP or same(gd.detach().cpu(), grads[False]), "the scatter-order setting must keep the scatter's bits"
    assert rel_l2(grads[True], grads[False]) < 3e-3 and tc_cosine(grads[True], grads[False]) > 0.99999
    assert not same(grads[True], grads[False]), "the switch changed nothing in a launch with eligible cutouts"


def tc_cosine(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a @ b) / (a.norm() * b.norm()))


def test_switch_returns_the_previous_value_and_queries():
    lib = _lib.load()
    start = lib.prx_cutout_bwd_separable(-1)
    try:
        assert lib.prx_cutout_bwd_separable(0) == start and lib.prx_cutout_bwd_separable(-1) == 0
        assert lib.prx_cutout_bwd_separable(1) == 0 and lib.prx_cutout_bwd_separable(-1) == 1
        assert lib.prx_cutout_bwd_separable(2) == 1 and lib.prx_cutout_bwd_separable(-1) == 2
        assert lib.prx_cutout_bwd_separable(7) == 2 and lib.prx_cutout_bwd_separable(-1) == 2
    finally:
        lib.prx_cutout_bwd_separable(start)
    assert lib.prx_cutout_bwd_separable(-1) == start


# ================================================================================================ the emulated subset
def emu_subset():
    """tests/test_cutout_separable_cpu.py: everything above on the emulated kernels (setting 2 by value: see LOCKSTEP)"""
    global LOCKSTEP
    LOCKSTEP = False
    try:
        _emu_subset()
    finally:
        LOCKSTEP = True


def _emu_subset():
    for stage in (1, 2):
        for shape in tc.SMALL:
            for off in (0.0, 4e-19, 1e-16):
                test_axis_aligned_cutouts_take_the_separable_path_and_equal_the_gather(off, *shape, stage)
            test_off_diagonals_of_1e_6_stay_on_the_scatter(*shape, stage)
        test_integer_shift_at_scale_one_is_bit_identical_on_every_path(stage)
        test_box_beyond_the_table_cap_falls_back_and_x4_does_not(stage)
        test_mixed_launch_the_branch_does_not_leak_between_cutouts(stage)
    test_one_iteration_descriptor_table_with_the_switch_on_and_off()
    test_switch_returns_the_previous_value_and_queries()
