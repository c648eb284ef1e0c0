"""Kernel-level float64 tests (GPU) of the cutout stages of csrc/cutouts.hip, one stage at a time: pool, rescale, stage A, stage B
(+ colour jitter + noise), forward and backward, and ALL THREE forms of the two warp backwards (0 workgroup scatter, 1 one-wave
scatter, 2 per-pixel gather) -- through `prx_k_*` -> the launchers `prx_cutouts_forward / _backward` call, with the form passed
explicitly instead of through the PRX_CUTOUT_BWD environment switch.

Method (helpers imported from tests/test_kernels_half_gpu.py / test_kernels_runner_gpu.py): outputs are pre-filled with NaN and carry
spare rows that must come back untouched; descriptors are written by hand (36 fp64 words, include/prx.h); the reference of a warp
stage is plain torch on the CPU in FLOAT64 -- the normalised grid built from the descriptor's matrix and grid flavour,
`F.grid_sample` with the padding mode / align_corners the mode prescribes, fill = zeros + (1 - warp(ones)) * fill, the stage-B
window a slice of the stage-A image, backwards through autograd.  Nothing of `project` / `make_taps` is restated.

Gates (none tuned against a kernel's output):

* forward, by counting (rule R2 of the runner file): |out - ref64| <= k * 2^-24 * (warp(|src|) + |fill|) + (du + dv) * D.
  The first term is the fp32 rounding of the four-tap sum, k counted at `FWD_K`; du, dv are the counted fp32 errors of the sampling
  coordinate (`coord_delta`) and D the largest difference between horizontally / vertically adjacent pixels of the (padded) source:
  bilinear sampling is continuous in the coordinate under every padding mode with slope <= D, so the bound holds everywhere.
* backward, rule R3 (reference against reference, evaluated in the test), for each of the three forms:
  rel-L2 <= 4 x the rel-L2 error of torch's own fp32 grid_sample backward (fp32 grid: F.affine_grid for the affine flavours, the
  rounded float64 meshgrid transform for the others) against the float64 gradient of the same case; and elementwise
  |err_i| <= c * (A^T|g|)_i + floor, A^T|g| = the float64 backward of |g|, c = 4 x the worst ratio torch-fp32 shows on the case,
  floor = (du + dv)_max * max|g| * K: a tap weight is off by at most the coordinate error whatever its size, and at most
  K = 4 * ceil(max_i (A^T 1)_i) + 4 destination pixels touch one source pixel (a footprint has four taps, their weights sum to 1).
  Each form runs twice: bit-identical.
* pool / rescale: R2 with the chains counted beside each use; argmax bit for bit.
* colour path (forward value, `grgb` = the pull-back through the jitter, final `ga`): R3 against a float64 evaluation of
  oracle/cutouts_ref.py's kornia ops (autograd Jacobian), rel-L2 and max-abs <= 4 x what the same ops in torch fp32 show; pixels
  the float64 reference places within 1e-4 of a kink of the Jacobian (max - min tiny but non-zero, two channels nearly tied, a
  hue-sector boundary, the saturation clamp) are left out of the Jacobian comparison and must be < 2 % of the case.

Ratios measured on an MI355X (worst kernel error / gate over the file; `python -m pytest -s` prints each): forward 0.30; backward
rel-L2 0.25 / 0.26 / 0.26 and elementwise 0.25 / 0.25 / 0.25 for forms 0 / 1 / 2 (i.e. the kernels' error equals torch-fp32's own);
colour forward 0.20, `grgb` 0.23, `ga` 0.26 (all three forms).  Every form was bit-identical between its two runs.

Mutation check on the emulated kernels: the high-edge mirror dropped, the HEAVY cooperative result not written back, one wave's
accumulator plane omitted (test_warp_every_mode_and_flavour) and a spot-masked cell left un-skipped in the pool backward
(test_pool_fwd_bwd) are caught.  Three are NOT, and cannot be by a value test: `eps = 0` in tile_intervals and truncation without the
+-0.25 in preimage_box only drop candidates whose raw coordinate sits on the boundary of a rectangle that already carries a whole
pixel of margin, i.e. whose tap weight is zero to rounding; and ignoring `sat_first` in the Jacobian kernel changes nothing beyond
rounding because the saturation scaling and the hue shift commute in HSV space (the round trip between them is the identity)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from pixray_amd._lib import PrxError, call

import test_kernels_half_gpu as th
import test_kernels_runner_gpu as tr
from test_kernels_half_gpu import guarded, untouched, within, rel_l2
from test_kernels_runner_gpu import stream, sync, check_f32

from oracle import cutouts_ref as cref

DEV = "cuda"          # tests/test_emu_cpu.py switches this (and the helper modules') to "cpu" for the emulated kernels
EPS32 = 2.0 ** -24
NAN = float("nan")
GRID_MESH, GRID_AFFINE, GRID_AFFINE_AC, GRID_MESH_AC = 0, 1, 2, 3
GRIDS = [GRID_MESH, GRID_AFFINE, GRID_AFFINE_AC, GRID_MESH_AC]
M_COPY, M_ZEROS, M_BORDER, M_REFLECT, M_FILL, M_REFLECT_AC = 0, 1, 2, 3, 4, 5
MODES = [M_ZEROS, M_BORDER, M_REFLECT, M_FILL, M_REFLECT_AC]
MODE_IDS = ["zeros", "border", "reflection", "fill", "reflection_ac"]
PAD = {M_ZEROS: "zeros", M_BORDER: "border", M_REFLECT: "reflection", M_FILL: "zeros", M_REFLECT_AC: "reflection"}
FORMS = [0, 1, 2]
# fp32 roundings of the four-tap sum (sample_plane): e = 1 - wx, s = 1 - wy (1 each, shared), the weight product (1), value * weight
# (1), three additions (3) -> at most 7 on any term; + the fill term's own chain (coverage: 3 per product, 3 additions; 1 - c; * fill;
# the final addition: 9 on |fill|).  One k for both: 9.
FWD_K = 9
FIGURES = {}          # name -> worst (error / gate) seen, printed by the tests (`pytest -s`)


def dev(t):
    return t.to(DEV)


def fig(name, ratio):
    FIGURES[name] = max(FIGURES.get(name, 0.0), float(ratio))
    print(f"[cutouts-fig] {name} {float(ratio):.4f}")


# ================================================================================================ descriptors, by hand
def desc_words(m1=None, m2=None, mode1=M_COPY, mode2=M_COPY, fill=0.0, jit=0, sat=1.0, hue=0.0, sat_first=0, noise=0.0, grid1=0,
               grid2=0, win=(0, 0, 0, 0), seed=0):
    """the 36 fp64 words of include/prx.h"""
    eye = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    w = list(eye if m1 is None else m1) + list(eye if m2 is None else m2)
    w += [mode1, mode2, fill, jit, sat, hue, sat_first, noise, grid1, grid2, win[0], win[1], win[2], win[3], seed, 0, 0, 0]
    assert len(w) == 36
    return [float(v) for v in w]


def desc_tensor(rows):
    return dev(torch.tensor(rows, dtype=torch.float64).contiguous())


def pixel_map(Hs, Ws, Hd, Wd, scale=(1.0, 1.0), rot_deg=0.0, shift=(0.0, 0.0), persp=(0.0, 0.0)):
    """destination pixel (x, y, 1) -> source pixel (u, v, w): scale (source pixels per destination pixel), rotation and shift about
    the two image centres; persp = the denominator's slope per destination pixel (denominator 1 at the destination centre)"""
    cd = ((Wd - 1) / 2.0, (Hd - 1) / 2.0)
    cs = ((Ws - 1) / 2.0 + shift[0], (Hs - 1) / 2.0 + shift[1])
    c, s = math.cos(math.radians(rot_deg)), math.sin(math.radians(rot_deg))
    L = torch.tensor([[scale[0] * c, -scale[1] * s, 0.0], [scale[0] * s, scale[1] * c, 0.0], [persp[0], persp[1], 1.0]], dtype=torch.float64)
    Tdst = torch.tensor([[1.0, 0.0, -cd[0]], [0.0, 1.0, -cd[1]], [0.0, 0.0, 1.0]], dtype=torch.float64)
    Tsrc = torch.tensor([[1.0, 0.0, cs[0]], [0.0, 1.0, cs[1]], [0.0, 0.0, 1.0]], dtype=torch.float64)
    return Tsrc @ L @ Tdst


def norm_matrix(P, gtype, Hs, Ws, Hd, Wd):
    """the descriptor matrix (normalised destination -> normalised source, as the flavour's kornia call builds its grid and
    F.grid_sample unnormalises it) of a pixel map P: test INPUT construction, the reference below goes the other way"""
    if gtype == GRID_AFFINE:
        D = torch.tensor([[2.0 / Wd, 0.0, 1.0 / Wd - 1.0], [0.0, 2.0 / Hd, 1.0 / Hd - 1.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    else:
        D = torch.tensor([[2.0 / (Wd - 1), 0.0, -1.0], [0.0, 2.0 / (Hd - 1), -1.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    if gtype >= GRID_AFFINE_AC:
        U = torch.tensor([[(Ws - 1) / 2.0, 0.0, (Ws - 1) / 2.0], [0.0, (Hs - 1) / 2.0, (Hs - 1) / 2.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    else:
        U = torch.tensor([[Ws / 2.0, 0.0, Ws / 2.0 - 0.5], [0.0, Hs / 2.0, Hs / 2.0 - 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)
    M = torch.linalg.inv(U) @ P @ torch.linalg.inv(D)
    return (M / M[2, 2]).flatten().tolist() if abs(float(M[2, 2])) > 1e-12 else M.flatten().tolist()


# ================================================================================================ the float64 reference of a warp stage
def _unnorm(g, n, ac):
    return (g + 1.0) / 2.0 * (n - 1) if ac else (g + 1.0) * n / 2.0 - 0.5


def _renorm(u, n, ac):
    return 2.0 * u / (n - 1) - 1.0 if ac else (2.0 * u + 1.0) / n - 1.0


def ref_grid(m, gtype, mode, Hs, Ws, Hd, Wd, dtype=torch.float64):
    """(grid [1,Hd,Wd,2] for F.grid_sample, its align_corners flag, raw pixel coordinates u, v in float64).
    dtype float32: the grid as torch itself builds it in fp32 (F.affine_grid for the affine flavours; the float64 meshgrid transform
    rounded to fp32 for the others, as kornia's warp_perspective does)."""
    M = torch.tensor(m, dtype=torch.float64).view(3, 3)
    xs, ys = torch.arange(Wd, dtype=torch.float64), torch.arange(Hd, dtype=torch.float64)
    fl_ac = gtype >= GRID_AFFINE_AC
    if gtype in (GRID_AFFINE, GRID_AFFINE_AC):
        xn = (2.0 * xs + 1.0) / Wd - 1.0 if gtype == GRID_AFFINE else 2.0 * xs / (Wd - 1) - 1.0
        yn = (2.0 * ys + 1.0) / Hd - 1.0 if gtype == GRID_AFFINE else 2.0 * ys / (Hd - 1) - 1.0
    else:
        xn, yn = 2.0 * xs / (Wd - 1) - 1.0, 2.0 * ys / (Hd - 1) - 1.0
    gy_, gx_ = torch.meshgrid(yn, xn, indexing="ij")
    X = M[0, 0] * gx_ + M[0, 1] * gy_ + M[0, 2]
    Y = M[1, 0] * gx_ + M[1, 1] * gy_ + M[1, 2]
    if gtype in (GRID_MESH, GRID_MESH_AC):
        Z = M[2, 0] * gx_ + M[2, 1] * gy_ + M[2, 2]
        sc = torch.where(Z.abs() > 1e-8, 1.0 / Z, torch.ones_like(Z))          # kornia convert_points_from_homogeneous
        X, Y = X * sc, Y * sc
    u, v = _unnorm(X, Ws, fl_ac), _unnorm(Y, Hs, fl_ac)
    if dtype == torch.float32:
        if gtype in (GRID_AFFINE, GRID_AFFINE_AC):
            g = F.affine_grid(M[:2].float()[None], [1, 3, Hd, Wd], align_corners=(gtype == GRID_AFFINE_AC))[0]
            X, Y = g[..., 0], g[..., 1]
        else:
            X, Y = X.float(), Y.float()
    # reflection reflects about the pixel centres (mode 5) or the pixel edges (mode 3) whatever the flavour's unnormalisation: hand
    # grid_sample the SAME pixel coordinate under the flag the mode needs
    ac = {M_REFLECT: False, M_REFLECT_AC: True}.get(mode, fl_ac)
    if ac != fl_ac:
        X, Y = _renorm(_unnorm(X, Ws, fl_ac), Ws, ac), _renorm(_unnorm(Y, Hs, fl_ac), Hs, ac)
    return torch.stack([X, Y], dim=-1)[None].to(dtype), ac, u, v


def ref_warp(src, m, gtype, mode, fill, Hd, Wd):
    """one cutout of a warp stage in src's dtype (float64: the reference; float32: torch's own fp32 evaluation). src [1,3,Hs,Ws]"""
    if mode == M_COPY:
        return src[:, :, :Hd, :Wd]
    Hs, Ws = src.shape[-2:]
    grid, ac, _, _ = ref_grid(m, gtype, mode, Hs, Ws, Hd, Wd, src.dtype)
    out = F.grid_sample(src, grid, mode="bilinear", padding_mode=PAD[mode], align_corners=ac)
    if mode == M_FILL:
        out = out + (1.0 - F.grid_sample(torch.ones_like(src), grid, mode="bilinear", padding_mode="zeros", align_corners=ac)) * fill
    return out


def coord_delta(m, gtype, mode, n_src, coord, row):
    """counted fp32 error of the kernel's sampling coordinate along one axis (row 0: u, row 1: v), per destination pixel.
    mesh flavours: the float64 quotient rounded to fp32 (1 rounding of g, |g| * n/2 <= |u| + 0.5 + n/2), g + 1 (|u + 0.5|), * n/2
    (|u + 0.5|), - 0.5 (|u|): 4|u| + n/2 + 1.5 units; align_corners=True drops one.  affine flavours: the base grid adds 3 roundings
    (step, step * i, -1 + .) and the pixel-centre flavour 2 more, on a value <= 1, through |m_r0| + |m_r1| and the n/2 of the
    unnormalisation.  reflection: |u - mn| (|u| + 0.5), span - extra + mn (2 roundings of values <= n)."""
    a = coord.abs()
    units = 4.0 * a + n_src / 2.0 + 1.5
    if gtype in (GRID_AFFINE, GRID_AFFINE_AC):
        units = units + 5.0 * (abs(m[3 * row]) + abs(m[3 * row + 1])) * n_src / 2.0
    if mode in (M_REFLECT, M_REFLECT_AC):
        units = units + a + 0.5 + 2.0 * n_src
    return EPS32 * units


def max_adjacent_diff(src, mode, fill):
    """largest |difference| between horizontally / vertically adjacent pixels; zeros / fill padding continue the image with a
    frame of 0 / fill"""
    s = src.double()
    if mode in (M_ZEROS, M_FILL):
        s = F.pad(s, (1, 1, 1, 1), value=float(fill) if mode == M_FILL else 0.0)
    return max(float((s[..., 1:] - s[..., :-1]).abs().max()), float((s[..., 1:, :] - s[..., :-1, :]).abs().max()))


# ================================================================================================ one stage, forward and the three backward forms
class Cut:
    """one cutout's geometry of ONE stage: matrix, flavour, mode, fill"""

    def __init__(self, m, gtype, mode, fill=0.0):
        self.m, self.gtype, self.mode, self.fill = m, gtype, mode, fill


def run_stage(stage, cuts, Hs, Ws, Hd, Wd, seed, positive_g=True, forms=FORMS, edge_window=False, name=""):
    """stage 1: source [3,Hs,Ws] shared by the cutouts -> [n,3,Hd,Wd].  stage 2: per-cutout stage-A images [n,3,Hs+11,Ws+13] read
    through a window of Hs x Ws at (5, 3) (strictly inside, not a multiple of 16; `edge_window`: at (13, 11), touching the right and
    the bottom edge) -> [n,3,Hd,Hd] (Hd == Wd).  Returns (float64 forward, float64 gradient, kernel gradient of form 0)."""
    torch.manual_seed(seed)
    n = len(cuts)
    if stage == 2:
        assert Hd == Wd
        HA, WA = Hs + 11, Ws + 13
        ox, oy = (13, 11) if edge_window else (5, 3)
        src = torch.rand(n, 3, HA, WA)
        rows = [desc_words(m2=c.m, mode2=c.mode, grid2=c.gtype, fill=c.fill, win=(ox, oy, Ws, Hs)) for c in cuts]
    else:
        src = torch.rand(1, 3, Hs, Ws)
        rows = [desc_words(m1=c.m, mode1=c.mode, grid1=c.gtype, fill=c.fill) for c in cuts]
    g = torch.rand(n, 3, Hd, Wd) + 0.5 if positive_g else torch.randn(n, 3, Hd, Wd)     # [0.5, 1.5]: a dropped candidate cannot cancel
    desc = desc_tensor(rows)
    src_d, g_d = dev(src), dev(g)

    def window(s, i):
        return s[i:i + 1, :, oy:oy + Hs, ox:ox + Ws] if stage == 2 else s

    # ---- references: float64 (values, gradient, A^T|g|, A^T 1) and torch's own fp32
    s64 = src.double().requires_grad_(True)
    out64 = torch.cat([ref_warp(window(s64, i), c.m, c.gtype, c.mode, c.fill, Hd, Wd) for i, c in enumerate(cuts)])
    g64, = torch.autograd.grad(out64, s64, g.double(), retain_graph=True)
    atg, = torch.autograd.grad(out64, s64, g.double().abs(), retain_graph=True)
    at1, = torch.autograd.grad(out64, s64, torch.ones_like(out64))
    s32 = src.clone().requires_grad_(True)
    out32 = torch.cat([ref_warp(window(s32, i), c.m, c.gtype, c.mode, c.fill, Hd, Wd) for i, c in enumerate(cuts)])
    g32, = torch.autograd.grad(out32, s32, g)
    out64 = out64.detach()

    # ---- forward
    full, out = guarded(n * 3 * Hd, Wd, torch.float32)
    if stage == 1:
        call("prx_k_warp_a_fwd", src_d, Hs, Ws, desc, full, n, Hd, Wd, stream())
    else:
        call("prx_k_warp_b_fwd", src_d, HA, WA, desc, None, full, n, Hd, stream())
    sync()
    assert untouched(full, n * 3 * Hd, Wd)
    out = out.view(n, 3, Hd, Wd).cpu()
    dmax = 0.0
    for i, c in enumerate(cuts):
        w = window(src.double(), i)
        if c.mode == M_COPY:
            assert torch.equal(out[i].double(), out64[i]), "copy mode is not an exact copy"
            continue
        _, _, u, v = ref_grid(c.m, c.gtype, c.mode, Hs, Ws, Hd, Wd)
        du, dv = coord_delta(c.m, c.gtype, c.mode, Ws, u, 0), coord_delta(c.m, c.gtype, c.mode, Hs, v, 1)
        inside = (u > -1) & (u < Ws) & (v > -1) & (v < Hs)                  # footprints that touch the image: where a weight matters
        if bool(inside.any()):
            dmax = max(dmax, float((du + dv)[inside].max()))
        A = ref_warp(w.abs(), c.m, c.gtype, c.mode, abs(c.fill), Hd, Wd)[0]
        # FWD_K roundings of the four-tap sum (+ fill chain) on A; (du + dv) * D for the coordinate (see the module docstring)
        tol = FWD_K * EPS32 * A + ((du + dv) * max_adjacent_diff(w, c.mode, c.fill))[None]
        ok, worst = within(out[i], out64[i], tol)
        assert ok, ("forward off by more than the counted gate", name, stage, i, worst)
        fig(f"fwd/{name}/stage{stage}", float(((out[i].double() - out64[i]).abs() / tol.clamp_min(1e-300)).max()))

    # ---- backward gates from the references
    e32 = (g32.double() - g64).abs()
    gmax = float(g.abs().max())
    K = 4 * math.ceil(float(at1.max())) + 4
    floor = dmax * gmax * K
    zero_ref = float(g64.abs().max()) == 0.0
    pos = atg > 0
    c_el = 4.0 * float(((e32 - floor).clamp_min(0.0)[pos] / atg[pos]).max()) if bool(pos.any()) else 0.0
    rel32 = rel_l2(g32, g64)

    res = {}
    for form in forms:
        runs = []
        for rep in range(2):
            if stage == 1:
                fuv, _ = guarded(1, n * Hd * Wd * 2, torch.float32)
                fpriv, _ = guarded(n * 3 * Hs, Ws, torch.float32)
                fg, gk = guarded(3 * Hs, Ws, torch.float32)
                call("prx_k_warp_a_bwd", g_d, Hs, Ws, desc, fuv, fpriv, fg, n, Hd, Wd, form, stream())
                sync()
                assert untouched(fg, 3 * Hs, Ws) and untouched(fpriv, n * 3 * Hs, Ws) and untouched(fuv, 1, n * Hd * Wd * 2)
                runs.append(gk.view(1, 3, Hs, Ws).cpu().clone())
            else:
                fuv, _ = guarded(1, n * Hd * Hd * 2, torch.float32)
                frgb, _ = guarded(n * 3 * Hd, Hd, torch.float32)
                fg, gk = guarded(n * 3 * HA, WA, torch.float32)
                maps = dev(torch.zeros(n * 16))
                call("prx_k_warp_b_bwd", src_d, HA, WA, desc, g_d, frgb, fuv, fg, n, Hd, maps, maps.numel() * 4, form, stream())
                sync()
                assert untouched(fg, n * 3 * HA, WA) and untouched(fuv, 1, n * Hd * Hd * 2)
                assert bool(torch.isnan(frgb).all()), "grgb written for a cutout without jitter"
                runs.append(gk.view(n, 3, HA, WA).cpu().clone())
        assert torch.equal(th.bits(runs[0]), th.bits(runs[1])), ("two runs of one form differ", name, stage, form)
        gk = runs[0]
        assert bool(torch.isfinite(gk).all()), ("unwritten / non-finite gradient element", name, stage, form)
        if zero_ref:
            assert int(torch.count_nonzero(gk)) == 0, ("gradient of a fully-outside / copy-free case must be exactly zero", name, form)
        else:
            rel = rel_l2(gk, g64)
            fig(f"bwd-rel/{name}/stage{stage}/form{form}", rel / max(4.0 * rel32, 1e-300))
            assert rel <= 4.0 * rel32, ("rel-L2 beyond 4 x torch-fp32's", name, stage, form, rel, rel32)
            tol = c_el * atg + floor
            err = (gk.double() - g64).abs()
            fig(f"bwd-el/{name}/stage{stage}/form{form}", float((err / tol.clamp_min(1e-300)).max()) if float(tol.max()) > 0 else 0.0)
            ok, worst = within(gk, g64, tol)
            assert ok, ("gradient element beyond c * A^T|g| + floor", name, stage, form, worst, c_el, floor)
        res[form] = gk
    return out64, g64, res


def outside_fraction(c, Hs, Ws, Hd, Wd):
    _, _, u, v = ref_grid(c.m, c.gtype, c.mode, Hs, Ws, Hd, Wd)
    return float(((u < 0) | (u > Ws - 1) | (v < 0) | (v > Hs - 1)).double().mean())


# ---- mode x flavour at the small shapes: four cutouts (the four flavours) per launch, each with its own mild rotation + scale + shift
SMALL = [(20, 37, 17, 23), (9, 9, 40, 40), (33, 16, 17, 23)]             # (Hs, Ws, Hd, Wd)
MILD = [(5.0, 1.06, (0.05, -0.04)), (-7.0, 1.08, (-0.04, 0.05)), (4.0, 1.05, (0.06, 0.03)), (-5.0, 1.07, (-0.03, -0.05))]   # rotation, zoom, shift / size


def mild_cuts(mode, Hs, Ws, Hd, Wd, fill=0.4):
    cuts = []
    for gtype, (rot, zoom, sh) in zip(GRIDS, MILD):
        P = pixel_map(Hs, Ws, Hd, Wd, scale=(zoom * (Ws - 1) / (Wd - 1), zoom * (Hs - 1) / (Hd - 1)), rot_deg=rot, shift=(sh[0] * Ws, sh[1] * Hs))
        cuts.append(Cut(norm_matrix(P, gtype, Hs, Ws, Hd, Wd), gtype, mode, fill))
        frac = outside_fraction(cuts[-1], Hs, Ws, Hd, Wd)
        assert 0.10 <= frac <= 0.30, ("a mild case must put 10-30 % of its samples outside the source", frac)
    return cuts


@pytest.mark.parametrize("stage", [1, 2])
@pytest.mark.parametrize("Hs,Ws,Hd,Wd", SMALL)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_warp_every_mode_and_flavour(mode, Hs, Ws, Hd, Wd, stage):
    """all five padding modes x all four grid flavours, 10-30 % of the samples outside, sources 20x37 / 9x9 (smaller than one tile) /
    33x16, destinations 17x23 / 40x40 (stage B is square: Hd x Hd), g in [0.5, 1.5]; forward and the three backward forms"""
    if stage == 2:
        Wd = Hd
    run_stage(stage, mild_cuts(mode, Hs, Ws, Hd, Wd), Hs, Ws, Hd, Wd, seed=mode * 100 + Hs, name=f"mild-{MODE_IDS[MODES.index(mode)]}-{Hs}x{Ws}")


@pytest.mark.parametrize("stage", [1, 2])
@pytest.mark.parametrize("n_cut", [1, 2, 3, 4])
def test_warp_mixed_descriptors_with_a_copy_cutout(n_cut, stage):
    """n_cut 1..4, a different descriptor per cutout, one of them mode 0 (exact copy; stage A then needs equal sizes, stage B a
    window no smaller than the output); randn gradients; on stage B the window touches the right and the bottom image edge"""
    Hs, Ws = 20, 37
    Hd, Wd = (20, 37) if stage == 1 else (17, 17)
    all_cuts = [Cut(None, 0, M_COPY)] + [mild_cuts(m, Hs, Ws, Hd, Wd)[i] for i, m in [(1, M_BORDER), (2, M_FILL), (0, M_REFLECT)]]
    all_cuts[0].m = desc_words()[:9]
    order = [all_cuts[1], all_cuts[0], all_cuts[2], all_cuts[3]] if n_cut > 1 else [all_cuts[0]]
    run_stage(stage, order[:n_cut], Hs, Ws, Hd, Wd, seed=n_cut, positive_g=False, edge_window=True, name=f"mixed{n_cut}")


def special_cuts(case, Hs, Ws, Hd, Wd):
    """the geometry cases of the search logic's fallbacks"""
    def one(P, gtype, mode, fill=0.0):
        return Cut(norm_matrix(P, gtype, Hs, Ws, Hd, Wd), gtype, mode, fill)
    if case == "magnify6":           # 1/6 source pixel per destination pixel: an 18-pixel tile span has 108 x 108 > STAGE_CAP pre-images
        return [one(pixel_map(Hs, Ws, Hd, Wd, scale=(1 / 6.0, 1 / 6.0), rot_deg=3.0), GRID_MESH, M_ZEROS),
                one(pixel_map(Hs, Ws, Hd, Wd, scale=(1 / 6.0, 1 / 6.0), rot_deg=-2.0, shift=(1.5, 0.5)), GRID_AFFINE, M_REFLECT)]
    if case == "minify5_border":     # 5 source pixels per destination pixel: most of the destination is beyond the edge pixels' strips
        return [one(pixel_map(Hs, Ws, Hd, Wd, scale=(5.0, 5.0), rot_deg=2.0), GRID_MESH, M_BORDER),
                one(pixel_map(Hs, Ws, Hd, Wd, scale=(5.0, 5.0), shift=(3.0, -2.0)), GRID_AFFINE_AC, M_BORDER)]
    if case == "rot45":
        return [one(pixel_map(Hs, Ws, Hd, Wd, scale=(Ws / Wd, Hs / Hd), rot_deg=45.0), g, m, 0.3)
                for g, m in [(GRID_MESH, M_ZEROS), (GRID_AFFINE, M_REFLECT), (GRID_AFFINE_AC, M_FILL), (GRID_MESH_AC, M_BORDER)]]
    if case == "persp3to1":          # denominator 0.5 .. 1.5 across the destination width: 3 : 1, positive
        return [one(pixel_map(Hs, Ws, Hd, Wd, scale=(Ws / Wd, Hs / Hd), persp=(1.0 / (Wd - 1), 0.0)), GRID_MESH, M_REFLECT),
                one(pixel_map(Hs, Ws, Hd, Wd, scale=(Ws / Wd, Hs / Hd), persp=(0.6 / (Wd - 1), 0.4 / (Hd - 1))), GRID_MESH_AC, M_FILL, 0.6)]
    if case == "persp_horizon":      # denominator 1.97 at one corner, 0.03 at the opposite one: the inverse map's denominator passes 0.05
        k = 0.97
        return [one(pixel_map(Hs, Ws, Hd, Wd, scale=(0.8 * Ws / Wd, 0.8 * Hs / Hd), persp=(k / (Wd - 1), k / (Hd - 1))), GRID_MESH, M_ZEROS),
                one(pixel_map(Hs, Ws, Hd, Wd, scale=(0.8 * Ws / Wd, 0.8 * Hs / Hd), persp=(-k / (Wd - 1), k / (Hd - 1))), GRID_MESH_AC, M_BORDER)]
    if case == "reflect_far":        # shifted by 1.6 image sizes: samples beyond the first-order mirror images
        return [one(pixel_map(Hs, Ws, Hd, Wd, scale=(Ws / Wd, Hs / Hd), rot_deg=4.0, shift=(1.6 * Ws, -1.6 * Hs)), g, m)
                for g, m in [(GRID_MESH, M_REFLECT), (GRID_AFFINE, M_REFLECT_AC), (GRID_AFFINE_AC, M_REFLECT), (GRID_MESH_AC, M_REFLECT_AC)]]
    if case == "outside":            # the whole destination 3 image sizes away
        return [one(pixel_map(Hs, Ws, Hd, Wd, scale=(Ws / Wd, Hs / Hd), shift=(3.0 * Ws, 3.0 * Hs)), GRID_MESH, M_ZEROS),
                one(pixel_map(Hs, Ws, Hd, Wd, scale=(Ws / Wd, Hs / Hd), shift=(-3.0 * Ws, 2.0 * Hs)), GRID_AFFINE, M_FILL, 0.7)]
    if case == "singular":           # every destination pixel samples the one source point (7.3, 5.6) / (2.25, 3.5)
        return [one(pixel_map(Hs, Ws, Hd, Wd, scale=(0.0, 0.0), shift=(7.3 - (Ws - 1) / 2.0, 5.6 - (Hs - 1) / 2.0)), GRID_MESH, M_ZEROS),
                one(pixel_map(Hs, Ws, Hd, Wd, scale=(0.0, 0.0), shift=(2.25 - (Ws - 1) / 2.0, 3.5 - (Hs - 1) / 2.0)), GRID_AFFINE, M_BORDER)]
    raise KeyError(case)


SPECIAL = {"magnify6": (20, 20, 104, 104), "minify5_border": (20, 37, 40, 40), "rot45": (20, 37, 40, 40), "persp3to1": (33, 16, 40, 40),
           "persp_horizon": (20, 37, 40, 40), "reflect_far": (20, 37, 17, 23), "outside": (9, 9, 17, 23), "singular": (20, 37, 17, 23)}


def special_case(case, stage):
    Hs, Ws, Hd, Wd = SPECIAL[case]
    if stage == 2:
        Wd = Hd
    cuts = special_cuts(case, Hs, Ws, Hd, Wd)
    out64, g64, res = run_stage(stage, cuts, Hs, Ws, Hd, Wd, seed=len(case), positive_g=case != "rot45", name=case)
    if case == "outside":
        assert float(out64[0].abs().max()) == 0.0 and bool((out64[1] == 0.7).all())        # all zero / all fill (run_stage: gradient exactly 0)
        assert float(g64.abs().max()) == 0.0
    if case == "minify5_border":     # an edge pixel's strip holds more than HEAVY = 96 destination pixels: the cooperative path runs
        _, _, u, v = ref_grid(cuts[0].m, cuts[0].gtype, cuts[0].mode, Hs, Ws, Hd, Wd)
        assert int(((u < 0) & (v > 4) & (v < 5)).sum()) + int((u < -1).sum()) > 96
    return res


@pytest.mark.parametrize("stage", [1, 2])
@pytest.mark.parametrize("case", list(SPECIAL))
def test_warp_search_fallbacks(case, stage):
    """x6 magnification (a tile's pre-image beyond STAGE_CAP; destination 104 x 104), x0.2 minification under border padding (edge
    pixels beyond HEAVY), 45 degrees, two perspectives (denominator 3 : 1; denominator near zero at one corner: the search-everything
    branch), reflection beyond one image size, a destination fully outside (exact zeros / fill, gradient exactly zero), a singular map"""
    special_case(case, stage)


# ================================================================================================ refusals
def test_warp_backwards_refuse_a_scratch_that_is_too_small():
    """stage A keeps its stage maps (52 bytes per cutout) in the 3 x Hs x Ws result buffer, stage B in `maps_scratch`: refused by name,
    nothing launched, nothing written"""
    n, Hs, Ws, Hd, Wd = 1, 2, 2, 5, 5                       # 3 * 2 * 2 * 4 = 48 bytes < 52
    P = pixel_map(Hs, Ws, Hd, Wd, scale=(0.4, 0.4))
    desc = desc_tensor([desc_words(m1=norm_matrix(P, 0, Hs, Ws, Hd, Wd), mode1=M_ZEROS)])
    g = dev(torch.ones(n, 3, Hd, Wd))
    for form in (0, 1):
        fuv, _ = guarded(1, n * Hd * Wd * 2, torch.float32)
        fpriv, _ = guarded(n * 3 * Hs, Ws, torch.float32)
        fg, _ = guarded(3 * Hs, Ws, torch.float32)
        with pytest.raises(PrxError, match="too many cutouts for the stage-map scratch"):
            call("prx_k_warp_a_bwd", g, Hs, Ws, desc, fuv, fpriv, fg, n, Hd, Wd, form, stream())
        sync()
        assert bool(torch.isnan(fuv).all()) and bool(torch.isnan(fpriv).all()) and bool(torch.isnan(fg).all())
    HA, WA, S = 12, 12, 5
    desc = desc_tensor([desc_words(m2=norm_matrix(pixel_map(8, 8, S, S), 0, 8, 8, S, S), mode2=M_ZEROS, win=(2, 2, 8, 8))] * 2)
    a, g = dev(torch.rand(2, 3, HA, WA)), dev(torch.ones(2, 3, S, S))
    maps = dev(torch.full((32,), NAN))
    for form in (0, 1):
        for scratch, nbytes in [(None, 1024), (maps, 2 * 52 - 1)]:
            fuv, _ = guarded(1, 2 * S * S * 2, torch.float32)
            frgb, _ = guarded(2 * 3 * S, S, torch.float32)
            fg, _ = guarded(2 * 3 * HA, WA, torch.float32)
            with pytest.raises(PrxError, match="stage-map scratch too small"):
                call("prx_k_warp_b_bwd", a, HA, WA, desc, g, frgb, fuv, fg, 2, S, scratch, nbytes, form, stream())
            sync()
            assert bool(torch.isnan(fuv).all()) and bool(torch.isnan(frgb).all()) and bool(torch.isnan(fg).all()) and bool(torch.isnan(maps).all())
    with pytest.raises(PrxError, match="form is not one of"):
        call("prx_k_warp_b_bwd", a, HA, WA, desc, g, frgb, fuv, fg, 2, S, maps, 128, 3, stream())


# ================================================================================================ pool
def pool_ref(img, S, mask):
    """(AdaptiveAvgPool2d + AdaptiveMaxPool2d) / 2 by the written-out window formula, float64: values, first-max argmax, A"""
    C, H, W = img.shape
    x = img.double()
    val, A = torch.zeros(C, S, S, dtype=torch.float64), torch.zeros(C, S, S, dtype=torch.float64)
    arg, cnt = torch.zeros(C, S, S, dtype=torch.int32), torch.zeros(S, S, dtype=torch.int64)
    for y in range(S):
        y0, y1 = (y * H) // S, -((-(y + 1) * H) // S)
        for xx in range(S):
            x0, x1 = (xx * W) // S, -((-(xx + 1) * W) // S)
            w = x[:, y0:y1, x0:x1].reshape(C, -1)
            mx = w.max(dim=1).values
            first = torch.stack([(w[c] == mx[c]).nonzero()[0, 0] for c in range(C)])        # first max in row-major scan order
            arg[:, y, xx] = ((y0 + first // (x1 - x0)) * W + x0 + first % (x1 - x0)).int()
            val[:, y, xx] = 0.5 * (w.mean(dim=1) + mx)
            A[:, y, xx] = w.abs().mean(dim=1) + mx.abs()
            cnt[y, xx] = w.shape[1]
    if mask is not None:
        val = torch.where(mask.bool(), torch.zeros_like(val), val)
    return val, arg, A, cnt


def pool_bwd_ref(g, arg, mask, H, W, S):
    C = g.shape[0]
    ref, A = torch.zeros(C, H, W, dtype=torch.float64), torch.zeros(C, H, W, dtype=torch.float64)
    cover = torch.zeros(H, W, dtype=torch.int64)
    g64 = g.double()
    for y in range(S):
        y0, y1 = (y * H) // S, -((-(y + 1) * H) // S)
        for x in range(S):
            x0, x1 = (x * W) // S, -((-(x + 1) * W) // S)
            cover[y0:y1, x0:x1] += 1
            for c in range(C):
                if mask is not None and bool(mask[c, y, x]):
                    continue                                                                 # a masked pooled pixel is a constant
                t = 0.5 * g64[c, y, x]
                ref[c, y0:y1, x0:x1] += t / ((y1 - y0) * (x1 - x0))
                A[c, y0:y1, x0:x1] += t.abs() / ((y1 - y0) * (x1 - x0))
                a = int(arg[c, y, x])
                ref[c, a // W, a % W] += t
                A[c, a // W, a % W] += t.abs()
    return ref, A, int(cover.max())


POOL_SHAPES = [(40, 40, 64), (50, 50, 16), (64, 64, 16), (30, 52, 16)]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("H,W,S", POOL_SHAPES)
def test_pool_fwd_bwd(H, W, S, masked):
    """40 -> 64 (windows of 1-2 pixels), 50 -> 16 (overlapping windows), 64 -> 16 (exact), 30 x 52 -> 16; values quantised to 1/8 plant
    exact ties in every window (first max wins); with and without a spot mask"""
    torch.manual_seed(H + S)
    img = torch.round(torch.rand(3, H, W) * 8) / 8
    img[:, 1::7, ::3] += torch.rand(3, len(range(1, H, 7)), len(range(0, W, 3))) * 0.01            # and some windows without ties
    mask = (torch.rand(3, S, S) < 0.3).to(torch.uint8) if masked else None
    val, arg, A, cnt = pool_ref(img, S, mask)
    fp, pooled = guarded(3 * S, S, torch.float32)
    fa = torch.full((3 * S + 3, S), -7, dtype=torch.int32, device=DEV)          # spare rows behind the argmax plane, too
    am = fa[:3 * S]
    call("prx_k_pool_fwd", dev(img), fp, fa, None if mask is None else dev(mask), 3, H, W, S, stream())
    sync()
    assert untouched(fp, 3 * S, S) and bool((fa[3 * S:] == -7).all())
    assert torch.equal(am.cpu().view(3, S, S), arg), "argmax differs from the first maximum in scan order"
    # k = (cnt - 1) additions + the division + the addition of the maximum (* 0.5 is exact)
    check_f32(pooled.cpu().view(3, S, S), val, int(cnt.max()) + 1, A)
    g = torch.randn(3, S, S)
    ref, Ab, cover = pool_bwd_ref(g, arg, mask, H, W, S)
    fgi, gimg = guarded(3 * H, W, torch.float32)
    call("prx_k_pool_bwd", dev(g), dev(arg), None if mask is None else dev(mask), fgi, 3, H, W, S, stream())
    sync()
    assert untouched(fgi, 3 * H, W)
    # per covering cell: the division, its addition, the argmax addition (0.5 * g is exact): 3 roundings, `cover` cells at most
    check_f32(gimg.cpu().view(3, H, W), ref, 3 * cover, Ab)
    if masked:
        assert float(ref.abs().max()) > 0


# ================================================================================================ rescale
RESCALE_SHAPES = [(16, 16, 29), (16, 23, 16), (16, 16, 16)]


@pytest.mark.parametrize("S,Hb,Wb", RESCALE_SHAPES)
def test_rescale_fwd_bwd(S, Hb, Wb):
    """F.interpolate(bilinear, align_corners=False) of [3,S,S] to [3,Hb,Wb] in float64, and its autograd gradient"""
    torch.manual_seed(Hb * Wb)
    p = torch.randn(3, S, S)
    p64 = p.double().requires_grad_(True)
    ref = F.interpolate(p64[None], size=(Hb, Wb), mode="bilinear", align_corners=False)
    A = F.interpolate(p.double().abs()[None], size=(Hb, Wb), mode="bilinear", align_corners=False)[0]
    fb, base = guarded(3 * Hb, Wb, torch.float32)
    call("prx_k_rescale_fwd", dev(p), fb, 3, S, Hb, Wb, stream())
    sync()
    assert untouched(fb, 3 * Hb, Wb)
    # the source coordinate (o + 0.5) * (S / out) - 0.5: the quotient (1 rounding), the product (1), the subtraction (1), on a value
    # <= S: 3 * 2^-24 * S per axis; a weight is off by that much, times the largest adjacent difference
    delta = 3 * EPS32 * S
    D = max(float((p[..., 1:] - p[..., :-1]).abs().max()), float((p[..., 1:, :] - p[..., :-1, :]).abs().max()))
    # k: 1 - w (1), the inner products (1) and sum (1), the outer product (1) and sum (1), twice nested: 6 on any term
    tol = 6 * EPS32 * A + 2 * delta * D
    ok, worst = within(base.cpu().view(3, Hb, Wb), ref[0].detach(), tol)
    assert ok, ("rescale forward off by more than the counted chain", worst)
    g = torch.randn(3, Hb, Wb)
    gref, = torch.autograd.grad(ref, p64, g.double()[None], retain_graph=True)
    Ab, = torch.autograd.grad(ref, p64, g.double().abs()[None])
    fg, gp = guarded(3 * S, S, torch.float32)
    call("prx_k_rescale_bwd", dev(g), fg, 3, S, Hb, Wb, stream())
    sync()
    assert untouched(fg, 3 * S, S)
    # contributors of one pooled pixel: destination pixels with source coordinate in (s - 1, s + 1): at most ceil(2 out / S) + 1 per
    # axis; each adds g * w with w a sum of <= 4 weight products (3 roundings each + 3 additions) and one accumulation: k = 8 per
    # contributor on A^T|g|, and every weight is off by <= 2 * delta
    cnt = (math.ceil(2 * Hb / S) + 1) * (math.ceil(2 * Wb / S) + 1)
    tol = 8 * cnt * EPS32 * Ab + 2 * delta * cnt * float(g.abs().max())
    ok, worst = within(gp.cpu().view(3, S, S), gref, tol)
    assert ok, ("rescale backward off by more than the counted chain", worst)


# ================================================================================================ stage-B colour path
ORDERINGS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
JITTER = [(1, 0.3, 0.4), (1, 1.7, -0.4), (1, 0.3, -0.4), (1, 1.7, 0.4), (0, 1.0, 0.0), (1, 1.7, 0.4)]      # (on, saturation, hue rad)
KINK = 1e-4


def jitter_ref(x, sat, hue, sat_first, kink=None):
    """kornia's saturation / hue ops as oracle/cutouts_ref.py states them, in x's dtype.  `kink` (a list): collects the float64
    reference's own distance-to-kink masks -- max - min tiny but non-zero or two channels nearly tied (the max / min selection),
    a hue-sector boundary of hsv_to_rgb, the saturation clamp; exactly gray pixels take the same tie branch on both sides and are kept"""
    def near(img_rgb, hsv_after, s_scaled):
        srt = img_rgb.sort(dim=1).values
        gaps = torch.minimum(srt[:, 1] - srt[:, 0], srt[:, 2] - srt[:, 1])
        gray = (srt[:, 2] - srt[:, 0]) == 0
        k = (~gray) & (gaps < KINK)
        h6 = hsv_after[:, 0] / cref.TWO_PI * 6
        k |= (~gray) & ((h6 - h6.round()).abs() < KINK)
        if s_scaled is not None:
            k |= (~gray) & ((s_scaled - 1.0).abs() < KINK)
        return k

    def sat_op(img):
        hsv = cref.rgb_to_hsv(img)
        s = hsv[:, 1:2] * sat
        out_hsv = torch.cat([hsv[:, 0:1], torch.clamp(s, 0.0, 1.0), hsv[:, 2:3]], dim=1)
        if kink is not None:
            kink.append(near(img.detach(), out_hsv.detach(), s.detach()[:, 0]))
        return cref.hsv_to_rgb(out_hsv)

    def hue_op(img):
        hsv = cref.rgb_to_hsv(img)
        out_hsv = torch.cat([torch.fmod(hsv[:, 0:1] + hue, cref.TWO_PI), hsv[:, 1:2], hsv[:, 2:3]], dim=1)
        if kink is not None:
            kink.append(near(img.detach(), out_hsv.detach(), None))
        return cref.hsv_to_rgb(out_hsv)
    return hue_op(sat_op(x)) if sat_first else sat_op(hue_op(x))


def colour_case(sat_first, S=24, HA=37, WA=41):
    """six cutouts: channel levels 0.2 / 0.5 / 0.8 +- 0.05 in the six orderings (the gaps survive bilinear mixing); a mild zoom under
    fill padding (fully uncovered pixels: exactly gray, kept in the comparison); saturation 0.3 and 1.7 (the clamp
    at 1 is active), hue +-0.4 rad, one cutout without jitter"""
    torch.manual_seed(11 + sat_first)
    n, Hs, Ws, ox, oy = 6, 22, 25, 7, 5
    a = torch.empty(n, 3, HA, WA)
    for i, o in enumerate(ORDERINGS):
        for c in range(3):
            a[i, c] = (0.2, 0.5, 0.8)[o[c]] + (torch.rand(HA, WA) - 0.5) * 0.1
    cuts, rows = [], []
    for i in range(n):
        # fill padding only: under zeros padding an uncovered pixel is black, where d(saturation)/d(rgb) = 1 / 1e-8 swamps any gate
        gtype, mode = GRIDS[i % 4], M_FILL
        P = pixel_map(Hs, Ws, S, S, scale=(1.15 * Ws / S, 1.15 * Hs / S), rot_deg=3.0 * (i - 2), shift=(0.5 * i, -0.4 * i))
        cuts.append(Cut(norm_matrix(P, gtype, Hs, Ws, S, S), gtype, mode, 0.5))
        on, sat, hue = JITTER[i]
        rows.append(desc_words(m2=cuts[-1].m, mode2=mode, grid2=gtype, fill=0.5, jit=on, sat=sat, hue=hue, sat_first=sat_first,
                               win=(ox, oy, Ws, Hs)))
    g = torch.randn(n, 3, S, S)

    def evaluate(dtype):
        s = a.to(dtype).requires_grad_(True)
        smp, outs, kinks = [], [], []
        for i, c in enumerate(cuts):
            x = ref_warp(s[i:i + 1, :, oy:oy + Hs, ox:ox + Ws], c.m, c.gtype, c.mode, c.fill, S, S)
            x.retain_grad()
            smp.append(x)
            kk = [] if dtype == torch.float64 else None
            on, sat, hue = JITTER[i]
            outs.append(jitter_ref(x, sat, hue, sat_first, kk) if on else x + 0.0)
            kinks.append(torch.stack(kk).any(dim=0)[0] if kk else torch.zeros(S, S, dtype=torch.bool))
        out = torch.cat(outs)
        out.backward(g.to(dtype))
        return out.detach(), torch.cat([x.grad for x in smp]), s.grad, torch.stack(kinks)
    out64, rgb64, ga64, kink = evaluate(torch.float64)
    out32, rgb32, ga32, _ = evaluate(torch.float32)
    frac = float(kink.double().mean())
    assert frac < 0.02, ("the reference alone must keep the near-kink pixels under 2 % of the case", frac)
    assert int(((out64[4] == 0.5).all(dim=0)).sum()) > 0, "no fully uncovered (exactly gray) fill pixel in the case"

    desc = desc_tensor(rows)
    a_d, g_d = dev(a), dev(g)
    fo, out = guarded(n * 3 * S, S, torch.float32)
    call("prx_k_warp_b_fwd", a_d, HA, WA, desc, None, fo, n, S, stream())
    sync()
    assert untouched(fo, n * 3 * S, S)
    out = out.cpu().view(n, 3, S, S)
    # forward value (continuous everywhere: no pixel left out), R3 against the same ops in torch fp32
    e, e32 = (out.double() - out64).abs(), (out32.double() - out64).abs()
    fig(f"colour-fwd/satfirst{sat_first}", float(e.max()) / (4 * float(e32.max())))
    assert rel_l2(out, out64) <= 4 * rel_l2(out32, out64) and float(e.max()) <= 4 * float(e32.max()), (float(e.max()), float(e32.max()))
    keep = (~kink)[:, None].expand(n, 3, S, S)
    jit_on = torch.tensor([j[0] for j in JITTER], dtype=torch.bool)
    for form in FORMS:
        runs = []
        for rep in range(2):
            fuv, _ = guarded(1, n * S * S * 2, torch.float32)
            frgb, grgb = guarded(n * 3 * S, S, torch.float32)
            fg, gk = guarded(n * 3 * HA, WA, torch.float32)
            maps = dev(torch.zeros(n * 16))
            call("prx_k_warp_b_bwd", a_d, HA, WA, desc, g_d, frgb, fuv, fg, n, S, maps, maps.numel() * 4, form, stream())
            sync()
            assert untouched(fg, n * 3 * HA, WA) and untouched(frgb, n * 3 * S, S)
            runs.append((grgb.cpu().view(n, 3, S, S).clone(), gk.cpu().view(n, 3, HA, WA).clone()))
        assert torch.equal(th.bits(runs[0][1]), th.bits(runs[1][1])) and torch.equal(th.bits(runs[0][0][jit_on]), th.bits(runs[1][0][jit_on]))
        grgb, ga = runs[0]
        assert bool(torch.isnan(grgb[~jit_on]).all()) and bool(torch.isfinite(grgb[jit_on]).all())       # written for jittered cutouts only
        # the pull-back through the jitter alone, away from the kinks
        k_on = keep[jit_on]
        er, er32 = ((grgb[jit_on].double() - rgb64[jit_on]).abs() * k_on), ((rgb32[jit_on].double() - rgb64[jit_on]).abs() * k_on)
        fig(f"colour-grgb/satfirst{sat_first}/form{form}", float(er.max()) / (4 * float(er32.max())))
        assert float(er.max()) <= 4 * float(er32.max()), ("jitter pull-back", form, float(er.max()), float(er32.max()))
        assert float(er.norm()) <= 4 * float(er32.norm())
        # the final stage-A gradient with the near-kink pixels' incoming gradient removed on both sides is not available from one
        # launch: compare where no near-kink pixel's footprint reaches (A^T kink == 0)
        s_probe = a.double().requires_grad_(True)
        probe = torch.cat([ref_warp(s_probe[i:i + 1, :, oy:oy + Hs, ox:ox + Ws], c.m, c.gtype, c.mode, c.fill, S, S) for i, c in enumerate(cuts)])
        reach, = torch.autograd.grad(probe, s_probe, kink[:, None].expand(n, 3, S, S).double())
        clean = reach == 0
        eg, eg32 = ((ga.double() - ga64).abs() * clean), ((ga32.double() - ga64).abs() * clean)
        fig(f"colour-ga/satfirst{sat_first}/form{form}", float(eg.max()) / (4 * float(eg32.max())))
        assert float(eg.max()) <= 4 * float(eg32.max()), ("stage-A gradient behind the jitter", form, float(eg.max()), float(eg32.max()))
        assert float(eg.norm()) <= 4 * float(eg32.norm())
    return out


@pytest.mark.parametrize("sat_first", [0, 1])
def test_stage_b_colour_path(sat_first):
    """jitter on / off, saturation-first both ways, saturation 0.3 / 1.7 (clamp active), hue +-0.4 rad: forward value, `grgb` and the
    final `ga` of the three forms against float64"""
    colour_case(sat_first)


def test_stage_b_explicit_noise_is_added_after_the_jitter():
    """out - jitter(sample) == factor * noise: the product (1 rounding) and the addition (1 rounding) on the noise-free output"""
    torch.manual_seed(3)
    n, S, HA, WA = 2, 17, 30, 30
    rows = []
    for i in range(n):
        P = pixel_map(20, 20, S, S, scale=(1.1 * 20 / S, 1.1 * 20 / S), rot_deg=5.0)
        rows.append(desc_words(m2=norm_matrix(P, i, 20, 20, S, S), mode2=M_FILL, grid2=i, fill=0.5, jit=1, sat=1.2, hue=0.3, sat_first=i,
                               noise=0.0, win=(5, 3, 20, 20)))
    a, noise = dev(torch.rand(n, 3, HA, WA)), dev(torch.randn(n, 3, S, S))
    f0, clean = guarded(n * 3 * S, S, torch.float32)
    call("prx_k_warp_b_fwd", a, HA, WA, desc_tensor(rows), None, f0, n, S, stream())
    facs = [0.07, 0.1]
    for i in range(n):
        rows[i][25] = facs[i]
    f1, noisy = guarded(n * 3 * S, S, torch.float32)
    call("prx_k_warp_b_fwd", a, HA, WA, desc_tensor(rows), noise, f1, n, S, stream())
    sync()
    assert untouched(f0, n * 3 * S, S) and untouched(f1, n * 3 * S, S)
    fac = torch.tensor(facs, dtype=torch.float32).double().view(n, 1, 1, 1)              # the kernel holds the factor in fp32
    term = fac * noise.cpu().double()
    ref = clean.cpu().view(n, 3, S, S).double() + term
    ok, worst = within(noisy.cpu().view(n, 3, S, S), ref, 2 * EPS32 * (clean.cpu().view(n, 3, S, S).double().abs() + term.abs()))
    assert ok, worst


# ================================================================================================ the emulated subset
def emu_subset():
    """tests/test_emu_cpu.py: every mode x flavour at the small shapes on both stages, the fallback cases (all three backward forms in
    each), the mixed / copy launches, pool, rescale, the jitter Jacobian case, the noise and the refusals, on the emulated kernels"""
    for stage in (1, 2):
        for mode in MODES:
            for shape in SMALL:
                test_warp_every_mode_and_flavour(mode, *shape, stage)
        for n_cut in (1, 4):
            test_warp_mixed_descriptors_with_a_copy_cutout(n_cut, stage)
        for case in SPECIAL:
            test_warp_search_fallbacks(case, stage)
    test_warp_backwards_refuse_a_scratch_that_is_too_small()
    for shape in POOL_SHAPES:
        for masked in (False, True):
            test_pool_fwd_bwd(*shape, masked)
    for shape in RESCALE_SHAPES:
        test_rescale_fwd_bwd(*shape)
    for sat_first in (0, 1):
        test_stage_b_colour_path(sat_first)
    test_stage_b_explicit_noise_is_added_after_the_jitter()
    return dict(FIGURES)
