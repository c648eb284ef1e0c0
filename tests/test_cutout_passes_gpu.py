"""The destination-parallel passes of csrc/cutouts.hip around the two warp scatters, one at a time (GPU; the emulated subset runs
from tests/test_cutout_passes_cpu.py): the merged stage-B pre-pass (raw coordinates + colour-jitter pull-back + stage maps in one
launch), the stage-A pre-pass (raw coordinates + stage maps), the two forward warps on their (plane, cutout) grid, the 16-byte and
scalar forms of the min/max renormalisation backward, and the 32-bit-index refusals.

What is bit for bit, and against what.  None of these passes may change arithmetic, so wherever the arithmetic can be restated as
plain IEEE operations the test holds the kernel to a FROZEN COPY of it, written here and never derived from a kernel's output:

* `project_frozen`: the sampling coordinate of a destination pixel -- float64 meshgrid transform or fp32 affine base grid, the
  conversion to fp32, ATen's unnormalisation -- as elementwise torch float64 / float32 operations in the kernel's order (every
  operation is a correctly rounded +, -, *, / or conversion, the file is built without fma contraction, so the bits are defined);
* `stage_map_frozen`: the stage map (pixel-space matrix, its inverse, the raw-coordinate range) in Python floats (IEEE double)
  with the fp32 conversions where the kernel has them;
* `renorm_apply_frozen`: g = (dA / std) * inv, + gmin where x == min, + gmax where x == max, gmin / gmax from the KERNEL'S OWN
  float64 sums.

Where restating is impractical (the forward-mode dual numbers of the HSV jitter; the four-tap sum under every padding mode) the
kernels are held to the float64 references of tests/test_kernels_cutouts_gpu.py at that file's gates: `run_stage` for the forward
warps (counted roundings), rule R3 (4 x torch-fp32's own error, near-kink pixels left out, < 2 % of the case) for `grgb`; the
renormalisation sums to tests/test_kernels_runner_gpu.py's counted gate.

Every launch runs twice and its outputs must be bit-identical.  The one exception are the two float64 renormalisation SUMS: their
blocks meet in atomics in no fixed order (they always did); they are held to the counted gate both times and the two exact counts
must be equal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pixray_amd._lib import PrxError, call

import test_kernels_half_gpu as th
import test_kernels_runner_gpu as tr
import test_kernels_cutouts_gpu as tc
from test_kernels_half_gpu import bits, guarded, untouched
from test_kernels_runner_gpu import stream, sync
from test_kernels_cutouts_gpu import (GRID_MESH, GRID_AFFINE, GRID_AFFINE_AC, GRID_MESH_AC, M_COPY, M_ZEROS, M_BORDER, M_REFLECT,
                                      M_FILL, Cut, desc_words, desc_tensor, norm_matrix, pixel_map)

NAN = float("nan")
MAP_WORDS = 13            # sizeof(StageMap) / 4: Pi[9], ulo, uhi, vlo, vhi


def dev(t):
    return tc.dev(t)       # follows tc.DEV ("cuda"; "cpu" on the emulated kernels)


def f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ================================================================================================ frozen arithmetic
def _linspace_pm1(n):
    """torch.linspace(-1, 1, n) in fp32, ATen's symmetric two-sided formula (linspace_pm1)"""
    i = torch.arange(n)
    step = f32(2.0) / f32(n - 1)
    lo = f32(-1.0) + step * i.to(torch.float32)
    hi = f32(1.0) - step * (n - 1 - i).to(torch.float32)
    return torch.where(i < n // 2, lo, hi)


def project_frozen(m, gtype, Wd, Hd, Ws, Hs):
    """(u, v) fp32 [Hd, Wd]: project() of csrc/cutouts.hip, operation by operation"""
    m = [float(v) for v in m]
    if gtype in (GRID_MESH, GRID_MESH_AC):
        xn = ((torch.arange(Wd, dtype=torch.float64) / float(Wd - 1) - 0.5) * 2.0)[None, :].expand(Hd, Wd)
        yn = ((torch.arange(Hd, dtype=torch.float64) / float(Hd - 1) - 0.5) * 2.0)[:, None].expand(Hd, Wd)
        X = m[0] * xn + m[1] * yn + m[2]
        Y = m[3] * xn + m[4] * yn + m[5]
        Z = m[6] * xn + m[7] * yn + m[8]
        sc = torch.where(Z.abs() > 1e-8, 1.0 / Z, torch.ones_like(Z))
        gx, gy = (X * sc).to(torch.float32), (Y * sc).to(torch.float32)
    else:
        xb, yb = _linspace_pm1(Wd), _linspace_pm1(Hd)
        if gtype == GRID_AFFINE:
            xb = (xb * f32(Wd - 1)) / f32(Wd)
            yb = (yb * f32(Hd - 1)) / f32(Hd)
        xb, yb = xb.double()[None, :].expand(Hd, Wd), yb.double()[:, None].expand(Hd, Wd)
        gx = (xb * m[0] + yb * m[1] + m[2]).to(torch.float32)
        gy = (xb * m[3] + yb * m[4] + m[5]).to(torch.float32)
    if gtype >= GRID_AFFINE_AC:
        u = ((gx + f32(1.0)) / f32(2.0)) * f32(Ws - 1)
        v = ((gy + f32(1.0)) / f32(2.0)) * f32(Hs - 1)
    else:
        u = (gx + f32(1.0)) * (f32(Ws) * f32(0.5)) - f32(0.5)
        v = (gy + f32(1.0)) * (f32(Hs) * f32(0.5)) - f32(0.5)
    return u.contiguous(), v.contiguous()


def stage_map_frozen(m, gtype, Wd, Hd, Ws, Hs):
    """the 13 fp32 words of a StageMap: stage_matrix + invert3 + build_stage_map of csrc/cutouts.hip in IEEE double (Python floats),
    fp32 (numpy.float32) where the kernel converts"""
    m = [float(v) for v in m]
    if gtype == GRID_AFFINE:
        ax, bx, ay, by = 2.0 / Wd, 1.0 / Wd - 1.0, 2.0 / Hd, 1.0 / Hd - 1.0
    else:
        ax, bx, ay, by = 2.0 / (Wd - 1), -1.0, 2.0 / (Hd - 1), -1.0
    T = [0.0] * 9
    for r in range(3):
        T[r * 3 + 0] = m[r * 3 + 0] * ax
        T[r * 3 + 1] = m[r * 3 + 1] * ay
        T[r * 3 + 2] = m[r * 3 + 0] * bx + m[r * 3 + 1] * by + m[r * 3 + 2]
    if gtype in (GRID_AFFINE, GRID_AFFINE_AC):
        T[6], T[7], T[8] = 0.0, 0.0, 1.0
    if gtype >= GRID_AFFINE_AC:
        sx = 0.5 * (Ws - 1); ox = sx; sy = 0.5 * (Hs - 1); oy = sy
    else:
        sx = 0.5 * Ws; ox = sx - 0.5; sy = 0.5 * Hs; oy = sy - 0.5
    a = [0.0] * 9
    for c in range(3):
        a[c] = sx * T[c] + ox * T[6 + c]
        a[3 + c] = sy * T[3 + c] + oy * T[6 + c]
        a[6 + c] = T[6 + c]
    c0, c1, c2 = a[4] * a[8] - a[5] * a[7], a[5] * a[6] - a[3] * a[8], a[3] * a[7] - a[4] * a[6]
    det = a[0] * c0 + a[1] * c1 + a[2] * c2
    idet = 1.0 / det if det != 0.0 else 0.0
    Pi = [c0 * idet, (a[2] * a[7] - a[1] * a[8]) * idet, (a[1] * a[5] - a[2] * a[4]) * idet,
          c1 * idet, (a[0] * a[8] - a[2] * a[6]) * idet, (a[2] * a[3] - a[0] * a[5]) * idet,
          c2 * idet, (a[1] * a[6] - a[0] * a[7]) * idet, (a[0] * a[4] - a[1] * a[3]) * idet]
    F = np.float32
    ulo, uhi, vlo, vhi = F(np.inf), F(-np.inf), F(np.inf), F(-np.inf)
    for k in range(4):
        x = float(Wd - 1) if (k & 1) else 0.0
        y = float(Hd - 1) if (k & 2) else 0.0
        z = a[6] * x + a[7] * y + a[8]
        u, v = (a[0] * x + a[1] * y + a[2]) / z, (a[3] * x + a[4] * y + a[5]) / z
        ulo, uhi, vlo, vhi = min(ulo, F(u)), max(uhi, F(u)), min(vlo, F(v)), max(vhi, F(v))
    zi = Pi[6] * (0.5 * float(F(ulo + uhi))) + Pi[7] * (0.5 * float(F(vlo + vhi))) + Pi[8]
    si = 1.0 / zi if zi != 0.0 else 1.0
    words = [F(p * si) for p in Pi] + [F(ulo - F(1.5)), F(uhi + F(1.5)), F(vlo - F(1.5)), F(vhi + F(1.5))]
    return torch.from_numpy(np.array(words, dtype=np.float32))


def renorm_apply_frozen(cut, mm, gimg, acc, std):
    """patchify_bwd_apply_kernel's element, fp32 operation by operation; `acc` are the kernel's own four float64 sums (CPU tensors)"""
    mn, mx = mm[0], mm[1]
    rng = mx - mn
    live = float(rng) != 0.0
    inv = (f32(1.0) / rng) if live else f32(1.0)
    a = [float(v) for v in acc.tolist()]
    gmin = f32((a[1] - a[0]) * float(inv) / max(a[2], 1.0)) if live else f32(0.0)
    gmax = f32(-a[1] * float(inv) / max(a[3], 1.0)) if live else f32(0.0)
    gy = gimg / torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1)
    g = gy * inv
    g = torch.where(cut == mn, g + gmin, g)
    g = torch.where(cut == mx, g + gmax, g)
    return g


# ================================================================================================ the six descriptors
S_B, HA_B, WA_B = 24, 28, 36
WIN_FULL, WIN_IN = (0, 0, WA_B, HA_B), (5, 3, 25, 22)          # whole stage-A image; ox, oy > 0 and ww < Wa
# (mode, flavour, (jitter on, saturation, hue), sat_first, window, perspective slope)
SIX = [(M_COPY, GRID_MESH, (0, 1.0, 0.0), 0, WIN_FULL, (0.0, 0.0)),                 # MODE_IDENT
       (M_FILL, GRID_AFFINE, (0, 1.0, 0.0), 0, WIN_FULL, (0.0, 0.0)),               # no jitter
       (M_FILL, GRID_MESH, (1, 0.3, 0.4), 1, WIN_FULL, (0.0, 0.0)),                 # jitter, saturation first
       (M_FILL, GRID_AFFINE_AC, (1, 1.7, -0.4), 0, WIN_FULL, (0.0, 0.0)),           # jitter, hue first
       (M_FILL, GRID_AFFINE, (1, 0.3, -0.4), 1, WIN_IN, (0.0, 0.0)),                # a window strictly inside
       (M_FILL, GRID_MESH_AC, (1, 1.7, 0.4), 0, WIN_FULL, (0.35, 0.25))]            # perspective grid


def six_descriptors(noise=0.0, seeds=None):
    """(descriptor rows, the stage-B Cut of every cutout)"""
    rows, cuts = [], []
    for i, (mode, gtype, (on, sat, hue), sat_first, win, persp) in enumerate(SIX):
        Ws, Hs = win[2], win[3]
        if mode == M_COPY:
            m = desc_words()[:9]
        else:
            P = pixel_map(Hs, Ws, S_B, S_B, scale=(1.15 * Ws / S_B, 1.15 * Hs / S_B), rot_deg=3.0 * (i - 2), shift=(0.5 * i, -0.4 * i),
                          persp=(persp[0] / (S_B - 1), persp[1] / (S_B - 1)))
            m = norm_matrix(P, gtype, Hs, Ws, S_B, S_B)
        cuts.append(Cut(m, gtype, mode, 0.5))
        rows.append(desc_words(m2=m, mode2=mode, grid2=gtype, fill=0.5, jit=on, sat=sat, hue=hue, sat_first=sat_first, noise=noise,
                               win=win, seed=0 if seeds is None else seeds[i]))
    return rows, cuts


def stage_a_image(n):
    """channel levels 0.2 / 0.5 / 0.8 +- 0.05 in the six orderings (tc.colour_case: the gaps survive bilinear mixing, so few pixels sit
    near a kink of the jitter's Jacobian)"""
    a = torch.empty(n, 3, HA_B, WA_B)
    for i in range(n):
        for c in range(3):
            a[i, c] = (0.2, 0.5, 0.8)[tc.ORDERINGS[i % 6][c]] + (torch.rand(HA_B, WA_B) - 0.5) * 0.1
    return a


# ================================================================================================ stage-B pre-pass
def _grgb_reference(a, g, cuts):
    """float64 / float32 pull-back of g through the jitter at the sampled rgb (tc.colour_case's evaluation), and the near-kink mask"""
    n = len(cuts)

    def evaluate(dtype):
        s = a.to(dtype)
        grads, kinks = [], []
        for i, c in enumerate(cuts):
            on, sat, hue = SIX[i][2]
            ox, oy, Ws, Hs = SIX[i][4]
            x = tc.ref_warp(s[i:i + 1, :, oy:oy + Hs, ox:ox + Ws], c.m, c.gtype, c.mode, c.fill, S_B, S_B).detach().requires_grad_(True)
            kk = [] if dtype == torch.float64 else None
            out = tc.jitter_ref(x, sat, hue, SIX[i][3], kk) if on else x + 0.0
            out.backward(g[i:i + 1].to(dtype))
            grads.append(x.grad)
            kinks.append(torch.stack(kk).any(dim=0)[0] if kk else torch.zeros(S_B, S_B, dtype=torch.bool))
        return torch.cat(grads), torch.stack(kinks)
    r64, kink = evaluate(torch.float64)
    r32, _ = evaluate(torch.float32)
    assert float(kink.double().mean()) < 0.02, "the reference alone must keep the near-kink pixels under 2 % of the case"
    return r64, r32, (~kink)[:, None].expand(n, 3, S_B, S_B)


def test_stage_b_prepass_writes_uv_grgb_and_maps_in_one_launch():
    """six cutouts, one each: MODE_IDENT, no jitter, jitter saturation-first, jitter hue-first, a window strictly inside the 28 x 36
    stage-A image, a perspective grid; S = 24 (576 pixels: 2.25 blocks).  uv == the frozen project() == what the stage-A pre-pass
    writes for the same words (the separate computation); maps == the frozen stage map (forms 0 and 1), untouched by form 2; the
    identity cutout's uv slice untouched; grgb written for the jittered cutouts only, against float64 at rule R3"""
    torch.manual_seed(21)
    n, S = len(SIX), S_B
    rows, cuts = six_descriptors()
    a, g = stage_a_image(n), torch.randn(n, 3, S, S)
    desc, a_d, g_d = desc_tensor(rows), dev(a), dev(g)
    ident = torch.tensor([s[0] == M_COPY for s in SIX])
    jit_on = torch.tensor([bool(s[2][0]) for s in SIX])
    uv_ref = torch.full((n, S * S, 2), NAN)
    map_ref = torch.zeros(n, MAP_WORDS)
    for i, c in enumerate(cuts):
        if c.mode == M_COPY:
            continue
        _, _, Ws, Hs = SIX[i][4]
        u, v = project_frozen(c.m, c.gtype, S, S, Ws, Hs)
        uv_ref[i] = torch.stack([u.flatten(), v.flatten()], dim=1)
        map_ref[i] = stage_map_frozen(c.m, c.gtype, S, S, Ws, Hs)
    r64, r32, keep = _grgb_reference(a, g, cuts)

    first = {}
    for form in tc.FORMS:
        runs = []
        for rep in range(2):
            fuv, uv = guarded(1, n * S * S * 2, torch.float32)
            frgb, grgb = guarded(n * 3 * S, S, torch.float32)
            fg, ga = guarded(n * 3 * HA_B, WA_B, torch.float32)
            maps = dev(torch.full((n * 16,), NAN))
            call("prx_k_warp_b_bwd", a_d, HA_B, WA_B, desc, g_d, frgb, fuv, fg, n, S, maps, maps.numel() * 4, form, stream())
            sync()
            assert untouched(fuv, 1, n * S * S * 2) and untouched(frgb, n * 3 * S, S) and untouched(fg, n * 3 * HA_B, WA_B)
            runs.append([t.cpu().clone() for t in (uv.reshape(n, S * S, 2), grgb.reshape(n, 3, S, S), ga.reshape(n, 3, HA_B, WA_B), maps)])
        assert all(same(x, y) for x, y in zip(*runs)), ("two launches of the stage-B backward differ", form)
        uv, grgb, ga, maps = runs[0]
        assert same(uv, uv_ref), ("uv is not the forward's coordinate, or an identity cutout's slice was written", form)
        if form == 2:
            assert bool(torch.isnan(maps).all()), "form 2 builds its own stage map: the scratch must stay untouched"
        else:
            assert same(maps[:n * MAP_WORDS].view(n, MAP_WORDS), map_ref), ("stage maps", form)
            assert bool((maps[:MAP_WORDS] == 0).all()) and bool(torch.isnan(maps[n * MAP_WORDS:]).all())
        assert bool(torch.isnan(grgb[~jit_on]).all()) and bool(torch.isfinite(grgb[jit_on]).all())
        k_on = keep[jit_on]
        er, er32 = (grgb[jit_on].double() - r64[jit_on]).abs() * k_on, (r32[jit_on].double() - r64[jit_on]).abs() * k_on
        print(f"[passes-fig] grgb/form{form} {float(er.max()) / (4 * float(er32.max())):.4f}")
        assert float(er.max()) <= 4 * float(er32.max()) and float(er.norm()) <= 4 * float(er32.norm()), ("jitter pull-back", form)
        assert bool(torch.isfinite(ga).all())
        first.setdefault("uv", uv); first.setdefault("grgb", grgb)
        assert same(uv, first["uv"]) and same(grgb, first["grgb"]), "the pre-pass must not depend on the form"

    # the separate computation: the stage-A pre-pass on the same words (stage-1 slots), one launch per window size
    for win in (WIN_FULL, WIN_IN):
        Ws, Hs = win[2], win[3]
        rows1 = [desc_words(m1=c.m, mode1=c.mode, grid1=c.gtype, fill=0.5) for c in cuts]
        for rep in range(2):
            fuv, uv1 = guarded(1, n * S * S * 2, torch.float32)
            fpriv, _ = guarded(n * 3 * Hs, Ws, torch.float32)
            fg, _ = guarded(3 * Hs, Ws, torch.float32)
            call("prx_k_warp_a_bwd", dev(torch.zeros(n, 3, S, S)), Hs, Ws, desc_tensor(rows1), fuv, fpriv, fg, n, S, S, 0, stream())
            sync()
            assert untouched(fuv, 1, n * S * S * 2) and untouched(fpriv, n * 3 * Hs, Ws) and untouched(fg, 3 * Hs, Ws)
            uv1 = uv1.cpu().reshape(n, S * S, 2)
            for i in range(n):
                if SIX[i][4] == win or ident[i]:
                    assert same(uv1[i], uv_ref[i]), ("stage-A pre-pass and stage-B pre-pass disagree on a coordinate", i)


def test_stage_a_prepass_coordinates_and_single_cutout():
    """the stage-A pre-pass alone: 17 x 23 destination (391 pixels, not a multiple of 256), four flavours and n_cut = 1, against the
    frozen project(); all three forms give the same uv"""
    Hs, Ws, Hd, Wd = 20, 37, 17, 23
    cuts = tc.mild_cuts(M_BORDER, Hs, Ws, Hd, Wd)
    for sub in (cuts, cuts[2:3]):
        n = len(sub)
        rows = [desc_words(m1=c.m, mode1=c.mode, grid1=c.gtype) for c in sub]
        ref = torch.stack([torch.stack([t.flatten() for t in project_frozen(c.m, c.gtype, Wd, Hd, Ws, Hs)], dim=1) for c in sub])
        for form in tc.FORMS:
            for rep in range(2):
                fuv, uv = guarded(1, n * Hd * Wd * 2, torch.float32)
                fpriv, _ = guarded(n * 3 * Hs, Ws, torch.float32)
                fg, _ = guarded(3 * Hs, Ws, torch.float32)
                call("prx_k_warp_a_bwd", dev(torch.ones(n, 3, Hd, Wd)), Hs, Ws, desc_tensor(rows), fuv, fpriv, fg, n, Hd, Wd, form, stream())
                sync()
                assert untouched(fuv, 1, n * Hd * Wd * 2) and untouched(fg, 3 * Hs, Ws)
                assert same(uv.cpu().reshape(n, Hd * Wd, 2), ref), ("stage-A uv", n, form)


# ================================================================================================ forward warps
def forward_cuts(Hs, Ws, Hd, Wd):
    """the six descriptor kinds as plain warps of one stage (tc.run_stage builds the words): copy, zeros + affine, fill + mesh,
    fill + corner-aligned affine, border + affine, reflection + perspective mesh"""
    def one(gtype, mode, rot, persp=(0.0, 0.0)):
        P = pixel_map(Hs, Ws, Hd, Wd, scale=(1.1 * (Ws - 1) / (Wd - 1), 1.1 * (Hs - 1) / (Hd - 1)), rot_deg=rot, shift=(0.04 * Ws, -0.03 * Hs),
                      persp=(persp[0] / (Wd - 1), persp[1] / (Hd - 1)))
        return Cut(norm_matrix(P, gtype, Hs, Ws, Hd, Wd), gtype, mode, 0.4)
    copy = Cut(desc_words()[:9], 0, M_COPY)
    return [copy, one(GRID_AFFINE, M_ZEROS, 4.0), one(GRID_MESH, M_FILL, -6.0), one(GRID_AFFINE_AC, M_FILL, 5.0),
            one(GRID_AFFINE, M_BORDER, -3.0), one(GRID_MESH_AC, M_REFLECT, 2.0, (0.35, 0.25))]


@pytest.mark.parametrize("stage", [1, 2])
def test_forward_warps_on_the_plane_grid(stage):
    """six cutouts and n_cut = 1 (the perspective one), planes of 621 / 576 pixels (not a multiple of 256, more than one block):
    every output element against the float64 reference at the counted forward gate of tc.run_stage"""
    Hs, Ws, Hd, Wd = (23, 27, 23, 27) if stage == 1 else (26, 31, 24, 24)
    cuts = forward_cuts(Hs, Ws, Hd, Wd)
    tc.run_stage(stage, cuts, Hs, Ws, Hd, Wd, seed=5 + stage, forms=(), name="passes-six")
    tc.run_stage(stage, cuts[5:6], Hs, Ws, Hd, Wd, seed=7 + stage, forms=(), name="passes-one")


def _launch_fwd(stage, src, H, W, desc, noise, n, Hd, Wd):
    outs = []
    for rep in range(2):
        full, out = guarded(n * 3 * Hd, Wd, torch.float32)
        if stage == 1:
            call("prx_k_warp_a_fwd", src, H, W, desc, full, n, Hd, Wd, stream())
        else:
            call("prx_k_warp_b_fwd", src, H, W, desc, noise, full, n, Hd, stream())
        sync()
        assert untouched(full, n * 3 * Hd, Wd)
        outs.append(out.cpu().reshape(n, 3, Hd, Wd).clone())
    assert same(outs[0], outs[1]), ("two launches of a forward warp differ", stage)
    assert bool(torch.isfinite(outs[0]).all())
    return outs[0]


def test_forward_warps_in_kernel_noise_equals_explicit_noise_for_the_same_key():
    """the Philox counter is the pixel index y * S + x and the key the seed word, whatever the grid: (1) on a zero canvas under the
    identity with factor 1 the output IS the draw of each key; (2) the six descriptors with those keys and factor 0.1 give the same
    bits with the draws made in the kernel as with the draws of (1) handed in as the noise tensor; (3) one cutout launched alone
    (n_cut = 1) sees the draws it sees in the batch; stage A twice: bit-identical"""
    torch.manual_seed(4)
    n, S = len(SIX), S_B
    seeds = [11, 12, 13, 2 ** 52 + 12345, 15, 11]
    ident_rows = [desc_words(noise=1.0, win=(0, 0, S, S), seed=k) for k in seeds]
    z = _launch_fwd(2, dev(torch.zeros(n, 3, S, S)), S, S, desc_tensor(ident_rows), None, n, S, S)
    assert same(z[0], z[5]) and not torch.equal(z[0], z[1]) and abs(float(z.std()) - 1.0) < 0.05
    a = dev(stage_a_image(n))
    rows, _ = six_descriptors(noise=0.1, seeds=seeds)
    drawn = _launch_fwd(2, a, HA_B, WA_B, desc_tensor(rows), None, n, S, S)
    rows0, _ = six_descriptors(noise=0.1)
    given = _launch_fwd(2, a, HA_B, WA_B, desc_tensor(rows0), dev(z), n, S, S)
    assert same(drawn, given), "in-kernel draws differ from the same draws handed in"
    clean = _launch_fwd(2, a, HA_B, WA_B, desc_tensor(rows0), None, n, S, S)              # no key, no tensor: no noise
    assert not torch.equal(clean, drawn)
    alone = _launch_fwd(2, a[4:5].contiguous(), HA_B, WA_B, desc_tensor(rows[4:5]), None, 1, S, S)
    assert same(alone[0], drawn[4]), "a cutout launched alone must see the batch's draws"
    Hs, Ws = 23, 27
    cuts = forward_cuts(Hs, Ws, Hs, Ws)
    rows1 = [desc_words(m1=c.m, mode1=c.mode, grid1=c.gtype, fill=c.fill) for c in cuts]
    _launch_fwd(1, dev(torch.rand(1, 3, Hs, Ws)), Hs, Ws, desc_tensor(rows1), None, len(cuts), Hs, Ws)


# ================================================================================================ renormalisation backward
RENORM = [(3, 32, 8, "16-byte"), (2, 28, 14, "scalar-padded"), (2, 30, 6, "scalar")]          # (N, S, P): Kp == K, Kp == K + 4, P % 4 != 0


def _planted(N, S, constant):
    """cutouts with the minimum planted twice and the maximum three times (or constant: range == 0)"""
    cut = torch.rand(N, 3, S, S) * 0.8 + 0.1
    if constant:
        cut.fill_(0.625)
    else:
        f = cut.view(-1)
        k = f.numel()
        f[[6, k // 2 + 1]] = 0.03125
        f[[19, k // 3, k - 2]] = 0.96875
    return dev(cut), dev(torch.stack([cut.min(), cut.max()]))


def _renorm_run(reduce_call, apply_call, cut, mm, gimg, std, N, S):
    """both passes twice: the sums at the counted gate (tr._check_reduce), the counts equal, gcut == the frozen formula on the kernel's
    own sums and bit-identical between the launches"""
    outs = []
    for rep in range(2):
        afull, acc = tr.flat(4, torch.float64)
        reduce_call(afull)
        sync()
        tr._check_reduce(acc, cut, mm, gimg.double(), std)
        assert untouched(afull, 1, 4)
        own = acc.clone().contiguous()
        gfull, gcut = guarded(N * 3 * S, S, torch.float32)
        apply_call(own, gfull)
        sync()
        assert untouched(gfull, N * 3 * S, S)
        want = renorm_apply_frozen(cut.cpu(), mm.cpu(), gimg.cpu(), own.cpu(), std)
        got = gcut.cpu().reshape(N, 3, S, S)
        assert same(got, want), ("gcut is not the parent formula on the kernel's own sums", int((bits(got) != bits(want)).sum()))
        outs.append((own.cpu(), got.clone()))
    assert outs[0][0][2:].tolist() == outs[1][0][2:].tolist()
    # the same sums handed to both launches: bit-identical gradients
    gs = []
    for rep in range(2):
        gfull, gcut = guarded(N * 3 * S, S, torch.float32)
        apply_call(dev(outs[0][0]).contiguous(), gfull)
        sync()
        gs.append(gcut.cpu().clone())
    assert same(gs[0], gs[1]) and same(gs[0].reshape(N, 3, S, S), outs[0][1])
    return outs[0]


def renorm_patch_case(N, S, P, constant=False, misalign=False):
    torch.manual_seed(S * 10 + P)
    G = S // P
    T, K, Kp = G * G + 1, 3 * P * P, tr._kp(P)
    mean, std = tr.NORMS["clip"]
    cut, mm = _planted(N, S, constant)
    store = dev(torch.empty(N * T * Kp + 1))
    dA = store[1:] if misalign else store[:-1]            # misalign: 4 bytes off a 16-byte boundary -> the scalar form must take it
    dA.copy_(torch.randn(N * T * Kp))                     # the same values either way
    assert (dA.data_ptr() % 16 != 0) == misalign
    gimg = tr._to_image(dA.reshape(N, T, Kp)[:, 1:, :K], N, S, P).contiguous()
    return _renorm_run(lambda afull: call("prx_k_patchify_bwd_reduce", cut, mm, dA, afull, N, S, P, T, *mean, *std, stream()),
                       lambda acc, gfull: call("prx_k_patchify_bwd_apply", cut, mm, dA, acc, gfull, N, S, P, T, *mean, *std, stream()),
                       cut, mm, gimg, std, N, S)


@pytest.mark.parametrize("N,S,P,path", RENORM)
def test_renorm_backward_patch_layout(N, S, P, path):
    """the 16-byte form (P % 4 == 0, S % 4 == 0), the scalar form with padded rows (P = 14: 588 -> 592 columns) and without; two
    pixels exactly at the minimum, three exactly at the maximum"""
    renorm_patch_case(N, S, P)


def test_renorm_backward_constant_image_and_misaligned_gradient():
    """range == 0 (inv = 1, no extremum terms) in the 16-byte form; and the 16-byte geometry with dA four bytes off alignment: the
    launcher must fall back to the scalar form and give the aligned launch's bits"""
    renorm_patch_case(3, 32, 8, constant=True)
    _, g_aligned = renorm_patch_case(3, 32, 8)
    _, g_off = renorm_patch_case(3, 32, 8, misalign=True)
    assert same(g_aligned, g_off)


@pytest.mark.parametrize("constant", [False, True])
def test_renorm_backward_image_layout(constant):
    """the image-layout entries (one `patch` = the image, P = S = 32, the pointer shifted back one row of K): the 16-byte form"""
    torch.manual_seed(33)
    N, S = 3, 32
    cut, mm = _planted(N, S, constant)
    dY = dev(torch.randn(N, 3, S, S))
    _renorm_run(lambda afull: call("prx_k_preproc_bwd_reduce", cut, mm, dY, afull, N, S, stream()),
                lambda acc, gfull: call("prx_k_preproc_bwd_apply", cut, mm, dY, acc, gfull, N, S, stream()),
                cut, mm, dY, tr.CLIP_STD, N, S)


# ================================================================================================ refusals
def test_planes_beyond_the_32_bit_index_are_refused_and_nothing_is_written():
    """sizes only (nothing of that size is allocated): a plane of 46341^2 >= 2^31 pixels for the four warp entries, 3 * 26755^2 >= 2^31
    elements for the four renormalisation entries, 65536 cutouts for a grid's rows; the error by name, every buffer still NaN"""
    B = 46341
    assert B * B >= 2 ** 31 > (B - 1) * (B - 1)
    desc = desc_tensor([desc_words(mode1=M_ZEROS, mode2=M_ZEROS, win=(0, 0, 4, 4))])
    small = dev(torch.rand(1, 3, 4, 4))
    bufs = [dev(torch.full((64,), NAN)) for _ in range(4)]
    maps = dev(torch.full((16,), NAN))
    msg = "exceeds? the 32-bit index range"
    with pytest.raises(PrxError, match=msg):
        call("prx_k_warp_a_fwd", small, 4, 4, desc, bufs[0], 1, B, B, stream())
    with pytest.raises(PrxError, match=msg):
        call("prx_k_warp_a_fwd", small, B, B, desc, bufs[0], 1, 4, 4, stream())
    with pytest.raises(PrxError, match="exceed the 65535 rows of a launch grid"):
        call("prx_k_warp_a_fwd", small, 4, 4, desc, bufs[0], 65536, 4, 4, stream())
    with pytest.raises(PrxError, match=msg):
        call("prx_k_warp_b_fwd", small, 4, 4, desc, None, bufs[0], 1, B, stream())
    for form in tc.FORMS:
        with pytest.raises(PrxError, match=msg):
            call("prx_k_warp_a_bwd", small, 4, 4, desc, bufs[0], bufs[1], bufs[2], 1, B, B, form, stream())
        with pytest.raises(PrxError, match=msg):
            call("prx_k_warp_b_bwd", small, 4, 4, desc, small, bufs[0], bufs[1], bufs[2], 1, B, maps, 64, form, stream())
    N, S = 1, 26755
    assert N * 3 * S * S >= 2 ** 31
    mm = dev(torch.tensor([0.0, 1.0]))
    acc = dev(torch.full((4,), NAN, dtype=torch.float64))
    mean, std = tr.NORMS["clip"]
    with pytest.raises(PrxError, match=msg):
        call("prx_k_patchify_bwd_reduce", small, mm, bufs[0], acc, N, S, S, 2, *mean, *std, stream())
    with pytest.raises(PrxError, match=msg):
        call("prx_k_patchify_bwd_apply", small, mm, bufs[0], dev(torch.zeros(4, dtype=torch.float64)), bufs[3], N, S, S, 2, *mean, *std, stream())
    with pytest.raises(PrxError, match=msg):
        call("prx_k_preproc_bwd_reduce", small, mm, bufs[0], acc, N, S, stream())
    with pytest.raises(PrxError, match=msg):
        call("prx_k_preproc_bwd_apply", small, mm, bufs[0], dev(torch.zeros(4, dtype=torch.float64)), bufs[3], N, S, stream())
    sync()
    assert all(bool(torch.isnan(b).all()) for b in bufs) and bool(torch.isnan(maps).all()) and bool(torch.isnan(acc).all())


# ================================================================================================ the emulated subset
def emu_subset():
    """tests/test_cutout_passes_cpu.py: everything above on the emulated kernels"""
    test_stage_b_prepass_writes_uv_grgb_and_maps_in_one_launch()
    test_stage_a_prepass_coordinates_and_single_cutout()
    for stage in (1, 2):
        test_forward_warps_on_the_plane_grid(stage)
    test_forward_warps_in_kernel_noise_equals_explicit_noise_for_the_same_key()
    for N, S, P, path in RENORM:
        test_renorm_backward_patch_layout(N, S, P, path)
    test_renorm_backward_constant_image_and_misaligned_gradient()
    for constant in (False, True):
        test_renorm_backward_image_layout(constant)
    test_planes_beyond_the_32_bit_index_are_refused_and_nothing_is_written()
