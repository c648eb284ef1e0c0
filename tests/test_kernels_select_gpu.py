"""Kernel-level float64 tests (GPU) of the kernels that make a discrete choice: `prompt_loss_kernel` (the mask of max(d, stop)),
`vq_dist_kernel` / `vq_select_kernel` (an argmin, first index on ties), `palette_kernel` / `color_lookup_kernel` (the nearest palette
entry) and `smoothness_fwd_kernel` / `smoothness_bwd_kernel` (a kink at s = 0.5, a zero subgradient at flat pixels, a hand-transposed
stencil), each through the C entry the product calls: `prx_prompt_loss_fwd_bwd`, `prx_k_vq_nearest` + `prx_k_sqnorm_rows`,
`prx_palette_fwd_bwd`, `prx_color_lookup_fwd`, `prx_smoothness_fwd` / `_bwd`.

Method (helpers and the three tolerance rules R1 / R2 / R3 of tests/test_kernels_runner_gpu.py, imported): every input is drawn on the
CPU from a seeded generator (the device sees the same bits as the emulation), outputs are pre-filled with NaN and carry spare rows that
must come back untouched, every call that reduces a scalar gets its own zeroed ticket word (read back: zero again) and its own
4 * 1024 doubles of partials.  References are plain torch in FLOAT64 on the fp32 inputs; every input is chosen so that the float64
reference ALONE decides each discrete choice, and the test asserts that condition (margins to `stop`, to the kink, between the two
nearest codes / entries) before it looks at the kernel:

* prompt: `oracle/prompt_ref.Prompt(...).double()`; the yardstick of R3 is the same class in fp32, its worst row in the case.  rowloss
  per row, the scalar and the gradient per row (row rel-L2) under R3.  On a tie d == stop (stop := the kernel's own fp32 d of a row) the
  gradient is half the float64 gradient (torch.maximum).  Planted angles of 1, 60, 90 and 150 degrees to the embed; 170 degrees and
  beyond are NOT tested: the fp32 reference itself is off by 5e-6 at 170 and by 1.5e-4 at 179 degrees (|xn - en| -> 2, where asin is
  vertical), so nothing could be concluded there.  A row parallel to the embed: only rounding noise remains on both sides, bounded by
  |grad_row| |x| denom / |w| <= 16 * 2^-24 (derivation at `test_prompt_row_parallel_to_the_embed`).
* VQ: `oracle/vqgan_ref.vq_exactness` (bad == 0, near-ties <= 1 per case) in NCHW and NHWC strides, zq bit-equal to codebook[idx];
  planted exact ties (bitwise equal code rows) must go to the LOWEST index.
* palette / lookup: float64 of the documented formula (include/prx.h); nearest = the lowest index among the entries whose float64
  squared distance is minimal; a pixel is a near-tie when the next float64 squared distance is closer than 8 * 2^-24 of itself
  (two subtractions, three squares, two additions, + 1: the chain of one fp32 squared distance against another), at most one per case.
* smoothness: float64 torch.gradient over the documented [n*h][w][3] view, flat pixels (ss == 0) left out of the sum, so that the
  reference states the zero subgradient instead of NaN; autograd for the gradient.

Measured (`python -m pytest -s` prints every figure as a `[select-fig]` line: name, kernel error, gate; no gate was moved after a run).
Yardsticks, torch fp32 against float64 on the CPU: prompt gradient rows 1.4e-7 .. 6.2e-7 at the random cases (rowloss 9.8e-8 ..
3.1e-7), 2.0e-6 / 8.2e-8 / 1.6e-7 / 8.1e-7 at 1 / 60 / 90 / 150 degrees; smoothness tfac 1.2e-8 .. 1.0e-7, grad 6.0e-8 .. 3.6e-7, loss
6.7e-9 .. 1.6e-7.  The `stop` cases split the pairs 76 / 44 and 84 / 36 at float64 margins of 7.7e-4 and 2.3e-3.
Worst kernel error / gate on an MI355X (on the CPU emulation in brackets): prompt rowloss 0.53 (0.42), scalar 0.49 (0.34), gradient
rows 0.51 (0.44); tie 0.39 (0.39); angles 0.31 (0.33); zero rows 0.33 (0.36); the parallel row 0.58 * 2^-24 against the bound of
16 * 2^-24 (float64 of the same inputs: 0.43 * 2^-24).  VQ: 0 near-ties and 0 differences from the float64 argmin at every shape and
layout; every planted tie at the lowest index.  Palette loss 0.16 (0.19), gradient 0.50 (0.50), lookup loss 0.33 (0.33), out bit-equal.
Smoothness (after the fix below) tfac 0.25 (0.25), gradient 0.31 (0.39), loss 0.25 (0.25).

Found and fixed: the smoothness forward evaluated each pixel in fp32 and only summed in double, so its scalar carried the per-pixel
roundings on top of its own conversion -- on the MI355X 9.15e-8 (1.5 * 2^-24) against a gate of 2.93e-8 at 1 x 3 x 3, eo 2, type 2,
spacing 1.0 (test_smoothness_loss_under_r3[1-3-3]; tfac and the gradient of that case were at 0.27 and 0.19 of their gates).  The
kernel now evaluates the pixel in double (stencil with 1 / spacing formed in double, root, logarithm): the scalar is the fp32
rounding of the float64 sum, which no fp32 result can beat, so its error cannot exceed that of torch's fp32 value.  After the fix on the MI355X: that case 7.3e-9 (the yardstick itself), worst loss 0.25 of its gate over the 78 cases,
tfac 0.25, gradient 0.31.  No defect was found in the other three families.

Mutation check on the emulated kernels (sources and tools/hipemu copied aside, one line changed, rebuilt, every test of this file run):
`d < best` -> `d <= best` in vq_dist_kernel: ties one-thread-neighbours ([6, 6, 6] for 5) and one-thread-two-quads (69 for 5) fail;
the cross-thread tie-break of vq_dist_kernel reduced to `v < best`: two-threads-lower-index-visited-last fails (68 for 8), reduced to
`v <= best`: two-threads fails (9 for 5); vq_select_kernel's loop with `v <= best`: select-loop-tile-1-and-257 fails (32901 for 133;
tiles 0 and 257 belong to two threads and do not reach that line), its reduction with `v <= ...`: two-tiles and
select-loop-tile-0-and-257 fail; mask 0.5f -> 1.f: the tie test fails (row 2 off by rel-L2 1.0); `(d > stop)` ->
`(d >= stop - 1e-3f)`: the tie test and test_prompt_stop_just_above_a_pair fail (the two random `stop` cases have no pair within
1e-3 BELOW stop and pass); stencil coefficient -0.5 -> 0.5 at i == 0: every edge-order-2 case fails (tfac rel-L2 0.05 .. 0.12,
loss 3e-4 .. 0.13); `s > 0 ? dv / s : 0` -> `dv / fmax(s, 1e-12)`: the flat patch fails for every type (tfac rel-L2 4e10).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from pixray_amd import _lib  # noqa: F401
from pixray_amd._lib import PrxError, call

from oracle import prompt_ref, vqgan_ref

import test_kernels_half_gpu as th  # noqa: F401
from test_kernels_half_gpu import guarded, untouched, within, rel_l2, bits  # noqa: F401  (within: behind check_f32)
from test_kernels_runner_gpu import stream, sync, flat, check_f32, same_bits

DEV = "cuda"          # tests/test_emu_cpu.py switches this (and the helper modules') to "cpu" for the emulated kernels
EPS32 = 2.0 ** -24
NAN = float("nan")
INF = float("inf")
F32 = torch.float32
FIGURES = {}          # name -> (worst kernel error, its gate), printed by the tests (`pytest -s`)


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
    print(f"[select-fig] {name} {err:.3e} {gate:.3e}")


def r3_gate(yard):
    """R3: 4 x the error of torch's own fp32 evaluation against the float64 reference, never above 1e-5"""
    return min(4.0 * float(yard), 1e-5)


def scratch():
    """a zeroed ticket word and 4 * 1024 doubles of partials for ONE call"""
    return torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(4 * 1024, dtype=torch.float64, device=DEV)


def row_rel(a, ref):
    """rel-L2 of every row (a zero reference row wants an exactly zero row); NaN stays NaN and fails every `<=`"""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    a, ref = a.reshape(a.shape[0], -1), ref.reshape(ref.shape[0], -1)
    return (a - ref).norm(dim=1) / (ref.norm(dim=1) + 1e-300)


def all_le(v, gate):
    return bool((v <= gate).all())


# ================================================================================================ 1. prompt loss
def prompt_inputs(n, m, D):
    g = torch.Generator().manual_seed(n + m + D)
    x = 3.0 * torch.randn(n, D, generator=g)          # not pre-normalised
    e = torch.randn(m, D, generator=g)
    return x, e


def prompt_launch(xd, ed, w, stop, want_loss=True, ticket=None, denom=None):
    """one call on fresh NaN buffers -> (rowloss [n], grad [n][D], loss [1]); the ticket is read back"""
    (n, D), m = xd.shape, ed.shape[0]
    rfull, rl = flat(n, F32)
    gfull, gr = guarded(n, D, F32)
    lfull, ls = flat(1, F32)
    tk = ticket if ticket is not None else torch.zeros(1, dtype=torch.int32, device=DEV)
    call("prx_prompt_loss_fwd_bwd", xd, ed, n, m, D, float(w), float(stop), float(n * m if denom is None else denom), rfull, gfull,
         lfull if want_loss else None, tk if want_loss else None, stream())
    sync()
    assert untouched(rfull, 1, n) and untouched(gfull, n, D)
    assert untouched(lfull, 1, 1) if want_loss else bool(torch.isnan(lfull).all())
    assert int(tk.item()) == 0, "the ticket word is not zero again on exit"
    return rl, gr, ls


def prompt_eval(x, e, w, stop, dtype):
    """oracle/prompt_ref.Prompt in `dtype` on the fp32 inputs -> (signed pair distances [n][m], rowloss [n], loss, grad [n][D])"""
    xr = x.clone().to(dtype).requires_grad_(True)
    P = prompt_ref.Prompt(e.clone(), w, stop).to(dtype)        # weight and stop: the fp32 values the kernel is handed
    loss = P(xr)
    (g,) = torch.autograd.grad(loss, xr)
    sign = float(torch.tensor(float(w)).sign())
    d = prompt_ref.spherical_dist_loss(x.to(dtype)[:, None, :], e.to(dtype)[None, :, :]) * sign
    return d, d.sum(dim=1), loss.detach(), g


def prompt_yard(x, e, w, stop):
    """(float64 reference, R3 gates of rowloss / scalar and of the gradient rows: the worst row of the fp32 evaluation)"""
    r64, r32 = prompt_eval(x, e, w, stop, torch.float64), prompt_eval(x, e, w, stop, F32)
    y_rl = float(((r32[1].double() - r64[1]).abs() / r64[1].abs()).max())
    y_g = float(row_rel(r32[3], r64[3]).max())
    return r64, y_rl, y_g


def prompt_check(name, out, r64, y_rl, y_g):
    rl, gr, ls = out
    d64, rl64, l64, g64 = r64
    e_rl = ((rl.double().cpu() - rl64).abs() / rl64.abs())
    e_l = abs(float(ls) - float(l64)) / abs(float(l64))
    e_g = row_rel(gr, g64)
    print(f"[select-fig] {name} yardsticks: rowloss {y_rl:.3e} grad {y_g:.3e}")
    fig(name + "/rowloss", e_rl.max(), r3_gate(y_rl))
    fig(name + "/loss", e_l, r3_gate(y_rl))
    fig(name + "/grad", e_g.max(), r3_gate(y_g))
    assert all_le(e_rl, r3_gate(y_rl)), ("rowloss", e_rl, r3_gate(y_rl))
    assert e_l <= r3_gate(y_rl), ("loss", e_l, r3_gate(y_rl))
    assert all_le(e_g, r3_gate(y_g)), ("grad rows", e_g, r3_gate(y_g))


def prompt_twice_and_without_loss(xd, ed, w, stop, out):
    """a second call on the same ticket: bit-identical; loss = NULL (no ticket): rowloss and grad bit-equal"""
    tk = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = prompt_launch(xd, ed, w, stop, ticket=tk)
    b = prompt_launch(xd, ed, w, stop, ticket=tk)
    for u, v, o in zip(a, b, out):
        assert torch.equal(bits(u), bits(v)) and torch.equal(bits(u), bits(o)), "two calls on one ticket differ"
    c = prompt_launch(xd, ed, w, stop, want_loss=False)
    assert torch.equal(bits(c[0]), bits(out[0])) and torch.equal(bits(c[1]), bits(out[1])), "loss = NULL changes rowloss / grad"


PROMPT_CASES = [(1, 1, 64, 1.0, -INF), (5, 1, 64, 1.0, -INF), (7, 3, 640, -0.5, -INF), (130, 2, 1024, 2.0, -INF),
                (30, 4, 768, 1.0, 1.2), (30, 4, 768, -1.0, -1.25), (6, 2, 512, 0.0, -INF)]


@pytest.mark.parametrize("n,m,D,w,stop", PROMPT_CASES)
def test_prompt_random_cases(n, m, D, w, stop):
    """n = 1, 5, 7, 130: ragged last workgroup, the `r += 64` loop of the last workgroup's sum; D = 640, 768, 1024 (MAXE); a finite
    `stop` that splits the pairs (both branches of the mask), its margin decided by the float64 reference alone; w = 0: exact zeros"""
    x, e = prompt_inputs(n, m, D)
    xd, ed = dev(x), dev(e)
    out = prompt_launch(xd, ed, w, stop)
    prompt_twice_and_without_loss(xd, ed, w, stop, out)
    if w == 0.0:
        for t in out:
            assert bool((t == 0).all()), "w = 0 must give exact zeros"
        return
    r64, y_rl, y_g = prompt_yard(x, e, w, stop)
    if stop != -INF:
        d64, s = r64[0], f32v(stop)
        above, below = int((d64 > s).sum()), int((d64 < s).sum())
        margin = float((d64 - s).abs().min())
        print(f"[select-fig] prompt-{n}-{m}-{D}-{w} pairs above / below stop {above} / {below}, min |d64 - stop| {margin:.3e}")
        assert min(above, below) * 4 >= n * m and margin > 1e-4, (above, below, margin)
    prompt_check(f"prompt-{n}-{m}-{D}-{w}-{stop}", out, r64, y_rl, y_g)


def test_prompt_stop_just_above_a_pair():
    """the comparison with `stop` at the resolution the margin rule allows: stop is put 5e-4 ABOVE a pair's float64 d (a pair near the
    median whose upper neighbour is at least 1e-3 away), so that pair is below stop by five times the asserted margin of 1e-4 and every
    other pair is further still -- a mask that is a few 1e-4 generous either way gives that pair the wrong branch"""
    n, m, D, w = 30, 4, 768, 1.0
    x, e = prompt_inputs(n, m, D)
    d = prompt_eval(x, e, w, -INF, torch.float64)[0].flatten().sort().values
    k = next(k for k in range(len(d) // 2, len(d) - 1) if float(d[k + 1] - d[k]) > 1e-3)
    stop = f32v(float(d[k]) + 5e-4)
    r64, y_rl, y_g = prompt_yard(x, e, w, stop)
    margin = float((r64[0] - stop).abs().min())
    assert 1e-4 < margin < 1e-3 and int((r64[0] < stop).sum()) == k + 1, (margin, k)
    prompt_check("prompt-stop-5e-4-above-a-pair", prompt_launch(dev(x), dev(e), w, stop), r64, y_rl, y_g)


def test_prompt_exact_tie_on_stop():
    """stop := the kernel's own fp32 d of row 2 (m = 1, w = 1): that row takes the 0.5 mask -- half its float64 gradient; the other
    rows are full or exactly zero by the sign of d64 - stop (margin asserted); the forward values do not depend on stop"""
    n, m, D, w = 5, 1, 64, 1.0
    x, e = prompt_inputs(n, m, D)
    xd, ed = dev(x), dev(e)
    first = prompt_launch(xd, ed, w, -INF)
    stop = float(first[0][2])
    out = prompt_launch(xd, ed, w, stop)
    assert torch.equal(bits(out[0]), bits(first[0])) and torch.equal(bits(out[2]), bits(first[2]))
    (d64, _, _, g64), _, y_g = prompt_yard(x, e, w, -INF)
    others = [i for i in range(n) if i != 2]
    margin = float((d64[others, 0] - stop).abs().min())
    assert margin > 1e-4, margin
    full = [i for i in others if float(d64[i, 0]) > stop]
    zero = [i for i in others if float(d64[i, 0]) < stop]
    assert full and zero, "the tie row must have rows on both sides of it"
    want = g64.clone()
    want[2] *= 0.5
    want[zero] = 0.0
    e_g = row_rel(out[1], want)
    fig("prompt-tie/grad", e_g.max(), r3_gate(y_g))
    assert all_le(e_g, r3_gate(y_g)), (e_g, r3_gate(y_g))
    assert bool((out[1][zero] == 0).all())


ANGLES = [1.0, 60.0, 90.0, 150.0]


def test_prompt_planted_angles():
    """x_i = 2.5 (cos t e^ + sin t o^), t = 1, 60, 90, 150 degrees, D = 512, one embed: every row under R3 with its own yardstick
    (all below the 1e-5 cap: torch fp32 measured 2.1e-6, 8.7e-8, 1.4e-7, 8.1e-7)"""
    D = 512
    g = torch.Generator().manual_seed(D)
    e = torch.randn(1, D, generator=g)
    eh = e[0].double() / e[0].double().norm()
    o = torch.randn(D, generator=g).double()
    o = o - eh * (eh @ o)
    o = o / o.norm()
    t = torch.tensor(ANGLES, dtype=torch.float64) * (torch.pi / 180.0)
    x = (2.5 * (torch.cos(t)[:, None] * eh[None] + torch.sin(t)[:, None] * o[None])).float()
    xd, ed = dev(x), dev(e)
    out = prompt_launch(xd, ed, 1.0, -INF)
    r64, r32 = prompt_eval(x, e, 1.0, -INF, torch.float64), prompt_eval(x, e, 1.0, -INF, F32)
    y_rl = (r32[1].double() - r64[1]).abs() / r64[1].abs()
    y_g = row_rel(r32[3], r64[3])
    e_rl = (out[0].double().cpu() - r64[1]).abs() / r64[1].abs()
    e_g = row_rel(out[1], r64[3])
    for i, a in enumerate(ANGLES):
        print(f"[select-fig] prompt-angle-{a:g} yardsticks: rowloss {float(y_rl[i]):.3e} grad {float(y_g[i]):.3e}")
        fig(f"prompt-angle-{a:g}/grad", e_g[i], r3_gate(y_g[i]))
        fig(f"prompt-angle-{a:g}/rowloss", e_rl[i], r3_gate(y_rl.max()))
        assert float(e_g[i]) <= r3_gate(y_g[i]), (a, float(e_g[i]), r3_gate(y_g[i]))
        assert float(e_rl[i]) <= r3_gate(y_rl.max()), (a, float(e_rl[i]), r3_gate(y_rl.max()))


def test_prompt_row_parallel_to_the_embed():
    """x_0 = 2.5 e: r = |xn - en| is rounding noise in the kernel and in both references.  With coef = (2a / sqrt(1 - r^2 / 4)) / r -> 1
    as r -> 0, the row's gradient is sc * (u - xn (xn . u)) / |x|, u = xn - en, sc = |w| / denom, i.e.
    |grad_row| |x| denom / |w| = |u_perp|.  The error of the two reciprocal norms moves u ALONG xn and is projected out; what is left
    of u is, per component, the roundings of x * (1 / |x|) and e * (1 / |e|) (2; the subtraction of two nearly equal numbers is
    exact), relative to unit-norm components: |u_perp| <= 2 * 2^-24 in fp32, + the float64 value of the fp32 inputs (2.5 e is rounded
    per component: 0.6 * 2^-24 measured), + coef, the projection and the final scaling (3 roundings ON that noise: second order).
    The bound of 16 * 2^-24 leaves that count a factor of five."""
    D = 512
    g = torch.Generator().manual_seed(D + 1)
    e = torch.randn(1, D, generator=g)
    x = torch.stack([2.5 * e[0], 3.0 * torch.randn(D, generator=g)])
    xd, ed = dev(x), dev(e)
    w, denom = 1.0, 2.0
    rl, gr, ls = prompt_launch(xd, ed, w, -INF)
    (_, _, _, g64), y_rl, y_g = prompt_yard(x, e, w, -INF)
    left64 = float(g64[0].norm() * x[0].double().norm() * denom / abs(w))
    left = float(gr[0].double().norm() * x[0].double().norm() * denom / abs(w))
    print(f"[select-fig] prompt-parallel float64 {left64 / EPS32:.2f} kernel {left / EPS32:.2f} (units of 2^-24; bound 16)")
    fig("prompt-parallel/grad", left, 16 * EPS32)
    assert left64 <= 16 * EPS32 and left <= 16 * EPS32, (left64 / EPS32, left / EPS32)
    assert bool(torch.isfinite(rl).all()) and bool(torch.isfinite(ls).all())
    e_g = row_rel(gr[1:], g64[1:])                        # the ordinary row beside it
    assert all_le(e_g, r3_gate(y_g)), (e_g, r3_gate(y_g))


def test_prompt_zero_rows():
    """rows of zeros at 0 and n - 1: F.normalize's eps floor (xn = 0, r = 1, the gradient scaled by 1 / eps = 1e12 -- finite)"""
    n, m, D, w = 6, 2, 128, 1.0
    x, e = prompt_inputs(n, m, D)
    x[0] = 0.0
    x[n - 1] = 0.0
    xd, ed = dev(x), dev(e)
    out = prompt_launch(xd, ed, w, -INF)
    r64, y_rl, y_g = prompt_yard(x, e, w, -INF)
    assert bool(torch.isfinite(out[1]).all()) and bool(torch.isfinite(r64[3]).all())
    prompt_check("prompt-zero-rows", out, r64, y_rl, y_g)


def test_prompt_refusals():
    n, m = 4, 1
    for D in (96, 1088):
        xd, ed = torch.zeros(n, D, device=DEV), torch.ones(m, D, device=DEV)
        with pytest.raises(PrxError):
            call("prx_prompt_loss_fwd_bwd", xd, ed, n, m, D, 1.0, -INF, float(n * m), torch.empty(n, device=DEV),
                 torch.empty(n, D, device=DEV), torch.empty(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), stream())
    D = 64
    xd, ed = torch.zeros(n, D, device=DEV), torch.ones(m, D, device=DEV)
    with pytest.raises(PrxError):                      # a scalar result without a ticket word
        call("prx_prompt_loss_fwd_bwd", xd, ed, n, m, D, 1.0, -INF, float(n * m), torch.empty(n, device=DEV),
             torch.empty(n, D, device=DEV), torch.empty(1, device=DEV), None, stream())
    sync()


# ================================================================================================ 2. VQ nearest
def vq_launch(tok, cb, layout, want_idx=True):
    """tokens [P][D] laid out NCHW (z[k * P + p]) or NHWC (z[p * D + k]) -> (idx [P] int64 on the CPU | None, zq [P][D])"""
    (P, D), NC = tok.shape, cb.shape[0]
    cbd = dev(cb)
    cfull, cn = flat(NC, F32)
    call("prx_k_sqnorm_rows", cbd, cfull, NC, D, stream())
    if layout == "nchw":
        z, ts, cs = dev(tok.t().contiguous()), 1, P
    else:
        z, ts, cs = dev(tok.contiguous()), D, 1
    nt = (NC + 63) // 64                                   # the header's scratch contract: [P][ceil(NC / 64)]
    pmfull, _ = guarded(P, nt, F32)
    pifull, _ = guarded(P, nt, F32)                        # int words behind a NaN pattern (no index equals its bits)
    ifull, iw = flat(P, F32)
    zfull, zq = guarded(P, D, F32)
    call("prx_k_vq_nearest", z, ts, cs, cbd, cfull, P, NC, D, pmfull, pifull, ifull if want_idx else None, zfull, stream())
    sync()
    assert untouched(cfull, 1, NC) and untouched(pmfull, P, nt) and untouched(pifull, P, nt) and untouched(zfull, P, D)
    if not want_idx:
        assert bool(torch.isnan(ifull).all())
        return None, zq
    assert untouched(ifull, 1, P)
    return iw.view(torch.int32).cpu().long(), zq


VQ_SHAPES = [(1, 1, 16), (65, 130, 16), (63, 129, 48), (140, 200, 32), (64, 128, 256), (130, 1000, 64), (257, 1024, 256),
             (5, 33000, 16)]


@pytest.mark.parametrize("P,NC,D", VQ_SHAPES)
def test_vq_shapes_both_layouts(P, NC, D):
    """P % 64 != 0, NC % 128 != 0, D = 16 (one K step: the prefetch branch never taken), 258 code tiles (`vq_select_kernel`'s second
    loop trip), NCHW and the encoder's NHWC strides"""
    g = torch.Generator().manual_seed(P * 7 + NC)
    cb = torch.randn(NC, D, generator=g)
    tok = torch.randn(P, D, generator=g)
    res = {}
    for layout in ("nchw", "nhwc"):
        idx, zq = vq_launch(tok, cb, layout)
        assert int(idx.min()) >= 0 and int(idx.max()) < NC
        if NC == 1:
            assert bool((idx == 0).all())
        else:
            bad, near, differs = vqgan_ref.vq_exactness(tok, cb, idx)
            print(f"[select-fig] vq-{P}-{NC}-{D}-{layout} near-ties {near} differs from the float64 argmin at {differs}")
            assert near <= 1, near                           # a property of the float64 distances alone
            assert bad == 0, bad
        same_bits(zq.cpu(), cb[idx])
        res[layout] = (idx, zq)
    assert torch.equal(res["nchw"][0], res["nhwc"][0])
    _, zq = vq_launch(tok, cb, "nchw", want_idx=False)       # idx_out = NULL
    same_bits(zq, res["nchw"][1])


# (NC, D, c, c2): the code row c copied to c2, bit for bit.  A thread holds the codes tx * 4 + {0..3} and 64 + tx * 4 + {0..3} of its
# 128-code tile; the workgroup's 16 partial minima are then visited in the order of tx, the tiles' in the order of the tile index
VQ_TIES = {"one-thread-neighbours": (200, 32, 5, 6), "one-thread-two-quads": (200, 32, 5, 69), "two-threads": (200, 32, 5, 9),
           "two-threads-lower-index-visited-last": (200, 32, 8, 68), "two-tiles": (300, 32, 5, 133),
           "select-loop-tile-0-and-257": (33000, 16, 5, 257 * 128 + 5),                   # two threads of vq_select_kernel
           "select-loop-tile-1-and-257": (33000, 16, 128 + 5, 257 * 128 + 5)}             # one thread, its two loop trips


@pytest.mark.parametrize("name", sorted(VQ_TIES))
def test_vq_planted_exact_ties_go_to_the_lowest_index(name):
    NC, D, c, c2 = VQ_TIES[name]
    P = 3
    g = torch.Generator().manual_seed(NC + c2)
    cb = torch.randn(NC, D, generator=g)
    cb[c2] = cb[c]
    tok = cb[c][None] + 0.05 * torch.randn(P, D, generator=g)
    xd, cd = tok.double(), cb.double()
    d64 = (xd * xd).sum(1, keepdim=True) + (cd * cd).sum(1)[None] - 2.0 * xd @ cd.t()
    pair = d64[:, c]
    rest = d64.clone()
    rest[:, [c, c2]] = INF
    tol = 8.0 * EPS32 * ((xd * xd).sum(1) + (cd * cd).sum(1)[c])         # vq_exactness's near-tie width
    assert bool((d64[:, c2] == pair).all()) and bool((rest.min(1).values - pair > 100 * tol).all())
    for layout in ("nchw", "nhwc"):
        idx, zq = vq_launch(tok, cb, layout)
        assert idx.tolist() == [c] * P, (name, layout, idx.tolist(), c, c2)
        same_bits(zq.cpu(), cb[idx])


def test_vq_refusals():
    P, NC = 4, 8
    for D, off in ((24, 0), (16, 1)):                        # D % 16 != 0; a codebook pointer 4 bytes off a 16-byte boundary
        cb = torch.zeros(NC * D + 4, device=DEV)
        assert cb.data_ptr() % 16 == 0
        nt = (NC + 63) // 64
        with pytest.raises(PrxError):
            call("prx_k_vq_nearest", torch.zeros(P * D, device=DEV), 1, P, cb[off:], torch.zeros(NC, device=DEV), P, NC, D,
                 torch.empty(P * nt, device=DEV), torch.empty(P * nt, device=DEV, dtype=torch.int32),
                 torch.empty(P, device=DEV, dtype=torch.int32), torch.empty(P * D, device=DEV), stream())
    sync()


# ================================================================================================ 3. palette loss, colour lookup
def nearest64(px, pal):
    """px [N][3], pal [np][3] (fp32) -> (idx: the lowest index among the float64-minimal entries, dmin, near-tie mask)"""
    diff = px.double()[:, None, :] - pal.double()[None, :, :]
    d2 = (diff * diff).sum(2)
    dmin = d2.min(1, keepdim=True).values
    tied = d2 == dmin
    ar = torch.arange(pal.shape[0])[None].expand_as(d2)
    idx = torch.where(tied, ar, torch.full_like(ar, pal.shape[0])).min(1).values
    nxt = d2.masked_fill(tied, INF).min(1).values
    # the fp32 chain between two squared distances: two subtractions, three squares, two additions (+ 1): 8 * 2^-24 of the second
    near = (nxt - dmin[:, 0]) < 8.0 * EPS32 * nxt
    return idx, dmin[:, 0], near, nxt


def pixels(x):
    """[n][c][hw] -> [n * hw][c]"""
    return x.permute(0, 2, 1).reshape(-1, x.shape[1])


def planes(p, n, hw):
    """[n * hw][c] -> [n][c][hw]"""
    return p.reshape(n, hw, -1).permute(0, 2, 1).contiguous()


def palette_case(name, x, pal, scale, max_near=1):
    """x [n][3][hw], pal [np][3] on the CPU: prx_palette_fwd_bwd against float64"""
    n, _, hw = x.shape
    npal = pal.shape[0]
    scale = f32v(scale)
    tk, partials = scratch()
    gfull, gr = guarded(n * 3, hw, F32)
    lfull, ls = flat(1, F32)
    call("prx_palette_fwd_bwd", dev(x), n, hw, dev(pal), npal, scale, partials, gfull, lfull, tk, stream())
    sync()
    assert untouched(gfull, n * 3, hw) and untouched(lfull, 1, 1) and int(tk.item()) == 0
    px = pixels(x)
    idx, dmin, near, nxt = nearest64(px, pal)
    assert int(near.sum()) <= max_near, int(near.sum())            # a property of the float64 distances alone
    nrm = dmin.sqrt()
    diff = px.double() - pal.double()[idx]
    g64 = torch.where(nrm[:, None] > 0, scale * diff / nrm[:, None].clamp_min(1e-300), torch.zeros_like(diff))
    loss64 = scale * float(nrm.sum())
    # R2, loss: per pixel the subtraction (1, squared: 2), the square (1) and two additions (2) under the root (halved: 2.5), the root (1):
    # 3.5 on every |p - c|; the sum and the product with scale are float64; the conversion to fp32 (1): k = 5 on the sum of positive terms
    slack = abs(scale) * float((nxt.sqrt() - nrm)[near].sum()) if bool(near.any()) else 0.0
    err = abs(float(ls) - loss64)
    fig(name + "/palette-loss", err, 5 * EPS32 * abs(loss64) + slack)
    assert err <= 5 * EPS32 * abs(loss64) + slack, (err, loss64)
    # R2, grad = (scale / nrm) * dr: nrm 3.5 (above), the division (1), dr's subtraction (1), the product (1): k = 7 on |g64|
    got, ok = pixels(gr.reshape(n, 3, hw).cpu()), ~near
    check_f32(got[ok], g64[ok], 7, g64[ok].abs())
    if bool(ok.any()) and float(g64[ok].abs().max()) > 0:
        fig(name + "/palette-grad", ((got[ok].double() - g64[ok]).abs() / g64[ok].abs().clamp_min(1e-300)).max(), 7 * EPS32)
    return idx, near, got


def lookup_case(name, x, pal, beta, max_near=1):
    """x [b][3 | 4][hw]: prx_color_lookup_fwd against float64 / bit for bit against fp32 x + (q - x)"""
    b, c, hw = x.shape
    beta = f32v(beta)
    tk, partials = scratch()
    ofull, out = guarded(b * c, hw, F32)
    qfull, lg = guarded(b * c, hw, F32)
    lfull, ls = flat(1, F32)
    call("prx_color_lookup_fwd", dev(x), b, c, hw, dev(pal), pal.shape[0], beta, partials, ofull, qfull, lfull, tk, stream())
    sync()
    assert untouched(ofull, b * c, hw) and untouched(qfull, b * c, hw) and untouched(lfull, 1, 1) and int(tk.item()) == 0
    px = pixels(x[:, :3])
    idx, dmin, near, nxt = nearest64(px, pal)
    assert int(near.sum()) <= max_near, int(near.sum())
    ok = ~near
    q = pal[idx]
    out, lg = out.reshape(b, c, hw).cpu(), lg.reshape(b, c, hw).cpu()
    same_bits(pixels(out[:, :3])[ok], (px + (q - px))[ok])                 # R1: the straight-through value, the reference's rounding
    N3 = 3.0 * b * hw
    lg64 = 2.0 * beta * (px.double() - q.double()) / N3
    # R2: gs = 2 beta / (3 N) (the division: 1), dv = q - x (1), the product (1): k = 3
    check_f32(pixels(lg[:, :3])[ok], lg64[ok], 3, lg64[ok].abs())
    loss64 = (beta + 1.0) * float(dmin.sum()) / N3
    # R2: dv (1, squared: 2), the sum and the mean in float64, the conversion (1), beta * m + m (2): k = 5
    slack = (beta + 1.0) * float((nxt - dmin)[near].sum()) / N3 if bool(near.any()) else 0.0
    err = abs(float(ls) - loss64)
    fig(name + "/lookup-loss", err, 5 * EPS32 * loss64 + slack)
    assert err <= 5 * EPS32 * loss64 + slack, (err, loss64)
    if c == 4:
        same_bits(out[:, 3], x[:, 3])                                      # R1: alpha copied
        assert bool((lg[:, 3] == 0).all())
    return idx, near, out, lg


PIXEL_SHAPES = [(1, 1), (1, 255), (1, 257), (3, 37 * 41)]


@pytest.mark.parametrize("npal", [1, 2, 7, 256])
def test_palette_and_lookup_random(npal):
    for n, hw in PIXEL_SHAPES:
        g = torch.Generator().manual_seed(1000 * npal + n * hw)
        pal = torch.rand(npal, 3, generator=g)
        c = 4 if hw % 2 else 3
        x = torch.rand(n, c, hw, generator=g) * 1.2 - 0.1
        palette_case(f"pal-{npal}-{n}x{hw}", x[:, :3].contiguous(), pal, 0.37 / (n * hw))
        lookup_case(f"pal-{npal}-{n}x{hw}", x, pal, 0.25 if npal != 7 else 1.7)


def test_palette_and_lookup_planted_ties():
    """duplicate entries at j and j + 3 (bitwise equal: either gives the same value -- nothing may go wrong around them); entries
    (0,0,0) and (1,0,0) with pixels (0.5, y, z): equidistant in fp32 and in float64 alike (0.25 + y^2 + z^2 both times), so entry 0;
    pixels bitwise on an entry: palette gradient exactly 0, lookup dv exactly 0"""
    g = torch.Generator().manual_seed(77)
    pal = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.2, 0.9, 0.9], [0.8, 0.85, 1.0], [0.5, 1.0, 0.8], [0.0, 0.0, 0.0],
                        [0.1, 0.8, 0.7], [0.9, 1.0, 0.85]])        # entries 2 .. 7 far from the x axis and from each other
    pal[5] = pal[2]                                         # j = 2, j + 3 = 5
    mid = torch.rand(20, 3, generator=g) * 0.2
    mid[:, 0] = 0.5
    dup = pal[2][None] + 0.02 * torch.randn(20, 3, generator=g)
    on = pal[[0, 1, 2, 3, 4, 5, 6, 7, 5, 2]]
    rnd = torch.rand(30, 3, generator=g)
    px = torch.cat([mid, dup, on, rnd])                     # 80 pixels = 2 x 40
    n, hw = 2, 40
    x = planes(px, n, hw)
    idx, near, got = palette_case("pal-planted", x, pal, 0.01, max_near=0)
    assert idx[:20].tolist() == [0] * 20 and idx[20:40].tolist() == [2] * 20 and idx[40:50].tolist() == [0, 1, 2, 3, 4, 2, 6, 7, 2, 2]
    assert bool((got[:20, 0] > 0).all()), "equidistant pixels must take entry 0 (the gradient points away from it)"
    assert bool((got[40:50] == 0).all()), "a pixel on its entry has the zero subgradient"
    alpha = torch.rand(n, 1, hw, generator=g)
    idx, near, out, lg = lookup_case("pal-planted", torch.cat([x, alpha], 1).contiguous(), pal, 0.25, max_near=0)
    o, l = pixels(out[:, :3]), pixels(lg[:, :3])
    assert bool((o[:20, 0] == 0).all()), "equidistant pixels must take entry 0"
    assert torch.equal(bits(o[40:50]), bits(px[40:50])) and bool((l[40:50] == 0).all())


def test_palette_and_lookup_refusals():
    x = torch.rand(1, 3, 16, device=DEV)
    pal = torch.rand(257, 3, device=DEV)
    for npal in (0, 257):
        tk, partials = scratch()
        with pytest.raises(PrxError):
            call("prx_palette_fwd_bwd", x, 1, 16, pal, npal, 1.0, partials, torch.empty_like(x), torch.empty(1, device=DEV), tk, stream())
        with pytest.raises(PrxError):
            call("prx_color_lookup_fwd", x, 1, 3, 16, pal, npal, 0.25, partials, torch.empty_like(x), torch.empty_like(x),
                 torch.empty(1, device=DEV), tk, stream())
    sync()


# ================================================================================================ 4. smoothness
def smooth_eval(x, typ, eo, sp, weight, gout, dtype):
    """float `dtype` reference on the fp32 input x [n][3][h][w] -> (loss, tfac [n][h * w], grad [n][3][h][w], s [n * h][w])"""
    n, _, h, w = x.shape
    xr = x.clone().to(dtype).requires_grad_(True)
    view = xr.permute(0, 2, 3, 1).reshape(n * h, w, 3)
    gy, gx = torch.gradient(view, spacing=sp, dim=(0, 1), edge_order=eo)
    ss = (gy * gy + gx * gx).sum(dim=2)
    nz = ss > 0                                             # flat pixels left out: the zero subgradient, not sqrt's NaN
    s = torch.sqrt(ss[nz])
    if typ == 1:
        val, dv = torch.clamp(s, max=0.5), (s <= 0.5).to(dtype)
    elif typ == 2:
        val, dv = torch.log(1.0 + s), 1.0 / (1.0 + s)
    else:
        val, dv = s, torch.ones_like(s)
    loss = weight * val.sum() / (n * h * w)
    (g,) = torch.autograd.grad(loss, xr)
    tfac = torch.zeros(n * h, w, dtype=dtype)
    tfac[nz] = (dv / s).detach()
    sfull = torch.zeros(n * h, w, dtype=dtype)
    sfull[nz] = s.detach()
    return loss.detach(), tfac.reshape(n, h * w), g * gout, sfull


def smooth_launch(x, typ, eo, sp, weight, gout):
    n, _, h, w = x.shape
    xd = dev(x)
    tk, partials = scratch()
    tfull, tf = flat(n * h * w, F32)
    lfull, ls = flat(1, F32)
    call("prx_smoothness_fwd", xd, n, h, w, typ, eo, sp, weight, partials, tfull, lfull, tk, stream())
    gfull, gr = guarded(n * 3 * h, w, F32)
    call("prx_smoothness_bwd", tfull, xd, n, h, w, eo, sp, weight, dev(torch.tensor([gout], dtype=F32)), gfull, stream())
    sync()
    assert untouched(tfull, 1, n * h * w) and untouched(lfull, 1, 1) and untouched(gfull, n * 3 * h, w) and int(tk.item()) == 0
    return ls, tf.reshape(n, h * w), gr.reshape(n, 3, h, w)


def smooth_case(name, x, typ, eo, sp, weight=0.75, gout=1.5, sides=None, loss_misses=None):
    """tfac per cutout plane and grad per (cutout, channel) plane under R3, the yardstick the worst plane of the fp32 evaluation;
    the loss under R3: asserted here, or -- with `loss_misses` -- handed back as (name, error, gate) for test_smoothness_loss_under_r3.
    type 1: every pixel at least 1e-4 from the kink in float64 (asserted), so the branch is the reference's"""
    n, _, h, w = x.shape
    ls, tf, gr = smooth_launch(x, typ, eo, sp, weight, gout)
    l64, t64, g64, s64 = smooth_eval(x, typ, eo, sp, weight, gout, torch.float64)
    l32, t32, g32, _ = smooth_eval(x, typ, eo, sp, weight, gout, F32)
    if typ == 1:
        margin = float((s64 - 0.5).abs().min())
        assert margin > 1e-4, margin
        if sides is not None:
            lo, hi = int((s64 < 0.5).sum()), int((s64 > 0.5).sum())
            assert min(lo, hi) * sides >= s64.numel(), (lo, hi)
    y_l = abs(float(l32) - float(l64)) / abs(float(l64))
    y_t = float(row_rel(t32, t64).max())
    y_g = float(row_rel(g32.reshape(n * 3, -1), g64.reshape(n * 3, -1)).max())
    e_l = abs(float(ls) - float(l64)) / abs(float(l64))
    e_t = row_rel(tf, t64)
    e_g = row_rel(gr.reshape(n * 3, -1), g64.reshape(n * 3, -1))
    print(f"[select-fig] {name} yardsticks: loss {y_l:.3e} tfac {y_t:.3e} grad {y_g:.3e}")
    fig(name + "/loss", e_l, r3_gate(y_l))
    fig(name + "/tfac", e_t.max(), r3_gate(y_t))
    fig(name + "/grad", e_g.max(), r3_gate(y_g))
    if loss_misses is None:
        assert all_le(e_t, r3_gate(y_t)), ("tfac", e_t, r3_gate(y_t))
        assert all_le(e_g, r3_gate(y_g)), ("grad", e_g, r3_gate(y_g))
    elif not e_l <= r3_gate(y_l):
        loss_misses.append((name, e_l, r3_gate(y_l)))
    return tf, gr


SMOOTH_SHAPES = [(1, 3, 3), (2, 4, 5), (3, 7, 6), (1, 17, 64)]


def flat_patch_input():
    g = torch.Generator().manual_seed(29)             # float64 margin to the kink 8.4e-4 with this draw (asserted in smooth_case)
    x = torch.rand(1, 3, 17, 64, generator=g)
    x[0, :, 5:10, 10:15] = torch.tensor([0.3, 0.6, 0.1])[:, None, None]
    return x


def smooth_all(n, h, w, loss_misses=None):
    for eo in (1, 2):
        for typ in (0, 1, 2):
            for sp in (1.0, 0.5):
                smooth_case(f"smooth-{n}x{h}x{w}-eo{eo}-t{typ}-sp{sp}", smooth_input(n, h, w, typ, eo, sp), typ, eo, sp,
                            loss_misses=loss_misses)


def smooth_input(n, h, w, typ, eo, sp):
    g = torch.Generator().manual_seed(100 * n + 10 * h + w + 7 * typ + eo)
    x = torch.rand(n, 3, h, w, generator=g)
    return x * sp if typ == 1 else x                      # type 1: magnitudes on both sides of the kink at either spacing


@pytest.mark.parametrize("n,h,w", SMOOTH_SHAPES)
def test_smoothness_cases(n, h, w):
    """3 x 3: the smallest size edge order 2 takes (every pixel an end point in both directions); 2 x 4 x 5 and 3 x 7 x 6: the row
    stencil crosses cutouts; 17 x 64: more than one workgroup"""
    smooth_all(n, h, w)


@pytest.mark.parametrize("n,h,w", SMOOTH_SHAPES)
def test_smoothness_loss_under_r3(n, h, w):
    """the scalar of the same cases (and, with the last shape, of the flat-patch cases): relative error against float64 within 4 x the
    relative error of torch's fp32 evaluation.  [1-3-3], eo 2, type 2, spacing 1.0 is the regression case of the per-pixel fp32 evaluation the
    forward kernel used to have (9.15e-8 against 2.93e-8 on the MI355X; module docstring)"""
    misses = []
    smooth_all(n, h, w, loss_misses=misses)
    if (n, h, w) == SMOOTH_SHAPES[-1]:
        for typ in (0, 1, 2):
            for eo in (1, 2):
                smooth_case(f"smooth-flat-t{typ}-eo{eo}", flat_patch_input(), typ, eo, 1.0, loss_misses=misses)
    assert misses == [], misses


@pytest.mark.parametrize("typ", [0, 1, 2])
def test_smoothness_flat_patch_and_kink(typ):
    """a constant 5 x 5 patch: tfac exactly 0 on its 3 x 3 interior (where the reference's formula is NaN), nothing flows from
    there -- the gradient at the patch's centre, whose four stencil neighbours are all flat, is exactly 0; type 1: pixels on both
    sides of s = 0.5, at least a fifth each"""
    n, h, w = 1, 17, 64
    x = flat_patch_input()
    for eo in (1, 2):
        tf, gr = smooth_case(f"smooth-flat-t{typ}-eo{eo}", x, typ, eo, 1.0, sides=5 if typ == 1 else None)
        assert bool((tf.reshape(h, w)[6:9, 11:14] == 0).all()), "tfac of a flat pixel must be exactly 0"
        assert bool((gr[0, :, 7, 12] == 0).all())
        assert bool(torch.isfinite(gr).all())


def test_smoothness_refusals():
    def fwd(h, w, typ, eo, sp):
        x = torch.rand(1, 3, h, w, device=DEV)
        tk, partials = scratch()
        call("prx_smoothness_fwd", x, 1, h, w, typ, eo, sp, 1.0, partials, torch.empty(h * w, device=DEV), torch.empty(1, device=DEV), tk,
             stream())

    def bwd(h, w, eo, sp):
        x = torch.rand(1, 3, h, w, device=DEV)
        call("prx_smoothness_bwd", torch.zeros(h * w, device=DEV), x, 1, h, w, eo, sp, 1.0, torch.ones(1, device=DEV), torch.empty_like(x),
             stream())
    for args in ((2, 4, 0, 2, 1.0), (4, 4, 3, 1, 1.0), (4, 4, 0, 1, 0.0)):      # h = 2 with edge order 2; type 3; spacing 0
        with pytest.raises(PrxError):
            fwd(*args)
    for args in ((2, 4, 2, 1.0), (4, 4, 1, 0.0)):
        with pytest.raises(PrxError):
            bwd(*args)
    sync()


# ================================================================================================ the CPU subset
def emu_subset():
    """every case of this file (they are sized for it) on the emulated kernels; returns the figures"""
    for case in PROMPT_CASES:
        test_prompt_random_cases(*case)
    test_prompt_stop_just_above_a_pair()
    test_prompt_exact_tie_on_stop()
    test_prompt_planted_angles()
    test_prompt_row_parallel_to_the_embed()
    test_prompt_zero_rows()
    test_prompt_refusals()
    for shape in VQ_SHAPES:
        test_vq_shapes_both_layouts(*shape)
    for name in sorted(VQ_TIES):
        test_vq_planted_exact_ties_go_to_the_lowest_index(name)
    test_vq_refusals()
    for npal in (1, 2, 7, 256):
        test_palette_and_lookup_random(npal)
    test_palette_and_lookup_planted_ties()
    test_palette_and_lookup_refusals()
    for shape in SMOOTH_SHAPES:
        test_smoothness_cases(*shape)
        test_smoothness_loss_under_r3(*shape)
    for typ in (0, 1, 2):
        test_smoothness_flat_patch_and_kink(typ)
    test_smoothness_refusals()
    return FIGURES
