"""Kernel-level float64 tests (GPU) of the StyleLoss plugin's kernels, one stage at a time: the nine kernels of csrc/strotss.hip (minima
pass + finalize, the count / scan / chunk / reduce chain of the relaxed-EMD backward, the self-similarity forward / finalize /
backward) and the two of csrc/hypercolumns.hip, through the C ABI itself (`prx_strotss_*`, `prx_hypercolumns_*`): G, xs, ys, the packs
and `stats` are plain operands there, so every situation below is planted by hand -- padded strides, hand-written packs and stats,
a workspace of exactly the documented size.

Method (helpers imported from tests/test_kernels_half_gpu.py / test_kernels_runner_gpu.py): outputs are pre-filled with NaN (the packs
with zeros: a zero pack would win every atomicMin if the launcher did not reset them) and carry spare rows and stride padding that
must come back untouched; the padding of padded INPUTS is NaN, so a kernel that reads it poisons its output; every launch runs twice
and must be bit-identical (the hyper-column backward, fp32 atomics, is the documented exception).  References are plain torch on the
CPU in FLOAT64, built from the fp32 operands exactly as given: `style_loss._cos_dist` / `_l2_dist` composed on (G, xs, ys)
(`dist64`), the clamp bounds being the fp32 constants torch's fp32 clamp compares with.  Gradients: autograd through
G64 = X64 @ Y64.T + D, xs64 = (X64 ** 2).sum(1) + d with the constant offsets that reproduce the fp32 G, xs handed to the kernel;
max(a, b) hands its gradient to the larger mean, half to each on a tie (torch.max).  Nothing of strotss.hip is restated.

Gates (rule R2 of the runner file: counted fp32 roundings on the absolute values of the float64 terms; none tuned against a kernel):

* distance (`dist_bound`): q = (G / |x|) / |y| carries two square roots and two divisions (4 on |q|), 1 - q one subtraction (1 on |v|);
  L2: s = (xs + ys) - 2 G carries the addition (on xs + ys) and the subtraction (on |s|; 2 G is exact); clamp is 1-Lipschitz and exact
  where s is beyond a bound by more than that; |sqrt(a) - sqrt(b)| <= |a - b| / sqrt(b); the division and the root (2 on l2), the
  final addition (1 on |v + l2|).  The chosen index must reach the float64 minimum within the two entries' bounds, and be the float64
  arg-minimum (smallest index among exact duplicates) wherever no other entry is that close -- every row and column of every case.
* relaxed-EMD backward: |dX - dX64| <= (P_i + c) 2^-24 (|b_i| |x| + sum |a_ij| |y_j|), P_i the row's pair count (one fma per pair),
  c counted at `C_COS` / `C_L2`.
* self-similarity: per entry 4 |qx| + |Dx| + 4 |qy| + |Dy| (+ the subtraction on the difference); an entry's sign is decided when
  |Dx64 - Dy64| exceeds that; Sx / Sy: 7 roundings where both roles are decided, one of the five values (s_r + s_c) k ix elsewhere;
  cx / cy: 9 roundings, widened by exactly 2 |k| |G| ix / xs per undecided role; undecided entries <= n + 0.1 % of n^2 (asserted).
* hyper-columns: forward bit-equal to torch's left-to-right fp32 sum and within 4 roundings of float64; backward (K + 1) roundings,
  K = the largest number of contributions sharing one tap (from `rows`).

Ratios measured on an MI355X (worst kernel error / gate per gate over the file; `python -m pytest -s` prints each as a `[strotss-fig]`
line; every gate was counted before that run and not moved after it): minima value 0.62 (cosine) / 0.49 (cosine + L2), stats 0.89;
relaxed-EMD backward 0.26 / 0.18 (L2) / 0.27 / 0.30 / 0.29 / 0.34 / 0.31 for d = 1 / 3 / 255 / 256 / 257 / 2181 / 4096 on the chunk-edge
selection, 0.37 on the exact-size workspace, 0.12 across column 16384, 0.40 at n = 2085; self-similarity forward 0.005, per-row partials
0.09, Sx 0.63, Sy 0.63; cx, cy 1.00 at every n > 1 and 0.50 at n = 1 -- the sign of the diagonal entries (Dx - Dy = rounding noise
there) came out opposite to the float64 reference's, which is exactly the widening of the gate and nothing more; hyper-columns
forward 0.79, backward 0.46.  Every launch was bit-identical between its two runs.

Defect found and fixed: `prx_strotss_remd_bwd` refused `ldg < m` / `lddx < d` with a message that named neither (it printed n, m and d
only); the message now carries ldg, ldx, ldy and lddx (test_remd_bwd_refusals).  No arithmetic defect was found.

Mutation check on the emulated kernels (tools/hipemu built from a scratch copy, `emu_subset` below as tests/test_emu_cpu.py runs it).
CAUGHT: `carry` not advanced in the scan (rows left unwritten), and `carry` advanced after the first 1024 rows only (scan-2085: rows from
1024 on left unwritten); `hi` off by one, either way (chunk-edge gate, row 3); the row-minimum
pair added in every chunk (rm == cm, chunk-edge gate); `remd_reduce_kernel` starting at c0 + 1; the tie weight 0.5 replaced by 1;
`in_clamp` ignored (the pairs below / above the clamp, error 1e8 x the gate); `s_c` dropped in the self-similarity backward (decided
entries of Sx); the minima compared on the key without the index (cos-70x600-ties: rows 6 and 21 take columns 9 and 20 for 5 and 12);
the launcher's pack reset removed (zero packs win every atomicMin); the `!g` skip removed (the emulated kernel dereferences NULL: the
process dies).  NOT caught, and cannot be: `rank + pc <= lo` changed to `<` -- when rank + pc == lo the word is then walked bit by bit
instead of skipped, every bit still has rank < lo and adds no pair, and rank ends at the same value: the two forms compute the same
thing, the skip is a shortcut only."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from pixray_amd import _lib
from pixray_amd._lib import PrxError, call

import test_kernels_half_gpu as th
from test_kernels_half_gpu import guarded, untouched, within, rel_l2
from test_kernels_runner_gpu import stream, sync, check_f32

DEV = "cuda"          # tests/test_emu_cpu.py switches this (and the helper modules') to "cpu" for the emulated kernels
EPS32 = 2.0 ** -24
NAN = float("nan")
INF = float("inf")
SLACK = 1.0 + 2.0 ** -20                                             # second-order terms of the counted first-order bounds
CL_LO = float(torch.tensor(1e-5, dtype=torch.float32))              # the bounds torch's fp32 clamp(d, 1e-5, 1e5) compares with
CL_HI = 1e5
REMD_CHUNK = 16384                                                   # columns per pass of the backward's match scan (include/prx.h: d <= 4096)
REMD_DMAX = 4096
FIGURES = {}          # name -> worst (error / gate) seen, printed by the tests (`pytest -s`)


def dev(t):
    return t.to(DEV)


def fig(name, ratio):
    FIGURES[name] = max(FIGURES.get(name, 0.0), float(ratio))
    print(f"[strotss-fig] {name} {float(ratio):.4f}")


def worst(err, tol):
    """largest err / tol; 0 / 0 counts as 0, x / 0 as inf, NaN as inf"""
    if err.numel() == 0:
        return 0.0
    r = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, INF), torch.zeros_like(err)))
    return float(r.nan_to_num(nan=INF).max())


def padded(t, ld):
    """device copy of a [r, c] matrix at leading dimension ld, the padding NaN"""
    r, c = t.shape
    full = torch.full((r, ld), NAN, dtype=t.dtype)
    full[:, :c] = t
    return dev(full)


def raw(t):
    return t.contiguous().view({4: torch.int32, 8: torch.int64}[t.element_size()])


def twice(launch):
    """every launch runs twice: bit-identical"""
    a, b = launch(), launch()
    for x, y in zip(a, b):
        assert torch.equal(raw(x), raw(y)), "two runs of one launch differ"
    return a


def unpack(p):
    """{ordered value << 32 | position} (include/prx.h) -> (fp32 value, position): the order-preserving map of a float to an unsigned
    sets the sign bit of a non-negative float and complements a negative one"""
    key, idx = (p >> 32) & 0xffffffff, p & 0xffffffff
    b = torch.where((key & 0x80000000) != 0, key & 0x7fffffff, (~key) & 0xffffffff)
    b = torch.where(b >= 2 ** 31, b - 2 ** 32, b)
    return b.to(torch.int32).view(torch.float32), idx


def pack(idx):
    """a pack whose value half is a quiet NaN's bits: the backward reads positions only"""
    return (torch.full_like(idx, 0x7fc00000) << 32) | idx


# ================================================================================================ the float64 reference of the distances
def dist64(G, xs, ys, l2, d):
    """`style_loss._cos_dist` (+ `_l2_dist` when l2) composed on the product and the squared norms, in the operands' dtype"""
    M = 1. - G / torch.sqrt(xs).view(-1, 1) / torch.sqrt(ys).view(1, -1)
    if l2:
        s = xs.view(-1, 1) + ys.view(1, -1) - 2.0 * G
        M = M + torch.sqrt(torch.clamp(s, CL_LO, CL_HI) / d)
    return M


def dist_bound(G, xs, ys, l2, d):
    """(float64 distance, its counted fp32 bound) of every entry"""
    G, xs, ys = G.double(), xs.double(), ys.double()
    q = G / torch.sqrt(xs).view(-1, 1) / torch.sqrt(ys).view(1, -1)
    v = 1. - q
    tol = EPS32 * (4 * q.abs() + v.abs())                # two square roots + two divisions on |q|, one subtraction on |v|
    if l2:
        a = xs.view(-1, 1) + ys.view(1, -1)
        s = a - 2.0 * G
        ds = EPS32 * (a + s.abs())                       # the addition on xs + ys, the subtraction on |s| (2 G is exact)
        ds = torch.where((s + ds < CL_LO) | (s - ds > CL_HI), torch.zeros_like(ds), ds)      # beyond a bound either way: the clamp is exact
        l = torch.sqrt(torch.clamp(s, CL_LO, CL_HI) / d)
        # |sqrt(a) - sqrt(b)| <= |a - b| / sqrt(b); the division and the root (2 on l), the final addition (1 on |v + l|)
        tol = tol + ds / (d * l) + 2 * EPS32 * l + EPS32 * (v + l).abs()
    return dist64(G, xs, ys, l2, d), tol * SLACK


# ================================================================================================ 1. the minima pass
MINIMA_SHAPES = [(1, 1), (31, 63), (33, 257), (70, 600), (1061, 40)]


def minima_operands(n, m, l2, ties, seed):
    """G, xs, ys as independent operands: target cosine distances T in [0.3, 0.6], every row's and every column's minimum planted with
    a gap of >= 0.002 in T (row i: 0.05 + 0.002 k at column i + 3; column j: 0.01 + 0.002 k at row j + 1, modulo the size, k counting the wrap-arounds),
    G = (1 - T) |x| |y|.  L2 (d = 3): squared norms within +-0.25 % of 1.3, so that the distance stays monotone in T, plus one pair with
    x == y (s = 0: below the clamp), the last row at |x|^2 = 3e5 and the last column at |y|^2 = 2e5 (s > 1e5), all the others inside.
    ties: a few columns of G / ys and rows of G / xs duplicated exactly (within one 256-column / 32-row block and across blocks).
    Returns the operands and the representative (smallest index) of each column's / row's class of exact duplicates."""
    g = torch.Generator().manual_seed(seed)
    spread = 0.005 if l2 else 0.5
    xs = (1.3 * (1 + spread * (torch.rand(n, generator=g, dtype=torch.float64) - 0.5))).float()
    ys = (1.3 * (1 + spread * (torch.rand(m, generator=g, dtype=torch.float64) - 0.5))).float()
    T = 0.3 + 0.3 * torch.rand(n, m, generator=g, dtype=torch.float64)
    special = l2 and n >= 31 and m >= 40
    nr, mc = (n - 1, m - 1) if special else (n, m)                  # the last row / column of a special case takes no plant: it is the huge one
    for i in range(n):
        T[i, (i + 3) % mc] = 0.05 + 0.002 * (i // mc)
    for j in range(m):
        T[(j + 1) % nr, j] = 0.01 + 0.002 * (j // nr)
    if special:
        xs[n - 1], ys[m - 1] = 3e5, 2e5
        xs[2], ys[6] = 1.25, 1.25
    G = ((1 - T) * torch.sqrt(xs.double()).view(-1, 1) * torch.sqrt(ys.double()).view(1, -1)).float()
    if special:
        G[2, 6] = 1.25
    crep, rrep = torch.arange(m), torch.arange(n)
    if ties and m >= 40 and n >= 31:
        cols = [(5, 9), (20, 12)] + ([(7, m - 1), (m - 2, 40)] if m > 256 else [])
        rws = [(15, 17), (25, 14)] + ([(3, n - 1), (n - 2, 19)] if n > 32 else [])
        for s, t in cols:
            G[:, t], ys[t] = G[:, s], ys[s]
            crep[max(s, t)] = min(s, t)
        for s, t in rws:
            G[t, :], xs[t] = G[s, :], xs[s]
            rrep[max(s, t)] = min(s, t)
    return G, xs, ys, crep, rrep


def check_minima(M, tol, val, idx, rep, what, want_gap):
    """one side (rows of M): the unpacked value within the bound of the float64 distance AT the chosen index; the index reaches the
    float64 minimum within the two entries' bounds and IS the float64 arg-minimum (first of its exact duplicates) wherever no entry
    outside that class is as close; the reference alone leaves no row ambiguous.  Returns the number of rows whose minimum is tied."""
    r, c = M.shape
    ar = torch.arange(r)
    assert bool(((idx >= 0) & (idx < c)).all()), (what, "position out of range")
    mn = M.min(1).values
    jmin = (M == mn[:, None]).int().argmax(1)                       # the first of the minimal entries
    if want_gap and c > 1:
        second = M.clone()
        second[ar, jmin] = INF
        assert float((second.min(1).values - mn).min()) >= 1e-3, (what, "a planted minimum has a gap below 1e-3")
    err = (val.double() - M[ar, idx]).abs()
    fig(f"minima-value/{what}", worst(err, tol[ar, idx]))
    assert bool((err <= tol[ar, idx]).all()), (what, "unpacked minimum off by more than the counted bound", worst(err, tol[ar, idx]))
    reach = M[ar, idx] - mn
    both = tol[ar, idx] + tol[ar, jmin]
    assert bool((reach <= both).all()), (what, "chosen position misses the float64 minimum by more than twice the bound", float((reach - both).max()))
    close = (M - mn[:, None]) <= tol + tol[ar, jmin][:, None]
    ambiguous = (close & (rep[None, :] != rep[jmin][:, None])).any(1)
    assert int(ambiguous.sum()) == 0, (what, "the reference leaves rows ambiguous", int(ambiguous.sum()))
    wrong = (idx != jmin).nonzero().flatten()
    assert wrong.numel() == 0, (what, "not the float64 arg-minimum (ties: the smallest position)", wrong[:8].tolist(), idx[wrong[:8]].tolist(), jmin[wrong[:8]].tolist())
    return int(((rep[None, :] == rep[jmin][:, None]).sum(1) > 1).sum())


def run_minima(G, xs, ys, l2, d, ldg):
    """prx_strotss_remd_fwd on zero-filled packs with spare entries, twice -> (row values, row positions, column values, column
    positions, stats)"""
    n, m = G.shape
    Gd, xsd, ysd = padded(G, ldg), dev(xs), dev(ys)

    def launch():
        rp = torch.zeros(n + 3, dtype=torch.int64, device=DEV)
        cp = torch.zeros(m + 3, dtype=torch.int64, device=DEV)
        st = torch.full((8,), NAN, dtype=torch.float32, device=DEV)
        call("prx_strotss_remd_fwd", Gd, ldg, xsd, ysd, n, m, int(l2), d, rp, cp, st, stream())
        sync()
        assert int(rp[n:].abs().sum()) == 0 and int(cp[m:].abs().sum()) == 0, "spare pack entries written"
        assert bool(torch.isnan(st[3:]).all()), "stats beyond the third word written"
        return rp[:n].cpu().clone(), cp[:m].cpu().clone(), st[:3].cpu().clone()
    rp, cp, st = twice(launch)
    rv, ri = unpack(rp)
    cv, ci = unpack(cp)
    return rv, ri, cv, ci, st


def check_stats(rv, cv, st, what):
    """stats[1] / [2]: the float64 means of the unpacked minima, one rounding; stats[0]: their maximum"""
    for k, v in ((1, rv), (2, cv)):
        mean = float(v.double().mean())
        fig(f"minima-stats/{what}", abs(float(st[k]) - mean) / max(EPS32 * abs(mean), 1e-300))
        assert abs(float(st[k]) - mean) <= EPS32 * abs(mean), (what, k, float(st[k]), mean)
    assert float(st[0]) == max(float(st[1]), float(st[2])), (what, st.tolist())


@pytest.mark.parametrize("ties", [False, True], ids=["gaps", "ties"])
@pytest.mark.parametrize("l2", [False, True], ids=["cos", "cos+l2"])
@pytest.mark.parametrize("n,m", MINIMA_SHAPES)
def test_minima_pass_values_positions_ties_and_stats(n, m, l2, ties):
    """cosine (d = 515) and cosine + L2 (d = 3); ldg = m + 3 on every other shape; planted gaps (no row or column ambiguous, asserted
    from the reference alone) and exact ties (the smaller position wins, within one block and across blocks)"""
    d = 3 if l2 else 515
    G, xs, ys, crep, rrep = minima_operands(n, m, l2, ties, seed=7 * n + m + l2)
    ldg = m + 3 if MINIMA_SHAPES.index((n, m)) % 2 == 0 else m
    rv, ri, cv, ci, st = run_minima(G, xs, ys, l2, d, ldg)
    M, tol = dist_bound(G, xs, ys, l2, d)
    what = f"{'l2' if l2 else 'cos'}-{n}x{m}{'-ties' if ties else ''}"
    tr = check_minima(M, tol, rv, ri, crep, what + "/rows", not ties)
    tc = check_minima(M.t(), tol.t(), cv, ci, rrep, what + "/cols", not ties)
    if ties and n >= 31 and m >= 40:
        assert tr > 0 and tc > 0, "no tied minimum in the tie case"
    check_stats(rv, cv, st, what)
    if l2 and n >= 31 and m >= 40 and not ties:                     # the clamp cases are among the SELECTED pairs
        s = xs.double().view(-1, 1) + ys.double().view(1, -1) - 2.0 * G.double()
        sel = s[torch.arange(n), ri]
        assert bool((sel < CL_LO).any()) and bool((sel > CL_HI).any()) and bool(((sel > CL_LO) & (sel < CL_HI)).any())


def test_minima_symmetric_operands_give_bitwise_equal_means():
    """unit rows, G = (G + G^T) / 2 with the diagonal lowered, xs = ys = 1 exactly: the row and the column minima are the same numbers,
    stats[1] == stats[2] bit for bit -- the `rm == cm` situation of the backward, reached through the forward"""
    n = 70
    g = torch.Generator().manual_seed(3)
    U = torch.randn(n, 9, generator=g, dtype=torch.float64).abs()
    U = (U / U.norm(dim=1, keepdim=True)).float()
    G = U @ U.t()
    G = (G + G.t()) / 2
    G.fill_diagonal_(0.3)
    assert torch.equal(G, G.t())
    one = torch.ones(n)
    rv, ri, cv, ci, st = run_minima(G, one, one, False, 9, n + 1)
    assert torch.equal(raw(rv), raw(cv)) and torch.equal(ri, ci)
    assert torch.equal(raw(st[1:2]), raw(st[2:3])) and float(st[0]) == float(st[1])
    M, tol = dist_bound(G, one, one, False, 9)
    check_minima(M, tol, rv, ri, torch.arange(n), "symmetric/rows", False)
    check_stats(rv, cv, st, "symmetric")


# ================================================================================================ 2. the relaxed-EMD backward
# fp32 roundings of one coefficient, cosine: wt = g * sel / n (2); a = -wt / (|x| |y|): two roots, the product, the division (4) -> 6;
# b = wt G / (xs |x| |y|): wt (2), wt * G (1), the root and xs * |x| (2), the root and * |y| (2), the division (1) -> 8.
# + 2: the fma that closes a chunk (b x + acc), and the in-order chunk additions of a row cut into chunks, which put at most one more
# rounding on a term than the P_i of a straight sum.
C_COS = 8 + 2
# L2 (d = 3) adds e = wt / (d * l2) to b and subtracts it from a (same signs: no cancellation).  l2 = sqrt(clamp(s) / d): the addition and
# the subtraction of s, amplified by (xs + ys + |s|) / s <= 5.2 on the selected pairs inside the clamp (asserted) and halved by the root
# (<= 3), the division (1), the root (1) -> 5; d * l2 (1), wt (2), the division (1) -> 9 on |e| against 8 on the cosine part, + the
# addition of the two (1) -> 10; + 2 as above.
C_L2 = 10 + 2
STATS = [(0.5, 0.25), (0.25, 0.5), (0.375, 0.375)]                  # (rmean, cmean): rows carry the gradient / columns / half each
GOUTS = [1.7, -0.6]
ALL_WEIGHTS = [(s, g) for s in STATS for g in GOUTS]


def owners_from_counts(counts, m, seed):
    """owner[j] = the row whose pair column j is: row i owns counts[i] columns, interleaved in column order"""
    assert sum(counts) == m
    own = torch.cat([torch.full((c,), i, dtype=torch.int64) for i, c in enumerate(counts)])
    return own[torch.randperm(m, generator=torch.Generator().manual_seed(seed))]


def selection(name):
    """(n, m, owner [m], ridx [n]) of the hand-written packs"""
    if name == "chunk-edges":                        # rows owning 0, 1, 31, 32, 33, 64, 65 and 400 columns (and 2, 30, 35, 7)
        counts = [33, 0, 64, 400, 1, 65, 31, 32, 2, 30, 35, 7]
        n, m = 12, 700
        owner = owners_from_counts(counts, m, 1)
    elif name == "ragged-40x33":                     # every row cut into two chunks, the second one pair long: the most chunks m allows
        n, m = 40, 1320
        owner = owners_from_counts([33] * n, m, 2)
    elif name == "straddle":                         # row 0: 31 early columns + 60 across column REMD_CHUNK; row 1: wholly behind it
        n, m = 3, REMD_CHUNK + 70
        owner = torch.full((m,), 2, dtype=torch.int64)
        owner[100:131] = 0
        owner[REMD_CHUNK - 40:REMD_CHUNK + 20] = 0
        owner[REMD_CHUNK + 26:m] = 1
    elif name == "scan-2085":                        # owners on both sides of rows 1024 and 2048; row 1023 takes two chunks
        n, m = 2085, 40
        owner = torch.full((m,), 1023, dtype=torch.int64)
        owner[torch.tensor([0, 5, 11, 17, 23, 29, 35])] = torch.tensor([2048, 0, 1024, 2084, 2047, 500, 1025])
    else:
        raise KeyError(name)
    ridx = (torch.arange(n) * 37 + 11) % m
    return n, m, owner, ridx


def remd_bwd_case(sel, d, l2=False, weights=ALL_WEIGHTS, seed=0):
    n, m, owner, ridx = selection(sel)
    owner, ridx = owner.clone(), ridx.clone()
    g = torch.Generator().manual_seed(1000 * seed + d)
    X = torch.randn(n, d, generator=g).abs() + 0.05
    Y = torch.randn(m, d, generator=g).abs() + 0.05
    if l2:
        assert d == 3 and sel == "chunk-edges"
        # squared norms in [0.5, 2] and target cosine distances in [0.3, 0.6] as independent operands: s >= 0.6 |x| |y| on every pair
        xs = 0.5 + 1.5 * torch.rand(n, generator=g)
        ys = 0.5 + 1.5 * torch.rand(m, generator=g)
        T = 0.3 + 0.3 * torch.rand(n, m, generator=g, dtype=torch.float64)
        # the row-minimum pairs of rows 8..11: s exactly ON the lower / the upper bound (all the float64 arithmetic exact: one non-zero
        # channel of 2^-9 / 256), x == y (s = 0: below), |x|^2 = 3e5 (above)
        ridx[8:12] = torch.tensor([10, 20, 30, 40])
        X[8], Y[10] = torch.tensor([2.0 ** -9, 0, 0]), torch.tensor([2.0 ** -9, 0, 0])
        X[9], Y[20] = torch.tensor([256.0, 0, 0]), torch.tensor([256.0, 0, 0])
        xs[8], ys[10], xs[9], ys[20] = CL_LO, CL_LO, CL_HI, CL_HI
        xs[10], ys[30], xs[11] = 1.25, 1.25, 3e5
        G = ((1 - T) * torch.sqrt(xs.double()).view(-1, 1) * torch.sqrt(ys.double()).view(1, -1)).float()
        G[8, 10], G[9, 20], G[10, 30], G[11, 40] = 0.5 * CL_LO, 5e4, 1.25, 100.0
    else:
        G, xs, ys = X @ Y.t(), (X * X).sum(1), (Y * Y).sum(1)
    cnt = torch.bincount(owner, minlength=n)
    ar_n, ar_m = torch.arange(n), torch.arange(m)

    # ---- float64: the two means at the packs' positions, their gradients and the coefficients a (d/dG) and b (2 d/dxs) of the gate
    X64, Y64 = X.double().requires_grad_(True), Y.double()
    P = X64 @ Y64.t()
    G64 = P + (G.double() - P.detach())
    sq = (X64 ** 2).sum(1)
    xs64 = sq + (xs.double() - sq.detach())
    M = dist64(G64, xs64, ys.double(), l2, d)
    pieces = []
    for mean in (M[ar_n, ridx].mean(), M[owner, ar_m].mean()):
        gX, gG, gxs = torch.autograd.grad(mean, (X64, G64, xs64), retain_graph=True)
        pieces.append((gX, gG, gxs))
    if l2:
        s = (xs64.view(-1, 1) + ys.double().view(1, -1) - 2.0 * G64).detach()
        a = xs.double().view(-1, 1) + ys.double().view(1, -1)
        ds = EPS32 * (a + s.abs())
        for ss, aa, dd in ((s[ar_n, ridx], a[ar_n, ridx], ds[ar_n, ridx]), (s[owner, ar_m], a[owner, ar_m], ds[owner, ar_m])):
            on = (ss == CL_LO) | (ss == CL_HI)
            assert bool((on | (((ss - CL_LO).abs() > dd) & ((ss - CL_HI).abs() > dd))).all()), "a selected pair's clamp gate is undecided"
            inside = (ss >= CL_LO) & (ss <= CL_HI)
            assert float(((aa + ss.abs()) / ss)[inside].max()) <= 5.2
        sr = s[ar_n, ridx]
        assert sr[8] == CL_LO and sr[9] == CL_HI and abs(float(sr[10])) < 1e-12 and sr[11] > CL_HI
        t = torch.tensor([CL_LO, CL_HI], dtype=torch.float64, requires_grad=True)                       # ON a bound: the gradient passes
        assert torch.autograd.grad(torch.clamp(t, CL_LO, CL_HI).sum(), t)[0].tolist() == [1.0, 1.0]

    ldg, ldx, ldy, lddx = m + 1, d + 2, d + 3, d + 5
    Gd, Xd, Yd, xsd, ysd = padded(G, ldg), padded(X, ldx), padded(Y, ldy), dev(xs), dev(ys)
    rp, cp = dev(pack(ridx)), dev(pack(owner))
    nbytes = int(_lib.load().prx_strotss_remd_bwd_workspace_bytes(n, m, d))
    c_count = C_L2 if l2 else C_COS
    for (rm, cm), go in weights:
        wr, wc = (1.0, 0.0) if rm > cm else ((0.0, 1.0) if cm > rm else (0.5, 0.5))
        ref = go * (wr * pieces[0][0] + wc * pieces[1][0])
        aG = go * (wr * pieces[0][1] + wc * pieces[1][1])
        b = 2.0 * go * (wr * pieces[0][2] + wc * pieces[1][2])
        A = aG.abs() @ Y64.abs() + b.abs().view(-1, 1) * X64.detach().abs()
        pairs = (1 if wr else 0) + (cnt if wc else torch.zeros_like(cnt))
        tol = (pairs + c_count).double().view(-1, 1) * EPS32 * A * SLACK
        stats = dev(torch.tensor([NAN, rm, cm, NAN], dtype=torch.float32))
        gout = dev(torch.tensor([go], dtype=torch.float32))

        def launch():
            full, dX = guarded(n, d, torch.float32, ld=lddx)
            work = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)       # exactly the documented size + a guarded tail
            call("prx_strotss_remd_bwd", Gd, ldg, Xd, ldx, Yd, ldy, d, xsd, ysd, rp, cp, n, m, int(l2), stats, gout, work, nbytes, full, lddx,
                 stream())
            sync()
            assert untouched(full, n, d), "dX: spare rows / stride padding written"
            assert bool((work[nbytes:] == 0xA5).all()), "written behind prx_strotss_remd_bwd_workspace_bytes"
            return (dX.cpu().clone(),)
        dX, = twice(launch)
        what = f"{sel}/d{d}{'-l2' if l2 else ''}"
        assert bool(torch.isfinite(dX).all()), (what, rm, cm, go, "rows left unwritten", torch.isnan(dX).any(1).nonzero().flatten()[:8].tolist())
        if wr == 0.0:
            assert int(torch.count_nonzero(dX[cnt == 0])) == 0, (what, "rows without a pair must be exact zeros")
        err = (dX.double() - ref).abs()
        fig(f"remd-bwd/{what}", worst(err, tol))
        ok, w = within(dX, ref, tol)
        assert ok, (what, rm, cm, go, "gradient element beyond (P_i + c) 2^-24 (|b||x| + sum |a||y|)", w, w[0] // d)
    return FIGURES


@pytest.mark.parametrize("d,l2", [(1, False), (3, True), (255, False), (256, False), (257, False), (2181, False), (REMD_DMAX, False)],
                         ids=["d1", "d3-l2", "d255", "d256", "d257", "d2181", "d4096"])
def test_remd_bwd_chunk_edges_every_channel_count(d, l2):
    """n = 12, m = 700: rows owning 0, 1, 31, 32, 33, 64, 65 and 400 columns interleaved in column order (the 400-column row takes its
    row-minimum pair in chunk 0); padded ldg / ldx / ldy / lddx; rm > cm, cm > rm, rm == cm; g_out 1.7 and -0.6.  d = 3: cosine + L2
    with row-minimum pairs below, above and exactly ON the clamp bounds."""
    remd_bwd_case("chunk-edges", d, l2)


@pytest.mark.parametrize("sel,d,l2", [("ragged-40x33", 257, False), ("straddle", 3, False), ("scan-2085", 7, False)])
def test_remd_bwd_workspace_worst_case_chunk_straddle_and_scan_carry(sel, d, l2):
    """every row cut into chunks with a ragged tail in a workspace of exactly the documented size; one row's matches across column
    REMD_CHUNK and another's wholly behind it; owners on both sides of rows 1024 and 2048 of the 1024-wide scan"""
    remd_bwd_case(sel, d, l2)


def test_remd_bwd_refusals():
    """d above REMD_DMAX, ldg < m, lddx < d, a workspace one byte short or off by four bytes: PrxError naming the quantity, dX untouched.
    (Every buffer is large enough for the call as if it were accepted.)"""
    n, m, d = 12, 70, 9
    big = REMD_DMAX + 1
    g = torch.Generator().manual_seed(5)
    X, Y = dev(torch.rand(n, big, generator=g) + 0.1), dev(torch.rand(m, big, generator=g) + 0.1)
    G, xs, ys = dev(torch.rand(n, m, generator=g) + 0.1), dev(torch.rand(n, generator=g) + 1), dev(torch.rand(m, generator=g) + 1)
    rp, cp = dev(pack(torch.arange(n) % m)), dev(pack(torch.arange(m) % n))
    stats, gout = dev(torch.tensor([0.5, 0.5, 0.25, 0.0])), dev(torch.tensor([1.0]))
    nb = int(_lib.load().prx_strotss_remd_bwd_workspace_bytes(n, m, d))
    nb_big = int(_lib.load().prx_strotss_remd_bwd_workspace_bytes(n, m, big))
    assert int(_lib.load().prx_strotss_remd_bwd_workspace_bytes(0, m, d)) == -1
    work = torch.zeros(nb_big + 64, dtype=torch.uint8, device=DEV)
    assert work.data_ptr() % 16 == 0
    off4 = work[4:]
    for dd, ldg, lddx, wk, wbytes, match in [(big, m, big, work, nb_big, rf"d={big}"), (d, m - 1, big, work, nb, rf"ldg={m - 1}"),
                                             (d, m, d - 1, work, nb, rf"lddx={d - 1}"), (d, m, big, work, nb - 1, rf"workspace of {nb} bytes"),
                                             (d, m, big, off4, nb, "16-byte aligned")]:
        full, _ = guarded(n, big, torch.float32)
        with pytest.raises(PrxError, match=match):
            call("prx_strotss_remd_bwd", G, ldg, X, big, Y, big, dd, xs, ys, rp, cp, n, m, 0, stats, gout, wk, wbytes, full, lddx, stream())
        sync()
        assert bool(torch.isnan(full).all()), "a refused call wrote dX"


# ================================================================================================ 3. self-similarity
SELFSIM_SHAPES = [(1, 4), (70, 5), (257, 130), (300, 3)]


def selfsim_case(n, d, go=0.6):
    """X = |randn|, Y = |X + 0.3 randn| (the existing test's inputs); padded ldgx / ldgy / lds"""
    g = torch.Generator().manual_seed(11 * n + d)
    X = torch.randn(n, d, generator=g).abs()
    Y = (X + 0.3 * torch.randn(n, d, generator=g)).abs()
    Gx, Gy, xs, ys = X @ X.t(), Y @ Y.t(), (X * X).sum(1), (Y * Y).sum(1)
    ldgx, ldgy, lds = n + 1, n + 2, n + 3
    Gxd, Gyd, xsd, ysd = padded(Gx, ldgx), padded(Gy, ldgy), dev(xs), dev(ys)
    what = f"{n}x{d}"

    # ---- float64
    Gx64, Gy64 = Gx.double().requires_grad_(True), Gy.double().requires_grad_(True)
    xs64, ys64 = xs.double().requires_grad_(True), ys.double().requires_grad_(True)
    Dx, Dy = dist64(Gx64, xs64, xs64, False, d), dist64(Gy64, ys64, ys64, False, d)
    diff = (Dx - Dy).detach()
    L = go * torch.abs(Dx - Dy).mean()
    gGx, gGy, gxs, gys = torch.autograd.grad(L, (Gx64, Gy64, xs64, ys64))
    Sx64, Sy64, cx64, cy64 = gGx + gGx.t(), gGy + gGy.t(), 2.0 * gxs, 2.0 * gys          # dX = S X + c (.) X with c = 2 dL/dxs
    qx, qy = 1.0 - Dx.detach(), 1.0 - Dy.detach()
    # per entry: two roots + two divisions on each |q| (8 roundings near |q| = 1), the subtraction 1 - q on each |D|
    tol_d = EPS32 * (4 * qx.abs() + Dx.detach().abs() + 4 * qy.abs() + Dy.detach().abs()) * SLACK
    tol_e = tol_d + EPS32 * diff.abs()                                                  # + the subtraction Dx - Dy

    # ---- forward
    def launch_fwd():
        fp, part = guarded(1, n, torch.float64)
        fo, out = guarded(1, 1, torch.float32)
        call("prx_strotss_selfsim_fwd", Gxd, ldgx, xsd, Gyd, ldgy, ysd, n, fp, fo, stream())
        sync()
        assert untouched(fp, 1, n) and untouched(fo, 1, 1)
        return part[0].cpu().clone(), out[0].cpu().clone()
    part, out = twice(launch_fwd)
    rows64, tol_rows = diff.abs().sum(1), tol_e.sum(1) * (1 + 1e-9)                     # the row sums are float64: n * 2^-53 is nothing
    fig(f"selfsim-fwd-partial/{what}", worst((part - rows64).abs(), tol_rows))
    assert bool(((part - rows64).abs() <= tol_rows).all())
    mean64 = float(diff.abs().mean())
    tol_mean = float(tol_e.mean()) + EPS32 * mean64                                     # the mean of the per-entry bounds + the final rounding
    fig(f"selfsim-fwd/{what}", abs(float(out) - mean64) / tol_mean)
    assert abs(float(out) - mean64) <= tol_mean, (float(out), mean64, tol_mean)

    # ---- backward
    gout = dev(torch.tensor([go], dtype=torch.float32))

    def launch_bwd():
        fsx, Sx = guarded(n, n, torch.float32, ld=lds)
        fsy, Sy = guarded(n, n, torch.float32, ld=lds)
        fcx, cx = guarded(1, n, torch.float32)
        fcy, cy = guarded(1, n, torch.float32)
        call("prx_strotss_selfsim_bwd", Gxd, ldgx, xsd, Gyd, ldgy, ysd, n, gout, fsx, fsy, lds, fcx, fcy, stream())
        sync()
        assert untouched(fsx, n, n) and untouched(fsy, n, n) and untouched(fcx, 1, n) and untouched(fcy, 1, n)
        return Sx.cpu().clone(), Sy.cpu().clone(), cx[0].cpu().clone(), cy[0].cpu().clone()
    Sx, Sy, cx, cy = twice(launch_bwd)
    decided = diff.abs() > tol_d                         # (i, j): the sign of entry (i, j), i in the row role
    und = ~decided
    share = int(und.sum())
    assert share <= n + 1e-3 * n * n, ("undecided entries", share)
    assert int((und & ~torch.eye(n, dtype=torch.bool)).sum()) <= 1e-3 * n * n
    both = decided & decided.t()
    k = abs(go) / (float(n) * float(n))
    for nm, S, S64, G_, s_ in (("Sx", Sx, Sx64, Gx, xs), ("Sy", Sy, Sy64, Gy, ys)):
        a = torch.sqrt(s_.double())
        ix = 1.0 / (a.view(-1, 1) * a.view(1, -1))
        # k = g / (n * n): the product and the division (2); ix = 1 / (a_i a_j): two roots, the product, the division (4); (s_r + s_c) k is
        # exact; the product with ix (1) -> 7 on the value
        t7 = 7 * EPS32 * SLACK
        e = (S.double() - S64).abs()
        fig(f"selfsim-bwd-{nm}/{what}", worst(e[both], t7 * S64.abs()[both]))
        assert bool((e <= t7 * S64.abs())[both].all()), (nm, "decided entry off by more than 7 roundings")
        units = S.double() / (k * ix)                    # elsewhere: one of (s_r + s_c) in {-2 .. 2}, to rounding
        near = units.round()
        assert bool(((near.abs() <= 2) & ((units - near).abs() <= t7 * near.abs()))[~both].all()), (nm, "an undecided entry is none of the five values")
        # c_i = sum_j (s_r G_ij + s_c G_ji) ix / xs_i: the two products with k G (2) and their sum (1), ix (4), the product (1), the final
        # rounding of the float64 quotient (1) -> 9; an undecided role's sign is off by at most 2
        terms = k * (G_.double().abs() + G_.double().t().abs()) * ix / s_.double().view(-1, 1)
        widen = 2 * k * ((G_.double().abs() * und) + (G_.double().t().abs() * und.t())) * ix / s_.double().view(-1, 1)
        tol_c = 9 * EPS32 * SLACK * terms.sum(1) + widen.sum(1)
        c, c64 = (cx, cx64) if nm == "Sx" else (cy, cy64)
        fig(f"selfsim-bwd-c{nm[1]}/{what}", worst((c.double() - c64).abs(), tol_c))
        ok, w = within(c, c64, tol_c)
        assert ok, (nm, "norm coefficient beyond the counted bound", w)
    return FIGURES


@pytest.mark.parametrize("n,d", SELFSIM_SHAPES)
def test_selfsim_fwd_bwd(n, d):
    """mean |D(X, X) - D(Y, Y)|, the per-row partials, the symmetrised d/dG of both products and the norm coefficients against float64"""
    selfsim_case(n, d)


# ================================================================================================ 4. hyper-columns
HC_MAPS = [(8, 11, 3), (8, 11, 1), (8, 11, 16), (4, 6, 1), (4, 6, 33), (4, 6, 8), (2, 3, 64), (5, 7, 5), (5, 7, 300), (1, 1, 7), (3, 3, 2),
           (8, 11, 9)]                                   # (h, w, C): 12 maps = HC_MAX_LAYERS, two of one channel, one 2 x 3, one 1 x 1
HC_NULL = 4                                              # the map whose gradient pointer is NULL


def hc_tables(n, seed):
    """hand-built rows [L, 4, n] / wts [4 L + 2, n]: taps (y0, x0), (y0, x1), (y1, x0), (y1, x1) with x1 = min(x0 + 1, w - 1) (same for y):
    sample 0 sits on the last row AND column (its four taps are one pixel), 1 on the last row, 2 on the last column"""
    g = torch.Generator().manual_seed(seed)
    L = len(HC_MAPS)
    rows, wts = torch.empty(L, 4, n, dtype=torch.int64), torch.empty(4 * L + 2, n)
    for l, (h, w, C) in enumerate(HC_MAPS):
        y0, x0 = torch.randint(0, h, (n,), generator=g), torch.randint(0, w, (n,), generator=g)
        y0[0], x0[0] = h - 1, w - 1
        if n > 2:
            y0[1], x0[2] = h - 1, w - 1
        y1, x1 = (y0 + 1).clamp(max=h - 1), (x0 + 1).clamp(max=w - 1)
        fx, fy = torch.rand(n, generator=g), torch.rand(n, generator=g)
        rows[l] = torch.stack([y0 * w + x0, y0 * w + x1, y1 * w + x0, y1 * w + x1])
        wts[4 * l:4 * l + 4] = torch.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy])
        assert int(rows[l].min()) >= 0 and int(rows[l].max()) < h * w
    wts[4 * L:] = torch.rand(2, n, generator=g) * 10
    return rows, wts


def _ptr_array(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


@pytest.mark.parametrize("n", [1, 300])
def test_hypercolumns_fwd_bwd(n):
    g = torch.Generator().manual_seed(40 + n)
    L = len(HC_MAPS)
    feats = [torch.randn(h * w, C, generator=g) for h, w, C in HC_MAPS]
    rows, wts = hc_tables(n, n)
    chans = (ctypes.c_int * L)(*[C for _, _, C in HC_MAPS])
    ctot = sum(C for _, _, C in HC_MAPS)
    ldo = ctot + 2 + 5
    fd, rows_d, wts_d = [dev(f) for f in feats], dev(rows), dev(wts)
    ptrs = _ptr_array(fd)
    # ---- forward: the left-to-right fp32 sum of the four products (bit-equal), float64 within 4 roundings (the product + three additions)
    r32, r64, A = [], [], []
    for l, f in enumerate(feats):
        p = [f[rows[l, k]] * wts[4 * l + k].view(-1, 1) for k in range(4)]
        r32.append(((p[0] + p[1]) + p[2]) + p[3])
        p64 = [f.double()[rows[l, k]] * wts[4 * l + k].double().view(-1, 1) for k in range(4)]
        r64.append(sum(p64))
        A.append(sum(x.abs() for x in p64))
    r32, r64, A = torch.cat(r32, 1), torch.cat(r64, 1), torch.cat(A, 1)

    def launch():
        full, out = guarded(n, ctot + 2, torch.float32, ld=ldo)
        call("prx_hypercolumns_fwd", ctypes.addressof(ptrs), ctypes.addressof(chans), L, rows_d, wts_d, n, full, ldo, stream())
        sync()
        assert untouched(full, n, ctot + 2)
        return (out.cpu().clone(),)
    out, = twice(launch)
    assert torch.equal(raw(out[:, :ctot]), raw(r32)), "not the left-to-right fp32 sum of the four products"
    assert torch.equal(raw(out[:, ctot:]), raw(wts[4 * L:].t().contiguous())), "coordinate channels"
    check_f32(out[:, :ctot], r64, 4, A)
    fig(f"hypercol-fwd/n{n}", worst((out[:, :ctot].double() - r64).abs(), 4 * EPS32 * A))
    assert rel_l2(out[:, :ctot], r64) < 1e-6

    # ---- backward: the float64 scatter; K contributions at most share one tap: the product (1) + at most K additions
    go = torch.randn(n, ctot + 2, generator=g)
    go_d = padded(go, ldo)
    fulls = [torch.full((h * w + 3, C), NAN, device=DEV) for h, w, C in HC_MAPS]
    for f, (h, w, C) in zip(fulls, HC_MAPS):
        f[:h * w] = 0
    gptrs = _ptr_array([None if l == HC_NULL else f for l, f in enumerate(fulls)])
    call("prx_hypercolumns_bwd", ctypes.addressof(gptrs), ctypes.addressof(chans), L, rows_d, wts_d, n, go_d, ldo, stream())
    sync()
    off = 0
    for l, (h, w, C) in enumerate(HC_MAPS):
        gv = go[:, off:off + C].double()
        off += C
        got = fulls[l].cpu()
        assert bool(torch.isnan(got[h * w:]).all())
        if l == HC_NULL:
            assert int(torch.count_nonzero(got[:h * w])) == 0
            continue
        ref, Ab = torch.zeros(h * w, C, dtype=torch.float64), torch.zeros(h * w, C, dtype=torch.float64)
        for k in range(4):
            t = gv * wts[4 * l + k].double().view(-1, 1)
            ref.index_add_(0, rows[l, k], t)
            Ab.index_add_(0, rows[l, k], t.abs())
        K = int(torch.bincount(rows[l].flatten(), minlength=h * w).max())
        fig(f"hypercol-bwd/n{n}", worst((got[:h * w].double() - ref).abs(), (K + 1) * EPS32 * Ab))
        check_f32(got[:h * w], ref, K + 1, Ab)

    # ---- refusals: a 13th map, ldo below the column
    for nl, ld_, match in ((L + 1, ldo, "feature maps"), (L, ctot + 1, f"ldo={ctot + 1}")):
        p13 = _ptr_array(fd + [fd[0]])
        g13 = _ptr_array([None if l == HC_NULL else f for l, f in enumerate(fulls)] + [None])
        c13 = (ctypes.c_int * (L + 1))(*([C for _, _, C in HC_MAPS] + [3]))
        full, _ = guarded(n, ctot + 5, torch.float32, ld=ldo + 8)
        with pytest.raises(PrxError, match=match):
            call("prx_hypercolumns_fwd", ctypes.addressof(p13), ctypes.addressof(c13), nl, rows_d, wts_d, n, full, ld_, stream())
        with pytest.raises(PrxError, match=match):
            call("prx_hypercolumns_bwd", ctypes.addressof(g13), ctypes.addressof(c13), nl, rows_d, wts_d, n, go_d, ld_, stream())
        sync()
        assert bool(torch.isnan(full).all())


# ================================================================================================ the emulated subset
def emu_subset():
    """tests/test_emu_cpu.py: the chunk-edge case (cosine at d = 257, cosine + L2 at d = 3), the REMD_CHUNK straddle, the n = 2085 scan, the
    worst-case workspace, the tie cases, the symmetric case, the refusals, one self-similarity case and the hyper-column case"""
    remd_bwd_case("chunk-edges", 257)
    remd_bwd_case("chunk-edges", 3, True)
    remd_bwd_case("straddle", 3, weights=[(STATS[1], 1.7), (STATS[2], -0.6)])
    remd_bwd_case("scan-2085", 7, weights=[(STATS[1], 1.7), (STATS[2], -0.6)])
    remd_bwd_case("ragged-40x33", 257, weights=[(STATS[1], 1.7)])
    test_remd_bwd_refusals()
    for l2 in (False, True):
        for ties in (False, True):
            test_minima_pass_values_positions_ties_and_stats(70, 600, l2, ties)
            test_minima_pass_values_positions_ties_and_stats(33, 257, l2, ties)
    test_minima_symmetric_operands_give_bitwise_equal_means()
    test_selfsim_fwd_bwd(70, 5)
    test_hypercolumns_fwd_bwd(300)
    test_hypercolumns_fwd_bwd(1)
    return dict(FIGURES)
