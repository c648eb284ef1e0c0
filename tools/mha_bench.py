"""General-T attention kernels at the BASELINE configurations' shapes (GPU): forward and backward time per layer.
    python tools/mha_bench.py            # the default route of every shape
    PRX_MHA_TILES=1 python tools/mha_bench.py   # the one-wave-per-tile kernels everywhere
    python tools/mha_bench.py --ab 577   # ViT-L/14@336px (N = 32, T = 577, 16 heads): the workgroup family against the tile kernels
                                         # on one build in one process, the two routes alternating over --rounds rounds (prx_mha_route,
                                         # include/prx.h); prints every round, the medians, each route's spread and the verdict
    python tools/mha_bench.py --hd96 257 --cutouts 16   # the 96-wide family (heads of 80 zero-padded, OpenCLIP ViT-H-14: 16 heads) alone:
                                         # every round, the median and the spread; a single measured value, not a comparison
    python tools/mha_bench.py --hdim 257 --cutouts 16   # head dims 80 and 88 (96 columns: ViT-H-14, ViT-g-14) and 104 (128 columns:
                                         # ViT-bigG-14) one after the other in one process
The A/B verdict follows the rule for comparing two timings: a route is "faster" in a direction only if the gap between the medians
exceeds the larger of the two spreads (max - min over the rounds) measured in this very run."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from pixray_amd import _lib
from pixray_amd._lib import call, current_stream as stream

DEV = "cuda"
SHAPES = [("ViT-B/16 @128 cutouts", 128, 197, 768, 12), ("ViT-L/14 @256 cutouts", 256, 257, 1024, 16),
          ("ViT-L/14 @32 cutouts", 32, 257, 1024, 16), ("RN50x4 attention pool @128", 128, 82, 2560, 40),
          ("ViT-L/14@336px @32 cutouts", 32, 577, 1024, 16), ("RN50x16 attention pool @32", 32, 145, 3072, 48),
          ("RN50x64 attention pool @32", 32, 197, 4096, 64)]


def make_case(N, T, C, heads, dtype=torch.bfloat16, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    qkv = torch.randn(N * T, 3 * C, device=DEV, generator=g).to(dtype)
    out = torch.empty(N * T, C, dtype=dtype, device=DEV)
    lse = torch.empty(N * heads * T, device=DEV)
    do = torch.randn(N * T, C, device=DEV, generator=g).to(dtype)
    dqkv = torch.empty(N * T, 3 * C, dtype=dtype, device=DEV)
    h16 = 1 if dtype == torch.float16 else 0
    fwd = lambda: call("prx_k_mha_fwd_gen_op", qkv, out, lse, N, T, C, heads, h16, stream())
    bwd = lambda: call("prx_k_mha_bwd_gen_op", qkv, out, do, lse, dqkv, N, T, C, heads, h16, stream())
    return fwd, bwd, out, dqkv


def time_us(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def table():
    for name, N, T, C, heads in SHAPES:
        fwd, bwd, _, _ = make_case(N, T, C, heads)
        res = [time_us(fn, 20) for fn in (fwd, bwd)]
        flop_f = 4.0 * N * heads * T * T * 64
        print(f"{name:30s} T={T:4d}: forward {res[0]:8.1f} us ({flop_f / res[0] / 1e6:6.1f} TFLOP/s)   backward {res[1]:8.1f} us "
              f"({2.5 * flop_f / res[1] / 1e6:6.1f} TFLOP/s)")


def ab(T, N, heads, rounds, iters):
    """workgroup family (route 0) against the tile kernels (route 1), alternating, both operand formats"""
    lib = _lib.load()
    C = 64 * heads
    verdicts = []
    for dtype in (torch.float16, torch.bfloat16):
        fwd, bwd, out, dqkv = make_case(N, T, C, heads, dtype)
        times = {(r, d): [] for r in (0, 1) for d in ("fwd", "bwd")}
        results = {}
        for rnd in range(rounds):
            for route in ((0, 1) if rnd % 2 == 0 else (1, 0)):
                lib.prx_mha_route(route)
                times[route, "fwd"].append(time_us(fwd, iters))
                times[route, "bwd"].append(time_us(bwd, iters))
                results[route] = (out.float().clone(), dqkv.float().clone())
        lib.prx_mha_route(-1)
        # faster and different is not faster: the two routes on the same operands
        for i, what in enumerate(("out", "dqkv")):
            a, b = results[0][i], results[1][i]
            print(f"  {str(dtype):15s} {what}: routes differ by rel-L2 {float((a - b).norm() / b.norm()):.2e}")
        for d in ("fwd", "bwd"):
            row = {}
            for route, nm in ((0, "workgroups"), (1, "tiles")):
                ts = times[route, d]
                row[route] = (statistics.median(ts), max(ts) - min(ts))
                print(f"  {str(dtype):15s} {d} {nm:10s}: " + " ".join(f"{t:8.1f}" for t in ts) + f"   median {row[route][0]:8.1f} us  spread {row[route][1]:6.1f} us")
            gap, noise = row[1][0] - row[0][0], max(row[0][1], row[1][1])
            v = "workgroups faster" if gap > noise else ("tiles faster" if -gap > noise else "no difference beyond the spread")
            verdicts.append(v)
            print(f"  {str(dtype):15s} {d}: tiles - workgroups = {gap:+.1f} us against a spread of {noise:.1f} us -> {v}")
    print(f"N={N} T={T} heads={heads}: " + ("the workgroup family is faster in every direction and format"
                                            if all(v == "workgroups faster" for v in verdicts) else "the workgroup family is NOT faster throughout: " + "; ".join(verdicts)))


def hd96(T, N, heads, rounds, iters):
    """prx_k_mha_{fwd,bwd}_hd_op at 96 columns per head (head dim 80, columns 80 .. 95 of every head zero), both operand formats"""
    C = 96 * heads
    for dtype in (torch.float16, torch.bfloat16):
        g = torch.Generator(device=DEV).manual_seed(0)
        qkv = torch.randn(N * T, 3, heads, 96, device=DEV, generator=g)
        do = torch.randn(N * T, heads, 96, device=DEV, generator=g)
        qkv[..., 80:] = 0
        do[..., 80:] = 0
        qkv, do = qkv.to(dtype), do.to(dtype)
        out = torch.empty(N * T, C, dtype=dtype, device=DEV)
        lse = torch.empty(N * heads * T, device=DEV)
        dqkv = torch.empty(N * T, 3 * C, dtype=dtype, device=DEV)
        h16 = 1 if dtype == torch.float16 else 0
        fwd = lambda: call("prx_k_mha_fwd_hd_op", qkv, out, lse, N, T, C, heads, h16, 96, stream())
        bwd = lambda: call("prx_k_mha_bwd_hd_op", qkv, out, do, lse, dqkv, N, T, C, heads, h16, 96, stream())
        flop_f = 4.0 * N * heads * T * T * 80            # algorithmic: the 80 live columns
        for d, fn, fl in (("fwd", fwd, flop_f), ("bwd", bwd, 2.5 * flop_f)):
            ts = [time_us(fn, iters) for _ in range(rounds)]
            med = statistics.median(ts)
            print(f"  hd96 N={N} T={T} heads={heads} {str(dtype):15s} {d}: " + " ".join(f"{t:8.1f}" for t in ts) +
                  f"   median {med:8.1f} us  spread {max(ts) - min(ts):6.1f} us  ({fl / med / 1e6:6.1f} TFLOP/s on the live columns)")


def hdim(T, N, heads, rounds, iters, hd):
    """prx_k_mha_{fwd,bwd}_hdim_op at head dim hd in its operand columns (80 | 88 in 96, 104 in 128; the pad columns zero), both formats"""
    cols = {80: 96, 88: 96, 104: 128}[hd]
    C = cols * heads
    for dtype in (torch.float16, torch.bfloat16):
        g = torch.Generator(device=DEV).manual_seed(0)
        qkv = torch.randn(N * T, 3, heads, cols, device=DEV, generator=g)
        do = torch.randn(N * T, heads, cols, device=DEV, generator=g)
        qkv[..., hd:] = 0
        do[..., hd:] = 0
        qkv, do = qkv.to(dtype), do.to(dtype)
        out = torch.empty(N * T, C, dtype=dtype, device=DEV)
        lse = torch.empty(N * heads * T, device=DEV)
        dqkv = torch.empty(N * T, 3 * C, dtype=dtype, device=DEV)
        h16 = 1 if dtype == torch.float16 else 0
        fwd = lambda: call("prx_k_mha_fwd_hdim_op", qkv, out, lse, N, T, C, heads, h16, cols, hd, stream())
        bwd = lambda: call("prx_k_mha_bwd_hdim_op", qkv, out, do, lse, dqkv, N, T, C, heads, h16, cols, hd, stream())
        flop_f = 4.0 * N * heads * T * T * hd            # algorithmic: the live columns
        for d, fn, fl in (("fwd", fwd, flop_f), ("bwd", bwd, 2.5 * flop_f)):
            ts = [time_us(fn, iters) for _ in range(rounds)]
            med = statistics.median(ts)
            print(f"  head dim {hd} in {cols} columns N={N} T={T} heads={heads} {str(dtype):15s} {d}: " + " ".join(f"{t:8.1f}" for t in ts) +
                  f"   median {med:8.1f} us  spread {max(ts) - min(ts):6.1f} us  ({fl / med / 1e6:6.1f} TFLOP/s on the live columns)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", type=int, default=0, metavar="T", help="A/B the two routes at T tokens (64 < T <= 640)")
    ap.add_argument("--cutouts", type=int, default=32)
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--hd96", type=int, default=0, metavar="T", help="time the 96-wide family at T tokens (T <= 640)")
    ap.add_argument("--hdim", type=int, default=0, metavar="T", help="time head dims 80, 88 (96 columns) and 104 (128 columns) side by side at T tokens")
    a = ap.parse_args()
    if a.hdim:
        for hd in (80, 88, 104):
            hdim(a.hdim, a.cutouts, a.heads, a.rounds, a.iters, hd)
    elif a.hd96:
        hd96(a.hd96, a.cutouts, a.heads, a.rounds, a.iters)
    elif a.ab:
        ab(a.ab, a.cutouts, a.heads, a.rounds, a.iters)
    else:
        table()
