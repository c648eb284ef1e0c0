"""Time the ConvNeXt runner's depthwise 7x7 kernel and the whole ConvNeXt towers on the device.

Part 1 (--kernel): prx_k_cnx_dwconv alone at the four stage maps of convnext_base_w (64 x 64 x 128 ... 8 x 8 x 1024), `--cutouts` maps,
half operands, forward (bias, operand-format output) and data gradient (flipped taps, fp32 `add`, both outputs), beside
torch.nn.functional.conv2d(groups=C) on the same values in channels-last half (forward and, through autograd, the input gradient alone),
and beside the HBM floor of one read plus one write of the map at 6.3 TB/s.  The two arms alternate inside every round; HIP events on
the launch stream; warm-up rounds first; median, minimum and maximum over the rounds.
Part 2 (--towers): one forward + backward to the cutouts per tower at full depth with synthetic weights, as tools/slip_bench.py times
the ViT towers.  Reported, not gated: clocks are not pinned, so compare ratios within one run.

    timeout -k 10 900 python tools/convnext_bench.py [--cutouts 64] [--iters 20] [--warmup 5] [--kernel 1] [--towers convnext_base_w,...]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixray_amd import _lib  # noqa: E402
from pixray_amd._lib import call  # noqa: E402

HBM_BYTES_PER_S = 6.3e12           # achievable streaming rate of the part (micro-architecture notes), not the datasheet's 8 TB/s


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def kernel_rows(n, iters, warmup):
    import torch.nn.functional as F
    rows = []
    s = _lib.current_stream()
    for H, C in ((64, 128), (32, 256), (16, 512), (8, 1024)):
        g = torch.Generator().manual_seed(H)
        x = torch.randn(n, H, H, C, generator=g).cuda().half()
        w = (torch.randn(C, 49, generator=g) / 7).cuda()
        bias = torch.randn(C, generator=g).cuda()
        add = torch.randn(n, H, H, C, generator=g).cuda()
        pack = torch.empty(2 * 49 * C, dtype=torch.float16, device="cuda")
        call("prx_k_cnx_pack_dw", w, pack, C, 2, s)
        out16, out32 = torch.empty_like(x), torch.empty_like(add)
        xt = x.permute(0, 3, 1, 2).detach().requires_grad_(True)            # NCHW view of the NHWC buffer = channels_last
        wt = w.half().view(C, 1, 7, 7)
        assert xt.is_contiguous(memory_format=torch.channels_last)
        yt = F.conv2d(xt, wt, bias.half(), padding=3, groups=C)
        gt = torch.randn_like(yt)

        def ours_fwd():
            call("prx_k_cnx_dwconv", x, pack, bias, None, out16, None, n, H, H, C, 0, 2, s)

        def ours_bwd():
            call("prx_k_cnx_dwconv", x, pack, None, add, out16, out32, n, H, H, C, 1, 2, s)

        def torch_fwd():
            with torch.no_grad():
                F.conv2d(xt, wt, bias.half(), padding=3, groups=C)

        def torch_bwd():
            torch.autograd.grad(yt, xt, gt, retain_graph=True)

        t = {k: [] for k in ("ours_fwd", "torch_fwd", "ours_bwd", "torch_bwd")}
        for it in range(warmup + iters):
            for k, fn in (("ours_fwd", ours_fwd), ("torch_fwd", torch_fwd), ("ours_bwd", ours_bwd), ("torch_bwd", torch_bwd)):
                ms = _timed(fn)
                if it >= warmup:
                    t[k].append(ms)
        call("prx_k_cnx_dwconv", x, pack, bias, None, out16, None, n, H, H, C, 0, 2, s)
        torch.cuda.synchronize()
        with torch.no_grad():
            ref = F.conv2d(xt, wt, bias.half(), padding=3, groups=C).permute(0, 2, 3, 1)
        agree = float((out16.float() - ref.float()).abs().max())
        floor_ms = 2 * x.numel() * 2 / HBM_BYTES_PER_S * 1e3                # one read + one write of the half map
        row = {"map": [n, H, H, C], "hbm_floor_ms": floor_ms, "max_abs_diff_vs_torch": agree}
        for k, v in t.items():
            row[k] = _stats(v)
        row["fwd_ours_over_torch"] = row["ours_fwd"]["median_ms"] / row["torch_fwd"]["median_ms"]
        row["bwd_ours_over_torch"] = row["ours_bwd"]["median_ms"] / row["torch_bwd"]["median_ms"]
        row["fwd_ours_over_floor"] = row["ours_fwd"]["median_ms"] / floor_ms
        # the data gradient also reads the fp32 `add` and writes an fp32 twin: 2 + 2 + 4 + 4 bytes per element
        row["bwd_ours_over_its_floor"] = row["ours_bwd"]["median_ms"] / (x.numel() * 12 / HBM_BYTES_PER_S * 1e3)
        row["bwd_ours_over_floor"] = row["ours_bwd"]["median_ms"] / floor_ms
        rows.append(row)
    return rows


def tower_row(name, n, iters, warmup, precision):
    from pixray_amd.perceptor import get_clip_perceptor
    perc = get_clip_perceptor(name, "cuda", max_batch=n, precision=precision)
    R = perc.input_resolution
    g = torch.Generator().manual_seed(1)
    cut = torch.rand(n, 3, R, R, generator=g).cuda().requires_grad_(True)
    gout = torch.randn(n, perc.output_dim, generator=g).cuda()
    gc = None

    def step():
        nonlocal gc
        e = perc.encode_image(cut)
        (gc,) = torch.autograd.grad(e, cut, gout)

    times = []
    for it in range(warmup + iters):
        ms = _timed(step)
        if it >= warmup:
            times.append(ms)
    assert torch.isfinite(gc).all()
    return {"tower": name, "cutouts": n, "resolution": R, "precision": precision, "passes": iters, **_stats(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cutouts", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--kernel", type=int, default=1)
    ap.add_argument("--towers", default="convnext_base,convnext_base_w,convnext_base_w_320,convnext_large_d,convnext_large_d_320,convnext_xxlarge")
    a = ap.parse_args()
    _lib.load()
    _lib.require_device()
    if a.kernel:
        for r in kernel_rows(a.cutouts, a.iters, a.warmup):
            print(json.dumps(r), flush=True)
    for t in [t for t in a.towers.split(",") if t]:
        print(json.dumps(tower_row(t, a.cutouts, a.iters, a.warmup, a.precision)), flush=True)


if __name__ == "__main__":
    main()
