"""Time the SLIP_VITB16 tower beside the ViT-B/16 tower of the same build: forward + backward to the cutouts at 64 cutouts, HIP
events on the launch stream, warm-up passes first, then >= 20 timed passes, one process (run it under a time limit, as in the usage line).  SLIP_VITS16 is timed too, with its algorithmic FLOPs beside those the
padded heads execute.  The two B/16 towers run the same product
shapes; they differ in one activation epilogue pair per layer (exact GELU on the generic epilogue, QuickGELU on a compile-time
one), a patch-embed bias and one LayerNorm.  Reported, not gated: clocks are not pinned, so compare ratios within one run.

    timeout -k 10 300 python tools/slip_bench.py [--cutouts 64] [--iters 20] [--warmup 5] [--precision fp16] [--towers ViT-B/16,SLIP_VITB16]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixray_amd.perceptor import get_clip_perceptor  # noqa: E402


def tower_flops(name):
    """algorithmic forward FLOPs per cutout of the blocks (2 m n k per product; attention at the tower's own head dim), and the same
    with the heads padded to 64 as the runner executes them: (algorithmic, executed)"""
    from pixray_amd.weights import CLIP_CONFIGS, SLIP_CONFIGS
    cfg = SLIP_CONFIGS.get(name) or CLIP_CONFIGS[name]
    w, t, heads = cfg.width, cfg.tokens, cfg.heads
    hd = w // heads

    def blocks(aw, d):
        qkv, proj, mlp = 2 * t * w * 3 * aw, 2 * t * aw * w, 2 * 2 * t * w * 4 * w
        att = 2 * 2 * heads * t * t * d
        return cfg.layers * (qkv + proj + mlp + att)
    return blocks(w, hd), blocks(heads * 64, 64)


def time_tower(name, n, iters, warmup, precision):
    """median over `iters` rounds of the time of one forward + backward pass; every round is timed between two HIP events on the
    launch stream, so host launch overhead that the device does not hide is part of the figure"""
    torch.cuda.init()
    free0 = torch.cuda.mem_get_info()[0]
    perc = get_clip_perceptor(name, "cuda", max_batch=n, precision=precision)
    g = torch.Generator().manual_seed(1)
    R = perc.input_resolution             # 224 for the ViT towers; --towers also takes the ConvNeXt names (256, 320: tools/convnext_bench.py)
    cut = torch.rand(n, 3, R, R, generator=g).cuda().requires_grad_(True)
    gout = torch.randn(n, perc.output_dim, generator=g).cuda()
    times = []
    for it in range(warmup + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        e = perc.encode_image(cut)
        (gc,) = torch.autograd.grad(e, cut, gout)
        b.record()
        b.synchronize()
        if it >= warmup:
            times.append(a.elapsed_time(b))
    assert torch.isfinite(gc).all()
    torch.cuda.empty_cache()              # what stays is the handles' own device memory (weights + activations for n cutouts) and `cut`
    row = {"tower": name, "cutouts": n, "precision": precision, "passes": iters, "median_ms": statistics.median(times),
           "min_ms": min(times), "max_ms": max(times), "device_gib_in_use": (free0 - torch.cuda.mem_get_info()[0]) / 2 ** 30}
    try:
        alg, run = tower_flops(name)
        row.update(fwd_gflop_per_cutout_algorithmic=alg / 1e9, fwd_gflop_per_cutout_executed=run / 1e9, executed_over_algorithmic=run / alg)
    except KeyError:
        pass
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cutouts", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--towers", default="ViT-B/16,SLIP_VITB16,SLIP_VITS16")
    a = ap.parse_args()
    rows = [time_tower(t, a.cutouts, max(a.iters, 20), a.warmup, a.precision) for t in a.towers.split(",")]
    for r in rows:
        print(json.dumps(r))
    for r in rows[1:]:
        print(json.dumps({"ratio_median": r["median_ms"] / rows[0]["median_ms"], "of": [r["tower"], rows[0]["tower"]]}))


if __name__ == "__main__":
    main()
