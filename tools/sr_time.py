"""Timing of the super_resolution drawer's RRDBNet x4 runner (csrc/rrdbnet.hip) on the GPU, one process:

  1. synth + backward of RealESRGAN_x4plus (23 blocks) at z = 64 x 64 (256^2 canvas) and 128 x 128 (512^2), in the half and the
     exact-f32 operand modes: HIP events around each repetition, warm-up first, the median of `--reps` (>= 20) repetitions;
  2. beside it the same network through torch's eager conv2d in fp32 on the same GPU (forward + backward to z: the reference's own
     execution, half=False), timed the same way;
  3. one whole iteration (drawer + 64 cutouts + CLIP ViT-B/32 + prompt + fused Adam) at a 256^2 canvas, eager and graph-replayed,
     as a host clock around `--iters` iterations that end in a device synchronise.

Prints one JSON line per measurement and a final table.  Needs an MI355X: there is no CPU fallback.

    python tools/sr_time.py [--reps 20] [--iters 20] [--sizes 64 128] [--skip-session]
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F


def event_median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def torch_rrdbnet(p, z, num_block):
    """the architecture in eager torch ops (what basicsr's module executes)"""
    lr = lambda t: F.leaky_relu(t, 0.2)
    c = lambda n, t: F.conv2d(t, p[n + ".weight"], p[n + ".bias"], padding=1)
    feat = c("conv_first", z)
    x = feat
    for i in range(num_block):
        y = x
        for r in (1, 2, 3):
            q = f"body.{i}.rdb{r}.conv"
            x1 = lr(c(q + "1", y))
            x2 = lr(c(q + "2", torch.cat((y, x1), 1)))
            x3 = lr(c(q + "3", torch.cat((y, x1, x2), 1)))
            x4 = lr(c(q + "4", torch.cat((y, x1, x2, x3), 1)))
            y = c(q + "5", torch.cat((y, x1, x2, x3, x4), 1)) * 0.2 + y
        x = y * 0.2 + x
    feat = feat + c("conv_body", x)
    feat = lr(c("conv_up1", F.interpolate(feat, scale_factor=2, mode="nearest")))
    feat = lr(c("conv_up2", F.interpolate(feat, scale_factor=2, mode="nearest")))
    return c("conv_last", lr(c("conv_hr", feat))).clamp(0, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--skip-session", action="store_true")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("tools/sr_time.py needs an MI355X")
    from pixray_amd import api, ops
    from pixray_amd.weights import RRDBNET_CONFIGS, synthetic_rrdbnet_params
    dev = torch.device("cuda")
    cfg = RRDBNET_CONFIGS["RealESRGAN_x4plus"]
    params = synthetic_rrdbnet_params(cfg, 0)
    rows = []
    for n in a.sizes:
        z = torch.rand(1, 3, n, n, device=dev, requires_grad=True)
        g = torch.randn(1, 3, 4 * n, 4 * n, device=dev)
        for mode in ("fp16", "f32"):
            handle = ops.RrdbNetHandle(cfg, params, (n, n), dev, precision=mode)

            def step():
                z.grad = None
                ops.rrdbnet_synth(z, handle, True).backward(g)
            med, lo, hi = event_median_ms(step, a.reps)
            row = dict(what="hip synth+backward", z=n, mode=mode, ms_median=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3), reps=a.reps)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del handle
            torch.cuda.empty_cache()
        pd = {k: v.to(dev) for k, v in params.items()}

        def tstep():
            z.grad = None
            torch_rrdbnet(pd, z, cfg.num_block).backward(g)
        med, lo, hi = event_median_ms(tstep, a.reps)
        row = dict(what="torch eager conv2d synth+backward", z=n, mode="f32", ms_median=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                   reps=a.reps)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del pd
        torch.cuda.empty_cache()
    if not a.skip_session:
        for kind in ("eager", "graph"):
            sess = api.build_super_resolution_clip_session(size=(256, 256), clip_model="ViT-B/32", num_cuts=64, iterations=10 ** 9, device="cuda")
            it = 0
            if kind == "graph":
                ok = sess.enable_graph(warmup=3)
                if not ok:
                    print(json.dumps(dict(what="iteration", kind=kind, error=sess.graph_error)), flush=True)
                    continue
                it = 3
            else:
                for it in range(3):
                    sess.train(it)
                it = 3
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(a.iters):
                sess.train(it + k)
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0) / a.iters
            row = dict(what="iteration 256^2 ViT-B/32 64 cutouts", kind=kind, mode="fp16", ms_per_iteration=round(ms, 3), iters=a.iters)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del sess
            torch.cuda.empty_cache()
    print("\n| measurement | z | mode | ms |")
    print("|---|---|---|---|")
    for r in rows:
        print(f"| {r['what']}{' (' + r['kind'] + ')' if 'kind' in r else ''} | {r.get('z', 64)} | {r['mode']} | {r.get('ms_median', r.get('ms_per_iteration'))} |")


if __name__ == "__main__":
    main()
