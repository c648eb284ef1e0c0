"""Forward + backward of the stroke drawers' HIP rasteriser (csrc/stroke_raster.hip) against a plain fp32 torch renderer of the
same semantics, on the GPU.  One JSON line.

    python tools/stroke_bench.py [--iters 20]

Cases: `line_sketch` at its defaults (24 strokes of 8 segments, paper underneath) at 576 x 324, and `clipdraw` with its default
1024 strokes at 384 x 216 and 768 x 432, the drawers' own initial scenes.  Per case: ms per forward + backward (device events
around `iters` repetitions after a warm-up) for the HIP kernels and for the torch version (per chunk of 64 paths: the samples in
each path's box, the closest point by the kernels' t grid and Newton steps from the best grid point only, coverage and "over"
with autograd), and the largest pixel difference between the two images (the kernels also polish the other local minima of a
segment, so the torch version can pick a farther point where a segment bends back on itself)."""
import argparse
import json
import os
import random
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _bez(t, P):
    m = 1 - t
    b = torch.stack([m * m * m, 3 * m * m * t, 3 * m * t * t, t * t * t], -1)
    b1 = torch.stack([-3 * m * m, 3 * m * m - 6 * m * t, 6 * m * t - 3 * t * t, 3 * t * t], -1)
    b2 = torch.stack([6 * m, 6 * t - 12 * m, 6 * m - 12 * t, 6 * t], -1)
    return (b[..., None] * P).sum(-2), (b1[..., None] * P).sum(-2), (b2[..., None] * P).sum(-2)


def torch_raster(points, path_start, widths, colors, paper, width, height, uv, chunk=64):
    """fp32 torch renderer: points [P, 2], widths [n], colors [n, 4], paper [4] or None (autograd) -> [H, W, 4]"""
    dev = points.device
    y, x = torch.meshgrid(torch.arange(height, device=dev, dtype=torch.float32), torch.arange(width, device=dev, dtype=torch.float32),
                          indexing="ij")
    s = torch.arange(4, device=dev)
    px = (x[..., None] + ((s & 1).float() + uv[..., 0]) * 0.5).reshape(-1)
    py = (y[..., None] + ((s >> 1).float() + uv[..., 1]) * 0.5).reshape(-1)
    S = px.numel()
    C = torch.zeros(S, 3, device=dev)
    A = torch.zeros(S, device=dev)
    if paper is not None:
        C = paper[3] * paper[:3].expand(S, 3)
        A = paper[3].expand(S)
    ps = [int(v) for v in path_start]
    tg = torch.linspace(0, 1, 33, device=dev)
    for k0 in range(0, len(ps) - 1, chunk):
        for k in range(k0, min(k0 + chunk, len(ps) - 1)):
            P = points[ps[k]:ps[k + 1]]
            r = widths[k].detach().clamp(min=0) + 1
            lo, hi = P.detach().min(0).values - r, P.detach().max(0).values + r
            idx = ((px >= lo[0]) & (px <= hi[0]) & (py >= lo[1]) & (py <= hi[1])).nonzero()[:, 0]
            if idx.numel() == 0:
                continue
            si = torch.stack([px[idx], py[idx]], 1)
            segs = torch.stack([P[3 * q:3 * q + 4] for q in range((P.shape[0] - 1) // 3)])        # [g, 4, 2]
            with torch.no_grad():
                Cg, _, _ = _bez(tg, segs.detach()[:, None])                                         # [g, 33, 2]
                d2 = ((Cg[None] - si[:, None, None]) ** 2).sum(-1)                                   # [m, g, 33]
                t = tg[d2.argmin(2)]                                                                 # [m, g]
                for _ in range(5):
                    c, c1, c2 = _bez(t, segs.detach()[None])
                    q = c - si[:, None]
                    f, fp = (q * c1).sum(-1), (c1 * c1).sum(-1) + (q * c2).sum(-1)
                    t = torch.where(fp > 0, (t - f / torch.where(fp > 0, fp, torch.ones_like(fp))).clamp(0, 1), t)
                c, _, _ = _bez(t, segs.detach()[None])
                seg = ((c - si[:, None]) ** 2).sum(-1).min(1).indices
                ts = t.gather(1, seg[:, None])[:, 0]
            cs, _, _ = _bez(ts, segs[seg])
            d = ((cs - si) ** 2).sum(1).clamp(min=1e-30).sqrt()
            a = torch.zeros(S, device=dev).index_copy(0, idx, colors[k, 3] * (widths[k] - d + 0.5).clamp(0, 1))
            C = a[:, None] * colors[k, :3] + (1 - a[:, None]) * C
            A = a + (1 - a) * A
    un = A > 1e-6
    rgb = torch.where(un[:, None], C / torch.where(un, A, torch.ones_like(A))[:, None], C)
    return torch.cat([rgb, A[:, None]], 1).reshape(height, width, 4, 4).mean(2)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "stroke_bench measures on the GPU"
    from pixray_amd import ops
    from pixray_amd.stroke_drawer import ClipDrawer, LineDrawer
    dev = torch.device("cuda")
    cases = [("line_sketch_576x324", LineDrawer, 576, 324, dict(strokes=24, stroke_length=8, min_stroke_width=0.5, max_stroke_width=2.0,
                                                                 allow_paper_color=False)),
             ("clipdraw_384x216", ClipDrawer, 384, 216, dict(strokes=1024, min_stroke_width=1.0, max_stroke_width=5.0)),
             ("clipdraw_768x432", ClipDrawer, 768, 432, dict(strokes=1024, min_stroke_width=1.0, max_stroke_width=5.0))]
    out = []
    for name, cls, w, h, opts in cases:
        st = types.SimpleNamespace(size=[w, h], **opts)
        random.seed(0)
        d = cls(st)
        d.load_model(st, dev)
        sc = d.scene
        pts, wd = d.points, d.widths
        col = d.colors.detach().clone().requires_grad_(True)
        paper = d.paper
        probe = torch.rand(h, w, 4, generator=torch.Generator().manual_seed(0)).to(dev)
        seed = torch.tensor([7], dtype=torch.int32, device=dev)
        uv = ops.stroke_sample_offsets(w, h, seed)

        def zero():
            pts.grad = wd.grad = col.grad = None

        def hip():
            zero()
            (ops.stroke_raster(pts, wd, col, paper, sc, seed) * probe).sum().backward()

        def dense():
            zero()
            (torch_raster(pts, d.path_start, wd, col, paper, w, h, uv) * probe).sum().backward()
        t_hip = timed(hip, args.iters)
        t_torch = timed(dense, 2)
        with torch.no_grad():
            diff = float((ops.stroke_raster(pts, wd, col, paper, sc, seed) - torch_raster(pts, d.path_start, wd, col, paper, w, h, uv)).abs().max())
        out.append(dict(case=name, size=[w, h], paths=sc.n_paths, points=sc.n_points, hip_fwd_bwd_ms=round(t_hip, 4),
                        torch_fwd_bwd_ms=round(t_torch, 2), speedup=round(t_torch / t_hip, 1), max_abs_pixel_diff=diff))
    print(json.dumps(dict(bench="stroke_raster", device=torch.cuda.get_device_name(0), cases=out)))


if __name__ == "__main__":
    main()
