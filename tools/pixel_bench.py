"""Forward + backward of the pixel drawer's HIP rasteriser (csrc/pixel_raster.hip) against a dense plain-torch rasteriser of the
same semantics, on the GPU.  One JSON line.

    python tools/pixel_bench.py [--iters 20]

Cases: the text2pixel preset (quality `better`, scale 2.5 -> 360 x 360) with 40 x 40 rect and 41 x 57 hex cells, and a large
canvas (1024 x 576, 81 x 91 diamond cells).  Per case: ms per forward + backward (device events around `iters` repetitions after
a warm-up), for the HIP kernels and for the torch version (which tests every sample against every shape in chunks of 64, then
composites the per-sample layers with autograd), the largest pixel difference between the two images (samples on an edge may be
decided differently), and -- for scale -- the same autograd round trip around a trivial op on the colours and the time of
three empty launches (the HIP path makes three)."""
import argparse
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_raster(verts, colors, width, height, uv):
    """dense fp32 torch rasteriser: verts [n, k, 2], colors [n, 4] (autograd), uv [H, W, 4, 2] -> [1, 4, H, W]"""
    dev = colors.device
    n, k, _ = verts.shape
    y, x = torch.meshgrid(torch.arange(height, device=dev, dtype=torch.float32), torch.arange(width, device=dev, dtype=torch.float32),
                          indexing="ij")
    s = torch.arange(4, device=dev)
    px = (x[..., None] + ((s & 1).float() + uv[..., 0]) * 0.5).reshape(-1)
    py = (y[..., None] + ((s >> 1).float() + uv[..., 1]) * 0.5).reshape(-1)
    S = px.numel()
    ss, kk = [], []
    for k0 in range(0, n, 64):
        v = verts[k0:k0 + 64]
        wn = torch.zeros(S, v.shape[0], dtype=torch.int32, device=dev)
        for e in range(k):
            ax, ay, bx, by = v[:, e - 1, 0], v[:, e - 1, 1], v[:, e, 0], v[:, e, 1]
            is_left = (bx - ax) * (py[:, None] - ay) - (px[:, None] - ax) * (by - ay)
            up = (ay <= py[:, None]) & (by > py[:, None]) & (is_left > 0)
            down = (ay > py[:, None]) & (by <= py[:, None]) & (is_left < 0)
            wn += up.int() - down.int()
        si, ji = torch.nonzero(wn != 0, as_tuple=True)
        ss.append(si)
        kk.append(ji + k0)
    si, ki = torch.cat(ss), torch.cat(kk)
    key, _ = torch.sort(si * n + ki)
    si, ki = key // n, key % n
    counts = torch.bincount(si, minlength=S)
    start = torch.cumsum(counts, 0) - counts
    depth = torch.arange(si.numel(), device=dev) - start[si]
    D = int(counts.max())
    layers = torch.full((S, max(D, 1)), -1, dtype=torch.int64, device=dev)
    layers[si, depth] = ki
    C = torch.zeros(S, 3, device=dev)
    A = torch.zeros(S, device=dev)
    for d in range(layers.shape[1]):
        ids = layers[:, d]
        on = ids >= 0
        cd = colors[ids.clamp(min=0)]
        a = cd[:, 3]
        C = torch.where(on[:, None], a[:, None] * cd[:, :3] + (1 - a[:, None]) * C, C)
        A = torch.where(on, a + (1 - a) * A, A)
    un = A > 1e-6
    rgb = torch.where(un[:, None], C / torch.where(un, A, torch.ones_like(A))[:, None], C)
    return torch.cat([rgb, A[:, None]], 1).reshape(height, width, 4, 4).mean(2).permute(2, 0, 1)[None]


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
    assert torch.cuda.is_available(), "pixel_bench measures on the GPU"
    from pixray_amd import ops
    from pixray_amd.pixel_drawer import PixelDrawer
    dev = torch.device("cuda")
    cases = [("text2pixel_rect", 360, 360, "rect"), ("text2pixel_hex", 360, 360, "hex"), ("diamond_1024x576", 1024, 576, "diamond")]
    out = []
    tiny = torch.zeros(1, device=dev)
    floor = timed(lambda: [tiny.add_(0) for _ in range(3)], 200)
    for name, w, h, typ in cases:
        st = types.SimpleNamespace(size=[w, h], pixel_size=None, pixel_scale=None, pixel_type=typ, pixel_edge_check=True,
                                   pixel_iso_check=True, transparent=False)
        d = PixelDrawer(st)
        d.load_model(st, dev)
        geom = d.geometry
        g = torch.Generator().manual_seed(0)
        col = torch.rand(geom.n_shapes, 4, generator=g)
        col[:, 3] = 1.0
        col = col.to(dev).requires_grad_(True)
        probe = torch.rand(1, 4, h, w, generator=g).to(dev)
        seed = torch.tensor([7], dtype=torch.int32, device=dev)
        verts = torch.from_numpy(d.vertices).to(dev)
        uv = ops.pixel_sample_offsets(w, h, seed)

        def hip():
            col.grad = None
            (ops.pixel_raster(col, geom, seed) * probe).sum().backward()

        def dense():
            col.grad = None
            (torch_raster(verts, col, w, h, uv) * probe).sum().backward()

        def harness():                   # the same autograd round trip around a trivial op on the colours
            col.grad = None
            (col * 1.0).sum().backward()
        t_hip = timed(hip, args.iters)
        t_harness = timed(harness, args.iters)
        t_torch = timed(dense, max(2, args.iters // 10))
        with torch.no_grad():
            diff = float((ops.pixel_raster(col, geom, seed) - torch_raster(verts, col, w, h, uv)).abs().max())
        out.append(dict(case=name, size=[w, h], grid=[d.num_cols, d.num_rows], shapes=geom.n_shapes, tile_entries=geom.n_entries,
                        hip_fwd_bwd_ms=round(t_hip, 4), trivial_op_fwd_bwd_ms=round(t_harness, 4),
                        torch_fwd_bwd_ms=round(t_torch, 3), speedup=round(t_torch / t_hip, 1), max_abs_pixel_diff=diff))
    print(json.dumps(dict(bench="pixel_raster", device=torch.cuda.get_device_name(0), three_empty_launches_ms=round(floor, 4),
                          cases=out)))


if __name__ == "__main__":
    main()
