"""Forward + backward time of each built-in loss / filter at the headline's size (64 x 224^2 cutouts, a 256^2 image) on the HIP
kernels against a plain-torch restatement of the same plugin on the same device.  Device-event timing, warmed up; one JSON
line per plugin.

    python tools/plugin_bench.py [--iters 50] [--out results/plugin_bench.json]"""
import argparse
import json
import os
import sys
import types

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_saturation(c, w=1.0):
    p = c.permute(0, 2, 3, 1).reshape(-1, 3)
    rg = p[:, 0] - p[:, 1]
    yb = 0.5 * (p[:, 0] + p[:, 1]) - p[:, 2]
    s1, m1 = torch.std_mean(rg)
    s2, m2 = torch.std_mean(yb)
    return -(torch.sqrt(s1 ** 2 + s2 ** 2) + 0.3 * torch.sqrt(m1 ** 2 + m2 ** 2)) * w / 10


def torch_smoothness(c, w=1.0):
    p = c.permute(0, 2, 3, 1).reshape(-1, c.shape[2], 3)
    gs = [g for ch in range(3) for g in torch.gradient(p[:, :, ch])]
    return torch.sqrt(sum(g ** 2 for g in gs)).mean() * w


def torch_palette(c, pal, w=1.0):
    p = c.permute(0, 2, 3, 1).reshape(-1, 3)
    idx = torch.cdist(pal, p).argmin(0)
    return torch.norm(p - pal[idx], 2, dim=1).mean() * c.shape[0] * w / 10


def torch_symmetry(o, w=1.0):
    return F.mse_loss(o, torch.flip(o, [3])) * w


def torch_edge(o, m=12):
    z = torch.ones_like(o)
    W = o.shape[3]
    loss = F.mse_loss(o[..., :m], z[..., :m]) + F.mse_loss(o[..., W - m:], z[..., W - m:])
    loss = loss + F.mse_loss(o[:, :, :m, m:W - m], z[:, :, :m, m:W - m]) + F.mse_loss(o[:, :, -m:, m:W - m], z[:, :, -m:, m:W - m])
    return (loss + 0.05 * F.mse_loss(o, z)) * 0.1


def torch_wallpaper_shift(o):
    two = torch.cat([o, torch.roll(o, shifts=(o.shape[3] // 2,), dims=(3,))], dim=2)
    return torch.roll(two, shifts=(37, 101), dims=(2, 3))


def torch_lookup(z, pal, beta=10.0):
    z3 = z.permute(0, 2, 3, 1).contiguous()
    ind = torch.cdist(z3, pal).argmin(-1)
    q = pal[ind.flatten()].view(z3.shape)
    loss = beta * torch.mean((q.detach() - z3) ** 2) + torch.mean((q - z3.detach()) ** 2)
    return (z3 + (q - z3).detach()).permute(0, 3, 1, 2), loss


def time_fb(fn, x, iters):
    """ms per forward + backward of fn(x) -> scalar (or (tensor, scalar))"""
    def step():
        xx = x.detach().requires_grad_(True)
        r = fn(xx)
        if isinstance(r, tuple):
            r = (r[0] * r[0]).sum() + r[1]
        elif isinstance(r, list):
            r = r[0]
        r.backward()
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plugin_bench measures on an MI355X; no GPU is visible")
    from pixray_amd import builtin_losses as bl, ops
    from pixray_amd.palette import palette_from_string
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    cut = torch.rand(64, 3, 224, 224, device=dev, generator=g)
    img = torch.rand(1, 3, 256, 256, device=dev, generator=g)
    palette = palette_from_string("red->yellow")
    pal = torch.tensor(palette, dtype=torch.float32, device=dev)
    ns = types.SimpleNamespace(saturation_weight=1.0, smoothness_weight=1.0, smoothness_type="default", smoothness_spacing=1,
                               smoothness_edge_order=1, smoothness_gaussian_kernel=0, smoothness_gaussian_std=1, palette=palette,
                               palette_weight=1.0, symmetry_weight=1.0, edge_color=(1.0, 1.0, 1.0), edge_margins=(5, 5, 5, 5),
                               edge_color_weight=0.1, global_color_weight=0.05, lookup_beta=10.0, wallpaper_type="shift",
                               wallpaper_edge_match=0)
    sh = torch.tensor([37, 101], dtype=torch.int32, device=dev)
    cases = [
        ("saturation", lambda c: bl.SaturationLoss().get_loss({224: c}, None, ns), torch_saturation, cut),
        ("smoothness", lambda c: bl.SmoothnessLoss().get_loss({224: c}, None, ns), torch_smoothness, cut),
        ("palette", lambda c: bl.PaletteLoss().get_loss({224: c}, None, ns), lambda c: torch_palette(c, pal), cut),
        ("symmetry", lambda o: bl.SymmetryLoss().get_loss({}, o, ns), torch_symmetry, img),
        ("edge", lambda o: bl.EdgeLoss().get_loss({}, o, ns), torch_edge, img),
        ("wallpaper_shift", lambda o: (ops.wallpaper(o, sh, "shift", 0)[0], 0.0), lambda o: (torch_wallpaper_shift(o), 0.0), img),
        ("lookup", lambda z: ops.color_lookup(z, pal, 10.0), lambda z: torch_lookup(z, pal), img),
    ]
    rows = []
    for name, hip_fn, ref_fn, x in cases:
        t_hip = time_fb(hip_fn, x, a.iters)
        t_ref = time_fb(ref_fn, x, a.iters)
        row = dict(plugin=name, shape=list(x.shape), hip_ms=round(t_hip, 4), torch_ms=round(t_ref, 4), speedup=round(t_ref / t_hip, 2))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
