"""TEST ORACLE: an independent float64 torch renderer of the stroke drawers' conventions ("Stroke drawers").

Per sample (the kernels' 2 x 2 jittered positions, formed in fp32 as they are): the distance to every segment of a path by
dense sampling of t (65 values), Newton polishing from every one of them and the minimum; the path's distance is the minimum
over its segments.  Coverage clamp(w - d + 0.5, 0, 1), alpha = colour.a * coverage, the paper (if any) under everything,
"over" in path order on premultiplied colour, un-premultiplied per sample when A > 1e-6, the mean of the four samples.
Gradients come from autograd through d = |C(t*) - s| with t* detached (the envelope theorem); d = 0 gives a zero gradient.

`kink` marks samples within KINK_PX of a point where the image is not differentiable: either end of the coverage ramp, two
segments of one path (or two separated points of one segment) at equal distance; two segments meeting at the same closest
point (a joint) are no kink.  Tests leave pixels holding such a sample
out of their probes, as the pixel drawer's tests do with EDGE_PX."""
import torch

KINK_PX = 1e-3
T_GRID = 65
NEWTON = 8


def _bez(t, P):
    """t [...], P [..., 4, 2] -> C(t), C'(t), C''(t) [..., 2]"""
    m = 1 - t
    b = torch.stack([m ** 3, 3 * m * m * t, 3 * m * t * t, t ** 3], -1)
    b1 = torch.stack([-3 * m * m, 3 * m * m - 6 * m * t, 6 * m * t - 3 * t * t, 3 * t * t], -1)
    b2 = torch.stack([6 * m, -12 * m + 6 * t, 6 * m - 12 * t, 6 * t], -1)
    return (b[..., None] * P).sum(-2), (b1[..., None] * P).sum(-2), (b2[..., None] * P).sum(-2)


def sample_positions(uv, x0, y0, x1, y1):
    """fp32 sample positions as the kernels form them -> float64 [h, w, 4, 2]"""
    u = torch.as_tensor(uv)[y0:y1, x0:x1].float()
    ys = torch.arange(y0, y1, dtype=torch.float32)[:, None, None]
    xs = torch.arange(x0, x1, dtype=torch.float32)[None, :, None]
    sx = torch.tensor([0.0, 1.0, 0.0, 1.0])
    sy = torch.tensor([0.0, 0.0, 1.0, 1.0])
    px = xs + (sx + u[..., 0]) * 0.5
    py = ys + (sy + u[..., 1]) * 0.5
    return torch.stack([px, py], -1).double()


@torch.no_grad()
def _segment_distance(P, s):
    """P [4, 2], s [m, 2] -> (d [m], t [m], second-minimum gap [m]) by dense t + Newton from every grid point"""
    t = torch.linspace(0, 1, T_GRID, dtype=torch.float64, device=s.device).expand(s.shape[0], T_GRID).clone()
    for _ in range(NEWTON):
        C, D1, D2 = _bez(t, P)
        q = C - s[:, None]
        f = (q * D1).sum(-1)
        fp = (D1 * D1).sum(-1) + (q * D2).sum(-1)
        step = torch.where(fp > 0, f / torch.where(fp > 0, fp, torch.ones_like(fp)), torch.zeros_like(fp))
        t = (t - step).clamp(0, 1)
    C, _, _ = _bez(t, P)
    d = (C - s[:, None]).norm(dim=-1)
    best, i = d.min(1)
    tb = t.gather(1, i[:, None])[:, 0]
    far = (t - tb[:, None]).abs() > 0.1
    gap = torch.where(far, d - best[:, None], torch.full_like(d, float("inf"))).min(1).values
    return best, tb, gap


def render(points, path_start, widths, colors, paper, width, height, uv, crop=None):
    """-> {"image": [h, w, 4] float64 RGBA (differentiable w.r.t. the float64 leaves passed in), "kink": [h, w, 4] bool} over
    the crop (x0, y0, x1, y1) of the canvas (the whole canvas by default)"""
    x0, y0, x1, y1 = crop or (0, 0, width, height)
    dev = points.device
    pos = sample_positions(uv, x0, y0, x1, y1).to(dev)
    h, w = pos.shape[0], pos.shape[1]
    s = pos.reshape(-1, 2)
    S = s.shape[0]
    C = torch.zeros(S, 3, dtype=torch.float64, device=dev)
    A = torch.zeros(S, dtype=torch.float64, device=dev)
    if paper is not None:
        a = paper[3].expand(S)
        C = a[:, None] * paper[:3] + (1 - a[:, None]) * C
        A = a + (1 - a) * A
    kink = torch.zeros(S, dtype=torch.bool, device=dev)
    ps = [int(v) for v in path_start]
    for k in range(len(ps) - 1):
        P = points[ps[k]:ps[k + 1]]
        nseg = (P.shape[0] - 1) // 3
        if nseg < 1:
            continue
        wk = widths[k]
        wf = float(wk.detach())
        r = max(wf, 0.0) + 1.0
        lo, hi = P.detach().min(0).values - r, P.detach().max(0).values + r
        inside = ((s >= lo) & (s <= hi)).all(1)
        idx = inside.nonzero()[:, 0]
        if idx.numel() == 0:
            continue
        si = s[idx]
        segs = torch.stack([P[3 * q:3 * q + 4] for q in range(nseg)])          # [nseg, 4, 2]
        res = [_segment_distance(segs[q].detach(), si) for q in range(nseg)]
        dq = torch.stack([x[0] for x in res], 1)                               # [m, nseg]
        tq = torch.stack([x[1] for x in res], 1)
        gq = torch.stack([x[2] for x in res], 1)
        dbest, seg = dq.min(1)
        tstar = tq.gather(1, seg[:, None])[:, 0]
        cq, _, _ = _bez(tq, segs.detach()[None])                              # every segment's closest point [m, nseg, 2]
        same = (cq - cq.gather(1, seg[:, None, None].expand(-1, 1, 2))).norm(dim=-1) < 1e-4      # the same point (a shared joint)
        other = torch.where(same, torch.full_like(dq, float("inf")), dq).min(1).values
        gap = torch.minimum(other - dbest, gq.gather(1, seg[:, None])[:, 0])
        Cs, _, _ = _bez(tstar, segs[seg])                                       # differentiable in the points, t* fixed
        q = Cs - si
        d2 = (q * q).sum(1)
        pos_d = d2 > 0
        d = torch.sqrt(torch.where(pos_d, d2, torch.ones_like(d2))) * pos_d
        ramp = wk - d + 0.5
        cov = ramp.clamp(0, 1)

        rd = wf - dbest + 0.5
        near = (rd.abs() <= KINK_PX) | ((rd - 1).abs() <= KINK_PX) | ((gap <= KINK_PX) & (dbest <= wf + 0.5 + KINK_PX))
        kink = kink.index_put((idx,), kink[idx] | near)
        a = torch.zeros(S, dtype=torch.float64, device=dev).index_copy(0, idx, colors[k, 3] * cov)
        C = a[:, None] * colors[k, :3] + (1 - a[:, None]) * C
        A = a + (1 - a) * A
    un = A > 1e-6
    rgb = torch.where(un[:, None], C / torch.where(un, A, torch.ones_like(A))[:, None], C)
    out = torch.cat([rgb, A[:, None]], 1).reshape(h, w, 4, 4).mean(2)
    return {"image": out, "kink": kink.reshape(h, w, 4)}
