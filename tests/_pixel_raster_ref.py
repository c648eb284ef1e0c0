"""TEST ORACLE for the pixel drawer's rasteriser (csrc/pixel_raster.hip), written independently of it in float64.

Semantics: 2 x 2 jittered samples per pixel at (x + (sx + u) / 2, y + (sy + v) / 2) (fp32 positions, as the
kernels form them, from the jitter the caller hands in -- the numpy twin `pixel_drawer.sample_offsets_np`), nonzero winding,
"over" in shape order on premultiplied colour, un-premultiply per sample when A > 1e-6, uncovered samples (0, 0, 0, 0), the pixel
the mean of its samples.  Coverage is decided once in float64 and then held fixed; the colours go through torch float64 autograd
on that coverage, layer by layer (a sample's d-th covering shape is layer d).  Each sample's distance to the nearest polygon edge
comes back too, so that a test can set aside the samples whose coverage fp32 and float64 may decide differently."""
import numpy as np
import torch


def sample_positions(width, height, uv):
    """float32 positions of every sample [H, W, 4] x 2 from the jitter uv [H, W, 4, 2], as the kernels form them"""
    y, x = np.meshgrid(np.arange(height, dtype=np.float32), np.arange(width, dtype=np.float32), indexing="ij")
    s = np.arange(4)
    sx, sy = (s & 1).astype(np.float32), (s >> 1).astype(np.float32)
    half = np.float32(0.5)
    px = x[..., None] + (sx + uv[..., 0]) * half
    py = y[..., None] + (sy + uv[..., 1]) * half
    return px.astype(np.float64), py.astype(np.float64)


def _winding(poly, px, py):
    wn = np.zeros(px.shape, dtype=np.int64)
    k = len(poly)
    for i in range(k):
        (ax, ay), (bx, by) = poly[i - 1], poly[i]
        is_left = (bx - ax) * (py - ay) - (px - ax) * (by - ay)
        wn += ((ay <= py) & (by > py) & (is_left > 0)).astype(np.int64)
        wn -= ((ay > py) & (by <= py) & (is_left < 0)).astype(np.int64)
    return wn


def _edge_distance(poly, px, py):
    d = np.full(px.shape, np.inf)
    for i in range(len(poly)):
        (ax, ay), (bx, by) = poly[i - 1], poly[i]
        ex, ey = bx - ax, by - ay
        ll = ex * ex + ey * ey
        t = np.clip(((px - ax) * ex + (py - ay) * ey) / ll, 0.0, 1.0) if ll > 0 else np.zeros_like(px)
        d = np.minimum(d, np.hypot(px - (ax + t * ex), py - (ay + t * ey)))
    return d


def coverage(verts, width, height, uv):
    """-> (layers [S, D] int64 shape ids ascending per sample, -1 padded; distance to the nearest edge [S]), S = H * W * 4 in
    [H, W, 4] order"""
    px, py = sample_positions(width, height, uv)
    px, py = px.reshape(height, width * 4), py.reshape(height, width * 4)
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    dist = np.full((height, width * 4), np.inf)
    pairs_s, pairs_k = [], []
    margin = 0.01
    for k in range(v.shape[0]):
        poly = v[k]
        x0, y0 = poly.min(0) - margin
        x1, y1 = poly.max(0) + margin
        c0, c1 = max(int(np.floor(x0)), 0), min(int(np.floor(x1)), width - 1)
        r0, r1 = max(int(np.floor(y0)), 0), min(int(np.floor(y1)), height - 1)
        if c0 > c1 or r0 > r1:
            continue
        sub_x, sub_y = px[r0:r1 + 1, 4 * c0:4 * c1 + 4], py[r0:r1 + 1, 4 * c0:4 * c1 + 4]
        inside = _winding(poly, sub_x, sub_y) != 0
        dd = _edge_distance(poly, sub_x, sub_y)
        blk = dist[r0:r1 + 1, 4 * c0:4 * c1 + 4]
        np.minimum(blk, dd, out=blk)
        rr, cc = np.nonzero(inside)
        pairs_s.append((rr + r0) * (width * 4) + cc + 4 * c0)
        pairs_k.append(np.full(len(rr), k, dtype=np.int64))
    S = height * width * 4
    if pairs_s:
        s_idx, k_idx = np.concatenate(pairs_s), np.concatenate(pairs_k)
    else:
        s_idx = k_idx = np.zeros(0, dtype=np.int64)
    order = np.lexsort((k_idx, s_idx))
    s_idx, k_idx = s_idx[order], k_idx[order]
    counts = np.bincount(s_idx, minlength=S)
    D = int(counts.max()) if S else 0
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    depth = np.arange(len(s_idx)) - start[s_idx]
    layers = np.full((S, max(D, 1)), -1, dtype=np.int64)
    layers[s_idx, depth] = k_idx
    return layers, dist.reshape(-1)


def composite(colors, layers, width, height):
    """float64 torch composite on fixed coverage -> (image [1, 4, H, W], per-sample RGBA [S, 4]); differentiable w.r.t. colors"""
    c = colors.double()
    S = layers.shape[0]
    C = torch.zeros(S, 3, dtype=torch.float64)
    A = torch.zeros(S, dtype=torch.float64)
    for d in range(layers.shape[1]):
        ids = torch.from_numpy(layers[:, d])
        on = ids >= 0
        cd = c[ids.clamp(min=0)]
        a = cd[:, 3]
        C = torch.where(on[:, None], a[:, None] * cd[:, :3] + (1 - a[:, None]) * C, C)
        A = torch.where(on, a + (1 - a) * A, A)
    un = A > 1e-6
    rgb = torch.where(un[:, None], C / torch.where(un, A, torch.ones_like(A))[:, None], C)
    samples = torch.cat([rgb, A[:, None]], 1)
    img = samples.reshape(height, width, 4, 4).mean(2).permute(2, 0, 1)[None]
    return img, samples


def shade(layers, dist, colors, width, height, probe=None):
    """-> dict(ids [H, W, 4] topmost shape or -1, dist [H, W, 4], image [1, 4, H, W] float64, grad [n, 4] float64 of
    sum(probe * image) (None without a probe)) on the coverage `coverage` returned"""
    col = torch.as_tensor(colors, dtype=torch.float64).detach().clone().requires_grad_(probe is not None)
    img, _ = composite(col, layers, width, height)
    grad = None
    if probe is not None:
        (grad,) = torch.autograd.grad((img * torch.as_tensor(probe, dtype=torch.float64)).sum(), col)
    valid = layers >= 0
    top = np.where(valid.any(1), layers[np.arange(len(layers)), np.maximum(valid.sum(1) - 1, 0)], -1)
    return dict(ids=top.reshape(height, width, 4), dist=dist.reshape(height, width, 4), image=img.detach(), grad=grad)


def render(verts, colors, width, height, uv, probe=None):
    """coverage + shade"""
    layers, dist = coverage(verts, width, height, uv)
    return shade(layers, dist, colors, width, height, probe)
