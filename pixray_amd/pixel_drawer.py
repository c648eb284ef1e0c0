"""`PixelDrawer`: pixray's `pixel` drawer (pixeldrawer.py:110-410) -- a grid of filled polygons, one colour each, of one of six
cell shapes (`--pixel_type` rect, rectshift, hex, tri, diamond, knit; anything else is drawn as rect, as in the reference).

The geometry is fixed when the drawer is initialised and only the RGBA fill colours are optimised (one leaf tensor [n, 4]; the
reference keeps n separate tensors, and Adam being elementwise the arithmetic is the same).  The reference renders the shapes
with diffvg; here the colours are rendered by the polygon-coverage rasteriser of csrc/pixel_raster.hip (ops.pixel_raster), whose
conventions -- 2 x 2 jittered samples per pixel seeded by the iteration, nonzero winding, "over" in shape order, per-sample
un-premultiply -- are stated in INTEGRATION.md.

The seed (the iteration number) reaches the kernels through a one-word device buffer.  In a replayed session
(engine.Session.enable_graph) `enable_static_buffers` puts a ring of pinned buffers in front of it and `Session._host_prep` calls
`host_prep`, which stages the iteration there before the device work; eager use fills the word directly.

`sample_offsets_np` is the host twin of the kernels' jitter generator."""
import random

import numpy as np
import torch

from .interfaces import DrawingInterface

SHIFT_PIXEL_TYPES = ("hex", "rectshift", "diamond")


def _str2bool(v):
    from .frontend import str2bool
    return str2bool(v)


def grid_size(width, height, pixel_size=None, pixel_scale=None, pixel_type="rect", edge_check=True, iso_check=True):
    """(columns, rows) of the grid, as PixelDrawer.__init__ sizes it: the default grids (40 x 40 square, 40 x 50 portrait, 80 x 45
    landscape), the tri / hex / diamond iso adjustments, `pixel_scale`, shrinking to the canvas and the odd / even edge checks"""
    if pixel_size is not None:
        cols, rows = pixel_size
    elif width == height:
        cols, rows = 40, 40
    elif width < height:
        cols, rows = 40, 50
    else:
        cols, rows = 80, 45
    if iso_check and pixel_size is None:
        if pixel_type == "tri":
            cols = int(1.414 * cols)
        elif pixel_type == "hex":
            rows = int(1.414 * rows)
        elif pixel_type == "diamond":
            rows = int(2 * rows)
    if pixel_scale is not None and pixel_scale > 0:
        cols, rows = int(cols / pixel_scale), int(rows / pixel_scale)
    shrink = cols > width or rows > height
    cols, rows = min(cols, width), min(rows, height)
    if shrink:
        print("pixel grid size should not be larger than output pixel size: reducing pixel grid")
    print(f"Running pixeldrawer with {cols}x{rows} grid")
    if edge_check:
        if pixel_type in SHIFT_PIXEL_TYPES:
            cols += cols % 2 == 0
            rows += rows % 2 == 0
        elif pixel_type == "tri":
            cols += cols % 2 == 0
            rows += rows % 2 == 1
    return cols, rows


def cell_layout(cols, rows, pixel_type):
    """row-major creation order of the cells -> (row, column within the row, column offset 0 | 0.5): rows with an even index
    hold cols - 1 cells shifted by half a cell for the shifted types"""
    r = np.repeat(np.arange(rows), cols)
    c = np.tile(np.arange(cols), rows)
    off = np.zeros(rows * cols)
    if pixel_type in SHIFT_PIXEL_TYPES:
        keep = (r % 2 == 1) | (c < cols - 1)
        r, c = r[keep], c[keep]
        off = np.where(r % 2 == 0, 0.5, 0.0)
    return r, c, off[: len(r)]


def _lerp(t, lo, hi):
    """t in [start1, stop1] -> [lo, hi] with t given as the fraction (n - start1) / (stop1 - start1): fraction * (hi - lo) + lo"""
    return t * (hi - lo) + lo


def shape_vertices(width, height, cols, rows, pixel_type):
    """float32 [n, k, 2] vertices of every cell (k = 4 rect / rectshift / diamond, 3 tri, 6 hex, 8 knit), computed in float64
    and rounded once, with the corner arithmetic of the reference's shape helpers"""
    r, c, off = cell_layout(cols, rows, pixel_type)
    cw, ch = width / cols, height / rows
    x1 = (off + c) * cw
    y1 = r * ch
    x2, y2 = x1 + cw, y1 + ch
    if pixel_type == "hex":
        f = lambda n: (n - -3) / (3 - -3)                     # noqa: E731   the corner grid spans -3 .. 3
        hxh = _lerp(f(0), x1, x2)
        ya, yb, yc, yd = (_lerp(f(n), y1, y2) for n in (4, 2, -2, -4))
        pts = [(hxh, ya), (x1, yb), (x1, yc), (hxh, yd), (x2, yc), (x2, yb)]
    elif pixel_type == "tri":
        f = lambda n: (n - -1) / (1 - -1)                     # noqa: E731
        xa, xb, xh = _lerp(f(2), x1, x2), _lerp(f(-2), x1, x2), _lerp(f(0), x1, x2)
        up = (r + c) % 2 == 0
        pts = [(xh, np.where(up, y1, y2)), (np.where(up, xb, xa), np.where(up, y2, y1)), (np.where(up, xa, xb), np.where(up, y2, y1))]
    elif pixel_type == "diamond":
        f = lambda n: (n - -1) / (1 - -1)                     # noqa: E731
        ya, yb, yh = _lerp(f(-2), y1, y2), _lerp(f(2), y1, y2), _lerp(f(0), y1, y2)
        xh = _lerp(f(0), x1, x2)
        pts = [(xh, ya), (x1, yh), (xh, yb), (x2, yh)]
    elif pixel_type == "knit":
        f = lambda n: (n - 0) / (1 - 0)                       # noqa: E731
        lean_up, slump_down, fall_back = 0.45, 0.30, 0.2
        xm = (x1 + x2) / 2.0
        y_up1, y_up2 = _lerp(f(lean_up), y2, y1), _lerp(f(1 + lean_up), y2, y1)
        y_down1, y_down2 = _lerp(f(slump_down), y1, y2), _lerp(f(1 + slump_down), y1, y2)
        x_back1, x_back2 = _lerp(f(fall_back), x2, xm), _lerp(f(fall_back), x1, xm)
        pts = [(xm, y_down2), (x2, y_up1), (x2, y_up2), (x_back1, y_up2), (xm, y_down1), (x_back2, y_up2), (x1, y_up2), (x1, y_up1)]
    else:
        pts = [(x1, y1), (x2, y1), (x2, y2), (x1, y2)]
    return np.stack([np.stack([np.broadcast_to(px, r.shape), np.broadcast_to(py, r.shape)], -1) for px, py in pts], 1).astype(np.float32)


def init_sample_table(tensor_hw, cols, rows, pixel_type):
    """encode_image's sub-sampling of an init tensor of size tensor_hw = (H, W): per cell and sub-sample (x outer, y inner,
    at most 4 x 4) the pixel it reads and whether it is inside the tensor -> (iy, ix, valid) int64 / bool [P, n]"""
    th, tw = tensor_hw
    tcw, tch = tw / cols, th / rows

    def subs(cell):
        if int(cell) < 4:
            return list(range(int(cell)))
        step = cell / 4
        return [int(i * step) for i in range(4)]
    r, c, off = cell_layout(cols, rows, pixel_type)
    cur_x = (off + c) * tcw
    cur_y = np.array([int(v) for v in r * tch], dtype=np.int64) if len(r) else np.zeros(0, np.int64)
    iy, ix, valid = [], [], []
    for t_x in subs(tcw):
        sx = cur_x + t_x
        for t_y in subs(tch):
            sy = cur_y + t_y
            ok = (sx < tw) & (sy < th)
            valid.append(ok)
            ix.append(np.where(ok, np.trunc(sx), 0).astype(np.int64))
            iy.append(np.where(ok, sy, 0))
    if not valid:
        z = np.zeros((0, len(r)), dtype=np.int64)
        return z, z, z.astype(bool)
    return np.stack(iy), np.stack(ix), np.stack(valid)


def init_colors(init_tensor, cols, rows, pixel_type):
    """encode_image's cell colours from a [1, 3, H, W] tensor in [-1, 1] on its device: the mean of the in-bounds sub-samples of
    (t + 1) / 2, summed in the reference's order in fp32 (a cell without one gets 0), alpha 1 -> [n, 4]"""
    dev = init_tensor.device
    img = (init_tensor[0] + 1.0) / 2.0
    iy, ix, valid = init_sample_table(tuple(init_tensor.shape[2:4]), cols, rows, pixel_type)
    n = iy.shape[1]
    total = torch.zeros(3, n, dtype=img.dtype, device=dev)
    count = torch.zeros(n, dtype=img.dtype, device=dev)
    if iy.shape[0]:
        iy_d, ix_d = torch.from_numpy(iy).to(dev), torch.from_numpy(ix).to(dev)
        ok = torch.from_numpy(valid).to(dev)
        vals = img[:3][:, iy_d, ix_d]                        # [3, P, n]
        for p in range(iy.shape[0]):                         # at most 16 sub-samples, in the reference's order
            total = torch.where(ok[p], total + vals[:, p], total)
        count = ok.sum(0).to(img.dtype)
    rgb = total / torch.clamp(count, min=1)
    return torch.cat([rgb.t(), torch.ones(n, 1, dtype=img.dtype, device=dev)], 1).float().contiguous()


_PCG_MULT = np.uint64(6364136223846793005)


def _pcg32_step(state, inc):
    old = state
    state = old * _PCG_MULT + (inc | np.uint64(1))
    xs = (((old >> np.uint64(18)) ^ old) >> np.uint64(27)).astype(np.uint32)
    rot = (old >> np.uint64(59)).astype(np.uint32)
    return state, (xs >> rot) | (xs << ((np.uint32(32) - rot) & np.uint32(31)))


def sample_offsets_np(width, height, seed):
    """host twin of the kernels' jitter: (u, v) of sample 2 sy + sx of every pixel, float32 [H, W, 4, 2]"""
    with np.errstate(over="ignore"):
        idx = np.arange(int(width) * int(height) * 4, dtype=np.uint64)
        inc = (idx << np.uint64(1)) | np.uint64(1)
        state, _ = _pcg32_step(np.zeros_like(idx), inc)
        state = state + np.uint64(int(seed) & 0xFFFFFFFF)
        state, _ = _pcg32_step(state, inc)
        state, ru = _pcg32_step(state, inc)
        state, rv = _pcg32_step(state, inc)
    to_f = lambda r: ((r >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1)    # noqa: E731
    return np.stack([to_f(ru), to_f(rv)], -1).reshape(int(height), int(width), 4, 2)


class PixelDrawer(DrawingInterface):
    @staticmethod
    def add_settings(parser):
        parser.add_argument("--pixel_size", nargs=2, type=int, help="Pixel size (width height)", default=None, dest='pixel_size')
        parser.add_argument("--pixel_scale", type=float, help="Pixel scale", default=None, dest='pixel_scale')
        parser.add_argument("--pixel_type", type=str, help="rect, rectshift, hex, tri, diamond, knit", default="rect", dest='pixel_type')
        parser.add_argument("--pixel_edge_check", type=_str2bool, help="ensure grid is symmetric", default=True, dest='pixel_edge_check')
        parser.add_argument("--pixel_iso_check", type=_str2bool, help="ensure tri and hex shapes are w/h scaled", default=True,
                            dest='pixel_iso_check')
        return parser

    def __init__(self, settings):
        self.canvas_width, self.canvas_height = settings.size[0], settings.size[1]
        self.pixel_type = getattr(settings, "pixel_type", "rect")
        self.num_cols, self.num_rows = grid_size(self.canvas_width, self.canvas_height, getattr(settings, "pixel_size", None),
                                                 getattr(settings, "pixel_scale", None), self.pixel_type,
                                                 getattr(settings, "pixel_edge_check", True), getattr(settings, "pixel_iso_check", True))
        self.transparent = bool(getattr(settings, "transparent", False))
        self.device = torch.device("cpu")
        self.z = None
        self.img = None
        self.opts = None
        self._geom = None
        self._seed = None                # eager: the seed word, filled per synth
        self._ring = None                # replayed sessions: PinnedRing in front of the seed word
        self._staged_it = None

    def load_model(self, settings, device):
        self.device = torch.device(device)

    @property
    def vertices(self):
        """float32 [n, k, 2] cell polygons in creation order"""
        return shape_vertices(self.canvas_width, self.canvas_height, self.num_cols, self.num_rows, self.pixel_type)

    @property
    def geometry(self):
        if self._geom is None:
            from . import ops
            self._geom = ops.PixelRasterGeometry(self.vertices, self.canvas_width, self.canvas_height, self.device)
        return self._geom

    def get_opts(self, decay_divisor=1):
        self.opts = [torch.optim.Adam([self.z], lr=0.03 / decay_divisor)]
        return self.opts

    def rand_init(self, toksX=None, toksY=None):
        self.init_from_tensor(None)

    def _encode(self, init_tensor):
        if init_tensor is None:
            n = self.geometry.n_shapes
            rgb = torch.tensor([random.random() for _ in range(3 * n)], dtype=torch.float32).reshape(n, 3)
            return torch.cat([rgb, torch.ones(n, 1)], 1).to(self.device)
        return init_colors(init_tensor.detach().to(self.device), self.num_cols, self.num_rows, self.pixel_type)

    def init_from_tensor(self, init_tensor):
        self.z = self._encode(init_tensor).contiguous().requires_grad_(True)
        with torch.no_grad():
            self.img = self.synth(0)

    def reapply_from_tensor(self, new_tensor):
        with torch.no_grad():
            self.z.copy_(self._encode(new_tensor))

    def get_z_from_tensor(self, ref_tensor):
        return None

    def get_num_resolutions(self):
        return None

    # ------------------------------------------------------------------ graph-replay protocol (engine.Session)
    @property
    def graph_capturable(self):
        return self._ring is not None

    def enable_static_buffers(self, device):
        from .cutouts import PinnedRing
        self._ring = PinnedRing((1,), torch.int32, torch.device(device))
        self._staged_it = None

    def host_prep(self, args, cur_iteration):
        if self._ring is not None:
            self._stage(cur_iteration)

    def _stage(self, it):
        self._ring.stage(torch.tensor([int(it)], dtype=torch.int32))
        self._staged_it = it

    def _seed_word(self, it):
        if self._ring is not None:
            if self._staged_it != it:
                self._stage(it)
            return self._ring.dev
        if self._seed is None or self._seed.device != self.z.device:
            self._seed = torch.zeros(1, dtype=torch.int32, device=self.z.device)
        self._seed.fill_(int(it))
        return self._seed

    def synth(self, cur_iteration, return_transparency: bool = False):
        """[1, 4, H, W] RGBA of the current colours, jittered by `cur_iteration` (< 0: the last image)"""
        if return_transparency:
            raise NotImplementedError("PixelDrawer.synth(return_transparency=True) (the reference's Perlin-noise backdrop) is not "
                                      "supported; --transparent composites the RGBA image in Session.do_synth_and_filter")
        if cur_iteration is not None and cur_iteration < 0:
            return self.img
        from . import ops
        it = 0 if cur_iteration is None else int(cur_iteration)
        self.img = ops.pixel_raster(self.z, self.geometry, self._seed_word(it))
        return self.img

    @torch.no_grad()
    def to_image(self):
        from PIL import Image
        img = self.img.detach()[0, :3].permute(1, 2, 0).cpu().numpy()
        return Image.fromarray(np.uint8(np.clip(img, 0, 1) * 255), mode="RGB")

    def clip_z(self):
        with torch.no_grad():
            self.z[:, :3].clamp_(0.0, 1.0)
            self.z[:, 3].clamp_(0.0 if self.transparent else 1.0, 1.0)

    def get_z(self):
        return self.z

    def get_z_copy(self):
        return self.z.detach().clone()

    def set_z(self, new_z):
        with torch.no_grad():
            self.z.copy_(new_z)
        return None
