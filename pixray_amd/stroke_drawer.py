"""`LineDrawer` and `ClipDrawer`: pixray's two stroke drawers, `line_sketch` (linedrawer.py) and `clipdraw` (clipdrawer.py).

Both draw open paths of cubic Bezier segments (1 + 3 S points per path, in pixels), each with a scalar stroke width and an RGBA
stroke colour, and optimise the control points and widths (and the colours for clipdraw, the paper colour for line_sketch with
`--allow_paper_color`).  Their options, the Python `random` initialisation and the optimisers are the reference's; one leaf
tensor holds each kind of parameter (points [P, 2] with a CSR `path_start`, widths [n], colours [n, 4], paper [4]) where the
reference keeps one tensor per path, and Adam being elementwise the steps are the same.

The reference renders with diffvg.  Here the strokes are rendered by csrc/stroke_raster.hip (ops.stroke_raster), whose
conventions -- the pixel drawer's 2 x 2 jittered samples, the exact distance to the centre line, stroke_width as the
half-width, a pre-filtered one-pixel coverage ramp and its exact gradient, "over" in path order above the paper -- are stated in
INTEGRATION.md.  `synth` composites the RGBA raster over white and returns [1, 3, H, W], as the reference does.

The seed (the iteration number) reaches the kernels through a one-word device buffer, staged through a pinned ring in a
replayed session (`enable_static_buffers` / `host_prep`), as in PixelDrawer."""
import random
from xml.sax.saxutils import quoteattr

import numpy as np
import torch

from .interfaces import DrawingInterface

PAPER_COLOR = (242 / 255.0, 238 / 255.0, 203 / 255.0, 1.0)
MAX_SEGMENTS = 64                        # per path: the kernels' limit (ops.STROKE_MAX_POINTS = 1 + 3 * 64)


def _str2bool(v):
    from .frontend import str2bool
    return str2bool(v)


def _clamp01(v):
    return max(0, min(1, v))


def line_sketch_paths(num_paths, stroke_length, width, height):
    """line_sketch's initial paths from Python's `random` (linedrawer.py:74-94): a random walk of `stroke_length` segments from
    near the centre, each segment's start clamped to the unit square -> list of float32 [1 + 3 S, 2] tensors in pixels"""
    paths = []
    for _ in range(num_paths):
        walk = []
        start = (0.5 + 0.5 * (random.random() - 0.5), 0.5 + 0.5 * (random.random() - 0.5))
        walk.append(start)
        for _ in range(stroke_length):
            ry = 1.0 / (stroke_length + 2)
            rx = ry * height / width
            prev = start
            for _ in range(3):
                prev = (prev[0] + rx * (random.random() - 0.5), prev[1] + ry * (random.random() - 0.5))
                walk.append(prev)
            start = (_clamp01(prev[0]), _clamp01(prev[1]))
        paths.append(_to_pixels(walk, width, height))
    return paths


def clipdraw_paths(num_paths, width, height):
    """clipdraw's initial paths and colours from Python's `random` (clipdrawer.py:48-69): 1 to 3 segments from a uniform
    start, each control point within 0.05 of the previous one -> (list of float32 [1 + 3 S, 2] tensors, float32 [n, 4])"""
    paths, colors = [], []
    for _ in range(num_paths):
        segments = random.randint(1, 3)
        prev = (random.random(), random.random())
        walk = [prev]
        for _ in range(segments):
            for _ in range(3):
                prev = (prev[0] + 0.1 * (random.random() - 0.5), prev[1] + 0.1 * (random.random() - 0.5))
                walk.append(prev)
        paths.append(_to_pixels(walk, width, height))
        colors.append(torch.tensor([random.random(), random.random(), random.random(), random.random()]))
    return paths, torch.stack(colors)


def _to_pixels(walk, width, height):
    p = torch.tensor(walk)
    p[:, 0] *= width
    p[:, 1] *= height
    return p


class _StrokeDrawer(DrawingInterface):
    """what both stroke drawers share: the leaves, the raster call, the seed staging, to_image / to_svg and the no-op z API"""

    def __init__(self, settings):
        self.canvas_width, self.canvas_height = settings.size[0], settings.size[1]
        self.num_paths = settings.strokes
        self.device = torch.device("cpu")
        self.points = self.widths = self.colors = self.paper = None
        self.path_start = None
        self.scene = None
        self.img = None
        self.opts = None
        self._seed = None                # eager: the seed word, filled per synth
        self._ring = None                # replayed sessions: PinnedRing in front of the seed word
        self._staged_it = None

    def _paths(self, settings, min_width, max_width):
        """-> (list of [1 + 3 S, 2] point tensors, width, colours [n, 4], paper [4] or None)"""
        raise NotImplementedError

    def load_model(self, settings, device):
        from . import ops
        self.device = torch.device(device)
        if int(self.num_paths) < 1:
            raise ValueError(f"{type(self).__name__}: --strokes must be at least 1, got {self.num_paths}")
        self.max_width = settings.max_stroke_width * self.canvas_height / 100
        self.min_width = settings.min_stroke_width * self.canvas_height / 100
        paths, width, colors, paper = self._paths(settings, self.min_width, self.max_width)
        counts = [len(p) for p in paths]
        self.path_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.scene = ops.StrokeRasterScene(self.path_start, self.canvas_width, self.canvas_height, self.device)
        self.points = torch.cat(paths).to(self.device).contiguous().requires_grad_(True)
        self.widths = torch.full((len(paths),), width, dtype=torch.float32).to(self.device).requires_grad_(True)
        self.colors = colors.to(self.device).contiguous()
        self.paper = paper.to(self.device) if paper is not None else None
        self._set_trainable()
        with torch.no_grad():
            self.synth(0)

    def _set_trainable(self):
        raise NotImplementedError

    @property
    def params(self):
        """the optimised leaves, in get_opts order"""
        raise NotImplementedError

    def segment_counts(self):
        return (np.diff(self.path_start) - 1) // 3

    # ------------------------------------------------------------------ the reference's no-op z API
    def rand_init(self, toksX=None, toksY=None):
        pass

    def init_from_tensor(self, init_tensor):
        pass

    def reapply_from_tensor(self, new_tensor):
        pass

    def get_z_from_tensor(self, ref_tensor):
        return None

    def get_num_resolutions(self):
        return None

    def get_z(self):
        return None

    def get_z_copy(self):
        return None

    def set_z(self, new_z):
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
        if self._seed is None or self._seed.device != self.points.device:
            self._seed = torch.zeros(1, dtype=torch.int32, device=self.points.device)
        self._seed.fill_(int(it))
        return self._seed

    # ------------------------------------------------------------------ rendering
    def raster(self, cur_iteration):
        """the RGBA raster [H, W, 4] of the current strokes, jittered by `cur_iteration`"""
        from . import ops
        return ops.stroke_raster(self.points, self.widths, self.colors, self.paper, self.scene, self._seed_word(int(cur_iteration)))

    def synth(self, cur_iteration):
        """[1, 3, H, W]: the raster composited over white (< 0: the last image)"""
        if cur_iteration is not None and cur_iteration < 0:
            return self.img
        img = self.raster(0 if cur_iteration is None else cur_iteration)
        img = img[:, :, 3:4] * img[:, :, :3] + torch.ones(img.shape[0], img.shape[1], 3, device=img.device) * (1 - img[:, :, 3:4])
        self.img = img.unsqueeze(0).permute(0, 3, 1, 2)
        return self.img

    @torch.no_grad()
    def to_image(self):
        from PIL import Image
        img = np.transpose(self.img.detach().cpu().numpy()[0], (1, 2, 0))
        return Image.fromarray(np.uint8(np.clip(img, 0, 1) * 254), mode="RGB")

    @torch.no_grad()
    def to_svg(self, path="lineout.svg"):
        """the scene as SVG: the paper as a full-canvas rect, then every path as cubic segments with stroke-width = 2 * width"""
        w, h = self.canvas_width, self.canvas_height

        def rgb(c):
            r, g, b = (int(round(float(np.clip(v, 0, 1)) * 255)) for v in c[:3])
            return f"rgb({r}, {g}, {b})"
        lines = ['<?xml version="1.0" encoding="UTF-8"?>',
                 f'<svg xmlns="http://www.w3.org/2000/svg" version="1.1" width="{w}" height="{h}" viewBox="0 0 {w} {h}">']
        if self.paper is not None:
            p = self.paper.detach().cpu().numpy()
            lines.append(f'<rect x="0" y="0" width="{w}" height="{h}" fill={quoteattr(rgb(p))} fill-opacity="{float(p[3]):.9g}"/>')
        pts = self.points.detach().cpu().numpy().astype(np.float64)
        widths = self.widths.detach().cpu().numpy().astype(np.float64)
        colors = self.colors.detach().cpu().numpy()
        for k in range(len(widths)):
            q = pts[self.path_start[k]:self.path_start[k + 1]]
            d = [f"M {q[0, 0]:.9g} {q[0, 1]:.9g}"]
            for s in range(1, len(q), 3):
                d.append("C " + " ".join(f"{x:.9g} {y:.9g}" for x, y in q[s:s + 3]))
            lines.append(f'<path d={quoteattr(" ".join(d))} fill="none" stroke={quoteattr(rgb(colors[k]))} '
                         f'stroke-opacity="{float(colors[k][3]):.9g}" stroke-width="{2 * widths[k]:.9g}" '
                         f'stroke-linecap="round" stroke-linejoin="round"/>')
        lines.append("</svg>")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        return path


class LineDrawer(_StrokeDrawer):
    """`--drawer line_sketch`: `strokes` black random-walk paths of `stroke_length` segments on a paper-coloured canvas"""

    @staticmethod
    def add_settings(parser):
        parser.add_argument("--strokes", type=int, help="number strokes", default=24, dest='strokes')
        parser.add_argument("--stroke_length", type=int, help="stroke length", default=8, dest='stroke_length')
        parser.add_argument("--min_stroke_width", type=float, help="min width (percent of height)", default=0.5, dest='min_stroke_width')
        parser.add_argument("--max_stroke_width", type=float, help="max width (percent of height)", default=2, dest='max_stroke_width')
        parser.add_argument("--allow_paper_color", type=_str2bool, help="allow paper color to change", default=False,
                            dest='allow_paper_color')
        return parser

    def __init__(self, settings):
        super().__init__(settings)
        self.stroke_length = settings.stroke_length
        self.allow_paper_color = bool(getattr(settings, "allow_paper_color", False))

    def _paths(self, settings, min_width, max_width):
        if not 1 <= int(self.stroke_length) <= MAX_SEGMENTS:
            raise ValueError(f"line_sketch: --stroke_length must be in 1 .. {MAX_SEGMENTS}, got {self.stroke_length}")
        paths = line_sketch_paths(self.num_paths, int(self.stroke_length), self.canvas_width, self.canvas_height)
        colors = torch.tensor([0.0, 0.0, 0.0, 1.0]).repeat(len(paths), 1)
        return paths, torch.tensor(max_width / 10).item(), colors, torch.tensor(PAPER_COLOR)

    def _set_trainable(self):
        if self.allow_paper_color:
            self.paper.requires_grad_(True)

    @property
    def params(self):
        return [self.points, self.widths] + ([self.paper] if self.allow_paper_color else [])

    def get_opts(self, decay_divisor=1):
        self.opts = [torch.optim.Adam([self.points], lr=1.0 / decay_divisor), torch.optim.Adam([self.widths], lr=0.1 / decay_divisor)]
        if self.allow_paper_color:
            self.opts.append(torch.optim.Adam([self.paper], lr=0.01 / decay_divisor))
        return self.opts

    def clip_z(self):
        with torch.no_grad():
            self.widths.clamp_(1.0, self.max_width)
            self.colors.clamp_(0.0, 1.0)


class ClipDrawer(_StrokeDrawer):
    """`--drawer clipdraw`: `strokes` short random paths of 1 to 3 segments with random, optimised RGBA colours on white"""

    @staticmethod
    def add_settings(parser):
        parser.add_argument("--strokes", type=int, help="number strokes", default=1024, dest='strokes')
        parser.add_argument("--min_stroke_width", type=float, help="min width (percent of height)", default=1, dest='min_stroke_width')
        parser.add_argument("--max_stroke_width", type=float, help="max width (percent of height)", default=5, dest='max_stroke_width')
        return parser

    def _paths(self, settings, min_width, max_width):
        paths, colors = clipdraw_paths(self.num_paths, self.canvas_width, self.canvas_height)
        return paths, torch.tensor((min_width + max_width) / 4).item(), colors, None

    def _set_trainable(self):
        self.colors.requires_grad_(True)

    @property
    def params(self):
        return [self.points, self.widths, self.colors]

    def get_opts(self, decay_divisor=1):
        self.opts = [torch.optim.Adam([self.points], lr=1.0 / decay_divisor), torch.optim.Adam([self.widths], lr=0.1 / decay_divisor),
                     torch.optim.Adam([self.colors], lr=0.01 / decay_divisor)]
        return self.opts

    def clip_z(self):
        with torch.no_grad():
            self.widths.clamp_(self.min_width, self.max_width)
            self.colors.clamp_(0.0, 1.0)
