"""pixray's built-in image filters (filters/*.py) on the HIP kernels of csrc/plugin_filters.hip.

`tiler` and `wallpaper` draw `rand_w`, then `rand_h`, from torch's global generator, as the reference does.  Run eagerly they
draw inside `forward`.  In a replayed session (engine.Session.enable_graph) `Session._host_prep` calls `host_prep`, which makes
the same two draws before the device work and stages them through a ring of pinned buffers into the fixed 2-word device buffer
the kernels read; `forward` then launches on that buffer without touching the host."""
import torch

from . import ops
from .interfaces import FilterInterface


class ColorLookup(FilterInterface):
    """Nearest `--palette` colour per pixel with a straight-through gradient, returning the commitment loss
    `lookup_beta * mean((q - z)^2) + mean((q - z)^2)` (only its first term has a gradient).  An RGBA input keeps its alpha."""
    supports_graph_replay = True

    @staticmethod
    def add_settings(parser):
        parser.add_argument("--lookup_beta", type=float, help="loss scaling", default=10.0, dest='lookup_beta')
        return parser

    def __init__(self, settings, device=None):
        super().__init__(settings, device)
        self.beta = settings.lookup_beta
        palette = getattr(settings, "palette", None)
        if palette is None:
            raise ValueError("the lookup filter needs a --palette (e.g. --palette \"black->white\\8\")")
        self.color_table = ops._palette_dev(palette, "cpu")
        self._dev_table = None

    def forward(self, z):
        if self._dev_table is None or self._dev_table.device != z.device:
            self._dev_table = self.color_table.to(z.device).contiguous()
        return ops.color_lookup(z, self._dev_table, self.beta)


class WallpaperFilter(FilterInterface):
    """Random tiled shifts: `--wallpaper_type` none (both axes) / horizontal / vertical / shift (two rows, the second offset by
    half the width), optionally trimming `--wallpaper_edge_match` // 2 pixels off the rolled edges and returning the
    `MSE(first em, last em) / em` seam loss."""
    supports_graph_replay = True
    mode = None

    @staticmethod
    def add_settings(parser):
        parser.add_argument("--wallpaper_type", type=str, help="none, shift, horizontal", default=None, dest='wallpaper_type')
        parser.add_argument("--wallpaper_edge_match", type=int, help="force repeating match in pixels", default=0, dest='wallpaper_edge_match')
        return parser

    def __init__(self, settings, device=None):
        super().__init__(settings, device)
        self.wallpaper_type = getattr(settings, "wallpaper_type", None)
        self.edge_match = getattr(settings, "wallpaper_edge_match", 0)
        if self.wallpaper_type not in ops.WALLPAPER_MODES:
            self.wallpaper_type = None           # the reference's fall-through branch: roll both axes
        self._hw = None                          # the last input's (H, W): host_prep draws against it
        self._ring = None                        # PinnedRing of the {rand_h, rand_w} buffer once static buffers are on
        self._static_device = None
        self._staged = False

    # ------------------------------------------------------------------ graph-replay protocol (engine.Session)
    @property
    def graph_capturable(self):
        return self._static_device is not None

    def enable_static_buffers(self, device):
        from .cutouts import PinnedRing
        self._static_device = torch.device(device)
        self._ring = PinnedRing((2,), torch.int32, self._static_device)

    def host_prep(self, args, cur_iteration):
        if self._static_device is None or self._hw is None:
            return
        self._ring.stage(self._draw(*self._hw))
        self._staged = True

    @staticmethod
    def _draw(H, W):
        rand_w = torch.randint(0, W, (1,))
        rand_h = torch.randint(0, H, (1,))
        return torch.tensor([int(rand_h), int(rand_w)], dtype=torch.int32)

    def forward(self, imgs):
        B, C, H, W = imgs.size()
        self._hw = (H, W)
        if self._staged:
            shifts = self._ring.dev
            self._staged = False
        else:
            shifts = self._draw(H, W).to(imgs.device)
        mode = self.mode if self.mode is not None else self.wallpaper_type
        return ops.wallpaper(imgs, shifts, mode, 0 if self.mode is not None else self.edge_match)


class TilerFilter(WallpaperFilter):
    """Random roll along both axes, no loss."""
    mode = "tiler"

    @staticmethod
    def add_settings(parser):
        return parser


BUILTIN_FILTERS = {"lookup": ColorLookup, "tiler": TilerFilter, "wallpaper": WallpaperFilter}
