"""pixray's built-in custom losses (Losses/*.py) on the HIP kernels of csrc/plugin_losses.hip.

Same registry names, options, defaults and `dest`s as the reference; `get_loss` returns what the reference's does (a list with
one term per cutout size for the cutout-batch losses, one scalar for the image losses).  None of them draws, uploads or branches
on the host inside `get_loss` once its constant tables are on the device (the first call puts them there), so every one declares
`supports_graph_replay`.

Not provided: `resmem` and `aesthetic` (their model weights are not part of this package), EdgeLoss's `--edge_input_image` /
`--edge_mask_image`, and the unregistered `GaussianLoss`."""
import torch

from . import ops
from .interfaces import LossInterface
from .palette import get_single_rgb, map_number


class SaturationLoss(LossInterface):
    """Hasler-Suesstrunk colourfulness of each cutout batch: -(std_rggb + 0.3 mean_rggb) * w / 10.  The statistics run over the
    whole batch, so a shard's value is not a share of it: scored on the full batch under cutout sharding."""
    needs_full_batch = True
    supports_graph_replay = True

    @staticmethod
    def add_settings(parser):
        parser.add_argument("--saturation_weight", type=float, help="strength of pallete loss effect", default=1, dest='saturation_weight')
        return parser

    def get_loss(self, cur_cutouts, out, args, globals=None, lossGlobals=None):
        return [ops.saturation_loss(c, args.saturation_weight) for c in cur_cutouts.values()]


class SymmetryLoss(LossInterface):
    """MSE(out, flip_W(out)) * w.  Reads the (replicated) image, not the cutouts."""
    supports_graph_replay = True

    @staticmethod
    def add_settings(parser):
        parser.add_argument("--symmetry_weight", type=float, help="how much symmetry is weighted in loss", default=1, dest='symmetry_weight')
        return parser

    def get_loss(self, cur_cutouts, out, args, globals=None, lossGlobals=None):
        return ops.symmetry_loss(out, args.symmetry_weight)


class SmoothnessLoss(LossInterface):
    """Mean gradient magnitude of each cutout batch (torch.gradient over the [n*S, S, 3] view), default / clipped / log, with an
    optional valid-padding Gaussian pre-blur.

    Batch-coupled, so `needs_full_batch = True`: the view stacks the cutouts' rows, and the row-direction stencil reads across
    the boundary between cutout i's last row and cutout i+1's first.  Scoring two shards separately would drop the pair of
    rows that meet at the shard boundary (each shard's end rows take one-sided differences instead) and would change the rows
    at that seam, so the two halves' sum does not equal the world-1 value.  Scored on the full gathered batch, every rank
    computes exactly the world-1 loss, and the weight is not divided.

    One intended divergence: where the magnitude is exactly 0 (a flat neighbourhood) the backward uses the zero subgradient;
    the reference's sqrt has an infinite derivative there and gives NaN."""
    needs_full_batch = True
    supports_graph_replay = True

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self._taps = None

    @staticmethod
    def add_settings(parser):
        parser.add_argument("--smoothness_weight", type=float, help="strength of smoothness loss effect", default=1, dest='smoothness_weight')
        parser.add_argument("--smoothness_type", type=str, help="enforce smoothness type: default/clipped/log", default='default', dest='smoothness_type')
        parser.add_argument("--smoothness_gaussian_kernel", type=float, help="enforce smoothness aux gaussian blur kernel", default=0, dest='smoothness_gaussian_kernel')
        parser.add_argument("--smoothness_gaussian_std", type=float, help="enforce smoothness aux gaussian blur std", default=1, dest='smoothness_gaussian_std')
        parser.add_argument("--smoothness_spacing", type=int, help="enforce smoothness spacing", default=1, dest='smoothness_spacing')
        parser.add_argument("--smoothness_edge_order", type=int, help="enforce smoothness edge order", default=1, dest='smoothness_edge_order')
        return parser

    def _blur_taps(self, args, device):
        if not args.smoothness_gaussian_kernel:
            return None
        key = (args.smoothness_gaussian_kernel, args.smoothness_gaussian_std, str(device))
        if self._taps is None or self._taps[0] != key:
            taps = ops.gaussian_taps(args.smoothness_gaussian_kernel, args.smoothness_gaussian_std)
            self._taps = (key, taps.to(device).contiguous())
        return self._taps[1]

    def get_loss(self, cur_cutouts, out, args, globals=None, lossGlobals=None):
        losses = []
        for c in cur_cutouts.values():
            losses.append(ops.smoothness_loss(c, args.smoothness_weight, args.smoothness_type, args.smoothness_spacing,
                                              args.smoothness_edge_order, self._blur_taps(args, c.device)))
        return losses


class PaletteLoss(LossInterface):
    """Mean distance of each cutout pixel to its nearest `--palette` colour, times the batch size n and w / 10.  The factor n
    makes a shard's value a different fraction of the whole than its share of the pixels: scored on the full batch."""
    needs_full_batch = True
    supports_graph_replay = True

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self._pal = None

    @staticmethod
    def add_settings(parser):
        parser.add_argument("--palette_weight", type=float, help="strength of pallete loss effect", default=1, dest='palette_weight')
        return parser

    def parse_settings(self, args):
        if getattr(args, "palette", None) is None:
            raise ValueError("the palette loss needs a --palette (e.g. --palette \"red->yellow\")")
        return args

    def _palette(self, args, device):
        key = (id(args.palette), str(device))
        if self._pal is None or self._pal[0] != key:
            self._pal = (key, ops._palette_dev(args.palette, device))
        return self._pal[1]

    def get_loss(self, cur_cutouts, out, args, globals=None, lossGlobals=None):
        return [ops.palette_loss(c, self._palette(args, c.device), args.palette_weight) for c in cur_cutouts.values()]


class EdgeLoss(LossInterface):
    """MSE against `--edge_color` in the four margin bands (percent of the image, `--edge_thickness` or `--edge_margins`
    left right up down), plus `--global_color_weight` times the MSE over the whole image, all times `--edge_color_weight`.
    Reads the (replicated) image."""
    supports_graph_replay = True

    @staticmethod
    def add_settings(parser):
        parser.add_argument("--edge_thickness", type=int, help="thickness of the edge area all the way around (percent)", default=5, dest='edge_thickness')
        parser.add_argument("--edge_margins", nargs=4, type=int, help="this is for the thickness of each edge (left, right, up, down) 0-pixel size", default=None, dest='edge_margins')
        parser.add_argument("--edge_color", type=str, help="this is the color of the specified region", default="white", dest='edge_color')
        parser.add_argument("--edge_color_weight", type=float, help="how much edge color is enforced", default=0.1, dest='edge_color_weight')
        parser.add_argument("--global_color_weight", type=float, help="how much global color is enforced ", default=0.05, dest='global_color_weight')
        parser.add_argument("--edge_input_image", type=str, help="not supported", default="", dest='edge_input_image')
        parser.add_argument("--edge_mask_image", type=str, help="not supported", default="", dest='edge_mask_image')
        return parser

    def parse_settings(self, args):
        if getattr(args, "edge_input_image", "") or getattr(args, "edge_mask_image", ""):
            raise ValueError("EdgeLoss: --edge_input_image / --edge_mask_image are not supported; use --edge_color")
        if isinstance(args.edge_color, str):
            args.edge_color = get_single_rgb(args.edge_color)
        if args.edge_margins is None:
            t = args.edge_thickness
            args.edge_margins = (t, t, t, t)
        return args

    def get_loss(self, cur_cutouts, out, args, globals=None, lossGlobals=None):
        h, w = out.shape[2], out.shape[3]
        left, right, upper, lower = args.edge_margins
        px = (int(map_number(left, 0, 100, 0, w)), int(map_number(right, 0, 100, 0, w)),
              int(map_number(upper, 0, 100, 0, h)), int(map_number(lower, 0, 100, 0, h)))
        return ops.edge_loss(out, args.edge_color, px, args.edge_color_weight, args.global_color_weight)


class _Unavailable(LossInterface):
    reason = ""

    def __init__(self, **kwargs):
        raise RuntimeError(self.reason)


class ResmemLoss(_Unavailable):
    reason = "the resmem loss needs the ResMem model weights, which are not part of this package"


class AestheticLoss(_Unavailable):
    reason = "the aesthetic loss needs the aesthetic-predictor weights, which are not part of this package"


BUILTIN_LOSSES = {"palette": PaletteLoss, "saturation": SaturationLoss, "symmetry": SymmetryLoss, "smoothness": SmoothnessLoss,
                  "edge": EdgeLoss}
UNAVAILABLE_LOSSES = {"resmem": ResmemLoss, "aesthetic": AestheticLoss}
