"""pixray's built-in custom losses (Losses/*.py) on the HIP kernels of csrc/plugin_losses.hip.

Same registry names, options, defaults and `dest`s as the reference; `get_loss` returns what the reference's does (a list with
one term per cutout size for the cutout-batch losses, one scalar for the image losses).  None of them draws, uploads or branches
on the host inside `get_loss` once its constant tables are on the device (the first call puts them there), so every one declares
`supports_graph_replay`.

`aesthetic` scores the cutout embeddings with a linear head read from a file the user supplies (`--aesthetic_model`; the weights
are neither shipped nor fetched).  `GaussianLoss` is exported but, as in pixray, carries no registry name: register it with
`frontend.add_custom_loss("gaussian", GaussianLoss)`.  No option fetches anything: a value containing `http` is an error.

Not provided: `resmem` (its network is not part of this package and cannot be loaded here)."""
import glob
import os

import torch
import torch.nn.functional as F

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


def _first_file(pattern, option, what):
    """`glob`, first match (style_loss.StyleLoss.parse_settings); nothing is fetched"""
    if "http" in pattern:
        raise ValueError(f"{what}: --{option} {pattern!r}: remote files are not fetched; download the file and pass its path")
    files = sorted(glob.glob(pattern))
    if not files:
        raise ValueError(f"{what}: --{option}: no file matches {pattern!r}")
    return files[0]


def _load_unit_image(path, mode):
    """an image file as an fp32 CPU tensor in [0, 1]: [1, 3, H, W] for "RGB", [1, 1, H, W] for "L" (TF.to_tensor's scaling)"""
    import numpy as np
    from PIL import Image
    a = np.asarray(Image.open(path).convert(mode), dtype=np.float32) / 255.0
    t = torch.from_numpy(a)
    return (t.permute(2, 0, 1) if t.dim() == 3 else t.unsqueeze(0)).unsqueeze(0).contiguous()


class EdgeLoss(LossInterface):
    """MSE against a target in the four margin bands (percent of the image, `--edge_thickness` or `--edge_margins`
    left right up down), plus `--global_color_weight` times the MSE over the whole image, all times `--edge_color_weight`.
    The target is `--edge_color`, or the picture `--edge_input_image` resized to the canvas.  With `--edge_mask_image` the bands
    are skipped: everything where the resized mask is <= 0 is pulled to the target (mean over all elements).
    Reads the (replicated) image.

    [UPSTREAM] pixray resizes with torchvision's tensor `resize(..., BICUBIC)` of its pinned version (no antialias, unclamped);
    torchvision is absent here, so `F.interpolate(mode="bicubic", align_corners=False)` stands in, as in style_loss.py.  The
    resize runs on the CPU in fp32 and the result is uploaded: the mask is thresholded at > 0, and a device bicubic that
    differs in the last bit would flip pixels."""
    supports_graph_replay = True

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.image = None          # [1, 3, h0, w0] fp32 CPU, [0, 1]
        self.mask = None           # [1, 1, h0, w0] fp32 CPU, [0, 1]
        self._resized = None       # ((h, w, device), target [1, 3, h, w] | None, mask [1, 1, h, w] | None) on the device

    @staticmethod
    def add_settings(parser):
        parser.add_argument("--edge_thickness", type=int, help="thickness of the edge area all the way around (percent)", default=5, dest='edge_thickness')
        parser.add_argument("--edge_margins", nargs=4, type=int, help="this is for the thickness of each edge (left, right, up, down) 0-pixel size", default=None, dest='edge_margins')
        parser.add_argument("--edge_color", type=str, help="this is the color of the specified region", default="white", dest='edge_color')
        parser.add_argument("--edge_color_weight", type=float, help="how much edge color is enforced", default=0.1, dest='edge_color_weight')
        parser.add_argument("--global_color_weight", type=float, help="how much global color is enforced ", default=0.05, dest='global_color_weight')
        parser.add_argument("--edge_input_image", type=str, help="picture (path or glob, first match) the region is pulled towards instead of --edge_color", default="", dest='edge_input_image')
        parser.add_argument("--edge_mask_image", type=str, help="mask (path or glob, first match): replaces the margin bands by everything where the mask is black", default="", dest='edge_mask_image')
        return parser

    def parse_settings(self, args):
        if isinstance(args.edge_color, str):
            args.edge_color = get_single_rgb(args.edge_color)
        if args.edge_margins is None:
            t = args.edge_thickness
            args.edge_margins = (t, t, t, t)
        self.image = self.mask = self._resized = None
        if getattr(args, "edge_input_image", ""):
            self.image = _load_unit_image(_first_file(args.edge_input_image, "edge_input_image", "EdgeLoss"), "RGB")
        if getattr(args, "edge_mask_image", ""):
            self.mask = _load_unit_image(_first_file(args.edge_mask_image, "edge_mask_image", "EdgeLoss"), "L")
        return args

    def _on_canvas(self, out):
        key = (int(out.shape[2]), int(out.shape[3]), str(out.device))
        if self._resized is None or self._resized[0] != key:
            # [UPSTREAM] stands in for torchvision's tensor resize (see the class docstring); on the CPU, then uploaded
            fit = [None if t is None else F.interpolate(t, key[:2], mode="bicubic", align_corners=False).to(out.device).contiguous()
                   for t in (self.image, self.mask)]
            self._resized = (key, fit[0], fit[1])
        return self._resized[1], self._resized[2]

    def get_loss(self, cur_cutouts, out, args, globals=None, lossGlobals=None):
        h, w = out.shape[2], out.shape[3]
        left, right, upper, lower = args.edge_margins
        px = (int(map_number(left, 0, 100, 0, w)), int(map_number(right, 0, 100, 0, w)),
              int(map_number(upper, 0, 100, 0, h)), int(map_number(lower, 0, 100, 0, h)))
        if self.image is None and self.mask is None:
            return ops.edge_loss(out, args.edge_color, px, args.edge_color_weight, args.global_color_weight)
        target, mask = self._on_canvas(out)
        return ops.edge_target_loss(out, target, args.edge_color, mask, px, args.edge_color_weight, args.global_color_weight)


class GaussianLoss(LossInterface):
    """pixray's Losses/GaussianLoss.py: mean(|out - `--gaussian_color`/255| * |1 - g|) * `--gaussian_weight`, g the outer product of
    two 1-D gaussians centred on the canvas: pulls everything away from the centre towards the colour.  `--gaussian_std` is
    (row std, column std), the order the reference passes to its `gkern(h, w, *std)`.  Reads the (replicated) image.

    pixray ships the class without a registry name; so does this package: `frontend.add_custom_loss("gaussian", GaussianLoss)`."""
    supports_graph_replay = True

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self._tables = None

    @staticmethod
    def add_settings(parser):
        parser.add_argument("--gaussian_weight", type=float, help="gaussian's weight", default=1, dest='gaussian_weight')
        parser.add_argument("--gaussian_std", nargs=2, type=float, help="gaussian's std (rows, columns)", default=(40, 40), dest='gaussian_std')
        parser.add_argument("--gaussian_color", nargs=3, type=float, help="color for gaussian to optimize to", default=(255, 255, 255), dest='gaussian_color')
        return parser

    @staticmethod
    def table(M, std):
        """GaussianLoss.py's gaussian_fn, on the host in fp32"""
        n = torch.arange(0, M) - (M - 1.0) / 2.0
        return torch.exp(-n ** 2 / (2 * std * std))

    def _gauss(self, out, std):
        key = (int(out.shape[2]), int(out.shape[3]), float(std[0]), float(std[1]), str(out.device))
        if self._tables is None or self._tables[0] != key:
            self._tables = (key, self.table(key[0], std[0]).to(out.device).contiguous(), self.table(key[1], std[1]).to(out.device).contiguous())
        return self._tables[1], self._tables[2]

    def get_loss(self, cur_cutouts, out, args, globals=None, lossGlobals=None):
        gy, gx = self._gauss(out, args.gaussian_std)
        return ops.gaussian_loss(out, gy, gx, [v / 255 for v in args.gaussian_color], args.gaussian_weight)


class AestheticLoss(LossInterface):
    """pixray's Losses/AestheticLoss.py: a linear head on the L2-normalised cutout embeddings of the LAST perceptor
    (`globals["embeds"]`) predicts a 0-10 rating; the loss is 0.02 * mean((rating - `--aesthetic_target`)^2).

    The head is read from `--aesthetic_model` (default `models/ava_vit_b_16_linear.pth`, where pixray keeps it, relative to the
    working directory): a `torch.load` dict with `weight` [1, d] and `bias` [1].  The file is neither shipped nor fetched.
    The mean runs over all cutouts, so a shard's value is not a share of it: scored on the full batch under cutout sharding."""
    needs_full_batch = True
    supports_graph_replay = True
    DEFAULT_MODEL = "models/ava_vit_b_16_linear.pth"

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.weight = self.bias = None
        self._dev = None

    @staticmethod
    def add_settings(parser):
        parser.add_argument("--aesthetic_target", type=float, help="0-10", default=10, dest='aesthetic_target')
        parser.add_argument("--aesthetic_model", type=str, help="file with the linear head's weight [1, d] and bias [1]", default=AestheticLoss.DEFAULT_MODEL, dest='aesthetic_model')
        return parser

    def parse_settings(self, args):
        path = getattr(args, "aesthetic_model", None) or self.DEFAULT_MODEL
        if "http" in path:
            raise ValueError(f"AestheticLoss: --aesthetic_model {path!r}: remote files are not fetched; download the file and pass its path")
        if not os.path.isfile(path):
            raise RuntimeError(f"the aesthetic loss needs the aesthetic-predictor head, looked for at {os.path.abspath(path)!r} "
                               "(--aesthetic_model): the weights are neither shipped with this package nor fetched")
        sd = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(sd, dict) or "weight" not in sd or "bias" not in sd or sd["weight"].dim() != 2 or sd["weight"].shape[0] != 1 \
                or sd["bias"].numel() != 1:
            raise ValueError(f"AestheticLoss: --aesthetic_model {path!r}: expected a dict with weight [1, d] and bias [1]")
        self.weight = sd["weight"].detach().to(torch.float32).reshape(-1).contiguous()
        self.bias = float(sd["bias"].detach().to(torch.float32).reshape(-1)[0])
        self._dev = None
        return args

    def get_loss(self, cur_cutouts, out, args, globals=None, lossGlobals=None):
        embeds = (globals or {}).get("embeds")
        if embeds is None:
            raise ValueError("AestheticLoss: no cutout embeddings (globals[\"embeds\"]): the aesthetic loss needs a perceptor")
        if self.weight is None:
            raise ValueError("AestheticLoss: parse_settings has not loaded --aesthetic_model")
        embeds = embeds.reshape(-1, embeds.shape[-1])
        if embeds.shape[1] != self.weight.numel():
            raise ValueError(f"AestheticLoss: the embeddings are {embeds.shape[1]} wide but the --aesthetic_model head is "
                             f"{self.weight.numel()} wide; pixray's head fits the 512-wide ViT-B towers")
        if self._dev is None or self._dev.device != embeds.device:
            self._dev = self.weight.to(embeds.device)
        return ops.aesthetic_loss(embeds.float(), self._dev, self.bias, getattr(args, "aesthetic_target", 10))


class _Unavailable(LossInterface):
    reason = ""

    def __init__(self, **kwargs):
        raise RuntimeError(self.reason)


class ResmemLoss(_Unavailable):
    reason = "the resmem loss needs the ResMem model weights, which are not part of this package"


BUILTIN_LOSSES = {"palette": PaletteLoss, "saturation": SaturationLoss, "symmetry": SymmetryLoss, "smoothness": SmoothnessLoss,
                  "edge": EdgeLoss, "aesthetic": AestheticLoss}
UNAVAILABLE_LOSSES = {"resmem": ResmemLoss}
