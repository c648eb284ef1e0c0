"""Registration of drawer / filter / custom-loss plugins, as the reference's module tables and `do_init` do it
(pixray.py:54-58, 72-99, 131-140, 612-626, 650-669, 961-995, 2104-2109).

`--custom_loss "style:0.5,saturation->arg1->arg2"` is a comma-separated list of `name[:weight[:stop]]` chunks, optionally
followed by `->`-separated instance arguments.  Each name is looked up in `loss_class_table`, instantiated with
`device=`, given its instance arguments, then every instance parses the settings (`parse_settings(args) -> args`) and
contributes its globals (`add_globals(args) -> dict`).  The result is the list of {"loss", "weight"} dicts `Session` takes
as `custom_losses=` and the `lossGlobals` dict handed to every `get_loss` call.

`class_table` maps `--drawer` names to drawer classes (the HIP VQGAN drawer, the fft spectrum drawer, the polygon grid of the
reference's `pixel` drawer on the HIP rasteriser, the nearest-upsampled pixel grid that stands in for its `fast_pixel`, and its
`line_sketch` and `clipdraw` stroke drawers on the HIP stroke rasteriser, and its `super_resolution` drawer on the HIP RRDBNet
x4 runner); `filters_class_table` holds the reference's three
filters (`lookup`, `tiler`, `wallpaper`: builtin_filters.py) and `loss_class_table` its losses (`style`: style_loss.py;
`palette`, `saturation`, `symmetry`, `smoothness`, `edge` -- with `--edge_input_image` / `--edge_mask_image` -- and `aesthetic`,
whose linear head is read from the file `--aesthetic_model` names: builtin_losses.py), all on HIP kernels.  `resmem` is
registered so that asking for it says why it is unavailable (its network is not shipped and cannot be loaded here).
`builtin_losses.GaussianLoss` has no registry name, as in the reference: `add_custom_loss("gaussian", GaussianLoss)`.
Further plugins register through `add_custom_filter` / `add_custom_loss`; the reference's own plain-torch plugin files drop
in unchanged that way (see tests/test_host_logic.py::test_unmodified_reference_plugins_drop_in)."""
from typing import Dict, List, Tuple

from .builtin_filters import BUILTIN_FILTERS
from .builtin_losses import BUILTIN_LOSSES, UNAVAILABLE_LOSSES
from .fft_drawer import FftDrawer
from .interfaces import DrawingInterface, FilterInterface, LossInterface
from .pixel_drawer import PixelDrawer
from .pixel_grid_drawer import PixelGridDrawer
from .prompt import parse_prompt
from .stroke_drawer import ClipDrawer, LineDrawer
from .style_loss import StyleLoss
from .super_resolution_drawer import SuperResolutionDrawer
from .vqgan_drawer import VqganDrawer

class_table: Dict[str, type] = {"vqgan": VqganDrawer, "pixel": PixelDrawer, "fft": FftDrawer, "fast_pixel": PixelGridDrawer,
                               "line_sketch": LineDrawer, "clipdraw": ClipDrawer, "super_resolution": SuperResolutionDrawer}
filters_class_table: Dict[str, type] = dict(BUILTIN_FILTERS)
loss_class_table: Dict[str, type] = {**BUILTIN_LOSSES, "style": StyleLoss, **UNAVAILABLE_LOSSES}


def add_custom_drawer(name: str, customdrawer: type) -> None:
    assert issubclass(customdrawer, DrawingInterface)
    class_table.update({name: customdrawer})


def add_custom_filter(name: str, customfilter: type) -> None:
    assert issubclass(customfilter, FilterInterface)
    filters_class_table.update({name: customfilter})


def make_drawer(args, device):
    """pixray.py:612-626 -> (drawer, (sideX, sideY)): the class named by `args.drawer` (KeyError when unknown), its model
    loaded, and the canvas size rounded down to a multiple of 2^(num_resolutions-1) when the drawer has resolutions"""
    drawer = class_table[args.drawer](args)
    drawer.load_model(args, device)
    num_resolutions = drawer.get_num_resolutions() if hasattr(drawer, "get_num_resolutions") else None
    if num_resolutions is not None:
        f = 2 ** (num_resolutions - 1)
        side = ((args.size[0] // f) * f, (args.size[1] // f) * f)
    else:
        side = (args.size[0], args.size[1])
    return drawer, side


def setup_filters(spec, args, device=None) -> List[dict]:
    """pixray.py:650-669: `--filters "name[:weight],..."` -> [{"filter", "weight"}]; an unknown name is a ValueError"""
    out: List[dict] = []
    if spec:
        for filt in [f.strip() for f in spec.split(",")]:
            filt_name, weight, _stop = parse_prompt(filt)
            if filt_name not in filters_class_table:
                raise ValueError(f"Requested filter not found, aborting: {filt_name}")
            cls = filters_class_table[filt_name]
            try:
                out.append({"filter": cls(args, device=device), "weight": weight})
            except TypeError as e:
                print(f"error in initializing {cls} - this message is to provide information")
                raise TypeError(e)
    return out


def add_custom_loss(name: str, customloss: type, needs_full_batch: bool = None) -> None:
    """pixray.py:2104-2109.  `needs_full_batch`: declare the class batch-coupled (engine.needs_full_batch) -- a loss written
    for this package sets the class attribute itself; the reference's own batch-coupled plugins (SaturationLoss,
    AestheticLoss, ResmemLoss) cannot, so they are marked HERE, at registration, by their reference class name."""
    assert issubclass(customloss, LossInterface)
    from .engine import REFERENCE_FULL_BATCH_LOSSES, mark_full_batch
    if needs_full_batch or (needs_full_batch is None and "needs_full_batch" not in vars(customloss)
                            and customloss.__name__ in REFERENCE_FULL_BATCH_LOSSES):
        mark_full_batch(customloss)
    loss_class_table.update({name: customloss})


def setup_custom_losses(spec, args, device=None) -> Tuple[List[dict], dict, object]:
    """pixray.py:961-995 -> (custom_losses, lossGlobals, args).  `spec` is the --custom_loss string (or None); an unknown
    name is a KeyError, a constructor that does not take `device=` re-raises its TypeError after the reference's hint."""
    losses: List[dict] = []
    loss_globals: dict = {}
    if spec:
        for chunk in [c.strip() for c in spec.split(",")]:
            if chunk.find("->") > 0:
                parts = chunk.split("->")
                name_part, instance_args = parts[0], parts[1:]
            else:
                name_part, instance_args = chunk, []
            loss_name, weight, _stop = parse_prompt(name_part)
            if loss_name not in loss_class_table:
                raise KeyError(f"Requested custom loss not found, aborting: {loss_name} (known: {', '.join(sorted(loss_class_table))})")
            cls = loss_class_table[loss_name]
            try:
                inst = cls(device=device)
                inst.instance_settings(instance_args)
                losses.append({"loss": inst, "weight": weight})
            except TypeError as e:
                print(f"error in initializing {cls} - this message is to provide information")
                raise TypeError(e)
    for t in losses:
        args = t["loss"].parse_settings(args)
    for t in losses:
        loss_globals.update(t["loss"].add_globals(args))
    return losses, loss_globals, args
