"""`SuperResolutionDrawer` with the reference's drawer surface (/root/reference/super_resolution.py:34-102) on the HIP RRDBNet
x4 runner (csrc/rrdbnet.hip).

`z` is an RGB image [1,3,h,w] in [0,1] at a quarter of the canvas; `synth` is `clamp_with_grad(RRDBNet(z), 0, 1)`: with the
arguments the reference's drawer passes (scale 4, tile 0, pre_pad 0, half=False) `RealESRGANer.enhance` neither pads, tiles nor
crops (real_esrganer.py:54-81, 147-169).  The network, the clamp and the whole data gradient run on the HIP kernels; the
image -> z resizes (`get_z_from_tensor`, `init_from_tensor`, `reapply_from_tensor`) are plain `F.interpolate`, off the
iteration's path, as in `PixelGridDrawer`.

Differences from the reference, on purpose:
  * `get_num_resolutions()` returns 3, not None.  The reference renders 4 * (size // 4) whatever the canvas and lets the rest
    of the loop believe the canvas has the requested size; here `plugins.make_drawer` rounds the canvas down to a multiple of
    4 (2 ** (3 - 1)), so the loop and the drawer agree.  Identical for sizes that already are multiples of 4.
  * `init_from_tensor(None)` starts from mid-grey plus small seeded noise (the reference would fail there).
  * Nothing is downloaded (the reference wgets the checkpoint): `models/super_resolution_<name>.ckpt` is used when it exists,
    else `settings.super_resolution_state_dict` when the caller has one, else seeded synthetic weights of the real
    architecture -- and a one-line message says so."""
import os

import torch
import torch.nn.functional as F

from . import ops
from .interfaces import DrawingInterface
from .weights import RRDBNET_CONFIGS, synthetic_rrdbnet_params


class SuperResolutionDrawer(DrawingInterface):
    @staticmethod
    def add_settings(parser):
        parser.add_argument("--super_resolution_model", type=str, help="Super resolution model", default="RealESRGAN_x4plus",
                            dest="super_resolution_model")
        return parser

    def __init__(self, settings):
        super(DrawingInterface, self).__init__()
        self.super_resolution_model = getattr(settings, "super_resolution_model", "RealESRGAN_x4plus")
        self.size = tuple(getattr(settings, "size", (256, 256)))          # (width, height) as in the reference
        self.state_dict = getattr(settings, "super_resolution_state_dict", None)
        self.weight_seed = getattr(settings, "weight_seed", 0)
        self.precision = getattr(settings, "precision", None)
        self.z = None
        self.handle = None
        self._fused_clamp = False

    def load_model(self, settings, device):
        if self.super_resolution_model not in RRDBNET_CONFIGS:
            raise ValueError(f"unknown super resolution model: {self.super_resolution_model} (known: {', '.join(RRDBNET_CONFIGS)})")
        self.cfg = RRDBNET_CONFIGS[self.super_resolution_model]
        self.device = torch.device(device)
        checkpoint_path = f"models/super_resolution_{self.super_resolution_model}.ckpt"
        if self.state_dict is not None:
            params = self.state_dict
        elif os.path.exists(checkpoint_path):
            from .checkpoints import load_rrdbnet
            params = load_rrdbnet(checkpoint_path, self.cfg)
        else:
            print(f"super_resolution: {checkpoint_path} not found (nothing is downloaded): seeded synthetic weights of {self.cfg.name}")
            params = synthetic_rrdbnet_params(self.cfg, self.weight_seed)
        w, h = self.size
        w, h = (w // 4) * 4, (h // 4) * 4
        if w == 0 or h == 0:
            raise ValueError(f"size {self.size} is smaller than one latent pixel (4 x 4)")
        self.size = (w, h)
        self.latent_hw = (h // 4, w // 4)
        self._params = params
        if self.device.type == "cuda":
            self.handle = ops.RrdbNetHandle(self.cfg, params, self.latent_hw, self.device, precision=self.precision)
            # scalar clip_z bounds for the fused optimiser kernels (engine.Session.rebuild_optimisers)
            self._zmin_flat = torch.zeros(3, device=self.device)
            self._zmax_flat = torch.ones(3, device=self.device)

    def get_opts(self, decay_divisor):
        return None

    def get_z_from_tensor(self, ref_tensor):
        size = [ref_tensor.shape[-2] // 4, ref_tensor.shape[-1] // 4]
        return F.interpolate((ref_tensor.to(self.device).float() + 1) / 2, size=size, mode="bilinear", align_corners=False)

    def init_from_tensor(self, init_tensor):
        if init_tensor is None:
            g = torch.Generator().manual_seed(self.weight_seed)
            z = 0.5 + 0.05 * torch.randn(1, 3, *self.latent_hw, generator=g)
            self.z = z.clamp(0, 1).to(self.device).requires_grad_(True)
            return
        z = self.get_z_from_tensor(init_tensor)
        if tuple(z.shape[-2:]) != self.latent_hw:
            z = F.interpolate(z, size=self.latent_hw, mode="bilinear", align_corners=False)
        self.z = z.detach().contiguous().requires_grad_(True)

    def reapply_from_tensor(self, new_tensor):
        new_z = self.get_z_from_tensor(new_tensor)
        if tuple(new_z.shape[-2:]) != self.latent_hw:
            new_z = F.interpolate(new_z, size=self.latent_hw, mode="bilinear", align_corners=False)
        with torch.no_grad():
            self.z.copy_(new_z)

    def get_num_resolutions(self):
        return 3

    def synth(self, cur_iteration):
        if self.handle is None:
            raise ops.PrxError("super_resolution: the RRDBNet runner needs an MI355X (there is no CPU path)")
        return ops.rrdbnet_synth(self.z, self.handle, True)

    @torch.no_grad()
    def to_image(self):
        from PIL import Image
        out = self.synth(None)
        arr = out[0].mul(255).round().clamp(0, 255).byte().permute(1, 2, 0).cpu().numpy()
        return Image.fromarray(arr)

    def clip_z(self):
        if self._fused_clamp:
            return          # the fused optimiser kernel already applied the [0,1] bounds this step
        with torch.no_grad():
            self.z.copy_(self.z.clip(0, 1))

    def get_z(self):
        return self.z

    def set_z(self, new_z):
        with torch.no_grad():
            return self.z.copy_(new_z)

    def get_z_copy(self):
        return self.z.clone()
