"""Writes tests/golden/more_plugins_golden.npz: what pixray's own EdgeLoss (with --edge_input_image / --edge_mask_image),
GaussianLoss and AestheticLoss (Losses/*.py) compute on seeded inputs -- loss values and input gradients -- run from the
reference checkout through tests/_refextract.py with stand-ins for what is absent offline.  The tests read only the npz.

    python tests/golden/make_golden_more_plugins.py

Stand-ins: `LossInterface` of this package; `braceexpand` as the identity list; torchvision's `TF.to_tensor` / `TF.resize`
(-> F.interpolate bicubic, align_corners=False: the tensor resize of pixray's pinned torchvision, no antialias); `wget_file` and
`urlopen` RAISE, so that no branch that would fetch anything can run unnoticed; `torch.Tensor.cuda` is the identity while
EdgeLoss runs (EdgeLoss.py:77).  The source picture and mask are stored in the npz as arrays; generator and tests write them to
PNG files in a temporary directory (`write_sources`)."""
import glob
import os
import re
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

OUT = os.path.join(HERE, "more_plugins_golden.npz")

CANVAS = (40, 48)
EDGE_CASES = {                      # name -> (thickness, margins, colour, colour weight, global weight, image?, mask?, batch)
    "img_thick10": (10, None, "white", 0.1, 0.05, True, False, 1),
    "img_margins": (5, [10, 5, 0, 20], "white", 0.3, 0.0, True, False, 1),
    "mask_red": (5, None, "red", 0.1, 0.05, False, True, 1),
    "img_mask": (5, None, "white", 0.2, 0.05, True, True, 1),
    "img_mask_b2": (5, None, "white", 0.2, 0.05, True, True, 2),
}
GAUSS_CASES = {                     # name -> (std (rows, columns), colour 0..255, weight, input)
    "std9_13": ((9.0, 13.0), (255.0, 128.0, 0.0), 0.7, "image"),
    "defaults": ((40, 40), (255, 255, 255), 1, "image"),
    "green_block": ((9.0, 13.0), (255.0, 128.0, 0.0), 0.7, "image_green"),
}
GREEN_BLOCK = (slice(10, 20), slice(12, 30))      # rows, columns of the green plane set to exactly float32(128 / 255)
AES_D, AES_BIAS, AES_SEED = 512, 5.0, 21
AES_CASES = {"n5_t10": (5, 10.0), "n5_t7.5": (5, 7.5), "n1_t10": (1, 10.0)}     # name -> (rows, target)


def small_input(seed, shape):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


def source_arrays():
    """the seeded source picture uint8 [14, 20, 3] and mask uint8 [14, 20]: zeros, a 255 rectangle, one grey pixel"""
    pic = torch.randint(0, 256, (14, 20, 3), generator=torch.Generator().manual_seed(7), dtype=torch.int64).numpy().astype(np.uint8)
    mask = np.zeros((14, 20), np.uint8)
    mask[3:10, 5:14] = 255
    mask[11, 17] = 100
    return pic, mask


def write_sources(pic, mask, directory):
    """-> (picture path, mask path): lossless PNG files of the two arrays"""
    from PIL import Image
    p, m = os.path.join(str(directory), "edge_picture.png"), os.path.join(str(directory), "edge_mask.png")
    Image.fromarray(np.ascontiguousarray(pic), "RGB").save(p)
    Image.fromarray(np.ascontiguousarray(mask), "L").save(m)
    return p, m


def aesthetic_head(d=AES_D, seed=AES_SEED, bias=AES_BIAS):
    """the seeded stand-in for ava_vit_b_16_linear.pth: {"weight": [1, d], "bias": [1]}"""
    g = torch.Generator().manual_seed(seed)
    return {"weight": torch.randn(1, d, generator=g) * 0.3, "bias": torch.full((1,), float(bias))}


def aesthetic_embeds(n, d=AES_D, seed=AES_SEED):
    return torch.randn(n, d, generator=torch.Generator().manual_seed(seed + 100 + n))


def edge_args(case, picture, mask):
    t, margins, colour, cw, gw, use_img, use_mask, _ = EDGE_CASES[case]
    return types.SimpleNamespace(edge_thickness=t, edge_margins=None if margins is None else list(margins), edge_color=colour,
                                 edge_color_weight=cw, global_color_weight=gw, edge_input_image=picture if use_img else "",
                                 edge_mask_image=mask if use_mask else "")


def gauss_args(case):
    std, colour, weight, _ = GAUSS_CASES[case]
    return types.SimpleNamespace(gaussian_std=std, gaussian_color=colour, gaussian_weight=weight)


def inputs():
    img = small_input(2, (1, 3, *CANVAS))
    img2 = small_input(4, (2, 3, *CANVAS))
    green = small_input(5, (1, 3, *CANVAS))
    green[0, 1][GREEN_BLOCK] = float(np.float32(128 / 255))
    return {"image": img, "image2": img2, "image_green": green}


def _fetch_refused(*a, **k):
    raise RuntimeError("the fixture generator fetches nothing")


def _ref():
    from _refextract import extract
    from PIL import Image
    from pixray_amd.interfaces import LossInterface
    import matplotlib.colors
    util = extract("util.py", ["real_glob", "map_number", "parse_triple_to_rgb", "get_single_rgb"],
                   {"re": re, "matplotlib": matplotlib, "glob": glob, "braceexpand": lambda s: [s]})

    def to_tensor(pil):
        a = torch.from_numpy(np.asarray(pil, dtype=np.uint8).copy())
        a = a.unsqueeze(2) if a.dim() == 2 else a
        return a.permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    TF = types.SimpleNamespace(to_tensor=to_tensor, InterpolationMode=types.SimpleNamespace(BICUBIC="bicubic"),
                               resize=lambda t, size, mode: F.interpolate(t, size=list(size), mode=mode, align_corners=False))
    ns = dict(LossInterface=LossInterface, get_single_rgb=util["get_single_rgb"], map_number=util["map_number"],
              real_glob=util["real_glob"], Image=Image, Path=Path, TF=TF, wget_file=_fetch_refused, urlopen=_fetch_refused,
              optim=torch.optim)
    R = types.SimpleNamespace()
    R.Edge = extract("Losses/EdgeLoss.py", ["EdgeLoss"], dict(ns))["EdgeLoss"]
    R.Gaussian = extract("Losses/GaussianLoss.py", ["gaussian_fn", "gkern", "GaussianLoss"], dict(ns))["GaussianLoss"]
    R.Aesthetic = extract("Losses/AestheticLoss.py", ["AestheticLoss"], dict(ns))["AestheticLoss"]
    return R


def _loss_and_grad(fn, x):
    x = x.clone().requires_grad_(True)
    loss = fn(x)
    loss.backward()
    return loss.detach(), x.grad


def main():
    from _refextract import available
    if not available():
        raise SystemExit("the reference checkout is needed to regenerate the fixture")
    R = _ref()
    rec = {}
    pic, mask = source_arrays()
    rec["in/edge_picture"], rec["in/edge_mask"] = pic, mask
    ins = inputs()
    for k, v in ins.items():
        rec[f"in/{k}"] = v.numpy()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        pic_path, mask_path = write_sources(pic, mask, tmp)
        saved = torch.Tensor.cuda
        torch.Tensor.cuda = lambda self, *a_, **k_: self          # EdgeLoss.py starts its sum with torch.tensor(0.).cuda()
        try:
            for case in EDGE_CASES:
                obj = R.Edge(device="cpu")
                a = obj.parse_settings(edge_args(case, pic_path, mask_path))
                x = ins["image2" if EDGE_CASES[case][7] == 2 else "image"]
                loss, grad = _loss_and_grad(lambda t: obj.get_loss({}, t, a), x)
                rec[f"edge/{case}/loss"], rec[f"edge/{case}/grad"] = loss.numpy(), grad.numpy()
                if obj.resized_mask is not None:
                    m = obj.resized_mask
                    nz = m[m != 0].abs().min().item()
                    print(f"edge/{case}: mask {m.min().item():.3f} .. {m.max().item():.3f}, {100 * (m > 0).float().mean().item():.0f}% > 0, "
                          f"smallest non-zero magnitude {nz:.2e}")
        finally:
            torch.Tensor.cuda = saved
        for case, (_, _, _, which) in GAUSS_CASES.items():
            obj = R.Gaussian(device="cpu")
            a = gauss_args(case)
            loss, grad = _loss_and_grad(lambda t: obj.get_loss({}, t, a), ins[which])
            rec[f"gauss/{case}/loss"], rec[f"gauss/{case}/grad"] = loss.numpy(), grad.numpy()
        # AestheticLoss looks for models/ava_vit_b_16_linear.pth under the working directory and downloads it when missing:
        # put the seeded head there and change directory BEFORE constructing the class
        os.makedirs(os.path.join(tmp, "models"))
        head = aesthetic_head()
        torch.save(head, os.path.join(tmp, "models", "ava_vit_b_16_linear.pth"))
        rec["aes/weight"], rec["aes/bias"] = head["weight"].numpy(), head["bias"].numpy()
        os.chdir(tmp)
        try:
            for case, (n, target) in AES_CASES.items():
                obj = R.Aesthetic(device="cpu")
                a = obj.parse_settings(types.SimpleNamespace(num_cuts=n, aesthetic_target=target))
                e = aesthetic_embeds(n)
                rating = obj.ae_reg(F.normalize(e, dim=-1)).detach()
                assert float((rating - target).abs().min()) >= 2.0, (case, rating.flatten().tolist())     # away from the loss's zero
                loss, grad = _loss_and_grad(lambda t: obj.get_loss({}, None, a, globals={"embeds": t}), e)
                rec[f"aes/{case}/embeds"], rec[f"aes/{case}/loss"], rec[f"aes/{case}/grad"] = e.numpy(), loss.numpy(), grad.numpy()
                print(f"aes/{case}: loss {float(loss):.4f}")
        finally:
            os.chdir(cwd)
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT}: {len(rec)} arrays, {os.path.getsize(OUT) / 1e3:.0f} kB")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
