"""Writes tests/golden/pixel_drawer_golden.npz: what pixray's own pixel drawer (pixeldrawer.py) builds for a table of settings --
the grid size its __init__ settles on, the fp32 polygon of every cell from its shape helpers, and the cell colours that
encode_image's loop takes from a seeded init image.  The reference code runs from the reference checkout through
tests/_refextract.py, with pydiffvg replaced by stand-ins that only record the polygons and fill colours (nothing is rendered).
The tests read only the npz.

    python tests/golden/make_golden_pixel.py

Per row r: `r{i}/grid` (cols, rows), `r{i}/verts` float32 [n, k, 2], `r{i}/colors` float32 [n, 4].  The init image of a row is
regenerated from its seed by `init_image`."""
import math
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

OUT = os.path.join(HERE, "pixel_drawer_golden.npz")

TYPES = ["rect", "rectshift", "hex", "tri", "diamond", "knit"]
# size = canvas (W, H); init = init image (W, H) when it differs from the canvas
ROWS = []
for _t in TYPES + ["blob"]:                     # an unknown type is drawn as rect
    ROWS.append(dict(pixel_type=_t, size=(64, 64), pixel_scale=2.0))
    ROWS.append(dict(pixel_type=_t, size=(48, 80), pixel_scale=2.0))
    ROWS.append(dict(pixel_type=_t, size=(120, 72), pixel_scale=4.0))
ROWS += [
    dict(pixel_type="rect", size=(360, 360), pixel_scale=2.5),            # the text2pixel preset (quality better): 40 x 40
    dict(pixel_type="hex", size=(360, 360), pixel_scale=2.5),             # 41 x 57
    dict(pixel_type="diamond", size=(90, 50)),                            # default landscape grid, rows doubled
    dict(pixel_type="tri", size=(50, 90)),                                # default portrait grid, columns * 1.414
    dict(pixel_type="hex", size=(70, 70), pixel_iso_check=False, pixel_scale=3.0),
    dict(pixel_type="tri", size=(70, 70), pixel_edge_check=False, pixel_scale=3.0),
    dict(pixel_type="diamond", size=(66, 40), pixel_edge_check=False, pixel_iso_check=False, pixel_scale=2.0),
    dict(pixel_type="knit", size=(64, 48), pixel_size=(10, 7)),
    dict(pixel_type="tri", size=(64, 48), pixel_size=(12, 9)),            # pixel_size given: no iso adjustment
    dict(pixel_type="rectshift", size=(30, 20)),                          # the default grid shrunk to the canvas
    dict(pixel_type="rect", size=(96, 64), pixel_size=(12, 8), init=(50, 30)),     # init image smaller than the canvas
    dict(pixel_type="hex", size=(96, 64), pixel_size=(9, 7), init=(200, 150)),      # sub-sampled with a non-integer step
    dict(pixel_type="diamond", size=(40, 40), pixel_size=(40, 40), init=(30, 30)),  # cells narrower than a pixel: no sub-samples
    dict(pixel_type="rect", size=(40, 30), pixel_scale=-1.0),             # a non-positive scale is ignored
]


def settings(row):
    return types.SimpleNamespace(size=list(row["size"]), pixel_size=row.get("pixel_size"), pixel_scale=row.get("pixel_scale"),
                                 pixel_type=row["pixel_type"], pixel_edge_check=row.get("pixel_edge_check", True),
                                 pixel_iso_check=row.get("pixel_iso_check", True), transparent=False)


def init_image(i):
    """the seeded init image of row i, [1, 3, H, W] in [-1, 1]"""
    w, h = ROWS[i].get("init", ROWS[i]["size"])
    return torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(500 + i)) * 2 - 1


def _reference_drawer_class():
    from _refextract import extract

    class DrawingInterface:
        pass

    class Polygon:
        def __init__(self, points, is_closed):
            self.points = points

    class ShapeGroup:
        def __init__(self, shape_ids, fill_color, stroke_color=None):
            self.fill_color = fill_color

    class RenderFunction:
        serialize_scene = staticmethod(lambda *a, **k: [])
        apply = staticmethod(lambda *a, **k: None)

    pydiffvg = types.SimpleNamespace(Polygon=Polygon, ShapeGroup=ShapeGroup, RenderFunction=RenderFunction)
    ns = extract("pixeldrawer.py", ["rect_from_corners", "map_number", "diamond_from_corners", "tri_from_corners", "hex_from_corners",
                                    "knit_from_corners", "shift_pixel_types", "PixelDrawer"],
                 {"DrawingInterface": DrawingInterface, "pydiffvg": pydiffvg, "np": np, "math": math, "random": random})
    return ns["PixelDrawer"]


def main():
    PixelDrawer = _reference_drawer_class()
    out = {}
    for i, row in enumerate(ROWS):
        d = PixelDrawer(settings(row))
        color_vars, _img, shapes, _groups = d.encode_image(init_image(i))
        out[f"r{i}/grid"] = np.array([d.num_cols, d.num_rows], dtype=np.int64)
        out[f"r{i}/verts"] = torch.stack([s.points for s in shapes]).numpy().astype(np.float32)
        out[f"r{i}/colors"] = torch.stack([c.detach() for c in color_vars]).numpy().astype(np.float32)
        print(i, row, (d.num_cols, d.num_rows), out[f"r{i}/verts"].shape)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
