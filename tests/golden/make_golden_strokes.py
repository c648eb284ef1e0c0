"""Writes tests/golden/stroke_drawers_golden.npz: what pixray's own stroke drawers (linedrawer.py `LineDrawer`, clipdrawer.py
`ClipDrawer`) build in load_model for a table of settings and Python `random` seeds -- every path's control points, segment
count and stroke width, the stroke colours and the paper colour.  The reference code runs from the reference checkout through
tests/_refextract.py, with pydiffvg replaced by stand-ins that only record the paths and shape groups (`render` returns zeros),
and skimage / ttools by empty modules.  The tests read only the npz.

    python tests/golden/make_golden_strokes.py

Per row r: `r{i}/points` float32 [P, 2] (all paths, in order), `r{i}/segments` int64 [n], `r{i}/widths` float32 [n],
`r{i}/colors` float32 [n, 4], and for line_sketch `r{i}/paper` float32 [4]."""
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

OUT = os.path.join(HERE, "stroke_drawers_golden.npz")

LINE_DEFAULTS = dict(strokes=24, stroke_length=8, min_stroke_width=0.5, max_stroke_width=2.0, allow_paper_color=False)
CLIP_DEFAULTS = dict(strokes=1024, min_stroke_width=1.0, max_stroke_width=5.0)
# drawer, canvas (W, H), Python random seed, option overrides
ROWS = [
    ("line_sketch", (384, 216), 0, {}),
    ("line_sketch", (576, 324), 1, {}),
    ("line_sketch", (64, 64), 2, dict(strokes=3, stroke_length=1)),
    ("line_sketch", (90, 160), 3, dict(strokes=5, stroke_length=20, max_stroke_width=4.0)),
    ("line_sketch", (200, 120), 4, dict(strokes=2, allow_paper_color=True)),
    ("line_sketch", (48, 30), 5, dict(strokes=60, stroke_length=3, min_stroke_width=1.0, max_stroke_width=6.0)),
    ("clipdraw", (384, 216), 0, {}),
    ("clipdraw", (576, 324), 1, {}),
    ("clipdraw", (64, 48), 2, dict(strokes=1)),
    ("clipdraw", (50, 90), 3, dict(strokes=40, min_stroke_width=0.5, max_stroke_width=2.0)),
    ("clipdraw", (128, 128), 4, dict(strokes=200)),
]


def settings(row):
    name, size, _seed, over = row
    opts = dict(LINE_DEFAULTS if name == "line_sketch" else CLIP_DEFAULTS, **over)
    return types.SimpleNamespace(size=list(size), **opts)


def _reference_classes():
    from _refextract import extract

    class DrawingInterface:
        pass

    class Path:
        def __init__(self, num_control_points, points, stroke_width, is_closed):
            self.num_control_points, self.points, self.stroke_width = num_control_points, points, stroke_width

    class Rect:
        def __init__(self, p_min, p_max):
            self.p_min, self.p_max = p_min, p_max

    class ShapeGroup:
        def __init__(self, shape_ids, fill_color, stroke_color=None):
            self.fill_color, self.stroke_color = fill_color, stroke_color

    def render(width, height, *a):
        return torch.zeros(height, width, 4)

    pydiffvg = types.SimpleNamespace(Path=Path, Rect=Rect, ShapeGroup=ShapeGroup, set_use_gpu=lambda *a: None,
                                     set_device=lambda *a: None, get_device=lambda: torch.device("cpu"),
                                     RenderFunction=types.SimpleNamespace(serialize_scene=lambda *a, **k: [], apply=render))
    base = {"DrawingInterface": DrawingInterface, "pydiffvg": pydiffvg, "np": np, "random": random,
            "skimage": types.ModuleType("skimage"), "ttools": types.ModuleType("ttools")}
    line = extract("linedrawer.py", ["bound", "LineDrawer"], dict(base))
    clip = extract("clipdrawer.py", ["ClipDrawer"], dict(base))
    return {"line_sketch": line["LineDrawer"], "clipdraw": clip["ClipDrawer"]}


def main():
    classes = _reference_classes()
    out = {}
    for i, row in enumerate(ROWS):
        name, _size, seed, _over = row
        st = settings(row)
        d = classes[name](st)
        random.seed(seed)
        d.load_model(st, "cpu")
        paths = [s for s in d.shapes if hasattr(s, "num_control_points")]
        groups = d.shape_groups[len(d.shape_groups) - len(paths):]
        out[f"r{i}/points"] = torch.cat([p.points.detach() for p in paths]).numpy().astype(np.float32)
        out[f"r{i}/segments"] = np.array([len(p.num_control_points) for p in paths], dtype=np.int64)
        out[f"r{i}/widths"] = np.array([float(p.stroke_width.detach()) for p in paths], dtype=np.float32)
        out[f"r{i}/colors"] = torch.stack([g.stroke_color.detach().float() for g in groups]).numpy().astype(np.float32)
        if name == "line_sketch":
            out[f"r{i}/paper"] = d.shape_groups[0].fill_color.detach().numpy().astype(np.float32)
        print(i, row, out[f"r{i}/points"].shape)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
