"""`--palette` strings -> lists of [r, g, b] in 0..1, and the linear `map_number` the built-in plugins share.

The grammar is pixray's (util.py, "PALETTE SECTION"):

    red                      16-step ramp from black to red
    rust\\8                   8-step ramp from black to rust
    red->yellow              16-step ramp from red to yellow; more `->` stops make a multi-stop ramp
    red->#ff0000\\20          20-step ramp
    [black, red, #ff0000]    exactly these colours; `[...]\\N` resamples the list to N steps
    red->white;blue          sections joined by `;` are concatenated

A single colour is `(r+g+b)` in 0..255, `[r+g+b]` in 0..1, one of the `pixel_*` names, `mat:<matplotlib name>`, an xkcd
colour name, or anything `matplotlib.colors.to_rgb` accepts.  Image / .act palette files (`@file`, URLs) are not read here.
"""
import re
from typing import List, Sequence

_PIXEL_COLOURS = {
    "pixel_green": [0.44, 1.00, 0.53],
    "pixel_orange": [1.00, 0.80, 0.20],
    "pixel_blue": [0.44, 0.53, 1.00],
    "pixel_red": [1.00, 0.53, 0.44],
    "pixel_grayscale": [1.00, 1.00, 1.00],
}
DEFAULT_RAMP_STEPS = 16


def map_number(n, start1, stop1, start2, stop2):
    """the value n in [start1, stop1] carried linearly onto [start2, stop2] (p5.js `map`)"""
    return ((n - start1) / (stop1 - start1)) * (stop2 - start2) + start2


def _mcolors():
    try:
        import matplotlib.colors as mcolors
    except ImportError as e:
        raise RuntimeError("named palette colours need matplotlib (matplotlib.colors); install it or give colours as "
                           "(r+g+b) / [r+g+b] triples") from e
    return mcolors


def _triple(s: str) -> List[float]:
    vals = [float(v) for v in re.sub(r"[()\[\]]", "", s).split("+")]
    return [v / 255.0 for v in vals] if s[0] == "(" else vals


def get_single_rgb(s: str):
    """one colour specification -> [r, g, b] (a tuple when matplotlib produced it)"""
    if s[0] in "([":
        return _triple(s)
    if s in _PIXEL_COLOURS:
        return _PIXEL_COLOURS[s]
    mc = _mcolors()
    if s.startswith("mat:"):
        return mc.to_rgb(s[4:])
    if mc.is_color_like(f"xkcd:{s}"):
        return mc.to_rgb(f"xkcd:{s}")
    return mc.to_rgb(s)


def _resample(colours: Sequence, steps: int) -> list:
    """`steps` colours spread evenly along the piecewise-linear path through `colours`"""
    out = []
    k = len(colours)
    for i in range(steps):
        pos = map_number(i, 0, steps - 1, 0, k - 1)
        lo = int(pos)
        frac = pos - lo
        if frac < 1e-6 or 1.0 - frac < 1e-6:
            out.append(colours[lo])
        else:
            a, b = colours[lo], colours[lo + 1]
            out.append([map_number(frac, 0, 1, a[c], b[c]) for c in range(3)])
    return out


def _split_steps(s: str):
    if s.find("\\") > 0:
        body, steps = s.split("\\")
        return body, int(steps)
    return s, None


def _section(s: str) -> list:
    s = s.strip()
    if s.startswith("@") or s.startswith("http"):
        raise ValueError(f"palette files and URLs are not supported: {s!r}")
    if s[0] == "[":
        body, steps = _split_steps(s)
        colours = [get_single_rgb(c.strip()) for c in body[1:-1].split(",")]
        return _resample(colours, steps) if steps is not None else colours
    stops = s.split("->") if s.find("->") > 0 else ["black", s]
    stops[-1], steps = _split_steps(stops[-1])
    return _resample([get_single_rgb(c) for c in stops], steps if steps is not None else DEFAULT_RAMP_STEPS)


def palette_from_string(s: str) -> list:
    """a whole `--palette` value -> list of colours (sections separated by `;`, concatenated)"""
    out = []
    for sec in s.strip().split(";"):
        out = out + _section(sec)
    return out
