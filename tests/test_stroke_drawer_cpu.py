"""The stroke drawers without a GPU: the drawer table and the front end's options, the reference fixture
(tests/golden/stroke_drawers_golden.npz), the float64 oracle of tests/_stroke_raster_ref.py against central differences, and
the kernels of csrc/stroke_raster.hip run on the emulated library (tests/_emu.py) against that oracle, through the check
functions of tests/test_stroke_drawer_gpu.py on CPU tensors.  Canvases stay small: the emulator runs every lane on the CPU."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _emu  # noqa: E402
import _stroke_raster_ref as ref  # noqa: E402
import test_stroke_drawer_gpu as sdg  # noqa: E402

needs_emu = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") or shutil.which("make") is None,
                               reason="needs the ROCm host clang++ and make to build tools/hipemu")


@pytest.fixture(scope="module")
def emu():
    with _emu.enable() as lib:
        sdg.DEV = "cpu"
        try:
            yield lib
        finally:
            sdg.DEV = "cuda"


def test_stroke_drawers_resolve_and_parse(tmp_path):
    """`--drawer line_sketch` / `--drawer clipdraw` (a KeyError before the drawers were registered) and their options"""
    sdg.check_names_resolve_and_parse(tmp_path)


def test_initialisation_matches_reference():
    sdg.check_fixture_init()


def test_oracle_gradient_matches_central_differences():
    """the oracle's autograd gradient (t* held fixed) against float64 central differences of its own image, away from kinks"""
    from pixray_amd.pixel_drawer import sample_offsets_np
    rng = np.random.default_rng(3)
    w, h = 14, 11
    paths = [sdg._walk(rng, 2, (4.0, 5.0), 4.0), sdg._cubic((2.1, 9.3), (6.2, 1.4), (9.7, 12.1), (12.6, 3.3))]
    pts, ps, wd, col, pa = sdg._scene_leaves(paths, [1.7, 1.2], [(0.8, 0.3, 0.1, 0.7), (0.2, 0.6, 0.9, 0.5)], (0.9, 0.8, 0.6, 0.8))
    uv = sample_offsets_np(w, h, 4)
    leaves = [t.double().requires_grad_(True) for t in (pts, wd, col, pa)]
    r = ref.render(leaves[0], ps, leaves[1], leaves[2], leaves[3], w, h, uv)
    probe = torch.randn(h, w, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * (~r["kink"].any(2))[..., None]
    (r["image"] * probe).sum().backward()
    eps = 1e-6
    for li, leaf in enumerate(leaves):
        flat = leaf.detach().reshape(-1)
        for j in range(flat.numel()):
            vals = []
            for sgn in (1, -1):
                moved = [x.detach().clone() for x in leaves]
                moved[li].view(-1)[j] += sgn * eps
                out = ref.render(moved[0], ps, moved[1], moved[2], moved[3], w, h, uv)["image"]
                vals.append(float((out * probe).sum()))
            fd = (vals[0] - vals[1]) / (2 * eps)
            assert abs(fd - float(leaf.grad.view(-1)[j])) <= 1e-5 * max(1.0, abs(fd)), (li, j, fd, float(leaf.grad.view(-1)[j]))


@needs_emu
def test_jitter_twin_on_emulated_kernels(emu):
    sdg.check_jitter_twin()


@needs_emu
def test_small_parity_on_emulated_kernels(emu):
    sdg.check_small_parity()


@needs_emu
def test_deep_stack_on_emulated_kernels(emu):
    sdg.check_deep_stack()


@needs_emu
def test_emulated_runs_bit_identical(emu):
    sdg.check_bit_identical_runs()


@needs_emu
def test_emulated_reverse_schedule_bit_identical(emu):
    """the per-(tile, path) partials and their per-path sums do not depend on the order workgroups run in"""
    img, g, again = sdg.check_deep_stack()
    emu.hipemu_set_reverse_order(1)
    try:
        img2, g2 = again()
    finally:
        emu.hipemu_set_reverse_order(0)
    assert torch.equal(img, img2) and all(torch.equal(a, b) for a, b in zip(g, g2) if a is not None)


@needs_emu
def test_fixture_rows_on_emulated_kernels(emu):
    """load_model end to end (small rows: the emulator is slow)"""
    sdg.check_fixture_rows(rows={2, 4, 8, 9})


@needs_emu
@pytest.mark.parametrize("name", ["line_sketch", "clipdraw"])
def test_drawer_surface_on_emulated_kernels(emu, name, tmp_path):
    sdg.check_drawer_surface(name, tmp_path)


@needs_emu
def test_refusals_on_emulated_kernels(emu):
    sdg.check_refusals()
