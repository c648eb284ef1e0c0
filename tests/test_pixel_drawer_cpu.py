"""The pixel drawer without a GPU: the drawer table and the front end's options, the reference fixture
(tests/golden/pixel_drawer_golden.npz), and every kernel of csrc/pixel_raster.hip run on the emulated library (tests/_emu.py)
against the float64 oracle of tests/_pixel_raster_ref.py, through the check functions of tests/test_pixel_drawer_gpu.py on CPU
tensors."""
import os
import shutil
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _emu  # noqa: E402
import test_pixel_drawer_gpu as pdg  # noqa: E402

needs_emu = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") or shutil.which("make") is None,
                               reason="needs the ROCm host clang++ and make to build tools/hipemu")


@pytest.fixture(scope="module")
def emu():
    with _emu.enable() as lib:
        pdg.DEV = "cpu"
        try:
            yield lib
        finally:
            pdg.DEV = "cuda"


def test_pixel_drawer_resolves_and_parses(tmp_path):
    """`--drawer pixel` (a KeyError before the drawer was registered) and its options"""
    pdg.check_names_resolve_and_parse(tmp_path)


def test_grid_sizes_match_reference():
    from make_golden_pixel import ROWS, settings
    from pixray_amd.pixel_drawer import PixelDrawer
    g = pdg.gold()
    for i, row in enumerate(ROWS):
        d = PixelDrawer(settings(row))
        assert (d.num_cols, d.num_rows) == tuple(g[f"r{i}/grid"]), (i, row)


@needs_emu
def test_fixture_rows_on_emulated_kernels(emu):
    pdg.check_fixture_rows()


@needs_emu
def test_jitter_twin_on_emulated_kernels(emu):
    pdg.check_jitter_twin()


@needs_emu
def test_parity_with_oracle_on_emulated_kernels(emu):
    pdg.check_small_parity()


@needs_emu
def test_overlapping_polygons_on_emulated_kernels(emu):
    pdg.check_overlapping_polygons()


@needs_emu
def test_integer_rect_cells_equal_pixel_grid_on_emulated_kernels(emu):
    pdg.check_integer_rect_cells_equal_pixel_grid()


@needs_emu
def test_emulated_runs_bit_identical(emu):
    pdg.check_bit_identical_runs()


@needs_emu
def test_emulated_reverse_schedule_bit_identical(emu):
    """the per-(tile, slot) partials and their per-shape sums do not depend on the order workgroups run in"""
    img, g, again = pdg.check_against_oracle(45, 37, "diamond", 8, "mixed", pixel_size=(7, 6))
    emu.hipemu_set_reverse_order(1)
    try:
        img2, g2 = again()
    finally:
        emu.hipemu_set_reverse_order(0)
    assert torch.equal(img, img2) and torch.equal(g, g2)


@needs_emu
def test_drawer_surface_on_emulated_kernels(emu):
    pdg.check_drawer_surface()
