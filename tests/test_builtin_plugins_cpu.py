"""The built-in custom losses and filters without a GPU: the plugin tables, the palette grammar, and every new kernel of
csrc/plugin_losses.hip / plugin_filters.hip run on the emulated library (tests/_emu.py) against the reference fixture
(tests/golden/builtin_plugins_golden.npz), through the check functions of tests/test_builtin_plugins_gpu.py on CPU tensors."""
import os
import shutil
import sys
import types

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _emu  # noqa: E402
import test_builtin_plugins_gpu as bp  # noqa: E402

needs_emu = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") or shutil.which("make") is None,
                               reason="needs the ROCm host clang++ and make to build tools/hipemu")


@pytest.fixture(scope="module")
def emu():
    with _emu.enable() as lib:
        bp.DEV = "cpu"
        bp.GRAD_RTOL = 1e-5
        try:
            yield lib
        finally:
            bp.DEV = "cuda"
            bp.GRAD_RTOL = 1e-4


def test_builtin_plugin_names_resolve():
    """every reference loss / filter name builds (KeyError / ValueError before the built-ins were registered)"""
    from pixray_amd import plugins
    bp.DEV = "cpu"
    try:
        bp.check_plugin_tables_build()
    finally:
        bp.DEV = "cuda"


def test_out_of_scope_plugins_fail_with_a_message():
    from pixray_amd import plugins
    args = types.SimpleNamespace()
    for name, what in (("resmem", "ResMem"), ("aesthetic", "aesthetic")):
        with pytest.raises(RuntimeError, match=what):
            plugins.setup_custom_losses(name, args)
    with pytest.raises(KeyError, match="gaussian"):
        plugins.setup_custom_losses("gaussian", args)
    from pixray_amd.builtin_losses import EdgeLoss, PaletteLoss
    with pytest.raises(ValueError, match="edge_mask_image"):
        EdgeLoss().parse_settings(types.SimpleNamespace(edge_input_image="", edge_mask_image="m.png", edge_color="white",
                                                        edge_margins=None, edge_thickness=5))
    with pytest.raises(ValueError, match="--palette"):
        PaletteLoss().parse_settings(types.SimpleNamespace(palette=None))


def test_palette_strings_match_reference():
    bp.check_palette_strings()


def test_frontend_converts_palette(tmp_path):
    from pixray_amd import frontend as fe
    run = fe.Run()
    run.settings = dict(skip_args=True, outdir=str(tmp_path / "a"), palette="red->yellow;[black]", custom_loss="palette", filters="wallpaper", wallpaper_type="shift")
    s = fe.apply_settings(run=run)
    assert len(s.palette) == 17 and s.palette[-1] == (0.0, 0.0, 0.0) and s.wallpaper_type == "shift" and s.palette_weight == 1
    run.settings = dict(skip_args=True, outdir=str(tmp_path / "b"))
    assert fe.apply_settings(run=run).palette is None


@needs_emu
def test_losses_match_reference_on_emulated_kernels(emu):
    bp.check_losses_small()


@needs_emu
def test_filters_match_reference_on_emulated_kernels(emu):
    bp.check_filters_small()


@needs_emu
def test_emulated_runs_bit_identical(emu):
    bp.check_bit_identical_runs()


@needs_emu
def test_emulated_reverse_schedule_bit_identical(emu):
    """the fixed-order reductions do not depend on the order workgroups finish in"""
    a = bp._all_outputs()
    emu.hipemu_set_reverse_order(1)
    try:
        b = bp._all_outputs()
    finally:
        emu.hipemu_set_reverse_order(0)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


@needs_emu
def test_full_batch_declarations_reproduce_unsharded_scores(emu):
    bp.check_shards_reproduce_full_batch()
