"""The aesthetic, image / mask edge and gaussian losses without a GPU: the new kernels of csrc/plugin_losses.hip run on the
emulated library (tests/_emu.py) against the reference fixture (tests/golden/more_plugins_golden.npz), through the check
functions of tests/test_more_plugins_gpu.py on CPU tensors, and the host-only paths (errors, option tables)."""
import argparse
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
import test_more_plugins_gpu as mp  # noqa: E402

needs_emu = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") or shutil.which("make") is None,
                               reason="needs the ROCm host clang++ and make to build tools/hipemu")


@pytest.fixture(scope="module")
def emu():
    with _emu.enable() as lib:
        mp.DEV = "cpu"
        mp.GRAD_RTOL = 1e-5
        try:
            yield lib
        finally:
            mp.DEV = "cuda"
            mp.GRAD_RTOL = 1e-4


# ------------------------------------------------------------------------------------------------ host only
def test_gaussian_is_exported_and_not_registered():
    from pixray_amd import plugins
    from pixray_amd.builtin_losses import BUILTIN_LOSSES, UNAVAILABLE_LOSSES, AestheticLoss, GaussianLoss
    assert "gaussian" not in plugins.loss_class_table and GaussianLoss not in BUILTIN_LOSSES.values()
    assert plugins.loss_class_table["aesthetic"] is AestheticLoss and BUILTIN_LOSSES["aesthetic"] is AestheticLoss
    assert list(UNAVAILABLE_LOSSES) == ["resmem"]
    assert AestheticLoss.needs_full_batch and all(c.supports_graph_replay for c in (AestheticLoss, GaussianLoss, BUILTIN_LOSSES["edge"]))


def test_plugin_table_builds_the_new_losses():
    mp.DEV = "cpu"
    try:
        mp.check_plugin_tables_build()
    finally:
        mp.DEV = "cuda"


def test_option_tables_follow_the_reference():
    from pixray_amd.builtin_losses import AestheticLoss, EdgeLoss, GaussianLoss
    p = argparse.ArgumentParser()
    for c in (AestheticLoss, EdgeLoss, GaussianLoss):
        c.add_settings(p)
    a = p.parse_args([])
    assert a.aesthetic_target == 10 and a.aesthetic_model == "models/ava_vit_b_16_linear.pth"
    assert a.gaussian_weight == 1 and tuple(a.gaussian_std) == (40, 40) and tuple(a.gaussian_color) == (255, 255, 255)
    assert a.edge_input_image == "" and a.edge_mask_image == ""
    helps = {x.dest: x.help for x in p._actions}
    assert "not supported" not in helps["edge_input_image"] and "not supported" not in helps["edge_mask_image"]
    a = p.parse_args(["--gaussian_std", "9", "13", "--gaussian_color", "255", "128", "0", "--aesthetic_model", "h.pth"])
    assert a.gaussian_std == [9.0, 13.0] and a.gaussian_color == [255.0, 128.0, 0.0] and a.aesthetic_model == "h.pth"


def test_gaussian_tables_are_the_reference_formula():
    from pixray_amd.builtin_losses import GaussianLoss
    for M, std in ((40, 9.0), (48, 13.0), (7, 40)):
        t = GaussianLoss.table(M, std)
        n = torch.arange(M, dtype=torch.float64) - (M - 1) / 2
        assert t.dtype == torch.float32 and t.shape == (M,)
        assert torch.allclose(t.double(), torch.exp(-n ** 2 / (2 * std * std)), rtol=1e-6, atol=0)
        assert torch.equal(t, t.flip(0))


def test_missing_aesthetic_file_says_where_it_looked(tmp_path):
    from pixray_amd.builtin_losses import AestheticLoss
    missing = str(tmp_path / "nope" / "head.pth")
    with pytest.raises(RuntimeError, match="aesthetic") as e:
        AestheticLoss().parse_settings(types.SimpleNamespace(aesthetic_model=missing))
    assert missing in str(e.value) and "aesthetic_model" in str(e.value) and "neither shipped" in str(e.value) and "fetched" in str(e.value)
    with pytest.raises(RuntimeError, match="ava_vit_b_16_linear.pth"):          # the default location, from an empty namespace
        AestheticLoss().parse_settings(types.SimpleNamespace())
    with pytest.raises(ValueError, match="aesthetic_model.*remote files are not fetched"):
        AestheticLoss().parse_settings(types.SimpleNamespace(aesthetic_model="https://example.org/head.pth"))


def test_aesthetic_embedding_width_mismatch(tmp_path):
    from pixray_amd.builtin_losses import AestheticLoss
    obj = AestheticLoss()
    args = obj.parse_settings(types.SimpleNamespace(aesthetic_model=mp._head_file(tmp_path, d=128), aesthetic_target=10))
    with pytest.raises(ValueError, match="AestheticLoss.*64 wide.*128 wide.*512-wide ViT-B"):
        obj.get_loss({}, None, args, globals={"embeds": torch.zeros(4, 64)})
    with pytest.raises(ValueError, match="embeds"):
        obj.get_loss({}, None, args, globals={"embeds": None})
    bad = str(tmp_path / "bad.pth")
    torch.save({"weight": torch.zeros(2, 8), "bias": torch.zeros(1)}, bad)
    with pytest.raises(ValueError, match="aesthetic_model"):
        AestheticLoss().parse_settings(types.SimpleNamespace(aesthetic_model=bad))


def _edge_ns(**kw):
    base = dict(edge_input_image="", edge_mask_image="", edge_color="white", edge_margins=None, edge_thickness=5)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_edge_file_options_fail_with_the_option_name(tmp_path):
    from pixray_amd.builtin_losses import EdgeLoss
    for opt in ("edge_input_image", "edge_mask_image"):
        with pytest.raises(ValueError, match=f"{opt}.*remote files are not fetched"):
            EdgeLoss().parse_settings(_edge_ns(**{opt: "http://example.org/a.png"}))
        pattern = str(tmp_path / "no_such_*.png")
        with pytest.raises(ValueError, match=opt) as e:
            EdgeLoss().parse_settings(_edge_ns(**{opt: pattern}))
        assert pattern in str(e.value)


def test_edge_files_load_by_glob_first_match(tmp_path):
    from pixray_amd.builtin_losses import EdgeLoss
    g = mp.gold()
    pic, mask = mp._sources(tmp_path)
    obj = EdgeLoss()
    args = obj.parse_settings(_edge_ns(edge_input_image=str(tmp_path / "edge_p*.png"), edge_mask_image=str(tmp_path / "edge_*.png")))
    assert args.edge_color == (1.0, 1.0, 1.0) or list(args.edge_color) == [1.0, 1.0, 1.0]
    assert torch.equal(obj.image, torch.from_numpy(g["in/edge_picture"]).permute(2, 0, 1).unsqueeze(0).float() / 255)
    # "edge_*.png" matches both files; sorted, the mask comes first
    assert torch.equal(obj.mask, torch.from_numpy(g["in/edge_mask"])[None, None].float() / 255)
    plain = EdgeLoss()
    plain.parse_settings(_edge_ns())
    assert plain.image is None and plain.mask is None


def test_new_ops_fail_loudly_without_a_gpu():
    from pixray_amd import _lib, ops
    if torch.cuda.is_available():
        return
    x = torch.rand(1, 3, 8, 8)
    with pytest.raises(_lib.PrxError):
        ops.aesthetic_loss(torch.randn(2, 8), torch.randn(8), 0.0, 10.0)
    with pytest.raises(_lib.PrxError):
        ops.edge_target_loss(x, None, (1, 1, 1), torch.ones(8, 8), (0, 0, 0, 0), 0.1, 0.05)
    with pytest.raises(_lib.PrxError):
        ops.gaussian_loss(x, torch.ones(8), torch.ones(8), (1, 1, 1), 1.0)


# ------------------------------------------------------------------------------------------------ emulated kernels
@needs_emu
def test_edge_matches_reference_on_emulated_kernels(emu):
    mp.check_edge_matches_reference()


@needs_emu
def test_edge_refits_on_a_new_canvas(emu):
    mp.check_edge_refits_on_a_new_canvas()


@needs_emu
def test_gaussian_matches_reference_on_emulated_kernels(emu):
    mp.check_gaussian_matches_reference()


@needs_emu
def test_aesthetic_matches_reference_on_emulated_kernels(emu):
    mp.check_aesthetic_matches_reference()


@needs_emu
def test_aesthetic_matches_float64_on_emulated_kernels(emu):
    mp.check_aesthetic_matches_float64()


@needs_emu
def test_argument_checks_of_the_new_ops(emu):
    from pixray_amd import _lib, ops
    x = torch.rand(1, 3, 8, 10)
    with pytest.raises(_lib.PrxError, match="3 channels"):
        ops.gaussian_loss(torch.rand(1, 4, 8, 10), torch.ones(8), torch.ones(10), (1, 1, 1), 1.0)
    with pytest.raises(_lib.PrxError, match="gx"):
        ops.gaussian_loss(x, torch.ones(8), torch.ones(8), (1, 1, 1), 1.0)
    with pytest.raises(_lib.PrxError, match="gy"):
        ops.gaussian_loss(x, torch.ones(8, dtype=torch.float64), torch.ones(10), (1, 1, 1), 1.0)
    with pytest.raises(_lib.PrxError, match="fp32"):
        ops.gaussian_loss(x.double(), torch.ones(8), torch.ones(10), (1, 1, 1), 1.0)
    with pytest.raises(_lib.PrxError, match="3 channels"):
        ops.edge_target_loss(torch.rand(1, 4, 8, 10), None, (1, 1, 1), None, (1, 1, 1, 1), 0.1, 0.0)
    with pytest.raises(_lib.PrxError, match="mask"):
        ops.edge_target_loss(x, None, (1, 1, 1), torch.ones(10, 8), (0, 0, 0, 0), 0.1, 0.0)
    with pytest.raises(_lib.PrxError, match="target"):
        ops.edge_target_loss(x, torch.ones(1, 1, 8, 10), (1, 1, 1), None, (1, 1, 1, 1), 0.1, 0.0)
    with pytest.raises(_lib.PrxError, match="empty band"):
        ops.edge_target_loss(x, torch.ones(1, 3, 8, 10), (1, 1, 1), None, (5, 5, 2, 0), 0.1, 0.0)
    with pytest.raises(_lib.PrxError, match="weight"):
        ops.aesthetic_loss(torch.randn(2, 8), torch.randn(7), 0.0, 10.0)
    with pytest.raises(_lib.PrxError, match=r"\[n, d\]"):
        ops.aesthetic_loss(torch.randn(2, 8, 1), torch.randn(8), 0.0, 10.0)


@needs_emu
def test_edge_target_without_files_is_the_flat_colour_kernel(emu):
    """target = null, mask = null: the new kernel adds up what edge_kernel adds up, bit for bit"""
    from pixray_amd import ops
    x = torch.rand(2, 3, 17, 23, generator=torch.Generator().manual_seed(9)).requires_grad_(True)
    outs = []
    for fn in (lambda: ops.edge_loss(x, (1.0, 0.5, 0.0), (3, 2, 0, 4), 0.3, 0.05),
               lambda: ops.edge_target_loss(x, None, (1.0, 0.5, 0.0), None, (3, 2, 0, 4), 0.3, 0.05)):
        loss = fn()
        (g,) = torch.autograd.grad(loss, x)
        outs.append((loss.detach(), g))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@needs_emu
def test_emulated_runs_bit_identical(emu):
    mp.check_bit_identical_runs()


@needs_emu
def test_emulated_reverse_schedule_bit_identical(emu):
    """the fixed-order reductions do not depend on the order workgroups finish in"""
    a = mp._all_outputs()
    emu.hipemu_set_reverse_order(1)
    try:
        b = mp._all_outputs()
    finally:
        emu.hipemu_set_reverse_order(0)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


@needs_emu
def test_aesthetic_needs_the_full_batch_under_sharding(emu):
    mp.check_sharding()
