"""The RRDBNet runner's HIP kernels (csrc/rrdbnet.hip), run on the CPU through tools/hipemu (see tests/test_emu_cpu.py for what
the emulation is and is not): the per-kernel tests of tests/test_kernels_rrdbnet_gpu.py on their smallest case each, and one
whole `tiny-RRDB` synth + backward at z = 5 x 7 against the float64 restatement, in both operand modes, with the gates of the GPU
tests."""
import os
import shutil
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _emu  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") or shutil.which("make") is None,
                                reason="needs the ROCm host clang++ and make to build tools/hipemu")


@pytest.fixture(scope="module")
def emu():
    with _emu.enable() as lib:
        import test_kernels_rrdbnet_gpu as tk
        import test_super_resolution_gpu as tsr
        tk.DEV = tsr.DEV = "cpu"
        yield lib, tk, tsr
        tk.DEV = tsr.DEV = "cuda"


def test_emulated_library_exports_the_rrdbnet_abi(emu):
    from pixray_amd import _lib
    names = [n for n in _lib._protos if "rrdb" in n]
    assert len(names) == 10 and all(hasattr(emu[0], n) for n in names)


@pytest.mark.parametrize("mode", ["f32", "fp16"])
def test_conv_family_smallest_cases(emu, mode):
    tk = emu[1]
    for cin in (64, 96, 128, 160):
        tk.conv_fwd_case(cin, 32, 5, 7, mode)
        tk.conv_dgrad_case(cin, 32, 5, 7, mode)
    tk.conv_fwd_case(192, 32, 5, 7, mode)
    tk.conv_dgrad_case(192, 32, 5, 7, mode)
    for resid in (1, 2):
        tk.conv_fwd_case(192, 64, 5, 7, mode, resid=resid, lrelu=False)
        tk.conv_dgrad_case(192, 64, 5, 7, mode, resid=resid)
    tk.test_conv_up_forward_and_backward(mode)


def test_ragged_tiles(emu):
    emu[1].conv_fwd_case(96, 32, 17, 33, "fp16")          # 561 pixels: the last tile of 16 is ragged
    emu[1].conv_dgrad_case(96, 32, 17, 33, "f32")


def test_leaky_relu_zero_and_refusals(emu):
    emu[1].test_leaky_relu_derivative_zero_takes_the_small_slope()
    emu[1].test_refusals_by_name()


@pytest.mark.parametrize("mode", ["f32", "fp16"])
def test_edge_convolutions(emu, mode):
    tk = emu[1]
    tk.test_conv_first_and_its_backward((5, 7), mode)
    tk.test_conv_last_forward_and_clamp((5, 7), mode)
    if mode == "f32":
        tk.test_conv_last_backward_clamp_rule((5, 7))


@pytest.mark.parametrize("mode", ["f32", "fp16"])
def test_tiny_rrdb_synth_and_backward(emu, mode):
    emu[2].network_case("tiny-RRDB", (5, 7), mode)
