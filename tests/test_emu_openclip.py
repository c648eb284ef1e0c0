"""A subset of tests/test_openclip_gpu.py on the CPU emulation of the kernels (tools/hipemu): the 96-wide attention forward and
backward at T = 33 and 129, a reduced tower with heads of 80, and the GELU text tower.  Test infrastructure; says nothing about speed."""
import os
import shutil
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _emu  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") or shutil.which("make") is None,
                                reason="needs the ROCm host clang++ and make to build tools/hipemu")


@pytest.fixture(scope="module")
def emu():
    with _emu.enable():
        import test_openclip_gpu as tg
        tg.DEV = "cpu"
        yield tg
        tg.DEV = "cuda"


@pytest.mark.parametrize("h16", [1, 0])
def test_mha_96_columns_on_the_emulated_kernels(emu, h16):
    for T in (33, 129):          # 129: one key in the second LDS chunk, one live lane in the fifth wave
        emu.attention96_checks(T, h16)


@pytest.mark.parametrize("precision", ["f32", "fp16"])
def test_reduced_tower_with_heads_of_80_on_the_emulated_kernels(emu, precision):
    emu.tower_checks("tiny-H-32", 1, precision)


def test_gelu_text_tower_on_the_emulated_kernels(emu):
    emu.text_checks(n=2)
