"""A subset of tests/test_openclip_big_gpu.py on the CPU emulation of the kernels (tools/hipemu): the ragged LayerNorm at C = 1408
(MAXV = 8), the 128-wide attention forward and backward at T = 1, 33 and 129, and heads of 88 on the 96-wide instances.  Test
infrastructure; says nothing about speed."""
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
        import test_openclip_big_gpu as tb
        tb.DEV = "cpu"
        yield tb
        tb.DEV = "cuda"


@pytest.mark.parametrize("h16", [1, 0])
@pytest.mark.parametrize("s16", [0, 7])
def test_ragged_layernorm_at_1408_on_the_emulated_kernels(emu, s16, h16):
    for rows in (1, 5):
        emu.layernorm_rag_checks(1408, rows, s16, h16, True)


@pytest.mark.parametrize("h16", [1, 0])
@pytest.mark.parametrize("T", [1, 33, 129])
def test_mha_128_columns_on_the_emulated_kernels(emu, T, h16):
    emu.attention_checks(104, T, 1, 2, h16)       # 129: one key in the second LDS chunk, one live lane in the fifth wave, two column passes


def test_mha_heads_of_88_on_the_emulated_kernels(emu):
    emu.attention_checks(88, 33, 1, 2, 1)
