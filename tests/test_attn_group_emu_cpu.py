"""The grouped GEMM launch, the softmax launches with a transpose rider and the decoder's AttnBlock switch on
the CPU emulation of the kernels (tools/hipemu, tests/_emu.py): the GPU tests' own functions with their device switched to "cpu",
at the sizes a CPU affords.  Logic only -- member selection by grid z, the rider's block split, the decoder's two launch
sequences; nothing about speed."""
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
    with _emu.enable() as lib:
        import test_gemm_group_gpu as tg
        import test_softmax_transpose_rider_gpu as ts
        import test_vqgan_attn_group_gpu as tv
        for m in (tg, ts, tv):
            m.DEV = "cpu"
        yield lib, tg, ts, tv
        for m in (tg, ts, tv):
            m.DEV = "cuda"


@pytest.mark.parametrize("prec", ["fp16", "bf16", "f32"])
def test_gemm_group_on_the_emulated_kernels(emu, prec):
    _, tg, _, _ = emu
    for n in (1, 2, 3):
        tg.test_gemm_group_leaves_the_bytes_of_separate_launches(prec, 35, 128, 40, True, n)
    tg.test_gemm_group_leaves_the_bytes_of_separate_launches(prec, 256, 512, 256, True, 3)
    tg.test_gemm_group_leaves_the_bytes_of_separate_launches(prec, 256, 512, 512, False, 2)


def test_gemm_group_member_limit_and_mismatched_members_on_the_emulated_kernels(emu):
    emu[1].test_gemm_group_refuses_more_members_than_the_kernel_takes_and_mismatched_members_run_separately()


@pytest.mark.parametrize("prec", ["fp16", "bf16", "f32"])
def test_softmax_transpose_riders_on_the_emulated_kernels(emu, prec):
    _, _, ts, _ = emu
    for P, P8, TC in ts.SHAPES:
        ts.test_softmax_rows_with_a_transpose_rider_leaves_the_bytes_of_the_two_launches(prec, P, P8, TC)
        ts.test_softmax_rows_bwd_with_a_transpose_rider_leaves_the_bytes_of_the_two_launches(prec, P, P8, TC)


@pytest.mark.parametrize("precision", ["fp16", "f32"])
def test_decoder_attn_group_switch_on_the_emulated_kernels(emu, monkeypatch, precision):
    emu[3].test_attn_group_switch_leaves_image_and_latent_gradient_bytes(monkeypatch, precision, (5, 7))
