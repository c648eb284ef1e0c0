"""The new CLIP towers' ground on the CPU through tools/hipemu (see tests/test_emu_cpu.py for what the emulation is and is not): a
ModifiedResNet of width 96 (stem 48, 48 heads) in the exact and the half mode against the oracle, and the workgroup-per-(image, head)
attention family at the 577 tokens of ViT-L/14@336px -- four workgroups of five waves per head, the last wave without tokens -- against
float64, with the gates of the GPU tests."""
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
        import test_clip_towers_gpu as tg
        mods = (tg.tp, tg.tf, tg.th)
        for m in mods:
            m.DEV = "cpu"
        tg.DEV = "cpu"
        yield lib, tg
        for m in mods:
            m.DEV = "cuda"
        tg.DEV = "cuda"


def test_emulated_library_exports_the_route_switch(emu):
    lib = emu[0]
    assert lib.prx_mha_route(1) == -1 and lib.prx_mha_route(0) == 1 and lib.prx_mha_route(-1) == 0 and lib.prx_mha_route(-1) == -1


@pytest.mark.parametrize("precision", ["f32", "fp16"])
def test_width_96_resnet_vs_oracle(emu, precision):
    """width 96, layers (1, 1, 1, 1), resolution 64 (a 2 x 2 final grid, 5 pool tokens), 48 heads, output 64; two cutouts: embeddings and
    d/dcutouts against the oracle at the gates of the `tiny-RN` tests"""
    tg = emu[1]
    from pixray_amd import weights
    weights.CLIP_RESNET_CONFIGS.setdefault("emu-RN96", weights.ClipResNetConfig("emu-RN96", 64, 96, (1, 1, 1, 1), 48, 64))
    if precision == "f32":
        tg.tf.test_clip_resnet_f32_vs_oracle("emu-RN96", 2)
    else:
        tg.tp.test_clip_resnet_vs_oracle("emu-RN96", 2, precision)


@pytest.mark.parametrize("h16", [0, 1], ids=["bf16", "half"])
def test_workgroup_attention_family_at_577_tokens(emu, h16):
    """one head, N = 1, T = 577, forward and backward through the workgroup family (19 token blocks on 4 x 5 waves) against float64 at
    test_kernels_half_gpu's gates; the tile kernels on the same operands agree with it to rounding and differ in bits"""
    import torch
    tg = emu[1]
    with tg.mha_route(tg.ROUTE_BLK):
        fig, out, dqkv, _, _ = tg.th.attention_case(1, 577, 64, 1, h16, general=True, seed=5)
    with tg.mha_route(tg.ROUTE_TILES):
        _, out_t, dqkv_t, _, _ = tg.th.attention_case(1, 577, 64, 1, h16, general=True, seed=5)
    print(fig)
    assert not torch.equal(out, out_t) or not torch.equal(dqkv, dqkv_t)
