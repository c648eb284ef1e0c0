"""A subset of tests/test_convnext_gpu.py on the CPU emulation of the kernels (tools/hipemu): the depthwise 7x7 kernel at its three
smallest shapes, the space-to-depth / pool / LayerNorm kernels, the reduced tower tiny-cnx and the refusals.  Test infrastructure; says
nothing about speed."""
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
        import test_convnext_gpu as tg
        tg.DEV = "cpu"
        yield tg
        tg.DEV = "cuda"


@pytest.mark.parametrize("precision", ["fp16", "bf16", "f32"])
@pytest.mark.parametrize("shape", [(2, 2, 2, 64), (1, 3, 3, 128), (1, 5, 9, 8)], ids=lambda s: "x".join(map(str, s)))
def test_depthwise_7x7_on_the_emulated_kernels(emu, shape, precision):
    emu.dwconv_checks(shape, precision)


@pytest.mark.parametrize("precision", ["fp16", "bf16", "f32"])
@pytest.mark.parametrize("shape", [(2, 2, 2, 64), (1, 6, 10, 192), (2, 16, 16, 128)], ids=lambda s: "x".join(map(str, s)))
def test_space_to_depth_and_pool_on_the_emulated_kernels(emu, shape, precision):
    emu.layout_checks(shape, precision)


@pytest.mark.parametrize("precision", ["fp16", "f32"])
@pytest.mark.parametrize("rows,C,group", [(9, 64, 4), (7, 96, 0), (3, 3072, 0)])
def test_channel_layernorm_on_the_emulated_kernels(emu, rows, C, group, precision):
    emu.layernorm_checks(rows, C, precision, group)


@pytest.mark.parametrize("precision", ["f32", "fp16"])
def test_reduced_tower_on_the_emulated_kernels(emu, precision):
    emu.tower_checks("tiny-cnx", 1, precision)


def test_refusals_on_the_emulated_kernels(emu):
    emu.refusal_checks()


@pytest.mark.parametrize("precision", ["fp16", "f32"])
@pytest.mark.parametrize("name", ["tiny-cnx", "tiny-cnx-d"])
def test_allocation_arithmetic_and_a_failed_create(emu, name, precision):
    """on the emulator's allocation hooks: the bytes a handle holds grow by weights.clip_convnext_activation_bytes per cutout of
    max_batch EXACTLY (the figure include/prx.h and the documents state for the real towers comes from that function); create + drop
    returns the live allocations to the baseline; with the k-th allocation refused the create raises PrxError naming the bytes asked
    for and the bytes held, nothing stays allocated, and the next create works"""
    import ctypes
    import gc
    import re
    import torch
    from pixray_amd import _lib, ops, weights
    lib = _lib.load()
    lib.hipemu_live_allocs.argtypes, lib.hipemu_live_allocs.restype = [ctypes.c_void_p, ctypes.c_void_p], None
    lib.hipemu_fail_alloc.argtypes, lib.hipemu_fail_alloc.restype = [ctypes.c_longlong], ctypes.c_longlong

    def live():
        gc.collect()
        n, b = ctypes.c_longlong(), ctypes.c_longlong()
        lib.hipemu_live_allocs(ctypes.addressof(n), ctypes.addressof(b))
        return n.value, b.value

    cfg = weights.CLIP_CONVNEXT_CONFIGS[name]
    params = weights.synthetic_clip_convnext_params(cfg, 0)
    cpu = torch.device("cpu")
    base = live()
    held = {}
    for mb in (1, 3):
        h = ops.ClipConvNextHandle(cfg, params, mb, cpu, precision=precision)
        now = live()
        held[mb] = (now[0] - base[0], now[1] - base[1])
        del h
        assert live() == base
    assert held[1][0] == held[3][0]
    assert held[3][1] - held[1][1] == 2 * weights.clip_convnext_activation_bytes(cfg, precision), (held, weights.clip_convnext_activation_bytes(cfg, precision))
    n_alloc = held[1][0]
    for k in sorted({0, n_alloc // 2, n_alloc - 1}):
        lib.hipemu_fail_alloc(k)
        try:
            with pytest.raises(_lib.PrxError, match=r"convnext_create: device allocation of \d+ bytes failed .* with \d+ bytes already held .*max_batch = 1 ") as ei:
                ops.ClipConvNextHandle(cfg, params, 1, cpu, precision=precision)
        finally:
            at_failure = lib.hipemu_fail_alloc(-1)
        assert int(re.search(r"with (\d+) bytes already held", str(ei.value)).group(1)) == at_failure - base[1]
        del ei
        assert live() == base, (k, live(), base)
    h = ops.ClipConvNextHandle(cfg, params, 1, cpu, precision=precision)
    assert bool(torch.isfinite(ops.clip_encode_image(torch.rand(1, 3, cfg.input_resolution, cfg.input_resolution), h)).all())
    del h
