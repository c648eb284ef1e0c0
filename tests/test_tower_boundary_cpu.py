"""The boundary every image tower shares (csrc/runner_core.h ImageTower, ops._ImageTowerHandle), on the CPU emulation of the kernels
(tools/hipemu): the capacity and no-forward-in-flight guards with the runner's own word in front, and one engine context per handle.
Test infrastructure; says nothing about speed."""
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

# constructor (by its reduced configuration) -> the word the runner's messages begin with
TOWERS = {"tiny-B/32": "vit", "tiny-SLIP/16": "vit", "tiny-H-32": "vit", "tiny-RN": "resnet", "tiny-cnx": "convnext"}


@pytest.fixture(scope="module")
def emu():
    with _emu.enable():
        import test_kernels_runner_gpu as tr
        yield tr


@pytest.mark.parametrize("model", list(TOWERS))
def test_tower_guards_and_engine_context(emu, model):
    from pixray_amd import ops
    from pixray_amd._lib import PrxError, call
    word = TOWERS[model]
    h, R = emu.tower_handle(model, 1, "fp16", "cpu")
    other, _ = emu.tower_handle(model, 1, "fp16", "cpu")
    assert type(h).__name__ == {"tiny-B/32": "ClipVitHandle", "tiny-SLIP/16": "SlipVitHandle", "tiny-H-32": "OpenClipVitHandle",
                                "tiny-RN": "ClipResNetHandle", "tiny-cnx": "ClipConvNextHandle"}[model]
    assert (h.max_batch, h.generation, h.precision, h.cfg.input_resolution) == (1, 0, ops.precision_code("fp16"), R)
    # one engine context per handle
    assert h.gemm_ctx and other.gemm_ctx and h.gemm_ctx != other.gemm_ctx
    cut, mm = torch.rand(2, 3, R, R), torch.tensor([0.0, 1.0])
    emb, acc, gc = torch.empty(2, h.cfg.output_dim), torch.empty(4, dtype=torch.float64), torch.empty(2, 3, R, R)
    # a backward before any forward
    for fn, args in (("_backward_reduce", (cut, mm, emb, acc)), ("_backward_finish", (cut, mm, acc, gc))):
        with pytest.raises(PrxError, match=rf"\): {word} backward: no forward in flight on this handle"):
            call(h.abi + fn, h.h, *args, 0)
    # one cutout more than the handle was made for: the min / max pass, the forward itself, and the Python entry
    with pytest.raises(PrxError, match=rf"_minmax failed \(rc=-2\): {word}: batch 2 exceeds handle capacity 1"):
        call(h.abi + "_minmax", h.h, cut, 2, mm, 0)
    with pytest.raises(PrxError, match=rf"_encode failed \(rc=-2\): {word}: batch 2 exceeds handle capacity 1"):
        call(h.abi + "_encode", h.h, cut, 2, mm, emb, 0)
    with pytest.raises(PrxError, match=rf"\): {word}: batch 2 exceeds handle capacity 1"):
        ops.clip_encode_image(cut, h)
    # a refused forward is not a forward in flight
    with pytest.raises(PrxError, match="no forward in flight"):
        call(h.abi + "_backward_reduce", h.h, cut, mm, emb, acc, 0)
    c1 = cut[:1].clone().requires_grad_(True)
    e = ops.clip_encode_image(c1, h)
    e.backward(torch.ones_like(e) * 1e-3)
    assert h.generation == 1 and bool(torch.isfinite(e).all()) and bool(torch.isfinite(c1.grad).all())
