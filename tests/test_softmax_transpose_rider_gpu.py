"""The decoder attention's softmax launches with a transpose riding along (csrc/elementwise.hip softmax_rows_tr_kernel /
softmax_rows_bwd_tr_kernel): one launch must leave exactly the bytes that the softmax launch followed by the stand-alone
transpose launch leave -- every output buffer is pre-filled with a sentinel, so pad columns and anything else the separate
launches do not write must come out untouched as well.  Comparisons are byte-for-byte: both forms run the same device code per
element, there is no tolerance to choose."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from pixray_amd import _lib
from pixray_amd._lib import call

DEV = "cuda"

PRECS = {"fp16": (_lib.PREC_F16, torch.float16), "bf16": (_lib.PREC_BF16, torch.bfloat16), "f32": (_lib.PREC_F32, torch.float32)}
# (tokens, pitch of the [*, tokens] operands, columns of the matrix that is transposed): 35 tokens in pitch 40 with q|k|v of a
# C = 128 block (ragged against the 4-row softmax blocks and the 32 x 32 transpose tiles), and the headline block's 256 / 3 x 512
SHAPES = [(35, 40, 384), (256, 256, 1536)]


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _sentinel(shape, dtype):
    n = 1
    for s in shape:
        n *= s
    return torch.full((n * torch.empty((), dtype=dtype).element_size(),), 0x5A, dtype=torch.uint8, device=DEV).view(dtype).view(*shape)


@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("P,P8,TC", SHAPES)
def test_softmax_rows_with_a_transpose_rider_leaves_the_bytes_of_the_two_launches(prec, P, P8, TC):
    code, dt = PRECS[prec]
    torch.manual_seed(P + TC)
    S = torch.randn(P, P, device=DEV) * 3
    X = torch.randn(P, TC, device=DEV).to(dt)                    # [tokens, 3C] -> X^T [3C, P8]
    scale = 1.0 / (TC / 3) ** 0.5
    outs = []
    for fused in (False, True):
        Pm, PT, XT = _sentinel((P, P8), dt), _sentinel((P, P8), dt), _sentinel((TC, P8), dt)
        if fused:
            call("prx_k_softmax_rows_tr_op", S, P, scale, Pm, P8, PT, P8, P, P, X, TC, XT, P8, P, TC, code, _lib.current_stream())
        else:
            call("prx_k_softmax_rows_op", S, P, scale, Pm, P8, PT, P8, P, P, code, _lib.current_stream())
            call("prx_k_transpose_op", X, TC, XT, P8, P, TC, int(code == _lib.PREC_F32), _lib.current_stream())
        torch.cuda.synchronize()
        outs.append((Pm, PT, XT))
    for a, b, name in zip(outs[0], outs[1], ("P", "P^T", "X^T")):
        assert torch.equal(_bytes(a), _bytes(b)), (name, prec, P, TC)
    # the separate launches did something: X^T holds X, the pad columns hold the sentinel
    assert torch.equal(_bytes(outs[1][2][:, :P]), _bytes(X.t()))
    if P8 != P:
        assert bool((_bytes(outs[1][2][:, P:]) == 0x5A).all()) and bool((_bytes(outs[1][0][:, P:]) == 0x5A).all())
    # P^T without a second output: the rider still runs
    Pm, XT = _sentinel((P, P8), dt), _sentinel((TC, P8), dt)
    call("prx_k_softmax_rows_tr_op", S, P, scale, Pm, P8, None, 0, P, P, X, TC, XT, P8, P, TC, code, _lib.current_stream())
    torch.cuda.synchronize()
    assert torch.equal(_bytes(Pm), _bytes(outs[0][0])) and torch.equal(_bytes(XT), _bytes(outs[0][2]))


@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("P,P8,TC", SHAPES)
def test_softmax_rows_bwd_with_a_transpose_rider_leaves_the_bytes_of_the_two_launches(prec, P, P8, TC):
    code, dt = PRECS[prec]
    torch.manual_seed(2 * P + TC)
    Pm = torch.zeros(P, P8, device=DEV, dtype=dt)
    Pm[:, :P] = torch.softmax(torch.randn(P, P, device=DEV) * 2, dim=1).to(dt)
    dP = torch.randn(P, P, device=DEV)
    X = torch.randn(P, TC, device=DEV).to(dt)
    scale = 1.0 / (TC / 3) ** 0.5
    outs = []
    for fused in (False, True):
        dS, dST, XT = _sentinel((P, P8), dt), _sentinel((P, P8), dt), _sentinel((TC, P8), dt)
        if fused:
            call("prx_k_softmax_rows_bwd_tr_op", Pm, P8, dP, P, scale, dS, P8, dST, P8, P, P, X, TC, XT, P8, P, TC, code, _lib.current_stream())
        else:
            call("prx_k_softmax_rows_bwd_op", Pm, P8, dP, P, scale, dS, P8, dST, P8, P, P, code, _lib.current_stream())
            call("prx_k_transpose_op", X, TC, XT, P8, P, TC, int(code == _lib.PREC_F32), _lib.current_stream())
        torch.cuda.synchronize()
        outs.append((dS, dST, XT))
    for a, b, name in zip(outs[0], outs[1], ("dS", "dS^T", "X^T")):
        assert torch.equal(_bytes(a), _bytes(b)), (name, prec, P, TC)
    assert torch.equal(_bytes(outs[1][2][:, :P]), _bytes(X.t()))
    if P8 != P:
        assert bool((_bytes(outs[1][2][:, P:]) == 0x5A).all()) and bool((_bytes(outs[1][1][:, P:]) == 0x5A).all())
