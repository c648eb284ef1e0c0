"""prx_k_gemm_group (csrc/gemm.hip prx_gemm_launch_group): n products that differ only in A, B and their output pointers, as ONE
launch of the direct-to-LDS tiled kernel whose grid z dimension is the member -- or, where the plan is anything else, n ordinary
launches.  Either way the bytes must be those of n separate prx_k_gemm calls: the grouped kernel runs the ordinary kernel's body
per member, so the comparison is byte-for-byte and needs no tolerance.  The members write disjoint column slices of one
[M, 3N] buffer (the decoder attention's dq | dk | dv layout); the buffer is pre-filled with a sentinel, so what the separate calls
leave alone must be left alone."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from pixray_amd import _lib
from pixray_amd._lib import GemmArgs, call

DEV = "cuda"

PRECS = {"fp16": (_lib.PREC_F16, torch.float16), "bf16": (_lib.PREC_BF16, torch.bfloat16), "f32": (_lib.PREC_F32, torch.float32)}
# (M, N, K, grouped in the 16-bit modes): 35 tokens with pitch 40 (a partial row tile, K no multiple of the 64-wide K tile); the
# headline dq / dk / dv product; and a shape the planner gives to a fit tile, which the group entry must run as separate launches
SHAPES = [(35, 128, 40, True), (256, 512, 256, True), (256, 512, 512, False)]


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _sentinel(shape, dtype):
    n = 1
    for s in shape:
        n *= s
    return torch.full((n * torch.empty((), dtype=dtype).element_size(),), 0x5A, dtype=torch.uint8, device=DEV).view(dtype).view(*shape)


def _members(n, As, Bs, M, N, K, code, out16, out32):
    """n descriptors over the given output buffers ([M, 3N]; member i owns columns [i N, (i + 1) N))"""
    arr = (GemmArgs * n)()
    for i in range(n):
        g = arr[i]
        g.A = As[i].data_ptr(); g.a_is_f32 = 0; g.a_mode = 0; g.lda = K
        g.B = Bs[i].data_ptr(); g.ldb = K
        g.M, g.N, g.K = M, N, K
        g.alpha = 1.0
        esz = out16.element_size() if out16 is not None else 0
        g.out_bf16 = out16.data_ptr() + i * N * esz if out16 is not None else None
        g.ldc_bf16 = 3 * N
        g.out_f32 = out32.data_ptr() + i * N * 4 if out32 is not None else None
        g.ldc_f32 = 3 * N
        g.f32 = code
        g.ctx = _lib.tool_ctx()
    return arr


@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("M,N,K,grouped", SHAPES)
@pytest.mark.parametrize("n", [1, 2, 3])
def test_gemm_group_leaves_the_bytes_of_separate_launches(prec, M, N, K, grouped, n):
    code, dt = PRECS[prec]
    lib = _lib.load()
    torch.manual_seed(M + N + K + n)
    As = [(torch.randn(M, K, device=DEV) * (1 + i)).to(dt) for i in range(3)]
    Bs = [(torch.randn(N, K, device=DEV) / K ** 0.5).to(dt) for i in range(3)]
    ws = torch.empty(8 << 20, dtype=torch.uint8, device=DEV)
    f32 = code == _lib.PREC_F32
    res = []
    for group in (False, True):
        out16 = None if f32 else _sentinel((M, 3 * N), dt)
        out32 = _sentinel((M, 3 * N), torch.float32)
        arr = _members(n, As, Bs, M, N, K, code, out16, out32)
        n0 = lib.prx_gemm_group_launches()
        if group:
            call("prx_k_gemm_group", ctypes.addressof(arr), n, ws, ws.numel(), _lib.current_stream())
        else:
            for i in range(n):
                call("prx_k_gemm", arr[i], ws, ws.numel(), _lib.current_stream())
        torch.cuda.synchronize()
        dn = lib.prx_gemm_group_launches() - n0
        # the exact mode plans onto the fp32 4-wave kernels, which have no grouped form: separate launches, like the fit shape
        assert dn == (1 if group and grouped and not f32 else 0), (prec, M, N, K, n, group, dn)
        res.append((out16, out32))
    for a, b in zip(res[0], res[1]):
        if a is not None:
            assert torch.equal(_bytes(a), _bytes(b)), (prec, M, N, K, n)
    o32 = res[1][1]
    if n < 3:
        assert bool((_bytes(o32[:, n * N:]) == 0x5A).all())
    ref = As[n - 1].double() @ Bs[n - 1].double().t()       # ... and the bytes are a product, not two equal mistakes
    got = o32[:, (n - 1) * N:n * N].double()
    assert ((got - ref).norm() / ref.norm()).item() < 1e-5


def test_gemm_group_refuses_more_members_than_the_kernel_takes_and_mismatched_members_run_separately():
    lib = _lib.load()
    code, dt = PRECS["fp16"]
    M, N, K = 35, 128, 40
    torch.manual_seed(0)
    As = [torch.randn(M, K, device=DEV).to(dt) for i in range(3)]
    Bs = [torch.randn(N, K, device=DEV).to(dt) for i in range(3)]
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    out32 = _sentinel((M, 3 * N), torch.float32)
    arr = (GemmArgs * 5)()
    with pytest.raises(_lib.PrxError):
        call("prx_k_gemm_group", ctypes.addressof(arr), 5, ws, ws.numel(), _lib.current_stream())
    # members that disagree in a shared field (alpha): n ordinary launches, each with its own descriptor
    res = []
    for group in (False, True):
        out32 = _sentinel((M, 3 * N), torch.float32)
        arr = _members(3, As, Bs, M, N, K, code, None, out32)
        arr[1].alpha = 0.5
        n0 = lib.prx_gemm_group_launches()
        if group:
            call("prx_k_gemm_group", ctypes.addressof(arr), 3, ws, ws.numel(), _lib.current_stream())
        else:
            for i in range(3):
                call("prx_k_gemm", arr[i], ws, ws.numel(), _lib.current_stream())
        torch.cuda.synchronize()
        assert lib.prx_gemm_group_launches() == n0
        res.append(out32)
    assert torch.equal(_bytes(res[0]), _bytes(res[1]))
