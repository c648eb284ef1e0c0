"""The attention dispatcher's routing table (csrc/attention.hip mha_plan, through prx_mha_describe: host only, nothing is launched),
row by row at the boundary shapes: which kernel family takes a (precision, head dim, T, causal, form, route), the operand columns per
head, whether `out` + `lse` are saved -- and what is refused, with the texts the GPU refusal tests match."""
import ctypes
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

BF16, F32, F16 = 0, 1, 2
WAVE, BLK, TILE, EXACT = 1, 2, 3, 4
TS = (1, 64, 65, 640, 641)
ROUTES = (-1, 0, 1)          # the rule, the workgroup family wherever able, the tile kernels
COLS = {64: 64, 80: 96, 88: 96, 104: 128}


@pytest.fixture(scope="module")
def describe():
    with _emu.enable():
        from pixray_amd import _lib

        def fn(prec, hd, T, causal=0, recompute=0, route=-1):
            """(family, cols, saves_out), or the refusal's text"""
            o = (ctypes.c_int * 3)(-1, -1, -1)
            a = ctypes.addressof(o)
            try:
                _lib.call("prx_mha_describe", prec, hd, T, causal, recompute, route, a, a + 4, a + 8)
            except _lib.PrxError as e:
                assert o[0] == 0
                return str(e)
            return o[0], o[1], o[2]
        lib = _lib.load()
        lib.prx_mha_route(-1)
        yield fn
        assert lib.prx_mha_route(-1) == -1, "prx_mha_describe takes the route as an argument: the process setting stays"


@pytest.mark.parametrize("prec", [BF16, F16])
def test_recomputing_form_is_the_wave_kernels_up_to_64_tokens(describe, prec):
    for route in ROUTES:
        for T in TS:
            got = describe(prec, 64, T, recompute=1, route=route)
            if T <= 64:
                assert got == (WAVE, 64, 0), (T, route, got)
            else:
                assert isinstance(got, str) and "T <= 64" in got, (T, route, got)


@pytest.mark.parametrize("prec", [BF16, F16])
def test_saving_form_at_64_columns_follows_the_route(describe, prec):
    for T in TS:
        want = {-1: BLK if T <= 640 else TILE, 0: BLK if T <= 640 else TILE, 1: TILE}
        for route in ROUTES:
            assert describe(prec, 64, T, route=route) == (want[route], 64, 1), (T, route)


@pytest.mark.parametrize("prec", [BF16, F16])
@pytest.mark.parametrize("hd", [80, 88, 104])
def test_padded_heads_have_the_workgroup_family_alone(describe, prec, hd):
    for route in ROUTES:
        for T in TS:
            got = describe(prec, hd, T, route=route)
            if T <= 640:
                assert got == (BLK, COLS[hd], 1), (T, route, got)
            else:
                assert isinstance(got, str) and "T <= 640" in got, (T, route, got)


@pytest.mark.parametrize("prec", [BF16, F16])
def test_causal_is_the_tile_forward_at_head_dim_64_only(describe, prec):
    for route in ROUTES:
        for T in TS:
            assert describe(prec, 64, T, causal=1, route=route) == (TILE, 64, 0), (T, route)
            for hd in (80, 88, 104):
                got = describe(prec, hd, T, causal=1, route=route)
                assert isinstance(got, str) and "head dim 64" in got, (hd, T, got)


@pytest.mark.parametrize("hd", [64, 80, 88, 104])
def test_fp32_is_the_exact_family_at_any_length(describe, hd):
    for route in ROUTES:
        for T in TS:
            assert describe(F32, hd, T, route=route) == (EXACT, COLS[hd], 1), (T, route)


@pytest.mark.parametrize("prec", [BF16, F32, F16])
@pytest.mark.parametrize("hd", [96, 112])
def test_head_dims_without_an_instance_are_refused_by_name(describe, prec, hd):
    for route in ROUTES:
        for T in TS:
            for recompute in (0, 1):
                got = describe(prec, hd, T, recompute=recompute, route=route)
                assert isinstance(got, str) and f"head dim {hd} at {hd} columns" in got and "columns per head" in got, (T, route, got)
