"""tests/test_cutout_passes_gpu.py on the emulated kernels (tools/hipemu: the product's HIP sources compiled for the host): the
merged pre-passes, the forward warps on their (plane, cutout) grid, both forms of the renormalisation backward and the refusals,
every check of that file at the same shapes -- the frozen-arithmetic comparisons are bit for bit here too, since the emulation
runs the same IEEE operations in the same order."""
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


def test_cutout_passes_on_the_emulated_kernels():
    with _emu.enable():
        import test_kernels_half_gpu as th
        import test_kernels_runner_gpu as tr
        import test_kernels_cutouts_gpu as tc
        import test_cutout_passes_gpu as tpass
        mods = (th, tr, tc)
        saved = [m.DEV for m in mods]
        for m in mods:
            m.DEV = "cpu"
        try:
            tpass.emu_subset()
        finally:
            for m, d in zip(mods, saved):
                m.DEV = d
