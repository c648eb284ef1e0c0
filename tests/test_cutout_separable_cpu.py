"""tests/test_cutout_separable_gpu.py on the emulated kernels (tools/hipemu: the product's HIP sources compiled for the host): the
separable tile path of the warp backward's form 0 and its switch, every case of that file at the same shapes.  Bit for bit here too:
setting 1 against form 2, settings 0 and 1 against each other where the path must not run, and setting 2 (the default) against the
frozen restatement of the scatter's order (scatter_order_frozen) -- which is what shows that the path ran at the default and summed in
the documented order.  NOT bit for bit here: setting 2 against setting 0.  The emulation runs the lanes of a wave one after another
between synchronisation points, so the emulated scatter adds in another order than a wave in lockstep; that comparison is held to
rel-L2 1e-5 here and to bits on the device."""
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


def test_separable_cutout_backward_on_the_emulated_kernels():
    with _emu.enable():
        import test_kernels_half_gpu as th
        import test_kernels_runner_gpu as tr
        import test_kernels_cutouts_gpu as tc
        import test_cutout_separable_gpu as tsep
        mods = (th, tr, tc)
        saved = [m.DEV for m in mods]
        for m in mods:
            m.DEV = "cpu"
        try:
            tsep.emu_subset()
        finally:
            for m, d in zip(mods, saved):
                m.DEV = d
