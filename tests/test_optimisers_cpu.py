"""`--optimiser` without a GPU: the front end and `engine.Session` honour the option on the host (`fast_pixel` drawer, CPU
stand-ins as in tests/test_frontend.py), and the fused kernels of csrc/optim.hip run on the CPU emulation (tools/hipemu) through
the bodies of tests/test_optimisers_gpu.py."""
import os
import shutil
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _emu  # noqa: E402
import test_optimisers_gpu as tg  # noqa: E402
from test_frontend import _factories, _settings  # noqa: E402
from pixray_amd import frontend as fe  # noqa: E402
from pixray_amd import optimisers  # noqa: E402

needs_emu = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") or shutil.which("make") is None,
                               reason="needs the ROCm host clang++ and make to build tools/hipemu")


# ------------------------------------------------------------------------------------------------ host: front end and session
def _session(tmp_path, **kw):
    run, s = _settings(tmp_path, **kw)
    return fe.do_init(s, run, **_factories(2))


@pytest.mark.parametrize("rule", ["AdamW", "Adagrad", "Adamax", "DiffGrad", "AdamP"])
def test_session_steps_with_the_rule_that_was_asked_for(tmp_path, rule):
    """three train() steps of a `fast_pixel` session against the rule itself (torch.optim, or the test's own restatement for
    DiffGrad / AdamP) driven by the gradients the session saw"""
    sess = _session(tmp_path, optimiser=rule)
    assert sess.optimiser == rule and type(sess.opts[0]) is optimisers._HOST[rule]
    z = sess.drawer.get_z()
    twin = z.detach().clone()
    ref = tg.make_ref(rule, twin, 0.05)
    moved = 0.0
    for it in range(3):
        before = z.detach().clone()
        assert sess.train(it)
        with torch.no_grad():
            ref.step(z.grad.clone())
            twin.clamp_(0, 1)                                   # the drawer's clip_z
        moved = max(moved, float((z.detach() - before).abs().max()))
        assert float((z.detach() - twin).abs().max()) <= 1e-6 * max(1.0, 0.05 * (it + 1)), (rule, it)
    assert moved > 1e-3


def test_adam_is_what_it_was_and_unknown_names_are_refused(tmp_path):
    sess = _session(tmp_path)
    assert sess.optimiser == "Adam" and type(sess.opts[0]) is torch.optim.Adam and sess.opts[0].param_groups[0]["lr"] == 0.05
    with pytest.raises(ValueError, match="Adam, AdamW, Adagrad, Adamax, DiffGrad, AdamP"):
        _session(tmp_path, optimiser="Nope")
    with pytest.raises(ValueError, match="Nope"):
        optimisers.make_optimiser("Nope", [torch.zeros(3)], 0.1)


def test_learning_rate_drop_keeps_the_rule(tmp_path):
    sess = _session(tmp_path, optimiser="Adamax", learning_rate_drops=["50"])
    (drop,) = sess.learning_rate_drops                  # 50% of the run: iteration 2, the rebuild follows that iteration's step
    first = sess.opts[0]
    for it in range(drop + 2):
        assert sess.train(it)
        assert (sess.opts[0] is first) == (it < drop)
    assert type(sess.opts[0]) is torch.optim.Adamax and sess.opts[0] is not first
    assert abs(sess.opts[0].param_groups[0]["lr"] - 0.005) < 1e-12
    assert int(sess.opts[0].state[sess.drawer.get_z()]["step"]) == 1        # fresh state at the drop, one step since


def test_optimiser_factory_still_wins(tmp_path):
    from pixray_amd.engine import Session
    sess = _session(tmp_path, optimiser="AdamW")
    made = []

    def factory(params, lr):
        made.append(lr)
        return torch.optim.SGD(params, lr=lr)
    again = Session(sess.drawer, sess.perceptors, sess.cutoutsTable, sess.pmsTable, learning_rate=0.05, optimiser="AdamW",
                    optimiser_factory=factory)
    assert type(again.opts[0]) is torch.optim.SGD and made == [0.05]


def test_host_restatements_match_the_tests_own():
    """pixray_amd.optimisers.DiffGrad / AdamP (host classes) against the restatements in tests/test_optimisers_gpu.py, both
    branches of AdamP included"""
    for rule, shape, fn in (("DiffGrad", (3, 5, 7), None), ("AdamP", (4, 6, 8, 10), tg.grad_orthogonal),
                            ("AdamP", (4, 6, 8, 10), tg.grad_layer_only), ("AdamP", (4, 6, 8, 10), tg.grad_aligned), ("AdamP", (33,), None)):
        g = torch.Generator().manual_seed(5)
        z0 = torch.randn(*shape, generator=g, dtype=torch.float64)
        p, twin = z0.clone().requires_grad_(True), z0.clone()
        opt, ref = optimisers._HOST[rule]([p], lr=0.3), tg.make_ref(rule, twin, 0.3)
        for t in range(5):
            grad = fn(t, twin) if fn is not None else torch.randn(*shape, generator=g, dtype=torch.float64)
            p.grad = grad.clone()
            opt.step()
            with torch.no_grad():
                ref.step(grad)
            assert float((p.detach() - twin).abs().max()) < 1e-12, (rule, shape, t)
        if fn is not None:
            assert {v for v, _ in ref.log} == {{"grad_orthogonal": 1, "grad_layer_only": 2, "grad_aligned": 0}[fn.__name__]}


# ------------------------------------------------------------------------------------------------ the kernels, emulated
@pytest.fixture(scope="module")
def emu():
    with _emu.enable() as lib:
        tg.DEV = "cpu"
        yield lib
        tg.DEV = "cuda"


@needs_emu
def test_emulated_library_exports_the_new_entry_points(emu):
    from pixray_amd import _lib
    assert emu.prx_abi_version() == 3
    for name in ("prx_optim_step_dev", "prx_optim_adamp_scratch_floats", "prx_optim_adamp_step_dev"):
        assert name in _lib._protos and hasattr(emu, name)


@needs_emu
@pytest.mark.parametrize("with_bounds", [True, False], ids=["bounds", "free"])
@pytest.mark.parametrize("shape_name", list(tg.SHAPES))
@pytest.mark.parametrize("rule", list(tg.LR))
def test_rule_against_float64(emu, rule, shape_name, with_bounds):
    tg.check_rule_against_float64(rule, shape_name, with_bounds)


@needs_emu
def test_adamp_branches(emu):
    tg.check_adamp_branches()


@needs_emu
def test_adamp_same_bits_in_any_workgroup_order(emu):
    """the partial sums are added in a fixed order: running the workgroups (and the waves of each) last-to-first gives the same bits"""
    z0, _, bounds = tg.seeded_case("rows4", False, seed=11)
    _, used = tg.run_ref("AdamP", z0, tg.grad_layer_only, bounds, torch.float64, 2.0)
    z1, s1 = tg.run_kernel("AdamP", z0, used, bounds, 2.0)
    emu.hipemu_set_reverse_order(1)
    try:
        z2, s2 = tg.run_kernel("AdamP", z0, used, bounds, 2.0)
    finally:
        emu.hipemu_set_reverse_order(0)
    assert torch.equal(z1, z2) and all(torch.equal(s1[k], s2[k]) for k in s1)
    tg.check_adamp_bit_reproducible()


@needs_emu
def test_kernel_refuses_what_it_cannot_do(emu):
    from pixray_amd import _lib, ops
    z = torch.zeros(2, 3, 4, 5)
    hyper = torch.zeros(4)
    with pytest.raises(_lib.PrxError, match="state tensors"):
        ops.optim_step_dev("DiffGrad", z, [torch.zeros_like(z)], torch.zeros_like(z), None, None, hyper)
    with pytest.raises(AssertionError):
        ops.optim_step_dev("AdamW", z, [torch.zeros_like(z)] * 2, torch.zeros_like(z), torch.zeros(4), torch.zeros(4), hyper)
    with pytest.raises(_lib.PrxError, match="scratch"):
        ops.adamp_step_dev(z, torch.zeros_like(z), torch.zeros_like(z), torch.zeros_like(z), None, None, hyper, torch.zeros(4))
