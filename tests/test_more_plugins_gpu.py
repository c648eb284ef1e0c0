"""The aesthetic, image / mask edge and gaussian losses (pixray_amd/builtin_losses.py on the kernels of csrc/plugin_losses.hip)
against what pixray's own classes compute (tests/golden/more_plugins_golden.npz, written by
tests/golden/make_golden_more_plugins.py), and the aesthetic kernel against float64 torch.
tests/test_more_plugins_cpu.py runs the `check_*` functions on the emulated kernels with DEV = "cpu"."""
import os
import sys
import tempfile
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "golden"))

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(HERE, "golden", "more_plugins_golden.npz")
LOSS_RTOL, GRAD_RTOL = 1e-5, 1e-4
_GOLD = None


def gold():
    global _GOLD
    if _GOLD is None:
        with np.load(GOLD) as g:
            _GOLD = {k: g[k] for k in g.files}
    return _GOLD


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _loss_grad(fn, x):
    x = x.clone().requires_grad_(True)
    loss = fn(x)
    loss.backward()
    return loss.detach(), x.grad


def _assert_close(name, loss, grad, ref_l, ref_g):
    ref_l = float(ref_l)
    print(name, "loss", float(loss), "ref", ref_l, "grad rel", _rel(grad, ref_g))
    assert abs(float(loss) - ref_l) <= LOSS_RTOL * abs(ref_l), (name, float(loss), ref_l)
    assert _rel(grad, ref_g) <= GRAD_RTOL, (name, _rel(grad, ref_g))


def _sources(directory):
    from make_golden_more_plugins import write_sources
    g = gold()
    return write_sources(g["in/edge_picture"], g["in/edge_mask"], directory)


def _head_file(directory, d=None):
    """the fixture's head (or a seeded d-wide one) as an --aesthetic_model file"""
    from make_golden_more_plugins import aesthetic_head
    g = gold()
    sd = {"weight": torch.from_numpy(g["aes/weight"]), "bias": torch.from_numpy(g["aes/bias"])} if d is None else aesthetic_head(d=d)
    path = os.path.join(str(directory), "head.pth")
    torch.save(sd, path)
    return path


def edge_objects(directory):
    """(name, EdgeLoss instance, args, input) for every edge case of the fixture"""
    from make_golden_more_plugins import EDGE_CASES, edge_args
    from pixray_amd.builtin_losses import EdgeLoss
    pic, mask = _sources(directory)
    g = gold()
    out = []
    for case in EDGE_CASES:
        obj = EdgeLoss(device=DEV)
        a = obj.parse_settings(edge_args(case, pic, mask))
        out.append((f"edge/{case}", obj, a, _t(g["in/image2" if EDGE_CASES[case][7] == 2 else "in/image"])))
    return out


def gauss_objects():
    from make_golden_more_plugins import GAUSS_CASES, gauss_args
    from pixray_amd.builtin_losses import GaussianLoss
    g = gold()
    return [(f"gauss/{case}", GaussianLoss(device=DEV), gauss_args(case), _t(g[f"in/{GAUSS_CASES[case][3]}"])) for case in GAUSS_CASES]


def aesthetic_objects(directory):
    """(name, AestheticLoss instance, args, embeddings) for every aesthetic case of the fixture"""
    from make_golden_more_plugins import AES_CASES
    from pixray_amd.builtin_losses import AestheticLoss
    g = gold()
    path = _head_file(directory)
    out = []
    for case, (n, target) in AES_CASES.items():
        obj = AestheticLoss(device=DEV)
        a = obj.parse_settings(types.SimpleNamespace(aesthetic_model=path, aesthetic_target=target, num_cuts=n))
        out.append((f"aes/{case}", obj, a, _t(g[f"aes/{case}/embeds"])))
    return out


def _image_score(obj, args):
    return lambda t: obj.get_loss({}, t, args)


def _embed_score(obj, args):
    return lambda t: obj.get_loss({}, None, args, globals={"embeds": t})


def check_edge_matches_reference():
    g = gold()
    with tempfile.TemporaryDirectory() as tmp:
        for name, obj, args, x in edge_objects(tmp):
            loss, grad = _loss_grad(_image_score(obj, args), x)
            _assert_close(name, loss, grad, g[f"{name}/loss"], g[f"{name}/grad"])


def check_edge_refits_on_a_new_canvas():
    """the resized picture and mask follow the canvas: a second size after the first scores against ITS resize"""
    from pixray_amd import ops
    from pixray_amd.builtin_losses import EdgeLoss
    from make_golden_more_plugins import edge_args
    g = gold()
    with tempfile.TemporaryDirectory() as tmp:
        pic, mask = _sources(tmp)
        obj = EdgeLoss(device=DEV)
        a = obj.parse_settings(edge_args("img_mask", pic, mask))
        x = _t(g["in/image"])
        first = obj.get_loss({}, x, a)
        small = x[:, :, :24, :30].contiguous()
        got = obj.get_loss({}, small, a)
        tgt = F.interpolate(obj.image, (24, 30), mode="bicubic", align_corners=False).to(DEV)
        msk = F.interpolate(obj.mask, (24, 30), mode="bicubic", align_corners=False).to(DEV)
        want = ops.edge_target_loss(small, tgt, a.edge_color, msk, (0, 0, 0, 0), a.edge_color_weight, a.global_color_weight)
        assert torch.equal(got, want) and torch.equal(obj.get_loss({}, x, a), first)


def check_gaussian_matches_reference():
    from make_golden_more_plugins import GREEN_BLOCK
    g = gold()
    for name, obj, args, x in gauss_objects():
        loss, grad = _loss_grad(_image_score(obj, args), x)
        _assert_close(name, loss, grad, g[f"{name}/loss"], g[f"{name}/grad"])
        if name.endswith("green_block"):        # |out - colour| sits on its kink there: the zero subgradient, as torch.abs
            block = grad[0, 1][GREEN_BLOCK]
            assert block.numel() == 180 and bool((block == 0).all())
            assert bool((torch.from_numpy(g[f"{name}/grad"])[0, 1][GREEN_BLOCK] == 0).all())
            assert bool((grad[0, 0] != 0).any()) and bool((grad[0, 1, :10] != 0).all())


def check_aesthetic_matches_reference():
    g = gold()
    with tempfile.TemporaryDirectory() as tmp:
        for name, obj, args, e in aesthetic_objects(tmp):
            loss, grad = _loss_grad(_embed_score(obj, args), e)
            _assert_close(name, loss, grad, g[f"{name}/loss"], g[f"{name}/grad"])


def _aesthetic_f64(e, w, b, target):
    e = e.detach().double().cpu().requires_grad_(True)
    loss = (F.linear(F.normalize(e, dim=-1), w.double().cpu().reshape(1, -1), torch.tensor([b], dtype=torch.float64)) - target).square().mean() * 0.02
    loss.backward()
    return loss.detach(), e.grad


def check_aesthetic_matches_float64():
    """d = 80 (a lane tail: 64 + 16) on 9 rows (three workgroups, the last with one row), and a batch with an all-zero row"""
    from pixray_amd import ops
    gen = torch.Generator().manual_seed(31)
    w = (torch.randn(80, generator=gen) * 0.3).to(DEV)
    e = torch.randn(9, 80, generator=gen).to(DEV)
    loss, grad = _loss_grad(lambda t: ops.aesthetic_loss(t, w, 5.0, 10.0), e)
    ref_l, ref_g = _aesthetic_f64(e, w, 5.0, 10.0)
    _assert_close("aes/f64_d80", loss, grad, ref_l, ref_g)
    # a zero row: F.normalize divides by its eps there, the rating is the bias, and the gradient is w * 1e12 * (0.04 / n) * diff
    n, target, bias = 3, 10.0, 5.0
    e = torch.randn(n, 80, generator=gen)
    e[1] = 0
    e = e.to(DEV)
    loss, grad = _loss_grad(lambda t: ops.aesthetic_loss(t, w, bias, target), e)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    ref_l, ref_g = _aesthetic_f64(e, w, bias, target)
    assert abs(float(loss) - float(ref_l)) <= LOSS_RTOL * abs(float(ref_l)), (float(loss), float(ref_l))
    want = w.double().cpu() * 1e12 * (0.04 / n) * (bias - target)
    assert _rel(grad[1], want) <= GRAD_RTOL, _rel(grad[1], want)
    assert _rel(grad[1], ref_g[1]) <= GRAD_RTOL and _rel(grad[[0, 2]], ref_g[[0, 2]]) <= GRAD_RTOL


def _all_outputs():
    """every new kernel's outputs on the fixture inputs (for the repeatability checks)"""
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, obj, args, x in edge_objects(tmp) + gauss_objects():
            res += list(_loss_grad(_image_score(obj, args), x))
        for name, obj, args, e in aesthetic_objects(tmp):
            res += list(_loss_grad(_embed_score(obj, args), e))
    return res


def check_bit_identical_runs():
    a, b = _all_outputs(), _all_outputs()
    assert len(a) == len(b) == 22 and all(torch.equal(u, v) for u, v in zip(a, b))


def check_sharding(world=2):
    """AestheticLoss under the scoring of test_builtin_plugins_gpu.check_shards_reproduce_full_batch (every rank scores the
    gathered batch, differentiable through its own shard, at the full weight) reproduces the unsharded value and gradient;
    scored per shard it would not.  Edge and gaussian read the replicated image: not batch-coupled."""
    from pixray_amd.builtin_losses import EdgeLoss, GaussianLoss
    from pixray_amd.engine import needs_full_batch
    assert not needs_full_batch(EdgeLoss(device=DEV)) and not needs_full_batch(GaussianLoss(device=DEV))
    with tempfile.TemporaryDirectory() as tmp:
        name, obj, args, e = aesthetic_objects(tmp)[0]
    assert needs_full_batch(obj) and e.shape[0] == 5
    score = _embed_score(obj, args)
    full_l, full_g = _loss_grad(score, e)
    shards = list(e.chunk(world))
    grad, vals = torch.zeros_like(e), []
    for r in range(world):
        own = shards[r].clone().requires_grad_(True)
        l = score(torch.cat([own if i == r else shards[i] for i in range(world)]))
        l.backward()
        vals.append(l.detach())
        lo = sum(s.shape[0] for s in shards[:r])
        grad[lo:lo + own.shape[0]] += own.grad
    assert abs(float(vals[0]) - float(full_l)) <= 1e-6 * abs(float(full_l)), (float(vals[0]), float(full_l))
    assert _rel(grad, full_g) <= 1e-6, _rel(grad, full_g)
    per_shard = sum(float(score(s)) for s in shards) / world
    assert abs(per_shard - float(full_l)) > 1e-4 * abs(float(full_l)), (per_shard, float(full_l))


def check_plugin_tables_build():
    from pixray_amd import frontend, plugins
    from pixray_amd.builtin_losses import GaussianLoss
    with tempfile.TemporaryDirectory() as tmp:
        pic, mask = _sources(tmp)
        args = types.SimpleNamespace(aesthetic_model=_head_file(tmp), aesthetic_target=10, edge_thickness=5, edge_margins=None,
                                     edge_color="white", edge_color_weight=0.1, global_color_weight=0.05, edge_input_image=pic,
                                     edge_mask_image=mask, gaussian_weight=1, gaussian_std=(40, 40), gaussian_color=(255, 255, 255))
        losses, _, args = plugins.setup_custom_losses("aesthetic:0.5,edge", args, device=DEV)
        assert [type(t["loss"]).__name__ for t in losses] == ["AestheticLoss", "EdgeLoss"] and [t["weight"] for t in losses] == [0.5, 1]
        assert all(t["loss"].supports_graph_replay for t in losses)
        assert losses[0]["loss"].weight.shape == (512,) and losses[1]["loss"].image.shape == (1, 3, 14, 20) \
            and losses[1]["loss"].mask.shape == (1, 1, 14, 20)
        assert "gaussian" not in plugins.loss_class_table
        try:
            frontend.add_custom_loss("gaussian", GaussianLoss)
            more, _, _ = plugins.setup_custom_losses("gaussian", args, device=DEV)
            assert type(more[0]["loss"]) is GaussianLoss and more[0]["loss"].supports_graph_replay
        finally:
            plugins.loss_class_table.pop("gaussian", None)


# ------------------------------------------------------------------------------------------------ GPU tests
def test_edge_with_image_and_mask_matches_reference():
    check_edge_matches_reference()


def test_edge_refits_on_a_new_canvas():
    check_edge_refits_on_a_new_canvas()


def test_gaussian_matches_reference():
    check_gaussian_matches_reference()


def test_aesthetic_matches_reference():
    check_aesthetic_matches_reference()


def test_aesthetic_matches_float64():
    check_aesthetic_matches_float64()


def test_two_runs_bit_identical():
    check_bit_identical_runs()


def test_aesthetic_needs_the_full_batch_under_sharding():
    check_sharding()


def test_plugin_table_builds_the_new_losses():
    check_plugin_tables_build()


def test_frontend_run_with_the_new_losses(tmp_path):
    from pixray_amd import frontend as fe, plugins
    from pixray_amd.builtin_losses import GaussianLoss
    pic, mask = _sources(tmp_path)
    head = _head_file(tmp_path, d=128)           # tiny-B/32 embeds 128 wide
    try:
        fe.add_custom_loss("gaussian", GaussianLoss)
        run = fe.Run()
        run.settings = dict(drawer="vqgan", vqgan_model="tiny_f4", clip_models="tiny-B/32", size=[64, 64], num_cuts=8, iterations=5,
                            save_every=5, display_every=5, outdir=str(tmp_path / "out"), seed=3, skip_args=True, init_noise="none",
                            vector_prompts="none", noise_prompt_seeds=[1], noise_prompt_weights=[1.0], learning_rate_drops=[],
                            custom_loss="aesthetic,edge,gaussian", edge_input_image=pic, edge_mask_image=mask, aesthetic_model=head)
        s = fe.apply_settings(run=run)
        sess = fe.do_init(s, run)
        assert [type(t["loss"]).__name__ for t in sess.custom_losses] == ["AestheticLoss", "EdgeLoss", "GaussianLoss"]
        z0 = sess.drawer.get_z_copy()
        while not fe.do_run(s, run=run):
            pass
    finally:
        plugins.loss_class_table.pop("gaussian", None)
    z = sess.drawer.get_z()
    assert sess.cur_iteration == 5 and torch.isfinite(z).all()
    assert float((z.detach() - z0).abs().max()) > 1e-3
    assert all(torch.isfinite(l).all() for l in sess.last_losses)


def test_graph_replay_with_the_new_losses(tmp_path):
    """a replayed session with the three losses: every iteration is the eager one (teacher-forced, with the criterion of
    tests/test_builtin_plugins_gpu.py::test_graph_replay_with_tiler_and_saturation)"""
    from make_golden_more_plugins import edge_args
    from pixray_amd import api
    from pixray_amd.builtin_losses import AestheticLoss, EdgeLoss, GaussianLoss
    pic, mask = _sources(tmp_path)
    head = _head_file(tmp_path, d=128)
    args = edge_args("img_mask", pic, mask)
    args.__dict__.update(aesthetic_model=head, aesthetic_target=10.0, gaussian_weight=1.0, gaussian_std=(12.0, 12.0),
                         gaussian_color=(255.0, 128.0, 0.0))

    def build():
        losses = [AestheticLoss(device="cuda"), EdgeLoss(device="cuda"), GaussianLoss(device="cuda")]
        a = args
        for l in losses:
            a = l.parse_settings(a)
        return api.build_vqgan_clip_session(size=(64, 64), vqgan_model="tiny_f4", clip_model="tiny-B/32", num_cuts=8, seed=3,
                                            custom_losses=[{"loss": l, "weight": 1.0} for l in losses])
    a, b = build(), build()
    a.args = b.args = args
    for mk in list(a.cutoutsTable.values()) + list(b.cutoutsTable.values()):
        mk.noise_fac = 0.0
    torch.manual_seed(77)
    for it in range(3):
        a.train(it)
    torch.manual_seed(77)
    assert b.enable_graph(warmup=2), getattr(b, "graph_error", None)
    b.train(2)
    assert b._graph is not None
    za, zb = a.drawer.get_z(), b.drawer.get_z()
    oa, ob = a.opts[0], b.opts[0]
    for it in range(3, 7):
        with torch.no_grad():
            zb.copy_(za)
            for k in ("exp_avg", "exp_avg_sq"):
                ob.state[zb][k].copy_(oa.state[za][k])
        torch.manual_seed(1000 + it)
        a.train(it)
        torch.manual_seed(1000 + it)
        b.train(it)
        d = (za.detach() - zb.detach()).abs()
        assert (d > 1e-3).float().mean().item() < 2e-2, (it, d.max().item())
    assert b._graph is not None
    assert len(a.last_losses) >= 4 and all(torch.isfinite(l).all() for l in a.last_losses)
