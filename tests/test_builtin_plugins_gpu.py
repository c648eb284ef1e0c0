"""The built-in custom losses and filters (pixray_amd/builtin_losses.py, builtin_filters.py on csrc/plugin_losses.hip,
plugin_filters.hip) against what pixray's own plugin code computes (tests/golden/builtin_plugins_golden.npz, written by
tests/golden/make_golden_plugins.py).  tests/test_builtin_plugins_cpu.py runs the `check_*` functions on the emulated kernels
with DEV = "cpu"."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "golden"))

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(HERE, "golden", "builtin_plugins_golden.npz")
LOSS_RTOL, GRAD_RTOL = 1e-5, 1e-4


def gold():
    return np.load(GOLD)


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _loss_grad(fn, x):
    x = x.clone().requires_grad_(True)
    loss = fn(x)
    if isinstance(loss, (list, tuple)):
        loss = loss[0]
    loss.backward()
    return loss.detach(), x.grad


def loss_objects(pal):
    """(name, plugin instance, args, reads) for every fixture case"""
    from make_golden_plugins import EDGE_CASES, SMOOTH_CASES
    from pixray_amd import builtin_losses as bl
    out = [("saturation", bl.SaturationLoss(device=DEV), types.SimpleNamespace(saturation_weight=1.3), "cutouts")]
    for name, (typ, sp, eo, gk, gs) in SMOOTH_CASES.items():
        a = types.SimpleNamespace(smoothness_weight=0.7, smoothness_type=typ, smoothness_spacing=sp, smoothness_edge_order=eo,
                                  smoothness_gaussian_kernel=gk, smoothness_gaussian_std=gs)
        out.append((f"smoothness_{name}", bl.SmoothnessLoss(device=DEV), a, "cutouts"))
    out.append(("palette", bl.PaletteLoss(device=DEV), types.SimpleNamespace(palette=pal, palette_weight=0.9), "cutouts"))
    out.append(("symmetry", bl.SymmetryLoss(device=DEV), types.SimpleNamespace(symmetry_weight=0.6), "image"))
    for case, (t, margins, colour, cw, gw) in EDGE_CASES.items():
        obj = bl.EdgeLoss(device=DEV)
        a = obj.parse_settings(types.SimpleNamespace(edge_thickness=t, edge_margins=margins, edge_color=colour, edge_color_weight=cw,
                                                     global_color_weight=gw, edge_input_image="", edge_mask_image=""))
        out.append((f"edge_{case}", obj, a, "image"))
    return out


def _score(obj, args, reads, x):
    if reads == "cutouts":
        return lambda t: obj.get_loss({8: t}, None, args)
    return lambda t: obj.get_loss({}, t, args)


def check_losses_small():
    g = gold()
    pal = g["in/palette"].tolist()
    for name, obj, args, reads in loss_objects(pal):
        x = _t(g["in/cutouts"] if reads == "cutouts" else g["in/image"])
        loss, grad = _loss_grad(_score(obj, args, reads, x), x)
        ref_l, ref_g = g[f"small/{name}/loss"], g[f"small/{name}/grad"]
        assert abs(float(loss) - float(ref_l)) <= LOSS_RTOL * abs(float(ref_l)), (name, float(loss), float(ref_l))
        assert _rel(grad, ref_g) <= GRAD_RTOL, (name, _rel(grad, ref_g))


def check_filters_small():
    from make_golden_plugins import WALL_CASES
    from pixray_amd import builtin_filters as bf
    g = gold()
    img = _t(g["in/filter_image"])
    for name, (typ, em) in WALL_CASES.items():
        f = bf.WallpaperFilter(types.SimpleNamespace(wallpaper_type=typ, wallpaper_edge_match=em), device=DEV)
        x = img.clone().requires_grad_(True)
        torch.manual_seed(int(g[f"wall/{name}/seed"]))
        o, loss = f(x)
        assert torch.equal(o.detach().cpu(), torch.from_numpy(g[f"wall/{name}/out"])), name      # a gather: exact
        ref_l = float(g[f"wall/{name}/loss"])
        assert abs(float(loss.detach()) - ref_l) <= LOSS_RTOL * abs(ref_l), (name, float(loss.detach()), ref_l)
        probe = torch.from_numpy(_probe(g, name, o.shape)).to(DEV)
        ((o * probe).sum() + 3 * loss).backward()
        assert _rel(x.grad, g[f"wall/{name}/grad"]) <= GRAD_RTOL, (name, _rel(x.grad, g[f"wall/{name}/grad"]))
    f = bf.TilerFilter(types.SimpleNamespace(), device=DEV)
    x = img.clone().requires_grad_(True)
    torch.manual_seed(150)
    o, loss = f(x)
    assert torch.equal(o.detach().cpu(), torch.from_numpy(g["tiler/out"])) and float(loss) == 0.0
    (o * torch.from_numpy(_probe_seed(250, o.shape)).to(DEV)).sum().backward()
    assert _rel(x.grad, g["tiler/grad"]) <= GRAD_RTOL
    pal = g["in/lookup_palette"].tolist()
    for c in (3, 4):
        f = bf.ColorLookup(types.SimpleNamespace(lookup_beta=2.5, palette=pal), device=DEV)
        x = _t(g[f"lookup{c}/in"]).requires_grad_(True)
        o, loss = f(x)
        assert torch.equal(o.detach().cpu(), torch.from_numpy(g[f"lookup{c}/out"])), c
        ref_l = float(g[f"lookup{c}/loss"])
        assert abs(float(loss) - ref_l) <= LOSS_RTOL * abs(ref_l), (c, float(loss), ref_l)
        ((o * torch.from_numpy(_probe_seed(310 + c, o.shape)).to(DEV)).sum() + 3 * loss).backward()
        assert _rel(x.grad, g[f"lookup{c}/grad"]) <= GRAD_RTOL, (c, _rel(x.grad, g[f"lookup{c}/grad"]))


def _probe_seed(seed, shape):
    return torch.rand(tuple(shape), generator=torch.Generator().manual_seed(seed)).numpy()


def _probe(g, name, shape):
    from make_golden_plugins import WALL_CASES
    return _probe_seed(200 + list(WALL_CASES).index(name), shape)


def check_palette_strings():
    from make_golden_plugins import PALETTE_STRINGS
    from pixray_amd.palette import palette_from_string
    g = gold()
    for i, s in enumerate(PALETTE_STRINGS):
        np.testing.assert_allclose(np.asarray(palette_from_string(s), dtype=np.float64), g[f"palette_str/{i}"], rtol=0, atol=1e-12, err_msg=s)


def _all_outputs():
    """every new kernel's outputs on the small fixture inputs (for the repeatability check)"""
    g = gold()
    res = []
    for name, obj, args, reads in loss_objects(g["in/palette"].tolist()):
        x = _t(g["in/cutouts"] if reads == "cutouts" else g["in/image"])
        res += list(_loss_grad(_score(obj, args, reads, x), x))
    from pixray_amd import ops
    img = _t(g["in/filter_image"]).requires_grad_(True)
    for mode, em in (("shift", 0), ("none", 4), ("horizontal", 4), ("vertical", 6)):
        o, loss = ops.wallpaper(img, torch.tensor([7, 5], dtype=torch.int32, device=DEV), mode, em)
        (gi,) = torch.autograd.grad((o * o).sum() + loss, img)
        res += [o.detach(), loss.detach(), gi]
    z = _t(g["lookup4/in"]).requires_grad_(True)
    o, loss = ops.color_lookup(z, ops._palette_dev(g["in/lookup_palette"], DEV), 2.5)
    (gz,) = torch.autograd.grad((o * o).sum() + loss, z)
    return res + [o.detach(), loss.detach(), gz]


def check_bit_identical_runs():
    a, b = _all_outputs(), _all_outputs()
    assert len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


def check_shards_reproduce_full_batch(world=2):
    """Each loss scored the way engine.Session scores it on `world` cutout shards (needs_full_batch: every rank scores the
    gathered batch, differentiable through its own shard, at the full weight; otherwise every rank scores its own shard at
    weight / world; an image loss sees the replicated image at weight / world and the image gradient is all-reduced) adds up to
    the unsharded value and gradient."""
    from pixray_amd.engine import needs_full_batch
    g = gold()
    for name, obj, args, reads in loss_objects(g["in/palette"].tolist()):
        x = _t(g["in/cutouts"] if reads == "cutouts" else g["in/image"])
        score = _score(obj, args, reads, x)
        full_l, full_g = _loss_grad(score, x)
        grad = torch.zeros_like(x)
        if reads == "image":
            assert not needs_full_batch(obj), name
            vals = []
            for r in range(world):
                l, gr = _loss_grad(lambda t: score(t) / world if not isinstance(score(t), list) else score(t)[0] / world, x)
                vals.append(l)
                grad += gr
            value = sum(vals)
        else:
            shards = list(x.chunk(world))
            vals = []
            for r in range(world):
                own = shards[r].clone().requires_grad_(True)
                if needs_full_batch(obj):
                    l = score(torch.cat([own if i == r else shards[i] for i in range(world)]))[0]
                else:
                    l = score(own)[0] / world
                l.backward()
                vals.append(l.detach())
                lo = sum(s.shape[0] for s in shards[:r])
                grad[lo:lo + own.shape[0]] += own.grad
            value = vals[0] if needs_full_batch(obj) else sum(vals)
        assert abs(float(value) - float(full_l)) <= 1e-6 * abs(float(full_l)), (name, float(value), float(full_l))
        assert _rel(grad, full_g) <= 1e-6, (name, _rel(grad, full_g))
        if reads == "cutouts":       # and the declaration matters: scored per shard, these losses would come out different
            shards = list(x.chunk(world))
            per_shard = sum(float(score(s)[0]) for s in shards) / world
            assert abs(per_shard - float(full_l)) > 1e-4 * abs(float(full_l)), name


def check_plugin_tables_build():
    from pixray_amd import plugins
    from pixray_amd.builtin_filters import ColorLookup, TilerFilter, WallpaperFilter
    from pixray_amd.palette import palette_from_string
    args = types.SimpleNamespace(palette=palette_from_string("red->yellow"), saturation_weight=1, symmetry_weight=1,
                                 smoothness_weight=1, smoothness_type="default", smoothness_gaussian_kernel=0, smoothness_gaussian_std=1,
                                 smoothness_spacing=1, smoothness_edge_order=1, palette_weight=1, edge_thickness=5, edge_margins=None,
                                 edge_color="white", edge_color_weight=0.1, global_color_weight=0.05, edge_input_image="",
                                 edge_mask_image="", lookup_beta=10.0, wallpaper_type="shift", wallpaper_edge_match=0)
    losses, _, args = plugins.setup_custom_losses("saturation,symmetry,smoothness:0.5,palette,edge", args, device=DEV)
    assert [type(t["loss"]).__name__ for t in losses] == ["SaturationLoss", "SymmetryLoss", "SmoothnessLoss", "PaletteLoss", "EdgeLoss"]
    assert [t["weight"] for t in losses] == [1, 1, 0.5, 1, 1] and args.edge_color == (1.0, 1.0, 1.0)
    assert all(t["loss"].supports_graph_replay for t in losses)
    filters = plugins.setup_filters("lookup,tiler,wallpaper", args, device=DEV)
    assert [type(f["filter"]) for f in filters] == [ColorLookup, TilerFilter, WallpaperFilter]
    return losses, filters


# ------------------------------------------------------------------------------------------------ GPU-only tests
def test_losses_match_reference_small():
    check_losses_small()


def test_filters_match_reference_small():
    check_filters_small()


def test_two_runs_bit_identical():
    check_bit_identical_runs()


def test_shards_reproduce_full_batch():
    check_shards_reproduce_full_batch()


def test_losses_match_reference_headline_size():
    from make_golden_plugins import headline_input
    g = gold()
    pal = g["in/palette"].tolist()
    inputs = {"cutouts": headline_input("cutouts").to(DEV), "image": headline_input("image").to(DEV)}
    probes = {"cutouts": headline_input("probe_cutouts").to(DEV), "image": headline_input("probe_image").to(DEV)}
    for name, obj, args, reads in loss_objects(pal):
        if f"head/{name}/loss" not in g:
            continue
        x = inputs[reads]
        loss, grad = _loss_grad(_score(obj, args, reads, x), x)
        ref_l = float(g[f"head/{name}/loss"])
        assert abs(float(loss) - ref_l) <= LOSS_RTOL * abs(ref_l), (name, float(loss), ref_l)
        gn, gp = float(grad.double().norm()), float((grad.double() * probes[reads].double()).sum())
        assert abs(gn - float(g[f"head/{name}/grad_norm"])) <= GRAD_RTOL * float(g[f"head/{name}/grad_norm"]), (name, gn)
        assert abs(gp - float(g[f"head/{name}/grad_probe"])) <= GRAD_RTOL * (abs(float(g[f"head/{name}/grad_probe"])) + gn), (name, gp)


def test_filters_headline_size_exact():
    """roll / wallpaper forwards at the image size of the headline are exact gathers: torch.roll on the same shifts"""
    from pixray_amd import ops
    img = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(5)).to(DEV)
    sh = torch.tensor([37, 201], dtype=torch.int32, device=DEV)
    o, _ = ops.wallpaper(img, sh, "none", 0)
    assert torch.equal(o, torch.roll(img, shifts=(37, 201), dims=(2, 3)))
    o, _ = ops.wallpaper(img, sh, "shift", 0)
    two = torch.cat([img, torch.roll(img, shifts=(128,), dims=(3,))], dim=2)
    assert torch.equal(o, torch.roll(two, shifts=(37, 201), dims=(2, 3)))
    o, _ = ops.wallpaper(img, sh, "horizontal", 8)
    assert torch.equal(o, torch.roll(img[:, :, :, 4:-4], shifts=(201,), dims=(3,)))


def test_frontend_run_with_builtin_plugins(tmp_path):
    from pixray_amd import frontend as fe
    run = fe.Run()
    run.settings = dict(drawer="vqgan", vqgan_model="tiny_f4", clip_models="tiny-B/32", size=[64, 64], num_cuts=8, iterations=5,
                        save_every=5, display_every=5, outdir=str(tmp_path / "out"), seed=3, skip_args=True, init_noise="none",
                        vector_prompts="none", noise_prompt_seeds=[1], noise_prompt_weights=[1.0], learning_rate_drops=[],
                        custom_loss="saturation,symmetry,smoothness:0.5,palette", palette="red->yellow", filters="wallpaper",
                        wallpaper_type="shift")
    s = fe.apply_settings(run=run)
    assert len(s.palette) == 16
    sess = fe.do_init(s, run)
    z0 = sess.drawer.get_z_copy()
    while not fe.do_run(s, run=run):
        pass
    z = sess.drawer.get_z()
    assert sess.cur_iteration == 5 and torch.isfinite(z).all()
    assert float((z - z0).abs().max()) > 1e-3
    assert all(torch.isfinite(l).all() for l in sess.last_losses)


def test_graph_replay_with_tiler_and_saturation():
    """a replayed session with a host-drawing filter: the tiler's shifts are staged by host_prep from the same global torch
    stream, so every iteration is the eager one (teacher-forced, as tests/test_e2e_gpu.py's replay test)"""
    from pixray_amd import api
    from pixray_amd.builtin_filters import TilerFilter
    from pixray_amd.builtin_losses import SaturationLoss

    def build():
        return api.build_vqgan_clip_session(size=(64, 64), vqgan_model="tiny_f4", clip_model="tiny-B/32", num_cuts=8, seed=3,
                                            filters=[{"filter": TilerFilter(types.SimpleNamespace(), device="cuda"), "weight": 1.0}],
                                            custom_losses=[{"loss": SaturationLoss(device="cuda"), "weight": 1.0}])
    a, b = build(), build()
    a.args = b.args = types.SimpleNamespace(saturation_weight=1.0)
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
