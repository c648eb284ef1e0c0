"""The pixel drawer (pixray_amd/pixel_drawer.py on csrc/pixel_raster.hip): grid sizes, polygons and init colours against what
pixray's own pixeldrawer.py builds (tests/golden/pixel_drawer_golden.npz, written by tests/golden/make_golden_pixel.py), the
jitter against its numpy twin, and the rendered ids / image / colour gradients against the independent float64 rasteriser of
tests/_pixel_raster_ref.py.  tests/test_pixel_drawer_cpu.py runs the `check_*` functions on the emulated kernels with
DEV = "cpu"."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import _pixel_raster_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EDGE_PX = 1e-3               # samples this close to a polygon edge may be decided differently in fp32 and float64
IMG_ATOL, GRAD_RTOL = 1e-5, 1e-5


def gold():
    from make_golden_pixel import OUT
    return np.load(OUT)


def make_drawer(width, height, pixel_type, **kw):
    from pixray_amd.pixel_drawer import PixelDrawer
    st = types.SimpleNamespace(size=[width, height], pixel_size=kw.get("pixel_size"), pixel_scale=kw.get("pixel_scale"),
                               pixel_type=pixel_type, pixel_edge_check=kw.get("edge_check", True),
                               pixel_iso_check=kw.get("iso_check", True), transparent=kw.get("transparent", False))
    d = PixelDrawer(st)
    d.load_model(st, DEV)
    return d


def seeded_colors(n, seed, alpha="opaque"):
    """RGB in [0, 1]; alpha 1 ("opaque"), or half the shapes semi-transparent ("mixed")"""
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(n, 4, generator=g)
    if alpha == "opaque":
        c[:, 3] = 1.0
    else:
        c[:, 3] = torch.where(torch.rand(n, generator=g) < 0.5, torch.ones(n), 0.1 + 0.8 * c[:, 3])
    return c


def _seed(it):
    return torch.tensor([it], dtype=torch.int32, device=DEV)


def check_names_resolve_and_parse(tmp_path):
    from pixray_amd import frontend as fe
    from pixray_amd import plugins
    from pixray_amd.pixel_drawer import PixelDrawer
    assert plugins.class_table["pixel"] is PixelDrawer
    run = fe.Run()
    run.settings = dict(outdir=str(tmp_path / "p"))
    s = fe.apply_settings(["--drawer", "pixel", "--pixel_type", "hex", "--pixel_iso_check", "false", "--pixel_scale", "2.5"], run=run)
    assert (s.drawer, s.pixel_type, s.pixel_iso_check, s.pixel_edge_check, s.pixel_scale, s.pixel_size) == \
        ("pixel", "hex", False, True, 2.5, None)


def check_fixture_rows():
    """grid size, every polygon (bit-equal) and the init colours (bit-equal) of every fixture row"""
    from make_golden_pixel import ROWS, init_image, settings
    from pixray_amd.pixel_drawer import PixelDrawer
    g = gold()
    for i, row in enumerate(ROWS):
        st = settings(row)
        d = PixelDrawer(st)
        d.load_model(st, DEV)
        assert (d.num_cols, d.num_rows) == tuple(g[f"r{i}/grid"]), (i, row)
        v = d.vertices
        assert v.dtype == np.float32 and np.array_equal(v, g[f"r{i}/verts"]), (i, row)
        d.init_from_tensor(init_image(i).to(DEV))
        assert d.z.shape == (len(v), 4) and d.z.is_leaf and d.z.requires_grad
        assert torch.equal(d.get_z_copy().cpu(), torch.from_numpy(g[f"r{i}/colors"])), (i, row)


def check_jitter_twin():
    from pixray_amd import ops
    from pixray_amd.pixel_drawer import sample_offsets_np
    for (w, h), seed in (((37, 23), 0), ((64, 48), 1), ((19, 61), 123457), ((8, 8), 2 ** 31 - 1)):
        uv = ops.pixel_sample_offsets(w, h, _seed(seed)).cpu().numpy()
        assert np.array_equal(uv, sample_offsets_np(w, h, seed)), ((w, h), seed)
        assert uv.min() >= 0 and uv.max() < 1
    a, b = sample_offsets_np(16, 16, 3), sample_offsets_np(16, 16, 4)
    assert not np.array_equal(a, b)


def check_against_oracle(width, height, pixel_type, seed, alpha, max_near=0.01, verts=None, **kw):
    """ids away from edges equal, image within IMG_ATOL and colour gradient within GRAD_RTOL (rel-L2) of the float64 oracle;
    pixels with a sample within EDGE_PX of an edge are left out of the image and gradient comparisons (their share is asserted
    small)"""
    from pixray_amd import ops
    from pixray_amd.pixel_drawer import sample_offsets_np
    if verts is None:
        d = make_drawer(width, height, pixel_type, **kw)
        geom, verts = d.geometry, d.vertices
    else:
        geom = ops.PixelRasterGeometry(verts, width, height, DEV)
    col = seeded_colors(geom.n_shapes, seed + 1, alpha)
    layers, dist = ref.coverage(verts, width, height, sample_offsets_np(width, height, seed))
    near = dist.reshape(height, width, 4) <= EDGE_PX
    assert near.mean() <= max_near, (pixel_type, float(near.mean()))
    keep = torch.from_numpy(~near.any(2))
    probe = torch.randn(1, 4, height, width, dtype=torch.float64, generator=torch.Generator().manual_seed(seed + 2)) * keep
    r = ref.shade(layers, dist, col, width, height, probe=probe)
    img_ids, ids = ops.pixel_raster_ids(col.to(DEV), geom, _seed(seed))
    assert np.array_equal(ids.cpu().numpy()[~near], r["ids"][~near]), pixel_type
    c = col.to(DEV).requires_grad_(True)
    img = ops.pixel_raster(c, geom, _seed(seed))
    assert torch.equal(img.detach(), img_ids)
    (img.double() * probe.to(DEV)).sum().backward()
    diff = (img.detach().double().cpu() - r["image"]).abs()[0].permute(1, 2, 0)[keep]
    assert float(diff.max()) <= IMG_ATOL, (pixel_type, float(diff.max()))
    rel = float((c.grad.double().cpu() - r["grad"]).norm() / r["grad"].norm())
    assert rel <= GRAD_RTOL, (pixel_type, rel)
    return img.detach(), c.grad, lambda: _render_and_grad(col, geom, seed, probe)


def _render_and_grad(col, geom, seed, probe):
    from pixray_amd import ops
    c = col.to(DEV).requires_grad_(True)
    img = ops.pixel_raster(c, geom, _seed(seed))
    (img.double() * probe.to(DEV)).sum().backward()
    return img.detach(), c.grad


PARITY_CASES = [(t, a) for t in ("rect", "rectshift", "hex", "tri", "diamond", "knit") for a in ("opaque", "mixed")]


def check_small_parity():
    """every pixel type, non-integer cells on a non-square canvas, opaque and semi-transparent colours"""
    for i, (t, a) in enumerate(PARITY_CASES):
        check_against_oracle(45, 37, t, 11 + i, a, pixel_size=(7, 6))


def check_overlapping_polygons():
    """a tile with more shapes than one LDS chunk holds (64): 150 overlapping, self-intersecting 7-gons"""
    rng = np.random.default_rng(1)
    v = (rng.uniform(-3, 24, (150, 1, 2)) + rng.uniform(-9, 9, (150, 7, 2))).astype(np.float32)
    check_against_oracle(21, 18, None, 5, "mixed", max_near=0.05, verts=v)


def check_integer_rect_cells_equal_pixel_grid():
    """rect cells of integer size render exactly PixelGridDrawer's nearest upsampling of the same colours, whatever the seed"""
    from pixray_amd import ops
    from pixray_amd.pixel_grid_drawer import PixelGridDrawer
    for (w, h), (cols, rows) in (((48, 40), (12, 10)), ((60, 24), (20, 4))):
        d = make_drawer(w, h, "rect", pixel_size=(cols, rows))
        col = seeded_colors(d.geometry.n_shapes, cols, "opaque")
        st = types.SimpleNamespace(size=[w, h], pixel_size=(cols, rows), pixel_scale=None)
        grid = PixelGridDrawer(st)
        grid.load_model(st, DEV)
        grid.z = col[:, :3].reshape(rows, cols, 3).permute(2, 0, 1)[None].contiguous().to(DEV)
        want = grid.synth(0)
        for seed in (0, 1, 99, 2 ** 20 + 7):
            img = ops.pixel_raster(col.to(DEV), d.geometry, _seed(seed))
            assert torch.equal(img[:, :3], want), ((w, h), seed)
            assert torch.equal(img[:, 3], torch.ones_like(img[:, 3]))


def check_bit_identical_runs():
    for t in ("hex", "knit"):
        img, g, again = check_against_oracle(45, 37, t, 3, "mixed", pixel_size=(7, 6))
        img2, g2 = again()
        assert torch.equal(img, img2) and torch.equal(g, g2), t


def check_drawer_surface():
    """the drawer API around the kernels: init from None (python `random`), synth / synth(-1) / to_image, clip_z, z accessors,
    Adam on the one leaf, the refusal of return_transparency"""
    import random
    d = make_drawer(30, 20, "tri", pixel_size=(5, 4))
    random.seed(4)
    d.init_from_tensor(None)
    random.seed(4)
    n = d.geometry.n_shapes
    want = torch.tensor([random.random() for _ in range(3 * n)], dtype=torch.float32).reshape(n, 3)
    z = d.get_z()
    assert z is d.z and z.is_leaf and torch.equal(z.detach()[:, :3].cpu(), want) and bool((z.detach()[:, 3] == 1).all())
    first = d.synth(-1)
    assert first.shape == (1, 4, 20, 30)
    img = d.synth(5)
    assert img.requires_grad and d.synth(-1) is img
    assert d.to_image().size == (30, 20) and d.to_image().mode == "RGB"
    with pytest.raises(NotImplementedError):
        d.synth(1, return_transparency=True)
    (opt,) = d.get_opts(10)
    assert isinstance(opt, torch.optim.Adam) and opt.param_groups[0]["lr"] == pytest.approx(0.003)
    assert opt.param_groups[0]["params"][0] is z
    with torch.no_grad():
        z.sub_(0.5)
        z[:, 3] = 0.5
    d.clip_z()
    assert float(z.detach()[:, :3].min()) == 0.0 and bool((z.detach()[:, 3] == 1).all())
    d.transparent = True
    with torch.no_grad():
        z[:, 3] = -0.5
    d.clip_z()
    assert bool((z.detach()[:, 3] == 0).all())
    copy = d.get_z_copy()
    d.set_z(torch.zeros_like(copy))
    assert float(d.get_z().detach().abs().sum()) == 0.0 and float(copy.abs().sum()) > 0
    d.reapply_from_tensor(torch.zeros(1, 3, 20, 30, device=DEV))
    assert torch.equal(d.get_z().detach().cpu(), torch.tensor([[0.5, 0.5, 0.5, 1.0]]).expand(n, 4))
    assert d.get_num_resolutions() is None and d.get_z_from_tensor(None) is None


# ------------------------------------------------------------------------------------------------ GPU-only tests
def test_names_resolve_and_parse(tmp_path):
    check_names_resolve_and_parse(tmp_path)


def test_fixture_rows():
    check_fixture_rows()


def test_jitter_twin():
    check_jitter_twin()


def test_small_parity():
    check_small_parity()


def test_overlapping_polygons():
    check_overlapping_polygons()


def test_integer_rect_cells_equal_pixel_grid():
    check_integer_rect_cells_equal_pixel_grid()


def test_two_runs_bit_identical():
    check_bit_identical_runs()


def test_drawer_surface():
    check_drawer_surface()


@pytest.mark.parametrize("w,h,typ", [(360, 360, "rect"), (360, 360, "hex"), (1024, 576, "diamond")],
                         ids=["text2pixel_rect", "text2pixel_hex", "diamond_1024x576"])
def test_preset_size_parity(w, h, typ):
    """the text2pixel canvas (quality `better` at scale 2.5: 360 x 360) with its default grids, and a large diamond grid"""
    d = make_drawer(w, h, typ)
    assert (d.num_cols, d.num_rows) == {"rect": (40, 40), "hex": (41, 57), "diamond": (81, 91)}[typ]
    img, g, again = check_against_oracle(w, h, typ, 17, "mixed")
    img2, g2 = again()
    assert torch.equal(img, img2) and torch.equal(g, g2)


def _session_settings(tmp_path, name, **kw):
    return {**dict(drawer="pixel", pixel_type="hex", clip_models="tiny-B/32", size=[72, 56], num_cuts=8, iterations=12, save_every=100,
                   display_every=100, outdir=str(tmp_path / name), seed=5, skip_args=True, init_noise="none", vector_prompts="none",
                   noise_prompt_seeds=[1], noise_prompt_weights=[1.0], learning_rate_drops=[]), **kw}


def test_graph_replay_matches_eager_session(tmp_path):
    """a replayed session draws the jitter of every iteration (the seed word is staged by host_prep), so its colours and losses
    are bit-equal to an eager session's; a seed frozen at capture would part them at the first replay.  Both sessions step with
    the fused Adam kernel (the replayed session swaps the drawer's torch Adam for it), and cutout noise is off (the device
    randn streams of capture and eager differ)."""
    from pixray_amd import frontend as fe
    from pixray_amd.engine import HipAdam

    def build(name):
        run = fe.Run()
        run.settings = _session_settings(tmp_path, name)
        sess = fe.do_init(fe.apply_settings(run=run), run)
        for mk in sess.cutoutsTable.values():
            mk.noise_fac = 0.0
        return sess
    a, b = build("eager"), build("graph")
    assert torch.equal(a.drawer.get_z(), b.drawer.get_z())
    a.opts = [HipAdam.from_adam(o) for o in a.opts]
    assert b.enable_graph(warmup=2), b.graph_error
    assert b._graph is not None and b.drawer.graph_capturable
    for it in range(2):
        a.train(it)
    for it in range(2, 10):
        a.train(it)
        b.train(it)
        assert torch.equal(a.drawer.get_z(), b.drawer.get_z()), it
        assert all(torch.equal(x, y) for x, y in zip(a.last_losses, b.last_losses)), it
    assert b._graph is not None
    z0 = a.drawer.get_z_copy()
    a.train(10)
    assert not torch.equal(a.drawer.get_z(), z0)


def test_frontend_run_writes_png(tmp_path):
    from PIL import Image
    from pixray_amd import frontend as fe
    run = fe.Run()
    run.settings = _session_settings(tmp_path, "fe", pixel_type="knit", iterations=6, save_every=3, display_every=3)
    s = fe.apply_settings(run=run)
    sess = fe.do_init(s, run)
    z0 = sess.drawer.get_z_copy()
    while not fe.do_run(s, run=run):
        pass
    z = sess.drawer.get_z()
    assert sess.cur_iteration == 6 and torch.isfinite(z).all() and float((z.detach() - z0).abs().max()) > 1e-3
    assert bool((z.detach()[:, 3] == 1).all()) and float(z.detach().min()) >= 0 and float(z.detach().max()) <= 1
    pngs = [f for f in os.listdir(tmp_path / "fe") if f.endswith(".png")]
    assert pngs
    img = Image.open(os.path.join(tmp_path / "fe", pngs[0]))
    assert img.size == (72, 56)
