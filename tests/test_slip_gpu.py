"""SLIP perceptors on the HIP ViT runner: the two GELU epilogue codes of the GEMM engine, the tower family against the plain-torch
restatement (tests/_slip_ref.py, float64), the runner's ablation switches, and a mixed CLIP + SLIP session.  The check functions
take their device from `DEV`, so tests/test_slip_cpu.py runs the same ones on the CPU emulation of the kernels.

Every test here fails on a tree without the SLIP family (no PRX_ACT_GELU, no prx_vit_tower_create, no SLIP_CONFIGS)."""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _slip_ref  # noqa: E402
from pixray_amd import _lib, ops, weights  # noqa: E402
from pixray_amd._lib import GemmArgs, call  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ACT_GELU, ACT_MUL_DGELU = 6, 7
F32_GATE = 1e-4          # tests/test_f32_mode_gpu.py: the stated gate of the exact mode


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def cosine(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-300)).item()


def stream():
    return _lib.current_stream()


# ------------------------------------------------------------------------------------------ GEMM epilogues
# kernel families a 16-bit row-major product can be forced onto (prx_gemm_tile_override), and the exact-f32 4-wave kernel
FAMILIES = {"4wave": (128, 128, False), "fit": (160, 256, True), "fit-kgroups": (80, 128, True), "8phase": (256, 256, False)}


def gelu_epilogue_checks(family, prec, shapes=((333, 520, 512), (197 * 2, 1024, 256))):
    """c_fc form (bias + GELU, 16-bit output + saved pre-activation) and dgrad form (* GELU'(aux)) of one kernel family against
    float64 on the same rounded operands: the 16-bit outputs within one rounding of the operand format (2^-11 / 2^-8 relative,
    in rel-L2 well under 5e-4 / 4e-3, the figures tests/test_kernels_gpu.py uses for these formats), fp32 at 1e-5"""
    lib = _lib.load()
    ctx = _lib.tool_ctx()
    f32 = prec == "f32"
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[prec]
    tol = {"fp16": 5e-4, "bf16": 4e-3, "f32": 1e-5}[prec]
    code = {"fp16": 2, "bf16": 0, "f32": 1}[prec]
    try:
        if not f32:
            bm, bn, fit = FAMILIES[family]
            lib.prx_gemm_tile_override(ctx, -12, 0, 1 if fit else 0)
            lib.prx_gemm_tile_override(ctx, bm, bn, 1)
        for (M, N, K) in shapes:
            g0 = torch.Generator().manual_seed(M + N + K)
            A = torch.randn(M, K, generator=g0).to(DEV).to(dt)
            Bt = (torch.randn(N, K, generator=g0) / math.sqrt(K)).to(DEV).to(dt)
            bias = torch.randn(N, generator=g0).to(DEV)
            aux = (1.5 * torch.randn(M, N, generator=g0)).to(DEV).to(dt)
            prod = A.double() @ Bt.double().T

            def args():
                g = GemmArgs()
                g.A = A.data_ptr(); g.a_is_f32 = 0; g.lda = K; g.B = Bt.data_ptr(); g.ldb = K; g.M, g.N, g.K = M, N, K
                g.alpha = 1.0; g.f32 = code
                return g
            g = args()
            g.bias_n = bias.data_ptr(); g.act = ACT_GELU
            u = torch.full((M + 1, N), float("nan"), device=DEV, dtype=dt); g.out_bf16 = u.data_ptr()
            t = torch.full((M + 1, N), float("nan"), device=DEV, dtype=dt); g.out_bf16_pre = t.data_ptr(); g.ldc_bf16 = N
            call("prx_k_gemm", g, None, 0, stream())
            pre = (prod + bias.double()).to(dt).double()            # the saved pre-activation is rounded, then activated
            assert torch.isnan(u[M].float()).all() and torch.isnan(t[M].float()).all(), "wrote past row M - 1"
            e_t, e_u = rel_l2(t[:M], pre), rel_l2(u[:M], _slip_ref.gelu(t[:M].double()))
            print(f"gelu epilogue {family} {prec} {M}x{N}x{K}: pre {e_t:.2e} act {e_u:.2e}")
            assert e_t < tol and e_u < tol, (family, prec, M, N, K, e_t, e_u)
            g = args()
            g.aux = aux.data_ptr(); g.ldaux = N; g.act = ACT_MUL_DGELU
            d = torch.full((M + 1, N), float("nan"), device=DEV, dtype=dt); g.out_bf16 = d.data_ptr(); g.ldc_bf16 = N
            call("prx_k_gemm", g, None, 0, stream())
            e_d = rel_l2(d[:M], prod * _slip_ref.dgelu(aux.double()))
            print(f"dgelu epilogue {family} {prec} {M}x{N}x{K}: {e_d:.2e}")
            assert torch.isnan(d[M].float()).all() and e_d < tol, (family, prec, M, N, K, e_d)
    finally:
        lib.prx_gemm_tile_override(ctx, 0, 0, 0)
        lib.prx_gemm_tile_override(ctx, -12, 0, 0)


@pytest.mark.parametrize("family,prec", [(f, p) for f in FAMILIES for p in ("fp16", "bf16")])
def test_gelu_epilogues_vs_float64(family, prec):
    gelu_epilogue_checks(family, prec)


def gelu_f32_refusal_check():
    """the exact-f32 kernels carry no GELU epilogue (their scalar epilogue must stay small, csrc/gemm_epi.h): prx_k_gemm refuses
    the two codes there with a message; the runner's parity mode applies the activation in a pass of its own (tower tests, f32)"""
    A = torch.randn(64, 64).to(DEV); Bt = torch.randn(64, 64).to(DEV); o = torch.empty(64, 64).to(DEV)
    g = GemmArgs()
    g.A = A.data_ptr(); g.lda = 64; g.B = Bt.data_ptr(); g.ldb = 64; g.M = g.N = g.K = 64; g.alpha = 1.0; g.f32 = 1
    g.act = ACT_GELU; g.out_bf16 = o.data_ptr(); g.ldc_bf16 = 64
    with pytest.raises(_lib.PrxError, match="GELU"):
        call("prx_k_gemm", g, None, 0, stream())


def test_gelu_codes_are_refused_by_the_f32_kernels():
    gelu_f32_refusal_check()


def test_gelu_launches_are_served_by_the_generic_fit_kernel():
    """which family serves the SLIP c_fc product and its dgrad at 197 tokens x 8 cutouts, widths 768 and 1024: the planner says a fit
    tile or the 8-phase kernel, and the launch counter of the compile-time epilogues does not move -- the generic epilogue serves
    the two new codes (FIT_EPI_GELU / DGELU are QuickGELU's)"""
    lib = _lib.load()
    for W in (768, 1024):
        M = 8 * 197
        A = torch.randn(M, W, device=DEV).half(); Bt = (torch.randn(4 * W, W, device=DEV) / math.sqrt(W)).half()
        bias = torch.randn(4 * W, device=DEV)
        u = torch.empty(M, 4 * W, device=DEV, dtype=torch.float16); t = torch.empty_like(u)
        g = GemmArgs()
        g.A = A.data_ptr(); g.lda = W; g.B = Bt.data_ptr(); g.ldb = W; g.M, g.N, g.K = M, 4 * W, W; g.alpha = 1.0; g.f32 = 2
        g.bias_n = bias.data_ptr(); g.act = ACT_GELU; g.out_bf16 = u.data_ptr(); g.out_bf16_pre = t.data_ptr(); g.ldc_bf16 = 4 * W
        import ctypes
        plan = (ctypes.c_int * 9)()
        assert lib.prx_gemm_plan(None, ctypes.addressof(g), 64 << 20, 256, ctypes.addressof(plan)) == 0
        print(f"c_fc plan at width {W}: family {plan[0]} tile {plan[1]}x{plan[2]}")
        assert plan[0] in (3, 4), list(plan)
        n0 = lib.prx_gemm_fit_spec_launches()
        call("prx_k_gemm", g, None, 0, stream())
        assert lib.prx_gemm_fit_spec_launches() == n0
        assert rel_l2(u, _slip_ref.gelu(t.double())) < 5e-4


# ------------------------------------------------------------------------------------------ tower vs restatement
def slip_cfg(name):
    if name in weights.SLIP_CONFIGS:
        return weights.SLIP_CONFIGS[name]
    width, layers, heads = {"test-384": (384, 2, 12), "test-768": (768, 2, 12), "test-1024": (1024, 2, 16)}[name]
    return weights.SlipVitConfig(name, width=width, layers=layers, heads=heads, output_dim=512, seed_offset=20)


def slip_case(name, n, precision, seed=5):
    cfg = slip_cfg(name)
    params = weights.synthetic_slip_vit_params(cfg, seed)
    g = torch.Generator().manual_seed(seed + 1)
    cut = torch.rand(n, 3, cfg.input_resolution, cfg.input_resolution, generator=g) * 1.2 - 0.1
    gout = torch.randn(n, cfg.output_dim, generator=g)
    ref, gref = _slip_ref.embed_and_grad(params, cfg, cut, gout, torch.float64)
    h = ops.SlipVitHandle(cfg, params, max_batch=n, device=DEV, precision=precision)
    cd = cut.to(DEV).requires_grad_(True)
    out = ops.clip_encode_image(cd, h)
    (gd,) = torch.autograd.grad(out, cd, gout.to(DEV))
    return ref, out, gref, gd


def tower_checks(name, n, precision):
    ref, out, gref, gd = slip_case(name, n, precision)
    figs = (rel_l2(out, ref), cosine(out, ref), rel_l2(gd, gref), cosine(gd, gref))
    print(f"SLIP tower {name} n={n} {precision}: emb rel-L2 {figs[0]:.3e} cos {figs[1]:.8f}  grad rel-L2 {figs[2]:.3e} cos {figs[3]:.8f}")
    if precision == "f32":
        assert figs[0] < F32_GATE and figs[2] < F32_GATE, figs
    elif precision == "fp16":       # the gates of tests/test_path_gpu.py::test_clip_vit_vs_oracle (the product default, IEEE half)
        assert figs[0] < 5e-3 and figs[1] > 0.9999 and figs[2] < 2e-2 and figs[3] > 0.9999, figs
    else:
        # bf16 keeps 8 significand bits where half keeps 11: operand rounding is 2^3 times coarser, so the rel-L2 gates are the
        # fp16 ones times 8, and the cosine gate (1 - cos grows with the square of the relative error) 1 - 64 * 1e-4
        assert figs[0] < 8 * 5e-3 and figs[1] > 1 - 64e-4 and figs[2] < 8 * 2e-2 and figs[3] > 1 - 64e-4, figs


@pytest.mark.parametrize("name,n,precision", [("tiny-SLIP/16", 3, "fp16"), ("tiny-SLIP/16", 3, "bf16"), ("tiny-SLIP/16", 3, "f32"),
                                              ("test-384", 2, "fp16"), ("test-384", 2, "f32"), ("SLIP_VITS16", 4, "fp16"),
                                              ("SLIP_VITS16", 4, "f32"), ("test-768", 2, "fp16"), ("test-768", 2, "f32"), ("test-1024", 2, "fp16"),
                                              ("test-1024", 2, "f32"), ("SLIP_VITB16", 8, "fp16"), ("SLIP_VITB16", 8, "f32")])
def test_slip_tower_vs_restatement(name, n, precision):
    """embeddings and d/d cutouts of the HIP tower against the float64 restatement: reduced 197-token towers at widths 256, 384
    (12 heads of 32, padded to 64 by the runner; the restatement runs the 32-wide heads), 768 and 1024 (2 layers), the full
    SLIP_VITS16 at 4 and the full SLIP_VITB16 at 8 cutouts.  Gates: the CLIP ViT towers' own (see tower_checks)."""
    tower_checks(name, n, precision)


def padded_head_checks(name, n, precision):
    """heads of 32 through the padded-head route: the tower's outputs are the restatement's 32-wide heads' (tower_checks' gates) and
    the padded lanes of d(qkv) -- lanes 32 .. 63 of every head of q, k and v -- are exactly zero"""
    cfg = slip_cfg(name)
    assert cfg.head_dim == 32
    params = weights.synthetic_slip_vit_params(cfg, 5)
    g = torch.Generator().manual_seed(8)
    cut = torch.rand(n, 3, 224, 224, generator=g) * 1.2 - 0.1
    gout = torch.randn(n, cfg.output_dim, generator=g)
    ref, gref = _slip_ref.embed_and_grad(params, cfg, cut, gout, torch.float64)
    h = ops.SlipVitHandle(cfg, params, max_batch=n, device=DEV, precision=precision)
    cd = cut.to(DEV).requires_grad_(True)
    out = ops.clip_encode_image(cd, h)
    (gd,) = torch.autograd.grad(out, cd, gout.to(DEV))
    figs = (rel_l2(out, ref), rel_l2(gd, gref))
    print(f"padded heads {name} n={n} {precision}: emb {figs[0]:.3e} grad {figs[1]:.3e}")
    if precision == "f32":
        assert figs[0] < F32_GATE and figs[1] < F32_GATE, figs
    else:
        assert figs[0] < 5e-3 and figs[1] < 2e-2 and cosine(out, ref) > 0.9999 and cosine(gd, gref) > 0.9999, figs
    dt = torch.float32 if precision == "f32" else torch.float16
    dqkv = torch.full((n * cfg.tokens, 3, cfg.heads, 64), float("nan"), dtype=dt, device=DEV)
    got = _lib.load().prx_vit_tower_debug_dqkv(h.h, dqkv.data_ptr(), dqkv.numel() * dqkv.element_size(), stream())
    if DEV != "cpu":
        torch.cuda.synchronize()
    assert got == dqkv.numel() * dqkv.element_size()
    assert torch.isfinite(dqkv.float()).all() and dqkv[..., :32].float().abs().max() > 0
    assert (dqkv[..., 32:] == 0).all(), "padded lanes of dqkv are not exactly zero"


@pytest.mark.parametrize("precision", ["f32", "fp16"])
def test_heads_of_32_equal_the_restatement_and_padded_lanes_are_zero(precision):
    padded_head_checks("test-384", 2, precision)


def switch_ab(env_name, precision, name="tiny-SLIP/16", n=4):
    cfg = slip_cfg(name)
    params = weights.synthetic_slip_vit_params(cfg, 5)
    g = torch.Generator().manual_seed(6)
    cut = torch.rand(n, 3, cfg.input_resolution, cfg.input_resolution, generator=g)
    gout = torch.randn(n, cfg.output_dim, generator=g)
    res, old = [], os.environ.get(env_name)
    try:
        for val in ("0", "1"):
            os.environ[env_name] = val
            h = ops.SlipVitHandle(cfg, params, max_batch=n, device=DEV, precision=precision)
            cd = cut.to(DEV).requires_grad_(True)
            out = ops.clip_encode_image(cd, h)
            (gd,) = torch.autograd.grad(out, cd, gout.to(DEV))
            res.append((out.detach().float().cpu(), gd.detach().float().cpu()))
    finally:
        if old is None:
            os.environ.pop(env_name, None)
        else:
            os.environ[env_name] = old
    return res


def test_slip_class_token_tail_is_the_same_tower():
    """as tests/test_path_gpu.py::test_vit_class_token_tail_is_the_same_tower, same bounds"""
    (e0, g0), (e1, g1) = switch_ab("PRX_VIT_CLS_TAIL", "f32")
    assert rel_l2(e1, e0) < 2e-6 and rel_l2(g1, g0) < 2e-5, (rel_l2(e1, e0), rel_l2(g1, g0))
    (e0, g0), (e1, g1) = switch_ab("PRX_VIT_CLS_TAIL", "fp16")
    assert rel_l2(e1, e0) < 2e-3 and rel_l2(g1, g0) < 5e-3, (rel_l2(e1, e0), rel_l2(g1, g0))


def test_slip_lean_streams_ab():
    """as tests/test_path_gpu.py::test_vit_lean_streams_ab, same bounds"""
    (e0, g0), (e1, g1) = switch_ab("PRX_LEAN", "fp16")
    assert rel_l2(e1, e0) < 3e-3 and rel_l2(g1, g0) < 1e-2, (rel_l2(e1, e0), rel_l2(g1, g0))
    assert not torch.equal(e0, e1)


def test_clip_family_through_the_tower_constructor_is_bit_identical():
    """prx_vit_tower_create with family CLIP, eps 1e-5 and CLIP's constants is prx_clip_vit_create: same embeddings, same gradient,
    bit for bit -- the switches left the CLIP tower where it was"""
    import ctypes
    cfg = weights.CLIP_CONFIGS["tiny-B/32"]
    params = weights.synthetic_clip_vit_params(cfg, 3)
    g = torch.Generator().manual_seed(4)
    cut = torch.rand(4, 3, 224, 224, generator=g).to(DEV)
    gout = torch.randn(4, cfg.output_dim, generator=g).to(DEV)
    res = []
    for via_tower in (False, True):
        h = ops.ClipVitHandle(cfg, params, max_batch=4, device=DEV)
        if via_tower:
            ws = ops._weights_in_abi_order(params, weights.clip_vit_param_shapes(cfg), DEV, "CLIP ViT")
            c = ops._VitTowerCfg(cfg.input_resolution, cfg.patch_size, cfg.width, cfg.layers, cfg.heads, cfg.output_dim, 4, h.precision,
                                 ops.VIT_FAMILY_CLIP, 64, 1e-5, (ctypes.c_float * 3)(0.48145466, 0.4578275, 0.40821073),
                                 (ctypes.c_float * 3)(0.26862954, 0.26130258, 0.27577711))
            ops._destroy_handle("prx_clip_vit_destroy", h.h)
            hh = ctypes.c_void_p()
            call("prx_vit_tower_create", ctypes.addressof(hh), ctypes.addressof(c), ops._keep(h, ops._weight_array(ws)), len(ws), stream())
            torch.cuda.synchronize()
            h.h = hh
        cd = cut.clone().requires_grad_(True)
        out = ops.clip_encode_image(cd, h)
        (gd,) = torch.autograd.grad(out, cd, gout)
        res.append((out.detach().cpu(), gd.detach().cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def perceptor_checks():
    """SlipPerceptor end to end: unit embeddings, apply_preprocess=False on preprocess()'s output gives the fused path's values
    and gradient, the ImageNet constants are the ones in use, encode_texts has SLIP_Base's [n, 1, D] shape"""
    from pixray_amd.perceptor import SlipPerceptor, get_clip_perceptor
    perc = get_clip_perceptor("tiny-SLIP/16", DEV, max_batch=4, precision="f32")
    assert isinstance(perc, SlipPerceptor) and perc.input_resolution == 224 and perc.output_dim == 128
    R = 224
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(3, 3, R, R, generator=g) * 1.7 - 0.3).to(DEV).requires_grad_(True)
    gout = torch.randn(3, perc.output_dim, generator=g).to(DEV)
    e0 = perc.encode_image(x)
    (g0,) = torch.autograd.grad(e0, x, gout)
    assert torch.allclose(e0.norm(dim=-1), torch.ones(3, device=DEV), atol=1e-5)
    ref, gref = _slip_ref.embed_and_grad(weights.synthetic_slip_vit_params(perc.cfg, 0), perc.cfg, x.detach().cpu(), gout.cpu())
    assert rel_l2(e0, ref) < F32_GATE and rel_l2(g0, gref) < F32_GATE, (rel_l2(e0, ref), rel_l2(g0, gref))
    p = perc.preprocess(x)
    lo, hi = float(x.detach().min()), float(x.detach().max())
    mean = torch.tensor((0.485, 0.456, 0.406), device=DEV).view(1, 3, 1, 1); std = torch.tensor((0.229, 0.224, 0.225), device=DEV).view(1, 3, 1, 1)
    assert torch.allclose(p, ((x - lo) / (hi - lo) - mean) / std, atol=1e-6)
    e1 = perc.encode_image(p, apply_preprocess=False)
    (g1,) = torch.autograd.grad(e1, x, gout)
    assert rel_l2(e1, e0) < 1e-5 and rel_l2(g1, g0) < 1e-4, (rel_l2(e1, e0), rel_l2(g1, g0))
    e2 = perc.encode_image(x.detach(), input_range=(-0.5, 2.0))            # slip.py:153: the range reaches adjust_range
    ref2 = _slip_ref.encode_image(_slip_ref.cast(weights.synthetic_slip_vit_params(perc.cfg, 0), torch.float64), perc.cfg,
                                  x.detach().cpu().double(), lo=-0.5, hi=2.0)
    assert rel_l2(e2, ref2) < F32_GATE
    toks = torch.zeros(2, 77, dtype=torch.int32); toks[:, 0] = 998; toks[0, 1:4] = torch.tensor([5, 6, 999]); toks[1, 1:3] = torch.tensor([7, 999])
    t1 = perc.encode_text(toks)
    t2 = perc.encode_texts(toks)
    assert t1.shape == (2, 128) and t2.shape == (2, 1, 128)
    assert torch.allclose(t2[:, 0], t1 / t1.norm(dim=-1, keepdim=True), atol=1e-6)


def test_slip_perceptor_surface():
    perceptor_checks()


def test_unknown_and_refused_names():
    from pixray_amd.perceptor import get_clip_perceptor
    with pytest.raises(KeyError):
        get_clip_perceptor("SLIP_NOPE", DEV)
    with pytest.raises(ValueError, match="no text side"):
        get_clip_perceptor("SIMCLR_VITS16", DEV)


# ------------------------------------------------------------------------------------------ session
def _mixed_session():
    from pixray_amd import api
    sess = api.build_vqgan_clip_session(size=(256, 256), clip_model=["ViT-B/16", "SLIP_VITB16"], num_cuts=8, seed=11)
    for mk in sess.cutoutsTable.values():
        mk.noise_fac = 0.0            # device randn streams differ between capture and eager launches: compare without noise
    return sess


def test_mixed_session_three_iterations_deterministic_and_graph():
    """VQGAN 256^2 + ViT-B/16 + SLIP_VITB16 (the `mixed` / `normal` pair), 8 cutouts, 3 iterations: finite losses, z moves, two
    runs are bit-identical, and enable_graph() either replays to the same z as eager launches or refuses with a graph_error"""
    zs = []
    for run in range(2):
        sess = _mixed_session()
        z0 = sess.drawer.get_z_copy().detach().clone()
        for it in range(3):
            assert sess.train(it)
            assert len(sess.last_losses) == 2 and all(torch.isfinite(l) for l in sess.last_losses), sess.last_losses
        z = sess.drawer.get_z_copy().detach().clone()
        assert torch.isfinite(z).all() and (z - z0).abs().max() > 1e-3
        zs.append(z.cpu())
    assert torch.equal(zs[0], zs[1]), "two eager runs differ"
    b = _mixed_session()
    if not b.enable_graph(warmup=2):          # iterations 0, 1 through train(); iteration 2 is staged and replayed by the next train()
        assert b.graph_error, "enable_graph() refused without a graph_error"
        print("enable_graph refused:", b.graph_error)
        return
    b.train(2)
    zb = b.drawer.get_z_copy().detach().cpu()
    print("graph replay vs eager launches: max |dz| =", (zb - zs[0]).abs().max().item())
    assert torch.equal(zb, zs[0]), "graph replay differs from eager launches"


# ------------------------------------------------------------------------------------------ sharding
def _shard_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pixray_amd.perceptor import get_clip_perceptor
        perc = get_clip_perceptor("tiny-SLIP/16", DEV, max_batch=2, precision="f32", group=dist.group.WORLD)
        g = torch.Generator().manual_seed(21)
        cut = torch.rand(4, 3, 224, 224, generator=g) * 1.4 - 0.2
        gout = torch.randn(4, perc.output_dim, generator=g)
        mine = cut[2 * rank:2 * rank + 2].to(DEV).requires_grad_(True)
        e = perc.encode_image(mine)
        (gc,) = torch.autograd.grad(e, mine, gout[2 * rank:2 * rank + 2].to(DEV))
        q.put((rank, e.detach().cpu(), gc.cpu()))
    finally:
        dist.destroy_process_group()


def test_sharded_slip_gradient_equals_the_unsharded_one():
    """two processes on one device, each with half of the cutouts (the pattern of tests/test_comm_gpu.py): the batch-global
    min / max and the four backward sums are all-reduced (gloo), so embeddings and d/d cutouts equal the one-process tower's"""
    import torch.multiprocessing as mp
    from pixray_amd.perceptor import get_clip_perceptor
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + os.getpid() % 2000
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=240) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    perc = get_clip_perceptor("tiny-SLIP/16", DEV, max_batch=4, precision="f32")
    g = torch.Generator().manual_seed(21)
    cut = (torch.rand(4, 3, 224, 224, generator=g) * 1.4 - 0.2).to(DEV).requires_grad_(True)
    gout = torch.randn(4, perc.output_dim, generator=g).to(DEV)
    e = perc.encode_image(cut)
    (gc,) = torch.autograd.grad(e, cut, gout)
    es, gs = torch.cat([t[1] for t in got]), torch.cat([t[2] for t in got])
    print("sharded vs unsharded: emb", rel_l2(es, e), "grad", rel_l2(gs, gc))
    assert rel_l2(es, e) < 1e-6 and rel_l2(gs, gc) < 1e-5
