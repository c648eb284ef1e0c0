"""The fused `--optimiser` kernels (csrc/optim.hip through pixray_amd/optimisers.py) on the device: every rule against the same
rule in float64, AdamP's two branches, bit-reproducibility, and hipGraph replay of a VQGAN session.  The `check_*` bodies are
also run on the kernels' CPU emulation by tests/test_optimisers_cpu.py (DEV = "cpu" there).

Yardsticks: `torch.optim` for AdamW / Adagrad / Adamax; for DiffGrad and AdamP the restatements below, written from the published
formulas and independent of pixray_amd.  The gate of every comparison: the kernel's max-abs distance from the float64 run is at
most GATE x the distance of the float32 run of the SAME yardstick from its float64 run, computed here on the same inputs (the
kernel may contract to FMAs and order the arithmetic differently; it may not be a different formula)."""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

pytestmark = pytest.mark.gpu
DEV = "cuda"
GATE = 4.0
STEPS = 10
LR = {"AdamW": 0.2, "Adagrad": 0.5, "Adamax": 0.5, "DiffGrad": 2.0, "AdamP": 2.0}     # the reference's hints (pixray.py:541-549)
STATES = {"AdamW": ("exp_avg", "exp_avg_sq"), "Adagrad": ("sum",), "Adamax": ("exp_avg", "exp_inf"),
          "DiffGrad": ("exp_avg", "exp_avg_sq", "previous_grad"), "AdamP": ("exp_avg", "exp_avg_sq")}
SHAPES = {"z256": (1, 256, 16, 16), "odd": (1, 5, 7, 9), "rows4": (4, 6, 8, 10)}


# ------------------------------------------------------------------------------------------------ yardsticks
class RefDiffGrad:
    """diffGrad (Dubey et al. 2019) as torch_optimizer states it: betas 0.9 / 0.999, eps 1e-8, no weight decay"""

    def __init__(self, p, lr):
        self.p, self.lr, self.t = p, lr, 0
        self.state = dict(exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p), previous_grad=torch.zeros_like(p))

    def step(self, g):
        b1, b2, eps, s = 0.9, 0.999, 1e-8, self.state
        self.t += 1
        s["exp_avg"] = b1 * s["exp_avg"] + (1 - b1) * g
        s["exp_avg_sq"] = b2 * s["exp_avg_sq"] + (1 - b2) * g * g
        dfc = 1 / (1 + torch.exp(-(s["previous_grad"] - g).abs()))
        s["previous_grad"] = g.clone()
        step_size = self.lr * math.sqrt(1 - b2 ** self.t) / (1 - b1 ** self.t)
        self.p -= step_size * (s["exp_avg"] * dfc) / (s["exp_avg_sq"].sqrt() + eps)


class RefAdamP:
    """AdamP (Heo et al. 2021) as torch_optimizer states it: betas 0.9 / 0.999, eps 1e-8, delta 0.1, no weight decay, no nesterov.
    `log` keeps, per step, the view that projected (0 none, 1 channel, 2 layer) and each view's (max cosine, threshold)."""

    def __init__(self, p, lr):
        self.p, self.lr, self.t, self.log = p, lr, 0, []
        self.state = dict(exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))

    def step(self, g):
        b1, b2, eps, delta, s, p = 0.9, 0.999, 1e-8, 0.1, self.state, self.p
        self.t += 1
        s["exp_avg"] = b1 * s["exp_avg"] + (1 - b1) * g
        s["exp_avg_sq"] = b2 * s["exp_avg_sq"] + (1 - b2) * g * g
        perturb = s["exp_avg"] / (s["exp_avg_sq"].sqrt() / math.sqrt(1 - b2 ** self.t) + eps)
        took, seen = 0, []
        if p.dim() > 1:
            for view, rows in ((1, p.shape[0]), (2, 1)):
                pv, gv, qv = p.reshape(rows, -1), g.reshape(rows, -1), perturb.reshape(rows, -1)
                cos = ((gv * pv).sum(1).abs() / (gv.norm(dim=1) * pv.norm(dim=1) + eps)).max().item()
                thr = delta / math.sqrt(pv.shape[1])
                seen.append((cos, thr))
                if cos < thr:
                    p_n = pv / (pv.norm(dim=1, keepdim=True) + eps)
                    perturb = (qv - p_n * (p_n * qv).sum(1, keepdim=True)).reshape(p.shape)
                    took = view
                    break
        self.log.append((took, seen))
        self.p -= self.lr / (1 - b1 ** self.t) * perturb


class _TorchRef:
    def __init__(self, cls, p, lr):
        self.p = p
        self.opt = cls([p], lr=lr)

    def step(self, g):
        self.p.grad = g
        self.opt.step()

    @property
    def state(self):
        return self.opt.state[self.p]


def make_ref(rule, p, lr):
    if rule == "DiffGrad":
        return RefDiffGrad(p, lr)
    if rule == "AdamP":
        return RefAdamP(p, lr)
    return _TorchRef(getattr(torch.optim, rule), p, lr)


def run_ref(rule, z0, grads, bounds, dtype, lr):
    """`grads`: a list of fp32 gradients, or a function (step, p) -> gradient that is evaluated on THIS run's p (float64 runs of
    the branch cases build their gradients from the current p; the rounded list is then replayed everywhere else)"""
    p = z0.to(dtype).clone()
    ref = make_ref(rule, p, lr)
    used = []
    with torch.no_grad():
        for t in range(STEPS):
            g = grads(t, p) if callable(grads) else grads[t]
            g = g.to(torch.float32)
            used.append(g)
            ref.step(g.to(dtype))
            if bounds is not None:
                zmin, zmax = (b.to(dtype)[None, :, None, None] for b in bounds)
                p.copy_(p.maximum(zmin).minimum(zmax))
    return ref, used


def run_kernel(rule, z0, grads, bounds, lr):
    from pixray_amd import optimisers
    z = z0.to(DEV).clone().requires_grad_(True)
    dev_bounds = tuple(b.to(DEV) for b in bounds) if bounds is not None else None
    opt = optimisers._HIP[rule]([z], lr=lr, bounds=dev_bounds)
    for g in grads:
        z.grad = g.to(DEV)
        opt.step()
        assert opt.clamped_last_step == (bounds is not None)
    if DEV != "cpu":
        torch.cuda.synchronize()
    assert opt._t == STEPS and int(opt.state[z]["step"]) == STEPS
    return z.detach().cpu(), {k: opt.state[z][k].cpu() for k in STATES[rule]}


def gated_compare(rule, z0, grads, bounds, label):
    lr = LR[rule]
    ref64, used = run_ref(rule, z0, grads, bounds, torch.float64, lr)
    ref32, _ = run_ref(rule, z0, used, bounds, torch.float32, lr)
    z, states = run_kernel(rule, z0, used, bounds, lr)
    worst = 0.0
    for name, mine, r32, r64 in [("z", z, ref32.p, ref64.p)] + [(k, states[k], ref32.state[k], ref64.state[k]) for k in STATES[rule]]:
        own = (r32.double() - r64).abs().max().item()
        dist = (mine.double() - r64).abs().max().item()
        ratio = dist / own if own > 0 else (0.0 if dist == 0 else float("inf"))
        print(f"{rule:8s} {label:24s} {name:14s} kernel-f64 {dist:.3e}  yardstick f32-f64 {own:.3e}  ratio {ratio:.2f}")
        assert dist <= GATE * own, (rule, label, name, dist, own)
        worst = max(worst, ratio)
    return ref64, worst


def seeded_case(shape_name, with_bounds, seed=3):
    shape = SHAPES[shape_name]
    g = torch.Generator().manual_seed(seed)
    z0 = torch.randn(*shape, generator=g)
    bounds = None
    if with_bounds:                      # as tests/test_path_gpu.py::test_adam_clamp_vs_torch
        bounds = (-torch.rand(shape[1], generator=g) - 0.5, torch.rand(shape[1], generator=g) + 0.5)
    grads = [torch.randn(*shape, generator=g) for _ in range(STEPS)]
    return z0, grads, bounds


# ------------------------------------------------------------------------------------------------ bodies (device and emulation)
def check_rule_against_float64(rule, shape_name, with_bounds):
    z0, grads, bounds = seeded_case(shape_name, with_bounds)
    ref64, _ = gated_compare(rule, z0, grads, bounds, f"{shape_name}{'+bounds' if with_bounds else ''}")
    if rule == "AdamP":                  # how far the seeded gradients keep from the decision threshold (1.0 = on it)
        print("         AdamP decisions:", [(took, [round(c / t, 3) for c, t in seen]) for took, seen in ref64.log])


def _rows(x, rows):
    return x.reshape(rows, -1)


def grad_aligned(t, p):
    """g = p + small noise: |cos| near 1, far above delta / sqrt(dim) in every view"""
    noise = torch.randn(p.shape, generator=torch.Generator().manual_seed(100 + t), dtype=torch.float64)
    return p + 0.05 * noise


def grad_orthogonal(t, p):
    """noise with its component along p removed row by row (float64): the channel view projects"""
    r = torch.randn(p.shape, generator=torch.Generator().manual_seed(200 + t), dtype=torch.float64)
    rv, pv = _rows(r, p.shape[0]), _rows(p, p.shape[0])
    return (rv - pv * ((rv * pv).sum(1, keepdim=True) / (pv * pv).sum(1, keepdim=True))).reshape(p.shape)


def grad_layer_only(t, p):
    """orthogonal to p as a whole, but rows 0 and 1 carry +c and -c of it along their own p rows: the channel view sees a
    cosine of about 0.45 there, the layer view sees none"""
    r = torch.randn(p.shape, generator=torch.Generator().manual_seed(300 + t), dtype=torch.float64)
    r = r - p * ((r * p).sum() / (p * p).sum())
    rv, pv = _rows(r, p.shape[0]).clone(), _rows(p, p.shape[0])
    c = 0.5 * rv[0].norm() * pv[0].norm()
    rv[0] += c / (pv[0] * pv[0]).sum() * pv[0]
    rv[1] -= c / (pv[1] * pv[1]).sum() * pv[1]
    return rv.reshape(p.shape)


def check_adamp_branches():
    """both outcomes of AdamP's projection test, each at least 10x away from the threshold on the float64 yardstick at every step"""
    took = {}
    for shape_name, with_bounds, name, fn in (("z256", True, "aligned", grad_aligned), ("z256", True, "orthogonal", grad_orthogonal),
                                              ("rows4", False, "aligned", grad_aligned), ("rows4", False, "orthogonal", grad_orthogonal),
                                              ("rows4", False, "layer_only", grad_layer_only)):
        z0, _, bounds = seeded_case(shape_name, with_bounds, seed=11)
        ref64, _ = gated_compare("AdamP", z0, fn, bounds, f"{shape_name} {name}")
        for view, seen in ref64.log:
            if name == "aligned":
                assert view == 0 and all(c >= 10 * thr for c, thr in seen), (name, view, seen)
            elif name == "orthogonal":
                assert view == 1 and seen[0][0] * 10 <= seen[0][1], (name, view, seen)
            else:
                assert view == 2 and seen[0][0] >= 10 * seen[0][1] and seen[1][0] * 10 <= seen[1][1], (name, view, seen)
        took[(shape_name, name)] = {view for view, _ in ref64.log}
    assert took[("z256", "aligned")] == {0} and took[("z256", "orthogonal")] == {1} and took[("rows4", "layer_only")] == {2}


def check_adamp_bit_reproducible():
    """the same 10 AdamP steps twice from the same state (the projecting branch, whose dot products are reductions)"""
    for shape_name, fn in (("z256", grad_orthogonal), ("rows4", grad_layer_only)):
        z0, _, bounds = seeded_case(shape_name, shape_name == "z256", seed=11)
        _, used = run_ref("AdamP", z0, fn, bounds, torch.float64, LR["AdamP"])
        z1, s1 = run_kernel("AdamP", z0, used, bounds, LR["AdamP"])
        z2, s2 = run_kernel("AdamP", z0, used, bounds, LR["AdamP"])
        assert torch.equal(z1, z2) and all(torch.equal(s1[k], s2[k]) for k in s1)
        assert not torch.equal(z1, z0)


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("with_bounds", [True, False], ids=["bounds", "free"])
@pytest.mark.parametrize("shape_name", list(SHAPES))
@pytest.mark.parametrize("rule", list(LR))
def test_rule_against_float64(rule, shape_name, with_bounds):
    check_rule_against_float64(rule, shape_name, with_bounds)


def test_adamp_branches():
    check_adamp_branches()


def test_adamp_bit_reproducible():
    check_adamp_bit_reproducible()


@pytest.mark.parametrize("rule", ["AdamP", "Adamax"])
def test_graph_replay_matches_eager_session(tmp_path, rule):
    """a small VQGAN session stepping with a fused rule: the captured iteration replays with each step's scalars (and, for
    AdamP, its scratch buffer) and stays bit-equal to an eager session over eight iterations; cutout noise is off (the device
    randn streams of capture and eager differ)"""
    from pixray_amd import frontend as fe
    from pixray_amd import optimisers

    def build(name):
        run = fe.Run()
        run.settings = dict(drawer="vqgan", vqgan_model="tiny_f4", clip_models="tiny-B/32", size=[64, 64], num_cuts=8, iterations=12,
                            save_every=100, display_every=100, outdir=str(tmp_path / name), seed=3, skip_args=True, init_noise="none",
                            vector_prompts="none", noise_prompt_seeds=[1, 2], noise_prompt_weights=[1.0, 0.5], precision="fp16",
                            learning_rate_drops=[], optimiser=rule, learning_rate=LR[rule])
        sess = fe.do_init(fe.apply_settings(run=run), run)
        for mk in sess.cutoutsTable.values():
            mk.noise_fac = 0.0
        return sess
    a, b = build("eager"), build("graph")
    assert type(a.opts[0]) is optimisers._HIP[rule] and type(b.opts[0]) is optimisers._HIP[rule]
    assert torch.equal(a.drawer.get_z(), b.drawer.get_z())
    assert b.enable_graph(warmup=2), b.graph_error
    assert b._graph is not None and type(b.opts[0]) is optimisers._HIP[rule]
    for it in range(2):
        a.train(it)
    for it in range(2, 10):
        a.train(it)
        b.train(it)
        assert torch.equal(a.drawer.get_z(), b.drawer.get_z()), it
        assert all(torch.equal(x, y) for x, y in zip(a.last_losses, b.last_losses)), it
    assert b._graph is not None and a.opts[0]._t == b.opts[0]._t == 10
    assert a.opts[0].clamped_last_step and b.opts[0].clamped_last_step
