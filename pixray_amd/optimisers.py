"""The six update rules of `--optimiser` (pixray.py:520-555 `rebuild_optimisers`): Adam, AdamW, Adagrad, Adamax (`torch.optim`),
DiffGrad, AdamP (`torch_optimizer` 0.1.0), each constructed with `lr` alone as the reference does.

On a device every rule is one fused HIP kernel with `clip_z` inside (csrc/optim.hip; two launches for AdamP; plain Adam keeps
`engine.HipAdam` on csrc/elementwise.hip) that reads its step-dependent scalars from device memory, so `Session.enable_graph()` can
capture and replay the step.  On the host the four `torch.optim` rules are torch's own; DiffGrad and AdamP are the small classes below.

DiffGrad and AdamP are restated from the published algorithms (Dubey et al., "diffGrad: An Optimization Method for Convolutional
Neural Networks", 2019; Heo et al., "AdamP: Slowing Down the Slowdown for Momentum Optimizers on Scale-invariant Weights", ICLR
2021) in the form `torch_optimizer` gives them: parity with that package is unpinned (it is not installed where this was written)."""
from __future__ import annotations

import math

import torch

OPTIMISERS = ("Adam", "AdamW", "Adagrad", "Adamax", "DiffGrad", "AdamP")


def check_name(name: str) -> str:
    if name not in OPTIMISERS:
        raise ValueError(f"unknown optimiser {name!r}: --optimiser takes one of {', '.join(OPTIMISERS)}")
    return name


# ------------------------------------------------------------------------------------------------ device: fused HIP kernels
class HipOptimiser(torch.optim.Optimizer):
    """What the fused rules share with `engine.HipAdam`: `prepare_step()` advances t and stages the step scalars through a ring
    of pinned buffers into one fixed device tensor, `step()` launches the same kernel with the same arguments every iteration
    (replayable from a captured hipGraph), `clamped_last_step` tells the session whether clip_z ran inside the kernel, and
    `state[p]["step"]` follows `_t` (state set from outside, e.g. teacher-forced moments, is followed instead).  fp32 tensors."""
    state_names = ()

    def __init__(self, params, defaults, bounds=None):
        super().__init__(list(params), defaults)
        self.bounds = bounds   # (zmin[C], zmax[C]) or None
        self._t = 0
        self._pending = False
        p = self.param_groups[0]["params"][0]
        from .cutouts import PinnedRing
        self._ring = PinnedRing((4,), torch.float32, p.device) if p.is_cuda else None
        self._hyper = self._ring.dev if self._ring is not None else torch.zeros(4, dtype=torch.float32, device=p.device)
        self.clamped_last_step = False

    def _scalars(self, group, t):
        """the rule's hyper[0..] at step t (include/prx.h), computed in double"""
        raise NotImplementedError

    def _launch(self, p, st, grad, zmin, zmax, group):
        raise NotImplementedError

    def _new_state(self, p):
        return {name: torch.zeros_like(p) for name in self.state_names}

    def prepare_step(self):
        """host side of the next step(): advance t and stage the rule's scalars (stream-ordered H2D)"""
        self._t += 1
        vals = list(self._scalars(self.param_groups[0], self._t))
        vals = torch.tensor(vals + [0.0] * (4 - len(vals)), dtype=torch.float32)
        if self._ring is not None:
            self._ring.stage(vals)       # the host may be iterations ahead of the queued H2D copies
        else:
            self._hyper.copy_(vals)      # host tensors: the kernels' CPU emulation (tests)
        self._pending = True

    @torch.no_grad()
    def step(self, closure=None):
        if not self._pending:
            self.prepare_step()
        self._pending = False
        self.clamped_last_step = False
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st.update(self._new_state(p))
                elif int(st["step"]) != self._t - 1:
                    self._t = int(st["step"])        # state was set from outside: follow its step count
                    self.prepare_step()
                    self._pending = False
                st["step"] = self._t
                zmin, zmax = self.bounds if self.bounds is not None else (None, None)
                self._launch(p, st, p.grad.contiguous(), zmin, zmax, group)
                self.clamped_last_step = zmin is not None


class _HipElementwise(HipOptimiser):
    rule = None

    def _launch(self, p, st, grad, zmin, zmax, group):
        from . import ops
        ops.optim_step_dev(self.rule, p, [st[n] for n in self.state_names], grad, zmin, zmax, self._hyper,
                           group.get("betas", (0.0, 0.0)), group["eps"])


class HipAdamW(_HipElementwise):
    """`optim.AdamW([z], lr)` (pixray.py:541)"""
    rule, state_names = "AdamW", ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=0.2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, bounds=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), bounds)

    def _scalars(self, g, t):
        b1, b2 = g["betas"]
        return g["lr"] / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t), 1.0 - g["lr"] * g["weight_decay"]


class HipAdagrad(_HipElementwise):
    """`optim.Adagrad([z], lr)` (pixray.py:543): lr_decay 0, accumulator from 0"""
    rule, state_names = "Adagrad", ("sum",)

    def __init__(self, params, lr=0.5, eps=1e-10, bounds=None):
        super().__init__(params, dict(lr=lr, eps=eps), bounds)

    def _scalars(self, g, t):
        return (g["lr"],)


class HipAdamax(_HipElementwise):
    """`optim.Adamax([z], lr)` (pixray.py:545)"""
    rule, state_names = "Adamax", ("exp_avg", "exp_inf")

    def __init__(self, params, lr=0.5, betas=(0.9, 0.999), eps=1e-8, bounds=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps), bounds)

    def _scalars(self, g, t):
        return (g["lr"] / (1.0 - g["betas"][0] ** t),)


class HipDiffGrad(_HipElementwise):
    """`DiffGrad([z], lr)` (pixray.py:547)"""
    rule, state_names = "DiffGrad", ("exp_avg", "exp_avg_sq", "previous_grad")

    def __init__(self, params, lr=2.0, betas=(0.9, 0.999), eps=1e-8, bounds=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps), bounds)

    def _scalars(self, g, t):
        b1, b2 = g["betas"]
        return (g["lr"] * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t),)


class HipAdamP(HipOptimiser):
    """`AdamP([z], lr)` (pixray.py:549): weight decay 0, nesterov off.  The projection's dot products are per-workgroup partials
    added in a fixed order (no atomics): the step is bit-reproducible."""
    state_names = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=2.0, betas=(0.9, 0.999), eps=1e-8, delta=0.1, bounds=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, delta=delta), bounds)
        self._scratch = {}

    def _scalars(self, g, t):
        b1, b2 = g["betas"]
        return g["lr"] / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)

    def _launch(self, p, st, grad, zmin, zmax, group):
        from . import ops
        if p not in self._scratch:
            self._scratch[p] = ops.adamp_scratch(p)
        ops.adamp_step_dev(p, st["exp_avg"], st["exp_avg_sq"], grad, zmin, zmax, self._hyper, self._scratch[p], group["betas"],
                           group["eps"], group["delta"])


# ------------------------------------------------------------------------------------------------ host: plain torch
class DiffGrad(torch.optim.Optimizer):
    """diffGrad on host tensors: Adam's moments, the step scaled by dfc = sigmoid(|g_prev - g|); eps is added to sqrt(v) before
    the bias correction.  weight_decay 0."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))

    @torch.no_grad()
    def step(self, closure=None):
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                g, st = p.grad, self.state[p]
                if not st:
                    st.update(step=0, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p), previous_grad=torch.zeros_like(p))
                st["step"] += 1
                st["exp_avg"].mul_(b1).add_(g, alpha=1 - b1)
                st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1 - b2)
                dfc = 1.0 / (1.0 + torch.exp(-(st["previous_grad"] - g).abs()))
                st["previous_grad"] = g.clone()
                step_size = group["lr"] * math.sqrt(1 - b2 ** st["step"]) / (1 - b1 ** st["step"])
                p.addcdiv_(st["exp_avg"] * dfc, st["exp_avg_sq"].sqrt().add_(group["eps"]), value=-step_size)


class AdamP(torch.optim.Optimizer):
    """AdamP on host tensors: Adam's update with its component along p removed when the gradient is (nearly) orthogonal to p,
    tested per row of the [shape[0], -1] view and then on the whole tensor.  weight_decay 0, nesterov off."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, delta=0.1):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, delta=delta))

    @staticmethod
    def _project(p, g, perturb, delta, eps):
        for rows in (p.shape[0], 1):
            pv, gv = p.reshape(rows, -1), g.reshape(rows, -1)
            cos = (gv * pv).sum(1).abs() / (gv.norm(dim=1) * pv.norm(dim=1) + eps)
            if cos.max() < delta / math.sqrt(pv.shape[1]):
                p_n = pv / (pv.norm(dim=1, keepdim=True) + eps)
                q = perturb.reshape(rows, -1)
                return (q - p_n * (p_n * q).sum(1, keepdim=True)).reshape(p.shape)
        return perturb

    @torch.no_grad()
    def step(self, closure=None):
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                g, st = p.grad, self.state[p]
                if not st:
                    st.update(step=0, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))
                st["step"] += 1
                st["exp_avg"].mul_(b1).add_(g, alpha=1 - b1)
                st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1 - b2)
                perturb = st["exp_avg"] / (st["exp_avg_sq"].sqrt() / math.sqrt(1 - b2 ** st["step"]) + group["eps"])
                if p.dim() > 1:
                    perturb = self._project(p, g, perturb, group["delta"], group["eps"])
                p.add_(perturb, alpha=-group["lr"] / (1 - b1 ** st["step"]))


_HIP = {"AdamW": HipAdamW, "Adagrad": HipAdagrad, "Adamax": HipAdamax, "DiffGrad": HipDiffGrad, "AdamP": HipAdamP}
_HOST = {"Adam": torch.optim.Adam, "AdamW": torch.optim.AdamW, "Adagrad": torch.optim.Adagrad, "Adamax": torch.optim.Adamax,
         "DiffGrad": DiffGrad, "AdamP": AdamP}


def make_optimiser(name, params, lr, bounds=None):
    """The optimiser `--optimiser name` stands for, over `params` at `lr` (every other setting the rule's default, as in the
    reference).  Device tensors get the fused HIP classes (`bounds`: clip_z inside the kernel); host tensors the plain-torch ones,
    which leave clip_z to the drawer."""
    check_name(name)
    params = list(params)
    if all(p.is_cuda for p in params):
        if name == "Adam":
            from .engine import HipAdam
            return HipAdam(params, lr=lr, bounds=bounds)
        return _HIP[name](params, lr=lr, bounds=bounds)
    return _HOST[name](params, lr=lr)
