"""torch.autograd.Function wrappers over the C ABI (include/prx.h).

Every op here enqueues HIP kernels on torch's current stream and returns real torch tensors with
a `grad_fn`, so unmodified reference plugins (`LossInterface.get_loss`, `FilterInterface.forward`,
custom drawers) compose with them through ordinary autograd.  There is no CPU
path: tensors must live on a ROCm device and the shared library must be built.
"""
from __future__ import annotations

import ctypes
from typing import Sequence

import torch

from . import _lib
from ._lib import PrxError, call, precision_code


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise PrxError("pixray_amd ops run on an MI355X only (got a CPU tensor); there is no CPU fallback")


def _stream():
    return _lib.current_stream()


_DEFERRED_DESTROY = []


def _destroy_handle(fn_name: str, h) -> None:
    """`prx_*_destroy` frees device memory (hipFree), which a hipGraph capture in progress does not survive: a handle whose
    last reference drops during a capture (an autograd ctx released by the captured backward, the garbage collector) is
    parked and destroyed by the next handle destruction outside a capture (or at interpreter exit with the process)."""
    try:
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
    except Exception:
        capturing = False
    if capturing:
        _DEFERRED_DESTROY.append((fn_name, h))
        return
    lib = _lib.load()
    while _DEFERRED_DESTROY:
        n, hh = _DEFERRED_DESTROY.pop()
        getattr(lib, n)(hh)
    getattr(lib, fn_name)(h)


def _weight_array(tensors: Sequence[torch.Tensor]):
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
            raise PrxError("weights must be contiguous fp32 device tensors")
        arr[i] = t.data_ptr()
    return arr


def _keep(obj, arr):
    obj._arr = arr   # keep the ctypes array alive for the duration of the call
    return ctypes.addressof(arr)


class _Handle:
    """Base of the runner handles.  `h` is the C handle (a ctypes.c_void_p, or the bare pointer `prx_fft_drawer_create` returns);
    `_destroy` names the `prx_*_destroy` that frees it with all its device memory (csrc/dev_arena.h); `_arr` is the ctypes array of
    weight pointers, `_keep`ed for the create call."""
    _destroy = None
    _arr = None
    h = None

    def __del__(self):
        h, self.h = self.h, None
        if getattr(h, "value", h):
            try:
                _destroy_handle(self._destroy, h)
            except Exception:
                pass


class _EngineHandle(_Handle):
    """A runner handle on the GEMM engine (csrc/runner_core.h RunnerEngine): `abi` is the prefix of its exported functions, and
    `gemm_ctx` the `prx_gemm_ctx` it owns (tile overrides, timing log)."""
    abi = None

    @property
    def gemm_ctx(self):
        return getattr(_lib.load(), self.abi + "_gemm_ctx")(self.h)


class _ImageTowerHandle(_EngineHandle):
    """An image tower behind `clip_encode_image`: `<abi>_minmax / _encode / _backward_reduce / _backward_finish / _gemm_ctx / _destroy`
    (csrc/runner_core.h ImageTower).  A subclass prepares its weights and its config struct and hands them to `_create`."""

    def _create(self, fn_name, cfg_struct, weights, *extra, cfg, device):
        """`fn_name(&h, &cfg_struct, *extra, weights, n, stream)`; `cfg_struct` carries max_batch and the precision code"""
        self.precision = cfg_struct.precision
        h = ctypes.c_void_p()
        call(fn_name, ctypes.addressof(h), ctypes.addressof(cfg_struct), *extra, _keep(self, _weight_array(weights)), len(weights), _stream())
        torch.cuda.synchronize(device)   # weight tensors may now be released
        self.h = h
        self.cfg = cfg
        self.max_batch = cfg_struct.max_batch
        self.device = device
        self.generation = 0              # bumped by every forward: the handle keeps ONE forward's activations (_ClipEncodeFn)


# --------------------------------------------------------------------------------------- cutouts
class _MakeCutoutsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, desc, noise, S, base_hw, spot_mask):
        _need_cuda(img, desc, noise, spot_mask)
        assert img.dim() == 4 and img.shape[0] == 1 and img.shape[1] == 3, "MakeCutouts expects [1,3,H,W]"
        img = img.contiguous().float()
        n = desc.shape[0]
        H, W = img.shape[2], img.shape[3]
        Hb, Wb = base_hw
        dev = img.device
        pooled = torch.empty(3, S, S, device=dev)
        argmax = torch.empty(3, S, S, device=dev, dtype=torch.int32)
        base = torch.empty(3, Hb, Wb, device=dev) if (Hb, Wb) != (S, S) else None
        stage_a = torch.empty(n, 3, Hb, Wb, device=dev)
        out = torch.empty(n, 3, S, S, device=dev)
        if spot_mask is not None:
            spot_mask = spot_mask.to(torch.uint8).contiguous()
            assert spot_mask.shape == (3, S, S), f"spot mask must be [3,{S},{S}]"
        call("prx_cutouts_forward", img, H, W, desc, noise, spot_mask, n, S, Hb, Wb, pooled, argmax, base, stage_a, out, _stream())
        ctx.save_for_backward(desc, argmax, stage_a)
        ctx.spot_mask = spot_mask
        ctx.geom = (n, S, Hb, Wb, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        desc, argmax, stage_a = ctx.saved_tensors
        n, S, Hb, Wb, H, W = ctx.geom
        g = g.contiguous().float()
        dev = g.device
        g_a = torch.empty(n, 3, Hb, Wb, device=dev)
        g_priv = torch.empty(n, 3, Hb, Wb, device=dev)
        uv = torch.empty(n, Hb * Wb, 2, device=dev)
        g_base = torch.empty(3, Hb, Wb, device=dev)
        g_pooled = torch.empty(3, S, S, device=dev)
        g_img = torch.empty(1, 3, H, W, device=dev)
        call("prx_cutouts_backward", g, desc, ctx.spot_mask, n, S, Hb, Wb, H, W, stage_a, argmax, g_a, g_priv, uv, g_base, g_pooled,
             g_img, _stream())
        return g_img, None, None, None, None, None


def make_cutouts(img, desc, noise, S, base_hw=None, spot_mask=None):
    """`base_hw`: size of the aspect-rescaled pooled image ((S, S) on a square canvas; pixray_amd.cutouts.base_size);
    `spot_mask`: bool/uint8 [3,S,S], pooled pixels to blank (spot prompts, pixray.py:453-466)."""
    return _MakeCutoutsFn.apply(img, desc, noise, S, tuple(base_hw) if base_hw is not None else (S, S), spot_mask)


# --------------------------------------------------------------------------------------- CLIP ViT
def _weights_in_abi_order(params, shapes, device, what):
    """the C ABI takes bare device pointers in a documented order (include/prx.h): a missing tensor or one whose shape is not the
    one the configuration implies would be read out of bounds on the device, so both are refused here by name"""
    ws = []
    for name, shape in shapes.items():
        if name not in params:
            raise KeyError(f"{what}: the weights have no tensor named {name!r}")
        t = params[name]
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, the configuration implies {tuple(shape)}")
        ws.append(t.to(device=device, dtype=torch.float32).contiguous())
    return ws


class ClipVitHandle(_ImageTowerHandle):
    """Owns a `prx_clip_vit` (packed weights + activation workspace for `max_batch` cutouts, allocated at create time; an allocation
    that fails raises PrxError with the bytes asked for and held, and the partly built handle is freed).
    `precision`: "fp16" (default) / "bf16" (fast paths) or "f32" (exact-f32 MFMA parity mode, include/prx.h PRX_PREC_*)."""
    _destroy = "prx_clip_vit_destroy"
    abi = "prx_clip_vit"

    def __init__(self, cfg, params, max_batch: int, device, precision=None):
        from .weights import clip_vit_param_shapes
        ws = _weights_in_abi_order(params, clip_vit_param_shapes(cfg), device, f"CLIP ViT {getattr(cfg, 'name', '')}")
        c = _ClipCfg(cfg.input_resolution, cfg.patch_size, cfg.width, cfg.layers, cfg.heads, cfg.output_dim, max_batch, precision_code(precision))
        self._create("prx_clip_vit_create", c, ws, cfg=cfg, device=device)


class _VitTowerCfg(ctypes.Structure):
    """mirror of `prx_vit_tower_config` (include/prx.h)"""
    _fields_ = [(n, ctypes.c_int) for n in ("input_resolution", "patch_size", "width", "layers", "heads", "output_dim", "max_batch",
                                            "precision", "family", "head_dim")] + \
               [("ln_eps", ctypes.c_float), ("mean", ctypes.c_float * 3), ("std", ctypes.c_float * 3)]


VIT_FAMILY_CLIP, VIT_FAMILY_SLIP, VIT_FAMILY_OPENCLIP = 0, 1, 2


class SlipVitHandle(ClipVitHandle):
    """A `prx_clip_vit` made by `prx_vit_tower_create` for the SLIP family (timm VisionTransformer + image_projection): the same
    handle type and protocol as ClipVitHandle (minmax / encode / backward_reduce / backward_finish / gemm_ctx / destroy)."""

    def __init__(self, cfg, params, max_batch: int, device, precision=None):
        from .weights import IMAGENET_MEAN, IMAGENET_STD, slip_vit_param_shapes
        ws = _weights_in_abi_order(params, slip_vit_param_shapes(cfg), device, f"SLIP ViT {getattr(cfg, 'name', '')}")
        c = _VitTowerCfg(cfg.input_resolution, cfg.patch_size, cfg.width, cfg.layers, cfg.heads, cfg.output_dim, max_batch, precision_code(precision),
                         VIT_FAMILY_SLIP, cfg.head_dim, cfg.ln_eps, (ctypes.c_float * 3)(*IMAGENET_MEAN), (ctypes.c_float * 3)(*IMAGENET_STD))
        self._create("prx_vit_tower_create", c, ws, cfg=cfg, device=device)


class OpenClipVitHandle(ClipVitHandle):
    """A `prx_clip_vit` made by `prx_vit_tower_create` for the OpenCLIP (LAION) family: CLIP's tensors and switches with the exact
    GELU; heads of 80 (ViT-H-14) and 88 (ViT-g-14) are zero-padded to 96 columns by the runner and run on the 96-wide attention kernels,
    heads of 104 (ViT-bigG-14) to 128 columns on the 128-wide ones.  A configuration whose MLP is not 4 x width (`cfg.mlp_width`) goes
    through `prx_vit_tower_create_mlp`."""

    def __init__(self, cfg, params, max_batch: int, device, precision=None):
        from .perceptor import ClipVitPerceptor
        from .weights import clip_vit_param_shapes
        ws = _weights_in_abi_order(params, clip_vit_param_shapes(cfg), device, f"OpenCLIP ViT {getattr(cfg, 'name', '')}")
        c = _VitTowerCfg(cfg.input_resolution, cfg.patch_size, cfg.width, cfg.layers, cfg.heads, cfg.output_dim, max_batch, precision_code(precision),
                         VIT_FAMILY_OPENCLIP, cfg.head_dim, 1e-5, (ctypes.c_float * 3)(*ClipVitPerceptor.CLIP_MEAN),
                         (ctypes.c_float * 3)(*ClipVitPerceptor.CLIP_STD))
        if getattr(cfg, "mlp_width", 0):
            self._create("prx_vit_tower_create_mlp", c, ws, int(cfg.mlp_width), cfg=cfg, device=device)
        else:
            self._create("prx_vit_tower_create", c, ws, cfg=cfg, device=device)


class _ClipResNetCfg(ctypes.Structure):
    _fields_ = [("input_resolution", ctypes.c_int), ("width", ctypes.c_int), ("layers", ctypes.c_int * 4), ("heads", ctypes.c_int),
                ("output_dim", ctypes.c_int), ("max_batch", ctypes.c_int), ("precision", ctypes.c_int)]


class ClipResNetHandle(_ImageTowerHandle):
    """Owns a `prx_clip_resnet` (CLIP ModifiedResNet tower: RN50, RN101, RN50x4, RN50x16, RN50x64); same protocol as ClipVitHandle.
    `params` is the OpenAI `visual.*` state dict (BatchNorm un-folded); the fold happens here.

    The runner allocates one forward's activations (and the backward's gradient streams) for `max_batch` cutouts when it is created.
    For RN50x64 at 448 x 448 that is 599 467 264 bytes (572 MiB) per cutout with IEEE-half operands (the default), 1 129 325 824
    (1077 MiB) with bf16 and 1 636 394 240 (1561 MiB) in the exact-f32 mode, beside 1.7 GB (half) of packed weights: 35.7 GiB at
    max_batch = 64 in the default mode.  RN50x16 at 384 x 384 takes 262 / 470 / 683 MiB per cutout.  An allocation that fails raises
    PrxError with the bytes asked for and the bytes held so far; the partly built handle is freed and the process goes on."""
    _destroy = "prx_clip_resnet_destroy"
    abi = "prx_clip_resnet"

    def __init__(self, cfg, params, max_batch: int, device, precision=None):
        from .weights import clip_resnet_param_shapes, fold_clip_resnet_params
        _weights_in_abi_order(params, clip_resnet_param_shapes(cfg), "cpu", f"CLIP ModifiedResNet {getattr(cfg, 'name', '')}")   # names / shapes only
        folded = fold_clip_resnet_params(cfg, params)
        ws = [t.to(device=device, dtype=torch.float32).contiguous() for t in folded.values()]
        c = _ClipResNetCfg()
        c.input_resolution, c.width, c.heads, c.output_dim, c.max_batch = cfg.input_resolution, cfg.width, cfg.heads, cfg.output_dim, max_batch
        c.precision = precision_code(precision)
        for i, l in enumerate(cfg.layers):
            c.layers[i] = l
        self._create("prx_clip_resnet_create", c, ws, cfg=cfg, device=device)


class _ClipConvNextCfg(ctypes.Structure):
    """mirror of `prx_clip_convnext_config` (include/prx.h)"""
    _fields_ = [("input_resolution", ctypes.c_int), ("depths", ctypes.c_int * 4), ("dims", ctypes.c_int * 4), ("output_dim", ctypes.c_int),
                ("proj_mlp", ctypes.c_int), ("ln_eps", ctypes.c_float), ("max_batch", ctypes.c_int), ("precision", ctypes.c_int)]


class ClipConvNextHandle(_ImageTowerHandle):
    """Owns a `prx_clip_convnext` (OpenCLIP ConvNeXt tower: convnext_base ... convnext_xxlarge); same protocol as ClipVitHandle.
    `params` is the open_clip `visual.*` state dict (`trunk.*`, `head.*`, the layer scale `gamma` un-folded); the fold into fc2 and
    the matrix layouts of the convolutions happen here (weights.fold_clip_convnext_params).

    The runner allocates one forward's activations and the backward's gradient streams for `max_batch` cutouts when it is created
    (weights.clip_convnext_activation_bytes: convnext_base_w at 256 x 256 takes 90.8 MiB per cutout with 16-bit operands, 155.5 MiB in the exact mode).  An
    allocation that fails raises PrxError with the bytes asked for and the bytes held so far; the partly built handle is freed."""
    _destroy = "prx_clip_convnext_destroy"
    abi = "prx_clip_convnext"

    def __init__(self, cfg, params, max_batch: int, device, precision=None):
        from .weights import clip_convnext_param_shapes, fold_clip_convnext_params
        _weights_in_abi_order(params, clip_convnext_param_shapes(cfg), "cpu", f"OpenCLIP ConvNeXt {getattr(cfg, 'name', '')}")   # names / shapes only
        folded = fold_clip_convnext_params(cfg, params)
        ws = [t.to(device=device, dtype=torch.float32).contiguous() for t in folded.values()]
        c = _ClipConvNextCfg()
        c.input_resolution, c.output_dim, c.proj_mlp, c.ln_eps = cfg.input_resolution, cfg.output_dim, int(cfg.proj == "mlp"), cfg.ln_eps
        c.max_batch, c.precision = max_batch, precision_code(precision)
        for i in range(4):
            c.depths[i], c.dims[i] = cfg.depths[i], cfg.dims[i]
        self._create("prx_clip_convnext_create", c, ws, cfg=cfg, device=device)


class _ClipCfg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("input_resolution", "patch_size", "width", "layers", "heads",
                                            "output_dim", "max_batch", "precision")]


class _VqganCfg(ctypes.Structure):
    _fields_ = [("ch", ctypes.c_int), ("ch_mult", ctypes.c_int * 8), ("n_mult", ctypes.c_int),
                ("num_res_blocks", ctypes.c_int), ("attn_resolution", ctypes.c_int), ("resolution", ctypes.c_int),
                ("z_channels", ctypes.c_int), ("embed_dim", ctypes.c_int), ("n_embed", ctypes.c_int),
                ("out_ch", ctypes.c_int), ("latent_h", ctypes.c_int), ("latent_w", ctypes.c_int), ("precision", ctypes.c_int)]


class _ClipEncodeFn(torch.autograd.Function):
    """perceptor.encode_image (slip.py:62-66) on a tower handle.

    The handle holds the activations of ONE forward (288 GB make "keep everything" cheap, but per forward).  pixray calls
    encode_image several times per iteration on the same perceptor (spot prompts pixray.py:1282-1292, image prompts
    1307-1336) before a single backward, so every forward bumps `handle.generation`, and a backward whose generation is
    no longer the handle's re-runs its forward (same cutouts, same min/max -> bit-identical activations) before it
    differentiates.  Nothing is ever differentiated through another call's activations."""

    @staticmethod
    def forward(ctx, cutouts, handle, group, comm=None, fixed_range=None):
        _need_cuda(cutouts)
        cutouts = cutouts.contiguous().float()
        n = cutouts.shape[0]
        R = handle.cfg.input_resolution
        assert cutouts.shape[1:] == (3, R, R), f"perceptor expects [n,3,{R},{R}] cutouts"
        dev = cutouts.device
        ctx.fixed_range = fixed_range is not None
        if fixed_range is not None:
            # a caller-given input range (slip.py:21-36 with input_range, or images that are already in [0, 1]): no batch min / max,
            # nothing to exchange between ranks, and no gradient through the range in the backward
            mm = torch.tensor([float(fixed_range[0]), float(fixed_range[1])], device=dev)
        else:
            mm = torch.empty(2, device=dev)
            call(handle.abi + "_minmax", handle.h, cutouts, n, mm, _stream())
        if fixed_range is None and (group is not None or comm is not None):
            # batch-global renorm couples every cutout (slip.py:21-36): min/max over all ranks -- on the C-ABI one-shot exchange
            # (csrc/comm.hip) when the session has one, else torch.distributed (RCCL)
            mm[0].neg_()
            if comm is not None:
                comm.all_reduce_(mm, "max")
            else:
                import torch.distributed as dist
                dist.all_reduce(mm, op=dist.ReduceOp.MAX, group=group)
            mm[0].neg_()
        emb = torch.empty(n, handle.cfg.output_dim, device=dev)
        call(handle.abi + "_encode", handle.h, cutouts, n, mm, emb, _stream())
        handle.generation += 1
        ctx.generation = handle.generation
        ctx.save_for_backward(cutouts, mm)
        ctx.handle = handle
        ctx.group = group
        ctx.comm = comm
        return emb

    @staticmethod
    def backward(ctx, g):
        cutouts, mm = ctx.saved_tensors
        handle = ctx.handle
        g = g.contiguous().float()
        dev = g.device
        if handle.generation != ctx.generation:
            # another forward ran on this handle since ours: restore our activations (deterministic kernels, same inputs)
            scratch = torch.empty(cutouts.shape[0], handle.cfg.output_dim, device=dev)
            call(handle.abi + "_encode", handle.h, cutouts, cutouts.shape[0], mm, scratch, _stream())
            handle.generation += 1
            ctx.generation = handle.generation
        acc = torch.empty(4, device=dev, dtype=torch.float64)
        call(handle.abi + "_backward_reduce", handle.h, cutouts, mm, g, acc, _stream())
        if ctx.fixed_range:
            acc.zero_()                       # the range is a constant of the call: no d/dmin, d/dmax terms
        elif ctx.comm is not None:
            ctx.comm.all_reduce_(acc, "sum")
        elif ctx.group is not None:
            import torch.distributed as dist
            dist.all_reduce(acc, op=dist.ReduceOp.SUM, group=ctx.group)
        gc = torch.empty_like(cutouts)
        call(handle.abi + "_backward_finish", handle.h, cutouts, mm, acc, gc, _stream())
        return gc, None, None, None, None


def clip_encode_image(cutouts, handle: ClipVitHandle, group=None, comm=None, fixed_range=None):
    """`fixed_range` = (lo, hi): renormalise with this range instead of the batch's min / max (slip.py:21-36 `input_range`)"""
    return _ClipEncodeFn.apply(cutouts, handle, group, comm, fixed_range)


class _ClipTextCfg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("vocab_size", "context_length", "width", "layers", "heads", "output_dim",
                                            "max_batch")]


class _TextTowerCfg(ctypes.Structure):
    """mirror of `prx_text_tower_config` (include/prx.h)"""
    _fields_ = _ClipTextCfg._fields_ + [("family", ctypes.c_int)]


TEXT_FAMILY_CLIP, TEXT_FAMILY_OPENCLIP = 0, 1


class ClipTextHandle(_Handle):
    """Owns a `prx_clip_text` (CLIP text transformer, forward only: CLIP_Base.encode_text, slip.py:68-70).  A configuration with
    `gelu` set (weights.OpenClipTextConfig) is built by `prx_text_tower_create` with the exact GELU in place of QuickGELU."""
    _destroy = "prx_clip_text_destroy"

    def __init__(self, cfg, params, max_batch: int, device):
        from .weights import clip_text_param_shapes
        ws = _weights_in_abi_order(params, clip_text_param_shapes(cfg), device, f"CLIP text tower {getattr(cfg, 'name', '')}")
        c = _ClipTextCfg(cfg.vocab_size, cfg.context_length, cfg.width, cfg.layers, cfg.heads, cfg.output_dim, max_batch)
        h = ctypes.c_void_p()
        if getattr(cfg, "gelu", False):
            c = _TextTowerCfg(cfg.vocab_size, cfg.context_length, cfg.width, cfg.layers, cfg.heads, cfg.output_dim, max_batch, TEXT_FAMILY_OPENCLIP)
            call("prx_text_tower_create", ctypes.addressof(h), ctypes.addressof(c), _keep(self, _weight_array(ws)), len(ws), _stream())
        else:
            call("prx_clip_text_create", ctypes.addressof(h), ctypes.addressof(c), _keep(self, _weight_array(ws)), len(ws), _stream())
        torch.cuda.synchronize(device)
        self.h = h
        self.cfg = cfg
        self.max_batch = max_batch
        self.device = device


@torch.no_grad()
def clip_encode_text_tokens(tokens, handle: ClipTextHandle):
    """tokens: integer tensor [n, context_length] as `clip.tokenize` returns -> fp32 [n, output_dim] (not normalised)."""
    if tokens.dim() != 2 or tokens.shape[1] != handle.cfg.context_length:
        raise ValueError(f"tokens must be [n, {handle.cfg.context_length}], got {tuple(tokens.shape)}")
    n = tokens.shape[0]
    if n < 1 or n > handle.max_batch:
        raise ValueError(f"batch {n} outside the text handle capacity 1..{handle.max_batch}")
    tk = tokens.detach().to("cpu")
    if int(tk.min()) < 0 or int(tk.max()) >= handle.cfg.vocab_size:
        raise ValueError(f"token ids must lie in [0, {handle.cfg.vocab_size})")
    tk = tk.to(device=handle.device, dtype=torch.int32).contiguous()
    out = torch.empty(n, handle.cfg.output_dim, device=handle.device)
    call("prx_clip_text_encode", handle.h, tk, n, out, _stream())
    return out


# --------------------------------------------------------------------------------------- VQGAN
def _single_attn_resolution(cfg) -> int:
    """taming places AttnBlocks at every level whose NOMINAL resolution (config `resolution` halved per level) is listed in
    `attn_resolutions`; the C ABI carries one such resolution (every published VQGAN config has one: [16], or [32]).  A config in
    which two listed resolutions are actually visited is refused here rather than built with attention missing."""
    visited = {cfg.resolution >> k for k in range(len(cfg.ch_mult))}
    hits = sorted(set(int(r) for r in cfg.attn_resolutions) & visited)
    if len(hits) > 1:
        raise ValueError(f"VQGAN config with attention at {len(hits)} resolutions {hits}: the runner supports one")
    return hits[0] if hits else -1


class VqganHandle(_EngineHandle):
    """Owns a `prx_vqgan` (codebook, weight packs, activations of one forward).  `precision`: "fp16" (default) | "bf16" | "f32"."""
    _destroy = "prx_vqgan_destroy"
    abi = "prx_vqgan"

    def __init__(self, cfg, params, latent_hw, device, precision=None):
        from .weights import vqgan_param_shapes
        ws = _weights_in_abi_order(params, vqgan_param_shapes(cfg), device, "VQGAN decoder")
        c = _VqganCfg()
        c.ch = cfg.ch
        for i, m in enumerate(cfg.ch_mult):
            c.ch_mult[i] = m
        c.n_mult = len(cfg.ch_mult)
        c.num_res_blocks = cfg.num_res_blocks
        c.attn_resolution = _single_attn_resolution(cfg)
        c.resolution = cfg.resolution
        c.z_channels = cfg.z_channels
        c.embed_dim = cfg.embed_dim
        c.n_embed = cfg.n_embed
        c.out_ch = cfg.out_ch
        c.latent_h, c.latent_w = latent_hw
        self.precision = precision_code(precision)
        c.precision = self.precision
        h = ctypes.c_void_p()
        call("prx_vqgan_create", ctypes.addressof(h), ctypes.addressof(c), _keep(self, _weight_array(ws)), len(ws), _stream())
        torch.cuda.synchronize(device)
        self.h = h
        self.cfg = cfg
        self.latent_hw = tuple(latent_hw)
        self.f = 2 ** (len(cfg.ch_mult) - 1)
        self.device = device
        self.last_indices = None
        self.generation = 0              # see _ClipEncodeFn: one forward's activations per handle

    def z_bounds(self):
        zmin = torch.empty(self.cfg.embed_dim, device=self.device)
        zmax = torch.empty(self.cfg.embed_dim, device=self.device)
        call("prx_vqgan_z_bounds", self.h, zmin, zmax, _stream())
        return zmin, zmax


class _VqganSynthFn(torch.autograd.Function):
    """VqganDrawer.synth (vqgan.py:190-195).  Same one-forward-per-handle rule as `_ClipEncodeFn`: a `to_image()` or a
    second `synth()` between this forward and its backward bumps the handle's generation, and the backward then re-runs
    the forward from the saved z before differentiating."""

    @staticmethod
    def forward(ctx, z, handle, quantize):
        _need_cuda(z)
        z = z.contiguous().float()
        hh, ww = handle.latent_hw
        assert z.shape == (1, handle.cfg.z_channels, hh, ww), f"z must be [1,{handle.cfg.z_channels},{hh},{ww}]"
        dev = z.device
        img = torch.empty(1, handle.cfg.out_ch, hh * handle.f, ww * handle.f, device=dev)
        idx = torch.empty(hh * ww, device=dev, dtype=torch.int32)
        call("prx_vqgan_synth", handle.h, z, img, idx, int(quantize), _stream())
        handle.last_indices = idx
        handle.generation += 1
        ctx.generation = handle.generation
        ctx.handle = handle
        ctx.quantize = int(quantize)
        ctx.save_for_backward(z)
        return img

    @staticmethod
    def backward(ctx, g):
        handle = ctx.handle
        (z,) = ctx.saved_tensors
        g = g.contiguous().float()
        hh, ww = handle.latent_hw
        if handle.generation != ctx.generation:
            scratch = torch.empty(1, handle.cfg.out_ch, hh * handle.f, ww * handle.f, device=g.device)
            call("prx_vqgan_synth", handle.h, z, scratch, None, ctx.quantize, _stream())
            handle.generation += 1
            ctx.generation = handle.generation
        dz = torch.empty(1, handle.cfg.z_channels, hh, ww, device=g.device)
        call("prx_vqgan_synth_backward", handle.h, g, dz, _stream())
        return dz, None, None


def vqgan_synth(z, handle: VqganHandle, quantize: bool = True):
    return _VqganSynthFn.apply(z, handle, quantize)


class VqganEncHandle(_Handle):
    """Owns a `prx_vqgan_enc` (taming Encoder + quant_conv + codebook) for one image size; forward only
    (VqganDrawer.init_from_tensor / reapply_from_tensor / get_z_from_tensor, vqgan.py:174-185)."""
    _destroy = "prx_vqgan_enc_destroy"

    def __init__(self, cfg, params, image_hw, device, in_channels: int = 3):
        from .weights import vqgan_encoder_param_shapes
        ws = _weights_in_abi_order(params, vqgan_encoder_param_shapes(cfg, in_channels), device, "VQGAN encoder")
        c = _VqganCfg()
        c.ch = cfg.ch
        for i, m in enumerate(cfg.ch_mult):
            c.ch_mult[i] = m
        c.n_mult = len(cfg.ch_mult)
        c.num_res_blocks = cfg.num_res_blocks
        c.attn_resolution = _single_attn_resolution(cfg)
        c.resolution = cfg.resolution
        c.z_channels = cfg.z_channels
        c.embed_dim = cfg.embed_dim
        c.n_embed = cfg.n_embed
        c.out_ch = cfg.out_ch
        self.f = 2 ** (len(cfg.ch_mult) - 1)
        H, W = image_hw
        c.latent_h, c.latent_w = H // self.f, W // self.f
        h = ctypes.c_void_p()
        call("prx_vqgan_enc_create", ctypes.addressof(h), ctypes.addressof(c), in_channels, H, W, _keep(self, _weight_array(ws)),
             len(ws), _stream())
        torch.cuda.synchronize(device)
        self.h = h
        self.cfg = cfg
        self.image_hw = (H, W)
        self.in_channels = in_channels
        self.device = device


@torch.no_grad()
def vqgan_encode(img, handle: VqganEncHandle, return_pre: bool = False):
    """img [1,C,H,W] in [-1,1] -> z [1,embed_dim,H/f,W/f] (the selected code vectors), int32 indices
    [, the latent before quantisation]."""
    _need_cuda(img)
    img = img.contiguous().float()
    H, W = handle.image_hw
    assert img.shape == (1, handle.in_channels, H, W), f"image must be [1,{handle.in_channels},{H},{W}], got {tuple(img.shape)}"
    h0, w0 = H // handle.f, W // handle.f
    z = torch.empty(1, handle.cfg.embed_dim, h0, w0, device=img.device)
    idx = torch.empty(h0 * w0, device=img.device, dtype=torch.int32)
    pre = torch.empty_like(z) if return_pre else None
    call("prx_vqgan_encode", handle.h, img, z, pre, idx, _stream())
    return (z, idx, pre) if return_pre else (z, idx)


# --------------------------------------------------------------------------------------- Prompt loss
_TICKETS = {}


def _ticket(device):
    """the prompt kernel's "last workgroup adds up" counter: a wrapping ticket (atomicInc modulo the grid), zero whenever no
    launch is in flight -- one resident word per (device, stream); a process uses a handful of streams, so the table stays small"""
    key = (str(device), _stream())
    t = _TICKETS.get(key)
    if t is None:
        t = _TICKETS[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return t


class _PromptLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, embed, weight, stop, denom):
        _need_cuda(input, embed)
        x = input.contiguous().float()
        e = embed.contiguous().float()
        n, D = x.shape
        m = e.shape[0]
        rowloss = torch.empty(n + 1, device=x.device)          # [n] row values, then the scalar |w| * sum / denom from the same launch
        grad = torch.empty_like(x)
        den = float(denom) if denom is not None else float(n * m)
        # (embeddings wider than 1024 -- OpenCLIP ViT-bigG-14: 1280 -- take the entry point whose cap is 2048)
        call("prx_prompt_loss_fwd_bwd" if D <= 1024 else "prx_prompt_loss_fwd_bwd_wide", x, e, n, m, D, float(weight), float(stop), den, rowloss, grad,
             rowloss[n:], _ticket(x.device), _stream())
        ctx.save_for_backward(grad)
        return rowloss[n]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None, None


def prompt_loss(input, embed, weight=1.0, stop=float("-inf"), denom=None):
    return _PromptLossFn.apply(input, embed, weight, stop, denom)


# --------------------------------------------------------------------------------------- optimiser
def adam_clamp_step_dev(z, exp_avg, exp_avg_sq, grad, zmin, zmax, hyper, betas=(0.9, 0.999), eps=1e-8):
    """Same, with {lr / bias_correction1, sqrt(bias_correction2)} read from the device tensor `hyper` (graph replay)."""
    _need_cuda(z, grad, hyper)
    hw = z.shape[-1] * z.shape[-2] if z.dim() >= 2 else z.numel()     # 1-D leaves (stroke widths, paper): one plane
    call("prx_adam_clamp_step_dev", z, exp_avg, exp_avg_sq, grad, zmin, zmax, hw, z.numel(), hyper, float(betas[0]),
         float(betas[1]), float(eps), _stream())


def adam_clamp_step(z, exp_avg, exp_avg_sq, grad, zmin, zmax, lr, step, betas=(0.9, 0.999), eps=1e-8):
    """In-place Adam step on z fused with the per-channel clip_z clamp."""
    _need_cuda(z, grad)
    assert z.is_contiguous() and grad.is_contiguous() and z.dtype == torch.float32
    hw = z.shape[-1] * z.shape[-2] if z.dim() >= 2 else z.numel()     # 1-D leaves (stroke widths, paper): one plane
    call("prx_adam_clamp_step", z, exp_avg, exp_avg_sq, grad, zmin, zmax, hw, z.numel(), float(lr), float(betas[0]),
         float(betas[1]), float(eps), int(step), _stream())


OPTIM_RULES = {"AdamW": 0, "Adagrad": 1, "Adamax": 2, "DiffGrad": 3}      # PRX_OPT_* (include/prx.h)


def _clamp_view(p, zmin, zmax):
    """(C, hw) of the [rows, C, hw] view the fused clip_z clamps in; (1, 1) without bounds (the kernels ignore them then)"""
    if zmin is None:
        assert zmax is None
        return 1, 1
    assert p.dim() >= 3 and zmin.numel() == zmax.numel() == p.shape[-3], "bounds are per channel of a [..., C, h, w] tensor"
    return p.shape[-3], p.shape[-2] * p.shape[-1]


def optim_step_dev(rule, p, states, grad, zmin, zmax, hyper, betas=(0.9, 0.999), eps=1e-8):
    """In-place AdamW / Adagrad / Adamax / DiffGrad step on p fused with the per-channel clip_z clamp; `states`: the rule's
    state tensors in the order of include/prx.h, `hyper`: its step scalars on the device (graph replay)."""
    _need_cuda(p, grad, hyper)
    assert p.is_contiguous() and grad.is_contiguous() and p.dtype == torch.float32 and all(s.is_contiguous() for s in states)
    C, hw = _clamp_view(p, zmin, zmax)
    s1, s2, s3 = (list(states) + [None, None])[:3]
    call("prx_optim_step_dev", OPTIM_RULES[rule], p, s1, s2, s3, grad, zmin, zmax, C, hw, p.numel(), hyper, float(betas[0]),
         float(betas[1]), float(eps), _stream())


def adamp_scratch(p):
    """the partial-sum buffer of `adamp_step_dev` for p (allocated once: a captured graph keeps its address)"""
    rows = p.shape[0] if p.dim() > 1 else 0
    return torch.empty(call("prx_optim_adamp_scratch_floats", rows, p.numel()), dtype=torch.float32, device=p.device)


def adamp_step_dev(p, exp_avg, exp_avg_sq, grad, zmin, zmax, hyper, scratch, betas=(0.9, 0.999), eps=1e-8, delta=0.1):
    """In-place AdamP step on p (projection test on the [shape[0], -1] view, then on [1, -1]) fused with the clip_z clamp:
    two launches, no atomics."""
    _need_cuda(p, grad, hyper, scratch)
    assert p.is_contiguous() and grad.is_contiguous() and p.dtype == torch.float32
    C, hw = _clamp_view(p, zmin, zmax)
    rows = p.shape[0] if p.dim() > 1 else 0
    call("prx_optim_adamp_step_dev", p, exp_avg, exp_avg_sq, grad, zmin, zmax, rows, C, hw, p.numel(), hyper, scratch,
         scratch.numel(), float(betas[0]), float(betas[1]), float(eps), float(delta), _stream())


# --------------------------------------------------------------------------------------- VGG16 features (StyleLoss plugin)
VGG16_CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)       # torchvision vgg16().features conv layers
VGG16_CAPTURE_LAYERS = (1, 3, 6, 8, 11, 13, 15, 22, 29)                     # Losses/StyleLoss.py:31


class Vgg16Handle(_EngineHandle):
    """Owns a `prx_vgg16` (torchvision VGG16 `features` up to relu5_3, frozen) for inputs up to `max_hw`.
    `params`: {"features.N.weight", "features.N.bias"} (torchvision state-dict names)."""
    _destroy = "prx_vgg16_destroy"
    abi = "prx_vgg16"

    def __init__(self, params, max_hw, device, precision=None):
        self.precision = precision_code(precision)
        from .weights import vgg16_param_shapes
        ws = _weights_in_abi_order(params, vgg16_param_shapes(), device, "VGG16")
        h = ctypes.c_void_p()
        call("prx_vgg16_create", ctypes.addressof(h), _keep(self, _weight_array(ws)), len(ws), int(max_hw[0]), int(max_hw[1]),
             self.precision, _stream())
        torch.cuda.synchronize(device)
        self.h = h
        self.max_hw = (int(max_hw[0]), int(max_hw[1]))
        self.device = device

    def feature_shape(self, H, W, k):
        h, w, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        call("prx_vgg16_feature_shape", int(H), int(W), int(k), ctypes.addressof(h), ctypes.addressof(w), ctypes.addressof(c))
        return h.value, w.value, c.value


class _Vgg16Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, handle):
        _need_cuda(x)
        assert x.dim() == 4 and x.shape[0] == 1 and x.shape[1] == 3, "the VGG16 extractor takes one [1,3,H,W] image"
        H, W = int(x.shape[2]), int(x.shape[3])
        x = x.detach().to(torch.float32).contiguous()
        nbytes = call("prx_vgg16_workspace_bytes", H, W, handle.precision)
        if nbytes <= 0:
            raise PrxError(f"VGG16 extractor: input {H}x{W} is too small")
        work = torch.empty(int(nbytes), dtype=torch.uint8, device=x.device)
        feats = []
        for k in range(len(VGG16_CAPTURE_LAYERS)):
            h, w, c = handle.feature_shape(H, W, k)
            feats.append(torch.empty(1, h, w, c, dtype=torch.float32, device=x.device))
        arr = (ctypes.c_void_p * len(feats))(*[f.data_ptr() for f in feats])
        call("prx_vgg16_forward", handle.h, x, H, W, work, ctypes.addressof(arr), _stream())
        ctx.handle, ctx.work, ctx.hw = handle, work, (H, W)
        return tuple(feats)

    @staticmethod
    def backward(ctx, *gs):
        H, W = ctx.hw
        keep = [None if g is None else g.to(torch.float32).contiguous() for g in gs]
        arr = (ctypes.c_void_p * len(keep))(*[None if g is None else g.data_ptr() for g in keep])
        gx = torch.empty(1, 3, H, W, dtype=torch.float32, device=ctx.work.device)
        call("prx_vgg16_backward", ctx.handle.h, H, W, ctx.work, ctypes.addressof(arr), gx, _stream())
        return gx, None


class _HypercolumnsFn(torch.autograd.Function):
    """`spatial_feature_extract` (Losses/StyleLoss.py:169-223) over all feature maps in one gather launch (and one scatter
    launch backward); rows int64 [L,4,n], wts fp32 [4L+2,n] (tap weights, then the two coordinate channels)"""

    @staticmethod
    def forward(ctx, rows, wts, *feats):
        L, n = len(feats), int(rows.shape[2])
        for f in feats:
            _need_cuda(f)
            if f.dtype != torch.float32 or not f.is_contiguous() or f.dim() != 4 or f.shape[0] != 1:
                raise PrxError("hypercolumns: feature maps must be contiguous fp32 [1,h,w,C] device tensors")
        if rows.dtype != torch.int64 or not rows.is_contiguous() or tuple(rows.shape) != (L, 4, n):
            raise PrxError("hypercolumns: rows must be a contiguous int64 [L,4,n] tensor")
        if wts.dtype != torch.float32 or not wts.is_contiguous() or tuple(wts.shape) != (4 * L + 2, n):
            raise PrxError("hypercolumns: weights must be a contiguous fp32 [4L+2,n] tensor")
        chans = (ctypes.c_int * L)(*[int(f.shape[3]) for f in feats])
        ptrs = (ctypes.c_void_p * L)(*[f.data_ptr() for f in feats])
        ctot = sum(chans)
        out = torch.empty(n, ctot + 2, dtype=torch.float32, device=feats[0].device)
        call("prx_hypercolumns_fwd", ctypes.addressof(ptrs), ctypes.addressof(chans), L, rows, wts, n, out, ctot + 2, _stream())
        ctx.save_for_backward(rows, wts)
        ctx.shapes = [tuple(f.shape) for f in feats]
        return out

    @staticmethod
    def backward(ctx, gout):
        rows, wts = ctx.saved_tensors
        L, n = len(ctx.shapes), int(rows.shape[2])
        gout = gout.to(torch.float32).contiguous()
        grads = [torch.zeros(sh, dtype=torch.float32, device=gout.device) if ctx.needs_input_grad[2 + l] else None
                 for l, sh in enumerate(ctx.shapes)]
        chans = (ctypes.c_int * L)(*[int(sh[3]) for sh in ctx.shapes])
        ptrs = (ctypes.c_void_p * L)(*[g.data_ptr() if g is not None else None for g in grads])
        call("prx_hypercolumns_bwd", ctypes.addressof(ptrs), ctypes.addressof(chans), L, rows, wts, n, gout, int(gout.shape[1]), _stream())
        return (None, None) + tuple(grads)


def hypercolumns(feats, rows, wts):
    """feats: list of [1,h,w,C] fp32 NHWC maps -> [n, sum(C)+2] sampled columns (+ the two coordinate channels)"""
    return _HypercolumnsFn.apply(rows, wts, *[f.contiguous() for f in feats])


def _f32c(t, what):
    _need_cuda(t)
    if t.dtype != torch.float32 or t.dim() != 2:
        raise PrxError(f"{what}: expected a 2-D fp32 device tensor, got {tuple(t.shape)} {t.dtype}")
    return t.contiguous()


def _row_sumsq(X):
    """|x_i|^2 as `pairwise_distances_cos` takes it ((x ** 2).sum(1), Losses/StyleLoss.py:227): the same reduction, so that the
    distance matrix -- and with it every arg-minimum -- is bit for bit the composed expression's"""
    return (X * X).sum(1)


class _RemdFn(torch.autograd.Function):
    """`style_loss` (Losses/StyleLoss.py:272-293) on columns X [n, d] (differentiated) and Y [m, d] (the style image's: no
    gradient): max of the mean row minimum and the mean column minimum of the cosine (+ L2 when `l2`) distance matrix.  The
    product X Y^T is a library GEMM; the distance / minima pass and the backward over the n + m selected pairs are
    csrc/strotss.hip.  `ys`: |y_j|^2, the caller's (the same style columns serve three evaluations)."""

    @staticmethod
    def forward(ctx, X, Y, ys, l2):
        X, Y = _f32c(X, "strotss_remd X"), _f32c(Y, "strotss_remd Y")
        n, d = int(X.shape[0]), int(X.shape[1])
        m = int(Y.shape[0])
        if int(Y.shape[1]) != d or tuple(ys.shape) != (m,):
            raise PrxError(f"strotss_remd: X {tuple(X.shape)}, Y {tuple(Y.shape)}, ys {tuple(ys.shape)} do not match")
        G = torch.mm(X, Y.t())
        xs = _row_sumsq(X)
        packs = torch.empty(n + m, dtype=torch.int64, device=X.device)
        stats = torch.empty(4, dtype=torch.float32, device=X.device)
        call("prx_strotss_remd_fwd", G, m, xs, ys, n, m, int(bool(l2)), d, packs, packs[n:], stats, _stream())
        ctx.save_for_backward(G, X, Y, xs, ys, packs, stats)
        ctx.l2 = int(bool(l2))
        return stats[0].clone()

    @staticmethod
    def backward(ctx, g):
        G, X, Y, xs, ys, packs, stats = ctx.saved_tensors
        n, d, m = int(X.shape[0]), int(X.shape[1]), int(Y.shape[0])
        g = g.to(torch.float32).reshape(1).contiguous()
        dX = torch.empty_like(X)
        nbytes = int(_lib.load().prx_strotss_remd_bwd_workspace_bytes(n, m, d))
        work = torch.empty(nbytes, dtype=torch.uint8, device=X.device)
        call("prx_strotss_remd_bwd", G, m, X, d, Y, d, d, xs, ys, packs, packs[n:], n, m, ctx.l2, stats, g, work, nbytes, dX, d, _stream())
        return dX, None, None, None


def strotss_remd(X, Y, ys=None, l2=False):
    if Y.requires_grad:
        raise PrxError("strotss_remd: the style columns take no gradient")
    if ys is None:
        ys = _row_sumsq(Y.detach())
    return _RemdFn.apply(X, Y, ys, l2)


class _SelfSimFn(torch.autograd.Function):
    """`content_loss` (Losses/StyleLoss.py:246-265): mean |cosine self-distance matrix of X - that of Y|, both [n, d] and both
    differentiated.  Products: library GEMMs; the distance passes: csrc/strotss.hip (the backward returns the symmetrised
    d/dG, so each operand costs one product)."""

    @staticmethod
    def forward(ctx, X, Y):
        X, Y = _f32c(X, "strotss_selfsim X"), _f32c(Y, "strotss_selfsim Y")
        if X.shape != Y.shape:
            raise PrxError(f"strotss_selfsim: X {tuple(X.shape)} and Y {tuple(Y.shape)} differ")
        n = int(X.shape[0])
        Gx, Gy = torch.mm(X, X.t()), torch.mm(Y, Y.t())
        xs, ys = _row_sumsq(X), _row_sumsq(Y)
        partial = torch.empty(n, dtype=torch.float64, device=X.device)
        out = torch.empty(1, dtype=torch.float32, device=X.device)
        call("prx_strotss_selfsim_fwd", Gx, n, xs, Gy, n, ys, n, partial, out, _stream())
        ctx.save_for_backward(Gx, Gy, xs, ys, X, Y)
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        Gx, Gy, xs, ys, X, Y = ctx.saved_tensors
        n = int(X.shape[0])
        g = g.to(torch.float32).reshape(1).contiguous()
        S = torch.empty(2, n, n, dtype=torch.float32, device=X.device)
        c = torch.empty(2, n, dtype=torch.float32, device=X.device)
        call("prx_strotss_selfsim_bwd", Gx, n, xs, Gy, n, ys, n, g, S[0], S[1], n, c[0], c[1], _stream())
        dX = torch.addcmul(torch.mm(S[0], X), X, c[0].unsqueeze(1)) if ctx.needs_input_grad[0] else None
        dY = torch.addcmul(torch.mm(S[1], Y), Y, c[1].unsqueeze(1)) if ctx.needs_input_grad[1] else None
        return dX, dY


def strotss_selfsim(X, Y):
    return _SelfSimFn.apply(X, Y)


def vgg16_features(x, handle: Vgg16Handle):
    """x [1,3,H,W] (already normalised for VGG) -> the nine captured feature maps as NHWC fp32 tensors [1,h,w,C]
    (channels-last is the engine's layout; `f.permute(0,3,1,2)` is the reference's NCHW view)."""
    return _Vgg16Fn.apply(x, handle)


# --------------------------------------------------------------------------------------- fft drawer (configs[3])
class FftDrawerHandle(_Handle):
    """`prx_fft_drawer` (csrc/fft_drawer.hip): spectrum [1,3,H,Wf,2] -> image [1,3,H,W] as exact-f32 GEMMs against twiddle
    matrices, and its backward.  One handle per canvas size."""
    _destroy = "prx_fft_drawer_destroy"

    def __init__(self, width: int, height: int, decay: float = 1.5, colors: float = 1.5):
        lib = _lib.load()
        self.h = lib.prx_fft_drawer_create(int(width), int(height), float(decay), float(colors))
        if not self.h:
            raise PrxError("prx_fft_drawer_create failed: " + _lib.last_error())
        self.width, self.height = int(width), int(height)
        self.freq_columns = lib.prx_fft_drawer_freq_columns(self.h)
        self.ticket = 0            # counts the synths: the handle keeps the state of the latest one only


class _FftSynthFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, handle, contrast):
        _need_cuda(params)
        p = params.detach().contiguous().float()
        if tuple(p.shape) != (1, 3, handle.height, handle.freq_columns, 2):
            raise PrxError(f"fft drawer: spectrum {tuple(p.shape)} does not fit a {handle.width} x {handle.height} canvas")
        img = torch.empty(1, 3, handle.height, handle.width, device=p.device)
        call("prx_fft_drawer_synth", handle.h, p, float(contrast), img, _stream())
        handle.ticket += 1
        ctx.handle, ctx.shape, ctx.ticket = handle, p.shape, handle.ticket
        return img

    @staticmethod
    def backward(ctx, g):
        if ctx.ticket != ctx.handle.ticket:
            raise PrxError(f"fft drawer: stale backward -- this is the backward of synth {ctx.ticket} of its handle, which now holds "
                           f"the state of synth {ctx.handle.ticket}; a handle differentiates its latest synth only")
        g = g.contiguous().float()
        gp = torch.empty(ctx.shape, device=g.device)
        call("prx_fft_drawer_backward", ctx.handle.h, g, gp, _stream())
        return gp, None, None


def fft_synth(params: torch.Tensor, handle: FftDrawerHandle, contrast: float = 0.9) -> torch.Tensor:
    """differentiable w.r.t. `params`; a backward differentiates the handle's LAST synth (one synth per backward, as the loop does):
    each synth takes a ticket on its handle, and the backward of an earlier synth raises PrxError instead of returning the gradient of
    another image.  Repeated backwards of the latest synth are fine."""
    return _FftSynthFn.apply(params, handle, contrast)


# --------------------------------------------------------------------------------------- RRDBNet x4 (super_resolution drawer)
class RrdbNetHandle(_Handle):
    """Owns a `prx_rrdbnet` (csrc/rrdbnet.hip): weight packs and every activation / gradient buffer of one latent size,
    allocated here and never afterwards.  `precision`: "fp16" (default) | "f32"; "bf16" is refused by name."""
    _destroy = "prx_rrdbnet_destroy"

    def __init__(self, cfg, params, latent_hw, device, precision=None):
        from .weights import rrdbnet_param_shapes
        ws = _weights_in_abi_order(params, rrdbnet_param_shapes(cfg), device, f"RRDBNet {getattr(cfg, 'name', '')}")
        self.precision = precision_code(precision)
        hh, ww = int(latent_hw[0]), int(latent_hw[1])
        h = ctypes.c_void_p()
        call("prx_rrdbnet_create", ctypes.addressof(h), cfg.num_feat, cfg.num_grow_ch, cfg.num_block, hh, ww, _keep(self, _weight_array(ws)),
             len(ws), self.precision, _stream())
        torch.cuda.synchronize(device)   # the weights are copied / packed: the tensors may now be released
        self.h = h
        self.cfg = cfg
        self.latent_hw = (hh, ww)
        self.device = device
        self.generation = 0              # see _ClipEncodeFn: one forward's activations per handle


class _RrdbNetSynthFn(torch.autograd.Function):
    """SuperResolutionDrawer.synth (super_resolution.py:81-83).  One forward's activations per handle: a backward whose
    generation is stale (a second `synth()` ran in between) fails by name instead of differentiating the wrong forward."""

    @staticmethod
    def forward(ctx, z, handle, clamp):
        _need_cuda(z)
        z = z.contiguous().float()
        hh, ww = handle.latent_hw
        if tuple(z.shape) != (1, 3, hh, ww):
            raise PrxError(f"rrdbnet_synth: z must be [1,3,{hh},{ww}], got {tuple(z.shape)}")
        img = torch.empty(1, 3, 4 * hh, 4 * ww, device=z.device)
        call("prx_rrdbnet_synth", handle.h, z, img, int(bool(clamp)), _stream())
        handle.generation += 1
        ctx.generation = handle.generation
        ctx.handle = handle
        return img

    @staticmethod
    def backward(ctx, g):
        handle = ctx.handle
        if handle.generation != ctx.generation:
            raise PrxError("rrdbnet_synth: stale backward -- the handle has run another synth since this forward "
                           "(it keeps ONE forward's activations; use one handle per live graph)")
        g = g.contiguous().float()
        hh, ww = handle.latent_hw
        dz = torch.empty(1, 3, hh, ww, device=g.device)
        call("prx_rrdbnet_backward", handle.h, g, dz, _stream())
        return dz, None, None


def rrdbnet_synth(z, handle: RrdbNetHandle, clamp: bool = True):
    """clamp_with_grad(RRDBNet(z), 0, 1) [1,3,4h,4w]; `clamp=False`: the raw network output (tests)"""
    return _RrdbNetSynthFn.apply(z, handle, clamp)


# --------------------------------------------------------------------------------------- built-in losses and filters
# (csrc/plugin_losses.hip, plugin_filters.hip).  Every loss scalar comes out of its launch through the same fixed-order
# "partials, then the last workgroup" reduction as the Prompt loss: `partials` is a scratch of 1024 rows x 4 doubles.
_PLUGIN_PARTIALS = {}
PALETTE_MAX = 256


def _partials(device):
    key = (str(device), _stream())
    t = _PLUGIN_PARTIALS.get(key)
    if t is None:
        t = _PLUGIN_PARTIALS[key] = torch.empty(1024 * 4, dtype=torch.float64, device=device)
    return t


def _f32_nchw(x, what):
    if x.dim() != 4 or x.dtype != torch.float32:
        raise PrxError(f"{what}: expected an fp32 [N, C, H, W] tensor, got {tuple(x.shape)} {x.dtype}")
    return x.contiguous()


def _palette_dev(palette, device):
    p = torch.as_tensor(palette, dtype=torch.float32, device=device).reshape(-1, 3).contiguous()
    if not 1 <= p.shape[0] <= PALETTE_MAX:
        raise PrxError(f"palette of {p.shape[0]} colours: 1 .. {PALETTE_MAX} are supported")
    return p


class _SaturationFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cutouts, weight):
        _need_cuda(cutouts)
        x = _f32_nchw(cutouts, "saturation_loss")
        n, c, h, w = x.shape
        assert c == 3
        stats = torch.empty(4, dtype=torch.float64, device=x.device)
        loss = torch.empty((), device=x.device)
        call("prx_saturation_fwd", x, n, h * w, float(weight), _partials(x.device), stats, loss, _ticket(x.device), _stream())
        ctx.save_for_backward(x, stats)
        ctx.weight = float(weight)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, stats = ctx.saved_tensors
        n, _, h, w = x.shape
        grad = torch.empty_like(x)
        call("prx_saturation_bwd", x, n, h * w, ctx.weight, stats, g.contiguous(), grad, _stream())
        return grad, None


def saturation_loss(cutouts, weight=1.0):
    """SaturationLoss of ONE cutout batch [n, 3, S, S]: -(std_rggb + 0.3 mean_rggb) * weight / 10"""
    return _SaturationFn.apply(cutouts, weight)


class _LocalGradLossFn(torch.autograd.Function):
    """a loss whose kernel wrote d loss / d input in the forward launch: the backward scales it"""
    @staticmethod
    def forward(ctx, x, launch):
        loss, grad = launch()
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None


def symmetry_loss(out, weight=1.0):
    """SymmetryLoss: MSE(out, flip_W(out)) * weight"""
    _need_cuda(out)
    x = _f32_nchw(out, "symmetry_loss")
    n, c, h, w = x.shape

    def launch():
        grad, loss = torch.empty_like(x), torch.empty((), device=x.device)
        call("prx_symmetry_fwd_bwd", x, n * c, h, w, float(weight), _partials(x.device), grad, loss, _ticket(x.device), _stream())
        return loss, grad
    return _LocalGradLossFn.apply(out, launch)


def _edge_bands(n, c, h, w, margins, what):
    """(left, right, upper, lower) pixel margins -> (ints, 1 / band elements per band, 0 where the band is off)"""
    left, right, upper, lower = (int(m) for m in margins)
    inner = max(0, (w - right) - left)
    bands = (n * c * h * max(0, min(left, w)), n * c * h * max(0, min(right, w)), n * c * max(0, min(upper, h)) * inner,
             n * c * max(0, min(lower, h)) * inner)
    for m, cnt in zip((left, right, upper, lower), bands):
        if m != 0 and cnt == 0:
            raise PrxError(f"{what}: margins {margins} leave an empty band on a {h} x {w} image")
    return (left, right, upper, lower), [1.0 / cnt if m != 0 else 0.0 for m, cnt in zip((left, right, upper, lower), bands)]


def edge_loss(out, color, margins, edge_weight, global_weight):
    """EdgeLoss (flat colour, no mask image): `margins` = (left, right, upper, lower) in PIXELS"""
    _need_cuda(out)
    x = _f32_nchw(out, "edge_loss")
    n, c, h, w = x.shape
    if c != 3:
        raise PrxError("edge_loss: expected 3 channels")
    (left, right, upper, lower), inv = _edge_bands(n, c, h, w, margins, "edge_loss")
    inv_all = float(global_weight) / x.numel() if global_weight else 0.0

    def launch():
        grad, loss = torch.empty_like(x), torch.empty((), device=x.device)
        call("prx_edge_fwd_bwd", x, n * c, h, w, float(color[0]), float(color[1]), float(color[2]), left, right, upper, lower,
             *[float(v) for v in inv], inv_all, float(edge_weight), _partials(x.device), grad, loss, _ticket(x.device), _stream())
        return loss, grad
    return _LocalGradLossFn.apply(out, launch)


def edge_target_loss(out, target, color, mask, margins, edge_weight, global_weight):
    """EdgeLoss with `--edge_input_image` / `--edge_mask_image`: `target` a [1, 3, H, W] (or [3, H, W]) fp32 device tensor or
    None (then the flat `color`), `mask` a [H, W] (any leading 1s) fp32 device tensor or None.  Without a mask the four margin
    bands (`margins` in PIXELS) are scored against the target; with one they are skipped and every element where mask <= 0 is
    scored, mean over ALL elements.  Plus global_weight * MSE over the image, all times edge_weight."""
    _need_cuda(out)
    x = _f32_nchw(out, "edge_target_loss")
    n, c, h, w = x.shape
    if c != 3:
        raise PrxError("edge_target_loss: expected 3 channels")
    for t, name, numel in ((target, "target", 3 * h * w), (mask, "mask", h * w)):
        if t is None:
            continue
        _need_cuda(t)
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != numel or tuple(t.shape[-2:]) != (h, w) or t.device != x.device:
            raise PrxError(f"edge_target_loss: {name} must be a contiguous fp32 tensor of {numel} elements ending in ({h}, {w}) on "
                           f"{x.device}, got {tuple(t.shape)} {t.dtype} on {t.device}")
    if mask is None:
        (left, right, upper, lower), inv = _edge_bands(n, c, h, w, margins, "edge_target_loss")
    else:
        (left, right, upper, lower), inv = (0, 0, 0, 0), [0.0, 0.0, 0.0, 0.0]
    inv_mask = 1.0 / x.numel() if mask is not None else 0.0
    inv_all = float(global_weight) / x.numel() if global_weight else 0.0

    def launch():
        grad, loss = torch.empty_like(x), torch.empty((), device=x.device)
        call("prx_edge_target_fwd_bwd", x, n * c, h, w, target, float(color[0]), float(color[1]), float(color[2]), mask, left, right,
             upper, lower, *[float(v) for v in inv], inv_mask, inv_all, float(edge_weight), _partials(x.device), grad, loss,
             _ticket(x.device), _stream())
        return loss, grad
    return _LocalGradLossFn.apply(out, launch)


def gaussian_loss(out, gy, gx, color01, weight=1.0):
    """GaussianLoss: mean(|out - colour| * |1 - gy (x) gx|) * weight.  `gy` [H], `gx` [W]: fp32 device tables; `color01` in [0, 1]"""
    _need_cuda(out, gy, gx)
    x = _f32_nchw(out, "gaussian_loss")
    n, c, h, w = x.shape
    if c != 3:
        raise PrxError("gaussian_loss: expected 3 channels")
    for t, name, numel in ((gy, "gy", h), (gx, "gx", w)):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (numel,) or t.device != x.device:
            raise PrxError(f"gaussian_loss: {name} must be a contiguous fp32 [{numel}] tensor on {x.device}, got {tuple(t.shape)} {t.dtype} on {t.device}")
    scale = float(weight) / x.numel()

    def launch():
        grad, loss = torch.empty_like(x), torch.empty((), device=x.device)
        call("prx_gaussian_fwd_bwd", x, n * c, h, w, gy, gx, float(color01[0]), float(color01[1]), float(color01[2]), scale,
             _partials(x.device), grad, loss, _ticket(x.device), _stream())
        return loss, grad
    return _LocalGradLossFn.apply(out, launch)


def aesthetic_loss(embeds, weight, bias, target):
    """AestheticLoss: 0.02 * mean((linear(normalize(embeds), weight, bias) - target)^2).  `embeds` [n, d] fp32, `weight` a
    [d] (or [1, d]) fp32 device tensor, `bias` and `target` floats"""
    _need_cuda(embeds, weight)
    if embeds.dim() != 2 or embeds.dtype != torch.float32 or embeds.shape[0] < 1 or embeds.shape[1] < 1:
        raise PrxError(f"aesthetic_loss: expected an fp32 [n, d] tensor, got {tuple(embeds.shape)} {embeds.dtype}")
    x = embeds.contiguous()
    n, d = x.shape
    if weight.dtype != torch.float32 or not weight.is_contiguous() or weight.numel() != d or weight.device != x.device:
        raise PrxError(f"aesthetic_loss: weight must be a contiguous fp32 tensor of {d} elements on {x.device}, got "
                       f"{tuple(weight.shape)} {weight.dtype} on {weight.device}")

    def launch():
        grad, loss = torch.empty_like(x), torch.empty((), device=x.device)
        call("prx_aesthetic_fwd_bwd", x, n, d, weight, float(bias), float(target), _partials(x.device), grad, loss,
             _ticket(x.device), _stream())
        return loss, grad
    return _LocalGradLossFn.apply(embeds, launch)


def palette_loss(cutouts, palette, weight=1.0):
    """PaletteLoss of ONE cutout batch: mean over pixels of |pixel - nearest palette colour| * n * weight / 10.  `palette`: a
    [k, 3] device tensor (or anything torch.as_tensor takes)"""
    _need_cuda(cutouts)
    x = _f32_nchw(cutouts, "palette_loss")
    n, c, h, w = x.shape
    pal = palette if isinstance(palette, torch.Tensor) and palette.device == x.device and palette.dtype == torch.float32 \
        and palette.is_contiguous() else _palette_dev(palette, x.device)
    if not 1 <= pal.shape[0] <= PALETTE_MAX:
        raise PrxError(f"palette of {pal.shape[0]} colours: 1 .. {PALETTE_MAX} are supported")
    scale = n * float(weight) / 10.0 / (n * h * w)

    def launch():
        grad, loss = torch.empty_like(x), torch.empty((), device=x.device)
        call("prx_palette_fwd_bwd", x, n, h * w, pal, pal.shape[0], float(scale), _partials(x.device), grad, loss,
             _ticket(x.device), _stream())
        return loss, grad
    return _LocalGradLossFn.apply(cutouts, launch)


SMOOTHNESS_TYPES = {"default": 0, "clipped": 1, "log": 2}


class _SmoothnessFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cutouts, weight, type_code, spacing, edge_order):
        x = cutouts.contiguous()
        n, _, h, w = x.shape
        tfac = torch.empty(n * h * w, device=x.device)
        loss = torch.empty((), device=x.device)
        call("prx_smoothness_fwd", x, n, h, w, int(type_code), int(edge_order), float(spacing), float(weight), _partials(x.device),
             tfac, loss, _ticket(x.device), _stream())
        ctx.save_for_backward(x, tfac)
        ctx.cfg = (int(edge_order), float(spacing), float(weight))
        return loss

    @staticmethod
    def backward(ctx, g):
        x, tfac = ctx.saved_tensors
        eo, spacing, weight = ctx.cfg
        n, _, h, w = x.shape
        grad = torch.empty_like(x)
        call("prx_smoothness_bwd", tfac, x, n, h, w, eo, spacing, weight, g.contiguous(), grad, _stream())
        return grad, None, None, None, None


class _BlurFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, taps):
        x = x.contiguous()
        n, c, h, w = x.shape
        k = taps.shape[-1]
        y = torch.empty(n, c, h - k + 1, w - k + 1, device=x.device)
        call("prx_blur_fwd", x, n * c, h, w, taps, k, y, _stream())
        ctx.save_for_backward(taps)
        ctx.hw = (n * c, h, w)
        return y

    @staticmethod
    def backward(ctx, g):
        (taps,) = ctx.saved_tensors
        planes, h, w = ctx.hw
        gx = torch.empty((planes // 3, 3, h, w), device=g.device)
        call("prx_blur_bwd", g.contiguous(), planes, h, w, taps, taps.shape[-1], gx, _stream())
        return gx, None


def gaussian_taps(kernel_size, std):
    """the k x k table of pixray's GaussianSmoothing (Losses/SmoothnessLoss.py) for one channel, fp32 on the host: the product
    of two exp(-((i - mean) / (2 std))^2) profiles, normalised to sum 1"""
    import math
    k = int(kernel_size)
    g = torch.arange(k, dtype=torch.float32)
    yy, xx = torch.meshgrid(g, g, indexing="ij")
    kern = 1
    mean = (kernel_size - 1) / 2
    for grid in (yy, xx):
        kern = kern * (1 / (std * math.sqrt(2 * math.pi)) * torch.exp(-((grid - mean) / (2 * std)) ** 2))
    return kern / torch.sum(kern)


def smoothness_loss(cutouts, weight=1.0, type="default", spacing=1, edge_order=1, blur_taps=None):
    """SmoothnessLoss of ONE cutout batch: mean gradient magnitude over the [n*S, S, 3] view, optionally after the valid-padding
    Gaussian blur whose k x k table `blur_taps` (a device tensor, gaussian_taps) holds.  Where the magnitude is exactly 0 the
    backward uses the zero subgradient (the reference's sqrt gives NaN there)."""
    _need_cuda(cutouts)
    x = _f32_nchw(cutouts, "smoothness_loss")
    if type not in SMOOTHNESS_TYPES:
        raise PrxError(f"smoothness type {type!r}: want one of {sorted(SMOOTHNESS_TYPES)}")
    if blur_taps is not None:
        x = _BlurFn.apply(x, blur_taps)
    return _SmoothnessFn.apply(x, weight, SMOOTHNESS_TYPES[type], spacing, edge_order)


class _ColorLookupFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, palette, beta):
        x = z.contiguous()
        b, c, h, w = x.shape
        out, lgrad = torch.empty_like(x), torch.empty_like(x)
        loss = torch.empty((), device=x.device)
        call("prx_color_lookup_fwd", x, b, c, h * w, palette, palette.shape[0], float(beta), _partials(x.device), out, lgrad, loss,
             _ticket(x.device), _stream())
        ctx.save_for_backward(lgrad)
        return out, loss

    @staticmethod
    def backward(ctx, gout, gloss):
        (lgrad,) = ctx.saved_tensors
        return torch.addcmul(gout, lgrad, gloss), None, None


def color_lookup(z, palette, beta):
    """ColorLookup filter: (nearest palette colour with a straight-through gradient, beta * commitment + codebook loss).
    z [B, 3 | 4, H, W] (alpha passes through); `palette` a [k <= 256, 3] fp32 device tensor"""
    _need_cuda(z)
    x = _f32_nchw(z, "color_lookup")
    if x.shape[1] not in (3, 4):
        raise PrxError("color_lookup: 3 or 4 channels")
    return _ColorLookupFn.apply(x, palette, beta)


WALLPAPER_MODES = {None: 0, "none": 0, "tiler": 0, "horizontal": 1, "vertical": 2, "shift": 3}


class _WallpaperFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, shifts, mode, em):
        x = img.contiguous()
        b, c, h, w = x.shape
        if mode == 3:
            ho, wo = 2 * h, w
        else:
            th = em // 2 if em and mode in (0, 2) else 0
            tw = em // 2 if em and mode in (0, 1) else 0
            ho, wo = h - 2 * th, w - 2 * tw
        out = torch.empty(b, c, ho, wo, device=x.device)
        loss = torch.empty((), device=x.device)
        call("prx_wallpaper_fwd", x, b * c, h, w, mode, em, shifts, _partials(x.device), out, loss, _ticket(x.device), _stream())
        ctx.save_for_backward(x, shifts)
        ctx.cfg = (mode, em)
        return out, loss

    @staticmethod
    def backward(ctx, gout, gloss):
        x, shifts = ctx.saved_tensors
        mode, em = ctx.cfg
        b, c, h, w = x.shape
        grad = torch.empty_like(x)
        call("prx_wallpaper_bwd", x, gout.contiguous(), b * c, h, w, mode, em, shifts, gloss.contiguous(), grad, _stream())
        return grad, None, None, None


def wallpaper(img, shifts, mode="none", edge_match=0):
    """TilerFilter / WallpaperFilter: -> (image, seam loss).  `shifts`: a 2-element int32 device tensor {rand_h, rand_w}, read by
    the kernels (a replayed graph sees what was staged there last); mode None / "none" / "tiler" rolls both axes"""
    _need_cuda(img)
    x = _f32_nchw(img, "wallpaper")
    if mode not in WALLPAPER_MODES:
        raise PrxError(f"wallpaper type {mode!r}: want one of none, horizontal, vertical, shift")
    m = WALLPAPER_MODES[mode]
    em = int(edge_match or 0)
    if m == 3:
        em = 0                           # the reference's shift branch ignores --wallpaper_edge_match
    if em == 1 or em < 0:
        raise PrxError(f"--wallpaper_edge_match {edge_match}: 0 (off) or >= 2 (the trim is edge_match // 2 on each side)")
    if shifts.dtype != torch.int32 or shifts.numel() != 2:
        raise PrxError("wallpaper: shifts must be a 2-element int32 device tensor")
    return _WallpaperFn.apply(x, shifts, m, em)


# --------------------------------------------------------------------------------------- pixel drawer (csrc/pixel_raster.hip)
PIXEL_TILE, PIXEL_MAX_VERTS = 16, 8


class PixelRasterGeometry:
    """Fixed polygons on a width x height canvas as the rasteriser reads them: vertices padded to 8, vertex counts, the per-tile
    shape lists (16 x 16-pixel tiles, row-major; the shapes whose bounding box, grown by 1e-3 px, meets the tile, ascending) and
    the inverse map (each shape's entries in those lists, in tile order).  `verts`: float32 [n, k <= 8, 2]."""

    def __init__(self, verts, width: int, height: int, device):
        import numpy as np
        v = np.asarray(verts, dtype=np.float32)
        if v.ndim != 3 or v.shape[2] != 2 or not 3 <= v.shape[1] <= PIXEL_MAX_VERTS or v.shape[0] < 1:
            raise PrxError(f"pixel raster: vertices must be [n >= 1, 3 .. {PIXEL_MAX_VERTS}, 2], got {v.shape}")
        n, k = v.shape[0], v.shape[1]
        self.width, self.height, self.n_shapes = int(width), int(height), n
        self.tiles_x = (self.width + PIXEL_TILE - 1) // PIXEL_TILE
        self.tiles_y = (self.height + PIXEL_TILE - 1) // PIXEL_TILE
        pad = np.zeros((n, PIXEL_MAX_VERTS, 2), dtype=np.float32)
        pad[:, :k] = v
        lo = v.astype(np.float64).min(axis=1) - 1e-3
        hi = v.astype(np.float64).max(axis=1) + 1e-3
        on = (hi[:, 0] >= 0) & (hi[:, 1] >= 0) & (lo[:, 0] < self.width) & (lo[:, 1] < self.height)
        tx0 = np.clip(np.floor(lo[:, 0] / PIXEL_TILE), 0, self.tiles_x - 1).astype(np.int64)
        tx1 = np.clip(np.floor(hi[:, 0] / PIXEL_TILE), 0, self.tiles_x - 1).astype(np.int64)
        ty0 = np.clip(np.floor(lo[:, 1] / PIXEL_TILE), 0, self.tiles_y - 1).astype(np.int64)
        ty1 = np.clip(np.floor(hi[:, 1] / PIXEL_TILE), 0, self.tiles_y - 1).astype(np.int64)
        nx = tx1 - tx0 + 1
        cnt = np.where(on, nx * (ty1 - ty0 + 1), 0)
        shape_start = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        total = int(shape_start[-1])
        shape_of = np.repeat(np.arange(n, dtype=np.int64), cnt)
        local = np.arange(total, dtype=np.int64) - np.repeat(shape_start[:-1], cnt)
        tile = (ty0[shape_of] + local // nx[shape_of]) * self.tiles_x + tx0[shape_of] + local % nx[shape_of]
        order = np.lexsort((shape_of, tile))                 # by tile, then by shape: the per-tile lists, ascending
        entry_of = np.empty(total, dtype=np.int64)
        entry_of[order] = np.arange(total, dtype=np.int64)   # each (shape, tile) pair's slot in the tile lists
        tile_start = np.concatenate([[0], np.cumsum(np.bincount(tile, minlength=self.tiles_x * self.tiles_y))])
        self.n_entries = total
        as_dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(device)    # noqa: E731
        self.verts = as_dev(pad, torch.float32)
        self.nverts = as_dev(np.full(n, k, dtype=np.int32), torch.int32)
        self.tile_start = as_dev(tile_start, torch.int32)
        self.tile_shapes = as_dev(shape_of[order], torch.int32)
        self.shape_start = as_dev(shape_start, torch.int32)
        self.shape_entries = as_dev(entry_of, torch.int32)

    def _args(self):
        return (self.verts, self.nverts)

    def _tiles(self):
        return (self.tile_start, self.tile_shapes, self.width, self.height)


def _pixel_seed(seed):
    if not isinstance(seed, torch.Tensor) or seed.dtype != torch.int32 or seed.numel() != 1:
        raise PrxError("pixel raster: the seed must be a one-word int32 device tensor")
    return seed


def _pixel_colors(colors, geom):
    if colors.dtype != torch.float32 or tuple(colors.shape) != (geom.n_shapes, 4):
        raise PrxError(f"pixel raster: colours must be fp32 [{geom.n_shapes}, 4], got {tuple(colors.shape)} {colors.dtype}")
    return colors.contiguous()


class _PixelRasterFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, colors, geom, seed):
        c = _pixel_colors(colors, geom)
        out = torch.empty(1, 4, geom.height, geom.width, device=c.device)
        call("prx_pixel_raster_fwd", *geom._args(), c, *geom._tiles(), seed, out, None, _stream())
        ctx.save_for_backward(c, seed)
        ctx.geom = geom
        return out

    @staticmethod
    def backward(ctx, g):
        c, seed = ctx.saved_tensors
        geom = ctx.geom
        partials = torch.empty(max(geom.n_entries, 1) * 4, dtype=torch.float64, device=c.device)
        grad = torch.empty_like(c)
        call("prx_pixel_raster_bwd", *geom._args(), c, *geom._tiles(), seed, g.contiguous(), partials, geom.shape_start,
             geom.shape_entries, geom.n_shapes, grad, _stream())
        return grad, None, None


def pixel_raster(colors, geom: PixelRasterGeometry, seed):
    """The pixel drawer's image [1, 4, H, W] (RGBA) of the shapes in `geom` filled with `colors` [n, 4], differentiable w.r.t.
    `colors`.  `seed`: a one-word int32 device tensor holding the jitter seed, read by the kernels (a replayed graph sees what was
    staged there last)."""
    _need_cuda(colors, seed)
    return _PixelRasterFn.apply(colors, geom, _pixel_seed(seed))


@torch.no_grad()
def pixel_raster_ids(colors, geom: PixelRasterGeometry, seed):
    """diagnostic: (image [1, 4, H, W], topmost shape id per sample [H, W, 4] int32, -1 where no shape covers the sample)"""
    _need_cuda(colors, seed)
    c = _pixel_colors(colors, geom)
    out = torch.empty(1, 4, geom.height, geom.width, device=c.device)
    ids = torch.empty(geom.height, geom.width, 4, dtype=torch.int32, device=c.device)
    call("prx_pixel_raster_fwd", *geom._args(), c, *geom._tiles(), _pixel_seed(seed), out, ids, _stream())
    return out, ids


def pixel_sample_offsets(width: int, height: int, seed):
    """diagnostic: the jitter (u, v) in [0, 1) of sample 2 sy + sx of every pixel, [H, W, 4, 2] fp32, for the seed in `seed`"""
    _need_cuda(seed)
    uv = torch.empty(int(height), int(width), 4, 2, device=seed.device)
    call("prx_pixel_sample_offsets", int(width), int(height), _pixel_seed(seed), uv, _stream())
    return uv


# --------------------------------------------------------------------------------------- stroke drawers (csrc/stroke_raster.hip)
STROKE_TILE, STROKE_MAX_POINTS = 16, 193
STROKE_MAX_PATHS = 16384
STROKE_MAX_WORKSPACE = 8 << 30          # bytes of fp64 partials the backward may ask for


class StrokeRasterScene:
    """The static sizes of a stroke scene and the kernels' workspaces, allocated once (the drawer's load_model): path k owns
    points[path_start[k] .. path_start[k + 1]) (1 + 3 S points for S cubic segments, at most STROKE_MAX_POINTS); the per-path
    boxes, the per-tile path lists ([tiles][n]: none can overflow) and the backward's per-(tile, path) partial gradients are
    sized from the path count, the longest path and the canvas alone, so that nothing is allocated or sized from device data
    in an iteration.  The geometry itself (points, widths) is read by every launch."""

    def __init__(self, path_start, width: int, height: int, device):
        import numpy as np
        ps = np.asarray(path_start, dtype=np.int64)
        if ps.ndim != 1 or len(ps) < 2 or ps[0] != 0:
            raise PrxError("stroke raster: path_start must be [n + 1] offsets from 0")
        counts = np.diff(ps)
        n = len(counts)
        if (counts < 1).any() or ((counts - 1) % 3 != 0).any():
            raise PrxError("stroke raster: every path needs 1 + 3 S points (S cubic segments)")
        if int(counts.max()) > STROKE_MAX_POINTS:
            raise PrxError(f"stroke raster: a path has {int(counts.max())} points; at most {STROKE_MAX_POINTS} "
                           f"({(STROKE_MAX_POINTS - 1) // 3} segments) are supported")
        if n > STROKE_MAX_PATHS:
            raise PrxError(f"stroke raster: {n} paths; at most {STROKE_MAX_PATHS} are supported")
        self.width, self.height, self.n_paths, self.n_points = int(width), int(height), n, int(ps[-1])
        if self.width < 1 or self.height < 1:
            raise PrxError(f"stroke raster: canvas {width} x {height}")
        self.max_points = int(counts.max())
        self.tiles = ((self.width + STROKE_TILE - 1) // STROKE_TILE) * ((self.height + STROKE_TILE - 1) // STROKE_TILE)
        self.slot = 2 * self.max_points + 5
        need = self.tiles * n * self.slot * 8
        if need > STROKE_MAX_WORKSPACE:
            raise PrxError(f"stroke raster: {n} paths of up to {self.max_points} points on a {width} x {height} canvas need "
                           f"{need / 2 ** 30:.1f} GiB of gradient partials; at most {STROKE_MAX_WORKSPACE >> 30} GiB are supported")
        self.device = torch.device(device)
        self.path_start = torch.from_numpy(ps.astype(np.int32)).to(self.device)
        self.boxes = torch.empty(n, 4, device=self.device)
        self.tile_count = torch.empty(self.tiles, dtype=torch.int32, device=self.device)
        self.tile_paths = torch.empty(self.tiles * n, dtype=torch.int32, device=self.device)
        self.partials = torch.empty(self.tiles * n * self.slot, dtype=torch.float64, device=self.device)
        self.paper_partials = torch.empty(self.tiles * 4, dtype=torch.float64, device=self.device)

    def _check(self, points, widths, colors, paper):
        n = self.n_paths
        for t, shape, what in ((points, (self.n_points, 2), "points"), (widths, (n,), "widths"), (colors, (n, 4), "colours")):
            if t.dtype != torch.float32 or tuple(t.shape) != shape:
                raise PrxError(f"stroke raster: {what} must be fp32 {list(shape)}, got {tuple(t.shape)} {t.dtype}")
        if paper is not None and (paper.dtype != torch.float32 or tuple(paper.shape) != (4,)):
            raise PrxError(f"stroke raster: the paper colour must be fp32 [4], got {tuple(paper.shape)} {paper.dtype}")


class _StrokeRasterFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, widths, colors, paper, scene, seed):
        scene._check(points, widths, colors, paper)
        p, w, c = points.contiguous(), widths.contiguous(), colors.contiguous()
        pa = paper.contiguous() if paper is not None else None
        out = torch.empty(scene.height, scene.width, 4, device=p.device)
        call("prx_stroke_raster_fwd", p, scene.path_start, scene.n_paths, scene.max_points, w, c, pa, scene.width, scene.height, seed,
             scene.boxes, scene.tile_count, scene.tile_paths, out, _stream())
        ctx.save_for_backward(p, w, c, pa, seed)
        ctx.scene = scene
        return out

    @staticmethod
    def backward(ctx, g):
        p, w, c, pa, seed = ctx.saved_tensors
        sc = ctx.scene
        gp, gw, gc = torch.empty_like(p), torch.empty_like(w), torch.empty_like(c)
        gpa = torch.empty_like(pa) if pa is not None and ctx.needs_input_grad[3] else None
        call("prx_stroke_raster_bwd", p, sc.path_start, sc.n_paths, sc.max_points, w, c, pa, sc.width, sc.height, seed, g.contiguous(),
             sc.boxes, sc.tile_count, sc.tile_paths, sc.partials, sc.paper_partials, gp, gw, gc, gpa, _stream())
        need = ctx.needs_input_grad
        return gp if need[0] else None, gw if need[1] else None, gc if need[2] else None, gpa, None, None


def stroke_raster(points, widths, colors, paper, scene: StrokeRasterScene, seed):
    """The stroke drawers' raster [H, W, 4] (RGBA, un-premultiplied) of the open cubic paths of `scene`: `points` [P, 2] in
    pixels, `widths` [n] (half-widths), `colors` [n, 4] RGBA, `paper` [4] RGBA under everything or None.  Differentiable
    w.r.t. all four.  `seed`: a one-word int32 device tensor holding the jitter seed, read by the kernels."""
    _need_cuda(points, widths, colors, seed)
    return _StrokeRasterFn.apply(points, widths, colors, paper, scene, _pixel_seed(seed))


def stroke_sample_offsets(width: int, height: int, seed):
    """diagnostic: the stroke kernels' jitter (u, v) of sample 2 sy + sx of every pixel, [H, W, 4, 2] fp32"""
    _need_cuda(seed)
    uv = torch.empty(int(height), int(width), 4, 2, device=seed.device)
    call("prx_stroke_sample_offsets", int(width), int(height), _pixel_seed(seed), uv, _stream())
    return uv
