"""TEST INFRASTRUCTURE: plain-torch restatement of the SLIP image tower (SLIP_Base.encode_image, slip.py:147-157), written from the
published architecture [UPSTREAM facebookresearch/SLIP models.py; timm vision_transformer.py VisionTransformer with
num_classes=0], not from any source text: the SLIP/ submodule of the reference checkout is empty.  dtype-generic (runs in the
dtype of the parameters it is given: float64 as the yardstick, float32 as the reference's own GPU arithmetic).

    x = conv2d(img, W[width,3,16,16], bias, stride 16) -> [N,196,width]
    x = cat([cls_token, x]) + pos_embed                     (no ln_pre)
    L x:  x = x + proj(MHA(LN1(x)));  x = x + fc2(GELU(fc1(LN2(x))))       LayerNorm eps 1e-6, exact GELU, qkv rows q|k|v
    e = LN(x)[:, 0] @ image_projection;  e / |e|

Parameter names are timm's state-dict ones (pixray_amd.weights.slip_vit_param_shapes)."""
import math

import torch
import torch.nn.functional as F

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def gelu(t):
    return 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))


def dgelu(t):
    """d gelu / dt = Phi(t) + t phi(t)"""
    return 0.5 * (1.0 + torch.erf(t / math.sqrt(2.0))) + t * torch.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)


def adjust_range(x, lo=None, hi=None):
    """slip.py:21-42 onto [0, 1]: the batch's own min / max when no range is given; divided only when the span is not 0"""
    lo = x.min() if lo is None else torch.as_tensor(lo, dtype=x.dtype)
    hi = x.max() if hi is None else torch.as_tensor(hi, dtype=x.dtype)
    span = hi - lo
    x = x - lo
    return x / span if float(span.detach()) != 0.0 else x


def normalize(x):
    mean = torch.tensor(IMAGENET_MEAN, dtype=x.dtype).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, dtype=x.dtype).view(1, 3, 1, 1)
    return (x - mean) / std


def attention(x, wqkv, bqkv, wproj, bproj, heads):
    n, t, w = x.shape
    hd = w // heads
    qkv = F.linear(x, wqkv, bqkv).view(n, t, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    a = torch.softmax((q @ k.transpose(-2, -1)) * hd ** -0.5, dim=-1)
    return F.linear((a @ v).transpose(1, 2).reshape(n, t, w), wproj, bproj)


def hidden_states(p, x, patch, layers, heads, eps=1e-6):
    """normalised images [N,3,R,R] -> the last hidden state after the final LayerNorm [N, T, width]"""
    w = p["patch_embed.proj.weight"].shape[0]
    x = F.conv2d(x, p["patch_embed.proj.weight"], p["patch_embed.proj.bias"], stride=patch).flatten(2).transpose(1, 2)
    x = torch.cat([p["cls_token"].expand(x.shape[0], -1, -1), x], 1) + p["pos_embed"]
    for i in range(layers):
        b = f"blocks.{i}."
        h = F.layer_norm(x, (w,), p[b + "norm1.weight"], p[b + "norm1.bias"], eps)
        x = x + attention(h, p[b + "attn.qkv.weight"], p[b + "attn.qkv.bias"], p[b + "attn.proj.weight"], p[b + "attn.proj.bias"], heads)
        h = F.layer_norm(x, (w,), p[b + "norm2.weight"], p[b + "norm2.bias"], eps)
        x = x + F.linear(gelu(F.linear(h, p[b + "mlp.fc1.weight"], p[b + "mlp.fc1.bias"])), p[b + "mlp.fc2.weight"], p[b + "mlp.fc2.bias"])
    return F.layer_norm(x, (w,), p["norm.weight"], p["norm.bias"], eps)


def encode_image(p, cfg, imgs, apply_preprocess=True, lo=None, hi=None):
    """SLIP_Base.encode_image on [N,3,224,224] inputs (Resize / CenterCrop are identities there): unit rows [N, output_dim]"""
    x = normalize(adjust_range(imgs, lo, hi)) if apply_preprocess else imgs
    h = hidden_states(p, x, cfg.patch_size, cfg.layers, cfg.heads, cfg.ln_eps)
    e = h[:, 0] @ p["image_projection"]
    return e / e.norm(dim=-1, keepdim=True)


def cast(params, dtype):
    return {k: v.to(dtype) for k, v in params.items()}


def embed_and_grad(params, cfg, cutouts, g_embeds, dtype=torch.float64):
    """(embeddings, d<embeddings, g_embeds>/d cutouts) in `dtype`"""
    p = cast(params, dtype)
    c = cutouts.detach().to(dtype).requires_grad_(True)
    e = encode_image(p, cfg, c)
    (gc,) = torch.autograd.grad((e * g_embeds.to(dtype)).sum(), c)
    return e.detach(), gc
