"""TEST INFRASTRUCTURE: plain-torch restatement of the OpenCLIP (LAION) ViT towers, written from the published architecture
[UPSTREAM mlfoundations/open_clip model.py / transformer.py: VisionTransformer and the text Transformer built with nn.GELU;
the package is not installed], not from any source text.  dtype-generic: it runs in the dtype of the parameters it is given
(float64 as the yardstick).  Self-contained: nothing is read from oracle/ (whose ViT hard-codes QuickGELU).

Image side (state-dict names are OpenAI's, pixray_amd.weights.clip_vit_param_shapes):
    x = conv2d(img, conv1.weight[width,3,P,P], no bias, stride P) -> [N,G*G,width]
    x = ln_pre(cat([class_embedding, x]) + positional_embedding)
    L x:  x = x + out_proj(MHA(ln_1(x)));  x = x + c_proj(GELU(c_fc(ln_2(x))))     LayerNorm eps 1e-5, exact GELU, in_proj rows q|k|v
    e = ln_post(x[:, 0]) @ proj;  e / |e|                                          heads of width / heads columns, scale 1/sqrt(that)
Text side (pixray_amd.weights.clip_text_param_shapes):
    x = token_embedding[tokens] + positional_embedding;  L x the same block under the causal mask
    e = ln_final(x)[i, argmax_j tokens[i, j]] @ text_projection                    (not normalised)"""
import math

import torch
import torch.nn.functional as F

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def gelu(t):
    return 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))


def quick_gelu(t):
    return t * torch.sigmoid(1.702 * t)


def adjust_range(x):
    """onto [0, 1] by the batch's own min / max; divided only when the span is not 0"""
    lo, hi = x.min(), x.max()
    x = x - lo
    return x / (hi - lo) if float((hi - lo).detach()) != 0.0 else x


def normalize(x):
    mean = torch.tensor(CLIP_MEAN, dtype=x.dtype).view(1, 3, 1, 1)
    std = torch.tensor(CLIP_STD, dtype=x.dtype).view(1, 3, 1, 1)
    return (x - mean) / std


def attention(x, p, b, heads, causal=False):
    n, t, w = x.shape
    hd = w // heads
    qkv = F.linear(x, p[b + "attn.in_proj_weight"], p[b + "attn.in_proj_bias"]).view(n, t, 3, heads, hd).permute(2, 0, 3, 1, 4)
    s = (qkv[0] @ qkv[1].transpose(-2, -1)) * hd ** -0.5
    if causal:
        s = s.masked_fill(torch.ones(t, t, dtype=torch.bool).triu(1), float("-inf"))
    o = (torch.softmax(s, dim=-1) @ qkv[2]).transpose(1, 2).reshape(n, t, w)
    return F.linear(o, p[b + "attn.out_proj.weight"], p[b + "attn.out_proj.bias"])


def blocks(p, x, layers, heads, causal=False, act=gelu):
    w = x.shape[-1]
    for i in range(layers):
        b = f"transformer.resblocks.{i}."
        x = x + attention(F.layer_norm(x, (w,), p[b + "ln_1.weight"], p[b + "ln_1.bias"], 1e-5), p, b, heads, causal)
        h = F.layer_norm(x, (w,), p[b + "ln_2.weight"], p[b + "ln_2.bias"], 1e-5)
        x = x + F.linear(act(F.linear(h, p[b + "mlp.c_fc.weight"], p[b + "mlp.c_fc.bias"])), p[b + "mlp.c_proj.weight"], p[b + "mlp.c_proj.bias"])
    return x


def encode_image(p, cfg, imgs):
    """[N,3,R,R] cutouts at the tower's resolution -> unit rows [N, output_dim]"""
    w = cfg.width
    x = normalize(adjust_range(imgs))
    x = F.conv2d(x, p["conv1.weight"], None, stride=cfg.patch_size).flatten(2).transpose(1, 2)
    x = torch.cat([p["class_embedding"].expand(x.shape[0], 1, -1), x], 1) + p["positional_embedding"]
    x = F.layer_norm(x, (w,), p["ln_pre.weight"], p["ln_pre.bias"], 1e-5)
    x = blocks(p, x, cfg.layers, cfg.heads)
    e = F.layer_norm(x[:, 0], (w,), p["ln_post.weight"], p["ln_post.bias"], 1e-5) @ p["proj"]
    return e / e.norm(dim=-1, keepdim=True)


def encode_text(p, cfg, tokens, act=gelu):
    """int tokens [n, context] -> [n, output_dim], not normalised"""
    x = p["token_embedding.weight"][tokens.long()] + p["positional_embedding"]
    x = blocks(p, x, cfg.layers, cfg.heads, causal=True, act=act)
    x = F.layer_norm(x, (cfg.width,), p["ln_final.weight"], p["ln_final.bias"], 1e-5)
    return x[torch.arange(x.shape[0]), tokens.long().argmax(dim=-1)] @ p["text_projection"]


def cast(params, dtype):
    return {k: v.to(dtype) for k, v in params.items()}


def embed_and_grad(params, cfg, cutouts, g_embeds, dtype=torch.float64):
    """(embeddings, d<embeddings, g_embeds>/d cutouts) in `dtype`"""
    p = cast(params, dtype)
    c = cutouts.detach().to(dtype).requires_grad_(True)
    e = encode_image(p, cfg, c)
    (gc,) = torch.autograd.grad((e * g_embeds.to(dtype)).sum(), c)
    return e.detach(), gc
