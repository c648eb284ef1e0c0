"""TEST INFRASTRUCTURE: plain-torch restatement of the OpenCLIP ConvNeXt visual towers, written from the published architecture
[UPSTREAM timm convnext.py (ConvNeXt, ConvNeXtBlock with the MLP over channels-last pixels) and open_clip timm_model.py (the
projection head); neither package is installed], not from any source text.  dtype-generic: it runs in the dtype of the parameters it
is given (float64 as the yardstick).  It works on the UNFOLDED parameters of pixray_amd.weights.clip_convnext_param_shapes -- the
layer scale `gamma` is a multiply here -- so a comparison with the runner tests the host-side fold as well.

    x = LayerNorm_C(conv2d(normalize(adjust_range(img)), stem.0 [d0,3,4,4] + bias, stride 4))
    per stage i:  (i > 0)  x = conv2d(LayerNorm_C(x), downsample.1 [d(i), d(i-1), 2, 2] + bias, stride 2)
                  per block  x = x + gamma * fc2(GELU(fc1(LayerNorm_C(conv2d(x, conv_dw [C,1,7,7] + bias, padding 3, groups C)))))
    e = head(LayerNorm(mean_HW(x)));  e / |e|        head: proj.weight (no bias) | mlp.fc2.weight GELU(mlp.fc1 + bias) (no bias on fc2)
LayerNorm_C normalises over the channels of every pixel; exact (erf) GELU; eps from the configuration."""
import torch
import torch.nn.functional as F

from _openclip_ref import adjust_range, cast, gelu, normalize  # noqa: F401


def ln_c(x, w, b, eps):
    """LayerNorm over the channel axis of an NCHW map"""
    return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), w, b, eps).permute(0, 3, 1, 2)


def block(p, q, x, eps):
    c = x.shape[1]
    y = F.conv2d(x, p[q + "conv_dw.weight"], p[q + "conv_dw.bias"], padding=3, groups=c)
    h = F.layer_norm(y.permute(0, 2, 3, 1), (c,), p[q + "norm.weight"], p[q + "norm.bias"], eps)
    h = F.linear(gelu(F.linear(h, p[q + "mlp.fc1.weight"], p[q + "mlp.fc1.bias"])), p[q + "mlp.fc2.weight"], p[q + "mlp.fc2.bias"])
    return x + (h * p[q + "gamma"]).permute(0, 3, 1, 2)


def trunk(p, cfg, x):
    """normalised images [N,3,R,R] -> the last stage's map [N, d3, R/32, R/32]"""
    eps = cfg.ln_eps
    x = F.conv2d(x, p["trunk.stem.0.weight"], p["trunk.stem.0.bias"], stride=4)
    x = ln_c(x, p["trunk.stem.1.weight"], p["trunk.stem.1.bias"], eps)
    for i in range(4):
        s = f"trunk.stages.{i}."
        if i > 0:
            x = ln_c(x, p[s + "downsample.0.weight"], p[s + "downsample.0.bias"], eps)
            x = F.conv2d(x, p[s + "downsample.1.weight"], p[s + "downsample.1.bias"], stride=2)
        for b in range(cfg.depths[i]):
            x = block(p, f"{s}blocks.{b}.", x, eps)
    return x


def encode_image(p, cfg, imgs):
    """[N,3,R,R] cutouts at the tower's resolution -> unit rows [N, output_dim]"""
    x = trunk(p, cfg, normalize(adjust_range(imgs)))
    h = F.layer_norm(x.mean(dim=(2, 3)), (x.shape[1],), p["trunk.head.norm.weight"], p["trunk.head.norm.bias"], cfg.ln_eps)
    if cfg.proj == "linear":
        e = F.linear(h, p["head.proj.weight"])
    else:
        e = F.linear(gelu(F.linear(h, p["head.mlp.fc1.weight"], p["head.mlp.fc1.bias"])), p["head.mlp.fc2.weight"])
    return e / e.norm(dim=-1, keepdim=True)


def embed_and_grad(params, cfg, cutouts, g_embeds, dtype=torch.float64):
    """(embeddings, d<embeddings, g_embeds>/d cutouts) in `dtype`"""
    p = cast(params, dtype)
    c = cutouts.detach().to(dtype).requires_grad_(True)
    e = encode_image(p, cfg, c)
    (gc,) = torch.autograd.grad((e * g_embeds.to(dtype)).sum(), c)
    return e.detach(), gc
