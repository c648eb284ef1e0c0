"""TEST INFRASTRUCTURE: a float64 restatement of RRDBNet x4 (basicsr's public architecture, as the super_resolution drawer
uses it) in plain torch on the CPU, written from the architecture's description; the yardsticks of the RRDBNet tests are
computed from it at the tests' own shapes.

`mode`:
  "f64"   plain float64;
  "f32"   torch's own fp32 evaluation of the same network (the yardstick of the exact-f32 kernels);
  "half"  float64 with every convolution's weights and input, and every gradient entering a convolution's data gradient,
          rounded to IEEE half (the yardstick of the half-operand kernels)."""
import torch
import torch.nn.functional as F


def q16(t):
    return t.half().to(t.dtype)


class _ConvQ(torch.autograd.Function):
    """conv2d(q16(x), q16(w)) + b, whose data gradient is taken of q16(g)"""

    @staticmethod
    def forward(ctx, x, w, b):
        wq = q16(w)
        ctx.save_for_backward(wq)
        return F.conv2d(q16(x), wq, b, padding=1)

    @staticmethod
    def backward(ctx, g):
        (wq,) = ctx.saved_tensors
        return F.conv_transpose2d(q16(g), wq, padding=1), None, None


def conv(x, w, b, mode):
    if mode == "half":
        return _ConvQ.apply(x, w, b)
    return F.conv2d(x, w, b, padding=1)


def lrelu(x):
    return F.leaky_relu(x, 0.2)


def cast_params(params, mode):
    dt = torch.float32 if mode == "f32" else torch.float64
    return {k: v.detach().to(dt) for k, v in params.items()}


def rdb(p, pre, x, mode):
    c = lambda k, t: conv(t, p[f"{pre}.conv{k}.weight"], p[f"{pre}.conv{k}.bias"], mode)
    x1 = lrelu(c(1, x))
    x2 = lrelu(c(2, torch.cat((x, x1), 1)))
    x3 = lrelu(c(3, torch.cat((x, x1, x2), 1)))
    x4 = lrelu(c(4, torch.cat((x, x1, x2, x3), 1)))
    x5 = c(5, torch.cat((x, x1, x2, x3, x4), 1))
    return x5 * 0.2 + x


def rrdbnet(params, z, num_block, mode="f64"):
    """z [1,3,h,w] -> the raw network output [1,3,4h,4w] (no clamp); `params` already cast (cast_params)"""
    p = params
    c = lambda n, t: conv(t, p[n + ".weight"], p[n + ".bias"], mode)
    feat = c("conv_first", z)
    x = feat
    for i in range(num_block):
        y = x
        for r in (1, 2, 3):
            y = rdb(p, f"body.{i}.rdb{r}", y, mode)
        x = y * 0.2 + x
    feat = feat + c("conv_body", x)
    feat = lrelu(c("conv_up1", F.interpolate(feat, scale_factor=2, mode="nearest")))
    feat = lrelu(c("conv_up2", F.interpolate(feat, scale_factor=2, mode="nearest")))
    return c("conv_last", lrelu(c("conv_hr", feat)))


def run(params, z, num_block, g=None, mode="f64"):
    """-> (raw output, d<raw, g>/dz) in float64"""
    p = cast_params(params, mode)
    dt = torch.float32 if mode == "f32" else torch.float64
    zz = z.detach().to(dt).requires_grad_(True)
    out = rrdbnet(p, zz, num_block, mode)
    if g is None:
        return out.detach().double(), None
    (dz,) = torch.autograd.grad(out, zz, g.to(dt))
    return out.detach().double(), dz.double()


def clamp_rule(g, x):
    """clamp_with_grad's backward: g * ((g * (x - clamp(x, 0, 1))) >= 0)"""
    return g * ((g * (x - x.clamp(0, 1))) >= 0)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


class ClampWithGrad(torch.autograd.Function):
    """clamp(x, 0, 1) whose backward passes g where it does not push further out of range (`clamp_rule`)"""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return x.clamp(0, 1)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return clamp_rule(g, x)


def run_clamped(params, z, num_block, g, mode="f64"):
    """-> (raw output, clamped image, d<image, g>/dz) in float64"""
    p = cast_params(params, mode)
    dt = torch.float32 if mode == "f32" else torch.float64
    zz = z.detach().to(dt).requires_grad_(True)
    raw = rrdbnet(p, zz, num_block, mode)
    img = ClampWithGrad.apply(raw)
    (dz,) = torch.autograd.grad(img, zz, g.to(dt))
    return raw.detach().double(), img.detach().double(), dz.double()
