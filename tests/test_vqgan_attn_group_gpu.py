"""The decoder's AttnBlock launch sequence (csrc/vqgan.hip, PRX_VQ_ATTN_GROUP): with the switch on (default) the two transposes ride
on the softmax launches and dq / dk / dv are one grouped GEMM launch; with it off the block runs its separate launches.  Neither
form changes a single operation on a single element, so image and latent gradient must be byte-identical -- no tolerance."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from pixray_amd import _lib, ops
from pixray_amd.weights import VqganConfig, synthetic_vqgan_params

DEV = "cuda"

# a reduced decoder whose three AttnBlocks (the middle one and two at the 16-nominal level) have C = 128: 32 GroupNorm groups of 4
# channels, the smallest width at which the GEMM epilogues still carry the GroupNorm sums, as they do at the headline's C = 512
CFG = VqganConfig(ch=128, ch_mult=(1, 1), num_res_blocks=1, attn_resolutions=(16,), resolution=32, z_channels=64, embed_dim=64, n_embed=256)
N_ATTN = 3


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _decoder_pass(monkeypatch, switch, params, latent_hw, precision, z, g):
    monkeypatch.setenv("PRX_VQ_ATTN_GROUP", switch)          # read once, when the handle is created
    h = ops.VqganHandle(CFG, params, latent_hw, torch.device(DEV), precision=precision)
    lib = _lib.load()
    zz = z.clone().requires_grad_(True)
    img = ops.vqgan_synth(zz, h, quantize=True)
    n0 = lib.prx_gemm_group_launches()
    img.backward(g)
    torch.cuda.synchronize()
    return img.detach(), zz.grad.detach(), lib.prx_gemm_group_launches() - n0


@pytest.mark.parametrize("precision", ["fp16", "bf16", "f32"])
@pytest.mark.parametrize("latent_hw", [(5, 7), (16, 16)])      # 35 tokens in pitch 40 (padded operands), and 256 tokens
def test_attn_group_switch_leaves_image_and_latent_gradient_bytes(monkeypatch, precision, latent_hw):
    torch.manual_seed(latent_hw[0])
    params = synthetic_vqgan_params(CFG, seed=1)
    z = torch.randn(1, CFG.z_channels, *latent_hw, device=DEV)
    g = torch.randn(1, CFG.out_ch, 2 * latent_hw[0], 2 * latent_hw[1], device=DEV)
    img1, dz1, n1 = _decoder_pass(monkeypatch, "1", params, latent_hw, precision, z, g)
    img0, dz0, n0 = _decoder_pass(monkeypatch, "0", params, latent_hw, precision, z, g)
    assert torch.isfinite(dz1).all() and dz1.abs().max() > 0
    assert torch.equal(_bytes(img1), _bytes(img0))
    assert torch.equal(_bytes(dz1), _bytes(dz0))
    # one grouped launch per AttnBlock and backward; the exact mode's products plan onto the fp32 4-wave kernels, which have no
    # grouped form, and run as separate launches through the same entry
    assert n1 == (0 if precision == "f32" else N_ATTN), n1
    assert n0 == 0, n0
