"""Host-side checks of the super_resolution drawer (no GPU): registration and front-end options, the new C-ABI prototypes, the
image -> z resize, canvas rounding, the RealESRGAN checkpoint adapter, and the synthetic initialisation's pre-clamp range
against the float64 restatement of the network (tests/_rrdbnet_ref.py)."""
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _rrdbnet_ref as R  # noqa: E402

from pixray_amd import _lib, checkpoints, frontend, plugins  # noqa: E402
from pixray_amd.super_resolution_drawer import SuperResolutionDrawer  # noqa: E402
from pixray_amd.weights import RRDBNET_CONFIGS, rrdbnet_param_shapes, synthetic_rrdbnet_params  # noqa: E402


def test_registered_and_accepted_by_the_front_end(tmp_path):
    assert plugins.class_table["super_resolution"] is SuperResolutionDrawer
    run = frontend.Run()
    run.settings = {}
    st = frontend.apply_settings(["--drawer", "super_resolution", "--super_resolution_model", "RealESRGAN_x4plus", "--outdir", str(tmp_path / "o")],
                                 run=run)
    assert st.drawer == "super_resolution" and st.super_resolution_model == "RealESRGAN_x4plus"
    assert "super_resolution" not in frontend.__doc__          # no longer listed among what is not carried over


def test_new_prototypes_parse():
    import ctypes
    protos = _lib.parse_header()
    names = {"prx_rrdbnet_create": 10, "prx_rrdbnet_destroy": 1, "prx_rrdbnet_synth": 5, "prx_rrdbnet_backward": 4, "prx_k_rrdb_conv": 30,
             "prx_k_rrdb_sum2x2": 6, "prx_k_rrdb_conv_first": 10, "prx_k_rrdb_conv_first_bwd": 9, "prx_k_rrdb_conv_last": 10,
             "prx_k_rrdb_conv_last_bwd": 8}
    for name, nargs in names.items():
        assert name in protos and len(protos[name][1]) == nargs, name
    assert protos["prx_rrdbnet_destroy"][0] is None and protos["prx_rrdbnet_create"][0] is ctypes.c_int
    assert protos["prx_k_rrdb_conv"][1][15] is ctypes.c_float and protos["prx_k_rrdb_conv"][1][16] is ctypes.c_float
    text = open(_lib.HEADER_PATH).read()
    assert "#define PRX_ABI_VERSION 3" in text


def _drawer(size, **kw):
    st = types.SimpleNamespace(size=size, drawer="super_resolution", super_resolution_model=kw.pop("model", "tiny-RRDB"), **kw)
    d = SuperResolutionDrawer(st)
    return d, st


def test_get_z_from_tensor_is_the_reference_expression():
    d, st = _drawer((28, 20))
    d.load_model(st, "cpu")
    t = torch.rand(1, 3, 20, 28, generator=torch.Generator().manual_seed(1)) * 2 - 1
    want = F.interpolate((t + 1) / 2, size=(torch.tensor(t.shape[-2:]) // 4).tolist(), mode="bilinear", align_corners=False)
    assert torch.equal(d.get_z_from_tensor(t), want) and tuple(want.shape) == (1, 3, 5, 7)
    d.init_from_tensor(t)
    assert torch.equal(d.get_z().detach(), want) and d.get_z().requires_grad
    d.reapply_from_tensor(-t)
    assert torch.equal(d.get_z().detach(), F.interpolate((1 - t) / 2, size=[5, 7], mode="bilinear", align_corners=False))
    d.set_z(torch.full((1, 3, 5, 7), 1.5))
    d.clip_z()
    assert float(d.get_z().detach().max()) == 1.0 and d.get_opts(1) is None


def test_init_from_none_is_seeded_mid_grey():
    d, st = _drawer((28, 20), weight_seed=3)
    d.load_model(st, "cpu")
    d.init_from_tensor(None)
    z = d.get_z().detach()
    assert tuple(z.shape) == (1, 3, 5, 7) and abs(float(z.mean()) - 0.5) < 0.05 and 0 < float(z.std()) < 0.1
    d2, st2 = _drawer((28, 20), weight_seed=3)
    d2.load_model(st2, "cpu")
    d2.init_from_tensor(None)
    assert torch.equal(d2.get_z().detach(), z)


def test_make_drawer_rounds_the_canvas_down_to_a_multiple_of_4(capsys):
    args = types.SimpleNamespace(drawer="super_resolution", size=(30, 22), super_resolution_model="tiny-RRDB")
    drawer, side = plugins.make_drawer(args, "cpu")
    assert side == (28, 20) and drawer.latent_hw == (5, 7) and drawer.get_num_resolutions() == 3
    assert "synthetic weights" in capsys.readouterr().out          # the one-line message: no checkpoint on disk
    with pytest.raises(ValueError, match="unknown super resolution model"):
        plugins.make_drawer(types.SimpleNamespace(drawer="super_resolution", size=(32, 32), super_resolution_model="nope"), "cpu")


def test_checkpoint_round_trip_and_strict_names(tmp_path):
    cfg = RRDBNET_CONFIGS["tiny-RRDB"]
    sd = synthetic_rrdbnet_params(cfg, 5)
    for key in ("params_ema", "params"):
        path = str(tmp_path / f"{key}.ckpt")
        torch.save({key: dict(sd)}, path)
        got = checkpoints.load_rrdbnet(path, cfg)
        assert list(got) == list(rrdbnet_param_shapes(cfg)) and all(torch.equal(got[k], sd[k]) for k in sd)
    both = str(tmp_path / "both.ckpt")
    torch.save({"params": {k: v + 1 for k, v in sd.items()}, "params_ema": dict(sd)}, both)
    assert torch.equal(checkpoints.load_rrdbnet(both, cfg)["conv_hr.bias"], sd["conv_hr.bias"])          # params_ema wins
    renamed = {("body.0.rdb2.convX.weight" if k == "body.0.rdb2.conv3.weight" else k): v for k, v in sd.items()}
    bad = str(tmp_path / "renamed.ckpt")
    torch.save({"params_ema": renamed}, bad)
    with pytest.raises(KeyError, match=r"body\.0\.rdb2\.conv3\.weight"):
        checkpoints.load_rrdbnet(bad, cfg)
    wrong = dict(sd)
    wrong["conv_up1.weight"] = torch.zeros(64, 32, 3, 3)
    torch.save({"params": wrong}, bad)
    with pytest.raises(ValueError, match=r"conv_up1\.weight"):
        checkpoints.load_rrdbnet(bad, cfg)
    torch.save({"state_dict": dict(sd)}, bad)
    with pytest.raises(KeyError, match="params_ema"):
        checkpoints.load_rrdbnet(bad, cfg)


def test_param_shapes_follow_the_architecture():
    cfg = RRDBNET_CONFIGS["RealESRGAN_x4plus"]
    sh = rrdbnet_param_shapes(cfg)
    assert len(sh) == 2 * (15 * 23 + 6) and (cfg.num_feat, cfg.num_grow_ch, cfg.num_block) == (64, 32, 23)
    assert list(sh)[:4] == ["conv_first.weight", "conv_first.bias", "body.0.rdb1.conv1.weight", "body.0.rdb1.conv1.bias"]
    assert sh["body.22.rdb3.conv4.weight"] == (32, 160, 3, 3) and sh["body.7.rdb2.conv5.weight"] == (64, 192, 3, 3)
    assert sh["conv_first.weight"] == (64, 3, 3, 3) and sh["conv_last.weight"] == (3, 64, 3, 3) and list(sh)[-1] == "conv_last.bias"
    tiny = RRDBNET_CONFIGS["tiny-RRDB"]
    assert (tiny.num_feat, tiny.num_grow_ch, tiny.num_block) == (64, 32, 1)


@pytest.mark.parametrize("seed", [0, 1])
def test_synthetic_init_does_not_start_saturated(seed):
    """z ~ U[0,1] at 16 x 16 through all 23 blocks in float64: between 2 % and 30 % of the pre-clamp values lie outside [0,1]
    (a Kaiming init with basicsr's x0.1 puts ~90 % outside); every bias is non-zero"""
    cfg = RRDBNET_CONFIGS["RealESRGAN_x4plus"]
    p = synthetic_rrdbnet_params(cfg, seed)
    assert all(bool((v != 0).all()) for k, v in p.items() if k.endswith(".bias"))
    z = torch.rand(1, 3, 16, 16, generator=torch.Generator().manual_seed(5 + seed))
    out, _ = R.run(p, z, cfg.num_block)
    outside = float(((out < 0) | (out > 1)).double().mean())
    print(f"[rrdb-fig] synthetic init seed {seed}: {outside:.4f} outside [0,1], range [{float(out.min()):.3f}, {float(out.max()):.3f}]")
    assert 0.02 <= outside <= 0.30
