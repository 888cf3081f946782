"""RegionCLIP ModifiedResNet backbone, host side: the float64 restatement against the reference's fixture, the weight conversion
(FrozenBN -> scale / shift, both checkpoint formats) and the config rules (quirk 1's table, quirk 2's token split, the refusals)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import regionclip_ref as RR
from patchioner_amd import weights as W
from patchioner_amd.backbones import _regionclip_setup
from patchioner_amd.model import Patchioner

GOLD = os.path.join(os.path.dirname(__file__), "golden", "regionclip.npz")
LAYERS = (1, 1, 1, 1)
CASES = (("RN50", 224, 11), ("RN50x4", 288, 12))     # tools/oracle/gen_golden_regionclip.py


def _case(name, res, seed):
    sd = W.synth_regionclip_rn(seed, name, layers=LAYERS, image_resolution=res)
    return W.regionclip_to_engine(sd), W.synth_images(seed + 100, 1, res)


@pytest.mark.parametrize("name,res,seed", CASES)
def test_float64_restatement_matches_the_reference_fp32_tower(name, res, seed):
    g = np.load(GOLD)
    esd, imgs = _case(name, res, seed)
    heads = W.regionclip_arch(name)[3]
    t64 = RR.tokens64(esd, imgs, LAYERS, heads).numpy()
    ref = g["%s_%d_tok32" % (name, res)]
    assert t64.shape == ref.shape
    # the reference's fp32 run against float64: sums of <= 4608 products per conv output, 7 convs deep, then unit-norm rows
    assert np.abs(t64 - ref).max() < 2e-5 * max(1.0, np.abs(ref).max() / 0.1)
    # the fp16 statement (rounding where the fp16 tower rounds) against the reference's own fp16 run: the sums' order differs, so
    # within a few of the fp16-vs-fp32 gap the fixture itself shows
    t16 = RR.tokens64(esd, imgs, LAYERS, heads, rnd=torch.float16).numpy()
    r16 = g["%s_%d_tok16" % (name, res)].astype(np.float64)
    gap = np.abs(r16 - ref).max()
    assert np.abs(t16 - r16).max() < 4 * gap


def test_cproj_patch_rows_without_attnpool():
    g = np.load(GOLD)
    esd, imgs = _case("RN50", 224, 11)
    t16 = RR.tokens64(esd, imgs, LAYERS, 32, spatial_attn=False, rnd=torch.float16).numpy()
    r16 = g["RN50_224_cproj_tok16"].astype(np.float64)
    gap = np.abs(g["RN50_224_tok16"].astype(np.float64) - g["RN50_224_tok32"]).max()
    assert np.abs(t16 - r16).max() < 4 * gap
    assert np.abs(t16[:, 0] - g["RN50_224_tok16"][:, 0]).max() < 4 * gap     # row 0 stays the attnpool's


def test_frozen_bn_scale_shift_is_eval_batch_norm():
    torch.manual_seed(0)
    c = 24
    w, b, m, v = torch.rand(c) + 0.5, torch.randn(c), torch.randn(c), torch.rand(c) + 0.1
    x = torch.randn(2, c, 5, 5)
    sc, sh = W.frozen_bn_affine(w, b, m, v)
    want = F.batch_norm(x, m, v, w, b, training=False, eps=1e-5)
    torch.testing.assert_close(x * sc[None, :, None, None] + sh[None, :, None, None], want, rtol=1e-6, atol=1e-6)


def test_both_checkpoint_formats_give_the_same_engine_weights():
    vis = W.synth_regionclip_rn(3, "RN50", layers=LAYERS)
    rc = {"model": {("backbone." + k[len("visual."):]): v for k, v in vis.items() if k.startswith("visual.")}}
    rc["model"]["lang_encoder.token_embedding.weight"] = torch.zeros(4, 4)
    a, b = W.regionclip_to_engine(vis), W.regionclip_to_engine(rc)
    assert a.keys() == b.keys()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert all(k.startswith("rn.") for k in a) and "rn.layer1.0.bn3.scale" in a and "rn.layer2.0.downsample.1.shift" in a
    assert not any(k.endswith(("running_mean", "running_var")) for k in a)
    C = 2048
    assert a["rn.attnpool.qkv.weight"].shape == (3 * C, C)
    assert torch.equal(a["rn.attnpool.qkv.weight"][C:2 * C], vis["visual.attnpool.k_proj.weight"])
    assert W.regionclip_layers(rc) == (LAYERS, 64, 7, 1024)
    assert W.regionclip_arch(200) == W.regionclip_arch("RN50x4") and W.regionclip_arch((3, 4, 6, 3))[1] == 64
    with pytest.raises(KeyError):
        W.regionclip_to_engine({"transformer.x": torch.zeros(1)})


def test_quirk1_position_table_is_redrawn_from_the_default_generator(capsys):
    cfg = {"MODEL": {"RESNETS": {"OUT_FEATURES": ["res4", "res5"], "IMAGE_RESOLUTION": 512}}, "patch_size": 32}
    torch.manual_seed(5)
    a = _regionclip_setup(dict(cfg, checkpoint=W.synth_regionclip_rn(1, "RN50", layers=LAYERS)), "regionclip_resnet50_p32.k", 512, None, None)
    out = capsys.readouterr().out
    assert "Removing incompatible positional embedding" in out and "Checkpoint spatial size: 7x7" in out and "requires 16x16" in out
    pos = a.state_dict["rn.attnpool.positional_embedding"]
    torch.manual_seed(5)
    want = torch.randn(16 * 16 + 1, 2048) / 2048 ** 0.5
    assert torch.equal(pos, want)
    # the native size keeps the checkpoint's table, silently
    b = _regionclip_setup(dict(cfg, MODEL={"RESNETS": {"OUT_FEATURES": ["res5"], "IMAGE_RESOLUTION": 224}}), "regionclip_x", 224, 0, None)
    assert "Removing" not in capsys.readouterr().out and b.state_dict["rn.attnpool.positional_embedding"].shape == (50, 2048)
    with pytest.raises(RuntimeError, match="must match"):       # the table is for IMAGE_RESOLUTION, the crop is another size
        _regionclip_setup(dict(cfg, checkpoint=W.synth_regionclip_rn(1, "RN50", layers=LAYERS)), "regionclip_x", 224, None, None)


def test_refusals_come_before_the_device():
    base = {"prefix_size": 1024, "support_memory_size": 0, "synthetic_seed": 0, "dino_model": "regionclip_resnet50_p32.k",
            "resize_dim": 224, "crop_dim": 224}
    rc = {"patch_size": 32, "MODEL": {"RESNETS": {"OUT_FEATURES": ["res4"], "IMAGE_RESOLUTION": 224}}}
    with pytest.raises(NotImplementedError, match="stride-16"):
        Patchioner.from_config(dict(base, regionclip_config=rc), device="cuda")
    rc5 = {"patch_size": 32, "MODEL": {"RESNETS": {"OUT_FEATURES": ["res4", "res5"], "IMAGE_RESOLUTION": 224}}}
    with pytest.raises(NotImplementedError, match="text tower"):
        Patchioner(None, "cuda", 1024, False, 10, dino_model="regionclip_resnet50_p32.k", regionclip_config=rc5, online_texts=["a"],
                   synthetic_seed=0, resize_dim=224, crop_dim=224)
    with pytest.raises(NotImplementedError, match="patch_size"):
        Patchioner.from_config(dict(base, regionclip_config=dict(rc5, patch_size=16)), device="cuda")
    with pytest.raises(FileNotFoundError):
        Patchioner.from_config(dict(base, synthetic_seed=None, decap_weights="x.pt", regionclip_config=rc5), device="cuda")
    with pytest.raises(ValueError):                 # without regionclip_config an RN name is still an unknown backbone
        Patchioner.from_config(dict(base, dino_model="RN50x4"), device="cuda")


def test_fp32_checkpoint_weights_become_the_fp16_values_the_reference_computes_with():
    """loader.py runs convert_weights before loading: every Conv2d / Linear weight and bias is an fp16 value; FrozenBN buffers and
    the attnpool's position table stay fp32.  A checkpoint whose values are NOT fp16 values must give the engine the rounded ones."""
    vis = W.synth_regionclip_rn(4, "RN50", layers=LAYERS)
    g = torch.Generator().manual_seed(9)
    raw = {k: (v + 1e-4 * torch.randn(v.shape, generator=g)) if v.is_floating_point() else v for k, v in vis.items()}
    e = W.regionclip_to_engine(raw)
    for k in ("rn.conv1.weight", "rn.layer2.0.conv2.weight", "rn.layer3.0.downsample.0.weight", "rn.attnpool.qkv.weight",
              "rn.attnpool.qkv.bias", "rn.attnpool.c_proj.weight", "rn.attnpool.c_proj.bias"):
        assert torch.equal(e[k], e[k].half().float()), k
    assert torch.equal(e["rn.conv1.weight"], raw["visual.conv1.weight"].half().float())
    assert torch.equal(e["rn.attnpool.c_proj.bias"], raw["visual.attnpool.c_proj.bias"].half().float())
    pos = raw["visual.attnpool.positional_embedding"]
    assert not torch.equal(pos, pos.half().float()) and torch.equal(e["rn.attnpool.positional_embedding"], pos)
    sc, _ = W.frozen_bn_affine(raw["visual.bn1.weight"], raw["visual.bn1.bias"], raw["visual.bn1.running_mean"], raw["visual.bn1.running_var"])
    assert torch.equal(e["rn.bn1.scale"], sc)                   # from the fp32 buffers, not rounded
