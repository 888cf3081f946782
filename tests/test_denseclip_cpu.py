"""DenseCLIP backbone, host side: config resolution in its three forms, the reference's routing order, the loader (only ``backbone.``
keys, nothing rounded), every refusal with its exception type, the bank file names, and the float tower (tests/denseclip_ref.py) against
the reference's own fp32 tokens and captions (tests/golden/denseclip.npz) -- all without a GPU."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

import denseclip_ref as DR
from patchioner_amd import denseclip as DC
from patchioner_amd import weights as W

torch.set_grad_enabled(False)
TAGS = list(DR.TOWERS)


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "denseclip.npz"))
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def meta(gold):
    return json.loads(bytes(gold["meta_json"]).decode())


# ---- the float tower against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_float_tower_matches_the_reference_tokens(gold, tag):
    """Both are fp32 evaluations of the same fp32 weights: <= 1e-5 of max |ref|.  Also the distance of the REFERENCE's fp32 tokens from
    a float64 evaluation, which the GPU test of the fp32 mode takes its bar from (DR.REF_FP32_VS_F64: the recorded value holds)."""
    t = DR.TOWERS[tag]
    ref = gold[tag + "__tokens"]
    imgs = DR.images(tag)
    got = DR.tower(tag).tokens(imgs)[:, ::t["stride"]].numpy()
    assert got.shape == ref.shape
    err = np.abs(got - ref).max() / np.abs(ref).max()
    t64 = DR.tower(tag, torch.float64).tokens(imgs)[:, ::t["stride"]].numpy()
    d64 = np.abs(ref - t64).max() / np.abs(ref).max()
    print("DenseCLIP %s: float tower vs reference %.2e; reference fp32 vs float64 %.3e (recorded %.3e)" % (tag, err, d64, DR.REF_FP32_VS_F64[tag]))
    assert err <= 1e-5, (tag, err)
    assert 0 < d64 <= DR.REF_FP32_VS_F64[tag] * 1.0001, (tag, d64)


def test_float_driver_reproduces_the_reference_captions_without_near_ties(gold, meta):
    from parity_helpers import MARGIN_BOUND
    for tag in TAGS:
        res = DR.TOWERS[tag]["resolution"]
        orc, dec = DR.driver(tag)
        for name, kw in DR.FORWARD_CASES:
            orc.call_log, orc.prefix_log = [], []
            outs = orc.forward(DR.images(tag), **DR.forward_args(kw, res))
            key = tag + "__" + name
            assert np.array_equal(torch.cat(orc.call_log).numpy(), gold[key + "__ids"]), key
            assert outs == meta[key], key
            P = torch.cat(orc.prefix_log)
            _, _, margin = dec.decode_ids(P[torch.isfinite(P).all(1)], cached=True)
            print("DenseCLIP %s: smallest top-2 margin of the reference's greedy steps %.3e" % (key, float(margin.min())))
            assert float(margin.min()) > MARGIN_BOUND, (key, float(margin.min()))


# ---- config resolution -------------------------------------------------------------------------------------------------------
def test_config_resolves_in_all_three_forms(tmp_path, monkeypatch):
    monkeypatch.delenv(DC.CONFIG_DIR_ENV, raising=False)
    d = DR.config("r128")
    got = DC.resolve_config(d)
    assert got == d and got is not d and got["model"] is not d["model"]           # a deep copy
    p = tmp_path / "my_denseclip.yaml"
    p.write_text(yaml.safe_dump(d))
    assert DC.resolve_config(str(p)) == d                                          # a .yaml path
    assert DC.resolve_config("my_denseclip", config_dir=str(tmp_path)) == d        # a bare name in a directory given by keyword
    assert DC.resolve_config("my_denseclip.yaml", config_dir=str(tmp_path)) == d   # the reference appends .yaml only when missing
    monkeypatch.setenv(DC.CONFIG_DIR_ENV, str(tmp_path))
    assert DC.resolve_config("my_denseclip") == d                                  # ... or by the package's environment variable
    monkeypatch.delenv(DC.CONFIG_DIR_ENV)
    with pytest.raises(FileNotFoundError, match="does not exist"):
        DC.resolve_config("my_denseclip")
    with pytest.raises(FileNotFoundError, match="does not exist"):
        DC.resolve_config("nothing_here", config_dir=str(tmp_path))
    with pytest.raises(TypeError):
        DC.resolve_config(7)
    # a file in the directory wins over a built-in name
    (tmp_path / "denseclip_segmentation_vitb16.yaml").write_text(yaml.safe_dump(d))
    assert DC.resolve_config("denseclip_segmentation_vitb16", config_dir=str(tmp_path)) == d


def test_built_in_names_hold_the_shipped_settings(monkeypatch):
    monkeypatch.delenv(DC.CONFIG_DIR_ENV, raising=False)
    assert set(DC.BUILTIN) == set(DR.SHIPPED_CONFIG_NAMES)
    for name, ctx, ck in (("denseclip_segmentation_vitb16", 13, "ViT-B-DenseCLIP.pth"),
                          ("denseclip_segmentation_vitb16_long_ctx", 77, "ViT-B-DenseCLIP_long_ctx.pth")):
        cfg = DC.resolve_config(name)
        assert cfg["model"]["vision"] == {"image_resolution": 640, "vision_layers": 12, "vision_width": 768, "vision_patch_size": 16,
                                          "embed_dim": 512}
        assert cfg["model"]["text"]["context_length"] == ctx and cfg["model"]["text"]["transformer_width"] == 512
        assert os.path.basename(cfg["checkpoint"]["path"]) == ck
        assert cfg["preprocessing"]["image_mean"] == [0.48145466, 0.4578275, 0.40821073]
        cfg["model"]["vision"]["image_resolution"] = 1                             # the built-in table is not the caller's to change
        assert DC.resolve_config(name)["model"]["vision"]["image_resolution"] == 640
        assert DC.vision_block(DC.resolve_config(name))["vision_width"] == 768
    with pytest.raises(KeyError, match="vision_layers"):
        DC.vision_block({"model": {"vision": {"image_resolution": 640}}})


# ---- routing -----------------------------------------------------------------------------------------------------------------
def test_routing_follows_the_references_elif_chains():
    from patchioner_amd.backbones import _denseclip_routed
    from patchioner_amd.model import _OUT_OF_SCOPE
    assert _OUT_OF_SCOPE == ("proxyclip_clipmodel",)
    dc = "denseclip_segmentation_vitb16"
    assert _denseclip_routed("INViTE_B16", dc)
    assert not _denseclip_routed(None, dc)                          # reached only with a dino_model
    assert not _denseclip_routed("INViTE_B16", None)
    for name in ("dinov2_vitb14_reg", "vit_base_patch16_clip_224.openai", "my_patch16", "x_patch14", "x_patch32", "foo.openai"):
        assert not _denseclip_routed(name, dc), name                # the name tests in front of it win
    assert not _denseclip_routed("INViTE_B16", dc, regionclip_config={"checkpoint": "x"})
    assert not _denseclip_routed("INViTE_B16", dc, invite_config={"name": "ViT-B/16"})


def _cfg(dc, res=128, **over):
    cfg = {"decap_weights": None, "prefix_size": 512, "support_memory_size": 0, "dino_model": "INViTE_B16", "normalize": False,
           "resize_dim": res, "crop_dim": res, "clip_model_name": "ViT-B/16", "use_talk2dino_project": False, "synthetic_seed": 3,
           "denseclip_config": dc}
    cfg.update(over)
    return cfg


def _build(cfg, **kw):
    from patchioner_amd import Patchioner
    return Patchioner.from_config(cfg, device="cpu", **kw)


def test_with_everything_in_order_the_constructor_reaches_the_device_check(tmp_path, monkeypatch):
    """The constructor gets as far as the device, and says that there is no CPU path (before this backbone existed: NotImplementedError)."""
    monkeypatch.delenv(DC.CONFIG_DIR_ENV, raising=False)
    with pytest.raises(RuntimeError, match="MI355X"):
        _build(_cfg(DR.config("r128")))                                                    # a dict, synthetic weights
    with pytest.raises(RuntimeError, match="MI355X"):
        _build(_cfg("denseclip_segmentation_vitb16_long_ctx", res=640))                    # a built-in name, as the YAML gives it
    p = tmp_path / "tower.yaml"
    p.write_text(yaml.safe_dump(DR.config("r224")))
    with pytest.raises(RuntimeError, match="MI355X"):
        _build(_cfg(str(p), res=224, synthetic_seed=None, decap_weights=W.synth_decap(1, prefix_size=512, n_layer=1),
                    denseclip_checkpoint=DR.checkpoint("r224")))                           # a path, the checkpoint as a state dict
    with pytest.raises(RuntimeError, match="MI355X"):
        _build(_cfg("tower", res=224, denseclip_config_dir=str(tmp_path)))                 # a name in a directory
    # a dino_model that the reference's name tests take wins over denseclip_config: the DINOv2 / timm-CLIP constructors run
    with pytest.raises(RuntimeError, match="MI355X"):
        _build(_cfg({"not": "read"}, res=224, dino_model="dinov2_vitb14_reg"))
    with pytest.raises(RuntimeError, match="MI355X"):
        _build(_cfg({"not": "read"}, res=224, dino_model="vit_base_patch16_clip_224.openai"))
    # beside invite_config or regionclip_config it keeps raising
    for other in (dict(invite_config={"name": "ViT-B/16"}), dict(regionclip_config={"checkpoint": None})):
        with pytest.raises(NotImplementedError):
            _build(_cfg(DR.config("r128"), **other))
    with pytest.raises(NotImplementedError):
        _build(_cfg(DR.config("r128"), proxyclip_clipmodel="ViT-B/16"))


def test_refusals_come_before_the_device_is_touched(tmp_path):
    ck = DR.checkpoint("r128")
    dec = W.synth_decap(1, prefix_size=512, n_layer=1)
    base = dict(synthetic_seed=None, decap_weights=dec)
    # a checkpoint without 'state_dict': the reference's text
    with pytest.raises(ValueError, match="Checkpoint doesn't contain 'state_dict'"):
        _build(_cfg(DR.config("r128"), denseclip_checkpoint=dict(ck["state_dict"]), **base))
    # a missing checkpoint file: the reference would caption with RANDOM weights
    with pytest.raises(FileNotFoundError, match="RANDOM"):
        _build(_cfg(DR.config("r128"), **base))
    with pytest.raises(FileNotFoundError, match="RANDOM"):
        _build(_cfg(DR.config("r128"), denseclip_checkpoint="/nonexistent/ViT-B-DenseCLIP.pth"))       # even with a synthetic_seed
    # a tower tensor the checkpoint lacks: ln_post and proj included
    for key in ("ln_post.weight", "proj", "transformer.resblocks.2.mlp.c_proj.bias", "class_embedding"):
        sd = {k: v for k, v in ck["state_dict"].items() if k != "backbone." + key}
        with pytest.raises(KeyError, match=key.replace(".", r"\.")):
            _build(_cfg(DR.config("r128"), denseclip_checkpoint={"state_dict": sd}, **base))
    # a position table of another grid: torch's size-mismatch error
    with pytest.raises(RuntimeError, match=r"size mismatch for positional_embedding.*\[65, 768\].*\[197, 768\]"):
        _build(_cfg(DR.config("r224"), res=224, denseclip_checkpoint=ck, **base))
    # a crop whose grid is not the tower's: the reference's tensor-size error
    with pytest.raises(RuntimeError, match=r"size of tensor a \(197\) must match the size of tensor b \(65\)"):
        _build(_cfg(DR.config("r128"), res=224, denseclip_checkpoint=ck, **base))
    # the bank of online_texts would need DenseCLIP's own text tower
    with pytest.raises(NotImplementedError, match="online_texts"):
        _build(_cfg(DR.config("r128"), denseclip_checkpoint=ck, support_memory_size=4, **base), online_texts=["a dog"])
    # a checkpoint file is read from disk
    p = tmp_path / "ck.pth"
    torch.save({"no_state_dict": 1}, str(p))
    with pytest.raises(ValueError, match="state_dict"):
        _build(_cfg(DR.config("r128", checkpoint_path=str(p)), **base))


def test_setup_attributes_equal_the_references(meta, tmp_path):
    from patchioner_amd.backbones import _denseclip_setup
    for tag in TAGS:
        res = DR.TOWERS[tag]["resolution"]
        p = tmp_path / (tag + ".pth")
        torch.save(DR.checkpoint(tag), str(p))
        cfg = DR.config(tag, checkpoint_path=str(p))
        s = _denseclip_setup(cfg, res, None, None)
        m = meta[tag]
        assert m["backbone_type"] == "DenseClip" and m["num_global_tokens"] == 1 and not m["has_blocks"] and m["num_attn_heads"] == 16
        assert (s.patch_size, s.embed_dim) == (m["patch_size"], m["embed_dim"]) == (16, 512)
        assert s.config["model"]["vision"] == m["vision"] and s.config == cfg and s.config is not cfg
        assert 1 + (res // s.patch_size) ** 2 == m["num_tokens"] == 1 + m["num_patch_tokens"]
        assert (s.width, s.depth, s.heads, s.token_dim, s.engine_kw["pretrain_grid"] * s.patch_size) == (768, 3, 12, 512, res)
        assert s.state_dict["pos_embed"].shape == (1, m["num_tokens"], 768)           # used at its own grid: nothing to resample
    # the reference's .get defaults: 16 and 512 (unreachable past DenseCLIPModel, which indexes the keys: its KeyError)
    cfg = DR.config("r128")
    del cfg["model"]["vision"]["embed_dim"]
    with pytest.raises(KeyError, match="embed_dim"):
        _denseclip_setup(cfg, 128, 3, None)


# ---- the loader ----------------------------------------------------------------------------------------------------------------
def test_loader_takes_only_the_tower_and_rounds_nothing():
    ck = DR.checkpoint("r128")
    sd = ck["state_dict"]
    assert any(k.startswith("backbone.fpn") for k in sd) and any(k.startswith("text_encoder.") for k in sd)
    assert any(k.startswith(("neck.", "decode_head.")) for k in sd)
    eng = W.denseclip_to_engine(ck, DR.vision("r128"))
    names = {"patch_embed.proj.weight": "conv1.weight", "head.weight": "proj", "cls_token": "class_embedding",
             "pos_embed": "positional_embedding", "norm_pre.weight": "ln_pre.weight", "norm_pre.bias": "ln_pre.bias",
             "norm.weight": "ln_post.weight", "norm.bias": "ln_post.bias"}
    for i in range(3):
        src, dst = "transformer.resblocks.%d." % i, "blocks.%d." % i
        for a, b in (("attn.in_proj_weight", "attn.qkv.weight"), ("attn.in_proj_bias", "attn.qkv.bias"), ("attn.out_proj.weight", "attn.proj.weight"),
                     ("attn.out_proj.bias", "attn.proj.bias"), ("mlp.c_fc.weight", "mlp.fc1.weight"), ("mlp.c_fc.bias", "mlp.fc1.bias"),
                     ("mlp.c_proj.weight", "mlp.fc2.weight"), ("mlp.c_proj.bias", "mlp.fc2.bias"), ("ln_1.weight", "norm1.weight"),
                     ("ln_1.bias", "norm1.bias"), ("ln_2.weight", "norm2.weight"), ("ln_2.bias", "norm2.bias")):
            names[dst + b] = src + a
    assert set(eng) == set(names)                                   # nothing of the FPN, the text tower, the neck or the heads
    assert sorted(names.values()) == sorted(W.denseclip_tower_keys(3))
    rounded = 0
    for k, s in names.items():
        want = sd["backbone." + s]
        want = want.t() if s == "proj" else want
        assert eng[k].dtype == torch.float32 and torch.equal(eng[k].reshape(want.shape), want), k      # the checkpoint's fp32 bits
        rounded += int(torch.equal(want, want.half().float()))
    assert rounded == 0                                             # and the synthetic values are not fp16-representable
    # more keys that are not the tower's change nothing
    more = dict(sd)
    more["backbone.fpn3.weight"] = torch.zeros(3)
    more["text_encoder.transformer.resblocks.0.ln_1.weight"] = torch.zeros(512)
    more["contexts"] = torch.zeros(1, 8, 512)
    eng2 = W.denseclip_to_engine({"state_dict": more}, DR.vision("r128"))
    assert set(eng2) == set(eng) and all(torch.equal(eng[k], eng2[k]) for k in eng)
    # the same seed gives the same bits, another resolution another table
    again = W.synth_denseclip_vit(DR.TOWERS["r128"]["seed_vit"], 128, 3)
    assert all(torch.equal(again["state_dict"][k], v) for k, v in sd.items())
    assert W.synth_denseclip_vit(1, 640, 1)["state_dict"]["backbone.positional_embedding"].shape == (1601, 768)


# ---- bank file names -----------------------------------------------------------------------------------------------------------
def test_bank_file_names_equal_the_references(meta):
    from patchioner_amd.bank import filename_components, memory_bank_filename
    for key, want in meta["bank_filenames"].items():
        name, t2d = key.split("|")
        got, dataset = memory_bank_filename("coco_captions", "ViT-B/16", 500000, use_talk2dino=bool(int(t2d)), denseclip_config=name)
        assert got == want and dataset == "coco_captions", (key, got)
    assert len(meta["bank_filenames"]) == 4
    assert filename_components("coco_captions", False, denseclip_config="/x/y/my_cfg.yaml")[::3] == ("denseclip-", "-denseclip-my_cfg")
    assert filename_components("coco_captions", False, denseclip_config="n", use_open_clip=True)[::3] == ("denseclip-", "-open_clip")
    # callers that do not pass it get the strings they got
    assert filename_components("coco_captions", False)[::3] == ("clip-", "")
    assert memory_bank_filename("coco_captions", None, 591753, True)[0] == "coco_captions_text_embeddings-B16-ViT-B.16-591753.h5"
    with pytest.raises(TypeError):
        filename_components("coco_captions", False, denseclip_config={"model": {}})
