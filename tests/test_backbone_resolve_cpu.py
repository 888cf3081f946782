"""backbones.resolve_backbone against what the constructor derived, family by family, before the record existed: the complete Engine
keywords, the model's public attributes and the backbone's state dict (names, shapes, dtypes, SHA-256 over names and bytes) were
recorded from ``Patchioner.from_config`` with a recording stand-in for the Engine, and are kept in tests/golden/backbone_resolve.json.
The resolver touches no device, so nothing here needs one.

The synthetic weights of most towers are drawn with trunc_normal_, whose values differ in the last bits between CPU types, so a digest
recorded on one machine does not hold on another (INViTE's and DenseCLIP's do: the fixture marks them ``portable``).  For every case
WEIGHTS therefore gives the state dict from weights.py alone; when the fixture was recorded, what the constructor loaded was bitwise
equal to it, and here the resolver's must be.  The digest is asserted as well where it is portable."""
import hashlib
import json
import os

import pytest
import torch

from patchioner_amd import weights as W

torch.set_grad_enabled(False)
GOLD = os.path.join(os.path.dirname(__file__), "golden", "backbone_resolve.json")

# what Patchioner.from_config hands to the resolver, by config key
RESOLVER_KEYS = {"dino_model": None, "regionclip_config": None, "invite_config": None, "denseclip_config": None, "alphaclip_config": None,
                 "dino_weights": None, "attention_type": "qkv", "resize_dim": 518, "crop_dim": 518, "synthetic_seed": None,
                 "denseclip_config_dir": None, "denseclip_checkpoint": None, "sparse_last_block": None}
# the Engine keywords that are no family's: the record's own fields or the constructor's arguments
COMMON_ENGINE_KEYS = {"depth", "num_heads", "crop_dim", "patch_size", "prefix_size", "max_batch", "max_prefixes", "vit_dtype", "device_index",
                      "readout_heads", "readout_scale"}
CONFIG_ATTRS = ("regionclip_config", "alphaclip_config", "denseclip_config")


def _base(dino_model, prefix_size, res=224, **over):
    cfg = {"decap_weights": None, "prefix_size": prefix_size, "support_memory_size": 0, "dino_model": dino_model, "normalize": False,
           "resize_dim": res, "crop_dim": res, "use_talk2dino_project": False, "synthetic_seed": 3}
    cfg.update(over)
    return cfg


def _invite(**over):
    return _base("INViTE_B16", 512, clip_model_name="ViT-B/32", invite_config={"name": "ViT-B/32", "extract_last_k_th_token": 2}, **over)


def _regionclip():
    rc = {"patch_size": 32, "MODEL": {"RESNETS": {"OUT_FEATURES": ["res4", "res5"], "IMAGE_RESOLUTION": 224}},
          "checkpoint": W.synth_regionclip_rn(1, "RN50", layers=(1, 1, 1, 1))}
    return _base("regionclip_resnet50_p32.k", 1024, regionclip_config=rc, invite_config={"name": "ViT-B/32", "extract_last_k_th_token": 2})


def _denseclip(**over):
    import denseclip_ref as DR
    return _base("INViTE_B16", 512, res=128, clip_model_name="ViT-B/16", denseclip_config=DR.config("r128"), **over)


ALPHA = {"patch_size": 16, "name": "ViT-B/16", "use_cls_for_localized_captions": True, "embed_dim": 512}
CLIP32 = "vit_base_patch32_clip_224.openai"
def _dinov2(name, order="qkv"):
    sd = dict(W.synth_dinov2(4, name))
    for k in ("blocks.11.attn.qkv.weight", "blocks.11.attn.qkv.bias"):            # the last block's q | k | v row blocks, re-ordered
        sd[k] = torch.cat([sd[k].chunk(3, 0)["qkv".index(c)] for c in order], 0)
    return sd


def _denseclip_weights():
    import denseclip_ref as DR
    return W.denseclip_to_engine(W.synth_denseclip_vit(4, 128, 3, 768, 16, 512), DR.vision("r128"))


# the state dict of each case, from weights.py alone: synthetic_seed + 1 = 4 seeds the tower
WEIGHTS = {
    "dinov2_vits14_reg": lambda cfg: _dinov2("dinov2_vits14_reg"),
    "dinov2_vits14_vkq": lambda cfg: _dinov2("dinov2_vits14", "vkq"),
    "timm_clip_b32": lambda cfg: W.synth_clip_vit(4, CLIP32),
    "timm_clip_b32_sparse": lambda cfg: W.synth_clip_vit(4, CLIP32),
    "timm_clip_b32_dense": lambda cfg: W.synth_clip_vit(4, CLIP32),
    "alphaclip_b16": lambda cfg: W.alphaclip_to_engine(W.synth_alphaclip_vit(4, "ViT-B/16")),
    "invite_b32": lambda cfg: W.invite_to_engine(W.synth_invite_vit(4, "ViT-B/32"), resolution=224),
    "invite_b32_beside_alphaclip": lambda cfg: W.invite_to_engine(W.synth_invite_vit(4, "ViT-B/32"), resolution=224),
    "regionclip_beside_invite": lambda cfg: W.regionclip_to_engine(cfg["regionclip_config"]["checkpoint"]),
    "denseclip_r128": lambda cfg: _denseclip_weights(),
    "denseclip_r128_dense": lambda cfg: _denseclip_weights(),
    "dinov2_name_beside_denseclip": lambda cfg: _dinov2("dinov2_vits14"),
}
CASES = {
    "dinov2_vits14_reg": lambda: _base("dinov2_vits14_reg", 384),
    "dinov2_vits14_vkq": lambda: _base("dinov2_vits14", 384, attention_type="vkq"),
    "timm_clip_b32": lambda: _base(CLIP32, 512),
    "timm_clip_b32_sparse": lambda: _base(CLIP32, 512, sparse_last_block=True),
    "timm_clip_b32_dense": lambda: _base(CLIP32, 512, sparse_last_block=False),
    "alphaclip_b16": lambda: _base("AlphaClip", 512, clip_model_name="ViT-B/16", alphaclip_config=dict(ALPHA)),
    "invite_b32": _invite,
    "invite_b32_beside_alphaclip": lambda: _invite(alphaclip_config=dict(ALPHA)),
    "regionclip_beside_invite": _regionclip,
    "denseclip_r128": _denseclip,
    "denseclip_r128_dense": lambda: _denseclip(sparse_last_block=False),
    "dinov2_name_beside_denseclip": lambda: _base("dinov2_vits14", 384, denseclip_config={"not": "read"}),
}


def state_dict_summary(sd):
    h = hashlib.sha256()
    tensors = []
    for k in sorted(sd):
        t = sd[k].detach().contiguous()
        h.update(k.encode())
        h.update(t.numpy().tobytes())
        tensors.append([k, list(t.shape), str(t.dtype)])
    return {"tensors": tensors, "sha256": h.hexdigest()}


def transform_summary(crop, no_crop):
    return {"crop": [crop.resize_dim, crop.crop_dim, crop.mean.ravel().tolist(), crop.std.ravel().tolist()],
            "no_crop": [no_crop.resize_dim, no_crop.mean.ravel().tolist(), no_crop.std.ravel().tolist()]}


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


def test_every_case_is_recorded(gold):
    assert set(gold) == set(CASES) == set(WEIGHTS)
    assert {g["attrs"]["backbone_type"] for g in gold.values()} == {"DINO", "CLIP", "AlphaClip", "INViTE", "DenseClip", "RegionCLIP"}


@pytest.mark.parametrize("name", list(CASES))
def test_resolver_gives_what_the_constructor_derived(gold, name):
    from patchioner_amd.backbones import resolve_backbone
    from patchioner_amd.preprocess import CLIP_MEAN, CLIP_STD, make_transforms
    cfg, g = CASES[name](), gold[name]
    bb = resolve_backbone(online_texts=None, **{k: cfg.get(k, d) for k, d in RESOLVER_KEYS.items()})
    a, ekw = g["attrs"], g["engine_kw"]

    # the family part of the Engine keywords, complete: with the family-independent ones they are exactly what the Engine got
    assert set(bb.engine_kw).isdisjoint(COMMON_ENGINE_KEYS) and set(bb.engine_kw) | COMMON_ENGINE_KEYS == set(ekw)
    assert json.loads(json.dumps(bb.engine_kw)) == {k: ekw[k] for k in bb.engine_kw}
    assert (bb.depth, bb.heads, bb.patch_size, bb.readout_heads) == (ekw["depth"], ekw["num_heads"], ekw["patch_size"], ekw["readout_heads"])
    assert bb.width == ekw["embed_dim"]

    # the public attributes
    assert (bb.kind, bb.num_global_tokens, bb.grid_globals, bb.token_dim, bb.embed_dim, bb.patch_size, bb.readout_heads) == \
        (a["backbone_type"], a["num_global_tokens"], a["_G"], a["token_dim"], a["embed_dim"], a["patch_size"], a["num_attn_heads"])
    n2 = (cfg["crop_dim"] // bb.patch_size) ** 2
    assert (n2, bb.num_global_tokens + n2) == (a["num_patch_tokens"], a["num_tokens"])
    assert a["model_name"] == cfg["dino_model"] and a["scale"] == 0.125
    assert bb.has_attention == ("DINO" in a["backbone_type"])
    assert bb.normalize_bank == ("dinov2" not in cfg["dino_model"])
    given = [k for k in CONFIG_ATTRS if bb.config is not None and bb.kind.lower() + "_config" == k]
    assert given == g["config_attrs"]
    if given:
        assert bb.config == cfg[given[0]] and bb.config is not cfg[given[0]]

    # the transforms the constructor builds from the record
    res = bb.transform_resolution
    stats = (CLIP_MEAN, CLIP_STD) if bb.clip_stats else (None, None)
    crop, no_crop = make_transforms(cfg["resize_dim"], cfg["crop_dim"], *stats)
    if res is not None:
        crop = make_transforms(res, res, *stats)[0]
    assert transform_summary(crop, no_crop) == g["transforms"]

    # the weights: names, shapes, dtypes and every byte
    s = state_dict_summary(bb.state_dict)
    assert s["tensors"] == g["state_dict"]["tensors"]
    want = WEIGHTS[name](cfg)
    assert g["state_dict"]["equal_to_WEIGHTS"] and set(want) == set(bb.state_dict)
    assert all(torch.equal(want[k], v) for k, v in bb.state_dict.items())
    if g["state_dict"]["portable"]:
        assert s["sha256"] == g["state_dict"]["sha256"]
