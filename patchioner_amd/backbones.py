"""The vision tower of a ``Patchioner``, resolved once: which family the constructor's keywords select (route_backbone, in the
reference's own order) and everything the model and the engine derive from that family, as one record (Backbone) that the family's
setup function returns.  Nothing here touches a device.  A new tower is one more setup function and one more line of the routing
chain ("The backbone seam")."""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, replace
from functools import partial

import torch

from . import weights as W


@dataclass(frozen=True)
class Backbone:
    kind: str                                   # the reference's backbone_type (model.py:634-651); pipeline.py and dist.py compare it
    state_dict: dict                            # the tower's weights under the engine's names
    depth: int
    heads: int
    patch_size: int
    token_dim: int                              # width of the tokens the tower returns (the memory bank's and the decoder prefix's)
    embed_dim: int                              # the reference's public embed_dim: config- or name-derived, not always the tower's width
    width: int                                  # the tower's own width: the embed_dim the engine is built with
    engine_kw: dict                             # the family's part of the Engine(...) keywords, complete
    num_global_tokens: int = 1                  # the reference's count (cls + registers); num_tokens adds it to the patches
    grid_globals: int = 1                       # rows in front of the patch rows of the engine's tokens (Patchioner._G)
    readout_heads: int = 16                     # num_attn_heads: heads of the cls-attention read-out
    clip_stats: bool = True                     # the transforms normalise with the OpenAI-CLIP statistics, else ImageNet's
    transform_resolution: int | None = None     # resize AND crop of the cropping transform, whatever resize_dim / crop_dim say
    normalize_bank: bool = True                 # the memory bank is L2-normalised at load (normalize_memory_embs, model.py:174)
    has_attention: bool = False                 # model.py:864-865: only the DINO backbones install the qkv hook
    config: dict | None = None                  # the copy exposed as <kind>_config (regionclip_ / alphaclip_ / denseclip_config)


def _load_state_dict(spec):
    if spec is None:
        return None
    if isinstance(spec, dict):
        return spec
    if not os.path.exists(spec):
        raise FileNotFoundError("checkpoint %r not found (no HuggingFace / torch.hub download on this target)" % (spec,))
    sd = torch.load(spec, map_location="cpu")
    return sd.get("state_dict", sd) if isinstance(sd, dict) else sd


def _depth(sd) -> int:
    return 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))


def _vit_engine_kw(sd, width, arch, out_dim=0, registers=0, self_only=0, sparse_last_block=None, sparse_default=False) -> dict:
    # sparse_clip_tail: the CLIP-type towers' traces-only calls take the sparse tail (last block, ln_post, head) when asked, DenseCLIP's
    # by default (the engine itself keeps towers with self-only blocks, AlphaCLIP and the fp32 mode dense)
    return dict(embed_dim=width, num_registers=registers, pretrain_grid=int(math.isqrt(sd["pos_embed"].shape[1] - 1)), vit_arch=arch,
                vit_out_dim=out_dim, vit_ln_eps=1e-6 if arch == "dinov2" else 1e-5, vit_self_only_layers=self_only,
                sparse_clip_tail=sparse_default if sparse_last_block is None else bool(sparse_last_block))


def _regionclip_setup(rc: dict, dino_model, crop_dim: int, synthetic_seed, online_texts) -> Backbone:
    """RegionCLIP's ModifiedResNet (P/src/model.py:427-457; regionclip/loader.py:39-231): checks the config, loads the checkpoint
    (``checkpoint``: a RegionCLIP ``backbone.*`` checkpoint or a CLIP ``visual.*`` dict; else synthetic weights from
    synthetic_seed) and returns the engine's weights with the tower's sizes.  Everything is checked before the device is touched."""
    resnets = rc.get('MODEL', {}).get('RESNETS', {})
    out_features = resnets.get('OUT_FEATURES', ['res4'])          # build_model_with_defaults' default (loader.py:158)
    if 'res5' not in out_features:
        raise NotImplementedError("RegionCLIP with OUT_FEATURES %r: without 'res5' the reference returns layer3's stride-16 grid, which "
                                  "disagrees with its own num_patch_tokens (crop / 32)^2 (clip_backbone.py:278-299)" % (out_features,))
    if online_texts is not None:
        raise NotImplementedError("online_texts with RegionCLIP: the bank would come from RegionCLIP's own text tower, which this build "
                                  "does not implement; pass the bank as a file or tensor (memory_bank)")
    if rc.get('patch_size', 32) != 32:
        raise NotImplementedError("regionclip_config patch_size %r: the res5 grid is crop / 32, patch_size must be 32" % (rc['patch_size'],))
    if crop_dim % 32 != 0:
        raise ValueError("crop_dim must be a multiple of 32 for the RegionCLIP ResNet")
    sd = _load_state_dict(rc.get('checkpoint', None)) if rc.get('checkpoint', None) is not None else None
    res = resnets.get('IMAGE_RESOLUTION', None)
    if sd is None:
        if synthetic_seed is None:
            raise FileNotFoundError("regionclip_config['checkpoint'] is required (or synthetic_seed)")
        name = rc.get('name') or ("RN50x4" if "50x4" in (dino_model or "") or resnets.get('DEPTH') == 200 else "RN50")
        sd = W.synth_regionclip_rn(synthetic_seed + 1, name, image_resolution=res or 224)
    layers, width, grid, out_dim = W.regionclip_layers(sd)
    embed = 32 * width                        # attnpool width and heads as the reference derives them (clip_backbone.py:198-200, 705)
    if res is None:
        res = grid * 32
    s = res // 32
    pos = None
    if res / 32 != grid:
        # build_model_with_defaults (loader.py:200-210) drops the checkpoint's table; the tower keeps AttentionPool2d.__init__'s
        # unseeded draw randn(s^2 + 1, C) / sqrt(C) (clip_backbone.py:76).  Drawn here from torch's default CPU generator: the reference
        # draws it after the rest of the model's initialisation, so its own values cannot be replayed bit for bit
        print("Warning: Removing incompatible positional embedding from checkpoint.")
        print(f"  Checkpoint spatial size: {grid}x{grid} (for image resolution {grid * 32})")
        print(f"  Config image resolution: {res} (requires {res // 32}x{res // 32})")
        pos = torch.randn(s * s + 1, embed) / embed ** 0.5
    if s != crop_dim // 32:
        raise RuntimeError("The size of tensor a (%d) must match the size of tensor b (%d) at non-singleton dimension 0: the attnpool "
                           "table is built for IMAGE_RESOLUTION %d" % ((crop_dim // 32) ** 2 + 1, s * s + 1, res))
    # model.py:214-216, 254-263: patch_size and embed_dim come from the config; the tokens are the attnpool's output width.
    # num_global_tokens is 5, as the reference's `"reg" in dino_model` makes it for 'regionclip_*' names (model.py:198) -- read only by
    # the attention read-out, which this backbone never reaches; its tokens are 1 cls row + n^2 patches (grid_globals)
    return Backbone('RegionCLIP', W.regionclip_to_engine(sd, pos=pos), depth=sum(layers), heads=embed // 64, patch_size=32,
                    token_dim=out_dim, embed_dim=rc.get('embed_dim', 1024), width=embed, config=dict(rc),
                    num_global_tokens=5 if dino_model is not None and "reg" in dino_model else 1,
                    engine_kw=dict(embed_dim=embed, num_registers=0, pretrain_grid=crop_dim // 32, vit_arch="regionclip", vit_out_dim=out_dim,
                                   vit_ln_eps=1e-5, rn_layers=layers, rn_width=width,
                                   rn_attnpool_spatial=bool(rc.get('use_attnpool_for_spatial_feats', True))))


def _invite_setup(ic: dict, resize_dim: int, crop_dim: int, synthetic_seed, sparse_last_block=None) -> Backbone:
    """INViTE's CLIP ViT (P/src/model.py:217-229, 264-301, 459-485; INViTE/loader.py; clipfolder/clip.py:94-143, model.py:468-515):
    checks the config, loads the checkpoint (``checkpoint``: a local file or a state dict, the tower alone or a full CLIP dict; else
    synthetic weights from synthetic_seed) and returns the engine's weights with the tower's sizes, the name-derived attributes and
    the number of self-only blocks.  Everything is checked before the device is touched."""
    if 'name' not in ic:
        raise KeyError("'name' key is required in config dictionary")               # INViTE/loader.py:44-45
    name = ic['name']
    if ic.get('jit', False):
        raise NotImplementedError("invite_config jit: true loads a TorchScript archive, which has neither extract_last_k_th_token nor "
                                  "get_all_last; use jit: false")
    if str(name).startswith('RN'):
        raise NotImplementedError("invite_config name %r: INViTE's ModifiedResNet towers take no get_all_last argument "
                                  "(P/src/model.py:821 fails on them); only the ViT towers are implemented" % (name,))
    if ic.get('viz', False):
        # ResidualAttentionBlock asks for nn.MultiheadAttentionViz (clipfolder/model.py:178), which torch does not have
        raise AttributeError("module 'torch.nn' has no attribute 'MultiheadAttentionViz'")
    # patch_size and embed_dim come from the NAME (model.py:217-229, 291-301), with the reference's defaults for unknown names
    if 'ViT-B/32' in name:
        patch_size = 32
    elif 'ViT-B/16' in name:
        patch_size = 16
    elif 'ViT-L/14' in name:
        patch_size = 14
    else:
        print(f"Unknown INViTE model {name}, using default patch size 32")
        patch_size = 32
    if 'ViT-L' in name:
        embed_dim = 768
    elif 'ViT-B' in name:
        embed_dim = 512
    else:
        print(f"Unknown INViTE model {name}, using default embedding dimension 512")
        embed_dim = 512
    sd = _load_state_dict(ic.get('checkpoint', None))
    if sd is None:
        if synthetic_seed is None:
            raise FileNotFoundError("invite_config['checkpoint'] is required (a local CLIP checkpoint or state dict): clip.load(%r) "
                                    "would download the weights, which needs network this target does not have; or synthetic_seed"
                                    % (name,))
        sd = W.synth_invite_vit(synthetic_seed + 1, name)
    width, layers, heads, tower_patch, out_dim, grid = W.invite_dims(sd)
    if tower_patch != patch_size:
        raise ValueError("invite_config name %r gives patch_size %d, the checkpoint's conv1 is %d x %d: the reference would map boxes "
                         "and traces to a grid the tower does not have" % (name, patch_size, tower_patch, tower_patch))
    res = ic.get('resolution', None) or tower_patch * grid
    n = res // tower_patch
    if crop_dim // tower_patch != n or crop_dim % tower_patch != 0:
        # clipfolder/model.py:264: the position table is built for `resolution`; the add fails for any other crop
        raise RuntimeError("The size of tensor a (%d) must match the size of tensor b (%d) at non-singleton dimension 1: the %s tower "
                           "is built for %d x %d inputs (invite_config resolution)" % ((crop_dim // tower_patch) ** 2 + 1, n * n + 1,
                                                                                        name, res, res))
    k = int(ic.get('extract_last_k_th_token', -1))
    # the tower is the CLIP engine whose last blocks attend to themselves only (clipfolder/model.py:216-217: k >= layers masks every
    # block); its table arrives at the tower's own grid (weights.invite_to_engine), so the engine resamples nothing.  The tokens are
    # ln_post(x) @ proj wide.  model.py:463-473: clip._transform(input_resolution) resizes AND crops to the tower's resolution
    sd = W.invite_to_engine(sd, resolution=res)
    return Backbone('INViTE', sd, depth=_depth(sd), heads=heads, patch_size=patch_size, token_dim=out_dim, embed_dim=embed_dim,
                    width=width, transform_resolution=res,
                    engine_kw=_vit_engine_kw(sd, width, "clip", out_dim, self_only=0 if k <= 0 else min(k, layers),
                                             sparse_last_block=sparse_last_block))


_DENSECLIP_BLOCKED_NAMES = ("dinov2", "patch16", "patch14", "patch32", "openai")


def _denseclip_routed(dino_model, denseclip_config, regionclip_config=None, invite_config=None) -> bool:
    """Does the reference's constructor reach its DenseClip branches (P/src/model.py:200-235, 254-304, 338-513, 584-610)?  Only with a
    dino_model (:200, :338), one that none of the name tests in front of it takes ('dinov2', 'patch16', 'patch14', 'patch32' at :201-208,
    'dinov2' / 'openai' at :339-358), and with regionclip_config and invite_config both None (:214-217, :427, :459: both are tested
    first).  The YAML says 'INViTE_B16'.  A name that wins leaves denseclip_config unread."""
    return (denseclip_config is not None and dino_model is not None and regionclip_config is None and invite_config is None
            and not any(t in dino_model for t in _DENSECLIP_BLOCKED_NAMES))


def _denseclip_setup(dc, crop_dim: int, synthetic_seed, online_texts, config_dir=None, checkpoint=None, sparse_last_block=None) -> Backbone:
    """DenseCLIP's CLIP ViT (P/src/model.py:230-234, 277-283, 302-304, 487-513, 639-641; denseclip/loader.py:19-33;
    clip_loader/denseclip_loader.py:35-49, 196-227, 230-316): resolves the config (denseclip.resolve_config), loads the checkpoint and
    returns the engine's weights with the tower's sizes and the attributes the reference derives.  The checkpoint is, in this order:
    ``checkpoint`` (this build's override: a local file or a {'state_dict': ...} dict), the config's ``checkpoint.path`` (a dict-form
    config may put the {'state_dict': ...} dict itself under ``checkpoint``), synthetic weights from synthetic_seed when that path does
    not exist.  Everything is checked before the device is touched."""
    from . import denseclip as DC
    if online_texts is not None:
        raise NotImplementedError("online_texts with DenseCLIP: the bank would come from DenseCLIP's own text tower and tokenizer, which "
                                  "this build does not implement; pass the bank as a file or tensor (memory_bank)")
    cfg = DC.resolve_config(dc, config_dir)
    vis_cfg = (cfg.get('model') or {}).get('vision') or {}
    patch_size = vis_cfg.get('vision_patch_size', 16)                               # model.py:234, 513
    embed_dim = vis_cfg.get('embed_dim', 512)                                       # model.py:283, 304
    vision = DC.vision_block(cfg)                                                   # DenseCLIPModel.__init__ indexes all five
    res, tower_patch = vision["image_resolution"], vision["vision_patch_size"]
    n = res // tower_patch
    if crop_dim // tower_patch != n or crop_dim % tower_patch != 0:
        # clip_loader/models.py:147, 161: the position table is built for image_resolution; the add fails for any other crop
        raise RuntimeError("The size of tensor a (%d) must match the size of tensor b (%d) at non-singleton dimension 1: the DenseCLIP "
                           "tower is built for %d x %d inputs (denseclip_config model.vision.image_resolution)"
                           % ((crop_dim // tower_patch) ** 2 + 1, n * n + 1, res, res))
    ck = checkpoint
    explicit = ck is not None
    if ck is None:
        ck = cfg.get('checkpoint')
        if isinstance(ck, dict) and 'state_dict' not in ck and 'path' in ck:
            ck = ck['path']
        explicit = isinstance(ck, dict)
    if isinstance(ck, (str, os.PathLike)):
        if not os.path.exists(ck):
            if explicit or synthetic_seed is None:
                # the reference prints "Checkpoint not found ... using random weights" and captions with a random tower
                raise FileNotFoundError("DenseCLIP checkpoint %r not found: the reference would go on with RANDOM weights "
                                        "(denseclip_loader.py:281-282); give a local file or state dict (denseclip_checkpoint, or the "
                                        "config's checkpoint.path), or synthetic_seed" % (os.fspath(ck),))
            ck = W.synth_denseclip_vit(synthetic_seed + 1, res, vision["vision_layers"], vision["vision_width"], tower_patch,
                                       vision["embed_dim"])
        else:
            ck = torch.load(ck, map_location="cpu")
    elif ck is None:
        if synthetic_seed is None:
            raise FileNotFoundError("denseclip_config has no checkpoint.path and no denseclip_checkpoint was given (or synthetic_seed)")
        ck = W.synth_denseclip_vit(synthetic_seed + 1, res, vision["vision_layers"], vision["vision_width"], tower_patch,
                                   vision["embed_dim"])
    # the plain CLIP engine on fp32 checkpoint values, its table at its own grid; the tokens are ln_post(x) @ proj wide; config is the
    # dict copy of model.py:641
    sd = W.denseclip_to_engine(ck, vision)
    return Backbone('DenseClip', sd, depth=_depth(sd), heads=vision["vision_width"] // 64, patch_size=patch_size,
                    token_dim=vision["embed_dim"], embed_dim=embed_dim, width=vision["vision_width"], config=cfg,
                    engine_kw=_vit_engine_kw(sd, vision["vision_width"], "clip", vision["embed_dim"], sparse_last_block=sparse_last_block,
                                             sparse_default=True))


def _alphaclip_setup(ac: dict, crop_dim: int, synthetic_seed, sparse_last_block=None) -> Backbone:
    """AlphaCLIP's ViT, the OpenAI-CLIP tower with an alpha input channel (P/src/model.py:305-310, 515-545;
    alphaclip_loader.load_alphaclip).  Name, crop and weights are checked here, before anything touches the device."""
    name = ac.get('name', None)
    width, _, heads, patch, out_dim, crop = W.alphaclip_arch(name)
    if ac.get('patch_size', patch) != patch:
        raise ValueError("alphaclip_config patch_size %r: the %s tower's patches are %d pixels" % (ac['patch_size'], name, patch))
    if crop_dim != crop:
        # alpha_clip/model.py:372: the position table is never resampled, the add fails for any other crop
        raise RuntimeError("The size of tensor a (%d) must match the size of tensor b (%d) at non-singleton dimension 1: the %s "
                           "tower takes %d x %d crops" % ((crop_dim // patch) ** 2 + 1, (crop // patch) ** 2 + 1, name, crop, crop))
    sd = _load_state_dict(ac.get('alpha_vision_checkpoint', None))
    if sd is None:
        if synthetic_seed is None:
            raise FileNotFoundError("alphaclip_config['alpha_vision_checkpoint'] is required (alpha_clip.load downloads the CLIP "
                                    "weights, which needs network this target does not have), or synthetic_seed")
        sd = W.synth_alphaclip_vit(synthetic_seed + 1, name)
    sd = W.alphaclip_to_engine(sd)
    # the tower is `width` wide; the reference's embed_dim is alphaclip_config['embed_dim'] (model.py:305-310), the head's width
    return Backbone('AlphaClip', sd, depth=_depth(sd), heads=heads, patch_size=patch, token_dim=out_dim, embed_dim=ac.get('embed_dim', out_dim),
                    width=width, config=dict(ac), engine_kw=_vit_engine_kw(sd, width, "alphaclip", out_dim, sparse_last_block=sparse_last_block))


def _named_weights(dino_model, dino_weights, crop_dim, patch_size, synthetic_seed, synth) -> dict:
    if crop_dim % patch_size != 0:          # the config-routed towers hold their crop to their own grid
        raise ValueError("crop_dim must be a multiple of %d (the reference's reshape fails otherwise)" % patch_size)
    sd = _load_state_dict(dino_weights)
    if sd is None:
        if synthetic_seed is None:
            raise FileNotFoundError("dino_weights is required: torch.hub.load('facebookresearch/dinov2', ...) / "
                                    "timm.create_model(..., pretrained=True) need network, which this target does not have")
        sd = synth(synthetic_seed + 1, dino_model)
    return sd


def _timm_clip_setup(dino_model, dino_weights, crop_dim: int, synthetic_seed, sparse_last_block=None) -> Backbone:
    """The timm OpenAI-CLIP towers of the "DeCap original" configurations (P/src/model.py:358-392; configs/decap_B16*.k.yaml,
    decap_B32.k.yaml)."""
    # timm VisionTransformer with pre_norm, nn.LayerNorm (eps 1e-5), QuickGELU (model.py:363-371); the reference hands
    # img_size=resize_dim to timm, which resamples the checkpoint's position table for any size but 224 at load
    # (configs/decap_B16_resize.k.yaml: 592): pio_finalize_weights does the same from the table's own grid
    width, _, heads, patch_size, out_dim = W.clip_arch(dino_model)
    sd = _named_weights(dino_model, dino_weights, crop_dim, patch_size, synthetic_seed, W.synth_clip_vit)
    G = 5 if "reg" in dino_model else 1                         # model.py:198, 336: registers and read-out heads come from the NAME
    return Backbone('CLIP', sd, depth=_depth(sd), heads=heads, patch_size=patch_size, token_dim=out_dim, embed_dim=width, width=width,
                    num_global_tokens=G, grid_globals=G, readout_heads=6 if 'vits' in dino_model else 16,
                    engine_kw=_vit_engine_kw(sd, width, "clip", out_dim, registers=G - 1, sparse_last_block=sparse_last_block))


def _dinov2_setup(dino_model, dino_weights, attention_type, crop_dim: int, synthetic_seed, sparse_last_block=None) -> Backbone:
    """DINOv2 ViT-S/B/L-14, with or without registers (P/src/model.py:339-357, 569-582); ``attention_type`` other than 'qkv' re-orders
    the last block's fused q|k|v rows as the reference does."""
    D, _, heads = W.dino_arch(dino_model)
    sd = _named_weights(dino_model, dino_weights, crop_dim, 14, synthetic_seed, W.synth_dinov2)
    depth = _depth(sd)
    if attention_type != 'qkv':
        sd = dict(sd)
        wk, bk = "blocks.%d.attn.qkv.weight" % (depth - 1), "blocks.%d.attn.qkv.bias" % (depth - 1)
        ws = dict(zip("qkv", sd[wk].reshape(3, D, D)))
        bs = dict(zip("qkv", sd[bk].reshape(3, D)))
        sd[wk] = torch.cat([ws[x] for x in attention_type], dim=0)
        sd[bk] = torch.cat([bs[x] for x in attention_type], dim=0)
    G = 5 if "reg" in dino_model else 1                         # model.py:198, 336: registers and read-out heads come from the NAME
    return Backbone('DINO', sd, depth=depth, heads=heads, patch_size=14, token_dim=D, embed_dim=D, width=D, clip_stats=False,
                    normalize_bank=False, has_attention=True, num_global_tokens=G, grid_globals=G, readout_heads=6 if 'vits' in dino_model else 16,
                    engine_kw=_vit_engine_kw(sd, D, "dinov2", registers=G - 1, sparse_last_block=sparse_last_block))


def route_backbone(*, dino_model, regionclip_config, invite_config, denseclip_config, alphaclip_config, dino_weights, attention_type,
                   resize_dim, crop_dim, synthetic_seed, online_texts, denseclip_config_dir, denseclip_checkpoint,
                   sparse_last_block):
    """Decides the family, once, in the reference's order, and refuses what no family takes.  The four config-routed families are set
    up here, checkpoint included.  The two name-routed ones read ``dino_weights`` only when the returned callable is called: the
    constructor calls it after its head, projection and device refusals, so a construction that is wrong twice keeps raising what it
    always raised (tests/test_cabi_cpu.py: projection_type before the missing dino_weights).  The callable returns the record."""
    if denseclip_config is not None and (regionclip_config is not None or invite_config is not None):
        raise NotImplementedError("denseclip_config beside regionclip_config / invite_config: the reference tests those two first "
                                  "(P/src/model.py:214-230) and never reads the DenseCLIP config; give one backbone config")
    if regionclip_config is not None:                                   # model.py:214-216, 427: tested first
        bb = _regionclip_setup(regionclip_config, dino_model, crop_dim, synthetic_seed, online_texts)
    elif invite_config is not None:                                     # model.py:217, 459: second, before alphaclip_config
        bb = _invite_setup(invite_config, resize_dim, crop_dim, synthetic_seed, sparse_last_block)
    elif _denseclip_routed(dino_model, denseclip_config):               # model.py:230, 487: after those two, before alphaclip_config
        bb = _denseclip_setup(denseclip_config, crop_dim, synthetic_seed, online_texts, denseclip_config_dir, denseclip_checkpoint,
                              sparse_last_block)
    elif alphaclip_config is not None:                                  # model.py:515
        bb = _alphaclip_setup(alphaclip_config, crop_dim, synthetic_seed, sparse_last_block)
    else:
        # P/src/model.py:339-392: 'dinov2' names load from torch.hub, 'openai' names are the timm OpenAI-CLIP towers of the
        # "DeCap original" configurations
        is_clip = dino_model is not None and 'openai' in dino_model and 'dinov2' not in dino_model
        if dino_model is None or 'dinotxt' in dino_model or not ('dinov2' in dino_model or is_clip):
            raise ValueError("Unsupported backbone %r: this build implements the DINOv2 ViT-S/B/L-14 family and the timm "
                             "OpenAI-CLIP ViTs (vit_base_patch16/32_clip_224.openai)" % (dino_model,))
        if not is_clip:
            return partial(_dinov2_setup, dino_model, dino_weights, attention_type, crop_dim, synthetic_seed, sparse_last_block)
        if resize_dim != crop_dim:
            # P/src/model.py:371 builds the tower with img_size=resize_dim: timm's PatchEmbed then asserts that every input is
            # resize_dim x resize_dim, while the transforms crop to crop_dim -- the reference's first forward fails; fail at once
            raise AssertionError("Input height (%d) doesn't match model (%d)." % (crop_dim, resize_dim))
        return partial(_timm_clip_setup, dino_model, dino_weights, crop_dim, synthetic_seed, sparse_last_block)
    bb = replace(bb, normalize_bank=dino_model is None or 'dinov2' not in dino_model)
    return lambda: bb


def resolve_backbone(**keywords) -> Backbone:
    """The record for the constructor's backbone keywords (those of route_backbone), weights loaded."""
    return route_backbone(**keywords)()
