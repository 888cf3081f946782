"""Seeded synthetic weights in the reference checkpoints' own key names.

There is no network on the build or GPU boxes, so the DINOv2 hub weights
(P/src/model.py:342-343), the DeCap decoder checkpoint (P/src/decap/decap.py:188-222) and the
text memory bank (P/src/decap/im2txtprojection/im2txtprojection.py:387-407) are replaced by
deterministic synthetic tensors of the same shapes and names.  Real checkpoints
load through the same dict interface (see ``model.Patchioner.from_config``).

All generators use a CPU ``torch.Generator`` so the numbers are identical on every box.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

DINO_ARCHS = {
    # name fragment -> (embed_dim, depth, heads)
    "vits14": (384, 12, 6),
    "vitb14": (768, 12, 12),
    "vitl14": (1024, 24, 16),
}


def dino_arch(dino_model: str):
    for k, v in DINO_ARCHS.items():
        if k in dino_model:
            return v
    raise ValueError("unsupported DINOv2 model name %r" % (dino_model,))


def _tn(g, shape, std):
    t = torch.empty(shape)
    torch.nn.init.trunc_normal_(t, std=std, a=-2 * std, b=2 * std, generator=g)
    return t


def synth_dinov2(seed: int, dino_model: str = "dinov2_vitb14_reg", depth: int | None = None,
                 pretrain_grid: int = 37) -> Dict[str, torch.Tensor]:
    """State dict shaped like ``torch.hub.load('facebookresearch/dinov2', dino_model).state_dict()``."""
    D, full_depth, _ = dino_arch(dino_model)
    depth = depth or full_depth
    R = 4 if "reg" in dino_model else 0
    g = torch.Generator().manual_seed(seed)
    w: Dict[str, torch.Tensor] = {}
    w["cls_token"] = _tn(g, (1, 1, D), 0.02)
    w["pos_embed"] = _tn(g, (1, 1 + pretrain_grid * pretrain_grid, D), 0.02)
    if R:
        w["register_tokens"] = _tn(g, (1, R, D), 0.02)
    w["mask_token"] = torch.zeros(1, D)
    w["patch_embed.proj.weight"] = _tn(g, (D, 3, 14, 14), 0.02)
    w["patch_embed.proj.bias"] = _tn(g, (D,), 0.02)
    for i in range(depth):
        p = "blocks.%d." % i
        for ln in ("norm1", "norm2"):
            w[p + ln + ".weight"] = 0.5 + torch.rand(D, generator=g)
            w[p + ln + ".bias"] = _tn(g, (D,), 0.02)
        # q/k rows scaled up so the attention maps are peaky (as trained DINOv2 maps are)
        qkv = _tn(g, (3 * D, D), 0.02)
        qkv[: 2 * D] *= 2.5
        w[p + "attn.qkv.weight"] = qkv
        w[p + "attn.qkv.bias"] = _tn(g, (3 * D,), 0.02)
        w[p + "attn.proj.weight"] = _tn(g, (D, D), 0.02)
        w[p + "attn.proj.bias"] = _tn(g, (D,), 0.02)
        w[p + "ls1.gamma"] = 0.1 * (0.5 + torch.rand(D, generator=g))
        w[p + "mlp.fc1.weight"] = _tn(g, (4 * D, D), 0.02)
        w[p + "mlp.fc1.bias"] = _tn(g, (4 * D,), 0.02)
        w[p + "mlp.fc2.weight"] = _tn(g, (D, 4 * D), 0.02)
        w[p + "mlp.fc2.bias"] = _tn(g, (D,), 0.02)
        w[p + "ls2.gamma"] = 0.1 * (0.5 + torch.rand(D, generator=g))
    w["norm.weight"] = 0.5 + torch.rand(D, generator=g)
    w["norm.bias"] = _tn(g, (D,), 0.02)
    return w


CLIP_ARCHS = {
    # timm model name fragment -> (embed_dim, depth, heads, patch, head width)
    "vit_base_patch16_clip_224": (768, 12, 12, 16, 512),
    "vit_base_patch32_clip_224": (768, 12, 12, 32, 512),
    "vit_large_patch14_clip_224": (1024, 24, 16, 14, 768),
}


def clip_arch(name: str):
    for k, v in CLIP_ARCHS.items():
        if k in name:
            return v
    raise ValueError("unsupported OpenAI-CLIP timm model name %r" % (name,))


def synth_clip_vit(seed: int, name: str = "vit_base_patch16_clip_224.openai", depth: int | None = None,
                   img: int = 224) -> Dict[str, torch.Tensor]:
    """State dict shaped like ``timm.create_model(name, act_layer=QuickGELU).state_dict()`` (P/src/model.py:371): the OpenAI
    CLIP vision tower in timm's VisionTransformer layout -- bias-free patch conv, cls token, learned positions for
    [cls | patches], norm_pre, pre-LN blocks without LayerScale, final norm, bias-free head to the joint space."""
    D, full_depth, _, p, out = clip_arch(name)
    depth = depth or full_depth
    n = img // p
    g = torch.Generator().manual_seed(seed)
    w: Dict[str, torch.Tensor] = {}
    w["cls_token"] = _tn(g, (1, 1, D), 0.02)
    w["pos_embed"] = _tn(g, (1, 1 + n * n, D), 0.02)
    w["patch_embed.proj.weight"] = _tn(g, (D, 3, p, p), 0.02)
    w["norm_pre.weight"] = 0.5 + torch.rand(D, generator=g)
    w["norm_pre.bias"] = _tn(g, (D,), 0.02)
    for i in range(depth):
        q = "blocks.%d." % i
        for ln in ("norm1", "norm2"):
            w[q + ln + ".weight"] = 0.5 + torch.rand(D, generator=g)
            w[q + ln + ".bias"] = _tn(g, (D,), 0.02)
        qkv = _tn(g, (3 * D, D), 0.02)
        qkv[: 2 * D] *= 2.5
        w[q + "attn.qkv.weight"] = qkv
        w[q + "attn.qkv.bias"] = _tn(g, (3 * D,), 0.02)
        w[q + "attn.proj.weight"] = _tn(g, (D, D), 0.02) * 0.3        # no LayerScale: small branch outputs keep the stream tame
        w[q + "attn.proj.bias"] = _tn(g, (D,), 0.02)
        w[q + "mlp.fc1.weight"] = _tn(g, (4 * D, D), 0.02)
        w[q + "mlp.fc1.bias"] = _tn(g, (4 * D,), 0.02)
        w[q + "mlp.fc2.weight"] = _tn(g, (D, 4 * D), 0.02) * 0.3
        w[q + "mlp.fc2.bias"] = _tn(g, (D,), 0.02)
    w["norm.weight"] = 0.5 + torch.rand(D, generator=g)
    w["norm.bias"] = _tn(g, (D,), 0.02)
    w["head.weight"] = _tn(g, (out, D), 0.03)
    return w


ALPHACLIP_ARCHS = {
    # alphaclip_config['name'] (alpha_clip.load names) -> the timm-named OpenAI-CLIP tower of the same shape (CLIP_ARCHS), native crop
    "ViT-B/16": ("vit_base_patch16_clip_224", 224),
    "ViT-B/32": ("vit_base_patch32_clip_224", 224),
    "ViT-L/14": ("vit_large_patch14_clip_224", 224),
}


def alphaclip_arch(name: str):
    """-> (embed_dim, depth, heads, patch, head width, native crop) of an AlphaCLIP tower name.  Unknown names raise RuntimeError like
    alpha_clip.load (alpha_clip.py: "Model ... not found")."""
    if name not in ALPHACLIP_ARCHS:
        raise RuntimeError("Model %s not found; available models = %s" % (name, list(ALPHACLIP_ARCHS)))
    timm_name, crop = ALPHACLIP_ARCHS[name]
    return clip_arch(timm_name) + (crop,)


def synth_alphaclip_vit(seed: int, name: str = "ViT-B/16", depth: int | None = None) -> Dict[str, torch.Tensor]:
    """State dict shaped like AlphaCLIP's ``model.visual.state_dict()`` (P/src/alphaclip/alpha_clip/model.py:336-349, the OpenAI
    layout with ``attn.in_proj.weight`` as alpha_clip.build_model renames it): conv1 and a NON-ZERO conv1_alpha (trained checkpoints
    start from zeros and learn it; zeros would hide the alpha path from every test), class_embedding, positional_embedding, ln_pre,
    transformer.resblocks.{i}.{ln_1, attn.in_proj, attn.out_proj, ln_2, mlp.c_fc, mlp.c_proj}, ln_post, proj [width, output_dim]."""
    D, full_depth, _, p, out, crop = alphaclip_arch(name)
    depth = depth or full_depth
    n = crop // p
    g = torch.Generator().manual_seed(seed)
    w: Dict[str, torch.Tensor] = {}
    w["conv1.weight"] = _tn(g, (D, 3, p, p), 0.02)
    w["conv1_alpha.weight"] = _tn(g, (D, 1, p, p), 0.05)
    w["class_embedding"] = _tn(g, (D,), 0.02)
    w["positional_embedding"] = _tn(g, (1 + n * n, D), 0.02)
    w["ln_pre.weight"] = 0.5 + torch.rand(D, generator=g)
    w["ln_pre.bias"] = _tn(g, (D,), 0.02)
    for i in range(depth):
        q = "transformer.resblocks.%d." % i
        for ln in ("ln_1", "ln_2"):
            w[q + ln + ".weight"] = 0.5 + torch.rand(D, generator=g)
            w[q + ln + ".bias"] = _tn(g, (D,), 0.02)
        qkv = _tn(g, (3 * D, D), 0.02)
        qkv[: 2 * D] *= 2.5
        w[q + "attn.in_proj.weight"] = qkv
        w[q + "attn.in_proj.bias"] = _tn(g, (3 * D,), 0.02)
        w[q + "attn.out_proj.weight"] = _tn(g, (D, D), 0.02) * 0.3
        w[q + "attn.out_proj.bias"] = _tn(g, (D,), 0.02)
        w[q + "mlp.c_fc.weight"] = _tn(g, (4 * D, D), 0.02)
        w[q + "mlp.c_fc.bias"] = _tn(g, (4 * D,), 0.02)
        w[q + "mlp.c_proj.weight"] = _tn(g, (D, 4 * D), 0.02) * 0.3
        w[q + "mlp.c_proj.bias"] = _tn(g, (D,), 0.02)
    w["ln_post.weight"] = 0.5 + torch.rand(D, generator=g)
    w["ln_post.bias"] = _tn(g, (D,), 0.02)
    w["proj"] = _tn(g, (D, out), 0.03)
    return w


_ALPHACLIP_BLOCK_KEYS = {"ln_1": "norm1", "ln_2": "norm2", "attn.in_proj": "attn.qkv", "attn.out_proj": "attn.proj",
                         "mlp.c_fc": "mlp.fc1", "mlp.c_proj": "mlp.fc2"}


def alphaclip_to_engine(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """AlphaCLIP visual state dict (OpenAI layout; ``attn.in_proj.weight`` or the checkpoint's own ``attn.in_proj_weight``; an optional
    ``visual.`` prefix) -> the engine's keys: the timm names of the CLIP tower (cls_token, pos_embed, patch_embed.proj.weight, norm_pre,
    blocks.{i}.*, norm, head.weight = proj^T) plus ``patch_embed.alpha.weight`` for conv1_alpha (zeros when the checkpoint has none,
    alpha_clip/model.py:603-606)."""
    out = _openai_visual_to_engine({(k[len("visual."):] if k.startswith("visual.") else k): v for k, v in sd.items()})
    if "patch_embed.alpha.weight" not in out:
        pw = out["patch_embed.proj.weight"]
        out["patch_embed.alpha.weight"] = torch.zeros(pw.shape[0], 1, pw.shape[2], pw.shape[3], dtype=pw.dtype)
    return out


def _openai_visual_to_engine(src: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The keys of an OpenAI-layout ``VisionTransformer`` state dict (no ``visual.`` prefix) under the engine's timm names."""
    out: Dict[str, torch.Tensor] = {}
    for k, v in src.items():
        k = k.replace("in_proj_weight", "in_proj.weight").replace("in_proj_bias", "in_proj.bias")
        if k.startswith("transformer.resblocks."):
            i, rest = k[len("transformer.resblocks."):].split(".", 1)
            mod, leaf = rest.rsplit(".", 1)
            if mod not in _ALPHACLIP_BLOCK_KEYS:
                raise KeyError("unexpected AlphaCLIP block key %r" % k)
            out["blocks.%s.%s.%s" % (i, _ALPHACLIP_BLOCK_KEYS[mod], leaf)] = v
        elif k == "conv1.weight":
            out["patch_embed.proj.weight"] = v
        elif k == "conv1_alpha.weight":
            out["patch_embed.alpha.weight"] = v
        elif k == "class_embedding":
            out["cls_token"] = v.reshape(1, 1, -1)
        elif k == "positional_embedding":
            out["pos_embed"] = v.reshape(1, v.shape[0], v.shape[1])
        elif k in ("ln_pre.weight", "ln_pre.bias"):
            out["norm_pre." + k.split(".")[1]] = v
        elif k in ("ln_post.weight", "ln_post.bias"):
            out["norm." + k.split(".")[1]] = v
        elif k == "proj":
            out["head.weight"] = v.t().contiguous()
        else:
            raise KeyError("unexpected AlphaCLIP visual key %r" % k)
    return out


INVITE_ARCHS = dict(ALPHACLIP_ARCHS, **{"ViT-L/14@336px": ("vit_large_patch14_clip_224", 336)})


def invite_arch(name: str):
    """-> (width, layers, heads, patch, output dim, native resolution) of an INViTE tower name (the ViT names of clip.available_models(),
    P/src/INViTE/clipfolder/clip.py:30-40).  Unknown names raise RuntimeError like clip.load (:125)."""
    if name not in INVITE_ARCHS:
        raise RuntimeError("Model %s not found; available models = %s" % (name, list(INVITE_ARCHS)))
    timm_name, res = INVITE_ARCHS[name]
    return clip_arch(timm_name) + (res,)


def _cn(g, shape, std):
    """Clamped normal: the generator's own randn, then clamp and scale, which are exact IEEE operations -- the same bits on every host.
    (_tn's trunc_normal_ goes through a vectorised erfinv whose last bit differs between CPUs: after a loader that rounds weights to
    fp16, such a bit moves a tower's fp32 tokens by 1e-5.)"""
    return torch.randn(shape, generator=g).clamp_(-2.0, 2.0) * std


def synth_invite_vit(seed: int, name: str = "ViT-B/16", depth: int | None = None) -> Dict[str, torch.Tensor]:
    """State dict of the visual tower of an OpenAI CLIP checkpoint, ``visual.`` prefix stripped, as INViTE's build_model reads it
    (P/src/INViTE/clipfolder/model.py:240-257, 468-515): conv1.weight, class_embedding, positional_embedding, ln_pre,
    transformer.resblocks.{i}.{ln_1, attn.in_proj_weight, attn.in_proj_bias, attn.out_proj, ln_2, mlp.c_fc, mlp.c_proj}, ln_post,
    proj [width, output_dim].  fp32 values that are NOT fp16-representable: the loader's rounding (invite_to_engine) is visible.
    Drawn with _cn, so that the checkpoint is the same bits on every host (a fixture of the reference's fp32 tokens is held to 1e-5)."""
    D, full_depth, _, p, out, res = invite_arch(name)
    return synth_invite_tower(seed, D, depth or full_depth, p, out, res // p)


def synth_invite_tower(seed: int, D: int, depth: int, p: int, out: int, n: int) -> Dict[str, torch.Tensor]:
    """synth_invite_vit's draws for a tower given by its sizes: width D, ``depth`` blocks, patch p, output dim ``out``, grid n."""
    g = torch.Generator().manual_seed(seed)
    w: Dict[str, torch.Tensor] = {}
    w["conv1.weight"] = _cn(g, (D, 3, p, p), 0.02)
    w["class_embedding"] = _cn(g, (D,), 0.02)
    w["positional_embedding"] = _cn(g, (1 + n * n, D), 0.02)
    w["ln_pre.weight"] = 0.5 + torch.rand(D, generator=g)
    w["ln_pre.bias"] = _cn(g, (D,), 0.02)
    for i in range(depth):
        q = "transformer.resblocks.%d." % i
        for ln in ("ln_1", "ln_2"):
            w[q + ln + ".weight"] = 0.5 + torch.rand(D, generator=g)
            w[q + ln + ".bias"] = _cn(g, (D,), 0.02)
        qkv = _cn(g, (3 * D, D), 0.02)
        qkv[: 2 * D] *= 2.5
        w[q + "attn.in_proj_weight"] = qkv
        w[q + "attn.in_proj_bias"] = _cn(g, (3 * D,), 0.02)
        w[q + "attn.out_proj.weight"] = _cn(g, (D, D), 0.02) * 0.3
        w[q + "attn.out_proj.bias"] = _cn(g, (D,), 0.02)
        w[q + "mlp.c_fc.weight"] = _cn(g, (4 * D, D), 0.02)
        w[q + "mlp.c_fc.bias"] = _cn(g, (4 * D,), 0.02)
        w[q + "mlp.c_proj.weight"] = _cn(g, (D, 4 * D), 0.02) * 0.3
        w[q + "mlp.c_proj.bias"] = _cn(g, (D,), 0.02)
    w["ln_post.weight"] = 0.5 + torch.rand(D, generator=g)
    w["ln_post.bias"] = _cn(g, (D,), 0.02)
    w["proj"] = _cn(g, (D, out), 0.03)
    return w


def invite_visual(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The visual tower of ``sd``: the ``visual.*`` keys of a full CLIP state dict (text tower beside them) without the prefix, or
    ``sd`` itself when it is the tower alone.  ResNet towers (``visual.layer1...``, no ``proj``) raise NotImplementedError."""
    vis = {k[len("visual."):]: v for k, v in sd.items() if k.startswith("visual.")} or dict(sd)
    if "proj" not in vis:
        raise NotImplementedError("INViTE with a ModifiedResNet tower (no visual.proj in the checkpoint): only the ViT towers carry "
                                  "extract_last_k_th_token (P/src/INViTE/clipfolder/model.py:536-546)")
    return vis


def invite_dims(sd: Dict[str, torch.Tensor]):
    """-> (width, layers, heads, patch, output dim, grid of the position table) read from the checkpoint's shapes, as build_model does
    (P/src/INViTE/clipfolder/model.py:471-477, 536: heads = width // 64)."""
    vis = invite_visual(sd)
    width, patch = int(vis["conv1.weight"].shape[0]), int(vis["conv1.weight"].shape[-1])
    layers = len([k for k in vis if k.endswith(".attn.in_proj_weight") or k.endswith(".attn.in_proj.weight")])
    grid = round((vis["positional_embedding"].shape[0] - 1) ** 0.5)
    return width, layers, width // 64, patch, int(vis["proj"].shape[1]), grid


def invite_resize_pos_embed(pe: torch.Tensor, grid: int) -> torch.Tensor:
    """resize_pos_embed (P/src/INViTE/clipfolder/model.py:454-466): the class row kept apart, the grid through
    F.interpolate(mode='bicubic', align_corners=False) WITHOUT antialias -- not timm's resampler, which the engine applies to a table
    of another grid (antialias=True).  [1 + g^2, C] -> [1 + grid^2, C], in the table's own dtype."""
    import torch.nn.functional as F
    g = int((pe.shape[0] - 1) ** 0.5)
    patch = pe[1:].reshape(1, g, g, -1).permute(0, 3, 1, 2)
    patch = F.interpolate(patch, size=(grid, grid), mode="bicubic", align_corners=False)
    return torch.cat([pe[:1], patch.permute(0, 2, 3, 1).reshape(grid * grid, -1)], dim=0)


_INVITE_FP16 = ("conv1.weight", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
                "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")


def invite_to_engine(sd: Dict[str, torch.Tensor], resolution: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """INViTE's loader (build_model, P/src/INViTE/clipfolder/model.py:468-515) -> the engine's CLIP keys (``vit_arch = 1``):

    * convert_weights (:425-449) makes the Conv2d / Linear / MultiheadAttention weights and biases and ``proj`` fp16 parameters, so
      load_state_dict rounds exactly those tensors to fp16 VALUES; class_embedding, positional_embedding and the LayerNorms stay fp32;
    * with ``resolution`` of another grid than the checkpoint's, the position table is resampled by resize_pos_embed (:454-466,
      510-512).  Done here, so that the engine gets a table at its own grid (pretrain_grid = the new grid) and its timm-style
      resampler stays out of it.

    Accepts the tower alone or a full CLIP state dict (``visual.`` prefix beside the text tower's keys)."""
    vis = invite_visual(sd)
    _, _, _, patch, _, grid = invite_dims(vis)
    src: Dict[str, torch.Tensor] = {}
    for k, v in vis.items():
        v = v.detach()
        if k == "proj" or k.endswith(_INVITE_FP16):
            v = v.half()
        src[k] = v.float()
    if resolution is not None and resolution // patch != grid:
        src["positional_embedding"] = invite_resize_pos_embed(vis["positional_embedding"].detach(), resolution // patch).float()
    return _openai_visual_to_engine(src)


def denseclip_tower_keys(layers: int):
    """The parameter names of DenseCLIP's CLIPVisionTransformer with ``layers`` blocks (P/src/denseclip/clip_loader/models.py:138-154)."""
    keys = ["conv1.weight", "class_embedding", "positional_embedding", "ln_pre.weight", "ln_pre.bias", "ln_post.weight", "ln_post.bias", "proj"]
    for i in range(layers):
        q = "transformer.resblocks.%d." % i
        keys += [q + k for k in ("ln_1.weight", "ln_1.bias", "ln_2.weight", "ln_2.bias", "attn.in_proj_weight", "attn.in_proj_bias",
                                 "attn.out_proj.weight", "attn.out_proj.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight",
                                 "mlp.c_proj.bias")]
    return keys


def synth_denseclip_vit(seed: int, resolution: int = 640, depth: int | None = None, width: int = 768, patch: int = 16,
                        embed_dim: int = 512) -> Dict[str, object]:
    """A DenseCLIP segmentation checkpoint as load_denseclip_weights reads it (P/src/denseclip/clip_loader/denseclip_loader.py:196-227):
    ``{'state_dict': {...}}`` with the visual tower under ``backbone.`` (OpenAI's names, the position table at ``resolution``'s grid),
    beside what the loader must ignore: FPN layers under ``backbone.fpn*``, a ``text_encoder.`` tensor, neck and decode-head tensors.
    fp32 values that are not fp16-representable (the loader rounds nothing); drawn with _cn, the same bits on every host."""
    depth = depth or 12
    tower = synth_invite_tower(seed, width, depth, patch, embed_dim, resolution // patch)
    g = torch.Generator().manual_seed(seed + 7919)
    sd: Dict[str, torch.Tensor] = {"backbone." + k: v for k, v in tower.items()}
    sd["backbone.fpn1.0.weight"] = _cn(g, (width, width, 2, 2), 0.02)
    sd["backbone.fpn1.0.bias"] = _cn(g, (width,), 0.02)
    sd["backbone.fpn2.0.weight"] = _cn(g, (width, width, 2, 2), 0.02)
    sd["text_encoder.positional_embedding"] = _cn(g, (13, 512), 0.01)
    sd["neck.lateral_convs.0.conv.weight"] = _cn(g, (256, width, 1, 1), 0.02)
    sd["decode_head.conv_seg.weight"] = _cn(g, (150, 128, 1, 1), 0.02)
    return {"state_dict": sd}


def denseclip_to_engine(ckpt, vision: dict) -> Dict[str, torch.Tensor]:
    """DenseCLIP's loader (load_denseclip_weights / load_denseclip_model, P/src/denseclip/clip_loader/denseclip_loader.py:196-227,
    255-270) -> the engine's CLIP keys (``vit_arch = 1``).  ``vision``: the config's model.vision block.

    * the checkpoint is ``{'state_dict': ...}``; its ``backbone.`` keys are the visual tower, ``text_encoder.`` and everything else (neck,
      decode heads) is not the tower's.  Keys under ``backbone.`` that CLIPVisionTransformer has no parameter for (the FPN layers) are what
      the reference's strict=False drops;
    * NOTHING is rounded: the reference never calls convert_weights here, the tower runs the checkpoint's fp32 values;
    * a tower parameter the checkpoint lacks would stay at its random initial value under strict=False: refused here, ln_post and proj
      included;
    * the position table must be the tower's own, (image_resolution / patch)^2 + 1 rows: load_state_dict's size-mismatch RuntimeError
      (strict=False does not excuse a shape).  It is used at that grid, nothing is resampled."""
    if not isinstance(ckpt, dict) or "state_dict" not in ckpt:
        raise ValueError("Checkpoint doesn't contain 'state_dict': a DenseCLIP checkpoint is {'state_dict': {'backbone.*': ..., ...}}")
    layers, width = int(vision["vision_layers"]), int(vision["vision_width"])
    patch, res = int(vision["vision_patch_size"]), int(vision["image_resolution"])
    want = denseclip_tower_keys(layers)
    vis = {k[len("backbone."):]: v for k, v in ckpt["state_dict"].items() if k.startswith("backbone.")}
    missing = [k for k in want if k not in vis]
    if missing:
        raise KeyError("DenseCLIP checkpoint lacks %d tower tensor(s) under 'backbone.' (first: %s): the reference's strict=False load "
                       "would leave them at their random initial values" % (len(missing), ", ".join(missing[:4])))
    rows = (res // patch) ** 2 + 1
    pe = vis["positional_embedding"]
    if tuple(pe.shape) != (rows, width):
        raise RuntimeError("Error(s) in loading state_dict for CLIPVisionTransformer:\n\tsize mismatch for positional_embedding: copying a "
                           "param with shape torch.Size([%s]) from checkpoint, the shape in current model is torch.Size([%d, %d])."
                           % (", ".join(str(int(d)) for d in pe.shape), rows, width))
    return _openai_visual_to_engine({k: vis[k].detach().float() for k in want})


def add_outlier_channels(w: Dict[str, torch.Tensor], channels=(7, 300, 611), block: int = 1, gain: float = 4000.0,
                         hidden_rows=(11, 2000), hidden_gain: float = 30.0) -> Dict[str, torch.Tensor]:
    """DINOv2-like massive activations for stress tests: the MLP branch of ``block`` is multiplied by ``gain`` on a few
    channels (from there on the fp32 residual stream carries values in the hundreds on those channels and every later
    LayerNorm sees a few dominant channels), and a few hidden units of every later MLP get ``hidden_gain``-times larger
    pre-activations (large fc2 operands).  Returns a modified copy."""
    w = dict(w)
    depth = 1 + max(int(k.split(".")[1]) for k in w if k.startswith("blocks."))
    g2 = w["blocks.%d.ls2.gamma" % block].clone()
    g2[list(channels)] *= gain
    w["blocks.%d.ls2.gamma" % block] = g2
    for i in range(block + 1, depth):
        f = w["blocks.%d.mlp.fc1.weight" % i].clone()
        f[list(hidden_rows)] *= hidden_gain
        w["blocks.%d.mlp.fc1.weight" % i] = f
    return w


CLIP_TEXT_ARCHS = {
    # clip.load name -> (width, layers, heads, embed_dim); context 77 and vocabulary 49 408 for all (clip/model.py build_model)
    "ViT-B/16": (512, 12, 8, 512),
    "ViT-B/32": (512, 12, 8, 512),
    "ViT-L/14": (768, 12, 12, 768),
    "ViT-L/14@336px": (768, 12, 12, 768),
}


def clip_text_arch(name: str):
    if name not in CLIP_TEXT_ARCHS:
        raise ValueError("unsupported CLIP model name %r (known: %s)" % (name, ", ".join(CLIP_TEXT_ARCHS)))
    return CLIP_TEXT_ARCHS[name]


def synth_clip_text(seed: int, name: str = "ViT-B/16", layers: int | None = None, context_length: int = 77,
                    vocab_size: int = 49408) -> Dict[str, torch.Tensor]:
    """State dict shaped like the text half of ``clip.load(name)[0].state_dict()``: token / positional embeddings,
    ``transformer.resblocks.{i}`` (pre-LN, packed ``attn.in_proj_weight``, ``mlp.c_fc`` / ``mlp.c_proj``), ``ln_final`` and
    ``text_projection`` [width, embed_dim]."""
    W, full_layers, _, E = clip_text_arch(name)
    layers = layers or full_layers
    g = torch.Generator().manual_seed(seed)
    w: Dict[str, torch.Tensor] = {}
    w["token_embedding.weight"] = _tn(g, (vocab_size, W), 0.02)
    w["positional_embedding"] = _tn(g, (context_length, W), 0.01)
    for i in range(layers):
        q = "transformer.resblocks.%d." % i
        for ln in ("ln_1", "ln_2"):
            w[q + ln + ".weight"] = 0.5 + torch.rand(W, generator=g)
            w[q + ln + ".bias"] = _tn(g, (W,), 0.02)
        qkv = _tn(g, (3 * W, W), 0.02)
        qkv[: 2 * W] *= 2.5
        w[q + "attn.in_proj_weight"] = qkv
        w[q + "attn.in_proj_bias"] = _tn(g, (3 * W,), 0.02)
        w[q + "attn.out_proj.weight"] = _tn(g, (W, W), 0.02) * 0.3
        w[q + "attn.out_proj.bias"] = _tn(g, (W,), 0.02)
        w[q + "mlp.c_fc.weight"] = _tn(g, (4 * W, W), 0.02)
        w[q + "mlp.c_fc.bias"] = _tn(g, (4 * W,), 0.02)
        w[q + "mlp.c_proj.weight"] = _tn(g, (W, 4 * W), 0.02) * 0.3
        w[q + "mlp.c_proj.bias"] = _tn(g, (W,), 0.02)
    w["ln_final.weight"] = 0.5 + torch.rand(W, generator=g)
    w["ln_final.bias"] = _tn(g, (W,), 0.02)
    w["text_projection"] = _tn(g, (W, E), W ** -0.5)
    return w


def synth_talk2dino(seed: int, clip_dim: int = 512, dino_dim: int = 768, hidden: bool = True) -> Dict[str, torch.Tensor]:
    """A Talk2DINO ``ProjectionLayer`` state dict (P/src/talk2dino/talk2dino.py:73-90): ``linear_layer`` [dino_dim, clip_dim] and,
    unless ``hidden`` is False (linear_talk2dino), ``hidden_layers.0`` [dino_dim, dino_dim]."""
    g = torch.Generator().manual_seed(seed)
    w = {"linear_layer.weight": _tn(g, (dino_dim, clip_dim), clip_dim ** -0.5), "linear_layer.bias": _tn(g, (dino_dim,), 0.02)}
    if hidden:
        w["hidden_layers.0.weight"] = _tn(g, (dino_dim, dino_dim), dino_dim ** -0.5)
        w["hidden_layers.0.bias"] = _tn(g, (dino_dim,), 0.02)
    return w


def synth_decap(seed: int, prefix_size: int = 768, n_layer: int = 4, n_embd: int = 768,
                vocab: int = 50257, n_positions: int = 1024, tok_vocab: int = 49408,
                std: float = 0.02) -> Dict[str, torch.Tensor]:
    """State dict shaped like a DeCap checkpoint (``clip_project`` + ``decoder`` = GPT2LMHeadModel).

    Embedding rows >= ``tok_vocab`` are zero: the LM head is tied, so their logits are exactly 0 and
    a random-weight argmax never emits an id the CLIP tokenizer cannot decode.
    """
    g = torch.Generator().manual_seed(seed)
    E = n_embd

    def n(*shape):
        return torch.randn(*shape, generator=g) * std

    w: Dict[str, torch.Tensor] = {}
    w["clip_project.model.0.weight"] = n(E, prefix_size)
    w["clip_project.model.0.bias"] = n(E)
    wte = n(vocab, E)
    wte[tok_vocab:] = 0
    w["decoder.transformer.wte.weight"] = wte
    w["decoder.transformer.wpe.weight"] = n(n_positions, E)
    for l in range(n_layer):
        p = "decoder.transformer.h.%d." % l
        w[p + "ln_1.weight"] = 0.5 + torch.rand(E, generator=g)
        w[p + "ln_1.bias"] = n(E)
        w[p + "attn.c_attn.weight"] = n(E, 3 * E)      # Conv1D: [in, out]
        w[p + "attn.c_attn.bias"] = n(3 * E)
        w[p + "attn.c_proj.weight"] = n(E, E)
        w[p + "attn.c_proj.bias"] = n(E)
        w[p + "ln_2.weight"] = 0.5 + torch.rand(E, generator=g)
        w[p + "ln_2.bias"] = n(E)
        w[p + "mlp.c_fc.weight"] = n(E, 4 * E)
        w[p + "mlp.c_fc.bias"] = n(4 * E)
        w[p + "mlp.c_proj.weight"] = n(4 * E, E)
        w[p + "mlp.c_proj.bias"] = n(E)
    w["decoder.transformer.ln_f.weight"] = 0.5 + torch.rand(E, generator=g)
    w["decoder.transformer.ln_f.bias"] = n(E)
    w["decoder.lm_head.weight"] = wte  # tied
    return w


def synth_bank(seed: int, rows: int, dim: int = 768) -> torch.Tensor:
    """Text-embedding memory bank ``[rows, dim] ~ N(0,1)`` (un-normalised, as the DINOv2 configs keep it,
    P/src/model.py:174)."""
    g = torch.Generator().manual_seed(seed)
    out = torch.empty(rows, dim)
    step = 65536
    for s in range(0, rows, step):
        e = min(rows, s + step)
        out[s:e] = torch.randn(e - s, dim, generator=g)
    return out


def synth_images(seed: int, batch: int, size: int = 224) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, 3, size, size, generator=g)


# ---------------------------------------------------------------------------------------------------------------------
# ViECap head (P/src/viecap): seeded stand-ins for the checkpoint, the GPT-2 tokenizer files and the entity vocabulary
# ---------------------------------------------------------------------------------------------------------------------
def synth_viecap(seed: int, clip_hidden_size: int = 768, n_layer: int = 12, n_embd: int = 768, vocab: int = 50257,
                 n_positions: int = 1024, tok_vocab: int = 50257, prompt_len: int = 10, project_len: int = 10,
                 map_layers: int = 8, std: float = 0.02) -> Dict[str, torch.Tensor]:
    """State dict shaped like ``ClipCaptionModel.state_dict()`` (P/src/viecap/ClipCap.py:155-200): ``mapping_network.*``
    (Linear C -> project_len x 768, prefix_const, 8 transformer layers with bias-free q / kv projections and a ratio-2 ReLU
    MLP) and ``gpt.*`` (GPT2LMHeadModel, GPT2Config() sizes).  Embedding rows >= ``tok_vocab`` are zero (tied head: logit 0),
    so a random-weight arg-max never leaves the tokenizer's vocabulary."""
    g = torch.Generator().manual_seed(seed)
    E = n_embd

    def n(*shape, s=std):
        return torch.randn(*shape, generator=g) * s

    w: Dict[str, torch.Tensor] = {}
    w["mapping_network.linear.weight"] = n(project_len * E, clip_hidden_size, s=0.05)
    w["mapping_network.linear.bias"] = n(project_len * E)
    w["mapping_network.prefix_const"] = n(prompt_len, E, s=0.5)
    for l in range(map_layers):
        p = "mapping_network.transformer.layers.%d." % l
        w[p + "norm1.weight"] = 0.5 + torch.rand(E, generator=g)
        w[p + "norm1.bias"] = n(E)
        w[p + "attn.to_queries.weight"] = n(E, E, s=0.04)
        w[p + "attn.to_keys_values.weight"] = n(2 * E, E, s=0.04)
        w[p + "attn.project.weight"] = n(E, E)
        w[p + "attn.project.bias"] = n(E)
        w[p + "norm2.weight"] = 0.5 + torch.rand(E, generator=g)
        w[p + "norm2.bias"] = n(E)
        w[p + "mlp.fc1.weight"] = n(2 * E, E)
        w[p + "mlp.fc1.bias"] = n(2 * E)
        w[p + "mlp.fc2.weight"] = n(E, 2 * E)
        w[p + "mlp.fc2.bias"] = n(E)
    wte = n(vocab, E)
    wte[tok_vocab:] = 0
    w["gpt.transformer.wte.weight"] = wte
    w["gpt.transformer.wpe.weight"] = n(n_positions, E)
    for l in range(n_layer):
        p = "gpt.transformer.h.%d." % l
        w[p + "ln_1.weight"] = 0.5 + torch.rand(E, generator=g)
        w[p + "ln_1.bias"] = n(E)
        w[p + "attn.c_attn.weight"] = n(E, 3 * E)      # Conv1D: [in, out]
        w[p + "attn.c_attn.bias"] = n(3 * E)
        w[p + "attn.c_proj.weight"] = n(E, E)
        w[p + "attn.c_proj.bias"] = n(E)
        w[p + "ln_2.weight"] = 0.5 + torch.rand(E, generator=g)
        w[p + "ln_2.bias"] = n(E)
        w[p + "mlp.c_fc.weight"] = n(E, 4 * E)
        w[p + "mlp.c_fc.bias"] = n(4 * E)
        w[p + "mlp.c_proj.weight"] = n(4 * E, E)
        w[p + "mlp.c_proj.bias"] = n(E)
    w["gpt.transformer.ln_f.weight"] = 0.5 + torch.rand(E, generator=g)
    w["gpt.transformer.ln_f.bias"] = n(E)
    w["gpt.lm_head.weight"] = wte  # tied
    return w


def synth_clipcap(seed: int, C: int = 768, prefix_length: int = 10, n_layer: int = 12, n_embd: int = 768, vocab: int = 50257,
                  n_positions: int = 1024, tok_vocab: int = 50257, std: float = 0.02) -> Dict[str, torch.Tensor]:
    """State dict shaped like the reference's ClipCap checkpoint with the MLP mapper (P/src/clipcap/entrypoint.py:20-31, 140-181):
    ``clip_project.model.0.*`` (Linear C -> prefix_length x n_embd / 2), ``clip_project.model.2.*`` (Linear -> prefix_length x n_embd)
    and ``gpt.*``, generated as for ViECap (synth_viecap)."""
    w = {k: v for k, v in synth_viecap(seed, n_layer=n_layer, n_embd=n_embd, vocab=vocab, n_positions=n_positions, tok_vocab=tok_vocab,
                                       map_layers=0, std=std).items() if k.startswith("gpt.")}
    g = torch.Generator().manual_seed(seed + 7919)
    H, O = prefix_length * n_embd // 2, prefix_length * n_embd
    w["clip_project.model.0.weight"] = torch.randn(H, C, generator=g) * (1.0 / C ** 0.5)
    w["clip_project.model.0.bias"] = torch.randn(H, generator=g) * 0.1
    w["clip_project.model.2.weight"] = torch.randn(O, H, generator=g) * (0.5 / H ** 0.5)
    w["clip_project.model.2.bias"] = torch.randn(O, generator=g) * 0.1
    return w


SYNTH_ENTITIES = ["person", "bicycle", "car", "motorcycle", "airplane", "bus", "train", "truck", "boat", "traffic light",
                  "fire hydrant", "stop sign", "bench", "bird", "cat", "dog", "horse", "sheep", "cow", "elephant", "bear", "zebra",
                  "giraffe", "backpack", "umbrella", "handbag", "tie", "suitcase", "frisbee", "skis", "kite", "baseball bat"]


def synth_entity_embeddings(seed: int, count: int, dim: int) -> torch.Tensor:
    return torch.randn(count, dim, generator=torch.Generator().manual_seed(seed))


def synth_bpe(seed: int = 0, merges: int = 400):
    """A small byte-level BPE vocabulary in GPT-2's file format (vocab dict, ranked merges) learnt on the words the ViECap
    hard prompt is made of ("There are ... in image.", the entity names) plus seeded filler words: the real ``vocab.json`` /
    ``merges.txt`` are not on this image.  -> (vocab: token -> id, merges: list of pairs); ids 0..255 are the byte tokens."""
    import random
    from .viecap import ByteLevelBPE, _bytes_to_unicode
    import regex
    rng = random.Random(seed)
    b2u = _bytes_to_unicode()
    words = ["There are something in image.", "There are " + ", ".join(SYNTH_ENTITIES) + " in image.", " .", "."]
    letters = "abcdefghijklmnopqrstuvwxyz"
    for _ in range(300):
        words.append(" " + "".join(rng.choice(letters) for _ in range(rng.randint(2, 8))))
    pat = regex.compile(ByteLevelBPE.PATTERN)
    corpus = []
    for t in words:
        for piece in pat.findall(t):
            corpus.append(["".join(b2u[b] for b in piece.encode("utf-8"))][0])
    seqs = [list(w) for w in corpus]
    vocab = {b2u[b]: b for b in range(256)}
    merge_list = []
    for _ in range(merges):
        counts = {}
        for sq in seqs:
            for a, b in zip(sq, sq[1:]):
                counts[(a, b)] = counts.get((a, b), 0) + 1
        if not counts:
            break
        best = max(sorted(counts), key=lambda p: counts[p])
        if counts[best] < 2:
            break
        merge_list.append(best)
        vocab[best[0] + best[1]] = len(vocab)
        for sq in seqs:
            i = 0
            while i < len(sq) - 1:
                if sq[i] == best[0] and sq[i + 1] == best[1]:
                    sq[i:i + 2] = [best[0] + best[1]]
                else:
                    i += 1
    return vocab, merge_list


# ---- RegionCLIP: CLIP's ModifiedResNet (P/src/regionclip/clip_backbone.py:112-300, loader.py:60-231) ----
# name -> (Bottleneck units per stage, stem width, attnpool width, heads, output width); heads = width * 32 // 64 (clip_backbone.py:705)
_REGIONCLIP_ARCH = {"RN50": ((3, 4, 6, 3), 64, 2048, 32, 1024), "RN50x4": ((4, 6, 10, 6), 80, 2560, 40, 640)}
FROZEN_BN_EPS = 1e-5     # detectron2.layers.FrozenBatchNorm2d(num_features, eps=1e-5)


def regionclip_arch(spec):
    """``spec``: "RN50" / "RN50x4", a detectron2 RESNETS.DEPTH (50 / 200, clip_backbone.py:183-192) or the (4,) layer counts
    -> (layers, width, embed_dim, heads, output_dim)."""
    if isinstance(spec, int):
        spec = {50: "RN50", 200: "RN50x4"}.get(spec, spec)
    if isinstance(spec, (tuple, list)):
        for v in _REGIONCLIP_ARCH.values():
            if tuple(spec) == v[0]:
                return v
        raise ValueError("RegionCLIP layers %r: this build knows RN50 %r and RN50x4 %r" % (tuple(spec), _REGIONCLIP_ARCH["RN50"][0],
                                                                                          _REGIONCLIP_ARCH["RN50x4"][0]))
    if spec not in _REGIONCLIP_ARCH:
        raise ValueError("RegionCLIP backbone %r: this build knows RN50 and RN50x4" % (spec,))
    return _REGIONCLIP_ARCH[spec]


def _rn_strip(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The visual tower's keys without their prefix: a RegionCLIP checkpoint's ``backbone.*`` (under 'model' or 'state_dict',
    loader.py:85-110) or a plain CLIP dict's ``visual.*``; the text tower's keys are dropped."""
    for wrap in ("model", "state_dict"):
        if wrap in sd and isinstance(sd[wrap], dict):
            sd = sd[wrap]
    out = {}
    for k, v in sd.items():
        for pre in ("backbone.", "visual."):
            if k.startswith(pre):
                out[k[len(pre):]] = v
    if not out:
        raise KeyError("no 'backbone.*' or 'visual.*' keys: not a RegionCLIP / CLIP ResNet checkpoint")
    return out


def regionclip_layers(sd: Dict[str, torch.Tensor]):
    """(layer counts, stem width, attnpool grid side, output width) of a tower's state dict (loader.py:193-199, 207)."""
    v = _rn_strip(sd)
    counts = tuple(len({k.split(".")[1] for k in v if k.startswith("layer%d." % b)}) for b in (1, 2, 3, 4))
    width = int(v["layer1.0.conv1.weight"].shape[0])
    grid = round((v["attnpool.positional_embedding"].shape[0] - 1) ** 0.5)
    return counts, width, grid, int(v["attnpool.c_proj.weight"].shape[0])


def frozen_bn_affine(w, b, mean, var, eps: float = FROZEN_BN_EPS):
    """FrozenBatchNorm2d in eval as F.batch_norm evaluates it on the CPU (ATen's batch_norm_cpu_inference: invstd = 1 / sqrt(var +
    eps), alpha = invstd * weight, beta = bias - mean * alpha, all fp32) -> (scale, shift), y = x * scale + shift."""
    w, b, mean, var = (t.detach().float() for t in (w, b, mean, var))
    inv = 1.0 / torch.sqrt(var + eps)
    scale = inv * w
    return scale, b - mean * scale


def regionclip_to_engine(sd: Dict[str, torch.Tensor], pos: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """RegionCLIP / CLIP ResNet state dict -> the engine's ``rn.*`` keys: convolutions rounded to fp16 values (_fp16_values), every FrozenBN as a
    ``.scale`` / ``.shift`` pair (frozen_bn_affine), the attnpool's q | k | v concatenated along the rows (the in_proj of
    F.multi_head_attention_forward, clip_backbone.py:87-102).  ``pos`` replaces the attnpool position table (quirk 1, model.py)."""
    v = _rn_strip(sd)
    out: Dict[str, torch.Tensor] = {}
    bn_names = {k[:-len(".running_var")] for k in v if k.endswith(".running_var")}
    for k, t in v.items():
        if k.startswith("attnpool."):
            continue
        base = k.rsplit(".", 1)[0]
        if base in bn_names:
            continue
        if k.endswith(".weight"):
            out["rn." + k] = _fp16_values(t)
    for base in bn_names:
        sc, sh = frozen_bn_affine(v[base + ".weight"], v[base + ".bias"], v[base + ".running_mean"], v[base + ".running_var"])
        out["rn.%s.scale" % base], out["rn.%s.shift" % base] = sc, sh
    a = "attnpool."
    out["rn.attnpool.positional_embedding"] = (v[a + "positional_embedding"] if pos is None else pos).detach().float()
    out["rn.attnpool.qkv.weight"] = _fp16_values(torch.cat([v[a + x + "_proj.weight"] for x in "qkv"], 0))
    out["rn.attnpool.qkv.bias"] = _fp16_values(torch.cat([v[a + x + "_proj.bias"] for x in "qkv"], 0))
    out["rn.attnpool.c_proj.weight"] = _fp16_values(v[a + "c_proj.weight"])
    out["rn.attnpool.c_proj.bias"] = _fp16_values(v[a + "c_proj.bias"])
    return out


def _fp16_values(t: torch.Tensor) -> torch.Tensor:
    """fp32 tensor holding the fp16 values the reference computes with: loader.py always runs convert_weights
    (clip_backbone.py:578-599), which turns every Conv2d / Linear weight and bias to fp16 before the checkpoint is loaded into
    them -- so a checkpoint's fp32 values are rounded, in the fp32 parity mode too.  FrozenBN buffers and the attnpool's position
    table are not converted (they stay fp32)."""
    return t.detach().float().half().float()


def synth_regionclip_rn(seed: int, name: str = "RN50", layers=None, image_resolution: int = 224,
                        prefix: str = "visual.") -> Dict[str, torch.Tensor]:
    """Seeded ModifiedResNet weights under ``prefix`` (``visual.`` = a CLIP dict, ``backbone.`` = a RegionCLIP checkpoint's):
    conv / Linear weights with fp16 values (loader.py always runs convert_weights), fp32 FrozenBN buffers with realistic
    statistics, bn3 weights nonzero but small so that every residual branch counts and fp16 activations stay O(1) through all
    blocks; ``layers`` overrides the unit counts (reduced depth for fast tests).  The attnpool table has
    (image_resolution / 32)^2 + 1 rows; ``text_projection`` [*, output width] is included (loader.py:207)."""
    arch_layers, width, embed, heads, out_dim = regionclip_arch(name)
    layers = tuple(layers) if layers is not None else arch_layers
    g = torch.Generator().manual_seed(seed)
    w: Dict[str, torch.Tensor] = {}

    def conv(key, cout, cin, k):
        w[prefix + key] = (torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5).half().float()

    def bn(key, c, gain=(0.6, 1.2)):
        w[prefix + key + ".weight"] = gain[0] + (gain[1] - gain[0]) * torch.rand(c, generator=g)
        w[prefix + key + ".bias"] = 0.1 * torch.randn(c, generator=g)
        w[prefix + key + ".running_mean"] = 0.1 * torch.randn(c, generator=g)
        w[prefix + key + ".running_var"] = 0.5 + torch.rand(c, generator=g)

    conv("conv1.weight", width // 2, 3, 3); bn("bn1", width // 2)
    conv("conv2.weight", width // 2, width // 2, 3); bn("bn2", width // 2)
    conv("conv3.weight", width, width // 2, 3); bn("bn3", width)
    inplanes = width
    for L in range(4):
        planes = width << L
        for i in range(layers[L]):
            p = "layer%d.%d." % (L + 1, i)
            conv(p + "conv1.weight", planes, inplanes, 1); bn(p + "bn1", planes)
            conv(p + "conv2.weight", planes, planes, 3); bn(p + "bn2", planes)
            conv(p + "conv3.weight", 4 * planes, planes, 1); bn(p + "bn3", 4 * planes, gain=(0.15, 0.35))
            if i == 0:
                conv(p + "downsample.0.weight", 4 * planes, inplanes, 1); bn(p + "downsample.1", 4 * planes, gain=(0.5, 1.0))
            inplanes = 4 * planes
    s = image_resolution // 32
    a = prefix + "attnpool."
    w[a + "positional_embedding"] = torch.randn(s * s + 1, embed, generator=g) / embed ** 0.5
    for x in "qkv":
        w[a + x + "_proj.weight"] = (torch.randn(embed, embed, generator=g) * embed ** -0.5).half().float()
        w[a + x + "_proj.bias"] = (0.02 * torch.randn(embed, generator=g)).half().float()
    w[a + "c_proj.weight"] = (torch.randn(out_dim, embed, generator=g) * embed ** -0.5).half().float()
    w[a + "c_proj.bias"] = (0.02 * torch.randn(out_dim, generator=g)).half().float()
    w["text_projection"] = torch.zeros(8, out_dim)
    return w
