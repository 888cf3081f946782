"""Seeded synthetic weights in the reference checkpoints' own key names.

There is no network on the build or GPU boxes, so the DINOv2 hub weights
(P/src/model.py:342-343), the DeCap decoder checkpoint (P/src/decap/decap.py:188-222) and the
text memory bank (P/src/decap/im2txtprojection/im2txtprojection.py:387-407) are replaced by
deterministic synthetic tensors of the same shapes and names.  Real checkpoints
load through the same dict interface (see ``model.Patchioner.from_config``).

All generators use a CPU ``torch.Generator`` so the numbers are identical on every box.
"""
from __future__ import annotations

from typing import Dict

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
    src = {(k[len("visual."):] if k.startswith("visual.") else k): v for k, v in sd.items()}
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
    if "patch_embed.alpha.weight" not in out:
        pw = out["patch_embed.proj.weight"]
        out["patch_embed.alpha.weight"] = torch.zeros(pw.shape[0], 1, pw.shape[2], pw.shape[3], dtype=pw.dtype)
    return out


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
