"""Host-side mirror of the reference ``Patchioner`` (P/src/model.py:96-1581) over the HIP engine.

Same constructor keywords, ``from_config`` / ``forward`` / ``caption_tokens`` / ``caption_bboxes`` signatures,
attributes (``image_transforms``, ``image_transforms_no_crop``, ``resize_dim``, ``crop_dim``, ``patch_size``,
``num_tokens``, ``embed_dim`` ...) and output dictionary as the reference, so the ``eval-*-captioning``
drivers run unchanged.  Everything numerical is a C-ABI call into libpatchioner_hip.so; there is no CPU
path (constructing the model without a GPU or without the built library raises).

Scope: the DINOv2(+registers), timm OpenAI-CLIP, AlphaCLIP, RegionCLIP, INViTE and DenseCLIP backbones with the
DeCap / CapDec, ViECap and ClipCap (MLP mapper) heads.  The other backbones and heads of the reference (ProxyCLIP, OpenCLIP, DINO.txt,
MeaCap) raise ``NotImplementedError`` or ``ValueError`` at construction.

Build-specific config keys (there is no network on the target, so nothing is fetched from torch.hub / HF):
  dino_weights     path (.pt/.pth state dict) or dict of the DINOv2 backbone weights
  memory_bank      path (.npy / .pt / .h5) or tensor [M, D] of the text memory bank
  synthetic_seed   int: synthesise any weights / bank not given (seeded; see weights.py)
  max_batch, max_prefixes, vit_dtype ("fp16" | "bf16")
  stop_at_eos      False (default) | True: the synchronous greedy decodes (DeCap / CapDec without compute_scores, the greedy ViECap head)
                   end once every caption of the call has emitted its end token, in segments of stop_segment steps (None: the engine's
                   default, engine.DEFAULT_STOP_SEGMENT).  Same strings; forward_async and the pipelines run full length as before.
                   ``model.stop_at_eos`` may be toggled after construction
  denseclip_config   a dict of the DenseCLIP YAML's structure, a .yaml path, or a config name (denseclip.py); denseclip_config_dir: where
                   names are looked up (else $PIO_DENSECLIP_CONFIG_DIR, else the two built-in names); denseclip_checkpoint: a local
                   checkpoint file or {'state_dict': ...} that replaces the config's checkpoint.path
  sparse_last_block  None (default): traces-only calls run the last block on the rows the traces read on the DINOv2 and DenseCLIP
                   backbones; True: on the timm-CLIP and INViTE (extract_last_k_th_token <= 0) towers as well; False: never
  clip_text_weights  path (clip.load JIT archive or state dict) or dict of the CLIP text tower that encodes
                   ``online_texts`` (clip_text.py).  Order of the sources: this key, ~/.cache/clip/<name>.pt (where clip.load
                   puts it), synthetic_seed, else FileNotFoundError
  clip_text_dtype  "fp16" (default) | "fp32": operands of that text tower (fp32 = the exact parity mode)
  talk2dino_projection_weights  path or dict of the Talk2DINO ProjectionLayer that maps the online_texts features into the
                   DINOv2 space (use_talk2dino_project).  Order: this key, talk2dino_weights, synthetic_seed, else
                   FileNotFoundError
"""
from __future__ import annotations

import os
import random
from typing import List, Optional

import torch
import torch.nn as nn
import yaml

from . import weights as W
from .backbones import _load_state_dict, route_backbone
from .backbones import _denseclip_routed, _denseclip_setup, _invite_setup, _regionclip_setup  # noqa: F401  (their old import path)
from .engine import Engine
from .preprocess import CLIP_MEAN, CLIP_STD, make_transforms
from .tokenizer import ClipDetokenizer

_OUT_OF_SCOPE = ("proxyclip_clipmodel",)


def load_memory_bank(spec, want_texts: bool = False):
    """[M, D] fp32 text-embedding bank (Im2TxtProjector._load_support_memory,
    P/src/decap/im2txtprojection/im2txtprojection.py:387-407: HDF5 datasets '<name>-embeddings' and '<name>-text',
    read by the dependency-free h5lite).  ``want_texts``: returns (bank, list of bytes | None)."""
    bank, texts = _load_memory_bank(spec)
    return (bank, texts) if want_texts else bank


def _load_memory_bank(spec):
    if isinstance(spec, torch.Tensor):
        return spec.float(), None
    if not os.path.exists(spec):
        raise FileNotFoundError("memory bank %r not found" % (spec,))
    if spec.endswith(".npy"):
        import numpy as np
        return torch.from_numpy(np.load(spec)).float(), None
    if spec.endswith(".pt") or spec.endswith(".pth"):
        return torch.load(spec, map_location="cpu").float(), None
    if spec.endswith(".h5") or spec.endswith(".hdf5"):
        from . import h5lite
        names = [k for k in h5lite.dataset_names(spec) if k.endswith("-embeddings")]
        if not names:
            raise KeyError("no '<name>-embeddings' dataset in %r" % spec)
        tname = names[0][:-len("-embeddings")] + "-text"
        d = h5lite.read_datasets(spec, names=(names[0], tname))
        return torch.from_numpy(d[names[0]]).float(), d.get(tname)
    raise ValueError("unsupported memory bank format: %r" % (spec,))


class Patchioner(nn.Module):

    def __init__(self, decoder_weights, device, prefix_size, linear_talk2dino, support_memory_size, projection_type=None,
                 dino_model=None, proxyclip_clipmodel=None, proxyclip_vfm=None, use_talk2dino_project=True, normalize=True,
                 attention_type='qkv', talk2dino_config=None, talk2dino_weights=None, resize_dim=518, crop_dim=518,
                 talk2dino_attn_type='qkv', calculate_argmax_text=False, online_texts=None, clip_model_name=None,
                 use_open_clip=False, viecap_config=None, regionclip_config=None, invite_config=None,
                 denseclip_config=None, alphaclip_config=None, clipcap_config=None, hf_repo_id=None,
                 dino_weights=None, memory_bank=None, synthetic_seed=None, max_batch=16, max_prefixes=128,
                 vit_dtype="fp16", memory_bank_texts=None, clip_text_weights=None, clip_text_dtype="fp16",
                 talk2dino_projection_weights=None, denseclip_config_dir=None, denseclip_checkpoint=None, sparse_last_block=None,
                 stop_at_eos=False, stop_segment=None, **kwargs):
        super().__init__(**kwargs)
        given = dict(proxyclip_clipmodel=proxyclip_clipmodel)
        for k in _OUT_OF_SCOPE:
            if given[k] is not None:
                raise NotImplementedError("%s: backbone/head outside the MI355X hot-path scope (DINOv2 + DeCap/CapDec)" % k)
        if clipcap_config is not None:
            # the ClipCap head's config is checked strictly, before anything touches the device, the weights or the tokenizer: a key
            # the head does not implement raises NotImplementedError naming it (the reference ignores unknown keys)
            from .clipcap import validate_config as _validate_clipcap
            clipcap_config = _validate_clipcap(clipcap_config)
        if use_open_clip:
            raise NotImplementedError("use_open_clip: OpenCLIP text-tower weights are not supported (the OpenAI CLIP text tower "
                                      "is: online_texts, bank.build_memory_bank)")
        if online_texts is not None and (isinstance(online_texts, (str, bytes)) or not all(isinstance(t, str) for t in online_texts)):
            raise TypeError("online_texts must be a list of str")
        if online_texts is not None and support_memory_size > 0 and len(online_texts) == 0:
            raise ValueError("online_texts is empty")
        # the family is decided here and the config-routed towers are set up (backbones.py); the two name-routed towers read their
        # weights when load_backbone() is called, behind the refusals below, as they always have
        load_backbone = route_backbone(dino_model=dino_model, regionclip_config=regionclip_config, invite_config=invite_config,
                                       denseclip_config=denseclip_config, alphaclip_config=alphaclip_config, dino_weights=dino_weights,
                                       attention_type=attention_type, resize_dim=resize_dim, crop_dim=crop_dim,
                                       synthetic_seed=synthetic_seed, online_texts=online_texts, denseclip_config_dir=denseclip_config_dir,
                                       denseclip_checkpoint=denseclip_checkpoint, sparse_last_block=sparse_last_block)
        if viecap_config is not None and viecap_config.get('meacap', False):
            raise NotImplementedError("MeaCap head (retrieved-caption scene graphs, flan-T5): outside the hot-path scope")
        if decoder_weights is None and synthetic_seed is None and not calculate_argmax_text and viecap_config is None and clipcap_config is None:
            raise ValueError("decap_weights is required (or synthetic_seed for seeded synthetic weights)")
        self.decoding_method = None
        self.viecap = None
        self.clipcap = None
        self.calculate_argmax_text = bool(calculate_argmax_text)
        self.text_dataset = memory_bank_texts

        # same validation order as the reference (P/src/model.py:144-162)
        if online_texts is not None or projection_type in ('coco', 'msmarco', 'blip', 'vg', 'vg-test') or support_memory_size == 0:
            pass
        elif projection_type is not None and os.path.exists(projection_type):
            pass
        elif memory_bank is None and synthetic_seed is None:
            raise Exception("The projection_type field must be 'coco', 'msmarco', 'blip' or 'vg'")

        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("patchioner_amd runs on an MI355X only (device=%r): there is no CPU path; the CPU "
                               "restatement used for parity lives in oracle/ and is test infrastructure" % (device,))
        self._device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())

        self.normalize = normalize
        # traces-only calls run the backbone's last block on the rows the traces read (forward, TraceCaptionPipeline); False: always dense
        # (sparse_last_block=None: on, for the backbones that take it by default -- DINOv2 and DenseCLIP; True: the timm-CLIP and INViTE
        # extract_last_k_th_token <= 0 towers as well, whose launches are otherwise exactly what they were)
        self.sparse_last_block = sparse_last_block is None or bool(sparse_last_block)
        self.resize_dim = resize_dim
        self.crop_dim = crop_dim
        self.model_name = dino_model
        bb = self._backbone = load_backbone()
        self.backbone_type = bb.kind
        self.num_global_tokens, self._G = bb.num_global_tokens, bb.grid_globals
        self.token_dim, self.embed_dim, self.patch_size = bb.token_dim, bb.embed_dim, bb.patch_size
        if bb.config is not None:
            setattr(self, bb.kind.lower() + "_config", bb.config)       # regionclip_config, alphaclip_config, denseclip_config
        self.num_patch_tokens = crop_dim // bb.patch_size * crop_dim // bb.patch_size
        self.num_tokens = self.num_global_tokens + self.num_patch_tokens
        self.num_attn_heads = bb.readout_heads
        self.scale = 0.125
        stats = (CLIP_MEAN, CLIP_STD) if bb.clip_stats else (None, None)
        self.image_transforms, self.image_transforms_no_crop = make_transforms(resize_dim, crop_dim, *stats)
        if bb.transform_resolution is not None:
            # the no-crop transform still squares to resize_dim
            self.image_transforms = make_transforms(bb.transform_resolution, bb.transform_resolution, *stats)[0]

        dec_sd = _load_state_dict(decoder_weights)
        if dec_sd is None and synthetic_seed is not None and viecap_config is None:
            dec_sd = W.synth_decap(synthetic_seed + 2, prefix_size)
        viecap_sd = None
        if viecap_config is not None:
            # P/src/model.py:107-113: the ViECap head replaces the DeCap decode (caption_tokens, :1394-1398).  The engine
            # holds ONE language model: GPT-2-base (12 layers, 12 heads) from the ViECap checkpoint; the DeCap weights the
            # reference also loads are never used on this path and are not loaded here.
            from .viecap import load_viecap_weights
            viecap_sd = load_viecap_weights(viecap_config)
            dec_sd = None
        clipcap_tok = None
        # with a ViECap block as well, the reference's caption_tokens tests viecap first (P/src/model.py:1394-1404): its ClipCap head is
        # built and never reached.  Here it is validated (above) and not built.
        if clipcap_config is not None and viecap_config is None:
            # P/src/model.py:115-121, 1399-1404: the ClipCap head replaces the DeCap decode; as for ViECap the engine holds ONE language
            # model, the checkpoint's GPT-2 (`gpt.*`), next to its MLP mapper (`clip_project.model.0 / .2`)
            from .clipcap import load_clipcap_weights, resolve_tokenizer
            clipcap_tok = resolve_tokenizer(clipcap_config)
            from .clipcap import DEFAULTS as _CLIPCAP_DEFAULTS
            if clipcap_config.get("weights") is None and synthetic_seed is not None and clipcap_config["weight_path"] == _CLIPCAP_DEFAULTS["weight_path"]:
                # the vocabulary is the tokenizer's: a sampled id (unlike a random-weight arg-max) would leave a smaller one
                nv = len(clipcap_tok) if hasattr(clipcap_tok, "__len__") else 50257
                viecap_sd = W.synth_clipcap(synthetic_seed + 2, C=self.token_dim, prefix_length=int(clipcap_config["prefix_length"]),
                                            vocab=nv, tok_vocab=nv)
            else:
                viecap_sd = load_clipcap_weights(clipcap_config)
            dec_sd = None

        self.embed_inversion = talk2dino_weights is not None
        inv_sd = {}
        if self.embed_inversion:
            t2d = _load_state_dict(talk2dino_weights)
            A = t2d["linear_layer.weight"].float()       # [dino_dim, clip_dim]
            U, S, Vh = torch.linalg.svd(A, full_matrices=False)      # get_pseudo_inverse, embedding_utils.py:3-15
            S_pinv = torch.zeros_like(S)
            S_pinv[S > 1e-10] = 1.0 / S[S > 1e-10]
            inv_sd["talk2dino.A_pinv"] = (Vh.T @ torch.diag(S_pinv) @ U.T).contiguous()
            inv_sd["talk2dino.b"] = t2d["linear_layer.bias"].float()

        dec_kw = {}
        if viecap_sd is not None:
            n_layer = 1 + max(int(k.split(".")[3]) for k in viecap_sd if k.startswith("gpt.transformer.h."))
            dec_kw = dict(dec_layers=n_layer, dec_heads=12, max_steps=256,
                          dec_vocab=int(viecap_sd["gpt.transformer.wte.weight"].shape[0]),
                          dec_positions=int(viecap_sd["gpt.transformer.wpe.weight"].shape[0]))
        self.engine = Engine(depth=bb.depth, num_heads=bb.heads, crop_dim=crop_dim, patch_size=bb.patch_size, prefix_size=prefix_size,
                             max_batch=max_batch, max_prefixes=max_prefixes, vit_dtype=vit_dtype,
                             device_index=self._device.index, readout_heads=self.num_attn_heads, readout_scale=self.scale,
                             **bb.engine_kw, **dec_kw)
        self.engine.load_state_dict(bb.state_dict)
        if dec_sd is not None:                         # calculate_argmax_text without decoder weights: no decoder (model.py:165)
            self.engine.load_state_dict(dec_sd)        # strict=False like the reference (decap.py:214)
        if viecap_sd is not None:
            self.engine.load_state_dict({k: v for k, v in viecap_sd.items() if k.startswith(("mapping_network.", "gpt.", "clip_project.model."))})
        if inv_sd:
            self.engine.load_state_dict(inv_sd)
        self.engine.finalize()
        if viecap_config is not None:
            from .viecap import VieCapHead
            self.viecap = VieCapHead(viecap_config, self.engine, clip_model_name)
        elif clipcap_config is not None:
            from .clipcap import ClipCapHead
            self.clipcap = ClipCapHead(clipcap_config, self.engine, tokenizer=clipcap_tok)

        if support_memory_size > 0:
            if online_texts is not None:
                # the reference's ONLINE_TEXTS bank (im2txtprojection.py:491-493, 551-553): the texts' features in order, no
                # padding to support_memory_size; zero-norm rows are dropped below (engine.set_memory_bank)
                texts = list(online_texts)
                bank = self._online_bank(texts, dino_model, clip_model_name, use_talk2dino_project, linear_talk2dino,
                                         clip_text_weights, clip_text_dtype, talk2dino_projection_weights, talk2dino_weights,
                                         synthetic_seed)
                bank = bank[bank.norm(dim=-1) != 0]
                self.text_dataset = [t.encode() for t in texts]
            elif memory_bank is not None:
                bank, texts = load_memory_bank(memory_bank, want_texts=True)
                if self.text_dataset is None:
                    self.text_dataset = texts
            elif synthetic_seed is not None:
                bank = W.synth_bank(synthetic_seed + 3, support_memory_size, self.token_dim)
            else:
                raise FileNotFoundError("support_memory_size > 0 needs `memory_bank` (path or tensor): building the "
                                        "bank (CLIP text tower + datasets) is offline work outside this scope")
            if bb.normalize_bank:      # normalize_memory_embs (P/src/model.py:174; im2txtprojection.py:348-349): the CLIP ViTs
                bank = bank / bank.norm(dim=-1, keepdim=True)
            if bank.dim() != 2 or bank.shape[1] != self.token_dim:
                raise ValueError("memory bank is %s, the %s backbone needs [M, %d]" % (tuple(bank.shape), dino_model, self.token_dim))
            self.engine.set_memory_bank(bank)
            self.im_proj = self.engine
        else:
            self.im_proj = None
        if self.calculate_argmax_text:
            if self.im_proj is None or self.text_dataset is None:
                raise ValueError("calculate_argmax_text needs the memory bank AND its caption texts (the '<name>-text' dataset of "
                                 "the bank's .h5, or `memory_bank_texts`)")
            self.text_dataset = [t if isinstance(t, bytes) else str(t).encode("utf-8") for t in self.text_dataset]
        self.tokenizer = ClipDetokenizer()
        self.last_ids = None
        # stop_at_eos: see the module docstring; last_decode_steps: steps every chunk of the last caption_tokens decode ran when it went
        # through the stopping entry points, None after a full-length or deferred decode
        self.stop_at_eos = bool(stop_at_eos)
        self.stop_segment = None if stop_segment is None else int(stop_segment)
        self.last_decode_steps = None
        self.call_log = None            # tests: a list collects (decoder prefix, greedy ids) of every caption_tokens call
        self._defer = False
        self.dino = self.engine     # callers test `model.dino is not None`
        # one zero-size parameter so `next(model.parameters()).device` works as in the reference
        self._anchor = nn.Parameter(torch.zeros(0, device=self._device), requires_grad=False)

    def _online_bank(self, texts, dino_model, clip_model_name, use_talk2dino, linear_talk2dino, clip_text_weights, clip_text_dtype,
                     talk2dino_projection_weights, talk2dino_weights, synthetic_seed) -> torch.Tensor:
        """CLIP text features of ``texts`` on the device (clip_text.ClipTextEncoder), through Talk2DINO's text projection
        with ``use_talk2dino`` (bank.py: the same step as a bank build).  The text tower's device memory is freed here."""
        from .bank import default_clip_model, talk2dino_text_weights
        from .clip_text import ClipTextEncoder
        name = clip_model_name or default_clip_model(use_talk2dino)
        enc = ClipTextEncoder(name, weights=clip_text_weights, synthetic_seed=None if synthetic_seed is None else synthetic_seed + 5,
                              operand_type=clip_text_dtype, device=self._device)
        try:
            feats = enc.encode_text(texts)
        finally:
            enc.close()
        if not use_talk2dino:
            return feats
        t2d = _load_state_dict(talk2dino_projection_weights if talk2dino_projection_weights is not None else talk2dino_weights)
        if t2d is None:
            if synthetic_seed is None:
                raise FileNotFoundError("online_texts with use_talk2dino_project needs the Talk2DINO projection: set "
                                        "talk2dino_projection_weights or talk2dino_weights (or synthetic_seed)")
            t2d = W.synth_talk2dino(synthetic_seed + 6, feats.shape[1], self.token_dim, hidden=not linear_talk2dino)
        w = talk2dino_text_weights(t2d)
        if linear_talk2dino:
            w["w2"] = w["b2"] = None
        return self.engine.text_project(feats, w["w1"], w["b1"], w["w2"], w["b2"], act="tanh")

    # ------------------------------------------------------------------------------------------
    @classmethod
    def from_config(cls, config, device='cpu', online_texts=None):
        if type(config) is str:
            if os.path.exists(config):
                with open(config, 'r') as f:
                    config = yaml.safe_load(f)
            else:
                raise FileNotFoundError("config %r is not a local YAML file (HuggingFace download needs network)" % (config,))
        model = cls(
            projection_type=config.get('projection_type', 'coco'),
            decoder_weights=config.get('decap_weights', None),
            device=device,
            prefix_size=config['prefix_size'],
            linear_talk2dino=config.get('linear_talk2dino', False),
            support_memory_size=config['support_memory_size'],
            dino_model=config.get('dino_model', None),
            proxyclip_clipmodel=config.get('proxyclip_clipmodel', None),
            proxyclip_vfm=config.get('proxyclip_vfm', None),
            use_talk2dino_project=config.get('use_talk2dino_project', True),
            normalize=config.get('normalize', True),
            attention_type=config.get('attention_type', 'qkv'),
            talk2dino_config=config.get('talk2dino_config', None),
            talk2dino_weights=config.get('talk2dino_weights', None),
            resize_dim=config.get('resize_dim', 518),
            crop_dim=config.get('crop_dim', 518),
            talk2dino_attn_type=config.get('talk2dino_attn_type', 'qkv'),
            calculate_argmax_text=config.get('calculate_argmax_text', False),
            clip_model_name=config.get('clip_model_name', None),
            online_texts=online_texts,
            use_open_clip=config.get('use_open_clip', False),
            viecap_config=config.get('viecap', None),
            regionclip_config=config.get('regionclip_config', None),
            invite_config=config.get('invite_config', None),
            denseclip_config=config.get('denseclip_config', None),
            alphaclip_config=config.get('alphaclip_config', None),
            clipcap_config=config.get('clipcap', None),
            hf_repo_id=config.get('hf_repo_id', None),
            dino_weights=config.get('dino_weights', None),
            memory_bank=config.get('memory_bank', None),
            memory_bank_texts=config.get('memory_bank_texts', None),
            synthetic_seed=config.get('synthetic_seed', None),
            max_batch=config.get('max_batch', 16),
            max_prefixes=config.get('max_prefixes', 128),       # what ONE greedy decode serves (the engine's limit)
            vit_dtype=config.get('vit_dtype', 'fp16'),
            clip_text_weights=config.get('clip_text_weights', None),
            clip_text_dtype=config.get('clip_text_dtype', 'fp16'),
            talk2dino_projection_weights=config.get('talk2dino_projection_weights', None),
            denseclip_config_dir=config.get('denseclip_config_dir', None),
            denseclip_checkpoint=config.get('denseclip_checkpoint', None),
            sparse_last_block=config.get('sparse_last_block', None),
            stop_at_eos=config.get('stop_at_eos', False),
            stop_segment=config.get('stop_segment', None),
        )
        model.to(device)
        return model

    def to(self, *args, **kwargs):
        """The weights live in the HIP library on the construction device: ``model.to(<that device>)`` (what the eval drivers
        do, eval_trace_captioning.py:185) returns self; any other device or a dtype change raises instead of silently
        leaving the model where it is."""
        device = kwargs.get("device")
        dtype = kwargs.get("dtype")
        for a in args:
            if isinstance(a, torch.dtype):
                dtype = a
            elif isinstance(a, (str, torch.device, int)):
                device = a
            elif isinstance(a, torch.Tensor):
                device, dtype = a.device, a.dtype
        if dtype is not None and dtype != torch.float32:
            raise RuntimeError("patchioner_amd: the model's precision is fixed when it is built (vit_dtype); .to(%s) is not supported" % dtype)
        if device is not None:
            d = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
            idx = d.index if d.index is not None else (torch.cuda.current_device() if d.type == "cuda" else None)
            if d.type != "cuda" or idx != self._device.index:
                raise RuntimeError("patchioner_amd: the model was built on %s and cannot move to %s; build it there with "
                                   "Patchioner.from_config(config, device=...)" % (self._device, d))
        return self

    # ------------------------------------------------------------------------------------------
    def forward(self, imgs,
                get_cls_capt=True,
                get_avg_self_attn_capt=False,
                get_attn_heads_capt=False,
                get_patch_capts=False,
                get_register_capts=False,
                bboxes=None,
                traces=None,
                get_controllable_capts=False,
                bs_factor=4,
                gaussian_avg=False,
                gaussian_bbox_variance=0.5,
                get_avg_patch_capt=False,
                gaussian_img_variance=1,
                use_attn_map_for_bboxes=False,
                use_attention_tracing=False,
                double_DINO_for_bboxes=False,
                double_DINO_for_bboxes_return_type="avg",
                double_DINO_use_cls=False,
                cleaning_type=None,
                clean_after_projection=True,
                alpha=1.0,
                clean_from="cls",
                caption_bboxes_type: str = None,
                return_n_best_sims=None,
                compute_scores: bool = False
                ):
        assert clean_from in ["cls", "avg_self_attn"]
        assert cleaning_type in [None, "orthogonal_projection", "contrastive_mask"]
        if double_DINO_for_bboxes and double_DINO_for_bboxes_return_type not in ("cls", "avg", "gaussian_avg"):
            raise ValueError("double_DINO_for_bboxes_return_type must be 'cls', 'avg' or 'gaussian_avg'")
        if cleaning_type is not None and self.im_proj is None:
            # the reference calls self.im_proj.project unconditionally here (model.py:900-913)
            raise AttributeError("cleaning_type needs the memory-bank projector (support_memory_size > 0)")
        if return_n_best_sims is not None and not self.calculate_argmax_text:
            # caption_tokens returns the similarities only on the calculate_argmax_text path (model.py:1408-1411); without
            # it the reference fails while unpacking (model.py:1030, 1036)
            raise ValueError("return_n_best_sims needs a model built with calculate_argmax_text")
        if self.backbone_type == 'AlphaClip' and bboxes is not None and double_DINO_for_bboxes:
            raise ValueError("double_DINO_for_bboxes is not supported with AlphaClip. AlphaClip processes regions differently.")
        if caption_bboxes_type is not None:
            return self.caption_bboxes(imgs, bboxes, caption_bboxes_type, compute_scores=compute_scores)
        if self.backbone_type == 'AlphaClip' and (bboxes is not None or traces is not None):
            # forward_alphaclip_with_regions (P/src/model.py:772-778, 1060-1354): a tower pass per region, the region keys only
            return self._forward_alphaclip_regions(imgs, bboxes, traces, get_controllable_capts, compute_scores, return_n_best_sims)

        eng = self.engine
        outs = {}
        bs = imgs.shape[0]
        # Traces and nothing else that reads the final tokens: only the patches the traces touch are needed, and the last block runs
        # on those rows alone (Engine.vit_forward_rows; the same bits as the dense forward, which stays the path of every other call).
        if (self.sparse_last_block and traces is not None and eng.sparse_ok and bs <= eng.max_batch
                and not (get_cls_capt or get_avg_self_attn_capt or get_attn_heads_capt or get_patch_capts or get_register_capts
                         or get_avg_patch_capt or bboxes is not None or use_attention_tracing or cleaning_type is not None)):
            grids, sel = eng.trace_grids(traces, select_rows=True)
            if sel is not None:
                tokens_c, row_map = eng.vit_forward_rows(imgs, sel)
                trace_embeds = eng.region_reduce_rows(tokens_c, row_map, grids.view(bs, -1), 1.0 / self.num_patch_tokens)
                outs['trace_capts'] = self.caption_tokens(trace_embeds)
                return outs
        # has_attention (model.py:864-865): only DINO backbones install the qkv hook.  Without it the reference never defines
        # self_attn / avg_self_attn_token / disentangled_self_attn and every option that reads them fails with
        # UnboundLocalError; clean_from == "avg_self_attn" falls back to the cls token (:886-890).
        has_attention = self._backbone.has_attention
        if double_DINO_for_bboxes and not has_attention:
            raise AttributeError("double_DINO_for_bboxes re-runs a DINOv2 block (bbox_utils.py:300-403): not a %s backbone" % self.backbone_type)
        tokens, qkv = eng.vit_forward(imgs, want_qkv=has_attention)
        G = self._G
        embed_dim = tokens.shape[-1]                 # model.py:924: the width of x_norm_patchtokens (512 behind the CLIP head)
        clean_avg = cleaning_type is not None and clean_from == "avg_self_attn" and has_attention
        if has_attention:
            self_attn, _, avg_self_attn_token, disentangled_self_attn = eng.cls_attention(
                qkv, tokens, want_maps=False, want_avg=get_avg_self_attn_capt or clean_avg, want_disentangled=get_attn_heads_capt)
        else:
            self_attn = avg_self_attn_token = disentangled_self_attn = None
            for flag, name in ((get_avg_self_attn_capt, "avg_self_attn_token"), (get_attn_heads_capt, "disentangled_self_attn"),
                               (use_attn_map_for_bboxes and bboxes is not None, "self_attn"),
                               (use_attention_tracing and traces is not None, "self_attn")):
                if flag:
                    raise UnboundLocalError("local variable %r referenced before assignment (the %s backbone has no "
                                            "attention hook, P/src/model.py:864-872)" % (name, self.backbone_type))
        if cleaning_type is not None:
            # P/src/model.py:879-922: every patch token goes through the memory-bank projection and ctx_cleaner (before
            # or after it); the cleaned, projected tokens REPLACE x_norm_patchtokens, and the patch / box captions
            # below skip their own projection.  (The reference's in-place normalisation of the tokens it hands to
            # project() is invisible afterwards: every later consumer projects, i.e. re-normalises, or uses the
            # replaced patch tokens.)
            n2 = self.num_patch_tokens
            patches = tokens[:, G:].contiguous()
            cf = avg_self_attn_token if clean_avg else tokens[:, 0].contiguous()
            if clean_after_projection:
                proj = eng.project_many(patches.view(-1, embed_dim), normalize=True).view(bs, n2, embed_dim)
                cleaned = eng.ctx_clean(proj, eng.project_many(cf.clone(), normalize=True), cleaning_type, alpha)
            else:
                cleaned = eng.ctx_clean(patches, cf, cleaning_type, alpha, normalize_inputs=True)
                cleaned = eng.project_many(cleaned.view(-1, embed_dim), normalize=True).view(bs, n2, embed_dim)
            tokens = torch.cat([tokens[:, :G], cleaned], dim=1)
        project_regions = cleaning_type is None

        def put(key, score_key, ret):
            if compute_scores is True:
                outs[key], outs[score_key] = ret
            else:
                outs[key] = ret

        if get_cls_capt:
            put('cls_capt', 'cls_capt_scores', self.caption_tokens(tokens[:, 0].contiguous(), compute_scores=compute_scores))
        if get_avg_self_attn_capt:
            put('avg_self_attn_capt', 'avg_self_attn_capt_scores',
                self.caption_tokens(avg_self_attn_token, compute_scores=compute_scores))
        if get_avg_patch_capt:
            put('avg_patch_capt', 'avg_patch_capt_scores',
                self.caption_tokens(self._region_means(tokens, gaussian_img_variance), compute_scores=compute_scores))
        if get_attn_heads_capt:
            ret = self.caption_tokens(disentangled_self_attn.view(-1, embed_dim), compute_scores=compute_scores)
            H = self.num_attn_heads
            caps = ret[0] if compute_scores is True else ret
            outs['attn_heads_capts'] = [caps[i * H:(i + 1) * H] for i in range(bs)]
            if compute_scores is True:
                outs['attn_heads_scores'] = [ret[1][i * H:(i + 1) * H] for i in range(bs)]
        if get_patch_capts:
            n_patches = self.num_patch_tokens
            ret = self.caption_tokens(tokens[:, G:].reshape(-1, embed_dim), project=project_regions, compute_scores=compute_scores)
            caps = ret[0] if compute_scores is True else ret
            outs['patch_tokens_capts'] = [caps[i * n_patches:(i + 1) * n_patches] for i in range(bs)]
            if compute_scores is True:
                outs['patch_tokens_scores'] = [ret[1][i * n_patches:(i + 1) * n_patches] for i in range(bs)]
        if get_register_capts:
            ret = self.caption_tokens(tokens[:, 1:G].reshape(-1, embed_dim), compute_scores=compute_scores)
            caps = ret[0] if compute_scores is True else ret
            outs['register_capts'] = [caps[i * 4:(i + 1) * 4] for i in range(bs)]
            if compute_scores is True:
                outs['register_scores'] = [ret[1][i * 4:(i + 1) * 4] for i in range(bs)]

        if bboxes is not None and not get_controllable_capts:
            bbox_bs = bs * bs_factor
            n_boxes = bboxes.shape[1]
            if double_DINO_for_bboxes:
                bbox_feats = self._bbox_feats_double_dino(tokens, bboxes, double_DINO_use_cls, double_DINO_for_bboxes_return_type,
                                                          gaussian_bbox_variance).view(-1, embed_dim)
            else:
                bbox_feats = self._bbox_feats(tokens, bboxes, gaussian_avg, gaussian_bbox_variance, False,
                                              self_attn if use_attn_map_for_bboxes else None).view(-1, embed_dim)
            # The reference captions the boxes in chunks of bbox_bs = bs * bs_factor (model.py:1000-1033), a memory
            # measure of its cache-less decode.  Projection and decode are row-independent, so ONE call gives the
            # same captions / scores; the engine splits at its own capacities (16 queries per bank pass, max_prefixes
            # per decode), e.g. 128 boxes decode as 2 x 64 instead of 4 x 32 prefixes.
            del bbox_bs
            ret = self.caption_tokens(bbox_feats, project=project_regions, return_n_best_sims=return_n_best_sims,
                                      compute_scores=compute_scores)
            if compute_scores is True:
                ret, scores = ret
                outs['bbox_scores'] = list(scores)
            if return_n_best_sims is not None:          # model.py:1023-1040: (captions, similarities) per chunk
                ret, sims = ret
                outs['bbox_sims'] = [list(sims)[i * n_boxes:(i + 1) * n_boxes] for i in range(bs)]
            outs['bbox_capts'] = [list(ret)[i * n_boxes:(i + 1) * n_boxes] for i in range(bs)]
            if compute_scores is True:
                outs['bbox_scores'] = [outs['bbox_scores'][i * n_boxes:(i + 1) * n_boxes] for i in range(bs)]
        elif bboxes is not None and get_controllable_capts:
            bbox_feats = self._bbox_feats(tokens, bboxes, gaussian_avg, gaussian_bbox_variance, True,
                                          self_attn if use_attn_map_for_bboxes else None)
            outs['set_controllable_capts'] = self.caption_tokens(bbox_feats)

        if traces is not None:
            # map_traces_to_grid + (grid * patches).mean((1,2))  (P/src/model.py:1049-1054): mean over n*n cells
            grids = eng.trace_grids(traces).view(bs, -1)
            if use_attention_tracing:
                grids = self_attn * grids
            trace_embeds = eng.region_reduce(tokens, grids, None, 1.0 / self.num_patch_tokens)
            outs['trace_capts'] = self.caption_tokens(trace_embeds)
        return outs

    # ------------------------------------------------------------------------------------------
    def _alphaclip_region_feats(self, imgs, regions):
        """Features of AlphaCLIP regions: ``regions`` = (image index, boxes [[x, y, w, h]], points [(x, y)]) per region.  Every region's
        pixel-level mask is rasterised in one launch, the tower runs over the regions in launches of max_batch sequences (each reads its
        image in place), and the feature is the CLS row (use_cls_for_localized_captions, the default) or the patch tokens averaged over
        the patch-level mask, sum(mask * patch) / (sum(mask) + 1e-8) (model.py:1096-1130)."""
        eng = self.engine
        R = len(regions)
        if R == 0:
            return torch.empty(0, self.token_dim, device=eng.device)
        tables = [(b, p) for _, b, p in regions]
        pix = eng.region_masks(tables, self.crop_dim, 1)
        idx = torch.tensor([i for i, _, _ in regions], dtype=torch.int32)
        use_cls = self.alphaclip_config.get('use_cls_for_localized_captions', True)
        cells = None if use_cls else eng.region_masks(tables, self.crop_dim // self.patch_size, self.patch_size).view(R, -1).float()
        feats = torch.empty(R, self.token_dim, device=eng.device, dtype=torch.float32)
        # one launch of max_batch regions at a time, each reduced to its features at once: the tokens held never exceed one launch's
        for s in range(0, R, eng.max_batch):
            e = min(R, s + eng.max_batch)
            tokens = eng.vit_forward_regions(imgs, idx[s:e], pix[s:e])
            if use_cls:
                feats[s:e] = tokens[:, 0]
            else:
                feats[s:e] = eng.region_reduce(tokens, cells[s:e], None, 1.0) / (cells[s:e].sum(dim=1, keepdim=True) + 1e-8)
        return feats

    def _forward_alphaclip_regions(self, imgs, bboxes, traces, get_controllable_capts, compute_scores, return_n_best_sims):
        """forward_alphaclip_with_regions (P/src/model.py:1060-1354) with the reference's per-region loop turned into one batch: all
        regions of the call are rasterised at once, the tower runs over them max_batch at a time, and one caption_tokens call captions
        them all; the results are re-nested as the reference returns them.  Masks follow alpha_mask_utils.py (boxes with an EXCLUSIVE
        end, the caller's ``bboxes`` untouched); a dummy box (components summing below 0) gets "" / 0.0 / [] and no pass."""
        bs = imgs.shape[0]
        rows = None
        if bboxes is not None:
            bt = bboxes if isinstance(bboxes, torch.Tensor) else torch.tensor(bboxes)
            bt = bt.detach().cpu()
            rows = [[(float(b.sum()) < 0, [float(v) for v in b.to(torch.float32).tolist()]) for b in bt[i]] for i in range(bs)]

        def points(trace):
            return [(p['x'], p['y']) for p in trace]

        if get_controllable_capts:
            regions = []
            for i in range(bs):
                boxes = [b for dummy, b in rows[i] if not dummy] if rows is not None else []
                pts = []
                if traces is not None:
                    # traces_to_alpha_mask(traces[i], grid) walks traces[i] as a list of TRACES (alpha_mask_utils.py): with the points of
                    # one trace there, map_traces_to_grid iterates a point's keys and fails on 'x'['x']
                    for tr in traces[i]:
                        if isinstance(tr, dict):
                            raise TypeError("string indices must be integers (traces_to_alpha_mask takes a list of traces per image)")
                        pts += points(tr)
                regions.append((i, boxes, pts))
            ret = self.caption_tokens(self._alphaclip_region_feats(imgs, regions), compute_scores=compute_scores)
            return {'set_controllable_capts': ret[0] if compute_scores else ret}

        regions, box_slot = [], []
        if rows is not None:
            for i in range(bs):
                for dummy, b in rows[i]:
                    box_slot.append(None if dummy else len(regions))
                    if not dummy:
                        regions.append((i, [b], []))
        n_box_regions = len(regions)
        if traces is not None:
            for i in range(bs):
                regions.append((i, [], points(traces[i])))
        feats = self._alphaclip_region_feats(imgs, regions)
        caps, scores, sims = [], [], None
        if return_n_best_sims is None:
            if len(regions):
                ret = self.caption_tokens(feats, compute_scores=compute_scores)
                caps, scores = (ret if compute_scores else (ret, None))
        else:
            # the box captions carry their similarities (model.py:1262-1271), the trace captions do not
            caps, scores, sims = [], [] if compute_scores else None, []
            if n_box_regions:
                ret = self.caption_tokens(feats[:n_box_regions].contiguous(), return_n_best_sims=return_n_best_sims, compute_scores=compute_scores)
                (c, sims), sc = ret if compute_scores else (ret, None)
                caps += list(c)
                if compute_scores:
                    scores += list(sc)
            if len(regions) > n_box_regions:
                ret = self.caption_tokens(feats[n_box_regions:].contiguous(), compute_scores=compute_scores)
                c, sc = ret if compute_scores else (ret, None)
                caps += list(c)
                if compute_scores:
                    scores += list(sc)
        outs = {}
        if rows is not None:
            nb = len(rows[0]) if bs else 0
            flat_caps = [caps[k] if k is not None else "" for k in box_slot]
            outs['bbox_capts'] = [flat_caps[i * nb:(i + 1) * nb] for i in range(bs)]
            if compute_scores:
                flat = [scores[k] if k is not None else 0.0 for k in box_slot]
                outs['bbox_scores'] = [flat[i * nb:(i + 1) * nb] for i in range(bs)]
            if return_n_best_sims is not None:
                flat = [sims[k] if k is not None else [] for k in box_slot]
                outs['bbox_sims'] = [flat[i * nb:(i + 1) * nb] for i in range(bs)]
        if traces is not None:
            outs['trace_capts'] = list(caps[n_box_regions:])
            if compute_scores:
                outs['trace_scores'] = list(scores[n_box_regions:])
        return outs

    def _region_means(self, tokens, variance):
        """compute_region_means (P/src/model.py:45-94)."""
        bs, eng = tokens.shape[0], self.engine
        n = eng.n
        if variance == 0:
            opts = [n // 2] if n % 2 == 1 else [n // 2 - 1, n // 2]
            wmap = torch.zeros(bs, n, n)
            for i in range(bs):
                cy = random.choice(opts)
                cx = random.choice(opts)
                wmap[i, cy, cx] = 1.0
            wmap = wmap.view(bs, -1).to(eng.device)
        else:
            wmap = eng.gaussian_map(variance).unsqueeze(0).expand(bs, -1).contiguous()
        return eng.region_reduce(tokens, wmap, None, 1.0)

    def _center_choices(self, boxes_i, single):
        """host draw of the var==0 centre cell, same RNG call order as bbox_utils.py:62-71"""
        n = self.engine.n
        B, NB = boxes_i.shape[:2]
        out = torch.zeros(B, NB, 2, dtype=torch.int32)

        def span(a, length):
            lo, hi = slice(a, a + length + 1).indices(n)[:2]
            return max(0, hi - lo)

        bl = boxes_i.tolist()
        for i in range(B):
            for j in range(NB):
                x1, y1, w, h = bl[i][j]
                if single and x1 + y1 + w + h < 0:
                    continue
                hs, ws = span(y1, h), span(x1, w)
                cy = [hs // 2] if hs % 2 == 1 else [hs // 2 - 1, hs // 2]
                cx = [ws // 2] if ws % 2 == 1 else [ws // 2 - 1, ws // 2]
                out[i, j, 0] = random.choice(cy)
                out[i, j, 1] = random.choice(cx)
        return out

    def _bbox_feats(self, tokens, bboxes, gaussian_avg, variance, single, attention_map):
        """extract_bboxes_feats (P/src/bbox_utils.py:8-109); `bboxes //= patch_size` mutates the caller's tensor."""
        eng = self.engine
        bboxes //= self.patch_size
        boxes_i = bboxes.int().cpu()
        B, NB = boxes_i.shape[:2]
        cc = None
        attn = None
        if attention_map is not None:
            mode = 3
            attn = attention_map.clone()        # the reference hands a .cpu() copy, so the original map survives
        elif gaussian_avg:
            if variance == 0:
                mode, cc = 2, self._center_choices(boxes_i, single)
            else:
                mode = 1
        else:
            mode = 0
        weights, single_map = eng.bbox_weights(boxes_i, mode, variance, cc, attn, single_map=single)
        if single:
            return eng.region_reduce(tokens, single_map, None, 1.0)
        idx = torch.arange(B, dtype=torch.int32).repeat_interleave(NB)
        return eng.region_reduce(tokens, weights, idx, 1.0).view(B, NB, self.token_dim)

    def _bbox_feats_double_dino(self, tokens, bboxes, use_cls, return_type, variance):
        """extract_bboxes_feats_double_dino (P/src/bbox_utils.py:300-403).  The reference floor-divides a CLONE of the
        xywh tensor by the patch size and reads it as (x1, y1, x2, y2) with inclusive python slices; the last block runs
        on [cls | registers | region patches] ("cls" / "avg": pio_bbox_double_dino); "gaussian_avg" weights the block's
        INPUT patches with a gaussian normalised to sum 1 and never needs the block."""
        if return_type == "cls" and not use_cls:
            raise AssertionError("return_type 'cls' needs double_DINO_use_cls")       # reference: assert return_type != "cls"
        idx = bboxes.clone()
        idx //= self.patch_size
        idx = idx.int().cpu()
        B, NB = idx.shape[:2]
        n = self.engine.n
        slices = torch.zeros(B, NB, 4, dtype=torch.int32)
        for i in range(B):
            for j in range(NB):
                x1, y1, x2, y2 = (int(v) for v in idx[i, j])
                ys, ye, _ = slice(y1, y2 + 1).indices(n)
                xs, xe, _ = slice(x1, x2 + 1).indices(n)
                slices[i, j] = torch.tensor([ys, max(ye, ys), xs, max(xe, xs)])
        if return_type != "gaussian_avg":
            return self.engine.bbox_double_dino(tokens, slices, use_cls, return_type)
        weights = torch.zeros(B * NB, n, n)
        for r, (ys, ye, xs, xe) in enumerate(slices.view(-1, 4).tolist()):
            h_span, w_span = ye - ys, xe - xs
            if h_span == 0 or w_span == 0:
                continue                                                              # empty region: sum of nothing = zeros
            yc, xc = torch.meshgrid(torch.linspace(-1, 1, h_span), torch.linspace(-1, 1, w_span), indexing="ij")
            w = torch.exp(-(xc ** 2 + yc ** 2) / variance)
            weights[r, ys:ye, xs:xe] = w / w.sum()
        img = torch.arange(B, dtype=torch.int32).repeat_interleave(NB)
        return self.engine.region_reduce(tokens, weights.to(tokens.device), img, 1.0).view(B, NB, self.embed_dim)

    # ------------------------------------------------------------------------------------------
    def preprocess_images(self, images, no_crop: bool = False):
        """Device-side ``torch.stack([self.image_transforms(im) for im in images]).to(device)`` (``no_crop``:
        ``image_transforms_no_crop``): same floats, computed on the GPU from the raw pixels (Engine.preprocess)."""
        return self.engine.preprocess(images, self.resize_dim, self.crop_dim, no_crop=no_crop)

    def caption_bboxes(self, imgs, bboxes, capt_type='cls_capt', crop_boxes=False, compute_scores=False):
        """P/src/model.py:1356-1390: crop each box from the PIL image, transform the crop (``image_transforms`` when
        ``crop_boxes`` else ``image_transforms_no_crop``) and caption it with a whole forward pass, ``bs`` crops at a time.
        process_bboxes (P/src/bbox_utils.py:406-421) runs the resampling on the host; here only PIL's crop (a copy of the
        pixels, its float box rounded by PIL as in the reference) stays there and resize / centre-crop / normalisation run
        on the GPU (pio_preprocess: the same floats as the PIL transform, tests/test_gpu_preprocess.py)."""
        bs = len(imgs)
        n_bboxes = bboxes.shape[1]
        regions = []
        for img, img_boxes in zip(imgs, bboxes.tolist()):
            for x_min, y_min, w, h in img_boxes:
                regions.append(img.crop((x_min, y_min, x_min + w, y_min + h)))
        crops = self.preprocess_images(regions, no_crop=not crop_boxes)
        capts, scores = [], []
        for i in range(n_bboxes):
            start = i * bs
            end = start + bs if i < n_bboxes - 1 else crops.shape[0]
            out = self.forward(crops[start:end], get_cls_capt=capt_type == 'cls_capt',
                               get_avg_self_attn_capt=capt_type == 'avg_self_attn_capt')
            capts += out[capt_type]
            if compute_scores:      # as in the reference: forward() is not asked for scores, so this key is missing (KeyError)
                scores += out[f"{capt_type}_scores"]
        ret = {'bbox_capts': [capts[i * n_bboxes:(i + 1) * n_bboxes] for i in range(bs)]}
        if compute_scores:
            ret['bbox_scores'] = [scores[i * n_bboxes:(i + 1) * n_bboxes] for i in range(bs)]
        return ret

    def caption_tokens(self, dino_tokens, project=True, return_n_best_sims=None, compute_scores: bool = False):
        """P/src/model.py:1392-1423."""
        eng = self.engine
        self.last_decode_steps = None
        if self.viecap is not None:
            if return_n_best_sims:
                raise Exception("return_n_best_sims is not supported with viecap")
            if self._defer:
                # forward_async: mapping, entity probabilities, hard prompt and the ragged decode (greedy) or the batched beam search
                # are enqueued; ids -> text in result()
                if compute_scores:
                    raise NotImplementedError("forward_async does not defer score lists; call forward() for compute_scores")
                if not self.viecap.args.using_greedy_search:
                    res = self.viecap.enqueue(dino_tokens)
                    self.last_ids = None              # as forward(): the beams of an image have their own lengths
                    return _PendingVieCapBeams(res, self.viecap)
                ids = self.viecap.enqueue(dino_tokens)
                self.last_ids = ids
                return _PendingVieCapCaptions(ids, self.viecap)
            out = self.viecap.forward(dino_tokens, compute_scores=compute_scores, stop_at_eos=self.stop_at_eos, stop_segment=self.stop_segment)
            self.last_ids = self.viecap.last_ids      # [N, 64] ids of the greedy search: what dist.sharded_* gathers
            self.last_decode_steps = self.viecap.last_decode_steps
            return out
        if self.clipcap is not None:
            if return_n_best_sims:
                raise Exception("return_n_best_sims is not supported with clipcap")
            if self._defer:
                # forward_async: the mapper and pio_lm_sample are enqueue-only; ids -> text in result()
                if compute_scores:
                    raise NotImplementedError("forward_async does not defer score lists; call forward() for compute_scores")
                ids = self.clipcap.enqueue(dino_tokens)
                self.last_ids = ids
                if ids is None:                        # entry_length 0: nothing to wait for
                    return [""] * int(dino_tokens.shape[0])
                return _PendingClipCapCaptions(ids, self.clipcap)
            out = self.clipcap.forward(dino_tokens, compute_scores=compute_scores)
            self.last_ids = self.clipcap.last_ids
            return out
        if self.im_proj is None:
            project = False
        x = dino_tokens
        if not isinstance(x, torch.Tensor):
            x = torch.tensor(x, dtype=torch.float)
        xd = x.to(device=eng.device, dtype=torch.float32).contiguous()
        if self.calculate_argmax_text:
            self.last_ids = None                       # no decoder on this path: nothing for dist.sharded_* to gather
            # model.py:1408-1411 -> im2txtprojection.py:367-375: the text of the most similar bank row, no decoder.  The row
            # index counts the rows kept at load while the texts are the file's unfiltered list (the reference's indexing).
            sims, rows = eng.topk_rows(xd, k=int(return_n_best_sims) if return_n_best_sims else 1)
            if isinstance(dino_tokens, torch.Tensor) and xd.data_ptr() != dino_tokens.data_ptr():
                dino_tokens.copy_(xd)           # normalised in place (im2txtprojection.py:368)
            captions = [self.text_dataset[int(r)].decode() for r in rows[:, 0].cpu().tolist()]
            if return_n_best_sims:
                captions = (captions, sims.cpu().tolist())
            return captions if compute_scores is False else (captions, [1.0] * len(captions))   # the reference's len(): 2 for a (texts, sims) pair
        if project:
            prefix = eng.project(xd, normalize=self.normalize)
            if isinstance(dino_tokens, torch.Tensor) and xd.data_ptr() != dino_tokens.data_ptr():
                dino_tokens.copy_(xd)           # quirk: the query is L2-normalised in place (im2txtprojection.py:368)
        else:
            prefix = xd
        if self.embed_inversion:
            prefix = eng.revert_transformation(prefix)
        if self.stop_at_eos and not self._defer and not compute_scores:
            # the score is exp of the sum of all 30 log-probabilities, so compute_scores takes the full decode
            ids, lp = eng.decode_greedy(prefix, steps=30, stop_id=self.tokenizer.eot_id, seg=self.stop_segment)
            self.last_decode_steps = list(eng.last_steps_run)
        else:
            ids, lp = eng.decode_greedy(prefix, steps=30, want_logprob=compute_scores)
        self.last_ids = ids
        if self.call_log is not None:
            self.call_log.append((prefix.detach().clone(), ids.detach().clone()))
        if self._defer:
            if compute_scores:
                raise NotImplementedError("forward_async does not defer score lists; call forward() for compute_scores")
            return _PendingCaptions(ids, self.tokenizer, self.decoding_method)
        outputs = self.tokenizer.batch_captions(ids.cpu().tolist(), decoding_method=self.decoding_method)
        if compute_scores:
            return outputs, torch.exp(lp.sum(dim=-1)).cpu().numpy().tolist()
        return outputs

    # ------------------------------------------------------------------------------------------
    def forward_async(self, imgs, stream: Optional["torch.cuda.Stream"] = None, **kwargs) -> "PendingForward":
        """Enqueue a whole forward on `stream` without waiting for the GPU: same arguments as ``forward`` (the
        flat caption outputs only: cls / avg_self_attn / avg_patch / trace / set_controllable captions), returns a
        handle whose ``result()`` gives exactly what ``forward`` would have returned.  Several model instances,
        each on its own stream, can keep several batches in flight (the decode of one batch is a chain of small
        latency-bound kernels that leaves most CUs idle, so it overlaps with the next batch's ViT)."""
        for k in ("bboxes", "get_attn_heads_capt", "get_patch_capts", "get_register_capts"):
            v = kwargs.get(k)
            if v is not None and v is not False:
                if not (k == "bboxes" and kwargs.get("get_controllable_capts")):
                    raise NotImplementedError("forward_async supports the flat caption outputs only (%s given)" % k)
        if self.backbone_type == 'AlphaClip' and (kwargs.get("bboxes") is not None or kwargs.get("traces") is not None):
            raise NotImplementedError("forward_async: AlphaCLIP region captions (a tower pass per region) run through forward() only")
        stream = stream or torch.cuda.current_stream()
        self._defer = True
        try:
            with torch.cuda.stream(stream):
                outs = self.forward(imgs, **kwargs)
                for v in outs.values():
                    if isinstance(v, _PendingCaptions):
                        v.start_copy()
                ev = torch.cuda.Event()
                ev.record(stream)
        finally:
            self._defer = False
        return PendingForward(outs, ev)

    def __len__(self):
        return self.engine.num_weights


class _PendingCaptions:
    """Greedy ids still on the device; resolved to the reference's list-of-strings on demand."""

    def __init__(self, ids_dev, tokenizer, decoding_method):
        self.ids_dev, self.tokenizer, self.decoding_method = ids_dev, tokenizer, decoding_method
        self.ids_host = None

    def start_copy(self):
        self.ids_host = torch.empty(self.ids_dev.shape, dtype=self.ids_dev.dtype).pin_memory()
        self.ids_host.copy_(self.ids_dev, non_blocking=True)

    def resolve(self):
        return self.tokenizer.batch_captions(self.ids_host.tolist(), decoding_method=self.decoding_method)


class _PendingVieCapCaptions(_PendingCaptions):
    """Greedy ids of the ViECap head still on the device; resolved as VieCapHead.forward would return them (a single row: a str)."""

    def __init__(self, ids_dev, head):
        super().__init__(ids_dev, None, None)
        self.head = head

    def resolve(self):
        return self.head.captions(self.ids_host.tolist())


class _PendingClipCapCaptions(_PendingCaptions):
    """Sampled ids of the ClipCap head still on the device; resolved as ClipCapHead.forward returns them (always a list)."""

    def __init__(self, ids_dev, head):
        super().__init__(ids_dev, None, None)
        self.head = head

    def resolve(self):
        return self.head.captions(self.ids_host.tolist())


class _PendingVieCapBeams(_PendingCaptions):
    """A beam head's (ids, lens, scores) still on the device; resolved as VieCapHead.forward returns them (a list, one text per image)."""

    def __init__(self, res, head):
        super().__init__(res[0], None, None)
        self.lens_dev, self.scores_dev, self.head = res[1], res[2], head

    def start_copy(self):
        super().start_copy()
        self.lens_host = torch.empty(self.lens_dev.shape, dtype=self.lens_dev.dtype).pin_memory()
        self.lens_host.copy_(self.lens_dev, non_blocking=True)
        self.scores_host = torch.empty(self.scores_dev.shape, dtype=self.scores_dev.dtype).pin_memory()
        self.scores_host.copy_(self.scores_dev, non_blocking=True)

    def resolve(self):
        return self.head.beam_captions(self.ids_host.tolist(), self.lens_host.tolist(), self.scores_host.tolist())


class PendingForward:
    def __init__(self, outs, event):
        self._outs, self._event = outs, event

    def done(self) -> bool:
        return self._event.query()

    def ids(self, key: str):
        """device tensor of the greedy ids behind output `key` (valid once result() or done())"""
        return self._outs[key].ids_dev

    def result(self) -> dict:
        self._event.synchronize()
        return {k: (v.resolve() if isinstance(v, _PendingCaptions) else v) for k, v in self._outs.items()}
