"""ClipCap head of the reference (``ClipCapModel``, P/src/clipcap/entrypoint.py:398-579), host side.

``Patchioner.caption_tokens`` hands the region features to ``self.clipcap.forward`` (P/src/model.py:1399-1404).  Everything numerical
is a C-ABI call: the MLP prefix mapper (``pio_clipcap_mapping``), the prefill, and ``entry_length`` rounds of top-p sampling and
advance (``pio_lm_sample``: one captured graph, every flag on the device).  What stays on the host is the text: detokenising a row,
cutting it at the first stop character, scoring the captions again when asked.

The config is validated strictly, before anything touches the device, the weights or the tokenizer: a key this head does not
implement raises ``NotImplementedError`` naming it (the reference ignores unknown keys silently).  Nothing is fetched from the hub:
``weight_path`` is a local file (or ``weights`` a state dict), the tokenizer comes from ``tokenizer_path`` (vocab.json + merges.txt)
or is an object with ``encode`` / ``decode`` (``tokenizer``), as for the ViECap head.

The draw is not ``torch.multinomial``'s stream: the DISTRIBUTION of every step is the reference's (nucleus set and probabilities
inside it), the uniforms are Philox4x32-10 under ``seed`` (csrc/common.h), or the caller's (``forward(..., uniforms=)``).
"""
from __future__ import annotations

import os
from argparse import Namespace
from typing import Dict, List, Optional

import torch

DEFAULTS = {  # ClipCapModel.defaults (entrypoint.py:438-452)
    "language_model": "gpt2", "prefix_length": 10, "clip_length": 10, "num_layers": 8, "mapping_type": "mlp", "only_prefix": True,
    "temperature": 1.0, "top_p": 0.8, "entry_length": 67, "stop_token": ".", "use_batched_generation": True, "normalize_prefix": False,
    "weight_path": "/raid/datasets/models_weights/clipcap/training-features/clipcap_dino_vitb14_len10_mlp.pt",
}
# the reference's own keys, its hub keys (accepted, never used: nothing is downloaded) and this build's local-path additions
IMPLEMENTED_KEYS = tuple(DEFAULTS) + ("hf_repo_id", "weight_path_hf_repo_id", "seed", "tokenizer", "tokenizer_path", "weights")


def validate_config(cfg: dict) -> dict:
    """The config with the reference's defaults filled in (a copy).  Pure: no device, file or tokenizer access."""
    if not isinstance(cfg, dict):
        raise TypeError("clipcap config must be a dict")
    for k in cfg:
        if k not in IMPLEMENTED_KEYS:
            raise NotImplementedError("clipcap config key %r is not implemented by this head (implemented: %s)" % (k, ", ".join(IMPLEMENTED_KEYS)))
    out = dict(cfg)
    for k, v in DEFAULTS.items():
        out.setdefault(k, v)
    out.setdefault("seed", 0)
    if out["mapping_type"] != "mlp":
        raise NotImplementedError("clipcap mapping_type %r: only the MLP mapper is built (the transformer mapper is ViECap's MappingNetwork "
                                  "without its in-place normalisation: a follow-up)" % (out["mapping_type"],))
    if "gpt" not in str(out["language_model"]):
        raise NotImplementedError("clipcap language_model %r: GPT-2 only" % (out["language_model"],))
    if int(out["entry_length"]) < 0:
        raise ValueError("clipcap entry_length must be >= 0")
    if not isinstance(out["stop_token"], str) or not out["stop_token"]:
        raise ValueError("clipcap stop_token must be a non-empty string")
    return out


def cut_caption(text: str, stop_token: str) -> str:
    """generate_batched's clean-up (entrypoint.py:303-305): the text up to the first stop CHARACTER (which may sit inside an earlier
    token than the stop token itself), plus the stop token."""
    return text.split(stop_token)[0] + stop_token


def captions_from_ids(tokenizer, rows: List[List[int]], stop_token: str) -> List[str]:
    """Rows of ``entry_length`` ids -> captions, over all ids of a row as the reference decodes them; no ids (entry_length 0): ''."""
    return [cut_caption(tokenizer.decode(list(r)), stop_token) if len(r) else "" for r in rows]


def load_clipcap_weights(cfg: dict) -> Dict[str, torch.Tensor]:
    sd = cfg.get("weights")
    if sd is None:
        path = cfg.get("weight_path", DEFAULTS["weight_path"])
        if not isinstance(path, str) or not os.path.exists(path):
            raise FileNotFoundError("ClipCap checkpoint %r not found (weight_path is a local file here: nothing is downloaded)" % (path,))
        sd = torch.load(path, map_location="cpu")
    return sd


def resolve_tokenizer(cfg: dict):
    tok = cfg.get("tokenizer")
    if tok is None:
        path = cfg.get("tokenizer_path")
        if not path or not os.path.exists(os.path.join(path, "vocab.json")) or not os.path.exists(os.path.join(path, "merges.txt")):
            raise FileNotFoundError("clipcap.tokenizer_path (a directory with GPT-2's vocab.json and merges.txt) is required: "
                                    "GPT2Tokenizer.from_pretrained('gpt2') needs network, which this target does not have (%r)" % (path,))
        from .viecap import ByteLevelBPE
        tok = ByteLevelBPE.from_files(path)
    return tok


class ClipCapHead:
    """Mirror of ``ClipCapModel`` (entrypoint.py:398): ``forward(dino_features, compute_scores)`` -> captions."""

    def __init__(self, args: dict, engine, tokenizer=None):
        self.cfg = validate_config(args)
        self.args = Namespace(**{k: v for k, v in self.cfg.items() if k not in ("tokenizer", "weights")})
        self.engine = engine
        self.device = engine.device
        self.tokenizer = tokenizer if tokenizer is not None else resolve_tokenizer(self.cfg)
        self.stop_token_index = int(self.tokenizer.encode(self.args.stop_token)[0])
        self.prefix_length = int(engine.lib.pio_clipcap_prefix_length(engine.h))
        if self.prefix_length != int(self.args.prefix_length):
            raise ValueError("clipcap prefix_length %d, the checkpoint's mapper gives %d" % (int(self.args.prefix_length), self.prefix_length))
        if self.prefix_length + int(self.args.entry_length) - 1 > engine.max_steps:
            raise ValueError("clipcap prefix_length + entry_length - 1 above the engine's %d positions" % engine.max_steps)
        self.last_ids = None

    @property
    def steps(self) -> int:
        return int(self.args.entry_length)

    def enqueue(self, feats: torch.Tensor, uniforms: Optional[torch.Tensor] = None, decoder=None):
        """Mapper, prefill and the sampling loop, enqueue-only -> ids [N, entry_length] int32 on the device (None at entry_length 0).
        ``decoder``: a DecoderClone to run the language model on (the mapper stays on the engine)."""
        a, eng = self.args, self.engine
        if not isinstance(feats, torch.Tensor):
            feats = torch.tensor(feats, dtype=torch.float)
        if self.steps == 0:
            self.last_ids = None
            return None
        prefix = eng.clipcap_mapping(feats, normalize=bool(a.normalize_prefix))
        ids, _ = (decoder or eng).lm_sample(prefix, self.steps, float(a.temperature), float(a.top_p), self.stop_token_index,
                                            seed=int(a.seed), uniforms=uniforms,
                                            rows_per_call=None if a.use_batched_generation else 1)
        self.last_ids = ids
        return ids

    def captions(self, rows: List[List[int]]) -> List[str]:
        return captions_from_ids(self.tokenizer, rows, self.args.stop_token)

    def forward(self, dino_features: torch.Tensor, compute_scores: bool = False, uniforms: Optional[torch.Tensor] = None):
        """entrypoint.py:471-552.  ``use_batched_generation: false`` runs the same device path one row per call (generate2 and
        generate_batched are the same distribution)."""
        N = int(dino_features.shape[0])
        ids = self.enqueue(dino_features, uniforms=uniforms)
        out = self.captions(ids.cpu().tolist()) if ids is not None else [""] * N
        if compute_scores:
            return out, self.compute_perplexity_scores(out)
        return out

    def compute_perplexity_scores(self, captions: List[str]) -> List[float]:
        """entrypoint.py:554-579: 1 / exp(mean next-token loss) of every caption tokenised again; 1.0 where the reference's bare
        ``except`` would give it (a caption of fewer than two tokens has no loss; a token outside the vocabulary)."""
        import math
        rows = [list(self.tokenizer.encode(c)) for c in captions]
        V = int(self.engine.cfg.dec_vocab)
        ok = [i for i, r in enumerate(rows) if len(r) >= 2 and len(r) <= self.engine.max_steps and all(0 <= int(t) < V for t in r)]
        scores = [1.0] * len(rows)
        if ok:
            nll = self.engine.lm_score([rows[i] for i in ok]).cpu().tolist()
            for i, s in zip(ok, nll):
                loss = s / (len(rows[i]) - 1)
                if math.isnan(loss):
                    continue
                ppl = math.exp(loss) if loss < 700 else math.inf
                scores[i] = 1.0 / ppl if ppl > 0 else 1.0
        return scores
