"""The CLIP text side on the MI355X: BPE encoder (host) and the text tower (``libpatchioner_hip``, csrc/text_encoder.hip).

What the reference does with the ``clip`` package -- ``clip.tokenize(texts)`` and ``clip_model.encode_text(ids)``
(P/src/decap/im2txtprojection/im2txtprojection.py:511-524, 650-657; the online_texts path :491-493) -- this module does
without it:

* ``ClipTokenizer.encode`` / ``tokenize``: the byte-level BPE of OpenAI CLIP with ``clip.tokenize``'s row layout
  ([49406] + ids + [49407], zero padded to 77, ``RuntimeError`` above 77 unless ``truncate``).  Merge r of the BPE joins two
  vocabulary entries into entry 512 + r; vocabulary strings are unique, so the merge is fixed by WHERE entry 512 + r's bytes
  split.  ``assets/clip_bpe_merge_splits.txt`` (plain text, produced by ``tools/oracle/gen_golden_clip_text.py`` from the BPE
  vocabulary file) lists that byte offset for every merge; the bytes of every entry come from the detokeniser's table
  (``assets/clip_bpe_decode_table.npz``).
* ``ClipTextEncoder``: the 12-layer causal text transformer, fp16 MFMA operands (fp32 accumulate and residual stream) or
  exact fp32 (parity mode), from a ``clip.load`` JIT archive, a state dict or seeded synthetic weights.
"""
from __future__ import annotations

import ctypes
import html
import os
import unicodedata
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .tokenizer import ClipDetokenizer

_ASSETS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets")
MERGES_ASSET = os.path.join(_ASSETS, "clip_bpe_merge_splits.txt")

SOT_ID = 49406
EOT_ID = 49407
_SPECIALS = {"<|startoftext|>": SOT_ID, "<|endoftext|>": EOT_ID}
_CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")

# ----------------------------------------------------------------------------------------------------------------------
# text cleaning
# ----------------------------------------------------------------------------------------------------------------------
_QUOTES = str.maketrans({"‘": "'", "’": "'", "‚": "'", "‛": "'",
                         "“": '"', "”": '"', "„": '"', "‟": '"'})


def fix_text(text: str) -> str:
    """The parts of ``ftfy.fix_text`` (which the reference calls first) that act on WELL-FORMED text: NFC normalisation and
    curly quotes to straight ones (ftfy's ``uncurl_quotes``).  Mojibake repair (text decoded with the wrong codec), terminal
    escapes, ligature and full-width fixes are out of scope: for such input the ids may differ from the reference's."""
    return unicodedata.normalize("NFC", text).translate(_QUOTES)


def _is_space(ch: str) -> bool:
    # the `regex` module's \\s in Unicode mode: str.isspace without the information separators U+001C..U+001F
    return ch.isspace() and not ("\x1c" <= ch <= "\x1f")


def _is_letter(ch: str) -> bool:
    return unicodedata.category(ch)[0] == "L"


def _is_number(ch: str) -> bool:
    return unicodedata.category(ch)[0] == "N"


def clean(text: str) -> str:
    """basic_clean + whitespace_clean + lower(): fix_text, html-unescape twice, strip; whitespace runs -> one space."""
    text = html.unescape(html.unescape(fix_text(text))).strip()
    out, prev_space = [], False
    for ch in text:
        if _is_space(ch):
            if not prev_space:
                out.append(" ")
            prev_space = True
        else:
            out.append(ch)
            prev_space = False
    return "".join(out).strip().lower()


def pre_tokenize(text: str) -> List[str]:
    """The split of CLIP's tokenizer, as a scanner: at each position the first of <|startoftext|> / <|endoftext|>, a
    contraction ('s 't 're 've 'm 'll 'd), a run of letters, ONE number character, or a run of characters that are neither
    whitespace, letters nor numbers; whitespace between tokens is skipped.  Letters / numbers are the Unicode categories L* /
    N* of Python's ``unicodedata``."""
    toks, i, n = [], 0, len(text)
    while i < n:
        ch = text[i]
        if _is_space(ch):
            i += 1
            continue
        hit = next((s for s in _SPECIALS if text.startswith(s, i)), None)
        if hit is None and ch == "'":
            hit = next((s for s in _CONTRACTIONS if text.startswith(s, i)), None)
        if hit is not None:
            toks.append(hit)
            i += len(hit)
            continue
        j = i + 1
        if _is_letter(ch):
            while j < n and _is_letter(text[j]):
                j += 1
        elif not _is_number(ch):
            while j < n and not (_is_space(text[j]) or _is_letter(text[j]) or _is_number(text[j])):
                j += 1
        toks.append(text[i:j])
        i = j
    return toks


# ----------------------------------------------------------------------------------------------------------------------
# BPE
# ----------------------------------------------------------------------------------------------------------------------
def read_merge_splits(path: str) -> List[int]:
    """The split offsets of the asset: whitespace-separated decimal integers, '#' starts a comment line."""
    with open(path, "r", encoding="ascii") as f:
        return [int(v) for line in f if not line.startswith("#") for v in line.split()]


def merges_from_splits(table: Sequence[bytes], splits: Sequence[int]) -> np.ndarray:
    """[len(splits), 2] vocabulary ids: merge r joins table[512 + r][:p] and table[512 + r][p:] (p = splits[r]), both entries
    that exist before it."""
    index = {b: i for i, b in enumerate(table)}
    if len(index) != len(table):
        raise ValueError("vocabulary entries are not unique")
    merges = np.zeros((len(splits), 2), np.int64)
    for r, p in enumerate(splits):
        s = table[512 + r]
        a, b = index.get(s[:p]), index.get(s[p:])
        if not 0 < p < len(s) or a is None or b is None or max(a, b) >= 512 + r:
            raise ValueError("merge %d: split %d of %r is not a pair of earlier vocabulary entries" % (r, p, s))
        merges[r] = a, b
    return merges


class ClipTokenizer:
    """``encode(text) -> list[int]`` and ``tokenize(texts, context_length=77, truncate=False) -> LongTensor [N, 77]`` with the
    semantics of ``clip.tokenize``.  Words already seen are cached."""

    def __init__(self, merges_path: Optional[str] = None, table_path: Optional[str] = None):
        self.detok = ClipDetokenizer(table_path)
        table = self.detok.table
        merges = merges_from_splits(table, read_merge_splits(merges_path or MERGES_ASSET))
        self.vocab_size = len(table)
        if 512 + len(merges) + 2 != self.vocab_size:
            raise ValueError("%d merges do not match a %d-entry vocabulary" % (len(merges), self.vocab_size))
        # ids 0..255: one byte each; 256..511: the same bytes ending a word (the "</w>" forms)
        self.byte_id = [0] * 256
        for i in range(256):
            if len(table[i]) != 1 or table[i + 256] != table[i] + b"</w>":
                raise ValueError("vocabulary entry %d is not a single byte" % i)
            self.byte_id[table[i][0]] = i
        self.ranks: Dict[tuple, int] = {(int(a), int(b)): r for r, (a, b) in enumerate(merges)}
        self.cache: Dict[str, List[int]] = {}

    def bpe(self, word: str) -> List[int]:
        """Ids of one pre-token: its UTF-8 bytes, the last one in its end-of-word form, merged by ascending rank."""
        hit = self.cache.get(word)
        if hit is not None:
            return hit
        if word in _SPECIALS:
            return [_SPECIALS[word]]
        ids = [self.byte_id[b] for b in word.encode("utf-8")]
        ids[-1] += 256
        ranks = self.ranks
        while len(ids) > 1:
            best, best_rank = None, None
            for p in zip(ids, ids[1:]):
                r = ranks.get(p)
                if r is not None and (best_rank is None or r < best_rank):
                    best, best_rank = p, r
            if best is None:
                break
            a, b = best
            new, i, n = [], 0, len(ids)
            while i < n:
                if i + 1 < n and ids[i] == a and ids[i + 1] == b:
                    new.append(512 + best_rank)
                    i += 2
                else:
                    new.append(ids[i])
                    i += 1
            ids = new
        self.cache[word] = ids
        return ids

    def encode(self, text: str) -> List[int]:
        out: List[int] = []
        for tok in pre_tokenize(clean(text)):
            out.extend(self.bpe(tok))
        return out

    def decode(self, ids: Sequence[int]) -> str:
        return self.detok.decode(ids)

    def tokenize(self, texts: Union[str, Sequence[str]], context_length: int = 77, truncate: bool = False) -> torch.Tensor:
        if isinstance(texts, str):
            texts = [texts]
        out = torch.zeros(len(texts), context_length, dtype=torch.long)
        for i, t in enumerate(texts):
            row = [SOT_ID] + self.encode(t) + [EOT_ID]
            if len(row) > context_length:
                if not truncate:
                    raise RuntimeError("Input %s is too long for context length %d" % (t, context_length))
                row = row[:context_length]
                row[-1] = EOT_ID
            out[i, :len(row)] = torch.tensor(row, dtype=torch.long)
        return out


_TOKENIZER: Optional[ClipTokenizer] = None


def default_tokenizer() -> ClipTokenizer:
    global _TOKENIZER
    if _TOKENIZER is None:
        _TOKENIZER = ClipTokenizer()
    return _TOKENIZER


def tokenize(texts, context_length: int = 77, truncate: bool = False) -> torch.Tensor:
    """``clip.tokenize`` (returns int64)."""
    return default_tokenizer().tokenize(texts, context_length, truncate)


# ----------------------------------------------------------------------------------------------------------------------
# weights
# ----------------------------------------------------------------------------------------------------------------------
_NON_TEXT_SCALARS = {"logit_scale", "input_resolution", "context_length", "vocab_size"}


def text_state_dict(sd) -> Dict[str, torch.Tensor]:
    """The text tower's tensors of a full CLIP state dict (``clip.load(...)[0].state_dict()`` or the JIT archive's), fp32.
    ``visual.*`` and the model's scalar attributes are ignored; every other key is handed to the library, which refuses names it
    does not know."""
    return {k: v.detach().float().contiguous() for k, v in sd.items()
            if not k.startswith("visual.") and k not in _NON_TEXT_SCALARS}


def clip_cache_path(name: str) -> str:
    """Where ``clip.load(name)`` stores its archive: ~/.cache/clip/<name with "/" and "@" -> "-">.pt (ViT-L/14@336px ->
    ViT-L-14-336px.pt, the basename of its download URL)."""
    return os.path.join(os.path.expanduser("~/.cache/clip"), name.replace("/", "-").replace("@", "-") + ".pt")


def load_clip_archive(path: str) -> Dict[str, torch.Tensor]:
    """A ``clip.load`` JIT archive (``torch.jit.load(path).state_dict()``: needs no ``clip`` package) or a saved state dict."""
    try:
        return dict(torch.jit.load(path, map_location="cpu").state_dict())
    except RuntimeError:
        sd = torch.load(path, map_location="cpu", weights_only=True)
        return dict(sd.state_dict() if hasattr(sd, "state_dict") else sd)


def resolve_text_weights(name: str, clip_text_weights=None, synthetic_seed: Optional[int] = None,
                         layers: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """Weight sources in order: ``clip_text_weights`` (a path or a state dict), ``~/.cache/clip/<name>.pt``,
    ``weights.synth_clip_text(synthetic_seed, name)``; otherwise ``FileNotFoundError``."""
    from . import weights as W
    W.clip_text_arch(name)                    # ValueError for an unknown name
    if clip_text_weights is not None:
        return text_state_dict(clip_text_weights if isinstance(clip_text_weights, dict) else load_clip_archive(clip_text_weights))
    cached = clip_cache_path(name)
    if os.path.exists(cached):
        return text_state_dict(load_clip_archive(cached))
    if synthetic_seed is not None:
        return W.synth_clip_text(int(synthetic_seed), name, layers=layers)
    raise FileNotFoundError("no CLIP text weights for %s: pass clip_text_weights, put the clip.load archive at %s, or set "
                            "synthetic_seed" % (name, cached))


# ----------------------------------------------------------------------------------------------------------------------
# the tower
# ----------------------------------------------------------------------------------------------------------------------
OPERAND_TYPES = {"fp16": 0, "fp32": 2}


class ClipTextEncoder:
    """``encode_text(list[str] | LongTensor [N, L]) -> [N, embed_dim]`` fp32 on the device, in input order.

    Captions are sorted by token count and encoded in buckets of at most ``max_texts``, each padded to its longest caption:
    a caption's feature has the same bits in any bucket (csrc/text_encoder.hip, invariance).  ``close()`` frees the device
    memory; the object is unusable afterwards."""

    def __init__(self, name: str = "ViT-B/16", weights=None, synthetic_seed: Optional[int] = None, operand_type: str = "fp16",
                 device: Union[str, torch.device] = "cuda:0", max_texts: int = 1024, layers: Optional[int] = None,
                 tokenizer: Optional[ClipTokenizer] = None):
        from . import weights as W
        width, full_layers, heads, embed = W.clip_text_arch(name)
        if operand_type not in OPERAND_TYPES:
            raise ValueError("operand_type must be one of %s" % sorted(OPERAND_TYPES))
        sd = resolve_text_weights(name, weights, synthetic_seed, layers)
        n_layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer.resblocks."))
        ctx, vocab = sd["positional_embedding"].shape[0], sd["token_embedding.weight"].shape[0]
        self.name, self.width, self.embed_dim, self.context_length = name, width, embed, ctx
        self.device = torch.device(device)
        self.max_texts = int(max_texts)
        self.tokenizer = tokenizer
        self._lib = _lib.load()
        cfg = _lib.PioTextConfig(device=self.device.index or 0, width=width, layers=n_layers, heads=heads, context_length=ctx,
                                 vocab_size=vocab, embed_dim=embed, max_texts=self.max_texts,
                                 operand_type=OPERAND_TYPES[operand_type])
        h = ctypes.c_void_p()
        _lib.check(self._lib.pio_text_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        try:
            for k, v in sd.items():
                shape = (ctypes.c_int64 * v.dim())(*v.shape)
                _lib.check(self._lib.pio_text_load_weight(self._h, k.encode(), v.data_ptr(), shape, v.dim()))
            _lib.check(self._lib.pio_text_finalize(self._h))
        except Exception:
            self.close()
            raise

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.pio_text_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encode_ids_raw(self, ids: torch.Tensor) -> torch.Tensor:
        """One launch: ids [N, L] (N <= max_texts, L <= context_length) as they are -> [N, embed_dim]."""
        if self._h is None:
            raise RuntimeError("ClipTextEncoder is closed")
        ids = ids.to(device=self.device, dtype=torch.int32).contiguous()
        out = torch.empty(ids.shape[0], self.embed_dim, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self._lib.pio_text_encode(self._h, ids.data_ptr(), ids.shape[0], ids.shape[1], out.data_ptr(), stream))
        return out

    def encode_text(self, texts) -> torch.Tensor:
        if isinstance(texts, torch.Tensor):
            ids = texts.detach().cpu().long()
            if ids.dim() != 2:
                raise ValueError("token ids must be [N, L]")
        else:
            tok = self.tokenizer or default_tokenizer()
            ids = tok.tokenize(list(texts), self.context_length)
        n = ids.shape[0]
        out = torch.empty(n, self.embed_dim, device=self.device, dtype=torch.float32)
        if n == 0:
            return out
        lens = ids.argmax(dim=1) + 1                               # through EOT (the first maximum)
        order = torch.argsort(lens, stable=True)
        for s in range(0, n, self.max_texts):
            idx = order[s:s + self.max_texts]
            L = int(lens[idx].max())
            out[idx.to(self.device)] = self.encode_ids_raw(ids[idx, :L])
        return out

    __call__ = encode_text
