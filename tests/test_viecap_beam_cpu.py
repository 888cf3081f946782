"""The batched beam search of the ViECap head without a GPU: the C entry points are declared, typed and exported; a beam head is
accepted by the device path; the pipeline sizes its groups by the beam width and says so when asked for more."""
import os
import re
import subprocess

import pytest
import torch

import golden_cases as gc
from patchioner_amd import viecap as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pio_lm_beam_search", "pio_viecap_build_prompt_ragged")


def test_entry_points_in_header_signatures_and_library():
    from patchioner_amd import _lib, build
    build.build()
    with open(os.path.join(ROOT, "include", "patchioner_hip.h")) as f:
        header = f.read()
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "patchioner_amd", "libpatchioner_hip.so")],
                          capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\b" % name, syms), name
    assert len(_lib.SIGNATURES["pio_lm_beam_search"][1]) == 13
    assert len(_lib.SIGNATURES["pio_viecap_build_prompt_ragged"][1]) == 10


@pytest.fixture(scope="module")
def case():
    w, (vocab, merges), ents, emb, x = gc.viecap_case()
    return w, V.ByteLevelBPE(vocab, merges), ents, emb, x


class _FakeLib:
    def pio_viecap_prompt_length(self, h):
        return 10


class _FakeEngine:
    device = torch.device("cpu")
    max_steps = 256
    max_prefixes = 128
    lib = _FakeLib()
    h = None

    def viecap_set_entities(self, e):
        self.n = e.shape[0]


def _head(case, **over):
    w, tok, ents, emb, _ = case
    cfg = dict(clip_hidden_size=gc.VIECAP["C"], entities_text=ents, texts_embeddings=emb, tokenizer=tok, using_greedy_search=False,
               beam_width=5, using_hard_prompt=True, top_k=gc.VIECAP["top_k"])
    cfg.update(over)
    return V.VieCapHead(cfg, _FakeEngine(), "ViT-B/16")


def test_beam_head_passes_check_device_path(case):
    _head(case).check_device_path()
    _head(case, using_hard_prompt=False).check_device_path()
    with pytest.raises(ValueError):
        _head(case, top_k=9).check_device_path()            # what the greedy head refuses, the beam head refuses too


def test_beam_order_and_captions(case):
    head = _head(case)
    scores = [-1.5, -0.25, -0.25, -3.0]
    assert head.beam_order(scores) == torch.tensor(scores).argsort(descending=True).tolist()
    tok = head.tokenizer
    a, b = tok.encode(" a dog."), tok.encode(" two cats on a bed.")
    ids = [[a + [0] * 3, b + [7] * 2]]
    assert head.beam_captions(ids, [[len(a), len(b)]], [[-2.0, -1.0]]) == [tok.decode(b)]
    assert head.beam_captions(ids, [[len(a), len(b)]], [[-0.5, -1.0]]) == [tok.decode(a)]


class _FakeModel:
    def __init__(self, head, max_prefixes=128):
        class Eng:
            pass
        self.engine = Eng()
        self.engine.max_prefixes = max_prefixes
        self.viecap = head


def test_pipeline_group_sizing_errors(case):
    from patchioner_amd.pipeline import TraceCaptionPipeline
    head = _head(case)
    with pytest.raises(ValueError, match="beam_search=True"):
        TraceCaptionPipeline(_FakeModel(head))
    with pytest.raises(ValueError, match=r"min\(128, 128\) // 5 = 25 images"):
        TraceCaptionPipeline(_FakeModel(head), group_batches=26, beam_search=True)
    with pytest.raises(ValueError, match=r"min\(40, 128\) // 8 = 5 images"):
        TraceCaptionPipeline(_FakeModel(_head(case, beam_width=8), max_prefixes=40), group_batches=6, beam_search=True)
