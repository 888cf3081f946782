"""The CLIP text side without a GPU: the BPE encoder against the reference tokenizer's own ids, clip.tokenize's row rules,
the state-dict key map, synthetic shapes, and the argument checks of online_texts / use_open_clip up to the device."""
import json
import os

import numpy as np
import pytest
import torch

from patchioner_amd import clip_text as CT
from patchioner_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tok():
    return CT.ClipTokenizer()


def _fixture(golden):
    z = golden("clip_tokenize")
    sents = json.loads(z["strings_json"].tobytes())
    offs, ids = z["offsets"], z["ids"]
    return sents, [ids[offs[i]:offs[i + 1]].tolist() for i in range(len(sents))]


def test_encode_matches_reference_tokenizer_fixture(golden, tok):
    """tools/oracle/gen_golden_clip_text.py: SimpleTokenizer.encode of ~200 sentences (captions, punctuation, contractions,
    digits, non-ASCII letters, empty strings, the 77-token boundary)."""
    sents, want = _fixture(golden)
    assert len(sents) >= 190
    bad = [(s, w, tok.encode(s)) for s, w in zip(sents, want) if tok.encode(s) != w]
    assert not bad, bad[:5]


def test_tokenize_rows_match_the_fixture_layout(golden, tok):
    sents, want = _fixture(golden)
    short = [(s, w) for s, w in zip(sents, want) if len(w) <= 75]
    rows = tok.tokenize([s for s, _ in short])
    assert rows.dtype == torch.long and rows.shape == (len(short), 77)
    for r, (_, w) in zip(rows.tolist(), short):
        assert r == [49406] + w + [49407] + [0] * (75 - len(w))


def test_context_boundary_77_accepted_78_raises_truncate_keeps_eot(tok):
    r = tok.tokenize(" ".join(["dog"] * 75))
    assert r.shape == (1, 77) and r[0, 0] == 49406 and r[0, 76] == 49407 and (r[0] > 0).all()
    with pytest.raises(RuntimeError, match="too long for context length 77"):
        tok.tokenize(" ".join(["dog"] * 76))
    t = tok.tokenize([" ".join(["dog"] * 76), "a cat"], truncate=True)
    assert t[0, 76] == 49407 and t[0, 0] == 49406 and t[0, 75] == t[0, 1]
    assert t[1].tolist()[:4] == [49406] + tok.encode("a cat") + [49407]
    assert tok.tokenize("", context_length=2).tolist() == [[49406, 49407]]


def test_decoding_returns_the_text(tok):
    for s in ["a dog sitting on a red couch.", "two zebras, standing!", "café crème 123", "it's a cat's toy"]:
        assert tok.decode(tok.encode(s)).strip() == " ".join(CT.pre_tokenize(CT.clean(s)))
    assert tok.decode(tok.encode("a man riding a horse")) == "a man riding a horse "


def test_cleaning_rules():
    assert CT.fix_text("“quoted” it’s") == "\"quoted\" it's"
    assert CT.fix_text("café") == "café"                      # NFC
    assert CT.clean("  Fish &amp;amp; Chips\t\n&lt;b&gt;  ") == "fish & chips <b>"
    assert CT.clean("A B　C") == "a b c"
    assert CT.pre_tokenize("it's a <|endoftext|>x 12ab!?") == ["it", "'s", "a", "<|endoftext|>", "x", "1", "2", "ab", "!?"]


def test_tokenizer_caches_words(tok):
    tok.encode("hippopotamus hippopotamus")
    assert "hippopotamus" in tok.cache


def test_merges_asset_is_consistent(tok):
    """The text asset (split offsets) rebuilds 48 894 merges, each joining two EARLIER vocabulary entries into entry 512 + r."""
    with open(CT.MERGES_ASSET, "rb") as f:
        raw = f.read()
    assert raw.isascii() and b"\0" not in raw
    splits = CT.read_merge_splits(CT.MERGES_ASSET)
    table = tok.detok.table
    m = CT.merges_from_splits(table, splits)
    assert m.shape == (48894, 2)
    assert (m >= 0).all() and (m < 512 + np.arange(len(m))[:, None]).all()
    for r in (0, 1, 100, 48893):
        assert table[512 + r] == table[m[r, 0]] + table[m[r, 1]]
    bad = list(splits)
    bad[5] = len(table[517])                                   # no right part
    with pytest.raises(ValueError, match="merge 5"):
        CT.merges_from_splits(table, bad)


@pytest.mark.parametrize("name,width,heads,embed", [("ViT-B/16", 512, 8, 512), ("ViT-L/14", 768, 12, 768)])
def test_synth_clip_text_shapes_and_key_map(name, width, heads, embed):
    w = W.synth_clip_text(3, name, layers=2)
    assert W.clip_text_arch(name) == (width, 12, heads, embed)
    assert w["token_embedding.weight"].shape == (49408, width)
    assert w["positional_embedding"].shape == (77, width)
    assert w["text_projection"].shape == (width, embed)
    p = "transformer.resblocks.1."
    assert w[p + "attn.in_proj_weight"].shape == (3 * width, width) and w[p + "attn.in_proj_bias"].shape == (3 * width,)
    assert w[p + "attn.out_proj.weight"].shape == (width, width)
    assert w[p + "mlp.c_fc.weight"].shape == (4 * width, width) and w[p + "mlp.c_proj.weight"].shape == (width, 4 * width)
    assert not any(k.startswith("transformer.resblocks.2.") for k in w)
    full = dict(w)
    full.update({"visual.conv1.weight": torch.zeros(4), "visual.proj": torch.zeros(2), "logit_scale": torch.tensor(4.6),
                 "input_resolution": torch.tensor(224), "context_length": torch.tensor(77), "vocab_size": torch.tensor(49408)})
    full["token_embedding.weight"] = full["token_embedding.weight"].half()
    sd = CT.text_state_dict(full)
    assert set(sd) == set(w)
    assert all(v.dtype == torch.float32 and v.is_contiguous() for v in sd.values())


def test_weight_sources_order(tmp_path, monkeypatch):
    monkeypatch.setenv("HOME", str(tmp_path))
    with pytest.raises(ValueError, match="unsupported CLIP model name"):
        CT.resolve_text_weights("RN50")
    with pytest.raises(FileNotFoundError, match="no CLIP text weights"):
        CT.resolve_text_weights("ViT-B/32")
    assert CT.clip_cache_path("ViT-L/14@336px").endswith(os.path.join(".cache", "clip", "ViT-L-14-336px.pt"))
    synth = CT.resolve_text_weights("ViT-B/32", synthetic_seed=4, layers=1)
    assert torch.equal(synth["text_projection"], W.synth_clip_text(4, "ViT-B/32", layers=1)["text_projection"])
    # the clip.load cache wins over synthetic weights, an explicit path over both
    cached = W.synth_clip_text(8, "ViT-B/32", layers=1)
    os.makedirs(os.path.dirname(CT.clip_cache_path("ViT-B/32")))
    torch.save(cached, CT.clip_cache_path("ViT-B/32"))
    got = CT.resolve_text_weights("ViT-B/32", synthetic_seed=4, layers=1)
    assert torch.equal(got["text_projection"], cached["text_projection"])
    explicit = W.synth_clip_text(9, "ViT-B/32", layers=1)
    torch.save(explicit, str(tmp_path / "w.pt"))
    got = CT.resolve_text_weights("ViT-B/32", clip_text_weights=str(tmp_path / "w.pt"), synthetic_seed=4)
    assert torch.equal(got["text_projection"], explicit["text_projection"])


def test_encoder_rejects_unknown_names_and_operand_types():
    with pytest.raises(ValueError, match="unsupported CLIP model name"):
        CT.ClipTextEncoder("ViT-H/14", synthetic_seed=1)
    with pytest.raises(ValueError, match="operand_type"):
        CT.ClipTextEncoder("ViT-B/16", synthetic_seed=1, operand_type="bf16")


def _cfg(**kw):
    c = {"prefix_size": 768, "support_memory_size": 4, "dino_model": "dinov2_vitb14_reg", "synthetic_seed": 1}
    c.update(kw)
    return c


def test_online_texts_skips_the_projection_type_check():
    from patchioner_amd import Patchioner
    bad = _cfg(projection_type="no-such-dataset", synthetic_seed=None, decap_weights={})
    with pytest.raises(Exception, match="projection_type field must be"):
        Patchioner.from_config(bad, device="cpu")
    # with online_texts the same config passes the check and stops only at the device (no CPU path)
    with pytest.raises(RuntimeError, match="no CPU path"):
        Patchioner.from_config(bad, device="cpu", online_texts=["a dog", "a cat"])


def test_online_texts_and_open_clip_argument_checks():
    from patchioner_amd import Patchioner
    with pytest.raises(NotImplementedError, match="OpenCLIP text-tower weights"):
        Patchioner.from_config(_cfg(use_open_clip=True), device="cpu")
    with pytest.raises(NotImplementedError, match="OpenCLIP"):
        Patchioner.from_config(_cfg(use_open_clip=True), device="cpu", online_texts=["a dog"])
    with pytest.raises(TypeError, match="list of str"):
        Patchioner.from_config(_cfg(), device="cpu", online_texts="a dog")
    with pytest.raises(ValueError, match="online_texts is empty"):
        Patchioner.from_config(_cfg(), device="cpu", online_texts=[])


def test_bank_default_clip_model():
    from patchioner_amd.bank import default_clip_model, memory_bank_filename
    assert default_clip_model(True) == "ViT-B/16" and default_clip_model(False) == "ViT-B/32"
    assert memory_bank_filename("online_texts", None, 3, use_talk2dino=True)[0].endswith("-ViT-B.16-3.h5")


def test_synth_talk2dino_shapes():
    w = W.synth_talk2dino(1, 512, 768)
    assert w["linear_layer.weight"].shape == (768, 512) and w["hidden_layers.0.weight"].shape == (768, 768)
    assert "hidden_layers.0.weight" not in W.synth_talk2dino(1, 512, 768, hidden=False)
