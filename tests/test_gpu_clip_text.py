"""The CLIP text tower on the MI355X (csrc/text_encoder.hip through clip_text.ClipTextEncoder), the bank build on it and
Patchioner's online_texts.

tests/golden/clip_text_hf.npz holds transformers.CLIPTextModelWithProjection outputs (an independent implementation of the
OpenAI text tower; fp32, CPU, eager attention, eos_token_id 49407) for weights.synth_clip_text(501, "ViT-B/16") and
(502, "ViT-L/14") at depth 12 (tools/oracle/gen_golden_clip_text.py).

Tolerances (max |err| / max |ref| over the compared features):
  * fp32 operands (the parity mode): 1e-5 -- fp32 rounding of the same sums in another order, no operand rounding;
  * fp16 operands: 4e-3 and a cosine >= 1 - 4 tol^2 per caption -- the bar of the fp16 ViT against its HF ports
    (tests/test_gpu_vit_hf.py), for the same operand precision (fp16 operands, fp32 accumulate and residual stream) through the
    same depth (12 pre-LN blocks with QuickGELU); the final LayerNorm and the projection run in fp32 on both paths.
"""
import json
import os

import numpy as np
import pytest
import torch

from patchioner_amd import _lib
from patchioner_amd import clip_text as CT
from patchioner_amd import weights as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SEEDS = {"ViT-B/16": 501, "ViT-L/14": 502}


def _rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


def _captions(n, seed=5):
    """COCO-like synthetic captions, 8-20 words."""
    rng = np.random.RandomState(seed)
    words = ("a an the two man woman dog cat bus train kitchen table red blue small large sitting standing riding eating "
             "next to on in of with near street field water grass plate pizza bike horse sky tree white black young old").split()
    return [" ".join(rng.choice(words, size=rng.randint(8, 21))) + rng.choice([".", "", "!"]) for _ in range(n)]


@pytest.mark.parametrize("tag,name", [("b16", "ViT-B/16"), ("l14", "ViT-L/14")])
@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-5), ("fp16", 4e-3)])
def test_tower_vs_hf(golden, tag, name, dtype, tol):
    g = golden("clip_text_hf")
    ids = torch.from_numpy(g["ids"]).long()
    ref = torch.from_numpy(g["%s_feats" % tag])
    enc = CT.ClipTextEncoder(name, synthetic_seed=SEEDS[name], operand_type=dtype, max_texts=64)
    try:
        got = enc.encode_text(ids).cpu()
        texts = json.loads(g["texts_json"].tobytes())
        from_text = enc.encode_text(texts).cpu()            # host BPE -> the same rows
    finally:
        enc.close()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    assert torch.equal(from_text, got)
    err = _rel(got, ref)
    cos = float(torch.nn.functional.cosine_similarity(got, ref, dim=1).min())
    print("CLIP text %s [%s]: rel-max-err %.2e, min cos %.8f" % (name, dtype, err, cos))
    assert err <= tol
    if dtype == "fp16":                                     # (in fp32 the bar would sit below the cosine's own rounding)
        assert cos >= 1 - 4 * tol * tol


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_caption_bits_do_not_depend_on_the_launch(dtype):
    """A caption's feature: alone (padded to its own length), in a mixed-length launch of 320 captions, padded to 77 -- and
    through encode_text's length buckets -- all the same bits."""
    texts = _captions(320)
    enc = CT.ClipTextEncoder("ViT-B/16", synthetic_seed=501, operand_type=dtype, max_texts=512)
    try:
        ids = enc.tokenizer.tokenize(texts) if enc.tokenizer else CT.tokenize(texts)
        lens = (ids.argmax(1) + 1).tolist()
        L = max(lens)
        assert L < 77 and min(lens) < L - 8
        batch = enc.encode_ids_raw(ids[:, :L]).cpu()
        pad77 = enc.encode_ids_raw(ids).cpu()
        bucketed = enc.encode_text(texts).cpu()
        alone = torch.cat([enc.encode_ids_raw(ids[i:i + 1, :lens[i]]).cpu() for i in range(len(texts))])
    finally:
        enc.close()
    assert torch.isfinite(batch).all()
    assert torch.equal(alone, batch)
    assert torch.equal(pad77, batch)
    assert torch.equal(bucketed, batch)


def test_edge_cases_and_errors():
    enc = CT.ClipTextEncoder("ViT-B/32", synthetic_seed=7, operand_type="fp16", max_texts=4, layers=2)
    try:
        edge = enc.encode_text(["", " ".join(["dog"] * 75)])
        assert edge.shape == (2, 512) and torch.isfinite(edge).all()
        bad = torch.tensor([[49406, 49408, 49407]])
        with pytest.raises(_lib.PioError, match="outside"):
            enc.encode_ids_raw(bad)
        with pytest.raises(_lib.PioError, match="max_texts"):
            enc.encode_ids_raw(torch.zeros(5, 3, dtype=torch.long))
        with pytest.raises(_lib.PioError, match="context_length"):
            enc.encode_ids_raw(torch.zeros(1, 78, dtype=torch.long))
        again = enc.encode_text(["", " ".join(["dog"] * 75)])     # the handle is still usable, the error flag cleared
        assert torch.equal(again, edge)
    finally:
        enc.close()
    sd = W.synth_clip_text(7, "ViT-B/32", layers=2)
    del sd["transformer.resblocks.1.mlp.c_fc.bias"]
    with pytest.raises(_lib.PioError, match="missing weight 'transformer.resblocks.1.mlp.c_fc.bias'"):
        CT.ClipTextEncoder("ViT-B/32", weights=sd)
    sd = W.synth_clip_text(7, "ViT-B/32", layers=2)
    sd["text_projection"] = sd["text_projection"][:, :256]
    with pytest.raises(_lib.PioError, match="text_projection"):
        CT.ClipTextEncoder("ViT-B/32", weights=sd)


def test_bank_builder_with_the_device_tower(golden, tmp_path):
    """build_memory_bank(engine, texts, encode_text=None): the rows are Talk2DINO's projection of the HF fixture's features
    (2e-5: the fp32 tower's 1e-5 plus the projection's own fp32 rounding, test_gpu_bank.py), and the file reads back through
    the model."""
    from patchioner_amd.bank import build_memory_bank
    from patchioner_amd.engine import Engine
    from patchioner_amd.model import Patchioner, load_memory_bank
    g = golden("clip_text_hf")
    texts = json.loads(g["texts_json"].tobytes())
    t2d = W.synth_talk2dino(11, 512, 768)
    e = Engine(embed_dim=768, depth=1, num_heads=12, num_registers=4, crop_dim=224, max_batch=1)
    try:
        path = build_memory_bank(e, texts, None, str(tmp_path), "coco_captions", None, None, talk2dino_state_dict=t2d,
                                 synthetic_seed=SEEDS["ViT-B/16"], clip_text_dtype="fp32", batch_size=3)
        want = e.text_project(torch.from_numpy(g["b16_feats"]), t2d["linear_layer.weight"], t2d["linear_layer.bias"],
                              t2d["hidden_layers.0.weight"], t2d["hidden_layers.0.bias"], act="tanh").cpu()
    finally:
        e.close()
    assert os.path.basename(path) == "coco_captions_text_embeddings-B16-ViT-B.16-%d.h5" % len(texts)
    bank, t = load_memory_bank(path, want_texts=True)
    assert [x.decode() for x in t] == texts
    assert _rel(bank, want) <= 2e-5
    m = Patchioner.from_config({"decap_weights": W.synth_decap(3), "prefix_size": 768, "support_memory_size": len(texts),
                                "dino_model": "dinov2_vitb14_reg", "memory_bank": path, "resize_dim": 224, "crop_dim": 224,
                                "dino_weights": W.synth_dinov2(1, "dinov2_vitb14_reg", depth=1), "calculate_argmax_text": True},
                               "cuda")
    assert m.caption_tokens(bank[[0, 3]].clone().cuda()) == [texts[0], texts[3]]


def _e2e_models(cfg, texts, bank_fn):
    from patchioner_amd import Patchioner
    online = Patchioner.from_config(dict(cfg), "cuda", online_texts=texts)
    bank = bank_fn(online)
    fixed = Patchioner.from_config(dict(cfg, memory_bank=bank.cpu(), memory_bank_texts=texts), "cuda")
    return online, fixed


@pytest.mark.parametrize("backbone", ["dinov2", "clip"])
def test_online_texts_end_to_end(backbone):
    """Synthetic-seed models with online_texts (fp32 text tower) against the same model given the identical bank as a
    memory_bank tensor: the same captions and the same arg-max texts, which are among online_texts."""
    seed = 40
    texts = _captions(300, seed=9) + ["", "a dog", "a dog"]
    if backbone == "dinov2":
        cfg = {"prefix_size": 768, "support_memory_size": 5000, "dino_model": "dinov2_vitb14_reg", "synthetic_seed": seed,
               "resize_dim": 224, "crop_dim": 224, "clip_text_dtype": "fp32", "projection_type": "no-such-dataset"}
        dim, name = 768, "ViT-B/16"
    else:
        cfg = {"prefix_size": 512, "support_memory_size": 5000, "dino_model": "vit_base_patch16_clip_224.openai",
               "synthetic_seed": seed, "resize_dim": 224, "crop_dim": 224, "clip_text_dtype": "fp32", "use_talk2dino_project": False}
        dim, name = 512, "ViT-B/32"

    def bank_fn(model):
        enc = CT.ClipTextEncoder(name, synthetic_seed=seed + 5, operand_type="fp32")
        try:
            f = enc.encode_text(texts)
        finally:
            enc.close()
        if backbone == "dinov2":
            t2d = W.synth_talk2dino(seed + 6, 512, 768)
            f = model.engine.text_project(f, t2d["linear_layer.weight"], t2d["linear_layer.bias"], t2d["hidden_layers.0.weight"],
                                          t2d["hidden_layers.0.bias"], act="tanh")
        return f

    q = torch.randn(6, dim, generator=torch.Generator().manual_seed(3))
    online, fixed = _e2e_models(cfg, texts, bank_fn)
    assert online.engine.bank_rows == len(texts)          # exactly the texts, no padding to support_memory_size
    assert online.text_dataset == [t.encode() for t in texts]
    assert online.caption_tokens(q.clone().cuda()) == fixed.caption_tokens(q.clone().cuda())
    a_online, a_fixed = _e2e_models(dict(cfg, calculate_argmax_text=True), texts, bank_fn)
    got = a_online.caption_tokens(q.clone().cuda())
    assert got == a_fixed.caption_tokens(q.clone().cuda())
    assert all(t in texts for t in got)
