"""Batched beam search of the ViECap head on the device (pio_lm_beam_search): N images x W beams as the rows of one decode, the
selection and its bookkeeping on the device.  Every bar is exact: each image's ids, lengths, score bits and order equal what
VieCapHead.beam_search gives for that image alone (the per-image loop forward() keeps)."""
import json

import numpy as np
import pytest
import torch

import golden_cases as gc
from patchioner_amd import viecap as V
from patchioner_amd import weights as W
from patchioner_amd._lib import PioError

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def case():
    w, (vocab, merges), ents, emb, x = gc.viecap_case()
    return w, V.ByteLevelBPE(vocab, merges), ents, emb, x


def _viecap_cfg(w, tok, ents, emb, **over):
    c = gc.VIECAP
    cfg = dict(clip_hidden_size=c["C"], weights=w, tokenizer=tok, entities_text=ents, texts_embeddings=emb, temperature=c["temperature"],
               top_k=c["top_k"], threshold=c["threshold"], using_hard_prompt=True, soft_prompt_first=True, using_greedy_search=False,
               beam_width=5)
    cfg.update(over)
    return cfg


def _model(viecap_cfg, **over):
    from patchioner_amd import Patchioner
    dino = "dinov2_vitb14_reg"
    cfg = {"decap_weights": None, "prefix_size": 768, "linear_talk2dino": False, "support_memory_size": 0, "dino_model": dino,
           "normalize": False, "resize_dim": 224, "crop_dim": 224, "dino_weights": W.synth_dinov2(91, dino, depth=2),
           "max_batch": 32, "max_prefixes": 128, "viecap": viecap_cfg}
    cfg.update(over)
    return Patchioner.from_config(cfg, device="cuda")


@pytest.fixture(scope="module")
def beam_model(case):
    w, tok, ents, emb, x = case
    return _model(_viecap_cfg(w, tok, ents, emb))


def _eos_strings(golden):
    meta = json.loads(bytes(golden("viecap_beam")["meta_json"]).decode())
    return tuple(meta["eos_strings"])


def _per_image(head, prompt, plen, W_, eos_strings):
    """head.beam_search on each image alone -> [(ids per beam, lens, score bits, order)]"""
    out = []
    for n in range(prompt.shape[0]):
        head.beam_search(prompt[n:n + 1, :int(plen[n])].contiguous(), W_, end_of_sentences=eos_strings)
        beams = head.last_beams
        out.append(([b[0] for b in beams], [int(b[1]) for b in beams],
                    np.array([b[2] for b in beams], dtype=np.float32).view(np.int32).tolist(), list(head.last_beam_order)))
    return out


def _device(head, ids, lens, scores):
    ids, lens, scores = ids.cpu(), lens.cpu(), scores.cpu()
    out = []
    for n in range(ids.shape[0]):
        Wn = ids.shape[1]
        out.append(([ids[n, b, :int(lens[n, b])].tolist() for b in range(Wn)], lens[n].tolist(),
                    scores[n].numpy().view(np.int32).tolist(), V.VieCapHead.beam_order(scores[n])))
    return out


def _prompts(m, seeds=(3, 4, 5), sizes=(16, 16, 12)):
    """Caption calls of different sizes (so of different padded hard-prompt lengths L_b) staged as forward_async stages them."""
    head, C = m.viecap, gc.VIECAP["C"]
    conts, toks, lens = [], [], []
    for seed, n in zip(seeds, sizes):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(n, C, generator=g) * 0.02
        cont, tok, ln = head.stage(x)
        conts.append(cont)
        toks.append(tok)
        lens.append(ln)
    cont, tok, ln = torch.cat(conts), torch.cat(toks), torch.cat(lens)
    return m.engine.viecap_build_prompt_ragged(cont, tok, ln, soft_first=head.soft_first())


def test_reference_fixture_in_one_call(golden, case, beam_model):
    """tests/golden/viecap_beam.npz: its three images in ONE pio_lm_beam_search, both eos sets.  Each equals head.beam_search on that
    image alone (ids, lengths, score bits, order); against the reference, test_viecap_beam_search_vs_reference_and_oracle's rule."""
    g = golden("viecap_beam")
    meta = json.loads(bytes(g["meta_json"]).decode())
    w, tok, ents, emb, x = case
    m, head, c = beam_model, beam_model.viecap, gc.VIECAP
    xd = x[:3].clone().cuda()
    cont = m.engine.viecap_mapping(xd)
    probs = m.engine.viecap_entity_logits(xd, c["temperature"]).cpu()
    rows = [tok.encode(V.compose_discrete_prompt_text(V.top_k_entities(ents, probs[i], c["top_k"], c["threshold"]))) for i in range(3)]
    L = max(len(r) for r in rows)
    tokens = torch.zeros(3, L, dtype=torch.int32)
    for i, r in enumerate(rows):
        tokens[i, :len(r)] = torch.tensor(r, dtype=torch.int32)
    prompts = m.engine.viecap_build_prompt(cont, tokens, soft_first=True)
    P = prompts.shape[1]
    exact = 0
    for eos_strings, label in (((".", " ."), "default"), (tuple(meta["eos_strings"]), None)):
        eos = [tok.encode(e)[-1] for e in eos_strings]
        got = _device(head, *m.engine.lm_beam_search(prompts, None, 5, eos))
        want = _per_image(head, prompts, [P] * 3, 5, eos_strings)
        assert got == want, eos_strings
        for call in meta["calls"]:
            if (call["label"] == "default") != (label == "default"):
                continue
            i = call["image"]
            ref = g["%s_%d_ids" % (call["label"], i)]
            exact += all(got[i][0][b] == ref[b, :int((ref[b] >= 0).sum())].tolist() for b in range(5))
    assert exact >= len(meta["calls"]) - 1


@pytest.mark.parametrize("W_", [1, 2, 5, 8])
def test_bits_at_scale(golden, beam_model, W_):
    """44 images from three caption calls (different L_b); eos ids the seeded model emits, so images freeze early, midway or never.
    W = 8: 16 images fill 128 rows exactly and the 17th starts the next chunk; W = 2: 64 images per chunk."""
    m, head = beam_model, beam_model.viecap
    eos_strings = _eos_strings(golden)
    eos = [head.tokenizer.encode(e)[-1] for e in eos_strings]
    prompt, plen = _prompts(m)
    assert len(set(plen.tolist())) >= 2
    got = _device(head, *m.engine.lm_beam_search(prompt, plen, W_, eos))
    want = _per_image(head, prompt, plen.tolist(), W_, eos_strings)
    for n in range(len(want)):
        assert got[n] == want[n], n
    longest = [max(lens) for _, lens, _, _ in got]
    print("W=%d: longest beam per image: %s" % (W_, sorted(longest)))
    assert min(longest) < 64, "the eos set should freeze some images before the last step"


def test_no_graph_and_clone_identical(golden, case, beam_model, monkeypatch):
    """The same search with graphs off (PIO_NO_GRAPH=1 at context creation) and on a decoder clone: identical results."""
    m, head = beam_model, beam_model.viecap
    eos = [head.tokenizer.encode(e)[-1] for e in _eos_strings(golden)]
    prompt, plen = _prompts(m)
    want = [t.cpu() for t in m.engine.lm_beam_search(prompt, plen, 5, eos)]
    clone = m.engine.clone_decoder()
    got = [t.cpu() for t in clone.lm_beam_search(prompt, plen, 5, eos)]
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    clone.close()
    w, tok, ents, emb, x = case
    monkeypatch.setenv("PIO_NO_GRAPH", "1")
    m2 = _model(_viecap_cfg(w, tok, ents, emb))
    monkeypatch.delenv("PIO_NO_GRAPH")
    prompt2, plen2 = _prompts(m2)
    assert torch.equal(prompt2.cpu(), prompt.cpu()) and torch.equal(plen2.cpu(), plen.cpu())
    got2 = [t.cpu() for t in m2.engine.lm_beam_search(prompt2, plen2, 5, eos)]
    assert all(torch.equal(a, b) for a, b in zip(got2, want))


def test_forward_async_equals_forward_and_does_not_wait(beam_model):
    m = beam_model
    imgs = W.synth_images(41, 16, 224).cuda()
    traces = [gc.block_trace(i % 13, (5 * i) % 13) for i in range(16)]
    want = m(imgs, traces=traces, use_attention_tracing=True)
    m.forward_async(imgs, traces=traces, use_attention_tracing=True).result()          # warm: workspaces and graphs exist
    torch.cuda.synchronize()
    torch.cuda._sleep(1_000_000_000)
    pend = m.forward_async(imgs, traces=traces, use_attention_tracing=True)
    assert pend.done() is False
    got = pend.result()
    assert got["trace_capts"] == want["trace_capts"] and got["cls_capt"] == want["cls_capt"]
    assert m.last_ids is None
    one = m(imgs[:1], traces=traces[:1], use_attention_tracing=True)["trace_capts"]
    assert m.forward_async(imgs[:1], traces=traces[:1], use_attention_tracing=True).result()["trace_capts"] == one


def test_pipeline_beam_search(beam_model):
    from patchioner_amd.pipeline import TraceCaptionPipeline
    m = beam_model
    batches, want = [], []
    for i, n in enumerate((16, 16, 16, 16, 5)):                     # the last group is short
        imgs = W.synth_images(60 + i, n, 224).cuda()
        tr = [gc.block_trace((3 * j + i) % 13, (7 * j) % 13) for j in range(n)]
        batches.append((imgs, tr))
        want.append(m(imgs, get_cls_capt=False, traces=tr, use_attention_tracing=True)["trace_capts"])
    pipe = TraceCaptionPipeline(m, group_batches=2, use_attention_tracing=True, beam_search=True)
    try:
        got = list(pipe.run(batches, total=len(batches)))
    finally:
        pipe.close()
    assert got == want
    with pytest.raises(ValueError):
        TraceCaptionPipeline(m)
    with pytest.raises(ValueError, match="25 images"):
        TraceCaptionPipeline(m, group_batches=26, beam_search=True)


def test_refusals(beam_model):
    """W = 9: PIO_ERR_INVALID_ARG (-1); N W above min(max_prefixes, 128), Pmax above 128, Pmax + steps - 1 above max_steps:
    PIO_ERR_CAPACITY (-6)."""
    from patchioner_amd._lib import ptr
    eng = beam_model.engine
    prompt = torch.zeros(26, 20, 768, device="cuda")
    ids = torch.empty(26 * 8 * 64, device="cuda", dtype=torch.int32)
    f = torch.empty(26 * 8, device="cuda", dtype=torch.float32)

    def call(N, Pmax, W_, steps=64):
        return eng.lib.pio_lm_beam_search(eng.h, ptr(prompt), None, N, Pmax, W_, steps, 13, 764, ptr(ids), ptr(ids), ptr(f), None)

    assert call(2, 20, 9) == -1
    assert call(26, 20, 5) == -6                                        # 130 rows
    assert call(2, 129, 5) == -6
    assert call(2, 128, 5, steps=65) == -6
    with pytest.raises(PioError):
        eng.lm_beam_search(prompt[:2], None, 9, (13, 764))
