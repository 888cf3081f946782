"""The ViECap head on the device path: hard prompts composed on the GPU (pio_viecap_compose_prompts), the ragged prompted decode
(pio_viecap_decode_ragged), forward_async without a sync, and TraceCaptionPipeline with a ViECap model.  Every bar is exact: token rows
equal to the host path's, ids equal to the uniform decode of each row alone, captions equal to forward()'s."""
import random

import numpy as np
import pytest
import torch

import golden_cases as gc
from patchioner_amd import viecap as V
from patchioner_amd import weights as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def case():
    w, (vocab, merges), ents, emb, x = gc.viecap_case()
    return w, V.ByteLevelBPE(vocab, merges), ents, emb, x


def _viecap_cfg(w, tok, ents, emb, **over):
    c = gc.VIECAP
    cfg = dict(clip_hidden_size=c["C"], weights=w, tokenizer=tok, entities_text=ents, texts_embeddings=emb, temperature=c["temperature"],
               top_k=c["top_k"], threshold=c["threshold"], using_hard_prompt=True, soft_prompt_first=True, using_greedy_search=True)
    cfg.update(over)
    return cfg


def _model(viecap_cfg, depth=2, **over):
    from patchioner_amd import Patchioner
    dino = "dinov2_vitb14_reg"
    cfg = {"decap_weights": None, "prefix_size": 768, "linear_talk2dino": False, "support_memory_size": 0, "dino_model": dino,
           "normalize": False, "resize_dim": 224, "crop_dim": 224, "dino_weights": W.synth_dinov2(91, dino, depth=depth),
           "max_batch": 32, "max_prefixes": 128, "viecap": viecap_cfg}
    cfg.update(over)
    return Patchioner.from_config(cfg, device="cuda")


def _host_rows(tok, ents, probs, top_k, threshold, calls, pad_id=0):
    """The host path: top_k_entities + encode + pad_sequence(.., pad_id) per caption call."""
    rows, lens = [], []
    for a, b in calls:
        r = [tok.encode(V.compose_discrete_prompt_text(V.top_k_entities(ents, probs[i], top_k, threshold))) for i in range(a, b)]
        L = max(len(t) for t in r)
        rows += [t + [pad_id] * (L - len(t)) for t in r]
        lens += [L] * (b - a)
    return rows, lens


def _probs(seed, N, K):
    """Entity probabilities with every kind of row: peaked on one entity, spread over three or eight, flat (nothing passes)."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(N, K, generator=g) * torch.linspace(0.5, 12.0, N)[:, None]
    p = torch.softmax(logits, dim=-1)
    p[0] = 1.0 / K                                                     # flat: the 'something' prompt
    p[1] = 0.0
    p[1, [K - 1, 3, 7]] = torch.tensor([0.3, 0.34, 0.36])              # three above any threshold < 0.3, last index first
    p[2] = 0.0
    p[2, [5 + 2 * j for j in range(8)]] = torch.tensor([0.09 + 0.002 * j for j in range(8)])   # eight, no exact tie
    return p.contiguous()


def test_device_composition_equals_the_host_path(case):
    w, tok, ents, emb, _ = case
    m = _model(_viecap_cfg(w, tok, ents, emb))
    eng = m.engine
    rng = random.Random(5)
    letters = "abcdefghijklmnopqrstuvwxyz"
    big = sorted({" ".join("".join(rng.choice(letters) for _ in range(rng.randint(2, 9))) for _ in range(rng.randint(1, 3)))
                  for _ in range(3000)})
    for vocab_ents, top_k, threshold in ((list(ents), 3, 0.2), (list(ents), 1, 0.05), (big, 8, 0.004), (big, 3, 0.02)):
        frag = V.PromptFragments(tok, vocab_ents, top_k)
        assert frag.bad == []
        frag.to(eng.device)
        N, K = 70, len(vocab_ents)
        probs = _probs(len(vocab_ents) + top_k, N, K)
        cuts = [0, 1, 9, 25, 26, 44, 70]                               # uneven calls, one of a single row
        calls = list(zip(cuts[:-1], cuts[1:]))
        seg = torch.tensor(sum([[i] * (b - a) for i, (a, b) in enumerate(calls)], []), dtype=torch.int32, device="cuda")
        tokens, lens = eng.viecap_compose_prompts(probs.cuda(), frag, top_k, threshold, pad_id=0, seg=seg)
        want_rows, want_lens = _host_rows(tok, vocab_ents, probs, top_k, threshold, calls)
        got, got_lens = tokens.cpu().tolist(), lens.cpu().tolist()
        assert got_lens == want_lens
        for i, r in enumerate(want_rows):
            assert got[i][:len(r)] == r, (i, got[i][:len(r)], r)
            assert all(t == 0 for t in got[i][len(r):])
        n_ent = [len(V.top_k_entities(vocab_ents, probs[i], top_k, threshold)) for i in range(N)]
        assert 0 in n_ent and top_k in n_ent                           # both kinds of rows were exercised
        # one call (seg=None): every row padded to the batch's longest
        tokens1, lens1 = eng.viecap_compose_prompts(probs.cuda(), frag, top_k, threshold, pad_id=0)
        want_rows, want_lens = _host_rows(tok, vocab_ents, probs, top_k, threshold, [(0, N)])
        assert lens1.cpu().tolist() == want_lens and tokens1[:, :want_lens[0]].cpu().tolist() == want_rows
    with pytest.raises(Exception):
        eng.viecap_compose_prompts(probs.cuda(), frag, 9, 0.1, pad_id=0)


@pytest.mark.parametrize("graphs,prefill", [(True, "1"), (False, "1"), (True, "0")])
def test_ragged_decode_rows_equal_the_uniform_decode_of_each_row(case, graphs, prefill, monkeypatch):
    """72 rows (above 64: the row counts at which the uniform decode switches to split-fp16 GEMMs), prompt lengths on both sides of 16
    (the uniform prefill's kernel family changes there), every prompt layout; PIO_DEC_PREFILL=0: the uniform decode prefills position
    by position."""
    monkeypatch.setenv("PIO_NO_GRAPH", "0" if graphs else "1")
    monkeypatch.setenv("PIO_DEC_PREFILL", prefill)
    w, tok, ents, emb, x = case
    m = _model(_viecap_cfg(w, tok, ents, emb))
    eng = m.engine
    N, Ltmax = 72, 20
    feats = torch.cat([x, gc.randn(77, N - x.shape[0], x.shape[1])]).cuda().contiguous()
    cont = eng.viecap_mapping(feats)
    g = torch.Generator().manual_seed(9)
    tokens = torch.randint(0, len(tok), (N, Ltmax), generator=g, dtype=torch.int32)
    lens = torch.tensor([1 + (7 * i) % Ltmax for i in range(N)], dtype=torch.int32)
    assert len(set(lens.tolist())) == Ltmax
    tok_d, lens_d = tokens.cuda(), lens.cuda()
    clone = eng.clone_decoder()
    try:
        for layout in ("soft_first", "hard_first", "only_hard", "no_hard"):
            c = None if layout == "only_hard" else cont
            t = None if layout == "no_hard" else tok_d
            ln = None if layout == "no_hard" else lens_d
            sf = layout != "hard_first"
            got = eng.viecap_decode_ragged(c, t, ln, soft_first=sf, steps=64).cpu()
            for i in range(N):
                ti = None if t is None else tok_d[i:i + 1, :int(lens[i])]
                want = eng.viecap_decode(None if c is None else c[i:i + 1], ti, soft_first=sf, steps=64).cpu()
                assert torch.equal(got[i:i + 1], want), (layout, i, int(lens[i]))
            if layout == "soft_first":
                assert torch.equal(clone.viecap_decode_ragged(c, t, ln, soft_first=sf, steps=64).cpu(), got)
                torch.cuda.synchronize()
    finally:
        torch.cuda.synchronize()
        clone.close()


def _batches(n_batches, seed, last_one=False):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n_batches):
        b = 1 if (last_one and i == n_batches - 1) else 16
        imgs = W.synth_images(seed * 100 + i, b, 224).cuda()
        traces = [gc.block_trace(int(rng.randint(0, 13)), int(rng.randint(0, 13))) for _ in range(b)]
        out.append((imgs, traces))
    return out


def _spread_entities(m, batches, ents, seed=11):
    """Entity embeddings that split the trace features of `batches` among the entities: the features share a large common direction,
    so random entities would all lose to the same one; these are orthogonal to it, and the temperature is set so that the probabilities
    are peaked on some rows and flat on others (prompts of many lengths)."""
    feats = []
    real = m.caption_tokens
    m.caption_tokens = lambda x, **kw: feats.append(x.clone()) or ["."] * x.shape[0]
    try:
        for imgs, tr in batches:
            m(imgs, get_cls_capt=False, traces=tr, use_attention_tracing=True)
    finally:
        m.caption_tokens = real
    f = torch.cat(feats).cpu().double()
    f = f / f.norm(dim=-1, keepdim=True)
    c = f.mean(0)
    c = c / c.norm()
    e = gc.randn(seed, len(ents), f.shape[1]).double()
    e = e - (e @ c)[:, None] * c[None]
    e = e / e.norm(dim=-1, keepdim=True)
    s = (f @ e.T).std().item()
    return e.float(), s / 2.5


def test_pipeline_equals_forward_for_a_viecap_model(case):
    from patchioner_amd.pipeline import TraceCaptionPipeline
    w, tok, ents, emb, _ = case
    batches = _batches(12, 3)
    probe = _model(_viecap_cfg(w, tok, ents, emb))
    emb2, temp = _spread_entities(probe, batches, ents)
    del probe
    base = dict(texts_embeddings=emb2, temperature=temp, top_k=3, threshold=0.3)
    m = _model(_viecap_cfg(w, tok, ents, emb, **base))
    want, Lb = [], []
    for imgs, tr in batches:
        want.append(m(imgs, get_cls_capt=False, traces=tr, use_attention_tracing=True)["trace_capts"])
        Lb.append(int(m.viecap.last_prompt_tokens.shape[1]))
    print("hard-prompt lengths per batch:", Lb)
    assert len(set(Lb)) >= 2, Lb                                       # the groups mix batches of different prompt lengths

    def run(model, bs, **kw):
        pipe = TraceCaptionPipeline(model, use_attention_tracing=True, **kw)
        try:
            return list(pipe.run(bs, total=len(bs)))
        finally:
            pipe.close()

    assert run(m, batches, group_batches=8, vit_batches=2) == want    # a group of 128 rows, then one of 64
    assert run(m, batches, group_batches=3, vit_batches=2, decode_clones=2) == want
    # CLS regions
    want_cls = [m(imgs, get_cls_capt=True)["cls_capt"] for imgs, _ in batches[:6]]
    assert run(m, [(imgs, None) for imgs, _ in batches[:6]], group_batches=4, vit_batches=2) == want_cls
    # a last batch of one image: a str, as forward() returns it
    short = batches[:4] + _batches(1, 8, last_one=True)
    want_short = [m(imgs, get_cls_capt=False, traces=tr, use_attention_tracing=True)["trace_capts"] for imgs, tr in short]
    assert isinstance(want_short[-1], str)
    assert run(m, short, group_batches=4, vit_batches=2) == want_short
    del m
    for over in (dict(soft_prompt_first=False), dict(only_hard_prompt=True), dict(using_hard_prompt=False)):
        mm = _model(_viecap_cfg(w, tok, ents, emb, **base, **over))
        want_o = [mm(imgs, get_cls_capt=False, traces=tr, use_attention_tracing=True)["trace_capts"] for imgs, tr in batches[:8]]
        assert run(mm, batches[:8], group_batches=4, vit_batches=2, decode_clones=1) == want_o, over
        del mm


def test_forward_async_does_not_wait_and_equals_forward(case):
    w, tok, ents, emb, x = case
    m = _model(_viecap_cfg(w, tok, ents, emb))
    imgs = W.synth_images(41, 16, 224).cuda()
    traces = [gc.block_trace(i % 13, (5 * i) % 13) for i in range(16)]
    want = m(imgs, traces=traces, use_attention_tracing=True)
    m.forward_async(imgs, traces=traces, use_attention_tracing=True).result()          # warm: workspaces and graphs exist
    torch.cuda.synchronize()
    torch.cuda._sleep(1_000_000_000)                                   # ~0.5 s of spin ahead of everything on the stream
    pend = m.forward_async(imgs, traces=traces, use_attention_tracing=True)
    assert pend.done() is False
    got = pend.result()
    assert got["trace_capts"] == want["trace_capts"] and got["cls_capt"] == want["cls_capt"]
    # a single image: the str quirk survives the deferred path
    one = m(imgs[:1], traces=traces[:1], use_attention_tracing=True)["trace_capts"]
    assert isinstance(one, str)
    assert m.forward_async(imgs[:1], traces=traces[:1], use_attention_tracing=True).result()["trace_capts"] == one
    with pytest.raises(NotImplementedError):                           # score lists are not deferred (as for the DeCap head)
        m.forward_async(imgs, get_cls_capt=True, compute_scores=True)


class _MergesKiteComma:
    def __init__(self, base):
        self.base, self.pad_token_id = base, None

    def encode(self, text):
        return self.base.encode(text.replace("kite, ", "kite\x01"))

    def decode(self, ids):
        return self.base.decode(ids)


def test_device_path_errors(case):
    from patchioner_amd.pipeline import BoxRegions, TraceCaptionPipeline
    w, tok, ents, emb, x = case
    beam = _model(_viecap_cfg(w, tok, ents, emb, using_greedy_search=False, beam_width=2))
    with pytest.raises(ValueError):
        TraceCaptionPipeline(beam)
    del beam
    bad = _model(_viecap_cfg(w, _MergesKiteComma(tok), ents, emb))
    imgs = W.synth_images(43, 2, 224).cuda()
    traces = [gc.block_trace(1, 2), gc.block_trace(7, 3)]
    assert isinstance(bad(imgs, get_cls_capt=False, traces=traces)["trace_capts"], list)    # the host path still works
    with pytest.raises(ValueError, match="'kite'"):
        bad.forward_async(imgs, traces=traces)
    with pytest.raises(ValueError, match="'kite'"):
        TraceCaptionPipeline(bad)
    del bad
    m = _model(_viecap_cfg(w, tok, ents, emb))
    pipe = TraceCaptionPipeline(m)
    boxes = BoxRegions(torch.tensor([[[0, 0, 100, 100]], [[20, 20, 90, 120]]], dtype=torch.float32))
    with pytest.raises(NotImplementedError):
        list(pipe.run([(imgs, boxes)]))
    pipe.close()
