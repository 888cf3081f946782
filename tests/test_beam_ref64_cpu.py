"""tests/beam_ref64.py tied to the reference before any GPU sees it: the float64 search reproduces the reference's own beams
(tests/golden/viecap_beam.npz), and its selection order and bookkeeping equal torch.topk plus the reference's lines (search.py:247-276)
wherever no tie makes torch's order unspecified."""
import json
import math

import pytest
import torch

import beam_ref64 as B
import golden_cases as gc
import viecap_ref64 as R
from parity_helpers import MARGIN_BOUND
from patchioner_amd import viecap as V

torch.set_grad_enabled(False)
F64 = torch.float64


def fixture_prompts64(w, tok, ents, emb, x):
    """entrypoint.py:108-135 in float64 on the fixture's first three features: soft prompt, then the hard prompt's word embeddings,
    the token rows padded to the longest of the three (pad_sequence)."""
    c = gc.VIECAP
    cont = R.mapping64(w, x[:3])
    probs, _ = R.entity_probs64(x[:3], emb, c["temperature"])
    rows = [tok.encode(V.compose_discrete_prompt_text([ents[j] for j in R.select_reference(probs[i].float(), c["top_k"], c["threshold"])]))
            for i in range(3)]
    pad = tok.pad_token_id if tok.pad_token_id is not None else 0
    L = max(len(r) for r in rows)
    tokens = torch.tensor([r + [pad] * (L - len(r)) for r in rows])
    wte = w["gpt.transformer.wte.weight"].double()
    return torch.cat((cont, wte[tokens]), dim=1)


def test_beam64_reproduces_the_reference_fixture(golden):
    """All six calls of the fixture (three prompts; the reference's own eos strings and two the seeded model emits), all 5 beams, ids up
    to each beam's length.  A call is excused only if one of ITS float64 margins is below MARGIN_BOUND (the fixture is fp32)."""
    g = golden("viecap_beam")
    meta = json.loads(bytes(g["meta_json"]).decode())
    w, (vocab, merges), ents, emb, x = gc.viecap_case()
    tok = V.ByteLevelBPE(vocab, merges)
    model = R.GPT2_64(w)
    prompts = fixture_prompts64(w, tok, ents, emb, x)
    excused, smallest = 0, math.inf
    for call in meta["calls"]:
        eos_strings = (".", " .") if call["label"] == "default" else tuple(meta["eos_strings"])
        eos = [tok.encode(e)[-1] for e in eos_strings]
        i = call["image"]
        out = B.beam64(model, prompts[i], 5, 64, eos)
        ref = g["%s_%d_ids" % (call["label"], i)]
        low = min(min(m) for m in out["margins"])
        smallest = min(smallest, low)
        same = all(out["ids"][b] == ref[b, :int((ref[b] >= 0).sum())].tolist() for b in range(5))
        same = same and out["lens"] == [int(l) for l in call["lengths"]]
        if not same:
            assert low < MARGIN_BOUND, "%s image %d departs from the fixture; its smallest float64 margin is %.3e" % (call["label"], i, low)
            excused += 1
    print("beam64 on the fixture: %d of %d calls identical, smallest float64 margin %.3e" % (len(meta["calls"]) - excused, len(meta["calls"]), smallest))
    assert excused <= 1


def _reference_lines(lp, scores, lens, stopped, tokens, W, eos):
    """search.py:256-276 on float64 tensors, statement by statement."""
    logits = lp.clone()
    logits[stopped] = -float("inf")
    logits[stopped, 0] = 0
    scores_sum = scores[:, None] + logits
    lens = lens.clone()
    lens[~stopped] += 1
    avg = scores_sum / lens[:, None]
    avg, nxt = avg.view(-1).topk(W, -1)
    src = torch.div(nxt, scores_sum.shape[1], rounding_mode="trunc")
    lens = lens[src]
    nxt = nxt % scores_sum.shape[1]
    tokens = torch.cat((tokens[src], nxt[:, None]), dim=1)
    scores = avg * lens
    stopped = stopped[src]
    stopped = stopped + (nxt.eq(eos[0]) | nxt.eq(eos[1]))
    return avg, src, nxt, scores, lens, stopped, tokens


@pytest.mark.parametrize("W,Vn", [(1, 37), (2, 1500), (5, 37), (5, 1500), (8, 50257)])
def test_select_and_step_spec_equal_topk_and_the_reference_lines(W, Vn):
    """Random tie-free log-probabilities, eos ids placed among the first winners so that beams stop at different steps; six selections
    chained, state against the reference's lines after each."""
    g = torch.Generator().manual_seed(100 * W + Vn)
    steps, npos = 6, 1024
    lp = torch.log_softmax(3.0 * torch.randn(W, Vn, generator=g, dtype=F64), dim=-1)
    vals, flat = B.select_spec(B.candidates64(lp[0]), W)
    top = lp[0].topk(W)
    assert flat == top.indices.tolist() and vals == top.values.tolist()
    eos = (flat[W // 2], flat[-1])
    state = B.step_spec(B.new_state(W, 3, steps, tstride=16), 0, vals, flat, Vn, eos, npos)
    scores, lens = top.values.clone(), torch.ones(W, dtype=F64)
    tokens = top.indices[:, None]
    stopped = top.indices.eq(eos[0]) | top.indices.eq(eos[1])
    assert state["stopped"] == stopped.int().tolist() and state["lens"] == [1.0] * W and state["xpos"] == 3
    lineage = [[b] for b in range(W)]                  # which rows wrote positions P .. of row b's history: the table's content
    for i in range(1, steps):
        lp = torch.log_softmax(3.0 * torch.randn(W, Vn, generator=g, dtype=F64), dim=-1)
        if bool(stopped.all()):
            frozen = B.step_spec(state, i, None, None, Vn, eos, npos)
            assert frozen["frozen"] and all(frozen[k] == state[k] for k in ("scores", "lens", "stopped", "tok", "hist", "tab"))
            break
        cand = B.candidates64(lp, state["scores"], state["lens"], state["stopped"])
        vals, flat = B.select_spec(cand, W)
        avg, src, nxt, scores, lens, stopped, tokens = _reference_lines(lp, scores, lens, stopped, tokens, W, eos)
        assert vals == avg.tolist() and flat == (src * Vn + nxt).tolist()
        state = B.step_spec(state, i, vals, flat, Vn, eos, npos)
        assert state["scores"] == scores.tolist() and state["lens"] == lens.tolist() and state["stopped"] == stopped.int().tolist()
        assert state["tok"] == nxt.tolist() and state["src"] == src.tolist()
        assert [h[:i + 1] for h in state["hist"]] == tokens.tolist() and all(h[i + 1:] == [-1] * (steps - i - 1) for h in state["hist"])
        lineage = [lineage[s][:] + [b] for b, s in enumerate(src.tolist())]
        for b in range(W):                             # prompt positions: the shared row; history: its lineage; beyond: its own slot
            assert state["tab"][b] == [0] * 3 + lineage[b][:-1] + [b] * (16 - 3 - i), (i, b)
        assert state["xpos"] == 3 + i
    assert B.step_spec(state, 5, vals, flat, Vn, eos, 7)["xpos"] == 6          # P + step = 8 >= npos: the clamp


def test_select_spec_order_on_ties_nan_and_infinities():
    nan, inf = float("nan"), float("inf")
    v = [1.0, nan, 3.0, 3.0, -inf, 3.0, inf, nan, -inf, 1.0]
    assert B.select_spec(v, 4) == ([inf, 3.0, 3.0, 3.0], [6, 2, 3, 5])
    assert B.select_spec(v, 8)[1] == [6, 2, 3, 5, 0, 9, 4, 8]
    assert B.select_spec(v, 8, extra=2) == ([inf, 3.0, 3.0, 3.0, 1.0, 1.0, -inf, -inf, -inf, -inf], [6, 2, 3, 5, 0, 9, 4, 8, -1, -1])
    assert B.select_spec([nan, nan], 2) == ([-inf, -inf], [-1, -1])
    big = torch.zeros(5000, dtype=F64)
    big[[4999, 17, 1024 + 17]] = 2.0                  # the value cut keeps every tie with the last rank
    assert B.select_spec(big, 4)[1] == [17, 1041, 4999, 0]


def test_candidates64_and_log_softmax64():
    lp = torch.tensor([[-1.0, -2.0, -3.0], [-0.5, -4.0, -0.25]], dtype=F64)
    c = B.candidates64(lp, [-2.0, -6.0], [1.0, 3.0], [0, 1])
    assert c.tolist() == [[-1.5, -2.0, -2.5], [-2.0, -float("inf"), -float("inf")]]
    assert B.candidates64(lp).tolist() == [[-1.0, -2.0, -3.0]]
    x = torch.tensor([[1000.0, 999.0, -1000.0]], dtype=F64)
    want = torch.log_softmax(x, dim=-1)
    assert torch.allclose(B.log_softmax64(x), want, rtol=0, atol=1e-12)
