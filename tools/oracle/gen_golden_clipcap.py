"""tests/golden/clipcap.npz: the REFERENCE's ClipCap head (through refshim) on the seeded case of tests/clipcap_case.py --
``ClipCapModel`` (P/src/clipcap/entrypoint.py:398-579) built by its own constructor, ``forward_batched`` -> ``generate_batched``
(:198-311) and ``forward_sequential`` -> ``generate2`` (:314-395), ``compute_perplexity_scores`` (:554-579).  What cannot exist
here is replaced in this process only: ``GPT2LMHeadModel.from_pretrained`` gives a random-weight ``GPT2Config()`` model (the
checkpoint then loads OUR seeded ``gpt.*`` and ``clip_project.*``), ``GPT2Tokenizer.from_pretrained`` the stub tokenizer, the
checkpoint loader our state dict.  ``torch.multinomial`` is patched to turn the reference's sampling into data: it returns the
inverse-CDF token (ascending token id) of the probability row it is handed for a recorded uniform u[row, step] and records the
row's kept set; ``torch.sort`` is wrapped to record the top of the temperature-scaled logits the reference sorts.

Recorded (seeds, inputs, results only): a greedy anchor (top_p = 0: ids, cut strings, top-2 margins, compute_scores) and two
sampled runs (top_p 0.8, temperature 1.0 and 0.7: uniforms, ids, kept-set sizes, the top logits and the log-sum-exp of every
sampled row).  generate2 is run on the second sampled run's uniforms and must give generate_batched's ids up to each row's stop.
    python tools/oracle/gen_golden_clipcap.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clipcap_case as cc  # noqa: E402
import refshim  # noqa: E402

torch.set_grad_enabled(False)
refshim.load()
import importlib  # noqa: E402

ep = importlib.import_module("refsrc.clipcap.entrypoint")
from transformers import GPT2Config, GPT2LMHeadModel  # noqa: E402

c = cc.CASE
sd = cc.weights()
x = cc.features()
N, S, K = c["N"], c["entry_length"], c["top_k_recorded"]

ep.GPT2LMHeadModel = type("_LM", (), {"from_pretrained": staticmethod(
    lambda name: GPT2LMHeadModel(GPT2Config(n_layer=c["gpt_layers"], attn_implementation="eager")).eval())})
ep.load_model_with_hf_fallback = lambda local_path, hf_repo_id=None, map_location=None: sd


class Recorder:
    """State of the patched torch.multinomial / torch.sort for one run."""

    def __init__(self, uniforms, sequential=False):
        self.u, self.sequential = uniforms, sequential
        self.row = self.step = 0
        self.kept = np.zeros((N, S), dtype=np.int32)
        self.top_logits = np.zeros((N, S, K), dtype=np.float32)
        self.top_ids = np.zeros((N, S, K), dtype=np.int32)
        self.lse = np.zeros((N, S), dtype=np.float64)
        self.sorted_rows = 0

    def sort(self, logits, descending=True):
        vals, idx = _sort(logits, descending=descending)
        v = vals.reshape(-1)
        if v.numel() == 50257 and descending:
            if self.sequential:
                r, s = self.row, self.step
            else:                                  # generate_batched sorts the active rows of a step in row order, before its multinomial
                r, s = self.pending.pop(0), self.step
            self.top_logits[r, s] = v[:K].numpy()
            self.top_ids[r, s] = idx.reshape(-1)[:K].numpy()
            self.lse[r, s] = float(torch.logsumexp(v.double(), 0))
        return vals, idx

    def multinomial(self, probs, num_samples=1):
        assert num_samples == 1 and probs.dim() == 2
        out = torch.zeros(probs.shape[0], 1, dtype=torch.long)
        for i in range(probs.shape[0]):
            r = self.row if self.sequential else i
            p = probs[i].double().numpy()
            cdf = np.cumsum(p) / p.sum()
            t = int(np.searchsorted(cdf, float(self.u[r, self.step]), side="right"))
            t = min(t, int(np.nonzero(p)[0][-1]))
            out[i, 0] = t
            if self.sequential or self.active[i]:
                self.kept[r, self.step] = int((p > 0).sum())
        return out


_sort, _multinomial = torch.sort, torch.multinomial


def run_batched(head, uniforms):
    """forward_batched under the recorder.  generate_batched keeps its ids to itself: the tokenizer's decode is wrapped to see them."""
    rec = Recorder(uniforms)
    rows = []
    dec = head.tokenizer.decode
    head.tokenizer.decode = lambda ids: (rows.append([int(t) for t in ids]), dec(ids))[1]
    state = {"active": [True] * N}

    def multinomial(probs, num_samples=1):
        rec.active = list(state["active"])
        out = rec.multinomial(probs, num_samples)
        for i in range(N):
            if state["active"][i] and int(out[i, 0]) == head.tokenizer.stop_id:
                state["active"][i] = False
        rec.step += 1
        rec.pending = [i for i in range(N) if state["active"][i]]
        return out

    rec.pending = list(range(N))
    torch.sort, torch.multinomial = rec.sort, multinomial
    try:
        caps = head.forward_batched(x.clone(), compute_scores=False)
    finally:
        torch.sort, torch.multinomial = _sort, _multinomial
        head.tokenizer.decode = dec
    ids = np.full((N, S), -1, dtype=np.int32)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = r
    return caps, ids, rec


def run_sequential(head, uniforms):
    rec = Recorder(uniforms, sequential=True)
    ids = np.full((N, S), -1, dtype=np.int32)

    def multinomial(probs, num_samples=1):
        out = rec.multinomial(probs, num_samples)
        t = int(out[0, 0])
        ids[rec.row, rec.step] = t
        rec.step += 1
        if t == head.tokenizer.stop_id or rec.step == S:
            rec.row, rec.step = rec.row + 1, 0
        return out

    torch.sort, torch.multinomial = rec.sort, multinomial
    try:
        caps = head.forward_sequential(x.clone(), compute_scores=False)
    finally:
        torch.sort, torch.multinomial = _sort, _multinomial
    return caps, ids, rec


def make_head(stop_id, top_p, temperature):
    ep.GPT2Tokenizer = type("_Tok", (), {"from_pretrained": staticmethod(lambda name: cc.StubTokenizer(stop_id))})
    return ep.ClipCapModel({"top_p": top_p, "temperature": temperature, "entry_length": S, "prefix_length": c["prefix_length"],
                            "weight_path": "unused"}, "cpu", dino_feature_dim=c["C"])


out, meta = {}, {"case": {k: (list(v) if isinstance(v, tuple) else v) for k, v in c.items()}}
rng = np.random.default_rng(c["features_seed"] + 1)
u = rng.random((len(c["temperatures"]), N, S)).astype(np.float32)
out["uniforms"] = u

# the stop id: a token the first sampled run does draw -- some row draws it before the end, some row never does
probe = run_batched(make_head(50256, c["top_p"], c["temperatures"][0]), u[0])[1]
stop_id = None

for s in range(5, S - 2):
    for r in range(N):
        t = int(probe[r, s])
        hit = [(probe[q] == t).any() for q in range(N)]
        if not all(hit) and not (probe[:, :5] == t).any():
            stop_id = t
            break
    if stop_id is not None:
        break
assert stop_id is not None
meta["stop_id"], meta["stop_token"] = stop_id, "."

# greedy anchor: top_p = 0 keeps exactly one token, the reference is deterministic
head = make_head(stop_id, 0.0, 1.0)
caps, ids, rec = run_batched(head, np.zeros((N, S), dtype=np.float32))
assert (rec.kept[ids >= 0] == 1).all()
out["greedy_ids"] = ids
out["greedy_margins"] = (rec.top_logits[:, :, 0] - rec.top_logits[:, :, 1]).astype(np.float32)
meta["greedy_captions"] = caps
out["greedy_scores"] = np.array(head.compute_perplexity_scores(caps), dtype=np.float64)

for k, T in enumerate(c["temperatures"]):
    head = make_head(stop_id, c["top_p"], T)
    caps, ids, rec = run_batched(head, u[k])
    assert rec.kept.max() < K, "kept set reaches the recorded top-%d" % K
    out["sampled%d_ids" % k], out["sampled%d_kept" % k] = ids, rec.kept
    out["sampled%d_top_logits" % k], out["sampled%d_top_ids" % k], out["sampled%d_lse" % k] = rec.top_logits, rec.top_ids, rec.lse
    meta["sampled%d_captions" % k] = caps
    stops = [(ids[r] == stop_id).any() for r in range(N)]
    print("T = %.1f: rows that stop: %s, kept sizes %d..%d" % (T, stops, rec.kept[rec.kept > 0].min(), rec.kept.max()))
    if k == 0:
        assert any(stops) and not all(stops)
    if k == len(c["temperatures"]) - 1:            # generate2: the same distribution, the same ids up to each row's stop
        caps2, ids2, rec2 = run_sequential(head, u[k])
        for r in range(N):
            n = int(np.argmax(ids[r] == stop_id)) + 1 if stops[r] else S
            assert (ids2[r, :n] == ids[r, :n]).all() and (rec2.kept[r, :n] == rec.kept[r, :n]).all(), r
        meta["sequential_captions"] = caps2

out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
path = os.path.join(ROOT, "tests", "golden", "clipcap.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes; stop id", stop_id, "greedy", caps if False else meta["greedy_captions"])
