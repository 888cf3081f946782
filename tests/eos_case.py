"""Seeded weights whose greedy decode EMITS its end token, and the canonical id table of stop_at_eos, in numpy.

With the plain seeded weights (patchioner_amd.weights.synth_*) no row ever emits an end token, so a decode that stops once every
caption has ended has nothing to stop on.  The recipe: add a ramp ``gamma * p * e`` to row ``p`` of the position table ``wpe``, where
``e`` is the unit vector of the end token's embedding row.  The LM head is tied to that table, so the end token's logit grows with the
position until it wins; every row stops, each at a column of its own.

DeCap (``decap_weights`` / ``decap_prefixes``): ``synth_decap(2, prefix_size=768, n_layer=4)``, 16 prefixes of seed 102, 30 steps, 4 heads, end token 49407.
First end-of-text column of every row and the smallest top-2 logit margin up to the stop, from DeCapOracle (held in
tests/test_stop_at_eos_cpu.py):

    gamma 0.3   [15,16,16,18,16,15,14,17,17,17,15,14,17,17,18,14]   1.09e-3
    gamma 0.6   [9,8,8,9,8,7,7,8,9,8,8,7,8,8,9,7]                   1.94e-3
    gamma 1.5   [4,3,4,3,4,3,3,3,4,3,3,3,3,3,4,3]                   1.94e-3
    gamma 0.15  rows 10 and 15 stop at 26 and 28, the other 14 never
    gamma 0     no row stops

The decoder's fixtures are decoded bit-exactly at margins of 1.9e-4, so ids at these margins are the oracle's.

ViECap (``viecap_case``): ``synth_viecap`` with 2 GPT-2 layers, the ramp aimed at the embedding of the tokenizer's "." and starting at
the prompt length of the shorter of the two prompts the case offers.
"""
import numpy as np
import torch

from patchioner_amd import weights as W

DECAP_EOT = 49407
DECAP_STEPS = 30
DECAP_FIRST = {
    0.3: [15, 16, 16, 18, 16, 15, 14, 17, 17, 17, 15, 14, 17, 17, 18, 14],
    0.6: [9, 8, 8, 9, 8, 7, 7, 8, 9, 8, 8, 7, 8, 8, 9, 7],
    1.5: [4, 3, 4, 3, 4, 3, 3, 3, 4, 3, 3, 3, 3, 3, 4, 3],
    0.15: [30] * 10 + [26] + [30] * 4 + [28],
}


def first_stop(ids, stop_ids):
    """[N] first column of every row of ids [N, steps] that holds one of ``stop_ids``; ``steps`` where there is none."""
    ids = np.asarray(ids)
    hit = np.isin(ids, np.asarray(list(stop_ids)))
    return np.where(hit.any(axis=1), hit.argmax(axis=1), ids.shape[1]).astype(np.int64)


def canon_ids(ids, stop_ids):
    """canon(ids): row n unchanged up to and including its first stop column f_n, ids[n][f_n] in every later column; a row without a
    stop id unchanged."""
    ids = np.asarray(ids)
    out = ids.copy()
    for n, f in enumerate(first_stop(ids, stop_ids)):
        if f < ids.shape[1]:
            out[n, f + 1:] = ids[n, f]
    return out


def steps_run(first, steps, seg):
    """Steps a decode in segments of ``seg`` runs when its rows first stop at columns ``first``: whole segments up to the one that holds
    the last row's stop, all ``steps`` when a row never stops."""
    last = int(np.max(first))
    if last >= steps:
        return steps
    return min(steps, seg * -(-(last + 1) // seg))


def _ramp(w, key, token, gamma, start=0):
    wte = w[key + "wte.weight"]
    e = wte[token] / wte[token].norm()
    wpe = w[key + "wpe.weight"].clone()
    p = torch.arange(wpe.shape[0] - start, dtype=torch.float32)
    wpe[start:] += gamma * p[:, None] * e[None, :]
    w[key + "wpe.weight"] = wpe
    return w


def decap_weights(gamma, n_layer=4):
    return _ramp(W.synth_decap(2, prefix_size=768, n_layer=n_layer), "decoder.transformer.", DECAP_EOT, gamma)


def decap_prefixes(n=16):
    return torch.randn(16, 768, generator=torch.Generator().manual_seed(102))[:n].contiguous()


# ---- ViECap -------------------------------------------------------------------------------------------------------------------------
VIECAP = dict(seed_w=311, seed_x=312, layers=2, Lc=10, Lt=(3, 7), N=3, steps=64)
VIECAP_GAMMA = 0.3                                    # chosen with the oracle: margins up to the stops >= 2.9e-3
VIECAP_FIRST = {0: [7, 3, 10], 1: [6, 6, 3]}          # first full-stop column of the 3 rows, per prompt length (13 and 17 positions)


def viecap_tokenizer():
    from patchioner_amd import viecap as V
    vocab, merges = W.synth_bpe(0)
    return V.ByteLevelBPE(vocab, merges)


def viecap_eos(tok):
    return [tok.encode(e)[-1] for e in (".", " .")]           # VieCapHead.eos (search.py:141)


def viecap_case(gamma, which=0, n=None):
    """(weights, soft prompt [n, Lc, 768], hard-prompt token rows [n, Lt] int32, stop ids) of the ViECap case; ``which`` picks one of
    the two hard-prompt lengths.  The ramp starts at the SHORTER prompt's length, so the longer prompt stops earlier."""
    c = VIECAP
    tok = viecap_tokenizer()
    eos = viecap_eos(tok)
    w = W.synth_viecap(c["seed_w"], n_layer=c["layers"], tok_vocab=len(tok))
    w = _ramp(w, "gpt.transformer.", eos[0], gamma, start=c["Lc"] + c["Lt"][0])
    w["gpt.lm_head.weight"] = w["gpt.transformer.wte.weight"]
    g = torch.Generator().manual_seed(c["seed_x"] + which)
    n = c["N"] if n is None else n
    cont = (torch.randn(c["N"], c["Lc"], 768, generator=g) * 0.5)[:n].contiguous()
    tokens = torch.randint(0, len(tok), (c["N"], c["Lt"][which]), generator=g).to(torch.int32)[:n].contiguous()
    return w, cont, tokens, eos


def viecap_oracle_ids(orc_gpt, cont, tokens, steps=64):
    """Greedy ids [n, steps] and top-2 margins of the oracle's cached GPT-2 (DeCapOracle over the gpt.* weights) on the prompt
    (soft prompt, then the tokens' embeddings): greedy_search without its cut."""
    wte = orc_gpt.w["decoder.transformer.wte.weight"]
    emb = torch.cat((cont, wte[tokens.long()]), dim=1)
    ids, margins = [], []
    logits, past = orc_gpt.gpt2_logits_cached(emb)
    for step in range(steps):
        nxt = logits.argmax(-1, keepdim=True)
        t2 = logits.topk(2, dim=-1).values
        ids.append(nxt)
        margins.append((t2[:, 0] - t2[:, 1])[:, None])
        if step + 1 < steps:
            logits, past = orc_gpt.gpt2_logits_cached(wte[nxt], past)
    return torch.cat(ids, 1), torch.cat(margins, 1)
