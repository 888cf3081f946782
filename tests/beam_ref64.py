"""Float64 statement of the ViECap beam search (search.py:193-285), for holding the device beam search to
(tests/test_beam_ref64_cpu.py, tests/test_gpu_beam_kernels.py).

Plain torch in float64 and Python lists, written from the reference's lines and the section's wording -- it imports neither
patchioner_amd/viecap.py nor the oracle, so an error shared by the device path and its host restatement cannot hide here.  No test
functions here.

  log_softmax64   x - max - log(sum(exp(x - max)))
  candidates64    the candidates of one selection: first (scores None) lp[0][v]; later stopped[b] ? (v == 0 ? scores[b] / lens[b] : -inf)
                  : (scores[b] + lp[b][v]) / (lens[b] + 1)          (:256-260)
  select_spec     the W largest under the total order "value descending, flat index ascending, NaN never enters", as a sort key
  step_spec       the bookkeeping after one selection, on plain lists (:247-249, :259-276): lens, scores, stop flags, token histories,
                  the key / value table rows, the frozen image (the reference's break) and the clamped position of the next input
  beam64          the whole search on viecap_ref64.GPT2_64 with its KV cache gathered by source beam; per selection the chosen flat
                  indices, the float64 margins between ranks r and r + 1 (r < W) and max |logit|
"""
import math
from typing import Callable, Dict, Iterator, List, Optional, Sequence

import torch

F64 = torch.float64
NEG_INF = float("-inf")


def _d(t) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        return torch.as_tensor(t, dtype=F64)                   # Python floats stay float64 (torch's default would round them to fp32)
    return t.detach().to("cpu", F64)


def log_softmax64(logits) -> torch.Tensor:
    x = _d(logits)
    m = x.max(dim=-1, keepdim=True).values
    z = x - m
    return z - torch.log(torch.exp(z).sum(dim=-1, keepdim=True))


def candidates64(lp, scores=None, lens=None, stopped=None) -> torch.Tensor:
    """lp [W][V] (first selection: [V] or [1][V]) -> the candidate values [rows][V] in float64 (rows = 1 on the first selection)."""
    lp = _d(lp)
    if scores is None:
        return lp.reshape(-1, lp.shape[-1])[:1].clone()
    sc, ln = _d(scores), _d(lens)
    out = (sc[:, None] + lp) / (ln[:, None] + 1.0)
    for b, st in enumerate(list(stopped)):
        if bool(st):
            out[b] = NEG_INF                                   # logits[is_stopped] = -inf; logits[is_stopped, 0] = 0: the score stays,
            out[b, 0] = sc[b] / ln[b]                          # and the length (not incremented for a stopped beam) divides it
    return out


def select_spec(values, W: int, extra: int = 0):
    """The first W + extra candidates of ``values`` (any shape, read flat) under the total order: larger value first, equal values by
    the lower flat index, NaN never enters -> (values, flat indices) as lists.  Fewer candidates than asked for: (-inf, -1) fills up.
    The order is a sort key; candidates below the (W + extra)-th largest value cannot be among the first W + extra and are left out of
    the sort (a cut by value alone, which keeps every tie with the last rank)."""
    v = _d(values).reshape(-1)
    k = W + extra
    ok = ~torch.isnan(v)
    idx = ok.nonzero().flatten()
    if idx.numel() > 4 * k:
        thr = torch.where(ok, v, torch.full_like(v, NEG_INF)).topk(k).values[-1]
        idx = (ok & (v >= thr)).nonzero().flatten()
    vals = v[idx].tolist()
    order = sorted(range(len(vals)), key=lambda i: (-vals[i], int(idx[i])))[:k]
    out_v = [vals[i] for i in order] + [NEG_INF] * (k - len(order))
    out_i = [int(idx[i]) for i in order] + [-1] * (k - len(order))
    return out_v, out_i


def new_state(W: int, P: int, steps: int, r0: int = 0, tstride: Optional[int] = None) -> Dict:
    """The state of one image before its first selection: rows r0 .. r0 + W - 1; table: positions < P the shared prompt row r0, later
    positions the row's own slot."""
    st = dict(W=W, P=P, r0=r0, steps=steps, scores=[0.0] * W, lens=[0.0] * W, stopped=[0] * W, tok=[0] * W,
              hist=[[-1] * steps for _ in range(W)], tab=None)
    if tstride is not None:
        st["tab"] = [[r0 if j < P else r0 + b for j in range(tstride)] for b in range(W)]
    return st


def step_spec(state: Dict, step: int, vals: Optional[Sequence[float]], flat: Optional[Sequence[int]], V: int, eos: Sequence[int], npos: int,
              mul: Callable[[float, float], float] = lambda a, b: a * b) -> Dict:
    """The state after selection ``step`` chose ``flat`` (values ``vals``): a new dict, the old one untouched.  ``mul``: the product
    behind scores = average x length (float64 here; the device's is one fp32 multiplication).  An image whose beams had all stopped
    before a later step is frozen: nothing but ``xpos`` is new (vals / flat are not read).  Extra keys: src [W] (None on step 0 / frozen),
    frozen, xpos = min(P + step, npos - 1), the position whose row of wpe the next input adds to wte[tok]."""
    W, P = state["W"], state["P"]
    new = dict(state)
    new["xpos"] = min(P + step, npos - 1)
    new["src"], new["frozen"] = None, False
    if step == 0:
        toks = [int(f) for f in flat]                                          # :247 scores, next_tokens = logits.topk(beam_width)
        new["scores"] = [float(v) for v in vals]
        new["lens"] = [1.0] * W
        new["stopped"] = [int(t in eos) for t in toks]                          # :276
        new["tok"] = toks
        new["hist"] = [[t] + list(h[1:]) for t, h in zip(toks, state["hist"])]
        return new
    if all(state["stopped"]):
        new["frozen"] = True                                                   # :277 break
        return new
    grown = [l if s else l + 1.0 for l, s in zip(state["lens"], state["stopped"])]       # :259 seq_lengths[~is_stopped] += 1
    src = [int(f) // V for f in flat]                                                    # :263
    toks = [int(f) % V for f in flat]                                                    # :265
    new["lens"] = [grown[s] for s in src]                                                # :264
    new["scores"] = [mul(float(v), l) for v, l in zip(vals, new["lens"])]                # :270
    new["stopped"] = [int(bool(state["stopped"][s]) or t in eos) for s, t in zip(src, toks)]     # :271, :276
    new["tok"] = toks
    new["hist"] = [list(state["hist"][s][:step]) + [t] + list(state["hist"][b][step + 1:]) for b, (s, t) in enumerate(zip(src, toks))]  # :267-268
    if state["tab"] is not None:
        pos = P + step - 1                                                     # the position this step's rows wrote: history is 0 .. pos
        new["tab"] = [list(state["tab"][s][:pos + 1]) + list(state["tab"][b][pos + 1:]) for b, s in enumerate(src)]     # :269 generated[src]
    new["src"] = src
    return new


def beam64_steps(model, embeds, W: int, steps: int, eos: Sequence[int]) -> Iterator[Dict]:
    """The search, one selection per item: dict(step, lp [rows][V] float64 log-probabilities the selection read (rows = 1 on step 0),
    flat [W], vals [W], margins [W] (value of rank r minus value of rank r + 1; inf where there is no rank r + 1), amax = max |logit|,
    state = step_spec's result).  Ends after ``steps`` selections or when every beam has stopped."""
    x = _d(embeds)
    P = x.shape[0]
    V, npos = model.V, model.wpe.shape[0]
    h, cache = model.forward((x + model.wpe[:P])[None])
    state = new_state(W, P, steps)
    for i in range(steps):
        if i > 0 and all(state["stopped"]):
            return
        if i == 1:
            cache = [(k.expand(W, -1, -1, -1), v.expand(W, -1, -1, -1)) for k, v in cache]
        if i > 0:
            if state["src"] is not None:
                src = torch.tensor(state["src"])
                cache = [(k[src], v[src]) for k, v in cache]                    # :269 generated = generated[next_tokens_source]
            tok = torch.tensor(state["tok"])
            h, cache = model.forward((model.wte[tok] + model.wpe[P + i - 1])[:, None], cache)
        lg = model.logits(h[:, -1])
        lp = log_softmax64(lg)
        cand = candidates64(lp) if i == 0 else candidates64(lp, state["scores"], state["lens"], state["stopped"])
        vals, flat = select_spec(cand, W, extra=1)
        margins = [vals[r] - vals[r + 1] if flat[r + 1] >= 0 and vals[r] > NEG_INF else math.inf for r in range(W)]
        state = step_spec(state, i, vals[:W], flat[:W], V, eos, npos)
        yield dict(step=i, lp=lp, flat=flat[:W], vals=vals[:W], margins=margins, amax=float(lg.abs().max()), state=state)


def beam64(model, embeds, W: int, steps: int, eos: Sequence[int]) -> Dict:
    """-> dict(ids [W] token lists cut at the beam's length, lens [W], scores [W] = accumulated score / length, in the order of the last
    selection; flat / margins / amax: one entry per selection made)."""
    flat, margins, amax, state = [], [], [], None
    for rec in beam64_steps(model, embeds, W, steps, eos):
        flat.append(rec["flat"])
        margins.append(rec["margins"])
        amax.append(rec["amax"])
        state = rec["state"]
    n = len(flat)
    lens = [int(l) for l in state["lens"]]
    return dict(ids=[list(h[:min(l, n)]) for h, l in zip(state["hist"], lens)], lens=lens,
                scores=[s / l for s, l in zip(state["scores"], state["lens"])], flat=flat, margins=margins, amax=amax)
