"""Float64 statements of the ViECap head's numerics, for holding its HIP kernels to (tests/test_gpu_viecap_kernels.py).

Plain torch in float64, written from the published architectures and the docstrings of patchioner_amd/viecap.py and
csrc/viecap.hip -- NOT the oracle (oracle/patchioner_oracle.py evaluates in fp32): a kernel's error is measured against these,
not against another fp32 summation order.  No test functions here.

  mapping64        ClipCap's MappingNetwork: feats / |feats|, Linear C -> Lp x E, cat prefix_const, pre-LN transformer layers
                   (8 heads, bias-free q and kv, ReLU MLP, LayerNorm eps 1e-5), the last Lc positions
  entity_probs64   softmax((f / |f|) (e / |e|)^T / T) and its log
  gpt2_nll64       teacher-forced sum of -log p(t[p+1] | t[..p]) under GPT-2 (two-pass LayerNorm)
  gpt2_greedy64    greedy ids from prompt embeddings, with the top-2 logit margin of every step
  select_reference the entities k_compose_prompts picks: larger first, NaN first, ties by the lower index, cut at the first
                   value below the threshold compared as the reference compares (a 0-d fp32 tensor against a Python float)
"""
import math
from typing import Dict, List, Sequence

import torch

F64 = torch.float64


def _d(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to("cpu", F64)


def layer_norm64(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float) -> torch.Tensor:
    """Two-pass LayerNorm: mean, then the mean of the squared deviations (biased, eps inside the root)."""
    mu = x.mean(-1, keepdim=True)
    c = x - mu
    var = (c * c).mean(-1, keepdim=True)
    return c / torch.sqrt(var + eps) * w + b


# ------------------------------------------------------------------------------------------------ mapping network
def mapping64(w: Dict[str, torch.Tensor], feats: torch.Tensor, heads: int = 8, eps: float = 1e-5) -> torch.Tensor:
    """MappingNetwork (ClipCap): w the ``mapping_network.*`` entries of a ViECap state dict, feats [N, C] -> soft prompt [N, Lc, E]."""
    p = "mapping_network."
    x = _d(feats)
    x = x / x.norm(dim=-1, keepdim=True)
    lw, lb, pc = _d(w[p + "linear.weight"]), _d(w[p + "linear.bias"]), _d(w[p + "prefix_const"])
    Lc, E = pc.shape
    Lp = lw.shape[0] // E
    N = x.shape[0]
    h = (x @ lw.T + lb).view(N, Lp, E)
    h = torch.cat([h, pc.expand(N, Lc, E)], dim=1)
    S, hd = Lp + Lc, E // heads
    layer = 0
    while (p + "transformer.layers.%d.norm1.weight" % layer) in w:
        q_ = p + "transformer.layers.%d." % layer
        g = lambda k: _d(w[q_ + k])                                           # noqa: E731
        y = layer_norm64(h, g("norm1.weight"), g("norm1.bias"), eps)
        q = (y @ g("attn.to_queries.weight").T).view(N, S, heads, hd)
        kv = (y @ g("attn.to_keys_values.weight").T).view(N, S, 2, heads, hd)
        k, v = kv[:, :, 0], kv[:, :, 1]
        a = torch.einsum("nihd,njhd->nhij", q, k) / math.sqrt(hd)
        a = torch.softmax(a, dim=-1)
        o = torch.einsum("nhij,njhd->nihd", a, v).reshape(N, S, E)
        h = h + (o @ g("attn.project.weight").T + g("attn.project.bias"))
        y = layer_norm64(h, g("norm2.weight"), g("norm2.bias"), eps)
        y = torch.relu(y @ g("mlp.fc1.weight").T + g("mlp.fc1.bias"))
        h = h + (y @ g("mlp.fc2.weight").T + g("mlp.fc2.bias"))
        layer += 1
    return h[:, Lp:]


# ------------------------------------------------------------------------------------------------ entity probabilities
def entity_probs64(feats: torch.Tensor, emb: torch.Tensor, T: float):
    """(probabilities [N, K], log-probabilities [N, K]) of softmax(cos(f, e) / T)."""
    f, e = _d(feats), _d(emb)
    f = f / f.norm(dim=-1, keepdim=True)
    e = e / e.norm(dim=-1, keepdim=True)
    logits = (f @ e.T) / float(T)
    logp = torch.log_softmax(logits, dim=-1)
    return logp.exp(), logp


# ------------------------------------------------------------------------------------------------ GPT-2
def _gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x.pow(3))))


class GPT2_64:
    """GPT2LMHeadModel (tied head, gelu_new, causal softmax(q k^T / sqrt(hd)), LayerNorm eps 1e-5) in float64 over the ``gpt.*``
    entries of a ViECap state dict.  Rows of wte that are exactly zero give a logit of exactly 0: the head multiplies only the others."""

    def __init__(self, w: Dict[str, torch.Tensor], heads: int = 12, eps: float = 1e-5):
        self.w = {k[4:]: _d(v) for k, v in w.items() if k.startswith("gpt.")}
        self.heads, self.eps = heads, eps
        self.wte, self.wpe = self.w["transformer.wte.weight"], self.w["transformer.wpe.weight"]
        self.V, self.E = self.wte.shape
        self.layers = 0
        while ("transformer.h.%d.ln_1.weight" % self.layers) in self.w:
            self.layers += 1
        self.live = (self.wte != 0).any(dim=1).nonzero().flatten()
        self.wte_live = self.wte[self.live]

    def logits(self, h: torch.Tensor) -> torch.Tensor:
        """Final LayerNorm + tied head of hidden rows h [..., E] -> [..., V]."""
        w = self.w
        y = layer_norm64(h, w["transformer.ln_f.weight"], w["transformer.ln_f.bias"], self.eps)
        out = torch.zeros(*y.shape[:-1], self.V, dtype=F64)
        out[..., self.live] = y @ self.wte_live.T
        return out

    def forward(self, x: torch.Tensor, cache=None):
        """x [N, P, E] input embeddings (position embeddings already added) after the cached positions -> (hidden [N, P, E], cache)."""
        w, H = self.w, self.heads
        N, P, E = x.shape
        hd = E // H
        cache = cache if cache is not None else [None] * self.layers
        new = []
        for l in range(self.layers):
            p = "transformer.h.%d." % l
            y = layer_norm64(x, w[p + "ln_1.weight"], w[p + "ln_1.bias"], self.eps)
            qkv = y @ w[p + "attn.c_attn.weight"] + w[p + "attn.c_attn.bias"]
            q, k, v = (t.reshape(N, P, H, hd).transpose(1, 2) for t in qkv.split(E, dim=-1))
            if cache[l] is not None:
                k = torch.cat([cache[l][0], k], dim=2)
                v = torch.cat([cache[l][1], v], dim=2)
            new.append((k, v))
            T = k.shape[2]
            a = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
            mask = torch.ones(P, T, dtype=torch.bool).tril(T - P)            # query i (absolute T - P + i) sees keys <= itself
            a = a.masked_fill(~mask, float("-inf")).softmax(-1)
            o = (a @ v).transpose(1, 2).reshape(N, P, E)
            x = x + (o @ w[p + "attn.c_proj.weight"] + w[p + "attn.c_proj.bias"])
            y = layer_norm64(x, w[p + "ln_2.weight"], w[p + "ln_2.bias"], self.eps)
            y = _gelu_new(y @ w[p + "mlp.c_fc.weight"] + w[p + "mlp.c_fc.bias"])
            x = x + (y @ w[p + "mlp.c_proj.weight"] + w[p + "mlp.c_proj.bias"])
        return x, new


def gpt2_nll64(w, rows: Sequence[Sequence[int]], model: GPT2_64 = None):
    """Teacher-forced sum over p + 1 < len of -log softmax(logits(t[..p]))[t[p+1]] per row -> (nll [N] float64, 0 for rows of length
    < 2; the largest |logit| of each row's scored positions [N] float64).  Ids outside [0, V) are clamped, as the device clamps them."""
    m = model or GPT2_64(w)
    out = torch.zeros(len(rows), dtype=F64)
    amax = torch.zeros(len(rows), dtype=F64)
    for i, r in enumerate(rows):
        if len(r) < 2:
            continue
        t = torch.tensor([min(max(int(v), 0), m.V - 1) for v in r])
        x = m.wte[t] + m.wpe[:len(t)]
        h, _ = m.forward(x[None])
        lg = m.logits(h[0, :-1])
        amax[i] = lg.abs().max()
        logp = torch.log_softmax(lg, dim=-1)
        out[i] = -logp.gather(1, t[1:, None]).sum()
    return out, amax


def gpt2_greedy64(w, embeds: torch.Tensor, steps: int, model: GPT2_64 = None):
    """Greedy search from prompt embeddings [N, P, E] (positions 0..P-1, then one generated token per step) -> (ids [N, steps] int64,
    top-2 logit margins [N, steps] float64, the largest |logit| seen per row [N] float64).  Ties go to the lower id."""
    m = model or GPT2_64(w)
    x = _d(embeds)
    N, P, _ = x.shape
    h, cache = m.forward(x + m.wpe[:P])
    ids, margins = [], []
    amax = torch.zeros(N, dtype=F64)
    for s in range(steps):
        lg = m.logits(h[:, -1])
        amax = torch.maximum(amax, lg.abs().max(dim=1).values)
        top = lg.topk(2, dim=-1).values
        nxt = lg.argmax(dim=-1)                                               # first occurrence of the maximum
        ids.append(nxt)
        margins.append(top[:, 0] - top[:, 1])
        if s + 1 < steps:
            h, cache = m.forward((m.wte[nxt] + m.wpe[P + s])[:, None], cache)
    return torch.stack(ids, 1), torch.stack(margins, 1), amax


# ------------------------------------------------------------------------------------------------ entity selection
def select_reference(probs_row, top_k: int, threshold: float) -> List[int]:
    """Indices of the entities the hard prompt names, in order.  Order: NaN before any number, larger first, equal values by the lower
    index (written out as a sort key, not through torch.sort / torch.topk).  Cut: at the first of the top_k whose value is below the
    threshold, compared as top_k_categories compares -- ``vals[j] < threshold`` with vals an fp32 tensor and threshold a Python float.
    A NaN is not below the threshold."""
    p = torch.as_tensor(probs_row, dtype=torch.float32).reshape(-1)
    vals = p.tolist()
    order = sorted(range(len(vals)), key=lambda i: (0, 0.0, i) if math.isnan(vals[i]) else (1, -vals[i], i))
    out = []
    for i in order[:top_k]:
        if bool(p[i] < threshold):
            break
        out.append(i)
    return out
