"""Float64 statements of the decoder's layer GEMMs and of its single-query attention (csrc/decoder.hip), the error bars the kernels
are held to, and the inputs both test files share (tests/test_decoder_ref64_cpu.py, tests/test_gpu_decoder_kernels.py).

Plain torch on the CPU; nothing here calls the package's kernels.  No test functions here.

References
  layer_gemm64   LN(x) W^T + b with two-pass statistics (or x W^T + b), then store / gelu_new / += old out / + extra row
  attention64    softmax(q . k_j / sqrt(hd)) over the keys 0 .. pos of one row and head, times the values, for any hd

Bars.  A bar is a function of float64 quantities of the CASE (inputs, weights, the float64 result), never of the device output, so it
cannot follow a wrong kernel.  Constants as in tests/test_gpu_viecap_kernels.py: u = U32 = 2^-24 for fp32 operands and accumulation,
U_SPLIT16 = 2^-22 where an operand is carried as a pair of fp16 numbers (k_dec_gemm_s), SAFETY = 8 over the random-walk estimate.

Layer GEMM, plain form  y = sum_k x_k w_k + b (+ old | + extra), S = sum_k |x_k| |w_k|:
  dot product     sqrt(K) u_dot S      K roundings of random sign, each relative to a partial sum below S; u_dot = U_SPLIT16 for the split
                                       kernel (both operands carry 22 bits; the dropped lo' lo' term is 2^-22 of a product)
  partial sums    u (S + |b|)          the wave / slab partials are added in fp32, then the bias
  epilogue        3 u |out|            the residual add (or + extra) and the store
Layer GEMM, LayerNorm form  y = r (s - mu c) + d,  s = x . w' (w' = W ln_w), r = 1 / sqrt(var + eps), A = sum_k |w'_k|:
  dot product     r sqrt(K) u_dot S'   S' = sum |x_k| |w'_k|   (w' itself is an fp32 product: u S', inside the term)
  mean            r sqrt(K) u m1 A     m1 = mean |x_k| bounds the error of the fp32 sum behind mu (|mu| <= m1), times |c| <= A; c's own
                                       rounding u |mu| |c| is inside it
  variance        (u E[x^2] / (var + eps)) / 2 |y - d|
                                       the kernels take var = E[x^2] - mu^2 in ONE pass.  Both sums are reduced as trees (a few values per
                                       lane, then lanes, then waves: depth about log2 K), so E[x^2] and mu^2 each carry a few u of E[x^2]
                                       (the squares' own roundings, sqrt(depth) u from the tree, twice mu's for mu^2), which SAFETY covers;
                                       the difference keeps that absolute error, so var + eps is off by the factor E[x^2] / (var + eps)
                                       more (1 for centred rows, 1 + mu^2 / var for rows with a common offset), and
                                       r = (var + eps)^-1/2 by half of it; r multiplies y - d
  rsqrtf          2 u |y - d|
  epilogue        u |d| + 3 u |y|      d is rounded once at load; multiply, subtract, add
  gelu_new        g(v) = v (1 + tanh(.)) / 2: |g'| <= 1.13 carries the bar of v, plus 4 u (|v| + |g|) for tanhf and the two products

Attention, one row and head, keys j = 0 .. pos, T_j = sum_c |q_c| |k_jc|, s_j = q . k_j / sqrt(hd):
  scores          a score is off by sqrt(hd) u T_j / sqrt(hd) = u T_j (the dot product, then the scale), the exponent's argument by
                  another u |s_j - max s|: delta = u (max_j T_j + max_j |s_j - max s|)
  probabilities   p_j = exp(s_j - max) / sum: off by the factor 2 delta + 4 u (numerator and normaliser; expf, the division)
  weighted sum    sqrt(keys) u for the fp32 sum of keys terms, + 2 u for the partial sums that meet in LDS
  out[c] is a convex combination of v_j[c]:  bar = SAFETY (2 delta + (sqrt(keys) + 6) u) max_j |v_j[c]|

Inputs (x_family): (i) unit Gaussian rows; (ii) rows scaled 1e-3 .. 1e3; (iii) "massive channels" 64 / 383 / 700 carrying 1e2, 3e2,
-1e3, and rows with a common offset of 10 standard deviations (mu^2 / var = 1e2: what strains the one-pass variance).  The weights
(layer_case) are GPT-2 sized Gaussians, except rows 5, 6 and 7, which are positive throughout: with the offset rows every product of
such a dot product has one sign, so an operand that is biased (an fp16 cut toward zero without its low half) cannot hide in a sum of
random signs.
"""
import math
from typing import Dict, Optional

import torch

F64 = torch.float64
U32, U_SPLIT16, SAFETY = 2.0 ** -24, 2.0 ** -22, 8.0
E = 768
MASSIVE = ((64, 1e2), (383, 3e2), (700, -1e3))
# name -> (Nout, K, epilogue, LayerNorm): the four GEMMs of a layer and the prefix projection (epilogue numbers: the hook's PIO_DEC_EPI_*)
STORE, RESID, GELU, EMBED = 0, 1, 2, 3
GEMMS = {"qkv": (2304, 768, STORE, True), "proj": (768, 768, RESID, False), "fc": (3072, 768, GELU, True), "fc2": (768, 3072, RESID, False)}


def _d(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to("cpu", F64)


def gelu_new64(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x.pow(3))))


# ------------------------------------------------------------------------------------------------ inputs
def layer_case(name: str, seed: int = 0, K: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """fp32 parameters of one GEMM: W [Nout][K] ([out][in]), b [Nout], and for the LayerNorm forms ln_w, ln_b [K]; "embed": the prefix
    projection from K inputs with the position row ``extra`` [Nout]."""
    if name == "embed":
        Nout, K_, epi, ln = E, int(K), EMBED, False
    else:
        Nout, K_, epi, ln = GEMMS[name]
    g = torch.Generator().manual_seed(1000 * seed + K_ + 7 * Nout + epi)
    W = torch.randn(Nout, K_, generator=g) * 0.05
    W[5:8] = W[5:8].abs()
    c = {"name": name, "Nout": Nout, "K": K_, "epi": epi, "ln": ln, "eps": 1e-5, "W": W.contiguous(),
         "b": (0.1 * torch.randn(Nout, generator=g)).contiguous()}
    if ln:
        c["ln_w"] = (1.0 + 0.2 * torch.randn(K_, generator=g)).contiguous()
        c["ln_b"] = (0.1 * torch.randn(K_, generator=g)).contiguous()
    if epi == EMBED:
        c["extra"] = (0.02 * torch.randn(Nout, generator=g)).contiguous()
    return c


def x_family(family: str, N: int, K: int, seed: int = 0) -> torch.Tensor:
    """fp32 rows [N][K]: "unit", "scales" (row n times 10^(-3 .. 3)), "massive" (even rows: three huge channels; odd rows: a common
    offset of 10 standard deviations), "split_edges" (the split kernel's range cases: rows of 1e-6 and 1e8 among ordinary ones)."""
    g = torch.Generator().manual_seed(77 * seed + N + 3 * K + len(family))
    x = torch.randn(N, K, generator=g)
    if family == "unit":
        pass
    elif family == "scales":
        x *= (10.0 ** (torch.arange(N) % 7 - 3.0))[:, None]
    elif family == "massive":
        for c, a in MASSIVE:
            x[0::2, c % K] += a
        x[1::2] += 10.0
        x[3::4] *= -1.0
    elif family == "split_edges":
        x *= torch.tensor([1.0, 1e-6, 1e8, 1.0, 3e4, 1e-3, 1.0, 1e-6])[torch.arange(N) % 8][:, None]
    else:
        raise ValueError(family)
    return x.contiguous()


FAMILIES = ("unit", "scales", "massive")


# ------------------------------------------------------------------------------------------------ layer GEMM
def layer_gemm64(c: Dict[str, torch.Tensor], x: torch.Tensor, old: Optional[torch.Tensor] = None):
    """(out, bar(u_dot) -> tensor) in float64 for the case's epilogue.  RESID adds onto ``old`` [N][Nout]."""
    x, W, b = _d(x), _d(c["W"]), _d(c["b"])
    K = W.shape[1]
    rk = math.sqrt(K)
    if c["ln"]:
        lw, lb, eps = _d(c["ln_w"]), _d(c["ln_b"]), float(c["eps"])
        mu = x.mean(-1, keepdim=True)
        xc = x - mu
        var = (xc * xc).mean(-1, keepdim=True)
        r = 1.0 / torch.sqrt(var + eps)
        v = (xc * r * lw + lb) @ W.T + b                       # the unfolded statement
        wf = W * lw
        d = W @ lb + b
        S = x.abs() @ wf.abs().T
        A = wf.abs().sum(-1)
        m1 = x.abs().mean(-1, keepdim=True)
        ex2 = (x * x).mean(-1, keepdim=True)
        cond = ex2 / (var + eps)
        yd = (v - d).abs()

        def pre_bar(u_dot):
            return r * rk * (u_dot * S + U32 * m1 * A) + (0.5 * U32 * cond + 2 * U32) * yd + U32 * (d.abs() + 3 * v.abs())
    else:
        v = x @ W.T + b
        S = x.abs() @ W.abs().T

        def pre_bar(u_dot):
            return rk * u_dot * S + U32 * (S + b.abs())
    epi = c["epi"]
    if epi == STORE:
        out = v
        bar = lambda u=U32: SAFETY * pre_bar(u)                                                     # noqa: E731
    elif epi == GELU:
        out = gelu_new64(v)
        bar = lambda u=U32: SAFETY * (1.13 * pre_bar(u) + 4 * U32 * (v.abs() + out.abs()))          # noqa: E731
    elif epi == RESID:
        out = _d(old) + v
        bar = lambda u=U32: SAFETY * (pre_bar(u) + 3 * U32 * out.abs())                             # noqa: E731
    elif epi == EMBED:
        out = v + _d(c["extra"])
        bar = lambda u=U32: SAFETY * (pre_bar(u) + 3 * U32 * out.abs())                             # noqa: E731
    else:
        raise ValueError(epi)
    return out, bar


def fold64(c):
    """The loader's fold (csrc/api.cpp: ln_fold_host) restated: w' = fp32(W ln_w); c, d summed in float64 and rounded once."""
    W, lw, lb, b = c["W"], c["ln_w"], c["ln_b"], c["b"]
    wf = (W * lw).float()
    cv = wf.double().sum(-1).float()
    dv = (W.double() @ lb.double() + b.double()).float()
    return wf.contiguous(), cv.contiguous(), dv.contiguous()


def worst_ratio(got: torch.Tensor, ref: torch.Tensor, bar: torch.Tensor) -> float:
    """max |got - ref| / bar over the elements whose reference is finite; a non-finite ``got`` there counts as infinitely wrong."""
    ok = torch.isfinite(ref)
    err = (got.double() - ref).abs()[ok]
    if err.numel() == 0:
        return 0.0
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return float((err / bar[ok]).max())


# ------------------------------------------------------------------------------------------------ attention
def attention64(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int):
    """q [E]; k, v [keys][E], the newest key / value last -> (out [E], bar [E]) in float64."""
    q, k, v = _d(q), _d(k), _d(v)
    keys, E_ = k.shape
    hd = E_ // heads
    qh, kh, vh = q.view(heads, hd), k.view(keys, heads, hd), v.view(keys, heads, hd)
    s = torch.einsum("hc,jhc->hj", qh, kh) / math.sqrt(hd)
    p = torch.softmax(s, dim=-1)
    out = torch.einsum("hj,jhc->hc", p, vh)
    T = torch.einsum("hc,jhc->hj", qh.abs(), kh.abs())
    delta = U32 * (T.max(-1).values + (s - s.max(-1, keepdim=True).values).abs().max(-1).values)        # [heads]
    bar = SAFETY * (2 * delta[:, None] + (math.sqrt(keys) + 6) * U32) * vh.abs().max(0).values
    return out.reshape(E_), bar.reshape(E_)


def attn_case(seed: int, N: int, heads: int, max_steps: int, rows: Optional[int] = None, spread: float = 0.0):
    """fp32 qkv [rows][3E], kcache / vcache [N][max_steps][E] of Gaussians (a different cache per row); ``spread`` > 0: the queries and
    keys are scaled so that |q . k| / sqrt(hd) is about ``spread``."""
    g = torch.Generator().manual_seed(31 * seed + heads + 5 * N)
    rows = N if rows is None else rows
    qkv = torch.randn(rows, 3 * E, generator=g)
    kc = torch.randn(N, max_steps, E, generator=g)
    vc = torch.randn(N, max_steps, E, generator=g)
    if spread > 0:
        a = math.sqrt(spread)
        qkv[:, :2 * E] *= a
        kc *= a
    return qkv.contiguous(), kc.contiguous(), vc.contiguous()
