"""Float64 statements of the exact-fp32 kernels -- k_sgemm_tn, k_layernorm_f32, k_activation_f32 (csrc/viecap.hip), k_attention_f32,
k_im2col_f32, k_embed_scatter_f32, k_resid_ls_f32, k_gelu_f32 (csrc/vit_fp32.hip), k_text_attention_f32, k_text_embed, k_text_pool
(csrc/text_encoder.hip) -- and the error bars they are held to, for tests/test_fp32_ref64_cpu.py and tests/test_gpu_fp32_kernels.py.
Plain torch on whatever device the operands live on; nothing here calls the package's kernels.  No test functions here.

Every function starts from the fp32 values the kernel is handed (scalars rounded to fp32 first, as the C ABI passes them), does
everything after that in float64, and returns the value AND the magnitudes its bar is made of.  A bar is a function of float64 quantities
of the case, never of the device output, so it cannot follow a wrong kernel; none is tuned to what a kernel happens to produce.

Bars.  u = 2^-24 (one rounding of a normal fp32 result, relative).  SUB = 2^-126 is added where a result can be subnormal (a flushed or
gradually underflowed value is off by less than the smallest normal number).  expf / erff / tanhf are the platform's math library, taken
at region_ref64.E_EXP = 4 (units of u, relative): the assumption stated there, imported, not restated.  1.01 covers second-order terms.

GEMM  c = alpha sum_k a_k w_k (+ bias) (ReLU) (+ C_old), S = sum_k |a_k w_k|:
    K products and K additions in ANY order (the MFMA adds four products per step in an unspecified internal order; a fused step
    only removes roundings): (K - 1) u S at most for the chain, one u for alpha, one each for the bias and the residual add:
        |got - ref| <= 1.01 (K + 3) u (|alpha| S + |bias| + |C_old|) + SUB.        ReLU is 1-Lipschitz: the bar passes through it.
    One missing product moves an element by |a_k w_k| ~ S / (0.8 K) >> (K + 3) u S for every K tested (K u <= 2e-4).

Attention (one query, keys j < len; len = T, lens[b], or t + 1 in the causal kernel), T_j = sum_c |q_c k_jc|:
    scores          s_j = scale (sum of 64 products, a serial chain): 64 u for the chain, one for the scale, one spare:
                        delta_j = 66 u scale T_j                                     (absolute)
    probabilities   p_j = e_j / sum, e_j = expf(s_j - max).  A shift of every score by at most delta = max_j delta_j moves p_j by the
                    factor 2 delta; expf E_EXP u; each lane adds ceil(len / 64) values, the wave tree 6 levels; 1 / sum and the final
                    product one u each:
                        rel_p = 2 delta + (E_EXP + ceil(len / 64) + 6 + 2) u        (relative, the same for every key of a query)
                    (Left out as below 2% of 2 delta at N(0, 1) operands: the rounding of s_j - max, u |s_j - max|, and the
                    normaliser's share of the expf error, at most E_EXP u more.  A case that failed by them would gain them as terms.)
    output          o_c = sum_j p_j v_jc, a serial chain of len products:
                        |got - ref| <= 1.01 (rel_p + (len + 2) u) sum_j p_j |v_jc| + SUB
    Rows len <= t < Tp are zero exactly.  One key too many moves a row by about 1 / len of |v|: 1e-2 at len = 100 against 1e-4.

LayerNorm, two passes (mean, then the centred second moment), as decoder_ref64 / vit_ref64 state it, summation depth d (one wave per
row: ceil(D / 64) serial adds per lane + 6 tree levels; k_text_pool: ceil(W / 256) + 6 + 2 for the four waves' partials):
    mean            |d mu| <= (d + 1) u mean|x|                      (the sum, the division)
    centred         c = x - mu: |d c| <= |d mu| + u |c|
    variance        relative (d + 3) u (squares, sum, division), the mean's error only at second order: (d mu)^2 / (var + eps)
    rstd            1 / sqrtf(var + eps): half the variance's (d + 3 + 1) u, plus 2 u each for the root and the division
                        rel_r = (d / 2 + 6) u + (d mu)^2 / (2 (var + eps))
    y = c rstd w + b: two products and the add
        |got - ref| <= 1.01 u (|w| rstd ((d + 1) mean|x| + (d / 2 + 9 + second order) |c|) + |y|) + SUB
    The unbiased variance moves rstd by 1 / (2 D) >= 2e-4 relative (D <= 2560) against (d / 2 + 9) u <= 2e-6.
    Text pool: out_e = sum_k y_k proj_ke, a chain of W FMAs:  sum_k bar(y_k) |proj_ke| + 1.01 (W + 2) u sum_k |y_k proj_ke| + SUB.

Pointwise (in place; the input v is exact, so only the function's own evaluation errs; g' carries the rounded argument):
    GELU-erf    0.5 v (1 + erff(t)), t = v c32 (c32 = fp32(1 / sqrt 2): 2 u on t):  erf(t) is off by E_EXP u |erf| + 2 u |t| erf'(t),
                1 + erf adds u |1 + erf|, the two products 2 u |g|:
                    u (0.5 |v| (E_EXP |erf t| + 2 |t| erf'(t) + |1 + erf t|) + 2 |g|) + SUB
    QuickGELU   v / (1 + expf(a)), a = -1.702f v (2 u |a| on a): e = exp(a) is off by (2 |a| + E_EXP) u relative, which reaches
                sigma = 1 / (1 + e) scaled by e / (1 + e) = 1 - sigma; the add, the division (2 u) and the product:
                    u |g| ((1 - sigma) (2 |a| + E_EXP) + 4) + SUB
    tanh        E_EXP u |tanh v| + SUB
    sigmoid     1 / (1 + expf(-v)): u sigma ((1 - sigma) E_EXP + 3) + SUB
    resid_ls    x + y ls.  The compiler may contract to one FMA (hipcc's default -ffp-contract=fast) or keep two roundings; the bar holds
                for both: u (|y ls| + |x + y ls|) + SUB  (the FMA form needs only the second term).

Copies (im2col, embed scatter, text embed) have no bar: a written element equals its source, or the single fp32 sum of two sources, bitwise.
"""
import math
from types import SimpleNamespace
from typing import Optional, Sequence

import numpy as np
import torch

from region_ref64 import E_EXP

F64 = torch.float64
U = 2.0 ** -24
SUB = 2.0 ** -126
SLOP = 1.01


def f32(v: float) -> float:
    """The scalar as the C ABI passes it: rounded to fp32, then exact."""
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------ GEMM
def sgemm64(A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], alpha: float, C_old: Optional[torch.Tensor], relu: bool,
            drop_k: Optional[int] = None) -> SimpleNamespace:
    """A [M][K], W [N][K] (views of the padded buffers), bias [N] | None, C_old [M][N] | None (the residual form).
    -> ref [M][N], mag = |alpha| sum |a w| + |bias| + |C_old|, bar.  drop_k: leave one k out (the CPU test's wrong reference)."""
    a, w = A.to(F64), W.to(F64)
    if drop_k is not None:
        keep = torch.ones(a.shape[1], dtype=torch.bool, device=a.device)
        keep[drop_k] = False
        a, w = a[:, keep], w[:, keep]
    al = f32(alpha)
    ref = al * (a @ w.t())
    mag = abs(al) * (a.abs() @ w.abs().t())
    if bias is not None:
        ref = ref + bias.to(F64)
        mag = mag + bias.to(F64).abs()
    if relu:
        ref = ref.clamp_min(0.0)
    if C_old is not None:
        ref = ref + C_old.to(F64)
        mag = mag + C_old.to(F64).abs()
    K = A.shape[1]
    return SimpleNamespace(ref=ref, mag=mag, bar=SLOP * (K + 3) * U * mag + SUB)


# ------------------------------------------------------------------------------------------------ attention
def attention64(qkv: torch.Tensor, B: int, H: int, Tp: int, scale: float, lens: Optional[Sequence[int]] = None, T: Optional[int] = None,
                causal: bool = False, extra_key: bool = False) -> SimpleNamespace:
    """qkv [B*Tp][3 D] (q | k | v), D = 64 H.  Keys of query (b, t): j < lens[b] (or T), causal: j <= t.  Queries t >= len give zero rows.
    -> out [B*Tp][D], scores / probs [B][H][Tp][Tp] (masked keys: -inf / 0), T_abs (sum |q k|), d_score, rel_p [B][H][Tp][1], bar
    [B*Tp][D].  extra_key: every query attends one key more than it should (the CPU test's wrong reference)."""
    D = 64 * H
    x = qkv.to(F64).view(B, Tp, 3, H, 64)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))          # [B][H][Tp][64]
    dev = qkv.device
    t = torch.arange(Tp, device=dev)
    if causal:
        n_keys = (t + 1).view(1, Tp).expand(B, Tp)
        live = torch.ones(B, Tp, dtype=torch.bool, device=dev)
    else:
        ln = torch.tensor([T] * B if lens is None else list(lens), device=dev).view(B, 1)
        n_keys = ln.expand(B, Tp)
        live = t.view(1, Tp) < ln
    n_keys = n_keys.clone()
    if extra_key:
        n_keys = (n_keys + 1).clamp_max(Tp)
    mask = (t.view(1, 1, Tp) < n_keys.view(B, Tp, 1)) & live.view(B, Tp, 1)          # [B][query][key]
    mask = mask.view(B, 1, Tp, Tp)
    sc = f32(scale)
    qz, kz, vz = (torch.nan_to_num(z, nan=0.0, posinf=0.0, neginf=0.0) for z in (q, k, v))   # masked rows may hold anything
    scores = sc * (qz @ kz.transpose(-1, -2))
    T_abs = qz.abs() @ kz.abs().transpose(-1, -2)
    scores = scores.masked_fill(~mask, float("-inf"))
    probs = torch.nan_to_num(torch.softmax(scores, dim=-1), nan=0.0)                   # rows without keys: zero
    out = probs @ vz
    d_score = (66.0 * U * sc * T_abs).masked_fill(~mask, 0.0)
    nk = n_keys.view(B, 1, Tp, 1).to(F64)
    rel_p = 2.0 * d_score.max(dim=-1, keepdim=True).values + (E_EXP + torch.ceil(nk / 64.0) + 6.0 + 2.0) * U
    bar = SLOP * (rel_p + (nk + 2.0) * U) * (probs @ vz.abs()) + SUB
    livef = live.view(B, 1, Tp, 1)
    bar = torch.where(livef, bar, torch.zeros_like(bar))
    flat = lambda z: z.permute(0, 2, 1, 3).reshape(B * Tp, D)  # noqa: E731
    return SimpleNamespace(out=flat(out), bar=flat(bar), scores=scores, probs=probs, T_abs=T_abs, d_score=d_score, rel_p=rel_p,
                           live=live.reshape(B * Tp))


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_depth(D: int) -> int:
    """k_layernorm_f32: one wave per row."""
    return -(-D // 64) + 6


def pool_depth(W: int) -> int:
    """k_text_pool: 256 threads per row, four wave partials."""
    return -(-W // 256) + 8


def layernorm64(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float, depth: Optional[int] = None,
                unbiased: bool = False) -> SimpleNamespace:
    """x [M][D] -> ref, bar [M][D], rstd [M][1].  unbiased: divides the second moment by D - 1 (the CPU test's wrong reference)."""
    x64, w64, b64 = x.to(F64), w.to(F64), b.to(F64)
    D = x.shape[-1]
    d = ln_depth(D) if depth is None else depth
    mu = x64.mean(-1, keepdim=True)
    c = x64 - mu
    var = (c * c).sum(-1, keepdim=True) / (D - 1 if unbiased else D)
    e = f32(eps)
    rstd = 1.0 / torch.sqrt(var + e)
    ref = c * rstd * w64 + b64
    dmu = (d + 1) * U * x64.abs().mean(-1, keepdim=True)
    second = dmu * dmu / (2.0 * (var + e)) / U
    bar = SLOP * U * (w64.abs() * rstd * ((d + 1) * x64.abs().mean(-1, keepdim=True) + (d / 2.0 + 9.0 + second) * c.abs()) + ref.abs()) + SUB
    return SimpleNamespace(ref=ref, bar=bar, rstd=rstd)


# ------------------------------------------------------------------------------------------------ pointwise
GELU_ERF, QUICKGELU, TANH, SIGMOID, RESID_LS = 0, 1, 2, 3, 4


def pointwise64(op: int, v: torch.Tensor) -> SimpleNamespace:
    """ops 0..3 on v (fp32 values) -> ref, bar."""
    x = v.to(F64)
    if op == GELU_ERF:
        t = x * f32(0.70710678118654752)
        er = torch.erf(t)
        ref = 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
        d_erf = 2.0 / math.sqrt(math.pi) * torch.exp(-t * t)
        bar = U * (0.5 * x.abs() * (E_EXP * er.abs() + 2.0 * t.abs() * d_erf + (1.0 + er).abs()) + 2.0 * ref.abs())
    elif op == QUICKGELU:
        a = -f32(1.702) * x
        sig = torch.sigmoid(-a)
        ref = x * torch.sigmoid(1.702 * x)
        bar = U * ref.abs() * ((1.0 - sig) * (2.0 * a.abs() + E_EXP) + 4.0)      # fp32(1.702) against 1.702 is inside 2 u |a|
    elif op == TANH:
        ref = torch.tanh(x)
        bar = E_EXP * U * ref.abs()
    elif op == SIGMOID:
        ref = torch.sigmoid(x)
        bar = U * ref * ((1.0 - ref) * E_EXP + 3.0)
    else:
        raise ValueError(op)
    return SimpleNamespace(ref=ref, bar=SLOP * bar + SUB)


def resid_ls64(x: torch.Tensor, y: torch.Tensor, ls: torch.Tensor) -> SimpleNamespace:
    """x [n], y [n], ls [D] -> x + y ls[i % D], bar (for the FMA and for the two-rounding form)."""
    n, D = x.numel(), ls.numel()
    l = ls.to(F64)[torch.arange(n, device=x.device) % D]
    prod = y.to(F64).view(-1) * l
    ref = x.to(F64).view(-1) + prod
    return SimpleNamespace(ref=ref, bar=SLOP * U * (prod.abs() + ref.abs()) + SUB)


# ------------------------------------------------------------------------------------------------ copies
def im2col_index(B: int, S: int, p: int):
    """-> (rows, cols, b, c, y, x) index tensors: out[rows, cols] = imgs[b, c, y, x] lists every element k_im2col_f32 writes."""
    n = S // p
    b, gy, gx, c, py, px = torch.meshgrid(*(torch.arange(m) for m in (B, n, n, 3, p, p)), indexing="ij")
    rows = (b * n + gy) * n + gx
    cols = c * p * p + py * p + px
    return tuple(z.reshape(-1) for z in (rows, cols, b, c, gy * p + py, gx * p + px))


def first_argmax(ids: torch.Tensor, second: bool = False) -> torch.Tensor:
    """EOT position of each id row: the FIRST maximum.  second: the last one instead (the CPU test's wrong reference)."""
    L = ids.shape[1]
    mx = ids.max(dim=1, keepdim=True).values
    pos = torch.arange(L, device=ids.device).view(1, L).expand_as(ids)
    if second:
        return torch.where(ids == mx, pos, torch.full_like(pos, -1)).max(dim=1).values
    return torch.where(ids == mx, pos, torch.full_like(pos, L)).min(dim=1).values


def text_pool64(x: torch.Tensor, ids: torch.Tensor, Tp: int, lw: torch.Tensor, lb: torch.Tensor, eps: float, proj: torch.Tensor,
                second: bool = False) -> SimpleNamespace:
    """x [N*Tp][W], ids [N][L], proj [W][E] -> ref [N][E], bar, eot [N]."""
    N, W = ids.shape[0], x.shape[1]
    eot = first_argmax(ids, second)
    rows = x[torch.arange(N, device=x.device) * Tp + eot]
    ln = layernorm64(rows, lw, lb, eps, depth=pool_depth(W))
    p64 = proj.to(F64)
    ref = ln.ref @ p64
    bar = ln.bar @ p64.abs() + SLOP * (W + 2) * U * (ln.ref.abs() @ p64.abs()) + SUB
    return SimpleNamespace(ref=ref, bar=bar, eot=eot)


# ------------------------------------------------------------------------------------------------ the cases both test files share
# (M, N, K, lda, ldw, ldc): one element; one full tile; ragged both ways at the smallest K; ragged with padded leading dimensions; several
# column tiles at the ViT-B width; a long chain (the fp32 MLP's K); the patch embed's Kpad = round_up(3 14^2, 32) over three row tiles
SGEMM_SHAPES = [(1, 1, 32, 32, 32, 1), (64, 64, 64, 64, 64, 64), (63, 65, 32, 32, 32, 65), (65, 63, 96, 100, 104, 66),
                (20, 129, 768, 768, 768, 129), (5, 70, 3072, 3072, 3072, 70), (130, 200, 608, 608, 608, 200)]
SGEMM_FORMS = [(0, 0), (1, 0), (0, 1)]          # (relu, resid)
SGEMM_ALPHAS = [1.0, 1.0 / 0.07]
HEAVY_ROWS = 2                                   # rows of A that carry the heavy, cancelling pair of columns


def sgemm_case(M: int, N: int, K: int, lda: int, ldw: int, ldc: int, seed: int = 0) -> SimpleNamespace:
    """fp32 operands in their padded buffers (the padding holds finite junk: a kernel that reads it is caught by the value).  Mixed
    signs; columns 3 and 4 of the first HEAVY_ROWS rows of A carry +-100 against weights that cancel pairwise (W[:, 4] = -W[:, 3]), so
    sum |a w| >> |sum a w| there."""
    g = torch.Generator().manual_seed(7919 * seed + M + 3 * N + 5 * K)
    A = torch.randn(M, lda, generator=g)
    W = torch.randn(N, ldw, generator=g) * 0.05
    A[:HEAVY_ROWS, 3] = 100.0
    A[:HEAVY_ROWS, 4] = 100.0
    W[:, 4] = -W[:, 3]
    bias = 0.1 * torch.randn(N, generator=g)
    C_old = torch.randn(M, ldc, generator=g)
    return SimpleNamespace(A=A.contiguous(), W=W.contiguous(), bias=bias, C_old=C_old.contiguous(), M=M, N=N, K=K)


def sgemm_int_case(M: int, N: int, K: int, lda: int, ldw: int, ldc: int, seed: int = 0) -> SimpleNamespace:
    """Integers: |a| <= 7, |w| <= 7, so |sum| <= 49 K <= 150 528 < 2^24 at K = 3072, with bias and C_old (|.| <= 1000) on top: every
    partial sum in any order is an exact fp32 integer."""
    g = torch.Generator().manual_seed(104729 * seed + M + 3 * N + 5 * K)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).to(torch.float32)  # noqa: E731
    return SimpleNamespace(A=ri(-7, 7, M, lda), W=ri(-7, 7, N, ldw), bias=ri(-1000, 1000, N), C_old=ri(-1000, 1000, M, ldc), M=M, N=N, K=K)


ATTN_B = 3
ATTN_PLAIN = [(8, 1), (8, 8), (64, 64), (72, 65), (136, 129), (136, 136)]            # (Tp, T) without lens
ATTN_LENS = {72: [(0, 1, 63), (64, 65, 72)], 136: [(0, 1, 63), (64, 65, 136)]}       # Tp -> lens rows: {0, 1, 63, 64, 65, Tp}
TEXT_TP = [8, 72, 80]
TEXT_N = 3


def qkv_case(B: int, H: int, Tp: int, seed: int = 0) -> torch.Tensor:
    """[B*Tp][3 D] N(0, 1), the first sequence's queries scaled by 3 (peaked softmax rows next to flat ones).  Sequence b's rows depend
    on (seed, b, H) alone and row t on t alone, so the same rows appear under every Tp."""
    D = 64 * H
    out = torch.empty(B, Tp, 3 * D)
    for b in range(B):
        g = torch.Generator().manual_seed(1000003 * seed + 97 * b + H)
        rows = torch.randn(160, 3 * D, generator=g)
        out[b] = rows[:Tp]
    out[0, :, :D] *= 3.0
    return out.view(B * Tp, 3 * D).contiguous()


LN_D = [64, 100, 384, 768, 2560]
LN_M = [1, 4, 5]


def ln_case(M: int, D: int, seed: int = 0) -> SimpleNamespace:
    """Rows N(0, 1); row 0 has a massive channel (1e3 among O(1)); with M >= 4: row 1 constant 3.0 (variance 0: only eps under the root),
    row 2 all 1e-20."""
    g = torch.Generator().manual_seed(31 * seed + 1009 * M + D)
    x = torch.randn(M, D, generator=g)
    x[0, D // 3] = 1e3
    if M >= 4:
        x[1] = 3.0
        x[2] = 1e-20
    return SimpleNamespace(x=x, w=1.0 + 0.1 * torch.randn(D, generator=g), b=0.1 * torch.randn(D, generator=g), eps=1e-5)


POINTWISE_N = [1, 255, 256, 257, 70001]
SWEEP = [0.0, 2.0 ** -130, 1e-3, 0.5, 1.0, 3.0, 10.0, 40.0, 100.0]


def pointwise_values(n: int, seed: int = 0) -> torch.Tensor:
    """+-SWEEP first (as many as fit), N(0, 3) after."""
    g = torch.Generator().manual_seed(53 * seed + n)
    v = 3.0 * torch.randn(n, generator=g)
    sweep = torch.tensor([s * x for x in SWEEP for s in (1.0, -1.0)], dtype=torch.float64).to(torch.float32)
    m = min(n, sweep.numel())
    v[:m] = sweep[:m] if n > 1 else sweep[2:3]
    return v
