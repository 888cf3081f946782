"""Float64 statements of the memory-bank projection (csrc/project.hip), the error bars its kernels are held to, and the inputs both test
files share (tests/test_project_ref64_cpu.py, tests/test_gpu_project_kernels.py).

Plain numpy on the CPU; nothing here calls the package's kernels.  No test functions here.

References
  inv_norm64     1 / |bank[r]|
  split_bank64   the operand image of the split form, EXACT bits: S a power of two, hi = fp16(x S) and lo = fp16(x S - hi), both round to
                 nearest even with fp16 subnormals kept; [M][2][D] as uint16
  abs_max_bits   max |x| as the bit pattern of a non-negative fp32; bank_scale: the loader's power of two (max|bank| S in [2^14, 2^15))
  slab_bounds    the layout contract of k_project2: the bank in units of 16 rows (one query group) or 32 rows (two or three groups),
                 ceil(units / parts) units per workgroup, in order; workgroups past the last unit are empty
  partials64     per workgroup and query  m = max_r z_r,  l = sum_r e^(z_r - m),  Acc = sum_r e^(z_r - m) bank[r]  over the slab's rows,
                 z_r = <q, bank[r]> inv_r / T;  an empty slab: m = -inf, l = 0, Acc = 0
  combine64      out = sum_b e^(m_b - m) Acc_b / sum_b e^(m_b - m) l_b,  m = max_b m_b
  project64      the whole call: q / |q|, inv_norm64, softmax over all rows, optional normalisation of the result
  sims64, topk64 cosines and the k largest per query, a tie going to the lower row index

Bars.  A bar is a function of float64 quantities of the CASE (inputs and the float64 result), never of the device output.  u = U32 = 2^-24
for fp32 operands and accumulation, U_SPLIT16 = 2^-22 where operands are pairs of fp16 numbers, SAFETY = 8 over the random-walk estimate
(the constants of tests/decoder_ref64.py).  For query n and row r:  s = sum_d q_d b_rd,  A_r = sum_d |q_d| |b_rd| inv_r,  z_r = s inv_r / T.
  similarity      sqrt(D) u_dot A_r    D roundings of random sign, each relative to a partial sum below sum |q_d| |b_rd|; u_dot = U_SPLIT16
                                       in the split form (each factor carries 22 bits, the dropped lo lo product is 2^-22 of a product)
                  + 2 u A_r            the four waves' partial sums meet in LDS and are added in fp32
  logit           delta_r = (sqrt(D) u_dot + 2 u) A_r / T + 2 u |z_r|      the 1 / T amplification; the products with inv_r and 1 / T
  split, small rows
                  + (2^-25 / S) inv_r / T + 2^-39 sum_d |b_rd| inv_r / T
                                       x S = hi + lo is good to 2^-23 |x S| only while lo is a normal fp16.  Below that lo's quantum is
                                       fp16's smallest subnormal, 2^-24: an absolute error of 2^-25 per element of x S, i.e. 2^-25 / S per
                                       element of the row, a random walk over the unit query: (2^-25 / S) inv_r in the cosine.  With
                                       rho_r = max_d |b_rd| / max|bank| (S max|bank| > 2^14, |b_r| >= max_d |b_rd|) that is at most
                                       2^-39 / rho_r: nothing at rho = 1, 2^-23 at rho = 2^-16, 2^-15 at rho = 2^-24 -- the "magnitude term".
                                       It assumes the hardware KEEPS fp16 subnormals (conversion and matrix instruction); the ladder test
                                       measures that.  The second summand is the same for the query, q 2^14 = qh + ql.
  weight          w_r = e^(z_r - m): relative error  eps_r = delta_r + delta_* + u (m - z_r) + 4 u (1 + tiles)
                                       delta_* = max delta over the slab (the running maximum is itself a computed logit); the subtraction
                                       z - m_run and every later rescale e^(m_old - m_new) round their argument: together u (m - z_r);
                                       expf and the product, once per tile the row lives through
  m               SAFETY delta_*
  l               SAFETY (sum_r w_r eps_r + (sqrt(R) + tiles + 2) u l)         R rows in the slab: the fp32 sum and the rescales
  Acc[d]          SAFETY (sum_r w_r eps_r |b_rd| + (sqrt(R) + tiles + 2) u G_d [+ split: 2 U_SPLIT16 G_d + 2^-39 sum_r |b_rd| + (2^-25 / S) l])
                                       G_d = sum_r w_r |b_rd|.  Split form: P 2^14 = Ph + Pl and the bank's hi + lo are each good to 2^-23
                                       of a factor; a P whose low half is subnormal keeps 2^-39 absolute, a bank element 2^-25 / S
  merged out[d]   the softmax p_r = w_r / sum w is normalised, so a common shift of the logits cancels: d out_d = sum_r p_r eps'_r (b_rd - out_d)
                  with eps'_r = delta_r + u (m - z_r) + 4 u (3 + tiles) (one more weight, e^(m_b - m), and the division):
                  SAFETY (sum_r p_r eps'_r (|b_rd| + |out_d|) + (sqrt(R) + tiles + sqrt(parts) + 4) u H_d [+ split: 2 U_SPLIT16 H_d +
                  2^-39 sum_r |b_rd| / L + 2^-25 / S]),   H_d = sum_r p_r |b_rd|,  L = sum_r e^(z_r - m)
  whole call      q is normalised and inv_norm computed by fp32 kernels: delta_r += 8 u |z_r|; the final normalisation adds
                  bar_d / |out| + |out_d| |bar|_2 / |out|^2 + 4 u |out_d| / |out|
  inv_norm        SAFETY u (sqrt(depth) / 2 + 2) inv_r, depth = 3 + D / 256 + 6: a lane adds D / 256 groups of four squares, six shuffle steps
                  join the lanes; 1 / sqrt halves the sum's error; sqrtf and the division.  Holds while every square is a normal fp32
  top-k           a similarity: SAFETY ((sqrt(D) u + 2 u) A_r + 10 u |c_r|).  An index may depart from float64's only where the float64
                  cosines of the two rows differ by no more than the sum of their bars; equal rows come in ascending order, always

What the bars see.  At T = 1 every row of a slab carries about the same weight, so a row dropped, doubled or read with another row's
inv_norm moves m, l or Acc by 1 / R or so, thousands of bars.  At T = 0.01 the logit bar is 100 times wider and a fault is seen only through
rows that carry weight: with a dominant row (the planted family: logit 100 against |z| < 15) a lost row of the same slab stays inside every bar
of that query and inside the merged bar of all of them.  The Gaussian family at M = 300 .. 600 has no dominant row -- among 16 queries and 80 rows
some row of the slab weighs enough -- and still sees a dropped row at T = 0.01 (tests/test_project_ref64_cpu.py asserts both).
"""
import math
from typing import Dict, List, Optional, Tuple

import numpy as np

U32, U_SPLIT16, SAFETY = 2.0 ** -24, 2.0 ** -22, 8.0
P_SCALE = 16384.0
WIDTHS = (384, 512, 640, 768, 1024)
F64 = np.float64


# ------------------------------------------------------------------------------------------------ references
def inv_norm64(bank) -> np.ndarray:
    b = np.asarray(bank, F64)
    return 1.0 / np.sqrt((b * b).sum(-1))


def inv_norm_bar(bank) -> np.ndarray:
    D = np.asarray(bank).shape[1]
    return SAFETY * U32 * (math.sqrt(3 + D / 256 + 6) / 2 + 2) * inv_norm64(bank)


def abs_max_bits(x) -> int:
    return int(np.abs(np.asarray(x, np.float32)).max().view(np.uint32))


def bank_scale(bank) -> float:
    """The loader's scale (csrc/api.cpp: bank_common): max|bank| = m 2^ex, m in [0.5, 1)  ->  2^(15 - ex)."""
    _, ex = math.frexp(float(np.abs(np.asarray(bank, np.float32)).max()))
    return math.ldexp(1.0, 15 - ex)


def split16(x32: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """fp32 -> (hi, lo) fp16, round to nearest even, subnormals kept (numpy's conversion)."""
    x32 = np.asarray(x32, np.float32)
    hi = x32.astype(np.float16)
    lo = (x32 - hi.astype(np.float32)).astype(np.float16)          # the difference is exact in fp32
    return hi, lo


def split_bank64(bank, S: float) -> np.ndarray:
    """[M][2][D] uint16: the bits k_split_bank must produce."""
    hi, lo = split16(np.asarray(bank, np.float32) * np.float32(S))
    return np.stack([hi, lo], 1).view(np.uint16)


def slab_bounds(M: int, parts: int, slab_unit: int) -> List[Tuple[int, int, int]]:
    """Per workgroup (first row, end row clipped to M, tiles of 16 rows it walks); an empty slab is (r, r, 0)."""
    units = (M + slab_unit - 1) // slab_unit
    per = (units + parts - 1) // parts
    out = []
    for b in range(parts):
        u0, u1 = min(b * per, units), min((b + 1) * per, units)
        r0 = u0 * slab_unit
        out.append((r0, max(r0, min(M, u1 * slab_unit)), (u1 - u0) * (slab_unit // 16)))
    return out


def logits64(bank, inv, q, T: float) -> np.ndarray:
    """z [N][M] from the kernel's own inputs (inv as given, q as given), all promoted to float64."""
    return (np.asarray(q, F64) @ np.asarray(bank, F64).T) * np.asarray(inv, F64)[None, :] / float(T)


def logit_bar(bank, inv, q, T: float, split: bool, S: float = 0.0, magnitude: bool = True, whole_call: bool = False) -> np.ndarray:
    """delta [N][M] of the docstring, without SAFETY."""
    b, iv, qq = np.asarray(bank, F64), np.asarray(inv, F64), np.asarray(q, F64)
    D = b.shape[1]
    A = (np.abs(qq) @ np.abs(b).T) * iv[None, :]
    z = (qq @ b.T) * iv[None, :] / T
    d = (math.sqrt(D) * (U_SPLIT16 if split else U32) + 2 * U32) * A / T + (10 if whole_call else 2) * U32 * np.abs(z)
    if split and magnitude:
        d = d + ((2.0 ** -25 / S) * iv + 2.0 ** -39 * np.abs(b).sum(-1) * iv)[None, :] / T
    return d


def partials64(bank, inv, q, T: float, bounds, split: bool = False, S: float = 0.0, magnitude: bool = True) -> Dict[str, np.ndarray]:
    """m, l [parts][N], acc [parts][N][D] and their bars bar_m, bar_l, bar_acc."""
    b = np.asarray(bank, F64)
    N, D, P = np.asarray(q).shape[0], b.shape[1], len(bounds)
    z = logits64(bank, inv, q, T)
    dl = logit_bar(bank, inv, q, T, split, S, magnitude)
    ab = np.abs(b)
    r = {"m": np.full((P, N), -np.inf), "l": np.zeros((P, N)), "acc": np.zeros((P, N, D)),
         "bar_m": np.zeros((P, N)), "bar_l": np.zeros((P, N)), "bar_acc": np.zeros((P, N, D))}
    for p, (r0, r1, tiles) in enumerate(bounds):
        if r1 <= r0:
            continue
        zs, ds = z[:, r0:r1], dl[:, r0:r1]
        m = zs.max(-1, keepdims=True)
        w = np.exp(zs - m)
        dstar = ds.max(-1, keepdims=True)
        eps = ds + dstar + U32 * (m - zs) + 4 * U32 * (1 + tiles)
        l = w.sum(-1)
        G = w @ ab[r0:r1]
        walk = (math.sqrt(r1 - r0) + tiles + 2) * U32
        r["m"][p], r["l"][p], r["acc"][p] = m[:, 0], l, w @ b[r0:r1]
        r["bar_m"][p] = SAFETY * dstar[:, 0]
        r["bar_l"][p] = SAFETY * ((w * eps).sum(-1) + walk * l)
        bar = (w * eps) @ ab[r0:r1] + walk * G
        if split:
            bar = bar + 2 * U_SPLIT16 * G + 2.0 ** -39 * ab[r0:r1].sum(0)[None, :] + (2.0 ** -25 / S) * l[:, None]
        r["bar_acc"][p] = SAFETY * bar
    return r


def combine64(m, l, acc) -> np.ndarray:
    """[parts][N], [parts][N], [parts][N][D] -> out [N][D]."""
    top = m.max(0)
    w = np.where(np.isinf(m), 0.0, np.exp(m - top[None, :]))
    return (w[:, :, None] * acc).sum(0) / (w * l).sum(0)[:, None]


def merged64(bank, inv, q, T: float, bounds, split: bool = False, S: float = 0.0, magnitude: bool = True, whole_call: bool = False):
    """(out [N][D], bar [N][D]) of one pass's merged result."""
    b = np.asarray(bank, F64)
    ab = np.abs(b)
    z = logits64(bank, inv, q, T)
    dl = logit_bar(bank, inv, q, T, split, S, magnitude, whole_call)
    m = z.max(-1, keepdims=True)
    w = np.exp(z - m)
    L = w.sum(-1, keepdims=True)
    p = w / L
    out = p @ b
    tiles = max(t for _, _, t in bounds)
    R = max(r1 - r0 for r0, r1, _ in bounds)
    eps = dl + U32 * (m - z) + 4 * U32 * (3 + tiles)
    H = p @ ab
    bar = (p * eps) @ ab + (p * eps).sum(-1, keepdims=True) * np.abs(out) + (math.sqrt(R) + tiles + math.sqrt(len(bounds)) + 4) * U32 * H
    if split:
        bar = bar + 2 * U_SPLIT16 * H + 2.0 ** -39 * ab.sum(0)[None, :] / L + 2.0 ** -25 / S
    return out, SAFETY * bar


def project64(bank, q, T: float, normalize: bool, split: bool, S: float = 0.0, parts: int = 512, magnitude: bool = True):
    """The whole call (pio_mem_project) on raw queries: (out [N][D], bar [N][D]).  The bar takes the geometry of the 32- and 48-query
    passes (parts / 2 workgroups on 32-row units)."""
    b = np.asarray(bank, F64)
    qq = np.asarray(q, F64)
    qq = qq / np.sqrt((qq * qq).sum(-1, keepdims=True))
    bounds = slab_bounds(b.shape[0], max(1, parts // 2), 32)
    out, bar = merged64(b, inv_norm64(b), qq, T, bounds, split, S, magnitude, True)
    if normalize:
        n = np.sqrt((out * out).sum(-1, keepdims=True))
        bar = bar / n + np.abs(out) * np.sqrt((bar * bar).sum(-1, keepdims=True)) / (n * n) + SAFETY * 4 * U32 * np.abs(out) / n
        out = out / n
    return out, bar


def sims64(bank, q):
    """Cosines [N][M] of raw queries against raw rows, and their bar."""
    b, qq = np.asarray(bank, F64), np.asarray(q, F64)
    qq = qq / np.sqrt((qq * qq).sum(-1, keepdims=True))
    iv = inv_norm64(b)
    c = (qq @ b.T) * iv[None, :]
    A = (np.abs(qq) @ np.abs(b).T) * iv[None, :]
    return c, SAFETY * ((math.sqrt(b.shape[1]) + 2) * U32 * A + 10 * U32 * np.abs(c))


def topk64(c: np.ndarray, k: int):
    """(values [N][k], rows [N][k]) descending; equal values: the lower row index first."""
    rows = np.stack([np.lexsort((np.arange(c.shape[1]), -c[n]))[:k] for n in range(c.shape[0])])
    return np.take_along_axis(c, rows, 1), rows


def topk_violations(c: np.ndarray, bar: np.ndarray, bank, got_vals, got_rows, k: int) -> List[str]:
    """What a device top-k (values, rows) breaks of the rule in the docstring; [] when it holds."""
    vals, rows = topk64(c, k)
    bank = np.asarray(bank)
    bad = []
    for n in range(c.shape[0]):
        gr = [int(x) for x in got_rows[n]]
        if len(set(gr)) != k or min(gr) < 0 or max(gr) >= c.shape[1]:
            bad.append("query %d: rows %s are not %d distinct rows of the bank" % (n, gr, k))
            continue
        for j in range(k):
            i, i64 = gr[j], int(rows[n, j])
            if abs(float(got_vals[n][j]) - c[n, i]) > bar[n, i]:
                bad.append("query %d rank %d: similarity of row %d off by %.3e (bar %.3e)" % (n, j, i, abs(float(got_vals[n][j]) - c[n, i]), bar[n, i]))
            if i != i64 and abs(c[n, i] - c[n, i64]) > bar[n, i] + bar[n, i64]:
                bad.append("query %d rank %d: row %d for %d, float64 gap %.3e" % (n, j, i, i64, abs(c[n, i] - c[n, i64])))
            if j and gr[j] < gr[j - 1] and np.array_equal(bank[gr[j]], bank[gr[j - 1]]):
                bad.append("query %d ranks %d, %d: equal rows %d, %d not in ascending order" % (n, j - 1, j, gr[j - 1], gr[j]))
    return bad


def worst(got, ref, bar) -> float:
    """max |got - ref| / bar over the elements with a finite reference; a non-finite ``got`` there is infinitely wrong.  Where the reference
    is -inf (an empty slab's m) ``got`` must be -inf too."""
    got, ref, bar = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(bar, F64)
    ok = np.isfinite(ref)
    if not np.array_equal(got[~ok], ref[~ok]):
        return float("inf")
    if not ok.any():
        return 0.0
    err = np.abs(got[ok] - ref[ok])
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bar[ok])
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------ inputs
def _unit(x: np.ndarray) -> np.ndarray:
    """Rows of unit norm to fp32 rounding (normalised in float64, rounded once)."""
    x = np.asarray(x, F64)
    return (x / np.sqrt((x * x).sum(-1, keepdims=True))).astype(np.float32)


def _biased_values(rng, shape, biased: np.ndarray) -> np.ndarray:
    """Positive numbers 2^14 (1 + j 2^-10), j < 64: fp16 grid points; where ``biased`` 0.45 of a grid step (16) is added, so that fp16(x)
    cuts the SAME 4.4e-4 of every such element and the low half carries it."""
    j = rng.integers(0, 64, size=shape)
    return 16384.0 * (1.0 + j / 1024.0) + 7.2 * biased


def make_case(family: str, M: int, D: int, N: int, seed: int = 0, planted: Tuple[int, ...] = (), qsel: int = 5) -> Tuple[np.ndarray, np.ndarray]:
    """(bank [M][D] fp32, q [N][D] fp32 unit rows).  Families:
      gauss      unit Gaussian rows                     scales    every 7th row 3 x, rows 3, 14, 25 .. 1e-3 x
      rising     all queries equal; rows sorted so that the running maximum rises in every tile
      never      all queries equal; rows sorted so that it never moves after a slab's first tile (the skip-rescale path)
      ballot     as never, but query ``qsel`` equals row ``planted[-1]``: the maximum moves for one query of the sixteen only
      planted    query n equals row planted[n % len(planted)] (that row dominates), Gaussian bank
      constant   every row the same Gaussian row
      biased     split-form operands with a one-signed low half: a positive bank, every x S 0.45 of a step above an fp16 grid point;
                 positive queries built the same way (their last channel tops the norm up to one).  Without the low halves of either
                 operand every logit, and with it m, drops by 4.3e-4 of itself
      biased_onehot  the same bank under one-hot queries (channel 7 n): sum |q||b| inv is 1 / sqrt(D), the weight bar at T = 1 is as narrow as
                 the accumulation allows, and Acc shows a bank whose low plane GEMM2 alone does not read (4.3e-4 of every element)
      biased_p   weights with a one-signed low half: one-hot queries (channel n % 2), and channels 0, 1 of row r set so that
                 e^(z_r - m) 2^14 sits 0.45 of a step above an fp16 grid point (T = 1; rows 0 mod 16 carry the maximum); the other channels positive"""
    rng = np.random.default_rng(1000 * seed + 7 * M + D + len(family))
    bank = rng.standard_normal((M, D))
    q = rng.standard_normal((N, D))
    if family == "gauss":
        pass
    elif family == "scales":
        bank[::7] *= 3.0
        bank[3::11] *= 1e-3
    elif family in ("rising", "never", "ballot"):
        q[:] = q[0]
        c = (bank @ q[0]) / np.sqrt((bank * bank).sum(-1))
        order = np.argsort(c)
        bank = bank[order if family == "rising" else order[::-1]]
        if family == "ballot":
            q[qsel % N] = bank[planted[-1]]
    elif family == "planted":
        for n in range(N):
            q[n] = bank[planted[n % len(planted)]]
    elif family == "constant":
        bank[:] = bank[0]
    elif family == "biased":
        bank = _biased_values(rng, (M, D), np.ones((M, 1))) / 16384.0                         # max < 2: S = 2^14
        qs = 512.0 * (1.0 + rng.integers(0, 64, size=(N, D)) / 1024.0) + 0.225                    # q 2^14: grid step 0.5 at 512
        q = qs / 16384.0
        q[:, :D // 2] *= 0.5                                                                      # |q| < 1 before the top-up
        q[:, -1] = np.sqrt(1.0 - (q[:, :-1] ** 2).sum(-1))
        return bank.astype(np.float32), q.astype(np.float32)
    elif family == "biased_onehot":
        bank = _biased_values(rng, (M, D), np.ones((M, 1))) / 16384.0
        q[:] = 0.0
        q[np.arange(N), (7 * np.arange(N)) % D] = 1.0
        return bank.astype(np.float32), q.astype(np.float32)
    elif family == "biased_p":
        bank = np.abs(bank) + 0.5
        q[:] = 0.0
        q[np.arange(N), np.arange(N) % 2] = 1.0
        # the weight wanted for row r (the same for every query): 1 for rows 0 mod 16, else 2^-1 (1 + j 2^-10) + 0.45 steps, as P 2^14
        target = _biased_values(rng, (M,), np.ones(M)) / 32768.0
        target[::16] = 1.0
        zr = 0.3 + np.log(target)                                       # cosine of row r with a one-hot query: its channel / its norm
        rest = np.sqrt((bank[:, 2:] ** 2).sum(-1))
        bank[:, :2] = (zr * rest / np.sqrt(1.0 - 2.0 * zr * zr))[:, None]   # channels 0, 1 carry the same v: v / sqrt(2 v^2 + rest^2) = zr
        return bank.astype(np.float32), q.astype(np.float32)
    else:
        raise ValueError(family)
    return bank.astype(np.float32), _unit(q)


FAMILIES = ("gauss", "scales", "rising", "never", "ballot", "planted", "constant")

# (groups, M, parts): the slab geometry cases of the hook tests; 16-row units for one group, 32-row units for two or three
GEOMETRY = (
    (1, 64, 4), (1, 128, 4), (1, 192, 4), (1, 320, 4),          # slabs of exactly 1, 2, 3 and 5 tiles
    (1, 300, 4),                                                # a partial last slab ending inside a tile
    (1, 33, 8),                                                 # more workgroups than units
    (1, 1, 2), (1, 15, 2), (1, 16, 2), (1, 17, 2), (1, 31, 2), (1, 33, 2),
    (1, 100, 1),                                                # one workgroup, seven tiles
    (2, 1, 2), (2, 15, 2), (2, 16, 2), (2, 17, 2), (2, 31, 2),
    (2, 33, 2),                                                 # the last 32-row unit's second tile lies wholly past M
    (2, 320, 4), (2, 300, 3), (2, 100, 1), (2, 65, 8),
    (3, 33, 2), (3, 300, 4), (3, 100, 1), (3, 17, 4),
)
GEOMETRY_1024 = ((1, 16384, 1024), (1, 16400, 1024), (2, 16400, 1024))   # D = 384: k_project_combine's s_w[1024] full


def families_geometry(groups: int) -> Tuple[int, int]:
    """(M, parts) of the input-family cases: slabs of several tiles, the last one partial."""
    return (300, 4) if groups == 1 else (600, 4)


def planted_rows(M: int, parts: int, groups: int) -> Tuple[int, ...]:
    """First and last row of the second slab, first row of the last slab, row M - 1, and a row in the third tile of the first slab."""
    b = slab_bounds(M, parts, 16 if groups == 1 else 32)
    s1 = b[min(1, len(b) - 1)]
    return (s1[0], s1[1] - 1, b[-1][0], M - 1, 40)


def hook_cases(D: int, groups: int) -> List[dict]:
    """The cases of one (width, query groups) pair that both test files run, in both forms: family, M, parts, nq = N - q0, q0, T."""
    full, q0 = 16 * groups, 3
    geo = [g for g in GEOMETRY + (GEOMETRY_1024 if D == 384 else ()) if g[0] == groups]
    cases = [dict(family="gauss", M=M, parts=parts, nq=full, q0=q0, T=1.0) for _, M, parts in geo]
    M, parts = families_geometry(groups)
    for fam in FAMILIES + ("biased", "biased_onehot", "biased_p"):
        for T in (1.0, 0.01):
            cases.append(dict(family=fam, M=M, parts=parts, nq=full, q0=q0, T=T))
    cases.append(dict(family="gauss", M=M, parts=parts, nq=full, q0=q0, T=1e-3))
    for nq in {1: (1, 15), 2: (17, 31), 3: (33, 47)}[groups]:
        cases.append(dict(family="gauss", M=100, parts=3, nq=nq, q0=q0, T=1.0))
    return cases


def build_case(c: dict, D: int, groups: int):
    """(bank, inv fp32, q, bounds, S) of a hook case: inv is the float64 inverse norm rounded once, S the loader's scale."""
    N = c["q0"] + c["nq"]
    bank, q = make_case(c["family"], c["M"], D, N, planted=planted_rows(c["M"], c["parts"], groups), qsel=c["q0"] + 5)
    return bank, inv_norm64(bank).astype(np.float32), q, slab_bounds(c["M"], c["parts"], 16 if groups == 1 else 32), bank_scale(bank)
