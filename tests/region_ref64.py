"""Float64 statements of the attention read-out and region-weighting stage (csrc/region.hip, the two box-sequence kernels of
csrc/vit_misc.hip, k_revert of csrc/project.hip), for tests/test_region_ref64_cpu.py and tests/test_gpu_region_kernels.py.  No test
functions here.

Written from the formulas of oracle/patchioner_oracle.py (process_self_attention, attention_weighted_means, extract_bboxes_feats,
compute_region_means, ctx_cleaner, revert_transformation, extract_bboxes_feats_double_dino) and from the kernel headers.

Operands.  Every function starts from the values the kernel is handed -- fp32 tensors, and scalars (variance, alpha, scale, the 1e-6 of
the contrastive mask) rounded to fp32 first -- and does everything after that in float64, on whatever device the operands live on.

Coordinates.  torch.linspace(-1, 1, steps) is defined in fp32 by its own evaluation order; the kernel evaluates it two-sided
(linspace_pm1: -1 + step i below steps / 2, 1 - step (steps - 1 - i) from there on, step = 2 / (steps - 1), steps == 1 -> -1).  The choice
here: the SAME two-sided formula evaluated in float64 (linspace_pm1_64).  The fp32 roundings of the coordinate (step, the product, the
sum: at most 4 units of 2^-24, |x| <= 1) are then part of the kernel's error and are accounted for in the bound (`rel` below), not in
the reference.

Bounds.  bbox_weights64 and gaussian_map64 also return `rel`: for every weight a first-order bound of the relative error of the fp32
evaluation in the kernel's order, in units of u = 2^-24.  It has to be carried along with the values because the attention-map mode
feeds a box's rounded output to the next overlapping box.  Per cell of a region, with arg = -(x^2 + y^2) / variance:
    coordinate: |dx| <= 4 u;  square: |d x^2| <= 8 u |x| + u x^2;  the sum of the two squares and the division: one u each of |arg|;
        |d arg| <= u (9 (|x| + |y|) / variance + 2 |arg|)           (x^2 <= |x|)
    expf: E_EXP units on top (the platform's expf, not the kernels': taken as 2 ulp = 4 u, an assumption: the HIP math-API accuracy
        table is not at hand) -> rel(v) = 9 (|x| + |y|) / variance + 2 |arg| + E_EXP
    the sum S of the region (at most 6 cells per thread in a row, then a 6-level wave and a 2-level block tree: SUM_DEPTH = 14):
        rel(S) = sum(v rel(v)) / S + SUM_DEPTH
    w = v (1 / S): two roundings -> rel(w) = rel(v) + rel(S) + 2.
The uniform mode has rel(v) = 0 (ones; the count is exact), the attention-map mode rel(v) = the bound its input cell already carries.
"""
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24
E_EXP = 4.0          # expf: 2 ulp = 4 u (assumption, see the module docstring)
SUM_DEPTH = 14.0     # k_bbox_weights / k_gaussian_map / k_softmax_rows sums: <= 6 serial adds per thread + 6 (wave) + 2 (block)


def f32(v: float) -> float:
    """The scalar as the C ABI passes it: rounded to fp32, then exact."""
    return float(np.float32(v))


def linspace_pm1_64(steps: int, device=None) -> torch.Tensor:
    """The kernel's two-sided linspace(-1, 1, steps), every operation in float64."""
    if steps == 1:
        return torch.full((1,), -1.0, dtype=F64, device=device)
    i = torch.arange(steps, dtype=F64, device=device)
    if steps == 0:
        return i
    step = 2.0 / (steps - 1)
    return torch.where(i < steps // 2, -1.0 + step * i, 1.0 - step * (steps - 1 - i))


# ------------------------------------------------------------------------------------------------ read-out
def cls_readout64(qkv: torch.Tensor, T: int, G: int, D: int, heads: int, scale: float, tokens: Optional[torch.Tensor] = None):
    """qkv [B][T][3 D] (q | k | v), tokens [B][T][Dt] (optional) -> self_attn [B][n2], maps [B][heads][n2] (the CLS row of
    (q scale) k^T over the patch keys), avg_self_attn_token [B][Dt], disentangled [B][heads][Dt]; both means are over all n2 cells."""
    B = qkv.shape[0]
    dh = D // heads
    q = qkv[:, 0, :D].to(F64).reshape(B, heads, dh) * f32(scale)
    k = qkv[:, G:, D:2 * D].to(F64).reshape(B, T - G, heads, dh)
    maps = torch.einsum("bhd,bphd->bhp", q, k)
    self_attn = torch.softmax(maps.mean(dim=1), dim=-1)
    if tokens is None:
        return self_attn, maps, None, None
    patches = tokens[:, G:].to(F64)
    avg = (self_attn.unsqueeze(-1) * patches).mean(dim=1)
    dis = torch.einsum("bhp,bpd->bhd", torch.softmax(maps, dim=-1), patches) / (T - G)
    return self_attn, maps, avg, dis


def softmax_rel64(logits: torch.Tensor, dlogit: torch.Tensor) -> torch.Tensor:
    """First-order relative bound (in units of u) of k_softmax_rows on rows whose logits are already off by at most `dlogit`
    (absolute, in units of u; [..., 1] or [..., n]): a shift of every logit by at most d moves p by 2 d relative; the kernel then rounds
    l - max (u |l - max| on the argument), takes expf (E_EXP), sums (SUM_DEPTH), and multiplies by a rounded 1 / sum (2)."""
    l = logits.to(F64)
    p = torch.softmax(l, dim=-1)
    own = (l - l.max(dim=-1, keepdim=True).values).abs() + E_EXP
    return 2.0 * dlogit.max(dim=-1, keepdim=True).values + own + (p * own).sum(dim=-1, keepdim=True) + SUM_DEPTH + 2.0


# ------------------------------------------------------------------------------------------------ box weights
def bbox_weights64(boxes_int: torch.Tensor, n: int, mode: int, variance: float = 0.5, center: Optional[torch.Tensor] = None,
                   attn: Optional[torch.Tensor] = None, single_map: bool = False) -> SimpleNamespace:
    """The weight construction of extract_bboxes_feats.  boxes_int [B][NB][4] integers (x1, y1, w, h) in grid units (after the floor
    division); the region is the python slice [y1 : y1 + h + 1, x1 : x1 + w + 1] of the n x n grid, taken with real `slice` objects on
    a real tensor, so clamping and negative wrap are python's.  mode 0 uniform (an empty slice gives a NaN row: the mean of nothing),
    1 gaussian (variance), 2 one-hot at center [B][NB][2] (row, column inside the slice; an empty slice has no cell: zeros), 3 the
    attention map attn [B][n2], renormalised IN PLACE per box so that later overlapping boxes read the rescaled values.
    single_map: boxes whose four numbers sum below zero are skipped (zero row), the per-box maps are summed and normalised.
    -> weights [B][NB][n2], single [B][n2] | None, attn_after [B][n2] | None, rel / single_rel / attn_rel: the bounds of the module
    docstring for each of them."""
    bx = boxes_int.to(torch.int64).cpu()
    B, NB = bx.shape[:2]
    dev = attn.device if attn is not None else None
    var = f32(variance)
    W = torch.zeros(B, NB, n, n, dtype=F64, device=dev)
    rel = torch.zeros(B, NB, n, n, dtype=F64, device=dev)
    am = attn.to(F64).clone().view(B, n, n) if attn is not None else None
    am_rel = torch.zeros(B, n, n, dtype=F64, device=dev)
    total = torch.zeros(B, n, n, dtype=F64, device=dev)
    total_err = torch.zeros(B, n, n, dtype=F64, device=dev)       # absolute, units of u
    for i in range(B):
        for j in range(NB):
            x1, y1, w, h = (int(v) for v in bx[i, j])
            if single_map and x1 + y1 + w + h < 0:
                continue
            ys, xs = slice(y1, y1 + h + 1), slice(x1, x1 + w + 1)
            hs, ws = W[i, j, ys, xs].shape
            if mode == 2:
                if hs * ws:
                    cy, cx = (int(v) for v in center[i, j])
                    W[i, j, ys, xs][cy, cx] = 1.0
                    total[i, ys, xs] += W[i, j, ys, xs]
                    total_err[i, ys, xs] += total[i, ys, xs]
                continue
            if mode == 0:
                if hs * ws == 0:
                    W[i, j] = float("nan")
                    continue
                v = torch.ones(hs, ws, dtype=F64, device=dev)
                rv = torch.zeros(hs, ws, dtype=F64, device=dev)
            elif mode == 1:
                yy, xx = linspace_pm1_64(hs, dev)[:, None], linspace_pm1_64(ws, dev)[None, :]
                arg = -(xx * xx + yy * yy) / var
                v = torch.exp(arg)
                rv = 9.0 * (xx.abs() + yy.abs()) / var + 2.0 * arg.abs() + E_EXP
            else:
                v, rv = am[i, ys, xs].clone(), am_rel[i, ys, xs].clone()
            S = v.sum()
            pw = v / S
            r = rv + ((v * rv).sum() / S + SUM_DEPTH) + 2.0
            W[i, j, ys, xs] = pw
            rel[i, j, ys, xs] = r
            if mode == 3:
                am[i, ys, xs] = pw
                am_rel[i, ys, xs] = r
            total[i, ys, xs] += pw
            total_err[i, ys, xs] += pw * r + total[i, ys, xs]     # the addend's own error and the rounding of the add
    out = SimpleNamespace(weights=W.view(B, NB, n * n), rel=rel.view(B, NB, n * n), single=None, single_rel=None,
                          attn_after=am.view(B, n * n) if am is not None else None, attn_rel=am_rel.view(B, n * n))
    if single_map:
        Tsum = total.sum(dim=(1, 2), keepdim=True)
        single = total / Tsum
        eT = total_err.sum(dim=(1, 2), keepdim=True) + SUM_DEPTH * Tsum
        out.single = single.view(B, n * n)
        # absolute bound of single in units of u, turned into a relative one where single > 0 (0 / x is exact)
        err = total_err / Tsum + single * (eT / Tsum + 1.0)
        out.single_rel = torch.where(single > 0, err / single, torch.zeros_like(err)).view(B, n * n)
    return out


def gaussian_map64(n: int, variance: float, device=None):
    """The whole-image weight map of compute_region_means: uniform 1 / n^2 for variance >= 100 (compared in fp32, as the kernel does),
    otherwise the normalised gaussian on linspace(-1, 1, n)^2.  -> (map [n][n], rel [n][n])."""
    var = f32(variance)
    if var >= 100.0:
        return (torch.full((n, n), 1.0 / (n * n), dtype=F64, device=device), torch.ones(n, n, dtype=F64, device=device))
    lin = linspace_pm1_64(n, device)
    yy, xx = lin[:, None], lin[None, :]
    arg = -(xx * xx + yy * yy) / var
    v = torch.exp(arg)
    rv = 9.0 * (xx.abs() + yy.abs()) / var + 2.0 * arg.abs() + E_EXP
    S = v.sum()
    return v / S, rv + ((v * rv).sum() / S + SUM_DEPTH) + 2.0


# ------------------------------------------------------------------------------------------------ weights x tokens
def region_reduce64(tokens: torch.Tensor, weights: torch.Tensor, img_index: Optional[torch.Tensor], scale: float, G: int = 0):
    """out[r] = scale sum_p weights[r][p] tokens[img(r)][G + p], img(r) = img_index[r] or r.  tokens [B][T][D], weights [R][n2] (the
    fp32 values handed to the kernel).  A NaN weight makes its row NaN and no other.  -> (out [R][D], mag [R][D] = scale sum |w| |t|)."""
    w = weights.to(F64)
    R, n2 = w.shape
    img = torch.arange(R) if img_index is None else img_index.to(torch.int64).cpu()
    D = tokens.shape[-1]
    out = torch.empty(R, D, dtype=F64, device=w.device)
    mag = torch.empty(R, D, dtype=F64, device=w.device)
    s = f32(scale)
    for b in torch.unique(img).tolist():
        rows = (img == b).nonzero().flatten().to(w.device)
        t = tokens[b, G:G + n2].to(F64)
        out[rows] = s * (w[rows] @ t)
        mag[rows] = s * (w[rows].abs() @ t.abs())
    return out, mag


# ------------------------------------------------------------------------------------------------ ctx_cleaner
def ctx_clean64(dirty: torch.Tensor, ctx: torch.Tensor, mode: int, alpha: float, normalize_inputs: bool = False) -> torch.Tensor:
    """dirty [B][S][D], ctx [B][D].  mode 0: dirty - alpha (dirty . ctx / |ctx|^2) ctx;  mode 1: dirty (1 - ctx / (|ctx| + 1e-6));
    normalize_inputs: both L2-normalised first."""
    d, c = dirty.to(F64), ctx.to(F64).unsqueeze(1)
    if normalize_inputs:
        d = d / d.norm(dim=-1, keepdim=True)
        c = c / c.norm(dim=-1, keepdim=True)
    if mode == 0:
        proj = (d * c).sum(dim=-1, keepdim=True) / (c * c).sum(dim=-1, keepdim=True)
        return d - f32(alpha) * proj * c
    return d * (1.0 - c / (c.norm(dim=-1, keepdim=True) + f32(1e-6)))


# ------------------------------------------------------------------------------------------------ double-DINO gather / reduce
def box_sequences64(tokens: torch.Tensor, slices: torch.Tensor, G: int, n: int, use_cls: bool):
    """The block input of every (image, box): [the G global rows, if use_cls | the patch rows of the region, row-major].  tokens
    [B][T][D], slices [B][NB][4] = (y_start, y_end, x_start, x_end), python-normalised.  -> a list of B NB tensors [len][D]."""
    B, NB = slices.shape[:2]
    D = tokens.shape[-1]
    seqs = []
    for b in range(B):
        grid = tokens[b, G:G + n * n].view(n, n, D)
        for j in range(NB):
            ys, ye, xs, xe = (int(v) for v in slices[b, j])
            region = grid[slice(ys, ye), slice(xs, xe)].reshape(-1, D)
            seqs.append(torch.cat([tokens[b, :G], region], dim=0) if use_cls else region)
    return seqs


def box_seq_reduce64(rows: torch.Tensor, Gs: int, mode: str) -> torch.Tensor:
    """rows [len][D] = the block's output for one sequence.  "cls": row 0;  "avg": the mean of the region rows (those after the Gs
    global ones), NaN when there is none."""
    return rows[0].to(F64) if mode == "cls" else rows[Gs:].to(F64).mean(dim=0)


def revert64(x: torch.Tensor, A_pinv: torch.Tensor, b: torch.Tensor):
    """(x - b) A_pinv^T.  x [N][D], A_pinv [P][D], b [D] -> (out [N][P], mag [N][P] = sum |x - b| |A_pinv|)."""
    d = x.to(F64) - b.to(F64)
    A = A_pinv.to(F64)
    return d @ A.t(), d.abs() @ A.abs().t()


# ------------------------------------------------------------------------------------------------ shared edge-case inputs
def edge_boxes(n: int) -> torch.Tensor:
    """[3][6][4] integer boxes (x1, y1, w, h) in grid units for an n x n grid, n >= 7.  Image 0: three boxes that overlap pairwise, an
    interior box (even x-span, odd y-span), the full grid, one cell.  Image 1: a one-cell-high row (odd span), a one-cell-wide column
    (even span), an end beyond the grid (clamps), a start beyond the grid (empty), a negative start that wraps, a negative start whose
    end is exactly 0 (empty).  Image 2: start and end both negative (wraps, not empty), both below -n (clamp to 0: empty), the all -1
    dummy, a start at exactly n (empty), the full grid, a negative y start over an earlier box."""
    return torch.tensor([
        [[1, 1, 3, 3], [2, 2, 3, 3], [3, 1, 2, 4], [2, 1, 3, 2], [0, 0, n - 1, n - 1], [3, 4, 0, 0]],
        [[1, 2, 4, 0], [2, 0, 0, 5], [n - 3, n - 2, 10, 10], [n + 2, 1, 2, 2], [-3, 1, 1, 2], [-2, 1, 1, 2]],
        [[-5, 1, 1, 2], [-n - 3, 0, 1, 1], [-1, -1, -1, -1], [n, 0, 1, 1], [0, 0, n - 1, n - 1], [1, -4, 2, 1]],
    ], dtype=torch.int64)


def box_spans(boxes_int: torch.Tensor, n: int) -> torch.Tensor:
    """[B][NB][4] python-normalised (y_start, y_end, x_start, x_end) of the boxes' slices, by slice.indices."""
    out = torch.zeros(boxes_int.shape, dtype=torch.int64)
    for i in range(boxes_int.shape[0]):
        for j in range(boxes_int.shape[1]):
            x1, y1, w, h = (int(v) for v in boxes_int[i, j])
            ys, ye, _ = slice(y1, y1 + h + 1).indices(n)
            xs, xe, _ = slice(x1, x1 + w + 1).indices(n)
            out[i, j] = torch.tensor([ys, max(ye, ys), xs, max(xe, xs)])
    return out


def edge_centers(boxes_int: torch.Tensor, n: int) -> torch.Tensor:
    """A cell inside every non-empty slice, away from its middle: (3 hs / 4, ws / 3); (0, 0) for the empty ones."""
    sp = box_spans(boxes_int, n)
    hs, ws = sp[..., 1] - sp[..., 0], sp[..., 3] - sp[..., 2]
    return torch.stack([(3 * hs) // 4, ws // 3], dim=-1)
