"""The exact-fp32 kernels, one launch at a time through the C ABI's test hooks, against the float64 statements and derived bars of
tests/fp32_ref64.py (its docstring derives every bar; tests/test_fp32_ref64_cpu.py shows each one to be non-vacuous): k_sgemm_tn,
k_attention_f32, k_text_attention_f32, k_layernorm_f32, k_gelu_f32, k_activation_f32, k_resid_ls_f32, k_im2col_f32,
k_embed_scatter_f32, k_text_embed, k_text_pool.

Buffer discipline (as tests/test_gpu_vit_kernels.py): every output lives in a Guarded buffer -- NaN-patterned sentinel in the slack before
and after it and in every slot the kernel's contract leaves alone (padding columns ldc > N, rows >= M, rows outside an image's patch
range, columns >= 3 p^2), compared bitwise after the launch; every other element is compared with its reference, none is skipped.
Bitwise claims (integer operands, one-hot sweeps, row / Tp / in-place invariance, masking) carry no tolerance.  Each test prints the worst
err / bar it saw; test_zz_worst_ratios_per_kernel prints the table.  On an MI355X every derived bar held as first written (no term had to
be added): k_sgemm_tn 0.10, k_attention_f32 0.014, k_text_attention_f32 0.012, k_layernorm_f32 0.20, k_text_pool 0.036, GELU-erf 0.61,
QuickGELU 0.59, tanh 0.57, sigmoid 0.49, k_resid_ls_f32 0.98 -- its bar is one rounding of the result plus one of the product, and every
output carried the bits of the single-rounding (FMA) form, which the compiler's default contraction allows."""
import numpy as np
import pytest
import torch

import fp32_ref64 as R
from patchioner_amd import _lib

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

F64 = torch.float64
DEV = "cuda"
SLACK = 1024
SENT = 0x7FBADBAD                # a NaN no kernel produces
ERR_INVALID = -1
WORST = {}                       # kernel -> worst err / bar


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """Number of elements whose bits differ."""
    return int((_bits(a) != _bits(b)).sum())


def _exact(label, differing):
    print("%-84s %d elements differ (exact)" % (label, differing))
    assert differing == 0, "%s: %d elements differ" % (label, differing)


def _held(kernel, label, got, ref, bar):
    """Every element of got against ref within bar (all float64-comparable, none skipped); prints and records the worst ratio."""
    assert got.shape == ref.shape == bar.shape, (got.shape, ref.shape, bar.shape)
    g = got.to(F64)
    assert bool(torch.isfinite(g).all()), "%s: %d non-finite outputs" % (label, int((~torch.isfinite(g)).sum()))
    err = (g - ref).abs()
    ratio = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = float(ratio.max()) if ratio.numel() else 0.0
    WORST[kernel] = max(WORST.get(kernel, 0.0), r)
    print("%-84s worst err / bar %.3e   (%s so far %.3e)" % (label, r, kernel, WORST[kernel]))
    assert r <= 1.0, "%s: %.3e of its bar" % (label, r)
    return r


class Guarded:
    """fp32 device buffer of `shape`, SLACK sentinels before and after, the inside sentinel-filled too (so: NaN before the launch)."""

    def __init__(self, shape):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.full = torch.empty(self.n + 2 * SLACK, dtype=torch.float32, device=DEV)
        self.full.view(torch.int32).fill_(SENT)
        self.t = self.full[SLACK:SLACK + self.n].view(self.shape)

    def check(self, label, written=None):
        """Everything outside `written` (bool of self.shape; None: nothing may be written) still holds the sentinel, the slack always."""
        iv = self.full.view(torch.int32)
        assert bool((iv[:SLACK] == SENT).all()) and bool((iv[SLACK + self.n:] == SENT).all()), label + ": store outside the buffer"
        inner = iv[SLACK:SLACK + self.n].view(self.shape)
        bad = int((inner != SENT).sum()) if written is None else int((inner[~written] != SENT).sum())
        assert bad == 0, "%s: %d elements written outside the kernel's contract" % (label, bad)


def _rect(shape, rows, cols):
    w = torch.zeros(shape, dtype=torch.bool, device=DEV)
    w[:rows, :cols] = True
    return w


# ------------------------------------------------------------------------------------------------ k_sgemm_tn
EXTRA_ROWS = 3                   # rows >= M of the C buffer: never written


def sgemm(A, W, bias, alpha, C, M, N, K, relu, resid, lda=None, ldw=None, expect_refusal=False):
    """A [>= M][lda], W [>= N][ldw] device tensors, C a Guarded [M + EXTRA_ROWS][ldc]."""
    L = _lib.load()
    rc = L.pio_test_sgemm(A.data_ptr(), A.shape[1] if lda is None else lda, W.data_ptr(), W.shape[1] if ldw is None else ldw,
                          None if bias is None else bias.data_ptr(), alpha, C.t.data_ptr(), C.shape[1], M, N, K, relu, resid, _stream())
    torch.cuda.synchronize()
    if expect_refusal:
        assert rc == ERR_INVALID, "not refused (rc %d)" % rc
        assert L.pio_last_error(), "refusal without a message"
        with pytest.raises(_lib.PioError):
            _lib.check(rc)
        return
    _lib.check(rc)


def _c_buffer(M, N, ldc, C_old=None):
    C = Guarded((M + EXTRA_ROWS, ldc))
    if C_old is not None:
        C.t[:M, :N] = C_old[:M, :N]
    return C


@pytest.mark.parametrize("shape", R.SGEMM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sgemm_against_float64(shape):
    M, N, K, lda, ldw, ldc = shape
    c = R.sgemm_case(*shape)
    A, W, bias, Cold = c.A.to(DEV), c.W.to(DEV), c.bias.to(DEV), c.C_old.to(DEV)
    wr = _rect((M + EXTRA_ROWS, ldc), M, N)
    for relu, resid in R.SGEMM_FORMS:
        for b in (None, bias):
            for alpha in R.SGEMM_ALPHAS:
                label = "sgemm %s relu %d resid %d bias %d alpha %.3f" % (shape, relu, resid, b is not None, alpha)
                C = _c_buffer(M, N, ldc, Cold if resid else None)
                sgemm(A, W, b, alpha, C, M, N, K, relu, resid)
                C.check(label, wr)
                r = R.sgemm64(A[:, :K], W[:, :K], b, alpha, Cold[:, :N] if resid else None, bool(relu))
                _held("k_sgemm_tn", label, C.t[:M, :N], r.ref, r.bar)


@pytest.mark.parametrize("shape", R.SGEMM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sgemm_integer_operands_are_exact(shape):
    """Small integers, every partial sum below 2^24 (tests/test_fp32_ref64_cpu.py checks the magnitudes): the int64 result, bitwise, on
    every form, with alpha 1 and 2 (a power of two keeps every value an exact integer)."""
    M, N, K, lda, ldw, ldc = shape
    c = R.sgemm_int_case(*shape)
    A, W, bias, Cold = c.A.to(DEV), c.W.to(DEV), c.bias.to(DEV), c.C_old.to(DEV)
    prod = (A[:, :K].to(F64) @ W[:, :K].to(F64).t()).to(torch.int64)          # exact: every float64 partial sum is an integer < 2^53
    wr = _rect((M + EXTRA_ROWS, ldc), M, N)
    differing = 0
    for relu, resid in R.SGEMM_FORMS:
        for b in (None, bias):
            for alpha in (1.0, 2.0):
                C = _c_buffer(M, N, ldc, Cold if resid else None)
                sgemm(A, W, b, alpha, C, M, N, K, relu, resid)
                C.check("sgemm integers %s" % (shape,), wr)
                want = int(alpha) * prod + (b.to(torch.int64) if b is not None else 0)
                want = want.clamp_min(0) if relu else want
                want = want + Cold[:, :N].to(torch.int64) if resid else want
                differing += _same(C.t[:M, :N], want.to(torch.float32))
    _exact("sgemm %s integer operands, 12 forms" % (shape,), differing)


def test_sgemm_one_hot_sweeps():
    """K = 96, ragged tiles both ways (96 = 64 + 32 rows, 63 columns; then 65 rows, 96 = 64 + 32 columns), padded leading dimensions:
    one-hot A rows return W's columns, one-hot W rows return A's columns, bit for bit, for every k."""
    K = 96
    g = torch.Generator().manual_seed(96)
    eye = torch.zeros(K, 100)
    eye[:, :K] = torch.eye(K)
    eye[:, K:] = 7.0                                         # the padding of the one-hot operand is never read
    Wr = torch.randn(63, 104, generator=g).to(DEV)
    C = _c_buffer(K, 63, 66)
    sgemm(eye.to(DEV), Wr, None, 1.0, C, K, 63, K, 0, 0)
    C.check("one-hot A", _rect((K + EXTRA_ROWS, 66), K, 63))
    _exact("sgemm one-hot A rows (k = 0 .. 95) return W's columns", _same(C.t[:K, :63], Wr[:, :K].t()))
    Ar = torch.randn(65, 104, generator=g).to(DEV)
    C = _c_buffer(65, K, 99)
    sgemm(Ar, eye.to(DEV), None, 1.0, C, 65, K, K, 0, 0)
    C.check("one-hot W", _rect((65 + EXTRA_ROWS, 99), 65, K))
    _exact("sgemm one-hot W rows (k = 0 .. 95) return A's columns", _same(C.t[:65, :K], Ar[:, :K]))


def test_sgemm_row_bits_do_not_depend_on_the_row_position():
    """The sparse CLIP tail (api.cpp) projects a subset of rows and relies on a row's bits depending on its A row alone."""
    N, K = 200, 608
    g = torch.Generator().manual_seed(608)
    row = torch.randn(K, generator=g)
    W = (0.05 * torch.randn(N, K, generator=g)).to(DEV)
    bias = (0.1 * torch.randn(N, generator=g)).to(DEV)
    outs = []
    for M in (1, 65, 130):
        A = torch.randn(M, K, generator=g)
        at = sorted({m for m in (0, 31, 63, 64, M - 1) if m < M})
        A[at] = row
        C = _c_buffer(M, N, N)
        sgemm(A.to(DEV), W, bias, 1.0 / 0.07, C, M, N, K, 0, 0)
        C.check("row invariance M %d" % M, _rect((M + EXTRA_ROWS, N), M, N))
        outs += [C.t[m].clone() for m in at]
    assert len(outs) == 1 + 4 + 5
    _exact("sgemm: one A row at m = 0, 31, 63, 64, M - 1 of M = 1, 65, 130", sum(_same(o, outs[0]) for o in outs[1:]))
    r = R.sgemm64(row.view(1, K).to(DEV), W, bias, 1.0 / 0.07, None, False)
    _held("k_sgemm_tn", "sgemm row invariance: the row itself", outs[0].view(1, N), r.ref, r.bar)


@pytest.mark.parametrize("K,lda,relu,resid,why", [(16, 16, 0, 0, "K < 32"), (40, 40, 0, 0, "K % 32"), (64, 66, 0, 0, "lda % 4"),
                                                  (64, 64, 1, 1, "relu with resid")])
def test_sgemm_refusals_leave_the_output_untouched(K, lda, relu, resid, why):
    A = torch.ones(8, 128, device=DEV)
    W = torch.ones(8, 128, device=DEV)
    C = Guarded((8, 8))
    sgemm(A, W, None, 1.0, C, 8, 8, K, relu, resid, lda=lda, ldw=K if lda == K else 64, expect_refusal=True)
    C.check("refused: " + why)
    print("sgemm refusal (%s): %s" % (why, _lib.load().pio_last_error().decode()))


# ------------------------------------------------------------------------------------------------ k_attention_f32 / k_text_attention_f32
SCALE = 0.125


def attention(kind, qkv, B, H, T, Tp, lens=None):
    """-> (out [B*Tp][D] clone, after the guard check: every row of [0, B Tp) is written, nothing else)."""
    D = 64 * H
    out = Guarded((B * Tp, D))
    lens_dev = None if lens is None else torch.tensor(list(lens), dtype=torch.int32, device=DEV)
    rc = _lib.load().pio_test_attention_f32(kind, qkv.data_ptr(), B, H, T, Tp, D, SCALE, None if lens is None else lens_dev.data_ptr(),
                                            out.t.data_ptr(), _stream())
    torch.cuda.synchronize()
    _lib.check(rc)
    out.check("attention_f32 kind %d" % kind, torch.ones(B * Tp, D, dtype=torch.bool, device=DEV))
    return out.t.clone()


def _poison(qkv, B, Tp, first_dead, value):
    """Rows t >= first_dead[b] of every sequence replaced by `value` (q, k and v alike)."""
    z = qkv.clone().view(B, Tp, -1)
    for b in range(B):
        z[b, first_dead[b]:] = value
    return z.view(B * Tp, -1)


def _vit_attention_cases():
    for Tp, T in R.ATTN_PLAIN:
        yield Tp, T, None
    for Tp, rows in R.ATTN_LENS.items():
        for lens in rows:
            yield Tp, Tp, lens


@pytest.mark.parametrize("H", [1, 2])
def test_attention_f32_against_float64_and_masking(H):
    B = R.ATTN_B
    seen = set()
    for Tp, T, lens in _vit_attention_cases():
        qkv = R.qkv_case(B, H, Tp, seed=2).to(DEV)
        label = "attention_f32 H %d Tp %d %s" % (H, Tp, "T %d" % T if lens is None else "lens %s" % (lens,))
        got = attention(0, qkv, B, H, T, Tp, lens)
        r = R.attention64(qkv, B, H, Tp, SCALE, lens=lens, T=T)
        _held("k_attention_f32", label, got[r.live], r.out[r.live], r.bar[r.live])
        dead = got[~r.live]
        _exact(label + ": rows len <= t < Tp are +0.0", int((_bits(dead) != 0).sum()) if dead.numel() else 0)
        first_dead = [T] * B if lens is None else list(lens)
        seen.update(first_dead)
        for value in (float("nan"), 1e30):
            again = attention(0, _poison(qkv, B, Tp, first_dead, value), B, H, T, Tp, lens)
            _exact(label + ": rows >= len set to %s, every output keeps its bits" % value, _same(again, got))
    assert {0, 1, 63, 64, 65, 72, 136} <= seen


@pytest.mark.parametrize("H", [1, 2])
def test_text_attention_f32_against_float64_future_keys_and_tp_invariance(H):
    N, D = R.TEXT_N, 64 * H
    outs = {}
    for Tp in R.TEXT_TP:
        qkv = R.qkv_case(N, H, Tp, seed=3).to(DEV)
        label = "text_attention_f32 H %d Tp %d" % (H, Tp)
        got = attention(1, qkv, N, H, Tp, Tp)
        outs[Tp] = got.view(N, Tp, D)
        r = R.attention64(qkv, N, H, Tp, SCALE, causal=True)
        _held("k_text_attention_f32", label, got, r.out, r.bar)
        for t0 in sorted({t for t in (0, 63, 64, Tp - 2) if 0 <= t < Tp - 1}):
            again = attention(1, _poison(qkv, N, Tp, [t0 + 1] * N, float("nan")), N, H, Tp, Tp).view(N, Tp, D)
            _exact(label + ": rows > %d NaN, rows <= %d keep their bits" % (t0, t0), _same(again[:, :t0 + 1], outs[Tp][:, :t0 + 1]))
            assert bool(torch.isnan(again[:, t0 + 1:]).all())          # and the poisoned queries do say so
    _exact("text_attention_f32 H %d: rows at Tp = 80 equal Tp = 72" % H, _same(outs[80][:, :72], outs[72]))
    _exact("text_attention_f32 H %d: rows at Tp = 80 equal Tp = 8" % H, _same(outs[80][:, :8], outs[8]))


def test_attention_f32_refusals():
    L = _lib.load()
    qkv = torch.zeros(8, 192, device=DEV)
    out = Guarded((8, 64))
    lens = torch.ones(1, dtype=torch.int32, device=DEV)
    for args in ((2, 1, 1, 8, 8, 64, None), (0, 1, 1, 9, 8, 64, None), (0, 1, 1, 0, 8, 64, None), (0, 1, 2, 8, 8, 64, None),
                 (1, 1, 1, 8, 8, 64, lens.data_ptr())):
        kind, B, H, T, Tp, D, ln = args
        assert L.pio_test_attention_f32(kind, qkv.data_ptr(), B, H, T, Tp, D, SCALE, ln, out.t.data_ptr(), _stream()) == ERR_INVALID, args
        assert L.pio_last_error()
    torch.cuda.synchronize()
    out.check("attention_f32 refusals")


# ------------------------------------------------------------------------------------------------ k_layernorm_f32
def layernorm(x, w, b, eps, y):
    M, D = x.shape
    rc = _lib.load().pio_test_layernorm_f32(x.data_ptr(), w.data_ptr(), b.data_ptr(), eps, M, D, y.data_ptr(), _stream())
    torch.cuda.synchronize()
    _lib.check(rc)


@pytest.mark.parametrize("D", R.LN_D)
def test_layernorm_f32_against_float64_and_in_place(D):
    for M in R.LN_M:
        c = R.ln_case(M, D)
        x, w, b = c.x.to(DEV), c.w.to(DEV), c.b.to(DEV)
        y = Guarded((M, D))
        layernorm(x, w, b, c.eps, y.t)
        y.check("layernorm_f32", torch.ones(M, D, dtype=torch.bool, device=DEV))
        r = R.layernorm64(x, w, b, c.eps)
        _held("k_layernorm_f32", "layernorm_f32 M %d D %d" % (M, D), y.t, r.ref, r.bar)
        z = Guarded((M, D))                                  # y == x, as api.cpp calls it for the CLIP pre-norm
        z.t.copy_(x)
        layernorm(z.t, w, b, c.eps, z.t)
        z.check("layernorm_f32 in place", torch.ones(M, D, dtype=torch.bool, device=DEV))
        _exact("layernorm_f32 M %d D %d in place == out of place" % (M, D), _same(z.t, y.t))
    L = _lib.load()
    y = Guarded((4, 64))
    for M_, D_, eps in ((0, 64, 1e-5), (4, 0, 1e-5), (4, 64, 0.0)):
        assert L.pio_test_layernorm_f32(y.t.data_ptr(), y.t.data_ptr(), y.t.data_ptr(), eps, M_, D_, y.t.data_ptr(), _stream()) == ERR_INVALID
    torch.cuda.synchronize()
    y.check("layernorm_f32 refusals")


# ------------------------------------------------------------------------------------------------ pointwise
OPN = {R.GELU_ERF: "k_gelu_f32 erf", R.QUICKGELU: "k_gelu_f32 quick", R.TANH: "k_activation_f32 tanh", R.SIGMOID: "k_activation_f32 sigmoid"}


@pytest.mark.parametrize("n", R.POINTWISE_N)
def test_pointwise_f32_against_float64(n):
    L = _lib.load()
    v = R.pointwise_values(n).to(DEV)
    for op in (R.GELU_ERF, R.QUICKGELU, R.TANH, R.SIGMOID):
        y = Guarded((n,))
        y.t.copy_(v)
        _lib.check(L.pio_test_pointwise_f32(op, y.t.data_ptr(), n, None, None, 0, _stream()))
        torch.cuda.synchronize()
        y.check(OPN[op], torch.ones(n, dtype=torch.bool, device=DEV))
        r = R.pointwise64(op, v)
        _held(OPN[op], "%s n %d" % (OPN[op], n), y.t, r.ref, r.bar)
    D = 100                                                  # 100 does not divide 256, and no n here is a multiple of both
    g = torch.Generator().manual_seed(n)
    aux, ls = torch.randn(n, generator=g).to(DEV), (0.1 * torch.randn(D, generator=g)).to(DEV)
    x = Guarded((n,))
    x.t.copy_(v)
    _lib.check(L.pio_test_pointwise_f32(R.RESID_LS, x.t.data_ptr(), n, aux.data_ptr(), ls.data_ptr(), D, _stream()))
    torch.cuda.synchronize()
    x.check("k_resid_ls_f32", torch.ones(n, dtype=torch.bool, device=DEV))
    r = R.resid_ls64(v, aux, ls)
    _held("k_resid_ls_f32", "k_resid_ls_f32 n %d D %d" % (n, D), x.t, r.ref, r.bar)
    lsi = ls.to(F64)[torch.arange(n, device=DEV) % D]
    fma = (v.to(F64) + aux.to(F64) * lsi).to(torch.float32)                       # (float64 holds the product exactly; the sum almost always)
    two = v + (aux.to(F64) * lsi).to(torch.float32)
    print("k_resid_ls_f32 n %d: %d outputs carry the one-rounding (FMA) bits, %d the two-rounding bits, %d neither"
          % (n, int((_bits(x.t) == _bits(fma)).sum()), int((_bits(x.t) == _bits(two)).sum()),
             int(((_bits(x.t) != _bits(fma)) & (_bits(x.t) != _bits(two))).sum())))


def test_pointwise_f32_refusals():
    L = _lib.load()
    y = Guarded((16,))
    p = y.t.data_ptr()
    for op, n, aux, ls, D in ((5, 16, None, None, 0), (-1, 16, None, None, 0), (0, 0, None, None, 0), (4, 16, None, p, 4), (4, 16, p, p, 4),
                              (4, 16, p + 32, p, 0)):
        assert L.pio_test_pointwise_f32(op, p, n, aux, ls, D, _stream()) == ERR_INVALID, (op, n, D)
        assert L.pio_last_error()
    torch.cuda.synchronize()
    y.check("pointwise refusals")


# ------------------------------------------------------------------------------------------------ k_im2col_f32 / k_embed_scatter_f32
@pytest.mark.parametrize("p", [14, 16, 32])
def test_im2col_f32_copies_pixels_and_leaves_the_pad_columns(p):
    """The columns >= 3 p^2 keep the sentinel: the kernel never writes them, the patch-embed GEMM multiplies them, so the forward relies
    on the one-time zero fill of its buffer."""
    L = _lib.load()
    B = 2
    kmin = (3 * p * p + 31) // 32 * 32
    for S in (2 * p, 3 * p):
        n = S // p
        imgs = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(S)).to(DEV)
        rows, cols, b, c, y, x = (z.to(DEV) for z in R.im2col_index(B, S, p))
        for Kpad in (kmin, kmin + 32):
            out = Guarded((B * n * n, Kpad))
            _lib.check(L.pio_test_im2col_f32(imgs.data_ptr(), B, S, p, Kpad, out.t.data_ptr(), _stream()))
            torch.cuda.synchronize()
            wr = _rect((B * n * n, Kpad), B * n * n, 3 * p * p)
            out.check("im2col_f32 p %d S %d Kpad %d" % (p, S, Kpad), wr)
            _exact("im2col_f32 p %d S %d Kpad %d: every written element is its pixel" % (p, S, Kpad),
                   _same(out.t[rows, cols], imgs[b, c, y, x]))
            assert rows.numel() == int(wr.sum())
    out = Guarded((4, 608))
    assert L.pio_test_im2col_f32(imgs.data_ptr(), 1, 28, 14, 576, out.t.data_ptr(), _stream()) == ERR_INVALID       # Kpad < 3 p^2
    assert L.pio_test_im2col_f32(imgs.data_ptr(), 1, 30, 14, 608, out.t.data_ptr(), _stream()) == ERR_INVALID       # S % p
    torch.cuda.synchronize()
    out.check("im2col_f32 refusals")


@pytest.mark.parametrize("G", [1, 5])
def test_embed_scatter_f32_adds_once_and_leaves_the_other_rows(G):
    L = _lib.load()
    B, D = 2, 100
    for n2 in (4, 9):
        Tp = G + n2 + 3
        g = torch.Generator().manual_seed(10 * G + n2)
        emb, pos = torch.randn(B * n2, D, generator=g).to(DEV), torch.randn(1 + n2, D, generator=g).to(DEV)
        pos[0] = float("nan")                                # the class row's position is not this kernel's to add
        x = Guarded((B * Tp, D))
        _lib.check(L.pio_test_embed_scatter_f32(emb.data_ptr(), pos.data_ptr(), B, n2, Tp, G, D, x.t.data_ptr(), _stream()))
        torch.cuda.synchronize()
        wr = torch.zeros(B, Tp, D, dtype=torch.bool, device=DEV)
        wr[:, G:G + n2] = True
        x.check("embed_scatter_f32 G %d n2 %d" % (G, n2), wr.view(B * Tp, D))
        want = emb.view(B, n2, D) + pos[1:].view(1, n2, D)                         # one IEEE fp32 add per element
        _exact("embed_scatter_f32 G %d n2 %d Tp %d D %d" % (G, n2, Tp, D), _same(x.t.view(B, Tp, D)[:, G:G + n2], want))
    x = Guarded((8, D))
    assert L.pio_test_embed_scatter_f32(emb.data_ptr(), pos.data_ptr(), 1, 4, 8, 5, D, x.t.data_ptr(), _stream()) == ERR_INVALID   # Tp < G + n2
    torch.cuda.synchronize()
    x.check("embed_scatter_f32 refusal")


# ------------------------------------------------------------------------------------------------ k_text_embed / k_text_pool
@pytest.mark.parametrize("W", [64, 100])
def test_text_embed_rows_zero_rows_and_bad_ids(W):
    L = _lib.load()
    V, N = 50, 3
    g = torch.Generator().manual_seed(W)
    tok = torch.randn(V, W, generator=g).to(DEV)
    for Lc in (1, 5, 77):
        pos = torch.randn(Lc, W, generator=g).to(DEV)
        ids = torch.randint(0, V, (N, Lc), generator=g, dtype=torch.int32)
        ids[0, 0], ids[1, Lc - 1] = 0, V - 1
        for Tp in ((Lc + 7) // 8 * 8, (Lc + 11 + 7) // 8 * 8):
            def run(id_rows):
                x, err = Guarded((N * Tp, W)), torch.zeros(1, dtype=torch.int32, device=DEV)
                d = id_rows.to(DEV)
                _lib.check(L.pio_test_text_embed(d.data_ptr(), N, Lc, Tp, V, W, tok.data_ptr(), pos.data_ptr(), x.t.data_ptr(), err.data_ptr(),
                                                 _stream()))
                torch.cuda.synchronize()
                x.check("text_embed", torch.ones(N * Tp, W, dtype=torch.bool, device=DEV))
                return x.t.view(N, Tp, W).clone(), int(err.item())
            label = "text_embed W %d L %d Tp %d" % (W, Lc, Tp)
            got, err = run(ids)
            want = torch.zeros(N, Tp, W, device=DEV)
            want[:, :Lc] = tok[ids.to(DEV).long()] + pos.view(1, Lc, W)                # one IEEE fp32 add; rows t >= L are +0.0
            _exact(label + ": tok + pos, zero rows after L", _same(got, want))
            assert err == 0
            for bad in (-1, V):
                wrong = ids.clone()
                s, t = 2, min(2, Lc - 1)
                wrong[s, t] = bad
                got2, err2 = run(wrong)
                want2 = want.clone()
                want2[s, t] = 0.0
                _exact(label + ": id %d gives a zero row, its neighbours keep their bits" % bad, _same(got2, want2))
                assert err2 == 1
    x = Guarded((8, W))
    e = torch.zeros(1, dtype=torch.int32, device=DEV)
    d = torch.zeros(8, dtype=torch.int32, device=DEV)
    for Lc, Tp in ((5, 4), (5, 12), (0, 8)):                                          # Tp < L, Tp % 8, L < 1
        assert L.pio_test_text_embed(d.data_ptr(), 1, Lc, Tp, V, W, tok.data_ptr(), tok.data_ptr(), x.t.data_ptr(), e.data_ptr(), _stream()) == ERR_INVALID
    torch.cuda.synchronize()
    x.check("text_embed refusals")


@pytest.mark.parametrize("W", [64, 512, 768, 1024])
def test_text_pool_gathers_the_first_maximum_and_projects(W):
    L = _lib.load()
    N, eps = 4, 1e-5
    for E in (1, 100, 512, 768):
        for Lc in (1, 77):
            Tp = (Lc + 7) // 8 * 8
            g = torch.Generator().manual_seed(W + 3 * E + Lc)
            ids = torch.randint(0, 100, (N, Lc), generator=g, dtype=torch.int32)
            if Lc > 1:
                ids[0, 0] = 200                               # the maximum at position 0,
                ids[1, Lc - 1] = 200                          # at L - 1,
                ids[2, 10], ids[2, 40] = 200, 200             # tied: the first wins, as torch.argmax
            eot = torch.argmax(ids.long(), dim=1)
            assert eot.tolist() == R.first_argmax(ids).tolist() and (Lc == 1 or eot.tolist()[:3] == [0, Lc - 1, 10])
            x = torch.full((N * Tp, W), float("nan"))         # every row but the EOT row is NaN: a wrong gather cannot pass
            x[torch.arange(N) * Tp + eot] = torch.randn(N, W, generator=g) * 2.0 + 0.5
            lw, lb = (1 + 0.1 * torch.randn(W, generator=g)).to(DEV), (0.1 * torch.randn(W, generator=g)).to(DEV)
            proj = (W ** -0.5 * torch.randn(W, E, generator=g)).to(DEV)
            x, ids = x.to(DEV), ids.to(DEV)
            out = Guarded((N, E))
            _lib.check(L.pio_test_text_pool(x.data_ptr(), ids.data_ptr(), N, Lc, Tp, W, E, lw.data_ptr(), lb.data_ptr(), eps, proj.data_ptr(),
                                            out.t.data_ptr(), _stream()))
            torch.cuda.synchronize()
            out.check("text_pool", torch.ones(N, E, dtype=torch.bool, device=DEV))
            r = R.text_pool64(x, ids, Tp, lw, lb, eps, proj)
            _held("k_text_pool", "text_pool W %d E %d L %d" % (W, E, Lc), out.t, r.ref, r.bar)
    out = Guarded((N, 8))
    big = torch.zeros(N * 8, 1056, device=DEV)
    rc = L.pio_test_text_pool(big.data_ptr(), ids.data_ptr(), N, 1, 8, 1056, 8, big.data_ptr(), big.data_ptr(), eps, big.data_ptr(), out.t.data_ptr(),
                              _stream())
    torch.cuda.synchronize()
    assert rc == ERR_INVALID and b"W <= 1024" in L.pio_last_error()
    out.check("text_pool W = 1056 refused")


def test_zz_worst_ratios_per_kernel():
    """The summary line of the file (runs last in file order): the worst err / bar of every kernel that has a bar."""
    for k in sorted(WORST):
        print("worst err / bar  %-28s %.3e" % (k, WORST[k]))
    assert all(v <= 1.0 for v in WORST.values())
