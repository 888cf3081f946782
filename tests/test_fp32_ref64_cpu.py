"""tests/fp32_ref64.py checked without a GPU: every float64 statement against torch's own float64 operator, and every bar shown to be
non-vacuous at every shape tests/test_gpu_fp32_kernels.py uses -- a float32 evaluation in ANOTHER summation order (torch's blocked CPU
kernels) stays inside it, and a reference with one deliberate mistake (one k index dropped, one key too many, the unbiased variance, the
last instead of the first maximum) falls outside it.  Also the C ABI of the hooks the GPU file calls: header, ctypes table, library."""
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

import fp32_ref64 as R
from conftest import ROOT

torch.set_grad_enabled(False)
F64 = torch.float64

HOOKS = {"pio_test_sgemm": 14, "pio_test_attention_f32": 11, "pio_test_layernorm_f32": 8, "pio_test_pointwise_f32": 7,
         "pio_test_im2col_f32": 7, "pio_test_embed_scatter_f32": 9, "pio_test_text_embed": 11, "pio_test_text_pool": 13}


def _ratio(label, got, ref, bar):
    r = float(((got.to(F64) - ref).abs() / bar).max())
    print("%-70s worst err / bar %.3e" % (label, r))
    return r


def test_hooks_in_header_signatures_and_library():
    from patchioner_amd import _lib, build
    build.build()
    with open(os.path.join(ROOT, "include", "patchioner_hip.h")) as f:
        header = f.read()
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "patchioner_amd", "libpatchioner_hip.so")],
                          capture_output=True, text=True, check=True).stdout
    for name, nargs in HOOKS.items():
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert re.search(r"\b%s\b" % name, syms), name
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    for name in HOOKS:
        assert name in doc, name


# ------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("shape", R.SGEMM_SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
def test_sgemm_reference_and_bar(shape):
    M, N, K, lda, ldw, ldc = shape
    c = R.sgemm_case(*shape)
    A, W, Cold = c.A[:, :K], c.W[:, :K], c.C_old[:, :N]
    worst, caught = 0.0, 1e30
    for relu, resid in R.SGEMM_FORMS:
        for bias in (None, c.bias):
            for alpha in R.SGEMM_ALPHAS:
                r = R.sgemm64(A, W, bias, alpha, Cold if resid else None, bool(relu))
                al = R.f32(alpha)
                t = al * F.linear(A.to(F64), W.to(F64))
                t = t + bias.to(F64) if bias is not None else t
                t = torch.relu(t) if relu else t
                t = t + Cold.to(F64) if resid else t
                assert float((r.ref - t).abs().max()) <= 1e-12 * float(r.mag.max())
                # fp32, torch's blocked order, epilogue in fp32
                g = torch.tensor(al, dtype=torch.float32) * (A @ W.t())
                g = g + bias if bias is not None else g
                g = torch.relu(g) if relu else g
                g = g + Cold if resid else g
                worst = max(worst, _ratio("sgemm fp32 other order %s relu %d resid %d" % (shape[:3], relu, resid), g, r.ref, r.bar))
                if not relu:                        # (ReLU hides a dropped product wherever the result is clamped)
                    wrong = R.sgemm64(A, W, bias, alpha, Cold if resid else None, False, drop_k=K // 2)
                    rows = slice(R.HEAVY_ROWS, None) if M > R.HEAVY_ROWS else slice(None)
                    caught = min(caught, float(((wrong.ref - r.ref).abs() / r.bar)[rows].max()))
    print("sgemm %s: other-order fp32 worst %.3f of the bar; one dropped k at least %.1f bars" % (shape, worst, caught))
    assert worst <= 1.0
    assert caught > 1.0
    # cancellation is present: sum |a w| >> |sum a w| on the heavy rows
    r = R.sgemm64(A, W, None, 1.0, None, False)
    if K > 32:
        assert float((r.mag[:R.HEAVY_ROWS] / r.ref[:R.HEAVY_ROWS].abs().clamp_min(1e-30)).median()) > 20


def test_sgemm_integer_case_is_exact_in_fp32():
    for shape in R.SGEMM_SHAPES:
        c = R.sgemm_int_case(*shape)
        M, N, K = shape[:3]
        top = c.A[:, :K].abs().to(F64) @ c.W[:, :K].abs().to(F64).t()
        assert float(top.max()) * 2 + 2000 < 2 ** 24          # alpha = 2 included


# ------------------------------------------------------------------------------------------------ attention
def _sdpa64(qkv, B, H, Tp, scale, mask):
    x = qkv.to(F64).view(B, Tp, 3, H, 64)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=R.f32(scale))
    return o.permute(0, 2, 1, 3).reshape(B * Tp, 64 * H)


def _attn_f32(qkv, B, H, Tp, scale, mask):
    x = qkv.view(B, Tp, 3, H, 64)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    s = (q @ k.transpose(-1, -2)) * torch.tensor(scale, dtype=torch.float32)
    s = s.masked_fill(~mask, float("-inf"))
    p = torch.softmax(s, dim=-1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B * Tp, 64 * H), s, p


def _attention_cases():
    for H in (1, 2):
        for Tp, T in R.ATTN_PLAIN:
            yield "plain", H, Tp, dict(T=T), [T] * R.ATTN_B
        for Tp, rows in R.ATTN_LENS.items():
            for lens in rows:
                yield "lens", H, Tp, dict(lens=lens), list(lens)
        for Tp in R.TEXT_TP:
            yield "causal", H, Tp, dict(causal=True), None


def test_attention_reference_and_bars():
    B = R.ATTN_B
    worst = {"out": 0.0, "score": 0.0, "prob": 0.0}
    for kind, H, Tp, kw, lens in _attention_cases():
        qkv = R.qkv_case(B, H, Tp, seed=1)
        r = R.attention64(qkv, B, H, Tp, 0.125, **kw)
        t = torch.arange(Tp)
        if kind == "causal":
            mask = (t.view(1, Tp) <= t.view(Tp, 1)).view(1, 1, Tp, Tp).expand(B, 1, Tp, Tp)
            live = torch.ones(B * Tp, dtype=torch.bool)
        else:
            ln = torch.tensor(lens).view(B, 1, 1, 1)
            mask = (t.view(1, 1, 1, Tp) < ln).expand(B, 1, Tp, Tp)
            live = (t.view(1, Tp) < ln.view(B, 1)).reshape(B * Tp)
        assert torch.equal(live, r.live)
        safe = mask | ~live.view(B, 1, Tp, 1)                     # SDPA on a row without keys is NaN: give dead rows every key, ignore them
        ref = _sdpa64(qkv, B, H, Tp, 0.125, safe)
        assert float((r.out[live] - ref[live]).abs().max()) < 1e-13 if live.any() else True
        assert float(r.out[~live].abs().max()) == 0.0 if (~live).any() else True
        assert float(r.bar[~live].abs().max()) == 0.0 if (~live).any() else True
        if not live.any():
            continue
        g, s32, p32 = _attn_f32(qkv, B, H, Tp, 0.125, safe)
        worst["out"] = max(worst["out"], _ratio("attention %s H %d Tp %d %s fp32" % (kind, H, Tp, kw), g[live], r.out[live], r.bar[live]))
        m4 = (mask & live.view(B, 1, Tp, 1)).expand(B, H, Tp, Tp)
        worst["score"] = max(worst["score"], float(((s32.to(F64) - r.scores).abs()[m4] / r.d_score[m4]).max()))
        rel = ((p32.to(F64) - r.probs).abs() / r.probs.clamp_min(1e-300))
        worst["prob"] = max(worst["prob"], float((rel / r.rel_p)[m4].max()))
        # one key too many: every query of the flat sequences (b >= 1; sequence 0's peaked rows may give the extra key no weight) that has a
        # key to spare must leave the bar
        wrong = R.attention64(qkv, B, H, Tp, 0.125, extra_key=True, **kw)
        n_keys = (t + 1).repeat(B) if kind == "causal" else torch.tensor(lens).repeat_interleave(Tp)
        spare = live & (n_keys < Tp) & (torch.arange(B * Tp) >= Tp)
        if spare.any():
            per_row = ((wrong.out - r.out).abs() / r.bar.clamp_min(1e-300))[spare].max(dim=1).values
            assert float(per_row.min()) > 1.0, (kind, H, Tp, kw, float(per_row.min()))
    print("attention: other-order fp32 worst err / bar: out %.3f, scores %.3f, probabilities %.3f" % (worst["out"], worst["score"], worst["prob"]))
    assert worst["out"] <= 1.0 and worst["score"] <= 1.0 and worst["prob"] <= 1.0
    assert worst["out"] > 1e-4                                     # the bar is within four decades of a real fp32 evaluation


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("D", R.LN_D)
def test_layernorm_reference_and_bar(D):
    for M in R.LN_M:
        c = R.ln_case(M, D)
        r = R.layernorm64(c.x, c.w, c.b, c.eps)
        t = F.layer_norm(c.x.to(F64), (D,), c.w.to(F64), c.b.to(F64), R.f32(c.eps))
        assert float((r.ref - t).abs().max()) < 1e-11
        g = F.layer_norm(c.x, (D,), c.w, c.b, c.eps)
        assert _ratio("layernorm M %d D %d fp32 (torch)" % (M, D), g, r.ref, r.bar) <= 1.0
        wrong = R.layernorm64(c.x, c.w, c.b, c.eps, unbiased=True)
        rows = [m for m in range(M) if not (M >= 4 and m in (1, 2))]             # constant rows have no variance to get wrong
        per_row = ((wrong.ref - r.ref).abs() / r.bar)[rows].max(dim=1).values
        print("layernorm M %d D %d: unbiased variance is at least %.1f bars away" % (M, D, float(per_row.min())))
        assert float(per_row.min()) > 1.0


# ------------------------------------------------------------------------------------------------ pointwise
@pytest.mark.parametrize("n", R.POINTWISE_N)
def test_pointwise_reference_and_bar(n):
    v = R.pointwise_values(n)
    x = v.to(F64)
    c32 = torch.tensor(0.70710678118654752, dtype=torch.float32)
    # (the fp32 GELU is the formula on torch.erf, not F.gelu: ATen's vectorised fp32 GELU is off by up to 1e-6 absolute near v = -3)
    for op, f64, f32 in ((R.GELU_ERF, lambda z: F.gelu(z), lambda z: 0.5 * z * (1.0 + torch.erf(z * c32))),
                         (R.QUICKGELU, lambda z: z * torch.sigmoid(1.702 * z), lambda z: z * torch.sigmoid(1.702 * z)),
                         (R.TANH, torch.tanh, torch.tanh), (R.SIGMOID, torch.sigmoid, torch.sigmoid)):
        r = R.pointwise64(op, v)
        assert float((r.ref - f64(x)).abs().max()) <= 1e-14 * max(1.0, float(x.abs().max()))
        assert _ratio("pointwise op %d n %d fp32 (torch)" % (op, n), f32(v), r.ref, r.bar) <= 1.0
        # non-vacuous: the bar is a few ulp of the result (or of |v| where 1 + erf cancels), never a loose absolute number
        assert float((r.bar / (x.abs() + r.ref.abs() + 1e-30)).max()) < 400 * R.U + 1e-7 or n == 1
    D = 100
    g = torch.Generator().manual_seed(n)
    y, ls = torch.randn(n, generator=g), 0.1 * torch.randn(D, generator=g)
    r = R.resid_ls64(v, y, ls)
    two = v + y * ls[torch.arange(n) % D]
    assert _ratio("resid_ls n %d two roundings" % n, two, r.ref, r.bar) <= 1.0
    fma = (v.to(F64) + y.to(F64) * ls.to(F64)[torch.arange(n) % D]).to(torch.float32)
    assert _ratio("resid_ls n %d one rounding" % n, fma, r.ref, r.bar) <= 1.0
    wrong = v.to(F64) + y.to(F64) * ls.to(F64)[(torch.arange(n) + 1) % D]      # ls indexed off by one
    assert float(((wrong - r.ref).abs() / r.bar).max()) > 1.0


# ------------------------------------------------------------------------------------------------ copies and the pool
@pytest.mark.parametrize("p,S", [(14, 28), (16, 48), (32, 64)])
def test_im2col_index_is_the_conv_unfold(p, S):
    B, n = 2, S // p
    imgs = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(p))
    rows, cols, b, c, y, x = R.im2col_index(B, S, p)
    out = torch.zeros(B * n * n, 3 * p * p)
    out[rows, cols] = imgs[b, c, y, x]
    ref = F.unfold(imgs, kernel_size=p, stride=p).transpose(1, 2).reshape(B * n * n, 3 * p * p)
    assert torch.equal(out, ref)
    assert rows.numel() == out.numel() and torch.unique(rows * 3 * p * p + cols).numel() == out.numel()


def test_first_argmax_and_text_pool():
    ids = torch.tensor([[9, 1, 2, 3], [0, 1, 2, 9], [1, 9, 3, 9], [5, 5, 5, 5]], dtype=torch.int32)
    assert R.first_argmax(ids).tolist() == [0, 3, 1, 0] == torch.argmax(ids.long(), dim=1).tolist()
    assert R.first_argmax(ids, second=True).tolist() == [0, 3, 3, 3]
    for W, E in ((64, 1), (512, 100), (768, 512), (1024, 768)):
        for L in (1, 77):
            Tp = (L + 7) // 8 * 8
            g = torch.Generator().manual_seed(W + E + L)
            N = 3
            ids = torch.randint(0, 100, (N, L), generator=g, dtype=torch.int32)
            if L > 1:
                ids[0, 0] = 200
                ids[1, L - 1] = 200
                ids[2, 10] = 200
                ids[2, 40] = 200
            x = torch.randn(N * Tp, W, generator=g)
            lw, lb, proj = 1 + 0.1 * torch.randn(W, generator=g), 0.1 * torch.randn(W, generator=g), W ** -0.5 * torch.randn(W, E, generator=g)
            r = R.text_pool64(x, ids, Tp, lw, lb, 1e-5, proj)
            assert r.eot.tolist() == torch.argmax(ids.long(), dim=1).tolist()
            rows = x[torch.arange(N) * Tp + r.eot]
            t = F.layer_norm(rows.to(F64), (W,), lw.to(F64), lb.to(F64), R.f32(1e-5)) @ proj.to(F64)
            assert float((r.ref - t).abs().max()) < 1e-11
            g32 = F.layer_norm(rows, (W,), lw, lb, 1e-5) @ proj
            assert _ratio("text pool W %d E %d L %d fp32 (torch)" % (W, E, L), g32, r.ref, r.bar) <= 1.0
            if L > 1:
                wrong = R.text_pool64(x, ids, Tp, lw, lb, 1e-5, proj, second=True)
                assert wrong.eot.tolist()[2] == 40 and r.eot.tolist()[2] == 10
                assert float(((wrong.ref - r.ref).abs() / r.bar)[2].max()) > 1.0
                assert float(((wrong.ref - r.ref).abs())[:2].max()) == 0.0
