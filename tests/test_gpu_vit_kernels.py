"""Every ViT block kernel on its own (through the C ABI's test hooks) against the float64 statements of tests/vit_ref64.py: the four GEMM
kernels in all their instantiated (epilogue, path) forms, the flash attention at every last-tile branch, the text tower's causal attention
and LayerNorm, for fp16 and bf16 operands, at the product's shapes (ViT-S / B / L at 224^2 and 518^2, CLIP B/16, small crops).

Four kinds of check:
  a. bit-exact constructions (no tolerance): one-hot rows of A pick single weights, and W holds every finite value of the operand type,
     subnormals included, so each output is one weight passed through its epilogue: q / k / V^T must carry the weight's bits, the fp32
     outputs must equal the float32 emulation of their epilogue's order, GELU / QuickGELU are held to float64 over their whole finite range.
  b. realistic operands against float64 with a per-element bar derived from the accumulation depth (below).
  c. cross-path bits: every path that fits a shape gives the same bits (kernels.h: the arithmetic every GEMM kernel follows).
  d. guard bands: every output buffer has slack before and after and a sentinel in every slot the kernel's store guards leave alone.

GEMM bar (b).  u = 2^-24.  A K-term sum on v_mfma_f32_32x32x16 takes K / 16 MFMA steps of 16 products; count two roundings per step (the
16-product block and its add into the accumulator) and a factor 2 for the MFMA's unspecified internal rounding, plus two roundings of the
epilogue (bias, then the position row / the old x): c = 2 (2 K / 16 + 2), and per element
    |got - ref| <= c u (sum_k |a||w| + |x| + |b| + |pos|)  (+ 1 ulp of the output type where the output is fp16 / bf16).
At the largest K tested (4096, ViT-L fc2) c = 1028, c u = 6.1e-5 of sum |a||w|; a dropped 64-wide K-tile moves an element by about
sqrt(64) sigma_aw against sum |a||w| ~ 0.64 K sigma_aw: 3e-3 of it, 50x the bar; one missing product (0.64 sigma_aw typical, and the
maximum over ~10^6 elements is taken) moves it by 2.4e-4 of it, 4x the bar.
GELU outputs add |GELU'| <= 1.13 on the pre-activation error plus the approximation common.h states for gelu_erf: 7.5e-7 absolute on
[-12, 12], |v| 6.25e-8 beyond (the clamp at u = 4.3 sqrt 2 leaves |v| erfc(4.3) / 2 = 6e-10 |v|).  QuickGELU: |d/dv v sigma(1.702 v)| <=
1.1, and v_exp_f32 / v_rcp_f32 (1 ulp each) plus the rounded exponent argument give at most 4 u |v| (the argument error enters as
1.702 |v| sigma (1 - sigma) <= 0.28 relative).
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import vit_ref64 as R
from patchioner_amd import _lib

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

U = 2.0 ** -24
F64 = torch.float64
OPS = {0: torch.float16, 1: torch.bfloat16}
OPN = {0: "fp16", 1: "bf16"}
PE, QKV, RES, GELU = 0, 1, 2, 3
EPN = {PE: "patch", QKV: "qkv", RES: "resid", GELU: "gelu"}
AUTO, NARROW, RES128, WIDE128, K256, ROLL = 0, 1, 2, 3, 4, 5
PN = {AUTO: "AUTO", NARROW: "NARROW", RES128: "RES128", WIDE128: "WIDE128", K256: "K256", ROLL: "ROLL"}
# the (epilogue, path) pairs the library instantiates (vit_gemm.hip launch_typed, vit_gemm256.hip, vit_gemm_roll.hip)
INSTANTIATED = {(PE, NARROW), (PE, K256), (QKV, WIDE128), (QKV, K256), (QKV, ROLL), (RES, NARROW), (RES, RES128), (RES, ROLL),
                (GELU, WIDE128), (GELU, K256), (GELU, ROLL)}
ERR_INVALID = -1
TALLY_RAN = {}       # (operand, epi, path) -> launches
TALLY_REFUSED = {}   # (operand, epi, path) -> refusals asserted

SLACK = 2048
SENT = {4: 0x7FBADBAD, 2: 0x7DAD}   # fp32 NaN / fp16 NaN (bf16: a finite 2.9e37 that no test output takes)


def _report(label, observed, bar=None):
    if bar is None:
        print("%-72s observed %.3e   (exact)" % (label, observed))
        assert observed == 0, "%s: %d elements differ" % (label, observed)
    else:
        print("%-72s observed %.3e   bar %.3e" % (label, observed, bar))
        assert observed <= bar, "%s: %.3e above its bar %.3e" % (label, observed, bar)


class Guarded:
    """A device buffer with SLACK elements of sentinel before and after, the region between filled with the sentinel too."""

    def __init__(self, shape, dtype):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.full = torch.empty(self.n + 2 * SLACK, dtype=dtype, device="cuda")
        self.isz = self.full.element_size()
        self.ints().fill_(self._sent())
        self.t = self.full[SLACK:SLACK + self.n].view(self.shape)

    def _sent(self):
        s = SENT[self.isz]
        return s - (1 << 32) if (self.isz == 4 and s >= 1 << 31) else s

    def ints(self):
        return self.full.view(torch.int32 if self.isz == 4 else torch.int16)

    def check(self, label, written):
        """Everything outside `written` (bool, self.shape) must still hold the sentinel; the slack always."""
        iv, s = self.ints(), self._sent()
        assert bool((iv[:SLACK] == s).all()) and bool((iv[SLACK + self.n:] == s).all()), label + ": store outside the buffer"
        inner = iv[SLACK:SLACK + self.n].view(self.shape)
        bad = int((inner[~written] != s).sum())
        assert bad == 0, "%s: %d elements written outside the kernel's contract" % (label, bad)


def _ulp(y, op):
    """Spacing of the operand type at |y| (subnormal spacing below its normal range)."""
    p, emin = (11, -14) if op == 0 else (8, -126)
    e = torch.floor(torch.log2(y.to(F64).abs().clamp_min(2.0 ** emin)))
    return torch.pow(2.0, e - (p - 1))


def _ptr(t):
    return None if t is None else t.data_ptr()


def gemm(op, epi, path, A, W, bias, M, N, K, x=None, pos=None, out16=None, q=None, k=None, vT=None, cap=None, T=0, Tp=0, Tk=0, G=0,
         n2=0, D=0, H=0, act=0, pf=None, expect_refusal=False):
    L = _lib.load()
    a = _lib.PioTestGemmArgs(_ptr(A), _ptr(W), _ptr(bias), M, N, K, A.shape[1], _ptr(x), _ptr(pos), _ptr(out16), _ptr(q), _ptr(k),
                             _ptr(vT), _ptr(cap), T, Tp, Tk, G, n2, D, H, act, _ptr(pf), 0 if pf is None else pf.numel() * pf.element_size())
    taken = ctypes.c_int32(-7)
    rc = L.pio_test_vit_gemm(op, epi, path, ctypes.byref(a), ctypes.byref(taken), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if expect_refusal:
        assert rc == ERR_INVALID, "%s %s on %s was not refused (rc %d)" % (OPN[op], EPN[epi], PN[path], rc)
        assert L.pio_last_error(), "refusal without a message"
        TALLY_REFUSED[(op, epi, path)] = TALLY_REFUSED.get((op, epi, path), 0) + 1
        return None
    _lib.check(rc)
    assert path == AUTO or taken.value == path
    TALLY_RAN[(op, epi, taken.value)] = TALLY_RAN.get((op, epi, taken.value), 0) + 1
    return taken.value


def route(epi, M, N, K, D, Tp, capture=False):
    return _lib.load().pio_test_gemm_route(epi, M, N, K, K, D, Tp, int(capture))


# ------------------------------------------------------------------------------------------------ one GEMM case, every output buffer
class Case:
    """Operands and guarded outputs of one GEMM; run(path) launches it and returns the outputs (cloned) after the guard checks."""

    def __init__(self, op, epi, M, N, K, D, H=0, T=0, Tp=0, Tk=0, G=0, n2=0, act=0, capture=False):
        self.op, self.epi, self.M, self.N, self.K, self.D, self.H = op, epi, M, N, K, D, H
        self.T, self.Tp, self.Tk, self.G, self.n2, self.act, self.capture = T, Tp, Tk, G, n2, act, capture
        self.B = M // n2 if epi == PE else (M // Tp if epi == QKV else 0)
        self.x0 = None
        self.pos = None

    def outputs(self):
        dt, o = OPS[self.op], {}
        if self.epi == PE:
            o["x"] = Guarded((self.B * self.Tp, self.D), torch.float32)
        elif self.epi == RES:
            o["x"] = Guarded((self.M, self.N), torch.float32)
            o["x"].t.copy_(self.x0)
        elif self.epi == GELU:
            o["out16"] = Guarded((self.M, self.N), dt)
        else:
            o["q"] = Guarded((self.B, self.H, self.Tk, 64), dt)
            o["k"] = Guarded((self.B, self.H, self.Tk, 64), dt)
            o["vT"] = Guarded((self.B, self.H, 64, self.Tk), dt)
            if self.capture:
                o["cap"] = Guarded((self.B, self.T, 3 * self.D), torch.float32)
        return o

    def written(self, name):
        """The contract of the kernels' store guards (vit_gemm.hip / vit_gemm256.hip / vit_gemm_roll.hip epilogues)."""
        dev = "cuda"
        if name == "x" and self.epi == PE:     # rows b Tp + G + p, p < n2: never the global rows nor the padding rows
            w = torch.zeros(self.B, self.Tp, self.D, dtype=torch.bool, device=dev)
            w[:, self.G:self.G + self.n2] = True
            return w.view(self.B * self.Tp, self.D)
        if name in ("x", "out16"):              # rows < M
            return torch.ones(self.M, self.N, dtype=torch.bool, device=dev)
        if name in ("q", "k"):                  # token slots t < Tp; [Tp, Tk) is left to the caller (zero padding)
            w = torch.zeros(self.B, self.H, self.Tk, 64, dtype=torch.bool, device=dev)
            w[:, :, :self.Tp] = True
            return w
        if name == "vT":
            w = torch.zeros(self.B, self.H, 64, self.Tk, dtype=torch.bool, device=dev)
            w[:, :, :, :self.Tp] = True
            return w
        return torch.ones(self.B, self.T, 3 * self.D, dtype=torch.bool, device=dev)   # capture: rows t < T only (the buffer)

    def run(self, path, A, W, bias, pf=None, expect_refusal=False):
        o = self.outputs()
        g = lambda n: o[n].t if n in o else None  # noqa: E731
        taken = gemm(self.op, self.epi, path, A, W, bias, self.M, self.N, self.K, x=g("x"), pos=self.pos, out16=g("out16"), q=g("q"),
                     k=g("k"), vT=g("vT"), cap=g("cap"), T=self.T, Tp=self.Tp, Tk=self.Tk, G=self.G, n2=self.n2, D=self.D, H=self.H,
                     act=self.act, pf=pf, expect_refusal=expect_refusal)
        label = "%s %s %s" % (OPN[self.op], EPN[self.epi], PN[path])
        for n, buf in o.items():
            if expect_refusal and n == "x" and self.epi == RES:      # refused: the residual stream keeps its old bits
                buf.check(label + " refused " + n, torch.ones(buf.shape, dtype=torch.bool, device="cuda"))
                assert _same_bits(buf.t, self.x0) == 0, label + ": refused, yet x changed"
            elif expect_refusal:                # refused: nothing launched, nothing written
                buf.check(label + " refused " + n, torch.zeros(buf.shape, dtype=torch.bool, device="cuda"))
            elif n == "x" and self.epi == RES:
                buf.check(label + " " + n, torch.ones(buf.shape, dtype=torch.bool, device="cuda"))
            else:
                buf.check(label + " " + n, self.written(n))
        if expect_refusal:
            return None, None
        return taken, {n: b.t.clone() for n, b in o.items()}

    def paths(self):
        return [p for p in (NARROW, RES128, WIDE128, K256, ROLL) if (self.epi, p) in INSTANTIATED]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b):
    return int((_bits(a) != _bits(b)).sum())


# product shapes: (name, D, H, T, Tp, Tk, B)
SHAPES = {
    "S224": (384, 6, 261, 264, 320, 3), "B224": (768, 12, 261, 264, 320, 3), "L224": (1024, 16, 261, 264, 320, 1),
    "S518": (384, 6, 1374, 1376, 1408, 1), "B518": (768, 12, 1374, 1376, 1408, 1), "L518": (1024, 16, 1374, 1376, 1408, 1),
    "CLIP16": (768, 12, 197, 200, 256, 3),
    "crop14": (768, 12, 6, 8, 64, 5), "crop28": (768, 12, 9, 16, 64, 5), "crop56": (384, 6, 21, 24, 64, 7),
}


def _gemm_case(op, epi, shape, K=None, act=0, capture=False, n2=None, G=5, seed=0):
    D, H, T, Tp, Tk, B = SHAPES[shape]
    if epi == PE:
        n2 = n2 or (T - G)
        c = Case(op, PE, B * n2, D, K, D, H, T, Tp, Tk, G, n2)
    elif epi == QKV:
        c = Case(op, QKV, B * Tp, 3 * D, D, D, H, T, Tp, Tk, capture=capture)
    elif epi == GELU:
        c = Case(op, GELU, B * Tp, 4 * D, D, D, act=act, Tp=Tp)
    else:
        c = Case(op, RES, B * Tp, D, K, D, Tp=Tp)
    return c


def _operands(c, seed, ls=None):
    g = torch.Generator(device="cuda").manual_seed(seed)
    dt = OPS[c.op]
    A = torch.randn(c.M, c.K, generator=g, device="cuda").to(dt)
    W = (torch.randn(c.N, c.K, generator=g, device="cuda") / math.sqrt(c.K))
    bias = 0.1 * torch.randn(c.N, generator=g, device="cuda")
    if ls is not None:                          # LayerScale folded as api.cpp does: W' = op(ls W) in fp32, b' = ls b
        W, bias = W * ls[:, None], bias * ls
    W = W.to(dt)
    if c.epi == RES:
        c.x0 = torch.randn(c.M, c.N, generator=g, device="cuda")
    if c.epi == PE:
        c.pos = 0.1 * torch.randn(1 + c.n2, c.D, generator=g, device="cuda")
    return A, W.contiguous(), bias.contiguous()


def _reference(c, A, W, bias):
    """(float64 reference, per-element bar) of every output, NaN where the kernel writes nothing."""
    acc, mag = R.gemm64(A, W), R.mag64(A, W)
    cK = 2.0 * (2.0 * c.K / 16 + 2)
    b64 = bias.to(F64)
    refs = {}
    if c.epi == PE:
        ref = R.patch_embed64(acc, bias, c.pos, c.n2, c.Tp, c.G)
        m = R.patch_embed64(mag, bias.abs(), c.pos.abs(), c.n2, c.Tp, c.G)
        refs["x"] = (ref, cK * U * m)
    elif c.epi == RES:
        ref = R.residual64(A, W, c.x0, bias)
        refs["x"] = (ref, cK * U * (mag + c.x0.to(F64).abs() + b64.abs()))
    elif c.epi == GELU:
        v = acc + b64
        vm = mag + b64.abs()
        if c.act == 0:
            ref = R.gelu_erf64(v)
            bar = 1.13 * cK * U * vm + 7.5e-7 * torch.clamp(v.abs() / 12, min=1.0) + _ulp(ref, c.op)
        else:
            ref = R.quick_gelu64(v)
            bar = 1.1 * cK * U * vm + 4 * U * v.abs() + _ulp(ref, c.op)
        refs["out16"] = (ref, bar)
    else:
        C = acc + b64
        q, k, vT = R.qkv_split64(C, c.B, c.Tp, c.Tk, c.H)
        mq, mk, mv = R.qkv_split64(mag + b64.abs(), c.B, c.Tp, c.Tk, c.H)
        refs["q"] = (q, cK * U * mq + _ulp(q.nan_to_num(), c.op))
        refs["k"] = (k, cK * U * mk + _ulp(k.nan_to_num(), c.op))
        refs["vT"] = (vT, cK * U * mv + _ulp(vT.nan_to_num(), c.op))
        if c.capture:
            refs["cap"] = (R.capture64(C, c.B, c.Tp, c.T), cK * U * R.capture64(mag + b64.abs(), c.B, c.Tp, c.T))
    return refs


def _check_against(label, outs, refs):
    for n, (ref, bar) in refs.items():
        got = outs[n].to(F64)
        sel = ~torch.isnan(ref)
        err = (got[sel] - ref[sel]).abs()
        assert not bool(torch.isnan(err).any()), label + " " + n + ": NaN"
        ratio = float((err / bar[sel]).max())
        _report("%s %s (max err / bar)" % (label, n), ratio, 1.0)


# ------------------------------------------------------------------------------------------------ b + c + d: realistic operands
REAL_CASES = [
    # (epilogue, shape, K, act, capture)
    (QKV, "S224", None, 0, False), (QKV, "B224", None, 0, True), (QKV, "B224", None, 0, False), (QKV, "L224", None, 0, False),
    (QKV, "B518", None, 0, False), (QKV, "L518", None, 0, True), (QKV, "CLIP16", None, 0, False), (QKV, "crop14", None, 0, True),
    (QKV, "crop56", None, 0, False),
    (GELU, "S224", None, 0, False), (GELU, "B224", None, 0, False), (GELU, "L224", None, 0, False), (GELU, "B518", None, 0, False),
    (GELU, "CLIP16", None, 1, False), (GELU, "B224", None, 1, False), (GELU, "crop28", None, 0, False),
    (RES, "S224", 384, 0, False), (RES, "S224", 1536, 0, False), (RES, "B224", 768, 0, False), (RES, "B224", 3072, 0, False),
    (RES, "L224", 4096, 0, False), (RES, "S518", 384, 0, False), (RES, "B518", 768, 0, False), (RES, "CLIP16", 768, 0, False),
    (RES, "crop14", 768, 0, False), (RES, "B224", 512, 0, False), (RES, "B224", 640, 0, False),
    (PE, "B224", 640, 0, False), (PE, "CLIP16", 768, 0, False), (PE, "crop14", 3072, 0, False), (PE, "B518", 640, 0, False),
]


def _real_id(c):
    e, s, K, act, cap = c
    return "%s-%s%s%s%s" % (EPN[e], s, "-K%d" % K if K else "", "-quick" if act else "", "-cap" if cap else "")


@pytest.mark.parametrize("op", [0, 1], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", REAL_CASES, ids=[_real_id(c) for c in REAL_CASES])
def test_gemm_paths_against_float64(op, case):
    """Every path that fits the shape: the float64 bar (b) on the first, identical bits on the others (c), guard bands on all (d); the
    paths that do not fit are asserted refused.  Residual cases carry LayerScale from 1e-5 to 3 across the columns."""
    epi, shape, K, act, cap = case
    if epi == PE and shape == "CLIP16":
        c = _gemm_case(op, PE, shape, K, G=1, n2=196)
    elif epi == PE and shape == "crop14":         # patch 32 at 224^2: 7 x 7 patches, one global token
        c = Case(op, PE, 5 * 49, 768, 3072, 768, 12, 50, 56, 64, 1, 49)
    else:
        c = _gemm_case(op, epi, shape, K, act=act, capture=cap)
    ls = None
    if epi == RES:
        ls = torch.logspace(math.log10(1e-5), math.log10(3.0), c.N, device="cuda")[torch.randperm(c.N, generator=torch.Generator().manual_seed(1)).cuda()]
    A, W, bias = _operands(c, seed=sum(map(ord, _real_id(case))) * 7 + op, ls=ls)
    label = "%s %s" % (OPN[op], _real_id(case))
    first = None
    for p in c.paths():
        fits = _fits(c, p)
        if not fits:
            c.run(p, A, W, bias, expect_refusal=True)
            continue
        _, outs = c.run(p, A, W, bias)
        if first is None:
            first = (p, outs)
            _check_against(label + " " + PN[p], outs, _reference(c, A, W, bias))
        else:
            diff = sum(_same_bits(outs[n], first[1][n]) for n in outs)
            _report("%s %s vs %s (elements with other bits)" % (label, PN[p], PN[first[0]]), diff)
    assert first is not None, label + ": no path fits"
    taken, outs = c.run(AUTO, A, W, bias)
    assert taken == route(epi, c.M, c.N, c.K, c.D, c.Tp if c.Tp else 8, cap)
    _report("%s AUTO (= %s) vs %s" % (label, PN[taken], PN[first[0]]), sum(_same_bits(outs[n], first[1][n]) for n in outs))


def _fits(c, p):
    """The kernels' own preconditions (vit_gemm.hip gemm128_fits / lazy_join_ok, vit_gemm256.hip and vit_gemm_roll.hip *_fits)."""
    nk = c.K // 64
    if p in (NARROW, RES128, WIDE128):
        return p != RES128 or nk >= 10
    if p == K256:
        return c.N % 256 == 0 and (c.epi != QKV or c.D % 256 == 0)
    if c.epi == RES:
        return c.N % 256 == 0 and nk >= 12
    if c.epi == QKV and (c.capture or c.D % 256 != 0):
        return False
    return c.N % 256 == 0 and c.Tp >= 256


# ------------------------------------------------------------------------------------------------ a: one-hot rows, every finite weight
def _finite_patterns(op):
    b = torch.arange(-32768, 32768, dtype=torch.int32)
    expo = (b & 0x7C00) == 0x7C00 if op == 0 else (b & 0x7F80) == 0x7F80
    return b[~expo].to(torch.int16)


ONEHOT = [(e, p, v) for (e, p) in sorted(INSTANTIATED) for v in ((0, False), (1, False), (0, True)) if
          (e == GELU or v[0] == 0) and (e == QKV and p != ROLL or not v[1])]


def _onehot_id(x):
    e, p, (act, cap) = x
    return "%s-%s%s%s" % (EPN[e], PN[p], "-quick" if act else "", "-cap" if cap else "")


@pytest.mark.parametrize("op", [0, 1], ids=["fp16", "bf16"])
@pytest.mark.parametrize("which", ONEHOT, ids=[_onehot_id(x) for x in ONEHOT])
def test_gemm_onehot_sweeps_every_finite_weight(op, which):
    """A[m][pi(m)] = 1 (pi(m) = (7 m + 3) mod K reaches every column: M >= K), W = every finite value of the operand type, subnormals
    included, so C[m][n] = W[n][pi(m)] exactly and every weight passes through the epilogue: q / k / V^T carry W's bits (bias 0; -0 comes
    out +0, the sum starts at +0), the capture, patch embedding and residual equal the float32 emulation of their order
    (fl(W + b), fl(fl(W + b) + pos), fl(fl(W + x) + b)), GELU / QuickGELU are within their bar of float64 over the whole finite range."""
    epi, path, (act, cap) = which
    dt = OPS[op]
    if epi == PE:
        c = Case(op, PE, 3 * 256, 768, 640, 768, 12, 261, 264, 320, 5, 256)
    elif epi == QKV:
        c = Case(op, QKV, 3 * 264, 2304, 768, 768, 12, 261, 264, 320, capture=cap)
    elif epi == GELU:
        c = Case(op, GELU, 3 * 264, 3072, 768, 768, act=act, Tp=264)
    else:
        c = Case(op, RES, 3 * 264, 768, 768, 768, Tp=264)
    pat = _finite_patterns(op).cuda()
    perm = torch.randperm(pat.numel(), generator=torch.Generator().manual_seed(op)).cuda()
    reps = -(-c.N * c.K // pat.numel())
    W = pat[perm].repeat(reps)[:c.N * c.K].view(c.N, c.K).view(dt).contiguous()
    m = torch.arange(c.M, device="cuda")
    pi = (7 * m + 3) % c.K
    A = torch.zeros(c.M, c.K, dtype=dt, device="cuda")
    A[m, pi] = 1
    g = torch.Generator(device="cuda").manual_seed(5)
    bias = torch.zeros(c.N, device="cuda") if epi in (QKV, GELU) else torch.randn(c.N, generator=g, device="cuda")
    if epi == RES:
        c.x0 = torch.randn(c.M, c.N, generator=g, device="cuda") * 4
    if epi == PE:
        c.pos = torch.randn(1 + c.n2, c.D, generator=g, device="cuda")
    taken, outs = c.run(path, A, W, bias)
    Cw = W.float()[:, pi].t().contiguous()        # [M][N] fp32: the one product each element holds
    label = "%s onehot %s" % (OPN[op], _onehot_id(which))
    if epi == QKV:
        C32 = (Cw + 0.0) + bias
        q, k, vT = R.qkv_split64(C32, c.B, c.Tp, c.Tk, c.H)
        for n, ref in (("q", q), ("k", k), ("vT", vT)):
            sel = ~torch.isnan(ref)
            _report(label + " " + n + " bits", _same_bits(outs[n][sel], ref[sel].to(dt)))
        if cap:
            _report(label + " capture bits", _same_bits(outs["cap"], C32.view(c.B, c.Tp, -1)[:, :c.T]))
    elif epi == PE:
        e32 = ((Cw + 0.0) + bias) + c.pos[1:1 + c.n2].repeat(c.B, 1)
        got = outs["x"].view(c.B, c.Tp, c.D)[:, c.G:c.G + c.n2].reshape(-1, c.D)
        _report(label + " x bits", _same_bits(got, e32))
    elif epi == RES:
        # The class's old x joins after K-tile J (kernels.h resid_join_ktile).  A weight in a K-tile <= J is the whole sum when x joins
        # (a VALU add: fl(W + x), round to nearest even); a weight in a later K-tile is added to x by the MFMA, whose accumulation
        # does not always round to nearest (measured: DESIGN.md, numerics): there the sum must be the nearest fp32 value or one of its
        # two neighbours (a faithful rounding is one of them).  Either way the bias follows as a VALU add.
        n_ = torch.arange(c.N, device="cuda")
        e = (m[:, None] & 3) + 4 * ((n_[None, :] >> 7) & 1)
        J = torch.clamp(e + 1, max=c.K // 64 - 1)
        valu = (pi // 64)[:, None] <= J
        r0 = Cw + c.x0                          # round to nearest even, and its two fp32 neighbours
        up = torch.nextafter(r0, torch.full_like(r0, float("inf")))
        dn = torch.nextafter(r0, torch.full_like(r0, float("-inf")))
        got = _bits(outs["x"])
        rne = _bits((Cw + c.x0) + bias)
        ok_faithful = (got == rne) | (got == _bits(up + bias)) | (got == _bits(dn + bias))
        _report(label + " x bits, weight before the join", int((got != rne)[valu].sum()))
        _report(label + " x bits, weight after the join (nearest or a neighbour)", int((~ok_faithful)[~valu].sum()))
        print("%-72s %d of %d" % (label + " MFMA-added elements not rounded to nearest", int((got != rne)[~valu].sum()), int((~valu).sum())))
    else:
        v = (Cw + 0.0) + bias
        if act == 0:
            ref = R.gelu_erf64(v)
            bar = 7.5e-7 * torch.clamp(v.to(F64).abs() / 12, min=1.0) + _ulp(ref, op)
        else:
            ref = R.quick_gelu64(v)
            bar = 4 * U * v.to(F64).abs() + _ulp(ref, op)
        got = outs["out16"].to(F64)
        assert not bool(torch.isnan(got).any()), label + ": NaN"
        _report(label + " (max err / bar)", float(((got - ref).abs() / bar).max()), 1.0)


def test_residual_with_zero_weights_is_x_plus_b_in_every_class():
    """W = 0: every element of every join class (row mod 4 + 4 column half) is fl(x + b) bitwise on every residual path, at K = 640
    (nk = 10: the lazy join's first legal depth) and 3072; a dropped or doubled join changes x."""
    for op in (0, 1):
        for K in (640, 3072):
            c = Case(op, RES, 3 * 264, 768, K, 768, Tp=264)
            g = torch.Generator(device="cuda").manual_seed(K + op)
            A = torch.randn(c.M, K, generator=g, device="cuda").to(OPS[op])
            W = torch.zeros(768, K, dtype=OPS[op], device="cuda")
            bias = torch.randn(768, generator=g, device="cuda")
            c.x0 = torch.randn(c.M, 768, generator=g, device="cuda") * 3
            for p in c.paths():
                if not _fits(c, p):
                    continue
                _, outs = c.run(p, A, W, bias)
                _report("%s resid W=0 K=%d %s bits" % (OPN[op], K, PN[p]), _same_bits(outs["x"], c.x0 + bias))


def test_integer_operands_are_exact_on_every_path():
    """Small integers (|a| <= 3, |w| <= 2 with 95 % of W zero, integer bias) keep every partial sum an integer far below 2^8, so every
    sum is exact in fp32 and every output exact in fp16 / bf16: every summation order, every path gives the float64 value bitwise."""
    for op in (0, 1):
        dt = OPS[op]
        g = torch.Generator(device="cuda").manual_seed(11 + op)
        c = Case(op, QKV, 3 * 264, 2304, 768, 768, 12, 261, 264, 320)
        A = torch.randint(-3, 4, (c.M, 768), generator=g, device="cuda").to(dt)
        W = torch.randint(-2, 3, (c.N, 768), generator=g, device="cuda") * (torch.rand(c.N, 768, generator=g, device="cuda") < 0.05)
        W = W.to(dt)
        bias = torch.randint(-4, 5, (c.N,), generator=g, device="cuda").float()
        ref = R.gemm64(A, W) + bias.to(F64)
        assert float(ref.abs().max()) < 256
        q, k, vT = R.qkv_split64(ref, c.B, c.Tp, c.Tk, c.H)
        for p in c.paths():
            if not _fits(c, p):
                continue
            _, outs = c.run(p, A, W, bias)
            for n, r in (("q", q), ("k", k), ("vT", vT)):
                sel = ~torch.isnan(r)
                _report("%s integer qkv %s %s" % (OPN[op], PN[p], n), int((outs[n][sel].to(F64) != r[sel]).sum()))


def test_prefetch_workgroups_write_nothing():
    """pf / pf_bytes set: the extra cache-warming workgroups of the 128-wide (WIDE128, NARROW) and 256 kernels only read; outputs are
    bitwise those of the launch without them and every guard band holds."""
    pf = torch.randn(1 << 20, device="cuda")
    for op in (0, 1):
        for epi, p in ((GELU, WIDE128), (QKV, WIDE128), (RES, NARROW), (PE, NARROW), (GELU, K256)):
            if epi == PE:
                c = Case(op, PE, 256, 768, 640, 768, 12, 261, 264, 320, 5, 256)
            elif epi == QKV:
                c = Case(op, QKV, 264, 2304, 768, 768, 12, 261, 264, 320, capture=True)
            else:
                c = _gemm_case(op, epi, "crop56" if epi == RES else "S224", 1536 if epi == RES else None)
            A, W, bias = _operands(c, 3)
            _, o1 = c.run(p, A, W, bias)
            _, o2 = c.run(p, A, W, bias, pf=pf)
            _report("%s %s %s with pf vs without" % (OPN[op], EPN[epi], PN[p]), sum(_same_bits(o1[n], o2[n]) for n in o1))


def test_refused_combinations():
    """Forms that are not instantiated, or whose preconditions fail, are refused with nothing written (guards checked in Case.run)."""
    for op in (0, 1):
        refusals = [
            (Case(op, GELU, 264, 3072, 768, 768, act=0, Tp=264), NARROW),             # GELU on the narrow form: not instantiated
            (Case(op, GELU, 264, 3072, 768, 768, act=0, Tp=264), RES128),
            (Case(op, QKV, 264, 2304, 768, 768, 12, 261, 264, 320), NARROW),
            (Case(op, PE, 256, 768, 640, 768, 12, 261, 264, 320, 5, 256), WIDE128),
            (Case(op, PE, 256, 768, 640, 768, 12, 261, 264, 320, 5, 256), ROLL),
            (Case(op, RES, 264, 768, 768, 768, Tp=264), K256),                          # residual at 256 x 256: the rolling kernel's
            (Case(op, RES, 264, 768, 768, 768, Tp=264), WIDE128),
            (Case(op, QKV, 264, 2304, 768, 768, 12, 261, 264, 320, capture=True), ROLL),   # capture on ROLL
            (Case(op, QKV, 264, 1152, 384, 384, 6, 261, 264, 320), K256),               # D % 256 != 0
            (Case(op, QKV, 264, 1152, 384, 384, 6, 261, 264, 320), ROLL),
            (Case(op, RES, 264, 384, 384, 384, Tp=264), RES128),                        # lazy join at nk = 6
            (Case(op, RES, 264, 768, 512, 768, Tp=264), RES128),                        # lazy join at nk = 8
            (Case(op, RES, 264, 768, 640, 768, Tp=264), ROLL),                          # rolling residual needs nk >= 12
            (Case(op, GELU, 5 * 8, 3072, 768, 768, act=0, Tp=8), ROLL),                 # Tp < 256: small crops
            (Case(op, QKV, 5 * 24, 2304, 768, 768, 12, 21, 24, 64), ROLL),
            (Case(op, GELU, 600, 3072, 768, 768, act=1, Tp=200), ROLL),                 # CLIP B/16: Tp = 200
        ]
        for c, p in refusals:
            if c.epi == RES:
                c.x0 = torch.zeros(c.M, c.N, device="cuda")
            if c.epi == PE:
                c.pos = torch.zeros(1 + c.n2, c.D, device="cuda")
            A, W, bias = _operands(c, 4)
            c.x0 = torch.zeros(c.M, c.N, device="cuda") if c.epi == RES else c.x0
            c.run(p, A, W, bias, expect_refusal=True)
    L = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    x = torch.zeros(8, 1028, device="cuda")
    w = torch.ones(1028, device="cuda")
    o = torch.empty(8, 1028, dtype=torch.float16, device="cuda")
    assert L.pio_test_layernorm(0, x.data_ptr(), w.data_ptr(), w.data_ptr(), 1e-6, 8, 1028, o.data_ptr(), None, 8, 8, s) == ERR_INVALID
    assert L.pio_test_layernorm(0, x.data_ptr(), w.data_ptr(), w.data_ptr(), 1e-6, 8, 390, o.data_ptr(), None, 8, 8, s) == ERR_INVALID
    q = torch.zeros(1, 6, 64, 64, dtype=torch.float16, device="cuda")
    assert L.pio_test_attention(0, 0, q.data_ptr(), q.data_ptr(), q.data_ptr(), q.data_ptr(), 1, 6, 9, 16, 60, 384, 0.125, None, s) == ERR_INVALID
    assert L.pio_test_attention(0, 0, q.data_ptr(), q.data_ptr(), q.data_ptr(), q.data_ptr(), 1, 6, 9, 16, 64, 380, 0.125, None, s) == ERR_INVALID


# ------------------------------------------------------------------------------------------------ attention
ATT_CASES = [  # (T, H, B, operand)
    (6, 6, 3, 0), (9, 12, 3, 1), (21, 6, 5, 0), (197, 12, 3, 1), (261, 16, 3, 0), (261, 6, 1, 1), (1374, 6, 1, 0), (1374, 16, 1, 1),
]
LENS = (1, 16, 17, 32, 33, 63, 64, 65, 128, 129)


def _attention_operands(op, B, H, T, Tk, lens, seed, causal=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    dt = OPS[op]
    q = (torch.randn(B, H, Tk, 64, generator=g, device="cuda").abs() + 0.1)     # positive queries: a leaked key of +8 dominates
    k = torch.randn(B, H, Tk, 64, generator=g, device="cuda")
    v = torch.randn(B, H, 64, Tk, generator=g, device="cuda")
    for b in range(B):
        n = int(lens[b])
        k[b, :, n:] = 8.0                      # keys that must stay masked: large, finite
        v[b, :, :, n:] = 1000.0
    return q.to(dt), k.to(dt), v.to(dt)


@pytest.mark.parametrize("T,H,B,op", ATT_CASES, ids=["T%d-H%d-B%d-%s" % (T, H, B, OPN[op]) for T, H, B, op in ATT_CASES])
def test_vit_attention_against_float64(T, H, B, op):
    """lens[b] over {1, 16, 17, 32, 33, 63, 64, 65, 128, 129, T} (those <= T), in one KV tile and in several: every last-tile branch of
    k_vit_attention (full, > 32 keys masked, <= 32 keys in one or two 16-key steps).  Keys >= lens[b] hold large finite values: one that
    leaks dominates.  Bar (P rounded to the operand type before P V: p = 11 / 8 significant bits): |got - ref| <= 3 2^-p max_valid |v| +
    2^-p |ref|, on the query rows t < T.  Rows past B Tp and the guard bands hold their sentinel."""
    Tp, Tk, D = -(-T // 8) * 8, -(-T // 64) * 64, 64 * H
    lens_all = sorted({n for n in LENS if n <= T} | {T})
    L = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    p = 11 if op == 0 else 8
    worst = 0.0
    for i in range(0, len(lens_all), B):
        lens = (lens_all[i:i + B] + [T] * B)[:B]
        q, k, vT = _attention_operands(op, B, H, T, Tk, lens, seed=T * 31 + i)
        lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
        out = Guarded((B * Tp, D), OPS[op])
        _lib.check(L.pio_test_attention(0, op, q.data_ptr(), k.data_ptr(), vT.data_ptr(), out.t.data_ptr(), B, H, T, Tp, Tk, D, 0.125,
                                        lens_d.data_ptr(), s))
        torch.cuda.synchronize()
        out.check("attention T=%d" % T, torch.ones(B * Tp, D, dtype=torch.bool, device="cuda"))
        ref = R.attention64(q, k, vT, 0.125, T, lens)                      # [B][H][T][64]
        got = out.t.view(B, Tp, H, 64)[:, :T].permute(0, 2, 1, 3).to(F64)
        for b in range(B):
            vmax = float(vT[b, :, :, :lens[b]].to(F64).abs().max())
            bar = 3 * 2.0 ** -p * vmax + 2.0 ** -p * ref[b].abs()
            err = (got[b] - ref[b]).abs()
            assert not bool(torch.isnan(err).any())
            worst = max(worst, float((err / bar).max()))
    _report("attention %s T=%d H=%d B=%d lens %s (max err / bar)" % (OPN[op], T, H, B, lens_all), worst, 1.0)


@pytest.mark.parametrize("H,op", [(8, 0), (12, 0), (8, 1), (12, 1)])
def test_text_attention_against_float64(H, op):
    """The text tower's causal attention at its shapes (context 77: Tp 80, Tk 128, as text_api.cpp sets them), every query row
    t < Tp attending keys <= t; key slots [Tp, Tk) hold large values and must never be read into a result.  Same bar as above."""
    B, T, Tp, Tk, D = 3, 77, 80, 128, 64 * H
    g = torch.Generator(device="cuda").manual_seed(H + op)
    dt = OPS[op]
    q = torch.randn(B, H, Tk, 64, generator=g, device="cuda").to(dt)
    k = torch.randn(B, H, Tk, 64, generator=g, device="cuda")
    v = torch.randn(B, H, 64, Tk, generator=g, device="cuda")
    k[:, :, Tp:] = 8.0
    v[:, :, :, Tp:] = 1000.0
    k, vT = k.to(dt), v.to(dt)
    out = Guarded((B * Tp, D), dt)
    L = _lib.load()
    _lib.check(L.pio_test_attention(1, op, q.data_ptr(), k.data_ptr(), vT.data_ptr(), out.t.data_ptr(), B, H, T, Tp, Tk, D, 0.125, None,
                                    torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out.check("text attention", torch.ones(B * Tp, D, dtype=torch.bool, device="cuda"))
    ref = R.attention64(q, k, vT, 0.125, Tp, causal=True)
    got = out.t.view(B, Tp, H, 64).permute(0, 2, 1, 3).to(F64)
    p = 11 if op == 0 else 8
    vmax = float(vT[:, :, :, :Tp].to(F64).abs().max())
    bar = 3 * 2.0 ** -p * vmax + 2.0 ** -p * ref.abs()
    _report("text attention %s H=%d (max err / bar)" % (OPN[op], H), float(((got - ref).abs() / bar).max()), 1.0)


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("D", [384, 512, 768, 1024])
def test_layernorm_against_float64(D):
    """Rows N(0, 1) with DINOv2-like outlier channels (a few at 1e2 - 1e3), zero rows and constant rows (exact sums: y == b bitwise),
    through out16 (every row) and out32 (rows t >= T of every Tp-row image dropped; the rows past B T stay sentinel).
    Bar: the kernel sums a row in at most 22 rounding levels (16 per thread, 6 across the wave): mean error <= 23 u mean|x|; the
    variance of the centred values carries (22 + 3) u relative and the error of the mean only at second order; rsqrt adds 1 ulp, so rstd
    is within 16 u; the centring, two products and the bias add one u each.  |dy| <= 2 u (|w| rstd (23 mean|x| + 20 |x - mu|) + 2 |y|)
    (+ 1 ulp of the operand type for out16), the factor 2 for the hardware rsqrt's and the reduction tree's slack."""
    B, T, Tp = 3, 261, 264
    M = B * Tp
    g = torch.Generator(device="cuda").manual_seed(D)
    x = torch.randn(M, D, generator=g, device="cuda")
    x[:, torch.randperm(D, generator=torch.Generator().manual_seed(D))[:4].cuda()] *= torch.tensor([100.0, -300.0, 1000.0, 550.0], device="cuda")
    x[7] = 0.0
    x[11] = 3.0
    x[12] = -0.5
    w = 1 + 0.1 * torch.randn(D, generator=g, device="cuda")
    b = 0.1 * torch.randn(D, generator=g, device="cuda")
    eps = 1e-6
    L = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    x64 = x.to(F64)
    ref = R.layer_norm64(x64, w.to(F64), b.to(F64), eps)
    mu = x64.mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(((x64 - mu) ** 2).mean(-1, keepdim=True) + eps)
    bar = 2 * U * (w.to(F64).abs() * rstd * (23 * x64.abs().mean(-1, keepdim=True) + 20 * (x64 - mu).abs()) + 2 * ref.abs())
    for op in (0, 1):
        o16 = Guarded((M, D), OPS[op])
        _lib.check(L.pio_test_layernorm(op, x.data_ptr(), w.data_ptr(), b.data_ptr(), eps, M, D, o16.t.data_ptr(), None, T, Tp, s))
        torch.cuda.synchronize()
        o16.check("layernorm out16", torch.ones(M, D, dtype=torch.bool, device="cuda"))
        _report("layernorm D=%d %s out16 (max err / bar)" % (D, OPN[op]),
                float(((o16.t.to(F64) - ref).abs() / (bar + _ulp(ref, op))).max()), 1.0)
        for r in (7, 11, 12):
            _report("layernorm D=%d %s out16 row %d == b" % (D, OPN[op], r), _same_bits(o16.t[r], b.to(OPS[op])))
    o32 = Guarded((M, D), torch.float32)       # the compacted rows fill B T of the M rows
    _lib.check(L.pio_test_layernorm(0, x.data_ptr(), w.data_ptr(), b.data_ptr(), eps, M, D, None, o32.t.data_ptr(), T, Tp, s))
    torch.cuda.synchronize()
    wr = torch.zeros(M, D, dtype=torch.bool, device="cuda")
    wr[:B * T] = True
    o32.check("layernorm out32", wr)
    keep = (torch.arange(M, device="cuda") % Tp) < T
    ref32, bar32 = ref[keep], bar[keep]
    _report("layernorm D=%d out32 (max err / bar)" % D, float(((o32.t[:B * T].to(F64) - ref32).abs() / bar32).max()), 1.0)
    for r in (7, 11, 12):
        _report("layernorm D=%d out32 row %d == b" % (D, r), _same_bits(o32.t[r], b))


# ------------------------------------------------------------------------------------------------ AUTO at production sizes
@pytest.mark.parametrize("imgs", [16, 80])
def test_auto_route_at_production_sizes(imgs):
    """16 and 80 images of ViT-B at 224^2: AUTO's path_taken equals pio_test_gemm_route's, and its bits equal an explicit launch of that
    path and of the 128-wide kernel (the forward's whole GEMM family at the sizes the pipeline launches)."""
    op, Tp = 0, 264
    M = imgs * Tp
    cases = [Case(op, QKV, M, 2304, 768, 768, 12, 261, Tp, 320), Case(op, GELU, M, 3072, 768, 768, act=0, Tp=Tp),
             Case(op, RES, M, 768, 768, 768, Tp=Tp), Case(op, RES, M, 768, 3072, 768, Tp=Tp)]
    for c in cases:
        A, W, bias = _operands(c, 9)
        taken, o_auto = c.run(AUTO, A, W, bias)
        assert taken == route(c.epi, c.M, c.N, c.K, c.D, Tp)
        _, o_exp = c.run(taken, A, W, bias)
        _report("%d images %s AUTO = %s vs explicit" % (imgs, EPN[c.epi], PN[taken]), sum(_same_bits(o_auto[n], o_exp[n]) for n in o_auto))
        other = NARROW if c.epi == RES else WIDE128
        if other != taken:
            _, o_o = c.run(other, A, W, bias)
            _report("%d images %s %s vs %s" % (imgs, EPN[c.epi], PN[taken], PN[other]), sum(_same_bits(o_auto[n], o_o[n]) for n in o_auto))


def test_zz_coverage_tally():
    """Every instantiated (operand, epilogue, path) triple ran at least once in this module, every refusal was asserted."""
    for k in sorted(TALLY_RAN):
        print("ran     %s %-6s %-8s %d" % (OPN[k[0]], EPN[k[1]], PN[k[2]], TALLY_RAN[k]))
    for k in sorted(TALLY_REFUSED):
        print("refused %s %-6s %-8s %d" % (OPN[k[0]], EPN[k[1]], PN[k[2]], TALLY_REFUSED[k]))
    if TALLY_RAN:
        missing = {(op, e, p) for op in (0, 1) for (e, p) in INSTANTIATED} - set(TALLY_RAN)
        assert not missing, "never ran: %s" % sorted(missing)
