"""The decoder's kernels (csrc/decoder.hip) one launch at a time against the float64 statements and derived bars of
tests/decoder_ref64.py (the derivation is in that module's docstring; tests/test_decoder_ref64_cpu.py shows the bars reject wrong
kernels).  The launches go through the layer pass's own dispatch (pio_test_dec_gemm -> dec_layer_gemm / dec_gemm, pio_test_dec_attention
-> the attention launches of dec_layers_step / dec_prompt_prefill), at every row count where that dispatch changes kernel or tile:

  k_dec_gemm    family A at 1 / 2 / 4 / 8 row groups (4 waves x 12 chunks); by rows: <= 16 rows, the 8-wave form at 33 .. 64 rows of the
                prefix projection, K = 384 .. 1024, two launches above 128 rows
  k_dec_gemm_b  every tile of dec_gemm_b_tile: (1,2,1) (2,2,1) (2,3,1) wide, (1,1,1) (2,1,1) narrow, (1,2,4) (2,2,4) (4,2,4) split-K.
                Family B takes any row count from 1 (dec_gemm_b_tile has a tile for <= 2 row groups; only dec_gemm keeps <= 16 rows on
                k_dec_gemm), so it is tested from 1 row
  k_dec_gemm_s  <3,1> qkv / proj, <NCG_FC,1> c_fc, <NCG_FC,4> mlp.c_proj from 65 rows; the fast path and the re-staged path (rows of
                1e-6 and 1e8, a NaN row, an inf element).  The decode itself never hands dec_gemm split weights for attn.c_proj
                (dec_layers: "never for proj"): the proj cases of the split kernel test an instance dec_gemm can reach, not one a
                decode runs
  k_dec_attention in its six forms and k_kv_append_masked; k_lmhead_f16<8> / <16>, k_lm_prep, k_dec_select_filter above 64 rows.

The LayerNorm operands (W', c, d) come from the loader's own fold (pio_host_ln_fold); the float64 reference is computed from the
unfolded W, ln_w, ln_b, b.  Output rows are dense ([N][Nout], no leading dimension), so a column overrun lands in the next row (an
error against the reference) or in the guard rows around the buffer, which hold a sentinel.  Each test prints observed / bar of its
worst element."""
import ctypes
import functools

import pytest
import torch

import decoder_ref64 as D
import viecap_ref64 as R
from patchioner_amd import _lib
from patchioner_amd import weights as W
from patchioner_amd._lib import check, ptr

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FAMILY_A, FAMILY_B, BY_ROWS, BY_ROWS_SPLIT = 0, 1, 2, 3
SEL_NAMES = {FAMILY_A: "family A", FAMILY_B: "family B", BY_ROWS: "by rows", BY_ROWS_SPLIT: "by rows + split"}
ROWS = (1, 15, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 127, 128, 129, 160, 161, 255, 256)
SPLIT_FROM = 65                        # PIO_DEC_SPLIT_MIN_RG = 5 row groups of 16
SENT = 12345.678
E = D.E


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _workspace():
    lib = _lib.load()
    nf, nt = ctypes.c_int64(), ctypes.c_int32()
    check(lib.pio_test_dec_workspace(ctypes.byref(nf), ctypes.byref(nt)))
    assert nf.value > 0 and nt.value > 0
    return torch.zeros(nf.value, device="cuda"), torch.zeros(nt.value, dtype=torch.int32, device="cuda")


@functools.lru_cache(maxsize=None)
def _dev_case(name, K=None):
    """The device operands of one GEMM as the loader produces them (+ the split-fp16 image of W)."""
    lib = _lib.load()
    c = D.layer_case(name, K=K)
    Nout, K_ = c["Nout"], c["K"]
    if c["ln"]:
        w, cv, dv = torch.empty(Nout, K_), torch.empty(Nout), torch.empty(Nout)
        check(lib.pio_host_ln_fold(c["W"].data_ptr(), 0, K_, Nout, c["ln_w"].data_ptr(), c["ln_b"].data_ptr(), c["b"].data_ptr(),
                                   w.data_ptr(), cv.data_ptr(), dv.data_ptr()))
    else:
        w, cv, dv = c["W"], None, c["b"]
    d = {"c": c, "W": w.cuda(), "bias": dv.cuda(), "cvec": None if cv is None else cv.cuda(),
         "extra": c["extra"].cuda() if "extra" in c else None, "Wsplit": None, "unscale": 0.0}
    if name != "embed":
        img = torch.empty(4 * Nout * K_, dtype=torch.uint8, device="cuda")
        un = ctypes.c_float()
        check(lib.pio_test_dec_split_weights(ptr(d["W"]), Nout * K_, ptr(img), ctypes.byref(un), _stream()))
        assert un.value > 0
        d["Wsplit"], d["unscale"] = img, un.value
    return d


@functools.lru_cache(maxsize=None)
def _ref(name, family, K=None, rows=256):
    """(x, old, reference, fp32 bar, split bar) on the device for `rows` rows; a launch of N rows uses the first N (rows are independent)."""
    c = D.layer_case(name, K=K)
    x = D.x_family(family, rows, c["K"])
    old = torch.randn(rows, c["Nout"], generator=torch.Generator().manual_seed(9)) if c["epi"] == D.RESID else None
    ref, bar = D.layer_gemm64(c, x, old=old)
    return x.cuda(), None if old is None else old.cuda(), ref.cuda(), bar(D.U32).cuda(), bar(D.U_SPLIT16).cuda()


def _launch(sel, d, x, N, old=None, use_split=True, ws=None, tk=None):
    """One pio_test_dec_gemm on the first N rows of x; the output sits between two pairs of sentinel rows."""
    lib = _lib.load()
    c = d["c"]
    Nout = c["Nout"]
    if c["K"] == 3072 and ws is None:
        ws, tk = _workspace()
    buf = torch.full((N + 4, Nout), SENT, device="cuda")
    if old is not None:
        buf[2:N + 2] = old[:N]
    out = buf[2:N + 2]
    check(lib.pio_test_dec_gemm(sel, c["epi"], ptr(d["W"]), ptr(d["Wsplit"]) if use_split else None, d["unscale"], ptr(x), N, Nout, c["K"],
                                ptr(d["bias"]), ptr(d["cvec"]), ptr(d["extra"]), c["eps"], out.data_ptr(), ptr(ws), ptr(tk), _stream()))
    assert bool((buf[:2] == SENT).all()) and bool((buf[N + 2:] == SENT).all()), "guard rows written (N = %d)" % N
    return out


def _ratio(got, ref, bar):
    ok = torch.isfinite(ref)
    err = (got.double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return float((err[ok] / bar[ok]).max())


def _rows_of(sel):
    return tuple(n for n in ROWS if n <= 128) if sel in (FAMILY_A, FAMILY_B) else ROWS


# ------------------------------------------------------------------------------------------------ 3.1 layer GEMMs
@pytest.mark.parametrize("name", ["qkv", "proj", "fc", "fc2"])
@pytest.mark.parametrize("sel", [FAMILY_A, FAMILY_B, BY_ROWS, BY_ROWS_SPLIT])
def test_layer_gemm_vs_float64(sel, name):
    """Every element within its bar at every row count of the dispatch; RESID adds onto a non-zero old out; guard rows untouched.  The
    split kernel (by rows + split, from 65 rows) is held to u = 2^-22 in the dot-product term, everything else to 2^-24."""
    d = _dev_case(name)
    for family in D.FAMILIES:
        x, old, ref, bar32, bar_s = _ref(name, family)
        worst, worst_s = (0.0, 0), (0.0, 0, 0.0)
        for N in _rows_of(sel):
            out = _launch(sel, d, x, N, old)
            split = sel == BY_ROWS_SPLIT and N >= SPLIT_FROM
            r = _ratio(out, ref[:N], (bar_s if split else bar32)[:N])
            if split:
                worst_s = max(worst_s, (r, N, _ratio(out, ref[:N], bar32[:N])))      # the last figure is printed, not asserted
            else:
                worst = max(worst, (r, N))
            assert r <= 1.0, "%s %s %s N=%d: observed / bar = %.3f" % (SEL_NAMES[sel], name, family, N, r)
        print("dec gemm %-16s %-4s %-8s observed / bar %.4f (N = %d)" % (SEL_NAMES[sel], name, family, worst[0], worst[1]))
        if sel == BY_ROWS_SPLIT:
            print("dec gemm %-16s %-4s %-8s observed / bar %.4f (N = %d; %.4f of the fp32 kernels' bar)" % (
                "k_dec_gemm_s", name, family, worst_s[0], worst_s[1], worst_s[2]))


@pytest.mark.parametrize("K", [384, 512, 640, 768, 1024])
def test_prefix_projection_vs_float64(K):
    """DE_EMBED (k_dec_gemm at every prefix width; one launch up to 128 rows, two above), extra = the wpe row."""
    d = _dev_case("embed", K)
    for family in D.FAMILIES:
        x, _, ref, bar32, _ = _ref("embed", family, K)
        worst = (0.0, 0)
        for N in (1, 16, 17, 64, 65, 128, 129, 256):
            out = _launch(BY_ROWS, d, x, N)
            r = _ratio(out, ref[:N], bar32[:N])
            worst = max(worst, (r, N))
            assert r <= 1.0, "embed K=%d %s N=%d: observed / bar = %.3f" % (K, family, N, r)
        print("dec gemm embed K=%-4d %-8s observed / bar %.4f (N = %d)" % (K, family, worst[0], worst[1]))


@pytest.mark.parametrize("name", ["qkv", "proj", "fc", "fc2"])
def test_split_kernel_starts_at_65_rows(name):
    """With split weights present the by-rows selector runs the fp32 kernels up to 64 rows (bit for bit what it runs without them) and
    k_dec_gemm_s from 65 (another summation: not the same bits)."""
    d = _dev_case(name)
    x, old, _, _, _ = _ref(name, "unit")
    for N in (1, 16, 64):
        assert torch.equal(_launch(BY_ROWS_SPLIT, d, x, N, old), _launch(BY_ROWS, d, x, N, old)), N
        assert torch.equal(_launch(BY_ROWS_SPLIT, d, x, N, old), _launch(BY_ROWS_SPLIT, d, x, N, old, use_split=False)), N
    for N in (65, 128, 256):
        assert not torch.equal(_launch(BY_ROWS_SPLIT, d, x, N, old), _launch(BY_ROWS_SPLIT, d, x, N, old, use_split=False)), N


@pytest.mark.parametrize("name", ["qkv", "proj", "fc", "fc2"])
def test_split_kernel_range_edges(name):
    """Rows of 1e-6 and 1e8 among ordinary ones (the workgroup stages its slice again, every row with its own power of two), a NaN row
    and an inf element inside one 32-row block.  The NaN row is NaN on every kernel.  The row with the inf element has no finite
    element on any kernel; in the LayerNorm forms the split kernel makes it NaN throughout, as the float64 statement does, while the
    fp32 kernels leave a mix of inf and NaN there (fmaxf(var, 0) turns the NaN variance inf - inf into 0, so r stays finite and the
    row is r (inf - inf c) + d element by element) -- the next LayerNorm of the layer pass turns either into NaN.  Every other row of
    the block and of the launch stays within its bar."""
    d = _dev_case(name)
    c = d["c"]
    N = 96
    x = D.x_family("split_edges", N, c["K"])
    x[37] = float("nan")
    x[38 + 16, 5] = float("inf")                        # rows 37 and 54: the block of rows 32 .. 63
    old = torch.randn(N, c["Nout"], generator=torch.Generator().manual_seed(9)) if c["epi"] == D.RESID else None
    ref, bar = D.layer_gemm64(c, x, old=old)
    ref, b = ref.cuda(), bar(D.U_SPLIT16).cuda()
    oldd = None if old is None else old.cuda()
    out = _launch(BY_ROWS_SPLIT, d, x.cuda(), N, oldd)
    f32 = _launch(BY_ROWS, d, x.cuda(), N, oldd)
    bad = torch.zeros(N, dtype=torch.bool, device="cuda")
    bad[37] = bad[54] = True
    assert bool(torch.isnan(out[37]).all()) and bool(torch.isnan(f32[37]).all())
    assert not bool(torch.isfinite(out[54]).any()) and not bool(torch.isfinite(f32[54]).any())
    if c["ln"]:
        assert bool(torch.isnan(out[54]).all())
    assert bool(torch.isfinite(out[~bad]).all())
    r = _ratio(out[~bad], ref[~bad], b[~bad])
    print("dec gemm split, range edges %-4s observed / bar %.4f" % (name, r))
    assert r <= 1.0
    assert _ratio(f32[~bad], ref[~bad], bar(D.U32).cuda()[~bad]) <= 1.0


def test_gemm_hook_refuses_what_the_kernels_do_not_take():
    lib = _lib.load()
    d = _dev_case("qkv")
    c = d["c"]
    x = torch.zeros(4, 768, device="cuda")
    out = torch.full((4, 2304), SENT, device="cuda")

    def call(sel=BY_ROWS, epi=c["epi"], N=4, Nout=2304, K=768, cvec=d["cvec"], xp=x, ws=None, tk=None, eps=1e-5):
        return lib.pio_test_dec_gemm(sel, epi, ptr(d["W"]), None, 0.0, ptr(xp), N, Nout, K, ptr(d["bias"]), ptr(cvec), None, eps, ptr(out),
                                     ptr(ws), ptr(tk), _stream())

    for kw in (dict(sel=4), dict(sel=-1), dict(epi=4), dict(N=0), dict(N=257), dict(Nout=768), dict(K=512), dict(cvec=None), dict(xp=None),
               dict(eps=0.0), dict(epi=D.RESID, Nout=768, K=3072), dict(epi=D.EMBED, Nout=768, K=768), dict(epi=D.EMBED, Nout=768, K=256)):
        assert call(**kw) == -1, kw
        assert b"pio_test_dec_gemm" in lib.pio_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    assert lib.pio_test_dec_workspace(None, None) == -1
    assert lib.pio_test_dec_split_weights(ptr(d["W"]), 12, ptr(out), ctypes.byref(ctypes.c_float()), _stream()) == -1


# ------------------------------------------------------------------------------------------------ 3.2 split-K
@pytest.mark.parametrize("sel", [FAMILY_A, FAMILY_B, BY_ROWS, BY_ROWS_SPLIT])
def test_split_k_writes_every_slab_and_rearms_its_tickets(sel):
    """mlp.c_proj: the workspace is NaN before the launch (a slab read before it was written would show), the tickets are zero
    afterwards, and a second launch on the same inputs gives the same bits.  (Families A and B above 128 rows: two chunks, 128 + the rest.)"""
    d = _dev_case("fc2")
    nf, nt = _workspace()[0].numel(), _workspace()[1].numel()
    x, old, ref, bar32, bar_s = _ref("fc2", "massive")
    for N in (1, 17, 65, 129, 256):
        ws = torch.full((nf,), float("nan"), device="cuda")
        tk = torch.zeros(nt, dtype=torch.int32, device="cuda")
        a = _launch(sel, d, x, N, old, ws=ws, tk=tk)
        assert bool((tk == 0).all()), "tickets not re-armed (N = %d)" % N
        b = _launch(sel, d, x, N, old, ws=ws, tk=tk)
        assert bool((tk == 0).all())
        assert torch.equal(a, b), "not deterministic (N = %d)" % N
        bar = bar_s if (sel == BY_ROWS_SPLIT and N >= SPLIT_FROM) else bar32
        r = _ratio(a, ref[:N], bar[:N])
        assert r <= 1.0, (N, r)


# ------------------------------------------------------------------------------------------------ 3.3 family bit contract
@pytest.mark.parametrize("name", ["qkv", "proj", "fc", "fc2"])
@pytest.mark.parametrize("sel", [FAMILY_A, FAMILY_B])
def test_a_rows_bits_do_not_depend_on_the_launch(sel, name):
    """Inside one family a row's result does not depend on the other rows of the launch (the comment above dec_gemm_cls; what
    launch_decode_prompted_ragged and launch_lm_beam_search rest on): every row of a launch of N rows -- family A at 1, 2, 4, 8 row
    groups, family B through every tile of its table -- equals the row launched alone, wherever it sits (first rows, and the launch
    reversed: the row that was last is first).  Massive-channel rows are the neighbours."""
    d = _dev_case(name)
    x, old, _, _, _ = _ref(name, "massive")
    alone = torch.cat([_launch(sel, d, x[r:r + 1].contiguous(), 1, None if old is None else old[r:r + 1]) for r in range(128)])
    for N in (2, 15, 16, 17, 32, 33, 48, 49, 64, 65, 80, 127, 128):
        out = _launch(sel, d, x, N, old)
        assert torch.equal(out, alone[:N]), "%s %s: a row of a %d-row launch differs from the row alone" % (SEL_NAMES[sel], name, N)
        xr = x[:N].flip(0).contiguous()
        out = _launch(sel, d, xr, N, None if old is None else old[:N].flip(0).contiguous())
        assert torch.equal(out, alone[:N].flip(0)), "%s %s: reversed launch of %d rows" % (SEL_NAMES[sel], name, N)


@pytest.mark.parametrize("name", ["qkv", "proj", "fc", "fc2"])
def test_a_rows_bits_do_not_depend_on_the_launch_split_kernel(name):
    """The same for k_dec_gemm_s over its whole range, 65 .. 256 rows: a row has the bits it has in the 256-row launch, in any 32-row
    block and beside any neighbours."""
    d = _dev_case(name)
    x, old, _, _, _ = _ref(name, "massive")
    base = _launch(BY_ROWS_SPLIT, d, x, 256, old)
    for N in (65, 96, 97, 129, 200, 255):
        assert torch.equal(_launch(BY_ROWS_SPLIT, d, x, N, old), base[:N]), N
        xr = x[:N].flip(0).contiguous()
        out = _launch(BY_ROWS_SPLIT, d, xr, N, None if old is None else old[:N].flip(0).contiguous())
        assert torch.equal(out, base[:N].flip(0)), "reversed launch of %d rows" % N


# ------------------------------------------------------------------------------------------------ 3.4 attention
STEP, PREFILL, RAGGED, RAGGED_TAB, MASK1, MASK2 = range(6)
POSITIONS = (0, 1, 4, 5, 31, 32, 34, 35, 36, 63, 64, 127, 128, 191, 192, 254, 255)


def _attn(form, qkv, kc, vc, N, heads, max_steps, pos=0, P=0, plen=None, split=0, tab=None, tstride=0):
    """One pio_test_dec_attention; att [rows][E] between two pairs of sentinel rows.  kc / vc are updated in place."""
    lib = _lib.load()
    rows = qkv.shape[0]
    buf = torch.full((rows + 4, E), SENT, device="cuda")
    att = buf[2:rows + 2]
    check(lib.pio_test_dec_attention(form, ptr(qkv), ptr(kc), ptr(vc), att.data_ptr(), N, heads, max_steps, pos, P, ptr(plen), split,
                                     ptr(tab), tstride, _stream()))
    assert bool((buf[:2] == SENT).all()) and bool((buf[rows + 2:] == SENT).all()), "guard rows of att written"
    return att


def _check_step(att, qkv, kc0, vc0, kc, vc, pos_of_row, heads, label):
    """att against float64 per row; the new key / value at slot pos bit for bit; every other slot as it was."""
    worst = 0.0
    qh, k0, v0 = qkv.cpu(), kc0.cpu(), vc0.cpu()
    for n, pos in enumerate(pos_of_row):
        q, kn, vn = qh[n, :E], qh[n, E:2 * E], qh[n, 2 * E:]
        ref, bar = D.attention64(q, torch.cat([k0[n, :pos], kn[None]]), torch.cat([v0[n, :pos], vn[None]]), heads)
        got = att[n].cpu()
        assert bool(torch.isfinite(got).all()), (label, n, pos)
        worst = max(worst, D.worst_ratio(got, ref, bar))
        want_k, want_v = kc0[n].clone(), vc0[n].clone()
        want_k[pos], want_v[pos] = qkv[n, E:2 * E], qkv[n, 2 * E:]
        assert torch.equal(kc[n], want_k) and torch.equal(vc[n], want_v), "%s: cache of row %d at pos %d" % (label, n, pos)
    assert worst <= 1.0, "%s: observed / bar = %.3f" % (label, worst)
    return worst


@pytest.mark.parametrize("heads", [3, 4, 6, 8, 12, 24])
def test_attention_step_vs_float64(heads):
    """hd = 256, 192, 128, 96, 64, 32 at the edges of the 32-key score pass, of the NJ x 7 preloaded values (NJ = 4 at hd 256, else 5)
    and of the four 64-score soft-max lanes; three rows with a cache each.  Slot pos of the cache holds other data before the launch:
    the new key / value must come from qkv."""
    N, ms = 3, 256
    qkv, kc0, vc0 = (t.cuda() for t in D.attn_case(heads, N, heads, ms))
    worst = 0.0
    for pos in POSITIONS:
        kc, vc = kc0.clone(), vc0.clone()
        att = _attn(STEP, qkv, kc, vc, N, heads, ms, pos=pos)
        worst = max(worst, _check_step(att, qkv, kc0, vc0, kc, vc, [pos] * N, heads, "heads %d pos %d" % (heads, pos)))
    print("dec attention step heads %-2d (hd %3d) observed / bar %.4f" % (heads, E // heads, worst))


def test_attention_with_large_score_spread():
    """|q . k| / sqrt(hd) about 80: exp underflows for most keys; the output is finite and within its bar."""
    N, ms, heads, pos = 3, 256, 12, 200
    qkv, kc0, vc0 = (t.cuda() for t in D.attn_case(2, N, heads, ms, spread=80.0))
    kc, vc = kc0.clone(), vc0.clone()
    att = _attn(STEP, qkv, kc, vc, N, heads, ms, pos=pos)
    worst = _check_step(att, qkv, kc0, vc0, kc, vc, [pos] * N, heads, "large spread")
    print("dec attention step, score spread 80           observed / bar %.4f" % worst)


@pytest.mark.parametrize("heads", [4, 12])
@pytest.mark.parametrize("P", [1, 2, 16, 17, 33, 128])
def test_attention_prefill_equals_the_step_bit_for_bit(heads, P):
    """k_kv_append_masked<0> + the grid.y = P launch: the cache holds every position's key / value (and nothing else changed), and row
    (n, p) equals the uniform step at pos = p on that cache ("same loads, same order")."""
    N, ms = 3, 256
    qkv, kc0, vc0 = (t.cuda() for t in D.attn_case(100 + P, N, heads, ms, rows=N * P))
    kc, vc = kc0.clone(), vc0.clone()
    att = _attn(PREFILL, qkv, kc, vc, N, heads, ms, P=P)
    q3 = qkv.view(N, P, 3 * E)
    assert torch.equal(kc[:, :P], q3[:, :, E:2 * E]) and torch.equal(vc[:, :P], q3[:, :, 2 * E:])
    assert torch.equal(kc[:, P:], kc0[:, P:]) and torch.equal(vc[:, P:], vc0[:, P:])
    att = att.view(N, P, E)
    for p in range(P):
        k2, v2 = kc.clone(), vc.clone()
        step = _attn(STEP, q3[:, p].contiguous(), k2, v2, N, heads, ms, pos=p)
        assert torch.equal(step, att[:, p]), "position %d of %d" % (p, P)
        assert torch.equal(k2, kc) and torch.equal(v2, vc)
    # and against float64 at the last position
    _check_step(att[:, P - 1], q3[:, P - 1], kc, vc, kc, vc, [P - 1] * N, heads, "prefill P %d" % P)


@pytest.mark.parametrize("heads", [4, 12])
def test_attention_ragged_and_tab_forms_equal_the_step_bit_for_bit(heads):
    """Ragged: row n runs position plen[n] + pos0 and equals the uniform step there.  tab: the history of row n is read through a table
    of cache rows (entries outside [0, N) clamped, dec_tab_row) and equals the uniform step on the gathered cache; the new key /
    value still go to row n's own slot."""
    N, ms, pos0 = 5, 256, 3
    qkv, kc0, vc0 = (t.cuda() for t in D.attn_case(7, N, heads, ms))
    plen_h = [1, 7, 29, 100, 252]
    plen = torch.tensor(plen_h, dtype=torch.int32, device="cuda")
    kc, vc = kc0.clone(), vc0.clone()
    att = _attn(RAGGED, qkv, kc, vc, N, heads, ms, pos=pos0, plen=plen)
    g = torch.Generator().manual_seed(11)
    tab_h = torch.randint(-3, N + 3, (N, ms), generator=g, dtype=torch.int32)
    # Row n writes its new key / value into slot pos_n of its own cache row during the launch: no history entry may name that slot of
    # that row (the beam search never does: a table names rows of the same image, which share a position), or the launch would race.
    for n in range(N):
        col = tab_h[:, plen_h[n] + pos0]
        col[col.clamp(0, N - 1) == n] = (n + 1) % N
    for n in range(N):
        assert not bool((tab_h[:, plen_h[n] + pos0].clamp(0, N - 1) == n).any())
    assert int(tab_h.min()) < 0 and int(tab_h.max()) >= N
    tab = tab_h.cuda()
    kt, vt = kc0.clone(), vc0.clone()
    att_t = _attn(RAGGED_TAB, qkv, kt, vt, N, heads, ms, pos=pos0, plen=plen, tab=tab, tstride=ms)
    rows = tab_h.clamp(0, N - 1).long().cuda()
    j = torch.arange(ms, device="cuda")
    kg, vg = kc0[rows, j[None]], vc0[rows, j[None]]                     # gathered[n][j] = cache[tab[n][j]][j]
    for n in range(N):
        pos = plen_h[n] + pos0
        k2, v2 = kc0.clone(), vc0.clone()
        step = _attn(STEP, qkv, k2, v2, N, heads, ms, pos=pos)
        assert torch.equal(step[n], att[n]), "ragged row %d" % n
        assert torch.equal(k2[n], kc[n]) and torch.equal(v2[n], vc[n])
        k3, v3 = kg.clone(), vg.clone()
        step = _attn(STEP, qkv, k3, v3, N, heads, ms, pos=pos)
        assert torch.equal(step[n], att_t[n]), "tab row %d" % n
        want_k, want_v = kc0[n].clone(), vc0[n].clone()
        want_k[pos], want_v[pos] = qkv[n, E:2 * E], qkv[n, 2 * E:]
        assert torch.equal(kt[n], want_k) and torch.equal(vt[n], want_v), "tab form: cache of row %d" % n
    _check_step(att, qkv, kc0, vc0, kc, vc, [p + pos0 for p in plen_h], heads, "ragged")


@pytest.mark.parametrize("heads", [4, 12])
def test_attention_masked_prefill_passes_share_the_cache(heads):
    """Pass 1 appends only for prefixes with plen <= split, pass 2 only for the others; together they write what the unmasked prefill
    writes, and a pass's own prefixes get the unmasked prefill's attention rows bit for bit."""
    N, ms, P, split = 4, 64, 24, 16
    qkv, kc0, vc0 = (t.cuda() for t in D.attn_case(13, N, heads, ms, rows=N * P))
    plen_h = [3, 20, 16, 17]
    plen = torch.tensor(plen_h, dtype=torch.int32, device="cuda")
    own1 = torch.tensor([p <= split for p in plen_h], device="cuda")
    ku, vu = kc0.clone(), vc0.clone()
    att_u = _attn(PREFILL, qkv, ku, vu, N, heads, ms, P=P).view(N, P, E)
    k1, v1 = kc0.clone(), vc0.clone()
    att_1 = _attn(MASK1, qkv, k1, v1, N, heads, ms, P=P, plen=plen, split=split).view(N, P, E)
    assert torch.equal(k1[own1], ku[own1]) and torch.equal(v1[own1], vu[own1])
    assert torch.equal(k1[~own1], kc0[~own1]) and torch.equal(v1[~own1], vc0[~own1]), "pass 1 touched the other pass's prefixes"
    assert torch.equal(att_1[own1], att_u[own1])
    k2, v2 = kc0.clone(), vc0.clone()
    att_2 = _attn(MASK2, qkv, k2, v2, N, heads, ms, P=P, plen=plen, split=split).view(N, P, E)
    assert torch.equal(k2[~own1], ku[~own1]) and torch.equal(v2[~own1], vu[~own1])
    assert torch.equal(k2[own1], kc0[own1]) and torch.equal(v2[own1], vc0[own1]), "pass 2 touched the other pass's prefixes"
    assert torch.equal(att_2[~own1], att_u[~own1])
    _attn(MASK2, qkv, k1, v1, N, heads, ms, P=P, plen=plen, split=split)          # pass 2 after pass 1, on the same cache
    assert torch.equal(k1, ku) and torch.equal(v1, vu)


def test_attention_hook_refuses_what_the_kernel_does_not_take():
    lib = _lib.load()
    qkv, kc, vc = (t.cuda() for t in D.attn_case(1, 2, 12, 32))
    att = torch.full((2, E), SENT, device="cuda")
    plen = torch.tensor([5, 30], dtype=torch.int32, device="cuda")

    def call(form=STEP, N=2, heads=12, ms=32, pos=0, P=0, pl=None, tab=None, ts=0, q=qkv):
        return lib.pio_test_dec_attention(form, ptr(q), ptr(kc), ptr(vc), ptr(att), N, heads, ms, pos, P, ptr(pl), 0, ptr(tab), ts, _stream())

    for kw in (dict(form=6), dict(heads=5), dict(heads=2), dict(heads=48), dict(ms=257), dict(pos=32), dict(pos=-1), dict(N=0), dict(q=None),
               dict(form=PREFILL, P=0), dict(form=PREFILL, P=33), dict(form=RAGGED), dict(form=RAGGED, pl=plen, pos=2),
               dict(form=RAGGED_TAB, pl=plen, pos=1), dict(form=MASK1, P=4)):
        assert call(**kw) == -1, kw
        assert b"pio_test_dec_attention" in lib.pio_last_error()
    torch.cuda.synchronize()
    assert bool((att == SENT).all())


# ------------------------------------------------------------------------------------------------ 3.5 LM head above 64 rows
def _adversarial_decap(seed=21):
    """The vocabulary of test_lm_head_fp16_filter_equals_the_exact_head_on_adversarial_vocabularies: every odd row of wte is its even
    neighbour times 1, 1 + 1e-4 or 1 - 1e-4."""
    sd = W.synth_decap(seed)
    wte = sd["decoder.transformer.wte.weight"]
    g = torch.Generator().manual_seed(5)
    d = torch.tensor([0.0, 1e-4, -1e-4])[torch.randint(0, 3, (24704,), generator=g)]
    wte[1:49408:2] = wte[0:49408:2] * (1.0 + d[:, None])
    return sd, g


def test_fp16_filter_above_64_rows_equals_the_exact_head():
    """k_lm_prep + k_lmhead_f16<8> (65 .. 128 rows) / <16> (129 .. 256) + k_dec_select_filter against the exact head (the log-probability
    path, chunks of at most 64 rows), rows of scale 1, 1e3 and 1e-3 side by side inside every 16-row group."""
    from patchioner_amd.engine import Engine
    sd, g = _adversarial_decap()
    e = Engine(embed_dim=768, depth=1, num_heads=12, num_registers=4, crop_dim=224, max_batch=2, max_prefixes=256, vit_dtype="fp16")
    try:
        e.load_state_dict(sd)
        e.finalize()
        x = torch.randn(256, 768, generator=g)
        x *= torch.tensor([1.0, 1e3, 1e-3])[torch.arange(256) % 3][:, None]
        twins = 0
        for N in (65, 97, 128, 129, 200, 256):
            xs = x[:N].contiguous()
            ids_f, _ = e.decode_greedy(xs, steps=2)
            ids_e, _ = e.decode_greedy(xs, steps=2, want_logprob=True)
            assert torch.equal(ids_f.cpu(), ids_e.cpu()), N
            twins += int((ids_e.cpu() % 2 == 0).sum())
        assert twins > 0
    finally:
        e.close()


@pytest.mark.parametrize("V_", [49408, 50257])
def test_exact_head_log_probability_vs_float64(V_):
    """Step 0 of the exact head: the log-probability of the chosen id against the float64 log-softmax of the float64 model on the same
    prefix; 50257 = 16 * 3141 + 1 leaves one column to the last column group.  The bar is test_lm_score_vs_float64's (_nll_bar)."""
    from patchioner_amd.engine import Engine
    from test_gpu_viecap_kernels import _nll_bar
    layers = 1
    sd = W.synth_decap(31, n_layer=layers, vocab=V_, tok_vocab=V_)
    e = Engine(embed_dim=768, depth=1, num_heads=12, num_registers=4, crop_dim=224, max_batch=2, max_prefixes=64, vit_dtype="fp16",
               dec_layers=layers, dec_vocab=V_)
    try:
        e.load_state_dict(sd)
        e.finalize()
        g = torch.Generator().manual_seed(V_)
        x = torch.randn(33, 768, generator=g)
        ids, lp = e.decode_greedy(x, steps=1, want_logprob=True)
        ids, lp = ids.cpu().long()[:, 0], lp.cpu().double()[:, 0]
        m = R.GPT2_64({"gpt." + k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}, heads=4)
        x0 = x.double() @ sd["clip_project.model.0.weight"].double().T + sd["clip_project.model.0.bias"].double() + m.wpe[0]
        h, _ = m.forward(x0[:, None])
        lg = m.logits(h[:, 0])
        logp = torch.log_softmax(lg, dim=-1)
        amax = lg.abs().max(dim=1).values
        # the chosen id is the float64 arg-max, or a column whose float64 logit is within the logit bar of it
        bar = torch.from_numpy(_nll_bar(layers, amax.numpy()))
        top = lg.max(dim=1).values
        assert bool((top - lg.gather(1, ids[:, None])[:, 0] <= bar).all())
        err = (lp - logp.gather(1, ids[:, None])[:, 0]).abs()
        worst = int((err / bar).argmax())
        print("exact head V=%d step-0 log-probability  observed %.3e   bar %.3e" % (V_, float(err[worst]), float(bar[worst])))
        assert bool((err <= bar).all())
    finally:
        e.close()
