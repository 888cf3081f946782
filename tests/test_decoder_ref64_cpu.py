"""The decoder references and bars of tests/decoder_ref64.py have teeth: emulations of RIGHT kernels (the folded fp32 form with one-pass
statistics; the split-fp16 form) stay inside the bars on the inputs the GPU tests use, emulations of WRONG kernels leave them by a
factor of at least 4.  The references agree with the project's other float64 GPT-2 (viecap_ref64.GPT2_64) on one layer, and the fold
restated in decoder_ref64.fold64 is the loader's (pio_host_ln_fold: the function upload_ln_folded calls)."""
import math

import pytest
import torch

import decoder_ref64 as D
import viecap_ref64 as R
from patchioner_amd import weights as W

torch.set_grad_enabled(False)
FACTOR = 4.0
N = 24


def _fp32_folded(c, x, mu_shift=0, use_c=True):
    """r (x W'^T - mu c) + d in fp32 with E[x^2] - mu^2, clamped at 0, as the kernels' epilogue."""
    wf, cv, dv = D.fold64(c)
    K = x.shape[1]
    s = x @ wf.T
    mu = x.sum(-1, keepdim=True) / K
    var = ((x * x).sum(-1, keepdim=True) / K - mu * mu).clamp_min(0.0)
    mu_used = torch.roll(mu, mu_shift, 0)
    y = torch.rsqrt(var + c["eps"]) * (s - (mu_used * cv if use_c else 0.0)) + dv
    return D.gelu_new64(y.double()).float() if c["epi"] == D.GELU else y


def _toward_zero_f16(x):
    h = x.to(torch.float16)
    over = h.float().abs() > x.abs()
    bits = h.view(torch.int16)
    return torch.where(over, (bits - 1).view(torch.float16), h)         # one step toward zero: the magnitude bits minus one


def _split_products(x, w, lo=True):
    """hi hi + (hi lo' + lo' hi) 2^-11, the three products of k_dec_gemm_s, accumulated exactly (float64)."""
    S = 2.0 ** (13 - math.floor(math.log2(float(w.abs().max()))))
    ws = w * S
    wh = ws.to(torch.float16)
    wl = ((ws - wh.float()) * 2048.0).to(torch.float16)
    xh = _toward_zero_f16(x)
    xl = ((x - xh.float()) * 2048.0).to(torch.float16)
    acc = xh.double() @ wh.double().T
    if lo:
        acc = acc + (xh.double() @ wl.double().T + xl.double() @ wh.double().T) / 2048.0
    return acc / S


@pytest.mark.parametrize("family", D.FAMILIES)
@pytest.mark.parametrize("name", ["qkv", "fc"])
def test_folded_fp32_form_passes_and_wrong_statistics_fail(name, family):
    c = D.layer_case(name)
    x = D.x_family(family, N, c["K"])
    ref, bar = D.layer_gemm64(c, x)
    good = D.worst_ratio(_fp32_folded(c, x), ref, bar())
    print("%s %-8s folded fp32 / bar %.3f" % (name, family, good))
    assert good <= 1.0
    assert D.worst_ratio(_fp32_folded(c, x, mu_shift=1), ref, bar()) >= FACTOR, "mu of the neighbouring row"
    assert D.worst_ratio(_fp32_folded(c, x, use_c=False), ref, bar()) >= FACTOR, "cvec omitted"


@pytest.mark.parametrize("family", D.FAMILIES + ("split_edges",))
@pytest.mark.parametrize("name", ["qkv", "proj", "fc2"])
def test_split_fp16_form_passes_and_its_wrong_variants_fail(name, family):
    c = D.layer_case(name)
    x = D.x_family(family, N, c["K"])
    if family == "split_edges":
        # the kernel re-stages such rows with a power of two of their own: the emulation scales them into fp16's range the same way
        e = torch.floor(torch.log2(x.abs().max(-1, keepdim=True).values)) - 13
        xs, back = x * 2.0 ** -e, 2.0 ** e.double()
    else:
        xs, back = x, 1.0
    old = torch.randn(N, c["Nout"], generator=torch.Generator().manual_seed(9))
    ref, bar = D.layer_gemm64(c, x, old=old)
    b = bar(D.U_SPLIT16)
    if c["ln"]:
        wf, cv, dv = D.fold64(c)
        mu = x.double().mean(-1, keepdim=True)
        r = 1.0 / torch.sqrt((x.double() ** 2).mean(-1, keepdim=True) - mu * mu + c["eps"])
        fin = lambda acc: r * (acc * back - mu * cv.double()) + dv.double()          # noqa: E731
        w = wf
    else:
        fin = lambda acc: old.double() + acc * back + c["b"].double()                # noqa: E731
        w = c["W"]
    good = D.worst_ratio(fin(_split_products(xs, w)), ref, b)
    print("%s %-11s split fp16 / bar %.3f" % (name, family, good))
    assert good <= 1.0
    # one 16-k MFMA step of one wave (16 columns) dropped
    acc = _split_products(xs, w)
    acc[:, 32:48] -= xs[:, 64:80].double() @ w[32:48, 64:80].double().T
    assert D.worst_ratio(fin(acc), ref, b) >= FACTOR, "a 16-k step dropped"
    if family == "massive" and name == "proj":
        # plain fp16 operands (no lo halves): hi is cut toward zero, so the rows with a common offset against the one-signed weight rows
        # 5..7 lose a fixed fraction of the sum -- what the bar's sqrt(K) u S does not allow
        assert D.worst_ratio(fin(_split_products(xs, w, lo=False))[:, 5:8], ref[:, 5:8], b[:, 5:8]) >= FACTOR, "lo halves dropped"


@pytest.mark.parametrize("family", D.FAMILIES)
def test_split_k_slab_sums_with_a_slab_missing_or_twice_fail(family):
    c = D.layer_case("fc2")
    x = D.x_family(family, N, c["K"])
    old = torch.randn(N, c["Nout"], generator=torch.Generator().manual_seed(9))
    ref, bar = D.layer_gemm64(c, x, old=old)
    slabs = [x[:, 768 * y:768 * (y + 1)] @ c["W"][:, 768 * y:768 * (y + 1)].T for y in range(4)]
    fin = lambda s: old + (s + c["b"])                                                # noqa: E731
    assert D.worst_ratio(fin(((slabs[0] + slabs[1]) + slabs[2]) + slabs[3]), ref, bar()) <= 1.0
    assert D.worst_ratio(fin((slabs[0] + slabs[1]) + slabs[3]), ref, bar()) >= FACTOR, "slab 2 missing"
    assert D.worst_ratio(fin(((slabs[0] + slabs[1]) + slabs[1]) + slabs[3]), ref, bar()) >= FACTOR, "slab 1 twice, slab 2 missing"
    assert D.worst_ratio(fin((((slabs[0] + slabs[1]) + slabs[2]) + slabs[3]) + slabs[3]), ref, bar()) >= FACTOR, "slab 3 twice"


@pytest.mark.parametrize("K", [384, 512, 640, 768, 1024])
def test_prefix_projection_fp32_passes(K):
    c = D.layer_case("embed", K=K)
    for family in D.FAMILIES:
        x = D.x_family(family, N, K)
        ref, bar = D.layer_gemm64(c, x)
        assert D.worst_ratio((x @ c["W"].T + c["b"]) + c["extra"], ref, bar()) <= 1.0
        assert D.worst_ratio(x @ c["W"].T + c["b"], ref, bar()) >= FACTOR, "the position row omitted"


@pytest.mark.parametrize("heads", [3, 4, 6, 8, 12, 24])
@pytest.mark.parametrize("pos", [0, 1, 5, 35, 128, 255])
def test_attention_bar_has_teeth(heads, pos):
    qkv, kc, vc = D.attn_case(1, 1, heads, 256)
    q, kn, vn = qkv[0, :D.E], qkv[0, D.E:2 * D.E], qkv[0, 2 * D.E:]
    k = torch.cat([kc[0, :pos], kn[None]])
    v = torch.cat([vc[0, :pos], vn[None]])
    ref, bar = D.attention64(q, k, v, heads)
    hd = D.E // heads

    def fp32_attn(k_, v_):
        s = torch.einsum("hc,jhc->hj", q.view(heads, hd), k_.view(-1, heads, hd)) / math.sqrt(hd)
        return torch.einsum("hj,jhc->hc", torch.softmax(s, -1), v_.view(-1, heads, hd)).reshape(-1)

    assert D.worst_ratio(fp32_attn(k, v), ref, bar) <= 1.0
    if pos > 0:
        assert D.worst_ratio(fp32_attn(k[:-1], v[:-1]), ref, bar) >= FACTOR, "newest key left out"
    stale_k = torch.cat([kc[0, :pos], kc[0, pos][None]])           # slot pos of the cache holds other data
    stale_v = torch.cat([vc[0, :pos], vc[0, pos][None]])
    assert D.worst_ratio(fp32_attn(stale_k, stale_v), ref, bar) >= FACTOR, "key pos read from the cache"


def test_attention_with_large_score_spread_stays_finite_and_inside_the_bar():
    qkv, kc, vc = D.attn_case(2, 1, 12, 256, spread=80.0)
    q, kn, vn = qkv[0, :D.E], qkv[0, D.E:2 * D.E], qkv[0, 2 * D.E:]
    k, v = torch.cat([kc[0, :200], kn[None]]), torch.cat([vc[0, :200], vn[None]])
    ref, bar = D.attention64(q, k, v, 12)
    s = torch.einsum("hc,jhc->hj", q.view(12, 64), k.view(-1, 12, 64)) / 8.0
    assert float(s.abs().max()) > 80.0
    got = torch.einsum("hj,jhc->hc", torch.softmax(s, -1), v.view(-1, 12, 64)).reshape(-1)
    assert bool(torch.isfinite(got).all()) and D.worst_ratio(got, ref, bar) <= 1.0


def test_references_agree_with_the_float64_gpt2_on_one_layer():
    """One GPT-2 layer put together from layer_gemm64 and attention64 equals GPT2_64.forward on the same weights, with a cache."""
    w = W.synth_viecap(481, clip_hidden_size=512, n_layer=1, tok_vocab=600, map_layers=1)
    m = R.GPT2_64(w)
    p = "gpt.transformer.h.0."
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 6, D.E, generator=g, dtype=torch.float64)
    want, _ = m.forward(x)

    def case(key, epi, ln):
        wt = w[p + key + ".weight"].double().T.contiguous()          # Conv1D stores [in][out]
        c = {"W": wt, "b": w[p + key + ".bias"].double(), "epi": epi, "ln": ln is not None, "eps": 1e-5}
        if ln:
            c["ln_w"], c["ln_b"] = w[p + ln + ".weight"].double(), w[p + ln + ".bias"].double()
        return c

    got = torch.empty_like(x)
    for n in range(2):
        h = x[n]
        qkv, _ = D.layer_gemm64(case("attn.c_attn", D.STORE, "ln_1"), h)
        att = torch.stack([D.attention64(qkv[t, :D.E], qkv[:t + 1, D.E:2 * D.E], qkv[:t + 1, 2 * D.E:], 12)[0] for t in range(6)])
        h, _ = D.layer_gemm64(case("attn.c_proj", D.RESID, None), att, old=h)
        hid, _ = D.layer_gemm64(case("mlp.c_fc", D.GELU, "ln_2"), h)
        got[n], _ = D.layer_gemm64(case("mlp.c_proj", D.RESID, None), hid, old=h)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.fixture(scope="module")
def lib():
    from patchioner_amd import build
    build.build()
    from patchioner_amd import _lib
    return _lib.load()


def test_fold_restatement_is_the_loaders(lib):
    """decoder_ref64.fold64 equals pio_host_ln_fold (the arithmetic upload_ln_folded runs): w' and d bit for bit, c to one unit in the
    last place (another order of the same double sum), in both weight layouts; and the folded form is the LayerNorm form in float64."""
    from patchioner_amd import _lib
    for name in ("qkv", "fc"):
        c = D.layer_case(name)
        Nout, K = c["Nout"], c["K"]
        wf, cv, dv = D.fold64(c)
        for in_major in (0, 1):
            src = c["W"].T.contiguous() if in_major else c["W"]
            w2, c2, d2 = torch.empty(Nout, K), torch.empty(Nout), torch.empty(Nout)
            _lib.check(lib.pio_host_ln_fold(src.data_ptr(), in_major, K, Nout, c["ln_w"].data_ptr(), c["ln_b"].data_ptr(), c["b"].data_ptr(),
                                            w2.data_ptr(), c2.data_ptr(), d2.data_ptr()))
            assert torch.equal(w2, wf) and torch.equal(d2, dv)
            # the loader adds the row sum sequentially in double, torch pairwise: the same fp32 number unless the sum sits on a rounding edge
            assert float((c2.double() - cv.double()).abs().max()) <= 2.0 ** -23 * float(cv.abs().max())
        x = D.x_family("massive", 8, K).double()
        mu = x.mean(-1, keepdim=True)
        r = 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + c["eps"])
        y = r * (x @ wf.double().T - mu * cv.double()) + dv.double()
        ref, bar = D.layer_gemm64(dict(c, epi=D.STORE), x)
        assert D.worst_ratio(y, ref, bar()) <= 1.0
    assert lib.pio_host_ln_fold(None, 0, 8, 8, None, None, None, None, None, None) == -1
