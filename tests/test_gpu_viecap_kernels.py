"""Every kernel of the ViECap head against a plain float64 statement of the same operation (tests/viecap_ref64.py), at the shapes and
values where these kernels change code path: ragged M and N tiles of k_sgemm_tn, k_softmax_rows above one 256-thread pass, the mapping
attention at its S <= 32 limit, the hard-prompt selection at ties / NaN / the threshold, k_dec_score at N = 64 and Lmax = max_steps, the
greedy decode above 64 rows (split-fp16 GEMMs) and around the prefill family change at 16 prompt tokens.

Bars are derived, not fitted.  Unit roundoff u = 2^-24 (fp32 operands and accumulation: the exact-fp32 MFMA chains); u = 2^-22 where an
operand is carried as a pair of fp16 values (22 significant bits: the split-fp16 layer GEMMs of a decode above 64 rows).  A
dot product of length K carries a rounding error of about sqrt(K) u relative to the magnitudes it sums (errors of random sign); through a
network of depth D each level adds its own, so relative to the largest output the error is about sqrt(K_max) D u; SAFETY = 8 covers the
constant of the random-walk estimate and the non-GEMM steps (LayerNorm, softmax, exp / log).  Where a golden bar of tests/test_gpu_viecap.py
exists (2e-4 mapping / probabilities, 5e-4 perplexity, 1e-3 logit units for a greedy departure) the bar is the smaller of the two.  Each
test prints its observed maximum next to its bar.  Ids and token rows are held exactly: a greedy id may depart from the float64 id only at
a step whose float64 top-2 margin is below the logit bar (no test accepts a fraction)."""
import math
import random

import numpy as np
import pytest
import torch

import golden_cases as gc
import viecap_ref64 as R
from parity_helpers import MARGIN_BOUND
from patchioner_amd import viecap as V
from patchioner_amd import weights as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

U32, U_SPLIT16, SAFETY = 2.0 ** -24, 2.0 ** -22, 8.0
GOLDEN_MAP, GOLDEN_PROB, GOLDEN_PPL = 2e-4, 2e-4, 5e-4


def _report(label, observed, bar):
    print("%-60s observed %.3e   bar %.3e" % (label, observed, bar))
    assert observed <= bar, "%s: %.3e above its bar %.3e" % (label, observed, bar)


@pytest.fixture(scope="module")
def tok():
    vocab, merges = W.synth_bpe(0)
    return V.ByteLevelBPE(vocab, merges)


def _model(w, tok, ents, emb, C, max_prefixes=136, **over):
    from patchioner_amd import Patchioner
    dino = "dinov2_vitb14_reg"
    vc = dict(clip_hidden_size=C, weights=w, tokenizer=tok, entities_text=ents, texts_embeddings=emb, temperature=0.01, top_k=3,
              threshold=0.2, using_hard_prompt=False, soft_prompt_first=True, using_greedy_search=True)
    vc.update(over)
    cfg = {"decap_weights": None, "prefix_size": 768, "linear_talk2dino": False, "support_memory_size": 0, "dino_model": dino,
           "normalize": False, "resize_dim": 224, "crop_dim": 224, "dino_weights": W.synth_dinov2(91, dino, depth=2),
           "max_batch": 4, "max_prefixes": max_prefixes, "viecap": vc}
    return Patchioner.from_config(cfg, device="cuda")


def _features(seed, N, C, spread=6):
    """Rows of very different norms (10^-spread .. 10^spread), some of them close to an entity direction."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, generator=g)
    scale = 10.0 ** (torch.rand(N, 1, generator=g) * 2 * spread - spread)
    return (x * scale).contiguous()


# ------------------------------------------------------------------------------------------------ mapping network
@pytest.mark.parametrize("C", [512, 768, 1024])
@pytest.mark.parametrize("Lp,Lc", [(10, 10), (16, 16)])
def test_mapping_network_vs_float64(tok, C, Lp, Lc):
    """k_l2norm_rows, then k_sgemm_tn (M = N, N = Lp E), 8 pre-LN layers of k_layernorm_f32 / k_sgemm_tn (M = N S: ragged 64-row tiles
    at N = 1, 3, 63, 65, 130) / k_map_attention (S = 32 at (16, 16): the kernel's limit).  Bar, relative to the largest output:
    SAFETY sqrt(K_max) (layers + 1) u, K_max = max(C, E, 2E) the longest dot product, capped at the golden 2e-4.  The in-place
    normalisation: a norm of C squares and one division per element, SAFETY (sqrt(C) + 2) u relative to the row's largest element."""
    E, layers = 768, 8
    w = W.synth_viecap(400 + C + Lp, clip_hidden_size=C, n_layer=2, tok_vocab=len(tok), prompt_len=Lc, project_len=Lp)
    ents = list(W.SYNTH_ENTITIES)
    m = _model(w, tok, ents, W.synth_entity_embeddings(7, len(ents), C), C)
    try:
        x = _features(C + Lp, 130, C)
        bar = min(SAFETY * math.sqrt(max(C, E, 2 * E)) * (layers + 1) * U32, GOLDEN_MAP)
        bar_n = SAFETY * (math.sqrt(C) + 2) * U32
        worst, worst_n = 0.0, 0.0
        for N in (1, 3, 63, 64, 65, 130):
            xd = x[:N].cuda().contiguous()
            cont = m.engine.viecap_mapping(xd).cpu().double()
            ref = R.mapping64(w, x[:N])
            assert cont.shape == ref.shape == (N, Lc, E)
            assert bool(torch.isfinite(cont).all())
            worst = max(worst, float((cont - ref).abs().max() / ref.abs().max()))
            xn = x[:N].double() / x[:N].double().norm(dim=-1, keepdim=True)
            worst_n = max(worst_n, float(((xd.cpu().double() - xn).abs().max(dim=1).values / xn.abs().max(dim=1).values).max()))
        _report("mapping C=%d S=%d, N in 1..130 (rel. to max)" % (C, Lp + Lc), worst, bar)
        _report("in-place L2 normalisation C=%d" % C, worst_n, bar_n)
    finally:
        m.engine.close()


def test_mapping_network_above_32_positions_is_refused(tok):
    """k_map_attention holds S <= 32 positions in LDS: a checkpoint with Lp + Lc = 33 is refused when the weights are finalised."""
    from patchioner_amd._lib import PioError
    w = W.synth_viecap(431, clip_hidden_size=512, n_layer=1, tok_vocab=len(tok), prompt_len=16, project_len=17, map_layers=1)
    ents = list(W.SYNTH_ENTITIES)
    with pytest.raises(PioError, match="32 tokens"):
        _model(w, tok, ents, W.synth_entity_embeddings(7, len(ents), 512), 512)


# ------------------------------------------------------------------------------------------------ entity probabilities
def _entities(seed, K, C):
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(K, C, generator=g)
    if K >= 4:
        e[2] = e[1] * 3.0                                  # the same direction: an exact tie in the cosine, up to rounding
        e[3] = e[1] + 1e-3 * torch.randn(C, generator=g)   # a near tie
    return e


def _prob_features(seed, N, e):
    """Peaked rows (an entity's direction, little noise), near-tied rows (the direction of entities 1-3), flat rows (a tiny feature
    nearly orthogonal to every entity) and plain noise at very different norms."""
    K, C = e.shape
    g = torch.Generator().manual_seed(seed)
    en = e / e.norm(dim=-1, keepdim=True)
    x = _features(seed, N, C, spread=4)
    for i in range(N):
        kind = i % 4
        if kind == 0:
            x[i] = en[(7 * i) % K] * 10.0 ** (i % 5 - 2) + 1e-3 * torch.randn(C, generator=g)
        elif kind == 1 and K >= 4:
            x[i] = en[1] + 1e-4 * torch.randn(C, generator=g)
        elif kind == 2:
            x[i] = 1e-3 * torch.randn(C, generator=g)
    return x.contiguous()


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 255, 256, 257, 4099])
def test_entity_probabilities_vs_float64(tok, K):
    """pio_viecap_entity_logits: k_sgemm_tn with alpha = 1/T (ragged N tile for K % 64 != 0), then k_softmax_rows (K above 256: more
    than one pass per thread).  Compared in log-probability space wherever p > 1e-30.  A cosine of unit vectors carries SAFETY (sqrt(C)
    + 4) u (the dot product, both normalisations), a logit that divided by T; a log-probability is a logit minus a log-sum-exp, each off
    by at most that: bar 2 SAFETY (sqrt(C) + 4) u / T, capped at the golden 2e-4.  Row sums: the fp32 sum of K terms behind the
    normaliser, SAFETY (sqrt(K) + 4) u."""
    C = 768
    ents = ["e%d" % i for i in range(K)]
    emb = _entities(K, K, C)
    w = W.synth_viecap(451, clip_hidden_size=C, n_layer=2, tok_vocab=len(tok), map_layers=1)
    m = _model(w, tok, ents, emb, C)
    try:
        for T in (1.0, 0.01):
            bar = min(2 * SAFETY * (math.sqrt(C) + 4) * U32 / T, GOLDEN_PROB)
            bar_sum = SAFETY * (math.sqrt(K) + 4) * U32
            worst, worst_sum = 0.0, 0.0
            for N in (1, 65):
                x = _prob_features(K + N, N, emb)
                xd = x.cuda()
                xd /= xd.norm(dim=-1, keepdim=True)        # the features reach the kernel normalised (pio_viecap_mapping does it)
                p = m.engine.viecap_entity_logits(xd.contiguous(), T).cpu().double()
                p64, logp64 = R.entity_probs64(x, emb, T)
                assert bool(torch.isfinite(p).all())
                live = p64 > 1e-30
                assert bool((p[live] > 0).all())
                worst = max(worst, float((p[live].log() - logp64[live]).abs().max()))
                worst_sum = max(worst_sum, float((p.sum(dim=1) - 1.0).abs().max()))
            _report("entity log-probs K=%d T=%g" % (K, T), worst, bar)
            _report("entity row sums K=%d T=%g" % (K, T), worst_sum, bar_sum)
    finally:
        m.engine.close()


# ------------------------------------------------------------------------------------------------ hard-prompt composition
nan = float("nan")


def _long_entities(tok, n=300):
    """n entities; 8 of them share a long prefix and end in two rare letters, chosen so that their middle and last fragments are the
    longest of the list and equally long: a top_k = 8 prompt of those 8 is a row of exactly Lmax tokens."""
    pre = "qzjx qzjx qzjx qzjx qzjx qzjx"
    shape = lambda e: (len(tok.encode(" " + e + ",")), len(tok.encode(" " + e + " in image.")))      # noqa: E731
    cands = [pre + " " + a + b for a in "qzjxvk" for b in "qzjxvk"]
    top = max(shape(e) for e in cands)
    long_ = [e for e in cands if shape(e) == top][:8]
    rng = random.Random(17)
    letters = "abcdefghijklmnopqrstuvwxyz"
    ents = set(long_)
    while len(ents) < n:
        ents.add(" ".join("".join(rng.choice(letters) for _ in range(rng.randint(2, 7))) for _ in range(rng.randint(1, 2))))
    return sorted(ents), long_


def _edge_rows(K, threshold, rng):
    """Rows of probabilities at the selection's edges: exact ties, a flat row, NaN entries, an all-NaN row, values equal to
    float32(threshold) and to the next fp32 value below it, zeros."""
    t32 = float(np.float32(threshold))
    below = float(np.nextafter(np.float32(threshold), np.float32(0)))
    rows = []
    flat = [1.0 / K] * K
    rows.append(flat)
    r = [0.0] * K
    for i in rng.sample(range(K), 5):
        r[i] = 0.3
    rows.append(r)                                                   # five-way exact tie
    r = [0.001] * K
    for i in rng.sample(range(K), 3):
        r[i] = nan
    r[rng.randrange(K)] = 0.5
    rows.append(r)                                                   # NaN first, then the largest
    rows.append([nan] * K)
    r = [0.0] * K
    idx = rng.sample(range(K), 4)
    r[idx[0]], r[idx[1]], r[idx[2]], r[idx[3]] = t32, below, t32, 0.9
    rows.append(r)                                                   # on the threshold and just below it
    rows.append([0.0] * K)
    levels = [0.0, 0.05, t32, below, 0.35, 0.7, nan]
    for _ in range(24):
        rows.append([rng.choice(levels[:-1]) if rng.random() > 0.05 else nan for _ in range(K)])
    return rows


def _reference_rows(frag, probs, top_k, threshold, calls, pad_id=0):
    picks = [R.select_reference(probs[i], top_k, threshold) for i in range(probs.shape[0])]
    rows, lens = [], []
    for a, b in calls:
        r = [frag.row(picks[i]) for i in range(a, b)]
        L = max(len(t) for t in r)
        rows += [t + [pad_id] * (L - len(t)) for t in r]
        lens += [L] * (b - a)
    return rows, lens, picks


def test_composition_vs_reference_selection(tok):
    """k_compose_prompts + k_pad_prompts against select_reference + the fragment table, token rows and lens exactly, and against the host
    path (top_k_entities + encode): the equality forward() vs forward_async / the pipeline rests on.  N = 300 rows (k_pad_prompts scans
    more than 256 rows per call) and N = 1; many calls, some of one row; top_k = 8 rows reach Lmax."""
    ents300, long_ = _long_entities(tok)
    assert len(long_) == 8
    w = W.synth_viecap(461, clip_hidden_size=512, n_layer=1, tok_vocab=len(tok), map_layers=1)
    small = list(W.SYNTH_ENTITIES)
    m = _model(w, tok, small, W.synth_entity_embeddings(7, len(small), 512), 512, max_prefixes=16)
    eng = m.engine
    rng = random.Random(3)
    try:
        for threshold, (ents, top_k) in ((t, c) for t in (0.2, 0.4, 0.35, 0.45, 0.7, 0.0) for c in ((small, 3), (ents300, 8), (ents300, 1))):
            frag = V.PromptFragments(tok, ents, top_k)
            assert frag.bad == []
            frag.to(eng.device)
            K = len(ents)
            rows = _edge_rows(K, threshold, rng)
            if top_k == 8:
                r = [0.0] * K
                for j, e in enumerate(long_):
                    r[ents.index(e)] = 0.9 - 0.01 * j
                rows.append(r)
            while len(rows) < 300:
                rows.append([rng.choice([0.0, 0.01, 0.2, 0.3, 0.35, 0.4, 0.45, 0.7, 1.0 / K]) for _ in range(K)])
            probs = torch.tensor(rows, dtype=torch.float32)
            for N in (300, 1):
                p = probs[:N].contiguous()
                if N == 1:
                    calls = [(0, 1)]
                    seg = None
                else:
                    cuts = sorted(set([0, 1, 2, 3, 40, 41, 100, 257, 258, 299, 300] + rng.sample(range(4, 299), 20)))
                    calls = list(zip(cuts[:-1], cuts[1:]))
                    seg = torch.tensor(sum([[i] * (b - a) for i, (a, b) in enumerate(calls)], []), dtype=torch.int32, device="cuda")
                tokens, lens = eng.viecap_compose_prompts(p.cuda(), frag, top_k, threshold, pad_id=0, seg=seg)
                want_rows, want_lens, picks = _reference_rows(frag, p, top_k, threshold, calls)
                got, got_lens = tokens.cpu().tolist(), lens.cpu().tolist()
                assert got_lens == want_lens
                for i, r in enumerate(want_rows):
                    assert got[i][:len(r)] == r, (i, p[i].tolist()[:8], picks[i])
                    assert all(t == 0 for t in got[i][len(r):])
                for i in range(N):                                   # the host path selects and tokenises the same
                    host = tok.encode(V.compose_discrete_prompt_text(V.top_k_entities(ents, p[i], top_k, threshold)))
                    assert host == frag.row(picks[i]), i
                if top_k == 8 and N == 300:
                    assert max(want_lens) == frag.Lmax == max(got_lens)
            print("composition threshold=%g K=%d top_k=%d: 300 + 1 rows exact" % (threshold, K, top_k))
    finally:
        m.engine.close()


# ------------------------------------------------------------------------------------------------ build_prompt
def test_build_prompt_is_the_concatenation_bit_for_bit(tok):
    """k_build_prompt copies: soft first, hard first, no soft prompt (Lc = 0), ids at 0 and V - 1."""
    w = W.synth_viecap(471, clip_hidden_size=512, n_layer=1, tok_vocab=50257, map_layers=1)     # every wte row live, V - 1 included
    ents = list(W.SYNTH_ENTITIES)
    m = _model(w, tok, ents, W.synth_entity_embeddings(7, len(ents), 512), 512, max_prefixes=16)
    eng = m.engine
    try:
        V_ = eng.cfg.dec_vocab
        wte = w["gpt.transformer.wte.weight"]
        g = torch.Generator().manual_seed(5)
        N, Lc, Lt = 5, 10, 7
        cont = torch.randn(N, Lc, 768, generator=g)
        tokens = torch.randint(0, V_, (N, Lt), generator=g, dtype=torch.int32)
        tokens[0, 0], tokens[1, -1], tokens[2, :] = 0, V_ - 1, V_ - 1
        tokens[3, 3] = 0
        hard = wte[tokens.long()]
        for soft_first in (True, False):
            got = eng.viecap_build_prompt(cont.cuda(), tokens, soft_first=soft_first).cpu()
            want = torch.cat((cont, hard), 1) if soft_first else torch.cat((hard, cont), 1)
            assert torch.equal(got, want), soft_first
        assert torch.equal(eng.viecap_build_prompt(None, tokens).cpu(), hard)
        assert torch.equal(eng.viecap_build_prompt(None, tokens[:, :1]).cpu(), hard[:, :1])
    finally:
        m.engine.close()


# ------------------------------------------------------------------------------------------------ teacher-forced score
def _nll_bar(layers, amax, u=U32):
    """Per scored position: a logit off by SAFETY sqrt(4E) (layers + 1) u max|logit| (the longest dot product, the layers and the head),
    the log-sum-exp by as much: twice that on -log p.  Capped at the golden perplexity bar 5e-4 (relative perplexity = the per-position
    mean of the nll error)."""
    return np.minimum(2 * SAFETY * math.sqrt(4 * 768) * (layers + 1) * u * amax, GOLDEN_PPL)


def _score_rows(V_, seed, max_steps):
    g = random.Random(seed)
    rows = [[0], [V_ - 1, 0], [0] * max_steps, [g.randrange(V_) for _ in range(max_steps)], [V_ - 1] * 9]
    while len(rows) < 64:
        n = g.choice([1, 2, 3, g.randint(4, 40)])
        rows.append([g.choice([0, V_ - 1, g.randrange(V_)]) for _ in range(n)])
    return rows


@pytest.mark.parametrize("massive", [False, True])
def test_lm_score_vs_float64(tok, massive):
    """pio_lm_score (k_dec_token_x, the layers, the exact head's partials, k_dec_score) against gpt2_nll64 at N = 1, 63, 64, lengths 1
    (nll 0, perplexity NaN), 2, mixed and max_steps = 256, ids 0 and V - 1.  ``massive``: three residual channels carry 1e2, 3e2 and
    1e3 through wpe (where real GPT-2 checkpoints put their massive activations); the decoder's LayerNorm statistics are one pass,
    E[x^2] - mu^2, folded into the GEMMs."""
    w = W.synth_viecap(481, clip_hidden_size=512, n_layer=2, tok_vocab=50257, map_layers=1)
    if massive:
        wpe = w["gpt.transformer.wpe.weight"].clone()
        for c, a in ((64, 1e2), (383, 3e2), (700, -1e3)):
            wpe[:, c] += a
        w["gpt.transformer.wpe.weight"] = wpe
    ents = list(W.SYNTH_ENTITIES)
    m = _model(w, tok, ents, W.synth_entity_embeddings(7, len(ents), 512), 512, max_prefixes=64)
    eng = m.engine
    try:
        V_ = eng.cfg.dec_vocab
        rows = _score_rows(V_, 3 + massive, 256)
        ref, amax = R.gpt2_nll64(w, rows)
        worst = (0.0, 0.0, 1.0)                        # (error / bar, error, bar) of the row closest to its bar
        for N in (64, 63, 1):
            got = eng.lm_score(rows[:N]).cpu().double()
            assert bool(torch.isfinite(got).all())
            for i in range(N):
                n = len(rows[i])
                if n < 2:
                    assert float(got[i]) == 0.0
                    continue
                err = abs(float(got[i]) - float(ref[i])) / (n - 1)
                bar = float(_nll_bar(2, float(amax[i])))
                worst = max(worst, (err / bar, err, bar))
                assert err <= bar, "row %d (length %d): per-position nll error %.3e above %.3e" % (i, n, err, bar)
        _report("lm_score per-position nll%s (row nearest its bar)" % (" massive channels" if massive else ""), worst[1], worst[2])
        ppl = m.viecap.compute_perplexity(["c", "a dog."])
        assert math.isnan(ppl[0]) and math.isfinite(ppl[1])
    finally:
        m.engine.close()


# ------------------------------------------------------------------------------------------------ greedy decode
def _departures_explained(got, ref_ids, ref_margins, bar, label):
    """Row by row: equal to the float64 ids, or equal up to a first departing step whose float64 top-2 margin is at most ``bar`` (after
    that the histories differ and nothing further is compared)."""
    departed, worst = 0, 0.0
    for r in range(got.shape[0]):
        d = (got[r] != ref_ids[r]).nonzero()
        if len(d) == 0:
            continue
        t = int(d[0])
        mg = float(ref_margins[r, t])
        departed += 1
        worst = max(worst, mg)
        assert mg <= bar[r], "%s: row %d departs from the float64 ids at step %d where their top-2 margin is %.3e (bar %.3e)" % (
            label, r, t, mg, bar[r])
    return departed, worst


def _greedy_bar(amax, layers, u):
    return np.minimum(2 * SAFETY * math.sqrt(4 * 768) * (layers + 1) * u * amax.numpy(), MARGIN_BOUND)


@pytest.fixture(scope="module")
def greedy_model(tok):
    w = W.synth_viecap(491, clip_hidden_size=768, n_layer=2, tok_vocab=len(tok), map_layers=2)
    ents = list(W.SYNTH_ENTITIES)
    m = _model(w, tok, ents, W.synth_entity_embeddings(7, len(ents), 768), 768, max_prefixes=128)
    ref = R.GPT2_64(w)
    x = _features(91, 128, 768, spread=2)
    cont = m.engine.viecap_mapping(x.cuda().contiguous())
    g = torch.Generator().manual_seed(13)
    tokens = torch.randint(0, len(tok), (128, 17), generator=g, dtype=torch.int32)
    tokens[::5, 0] = 0
    yield m, w, ref, cont, tokens
    m.engine.close()


def _embeds(ref, cont, tokens, soft_first):
    parts = [cont.cpu().double()] if cont is not None else []
    if tokens is not None and tokens.shape[1] > 0:
        hard = ref.wte[tokens.long()]
        parts = parts + [hard] if soft_first else [hard] + parts
    return torch.cat(parts, dim=1)


@pytest.mark.parametrize("Lt,soft_first", [(0, True), (1, True), (1, False), (15, True), (15, False), (16, True), (16, False),
                                           (17, True), (17, False)])
def test_greedy_decode_vs_float64(greedy_model, Lt, soft_first):
    """pio_viecap_decode at N = 1, 17, 65, 128 (above 64 rows: split-fp16 layer GEMMs, u = 2^-22 in the bar) with Lt hard-prompt tokens
    around 16 (the prefill's kernel family changes there), both prompt orders; 64 steps.  The float64 search runs on the device's own
    soft prompt.  Departure bar: two logits each off by SAFETY sqrt(4E) (layers + 1) u max|logit|, capped at the golden 1e-3."""
    m, w, ref, cont, tokens = greedy_model
    tok_ = tokens[:, :Lt] if Lt else None
    ids64, margins, amax = R.gpt2_greedy64(w, _embeds(ref, cont, tok_, soft_first), 64, model=ref)
    for N in (1, 17, 65, 128):
        got = m.engine.viecap_decode(cont[:N], tok_[:N] if tok_ is not None else None, soft_first=soft_first, steps=64).cpu().long()
        u = U_SPLIT16 if N > 64 else U32
        bar = _greedy_bar(amax[:N], 2, u)
        dep, worst = _departures_explained(got, ids64[:N], margins[:N], bar, "decode Lt=%d N=%d" % (Lt, N))
        print("decode Lt=%2d %s N=%3d: %d / %d rows equal to float64, departures at margins <= %.2e (bar >= %.2e)"
              % (Lt, "soft-first" if soft_first else "hard-first", N, N - dep, N, worst, float(bar.min())))


@pytest.mark.parametrize("soft_first", [True, False])
def test_ragged_decode_vs_float64(greedy_model, soft_first):
    """pio_viecap_decode_ragged at N = 1, 17, 65, 128 with per-row hard-prompt lengths 0..17 (prompt lengths on both sides of 16), each
    row against the float64 search on its own prompt; the one-row kernels whatever N (u = 2^-24)."""
    m, w, ref, cont, tokens = greedy_model
    lens = torch.tensor([(5 * i) % 18 for i in range(128)], dtype=torch.int32)
    ids64 = torch.zeros(128, 64, dtype=torch.long)
    margins = torch.zeros(128, 64, dtype=torch.float64)
    amax = torch.zeros(128, dtype=torch.float64)
    for L in sorted(set(lens.tolist())):
        rows = (lens == L).nonzero().flatten()
        i_, m_, a_ = R.gpt2_greedy64(w, _embeds(ref, cont[rows], tokens[rows, :L], soft_first), 64, model=ref)
        ids64[rows], margins[rows], amax[rows] = i_, m_, a_
    tok_d, lens_d = tokens.cuda(), lens.cuda()
    for N in (1, 17, 65, 128):
        got = m.engine.viecap_decode_ragged(cont[:N], tok_d[:N], lens_d[:N], soft_first=soft_first, steps=64).cpu().long()
        bar = _greedy_bar(amax[:N], 2, U32)
        dep, worst = _departures_explained(got, ids64[:N], margins[:N], bar, "ragged N=%d" % N)
        print("ragged decode %s N=%3d: %d / %d rows equal to float64, departures at margins <= %.2e"
              % ("soft-first" if soft_first else "hard-first", N, N - dep, N, worst))


# ------------------------------------------------------------------------------------------------ full depth, once
def test_full_depth_head_at_the_golden_size_vs_float64(tok):
    """The golden case's model (12 GPT-2 layers, 8 mapping layers, C = 768, 6 features): mapping, entity probabilities, the hard-prompt
    selection, greedy ids on the device's own prompt and the teacher-forced score, each against its float64 statement, bars as above
    with 12 layers."""
    w, _, ents, emb, x = gc.viecap_case()
    c = gc.VIECAP
    m = _model(w, tok, ents, emb, c["C"], max_prefixes=16, temperature=c["temperature"], top_k=c["top_k"], threshold=c["threshold"],
               using_hard_prompt=True)
    eng = m.engine
    try:
        xd = x.clone().cuda()
        cont = eng.viecap_mapping(xd)
        ref = R.mapping64(w, x)
        _report("full depth: mapping (rel. to max)", float((cont.cpu().double() - ref).abs().max() / ref.abs().max()),
                min(SAFETY * math.sqrt(1536) * 9 * U32, GOLDEN_MAP))
        p = eng.viecap_entity_logits(xd, c["temperature"]).cpu()
        _, logp64 = R.entity_probs64(x, emb, c["temperature"])
        live = logp64 > math.log(1e-30)
        _report("full depth: entity log-probs", float((p.double()[live].log() - logp64[live]).abs().max()),
                min(2 * SAFETY * (math.sqrt(768) + 4) * U32 / c["temperature"], GOLDEN_PROB))
        caps = m.viecap.forward(x.clone())
        prompt = m.viecap.last_prompt_tokens
        for i in range(x.shape[0]):
            picks = R.select_reference(p[i], c["top_k"], c["threshold"])
            want = tok.encode(V.compose_discrete_prompt_text([ents[j] for j in picks]))
            assert prompt[i, :len(want)].tolist() == want
        g64 = R.GPT2_64(w)
        ids64, margins, amax = R.gpt2_greedy64(w, _embeds(g64, cont, prompt, True), 64, model=g64)
        got = m.viecap.last_ids.cpu().long()
        dep, worst = _departures_explained(got, ids64, margins, _greedy_bar(amax, 12, U32), "full depth decode")
        print("full depth decode: %d / %d rows equal to float64 (worst departure margin %.2e)" % (6 - dep, 6, worst))
        rows = [tok.encode(s) for s in caps] + [tok.encode("a dog on the road."), [0, 50256, 5]]
        nll64, amax = R.gpt2_nll64(w, rows, model=g64)
        got = eng.lm_score(rows).cpu().double()
        worst = (0.0, 0.0, 1.0)
        for i, r in enumerate(rows):
            if len(r) > 1:
                err, bar = abs(float(got[i] - nll64[i])) / (len(r) - 1), float(_nll_bar(12, float(amax[i])))
                worst = max(worst, (err / bar, err, bar))
                assert err <= bar, (i, err, bar)
        _report("full depth: lm_score per-position nll (row nearest its bar)", worst[1], worst[2])
    finally:
        m.engine.close()
