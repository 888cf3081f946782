"""ClipCap head on the device: the nucleus sampler against the float64 statement (tests/clipcap_ref64.py), its edge rows, placement
invariance, the device Philox against the host copy, the MLP mapper against float64, and the head through the public API.

Boundary rule of the sampler comparisons.  The kernel's sums are fp32: every term w_i = exp(s_i - max) carries the subtraction's
rounding, 2^-24 |s_i - max| in the exponent (<= 2^-24 x 16 = 9.5e-7 for every token of more than 1e-7 of the largest mass; the
rest together hold less than 1e-6 of it), plus expf's 1 ulp, 2^-23 = 1.2e-7; the reduction is a fixed tree of depth 6 (a thread's 50
values) + 6 (the wave) + 4 (16 waves) = 16 roundings over non-negative terms, 16 x 2^-24 = 9.5e-7.  A sum is therefore off by at
most 2.0e-6 relative; the kept-set test compares S against top_p x Z (two sums: 4.1e-6, + one product rounding), the draw compares a
prefix sum against u x Z_kept (the same).  DELTA = 5e-6 covers both; rows of the float64 statement closer than DELTA to top_p at the
nucleus edge, or to a CDF step at the draw, are boundary cases: there the token may be the kept-set neighbour and the kept-set size
may differ.  V above 51 200 takes the kernel's re-reading path, a chain of ceil(V / 1024) terms per thread: (51 + 6 + 4) x 2^-24 =
3.6e-6 per sum, still inside 2 x DELTA = 1e-5 for the pair, the bar used for that one shape.  At most 5 % of rows may be boundary cases."""
import ctypes

import numpy as np
import pytest
import torch

import clipcap_ref64 as R
from patchioner_amd import _lib
from patchioner_amd import weights as W
from patchioner_amd import viecap as V_

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DELTA = 5e-6
STOP = 13


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _sample(lib, scores, u, T, top_p, stop=STOP, active=None):
    s = torch.as_tensor(scores, dtype=torch.float32).cuda().contiguous()
    N, V = s.shape
    ud = torch.as_tensor(u, dtype=torch.float32).cuda().contiguous()
    act = torch.ones(N, dtype=torch.int32, device="cuda") if active is None else torch.as_tensor(active, dtype=torch.int32).cuda()
    tok = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    kept = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.pio_test_nucleus_sample(_lib.ptr(s), N, V, float(T), float(top_p), _lib.ptr(ud), stop, _lib.ptr(act), _lib.ptr(tok),
                                           _lib.ptr(kept), None))
    torch.cuda.synchronize()
    return tok.cpu().numpy(), act.cpu().numpy(), kept.cpu().numpy()


def _rows(V, N, sigma):
    rng = np.random.default_rng(7)
    s, u = [], []
    for _ in range(N):
        s.append((rng.standard_normal(V) * sigma).astype(np.float32))
        u.append(rng.random(8))
    return np.stack(s), np.stack(u).astype(np.float32)


@pytest.mark.parametrize("V,N", [(1, 3), (63, 3), (64, 3), (65, 3), (1024, 3), (1025, 3), (50257, 3), (51201, 3), (50257, 64)])
@pytest.mark.parametrize("sigma", [4.0, 8.0])
def test_kernel_against_float64(lib, V, N, sigma):
    scores, us = _rows(V, N, sigma)
    delta = DELTA if V <= 51200 else 2 * DELTA
    ref = [R.nucleus(scores[n], 1.0, 0.8) for n in range(N)]
    edge_rows = {n for n in range(N) if ref[n][2] <= delta}
    boundary_rows = set(edge_rows)
    for k in range(8):
        tok, act, kept = _sample(lib, scores, us[:, k], 1.0, 0.8)
        for n in range(N):
            km, p, _ = ref[n]
            want, gap, nb = R.draw(km, p, float(us[n, k]))
            print("V=%d row=%d draw=%d kept %d/%d token %d/%d edge_gap %.2e cdf_gap %.2e" % (V, n, k, kept[n], km.sum(), tok[n], want, ref[n][2], gap))
            assert act[n] == (0 if tok[n] == STOP else 1)
            if n in edge_rows:
                # the nucleus edge lies within delta of top_p: the kept set is one of the two on either side of the edge, and the token
                # the float64 draw from one of them, or its neighbour there
                sides = [R.nucleus(scores[n], 1.0, 0.8 + d) for d in (-delta, delta)]
                assert int(kept[n]) in {int(sd[0].sum()) for sd in sides}, (n, k, int(kept[n]))
                allowed = set()
                for sd in sides:
                    allowed |= R.draw(sd[0], sd[1], float(us[n, k]))[2]
                assert int(tok[n]) in allowed, (n, k, int(tok[n]), sorted(allowed))
                continue
            assert kept[n] == km.sum(), (n, k)
            if tok[n] != want:
                assert gap <= delta and int(tok[n]) in nb, (n, k, int(tok[n]), want, gap)
                boundary_rows.add(n)
    assert len(boundary_rows) <= 0.05 * N, (sorted(boundary_rows), N)


def test_edge_rows(lib):
    V = 50257
    rng = np.random.default_rng(11)
    s = (rng.standard_normal((8, V)) * 4).astype(np.float32)
    u = rng.random(8).astype(np.float32)
    am = s.argmax(1)
    tok, act, kept = _sample(lib, s, u, 1.0, 0.0)
    assert (tok == am).all() and (kept == 1).all()                                   # top_p = 0: the arg-max
    for tp in (1.0, 1.5):
        tok, act, kept = _sample(lib, s, u, 1.0, tp)
        assert (kept == V).all()                                                     # top_p >= 1: everything kept
    a = _sample(lib, s, u, 1.0, 0.8)
    for T in (0.0, -2.0):
        b = _sample(lib, s, u, T, 0.8)
        assert all((x == y).all() for x, y in zip(a, b))                             # temperature <= 0 is 1
    bad = s.copy()
    bad[1, 777] = np.nan
    bad[2, 5] = np.inf
    bad[3, 50256] = -np.inf
    tok, act, kept = _sample(lib, bad, u, 1.0, 0.8)
    assert (tok[1:4] == STOP).all() and (act[1:4] == 0).all() and act[0] == 1        # NaN (and inf): the stop token
    assert tok[0] == a[0][0] and (tok[4:] == a[0][4:]).all()
    tok, act, kept = _sample(lib, s, u, 1.0, 0.8, active=[1, 0, 1, 0, 1, 1, 1, 1])
    assert tok[1] == STOP and tok[3] == STOP and act[1] == 0 and act[3] == 0 and act[0] == 1     # inactive rows stay inactive
    one = np.full((2, V), -30.0, dtype=np.float32)
    one[0, 4242] = 20.0
    one[1, STOP] = 20.0
    tok, act, kept = _sample(lib, one, [0.5, 0.5], 1.0, 0.8)
    assert tok[0] == 4242 and kept[0] == 1 and act[0] == 1                            # one token at mass ~ 1
    assert tok[1] == STOP and act[1] == 0                                             # an active row that draws the stop token turns inactive
    km, p, _ = R.nucleus(s[0], 1.0, 0.8)
    ids = np.nonzero(km)[0]
    tok, _, _ = _sample(lib, s[:1], [0.0], 1.0, 0.8)
    assert tok[0] == ids[0]                                                           # u = 0: the first kept id
    tok, _, _ = _sample(lib, s[:1], [np.nextafter(np.float32(1), np.float32(0))], 1.0, 0.8)
    assert tok[0] == ids[-1]                                                          # the largest u below 1: the last kept id


def test_placement_invariance(lib):
    V = 50257
    rng = np.random.default_rng(3)
    s = (rng.standard_normal((64, V)) * 4).astype(np.float32)
    u = rng.random(64).astype(np.float32)
    for r in (0, 17, 63):
        s[r] = s[5]
        u[r] = u[5]
    tok, _, kept = _sample(lib, s, u, 1.0, 0.8)
    alone, _, kalone = _sample(lib, s[5:6], u[5:6], 1.0, 0.8)
    assert tok[0] == tok[17] == tok[63] == tok[5] == alone[0]
    assert kept[0] == kept[17] == kept[63] == kalone[0]


# ------------------------------------------------------------------------------------------------ engine-level
@pytest.fixture(scope="module")
def tok():
    vocab, merges = W.synth_bpe(0)
    return V_.ByteLevelBPE(vocab, merges)


def _model(tok, seed=5, **cc):
    from patchioner_amd import Patchioner
    dino = "dinov2_vitb14_reg"
    cfg = {"decap_weights": None, "prefix_size": 768, "linear_talk2dino": False, "support_memory_size": 0, "dino_model": dino,
           "normalize": False, "resize_dim": 224, "crop_dim": 224, "dino_weights": W.synth_dinov2(91, dino, depth=2),
           "max_batch": 8, "max_prefixes": 128, "synthetic_seed": seed,
           "clipcap": dict({"tokenizer": tok, "entry_length": 12, "normalize_prefix": True}, **cc)}
    return Patchioner.from_config(cfg, device="cuda")


@pytest.fixture(scope="module")
def model(tok):
    return _model(tok)


def test_device_philox_equals_the_host_copy(lib, model):
    eng, head = model.engine, model.clipcap
    N, steps, seed = 5, 12, 0x1234567890
    x = torch.randn(N, 768, generator=torch.Generator().manual_seed(1)).cuda()
    prefix = eng.clipcap_mapping(x, normalize=True)
    u = np.zeros((N, steps), dtype=np.float32)
    f = ctypes.c_float()
    for n in range(N):
        for k in range(steps):
            assert lib.pio_host_philox_uniform(seed, n, k, ctypes.byref(f)) == 0
            u[n, k] = f.value
    a, la = eng.lm_sample(prefix, steps, 1.0, 0.8, head.stop_token_index, seed=seed)
    b, lb = eng.lm_sample(prefix, steps, 1.0, 0.8, head.stop_token_index, seed=999, uniforms=torch.from_numpy(u))
    assert torch.equal(a, b) and torch.equal(la, lb)
    rows = a.cpu().tolist()
    for r, l in zip(rows, la.cpu().tolist()):
        first = r.index(head.stop_token_index) + 1 if head.stop_token_index in r else steps
        assert l == first and all(t == head.stop_token_index for t in r[first:])
    clone = eng.clone_decoder()
    c, lc = clone.lm_sample(prefix, steps, 1.0, 0.8, head.stop_token_index, seed=seed)
    assert torch.equal(a, c) and torch.equal(la, lc)                                 # a decoder clone gives the same ids
    clone.close()


def test_sampling_prefill_batched_equals_position_by_position(tok, model, monkeypatch):
    """pio_lm_sample takes its prompt through the decoder's one prompt prefill (decoder.hip: dec_prompt_prefill), as the prompted greedy
    decode does: all N x P prompt rows as one batch by default, position by position on a handle created under PIO_DEC_PREFILL=0.  With
    the same uniforms both handles must give the same ids and lens.  N = 3, P = 11, steps = 8: the prompts fit one group of the prefill
    workspace (33 rows, one launch per GEMM).  This is no structural bit identity: the 33-row batch runs k_dec_gemm_b, which sums a GEMM
    row in another order than the 3-row launches of k_dec_gemm, so the two caches differ at rounding level.  The ids are equal as long
    as no such difference moves a draw across a CDF step, which holds for these seeded weights, inputs and uniforms; it is the same kind
    of pin as the one test_gpu_viecap.py puts on the greedy ids of the two paths."""
    N, P, steps = 3, 11, 8
    stop = model.clipcap.stop_token_index
    x = torch.randn(N, 768, generator=torch.Generator().manual_seed(3)).cuda()
    prefix = model.engine.clipcap_mapping(x, normalize=True)
    embeds = prefix.repeat(1, -(-P // prefix.shape[1]), 1)[:, :P].contiguous()
    u = torch.rand(N, steps, generator=torch.Generator().manual_seed(4))
    ids_b, lens_b = model.engine.lm_sample(embeds, steps, 1.0, 0.8, stop, uniforms=u)
    monkeypatch.setenv("PIO_DEC_PREFILL", "0")
    serial = _model(tok)
    ids_s, lens_s = serial.engine.lm_sample(embeds, steps, 1.0, 0.8, stop, uniforms=u)
    torch.cuda.synchronize()
    assert ids_b.shape == (N, steps) and torch.equal(ids_b.cpu(), ids_s.cpu()) and torch.equal(lens_b.cpu(), lens_s.cpu())
    serial.engine.close()


@pytest.mark.parametrize("C", [512, 768, 1024])
def test_mapper_against_float64(C):
    """The decode GEMMs' bar (tests/test_gpu_viecap_kernels.py): SAFETY sqrt(K_max) (levels) u relative to the largest output, K_max = 3840
    the longer dot product, two levels, u = 2^-24, SAFETY = 8: 8 x 61.97 x 2 x 5.96e-8 = 5.9e-5."""
    import math
    from patchioner_amd.engine import Engine
    sd = W.synth_clipcap(21, C=C, n_layer=1, vocab=512, n_positions=64, tok_vocab=512)
    eng = Engine(embed_dim=768, depth=2, num_heads=12, num_registers=4, crop_dim=224, prefix_size=768, max_prefixes=128, max_steps=64,
                 dec_layers=1, dec_heads=12, dec_vocab=512, dec_positions=64)
    eng.load_state_dict(sd)
    eng.finalize()
    bar = 8 * math.sqrt(3840) * 2 * 2.0 ** -24
    w = {k: sd["clip_project.model.%s" % k].double().numpy() for k in ("0.weight", "0.bias", "2.weight", "2.bias")}
    for N in (1, 5, 128):
        x = torch.randn(N, C, generator=torch.Generator().manual_seed(N)) * 3
        for norm in (False, True):
            xd = x.cuda()
            got = eng.clipcap_mapping(xd, normalize=norm).cpu().double().numpy().reshape(N, -1)
            assert torch.equal(xd.cpu(), x)                                          # the features are not written through
            ref = R.mlp_mapper(x.numpy(), w["0.weight"], w["0.bias"], w["2.weight"], w["2.bias"], norm)
            err = np.abs(got - ref).max() / np.abs(ref).max()
            print("C=%d N=%d normalize=%s rel err %.2e (bar %.2e)" % (C, N, norm, err, bar))
            assert err <= bar
    eng.close()


def test_api(tok, model):
    import golden_cases as gc
    imgs = W.synth_images(0, 2, 224).cuda()
    traces = [gc.block_trace(3, 5), gc.block_trace(9, 1)]
    bboxes = torch.tensor([[[10, 10, 80, 80], [40, 60, 100, 90]], [[0, 0, 224, 224], [100, 20, 50, 120]]], dtype=torch.float32)
    def run(fn):
        a = fn(imgs, get_cls_capt=True, traces=traces)
        a.update(fn(imgs, bboxes=bboxes.clone()))        # forward() rescales the boxes it is given in place, as the reference does
        return a
    out = run(model)
    for key in ("cls_capt", "trace_capts"):
        assert len(out[key]) == 2 and all(isinstance(s, str) and s.endswith(".") for s in out[key]), key
    assert len(out["bbox_capts"]) == 2 and all(len(b) == 2 and all(isinstance(s, str) for s in b) for b in out["bbox_capts"])
    again = run(model)
    res = model.forward_async(imgs, get_cls_capt=True, traces=traces).result()     # forward_async takes the flat caption outputs only
    for key in ("cls_capt", "trace_capts", "bbox_capts"):
        assert again[key] == out[key], key               # the same seed: the same captions
    for key in ("cls_capt", "trace_capts"):
        assert res[key] == out[key], key                 # forward_async equals forward
    feats = torch.randn(3, 768, generator=torch.Generator().manual_seed(2)).cuda()
    with pytest.raises(Exception, match="return_n_best_sims is not supported with clipcap"):
        model.caption_tokens(feats, return_n_best_sims=3)
    caps, scores = model.caption_tokens(feats.clone(), compute_scores=True)
    assert len(caps) == 3 and len(scores) == 3 and all(0.0 < s <= 1.0 for s in scores)
    ids_a = model.clipcap.last_ids.cpu()
    model.clipcap.args.seed = 1
    model.caption_tokens(feats.clone())
    assert not torch.equal(ids_a, model.clipcap.last_ids.cpu())                      # another seed: other draws
    model.clipcap.args.seed = 0
    model.clipcap.args.use_batched_generation = False                                # row by row: the same device path, the same counters
    model.caption_tokens(feats.clone())
    assert torch.equal(ids_a, model.clipcap.last_ids.cpu())
    model.clipcap.args.use_batched_generation = True
    from patchioner_amd.pipeline import TraceCaptionPipeline
    with pytest.raises(NotImplementedError, match="ClipCap"):
        TraceCaptionPipeline(model)


# ------------------------------------------------------------------------------------------------ the reference fixture
@pytest.fixture(scope="module")
def ref(golden):
    import json
    g = golden("clipcap")
    return g, json.loads(bytes(g["meta_json"]).decode())


def _ref_model(meta, top_p, temperature):
    import clipcap_case as cc
    from patchioner_amd import Patchioner
    dino = "dinov2_vitb14_reg"
    c = meta["case"]
    cfg = {"decap_weights": None, "prefix_size": 768, "linear_talk2dino": False, "support_memory_size": 0, "dino_model": dino,
           "normalize": False, "resize_dim": 224, "crop_dim": 224, "dino_weights": W.synth_dinov2(91, dino, depth=1),
           "max_batch": 4, "max_prefixes": 16,
           "clipcap": {"weights": cc.weights(), "tokenizer": cc.StubTokenizer(meta["stop_id"], meta["stop_token"]),
                       "entry_length": c["entry_length"], "top_p": top_p, "temperature": temperature}}
    return Patchioner.from_config(cfg, device="cuda")


def _upto_stop(row, stop_id):
    hit = np.nonzero(row == stop_id)[0]
    return int(hit[0]) + 1 if hit.size else row.shape[0]


def test_greedy_anchor_vs_reference_fixture(ref):
    """top_p = 0: the reference is deterministic.  Ids under the rule of tests/test_gpu_viecap.py (_explained): a row's first departure must sit where the reference's own
    top-2 margin is inside MARGIN_BOUND, and at most one of the four rows may depart; rows compared up to the reference's stop (it
    keeps sampling a stopped row, the device emits stop_id).  Strings equal; compute_scores within the ViECap perplexity tolerance
    (rtol 5e-4)."""
    import clipcap_case as cc
    from parity_helpers import MARGIN_BOUND
    g, meta = ref
    m = _ref_model(meta, 0.0, 1.0)
    caps, scores = m.caption_tokens(cc.features().cuda(), compute_scores=True)
    got, want = m.clipcap.last_ids.cpu().numpy(), g["greedy_ids"]
    departed = []
    for r in range(want.shape[0]):
        n = _upto_stop(want[r], meta["stop_id"])
        diff = np.nonzero(got[r, :n] != want[r, :n])[0]
        if diff.size:
            assert g["greedy_margins"][r, diff[0]] <= MARGIN_BOUND, (r, int(diff[0]), float(g["greedy_margins"][r, diff[0]]))
            departed.append(r)
            continue
        assert (got[r, n:] == meta["stop_id"]).all()
        assert caps[r] == meta["greedy_captions"][r]
        np.testing.assert_allclose(scores[r], g["greedy_scores"][r], rtol=5e-4)
    assert len(departed) <= 1, departed


def test_sampled_run_vs_reference_fixture(ref):
    """The fixture's uniforms, both runs (temperature 1.0 and 0.7): the ids equal the reference's row by row, up to the reference's
    stop.  A row's first departure ends its comparison and must be a boundary case of the float64 statement (DELTA, module docstring)
    on the device's own scores for that step, read back through pio_lm_prefill / pio_lm_advance.  At most 1 row of the 8 may depart."""
    import clipcap_case as cc
    g, meta = ref
    x = cc.features().cuda()
    departed = []
    for k, T in enumerate(meta["case"]["temperatures"]):
        m = _ref_model(meta, meta["case"]["top_p"], T)
        eng, head = m.engine, m.clipcap
        u = torch.from_numpy(g["uniforms"][k])
        caps = head.forward(x, uniforms=u)
        got, want = head.last_ids.cpu().numpy(), g["sampled%d_ids" % k]
        prefix = eng.clipcap_mapping(x, normalize=False)
        for r in range(want.shape[0]):
            n = _upto_stop(want[r], meta["stop_id"])
            diff = np.nonzero(got[r, :n] != want[r, :n])[0]
            if not diff.size:
                assert (got[r, n:] == meta["stop_id"]).all()
                assert caps[r] == meta["sampled%d_captions" % k][r]
                continue
            t = int(diff[0])
            departed.append((k, r, t))
            logp = eng.lm_prefill(prefix[r:r + 1].contiguous())
            for j in range(t):
                logp = eng.lm_advance(torch.tensor([int(want[r, j])], dtype=torch.int32), None, pos=prefix.shape[1] + j)
            km, p, edge = R.nucleus(logp[0].cpu().numpy(), T, meta["case"]["top_p"])
            tok64, gap, nb = R.draw(km, p, float(u[r, t]))
            print("run %d row %d departs at step %d: device %d reference %d float64 %d edge_gap %.2e cdf_gap %.2e" % (k, r, t, got[r, t], want[r, t], tok64, edge, gap))
            assert edge <= DELTA or (gap <= DELTA and int(got[r, t]) in nb), (k, r, t)
        del m
    assert len(departed) <= 1, departed
