"""stop_at_eos on the GPU: the two bookkeeping kernels bit for bit on constructed tables, then the stopping decodes of the engine (DeCap and
ViECap) and of the model against canon(full-length decode) -- bit for bit, whatever the segment length -- with the steps they ran.

The weights are tests/eos_case.py's (a ramp towards the end token in the position table); their stop columns and margins are held against
the oracle in tests/test_stop_at_eos_cpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import eos_case as ec
import golden_cases as gc
from patchioner_amd import weights as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

S0, S1 = 13, 764            # the stop ids of the constructed tables
POISON = S0


def _lib():
    from patchioner_amd import _lib
    return _lib.load(), _lib.check, _lib.ptr


def _scan(ids_dev, s0, s1, stops, first_dev):
    lib, check, ptr = _lib()
    live = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    N, steps = ids_dev.shape
    check(lib.pio_test_dec_stop_scan(ptr(ids_dev), N, steps, s0, s1, stops[0], stops[1], ptr(first_dev), ptr(live), None))
    torch.cuda.synchronize()
    return first_dev.cpu().numpy().astype(np.int64), int(live.item())


def _pad(ids_dev, first_dev):
    lib, check, ptr = _lib()
    out = torch.full_like(ids_dev, -9)
    check(lib.pio_test_dec_stop_pad(ptr(ids_dev), ptr(first_dev), ids_dev.shape[0], ids_dev.shape[1], ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _table(N, steps, seg, seed):
    """ids [N, steps] without a stop id, then per row (row % 8): a stop in column 0; in the first column of the second segment; in the
    last column of the first segment and the first of the second (both sides of the edge); in the last column of the table; nowhere;
    both stop ids, S1 first; two stops of which the second lies in a later segment; a random column."""
    g = np.random.default_rng(seed)
    ids = g.integers(1000, 40000, size=(N, steps)).astype(np.int32)
    e = min(seg, steps - 1)                                    # first column of the second segment (the last column when there is one segment)
    for r in range(N):
        k = r % 8
        if k == 0:
            ids[r, 0] = S0
        elif k == 1:
            ids[r, e] = S0
        elif k == 2:
            ids[r, max(e - 1, 0)] = S0
            ids[r, e] = S1
        elif k == 3:
            ids[r, steps - 1] = S1
        elif k == 5:
            j = int(g.integers(0, steps))
            ids[r, j] = S1
            ids[r, min(j + 1, steps - 1)] = S0 if j + 1 < steps else S1
        elif k == 6:
            j = int(g.integers(0, max(steps - seg, 1)))
            ids[r, j] = S0
            ids[r, min(j + seg, steps - 1)] = S1 if j + seg < steps else ids[r, min(j + seg, steps - 1)]
        elif k == 7:
            ids[r, int(g.integers(0, steps))] = S0
    return ids


@pytest.mark.parametrize("steps", [1, 30, 64])
@pytest.mark.parametrize("N", [1, 5, 64, 128])
def test_scan_walks_the_segments_and_never_reads_past_them(N, steps):
    """After every segment [s0, s1): first == the first stop column of ids[:, :s1], live == the rows without one -- with EVERY column
    >= s1 holding a stop id on the device (what an earlier decode may have left there) and first[] starting as garbage."""
    for seg in sorted({1, 4, 7, steps}):
        if seg > steps:
            continue
        ids = _table(N, steps, seg, 1000 * N + steps + seg)
        first_dev = torch.full((N,), 3, dtype=torch.int32, device="cuda")          # garbage: ignored at s0 == 0
        for s0 in range(0, steps, seg):
            s1 = min(steps, s0 + seg)
            dev = torch.from_numpy(ids).cuda()
            dev[:, s1:] = POISON
            first, live = _scan(dev, s0, s1, (S0, S1), first_dev)
            want = ec.first_stop(ids[:, :s1], (S0, S1))
            want[want == s1] = steps
            assert np.array_equal(first, want), (N, steps, seg, s0)
            assert live == int((want == steps).sum()), (N, steps, seg, s0)
        assert np.array_equal(first, ec.first_stop(ids, (S0, S1)))
        out = _pad(torch.from_numpy(ids).cuda(), first_dev)
        assert np.array_equal(out, ec.canon_ids(ids, (S0, S1))), (N, steps, seg)


def test_scan_keeps_an_earlier_stop_and_takes_one_stop_id_when_the_second_is_absent():
    ids = np.full((6, 30), 7, dtype=np.int32)
    ids[0, 2] = S0; ids[0, 12] = S0            # a stop before s0 (first says so) and another inside [s0, s1): kept
    ids[1, 12] = S1                            # S1 is no stop id when stop1 < 0
    ids[2, 10] = S0                            # column s0
    ids[3, 14] = S0                            # column s1 - 1
    ids[4, 9] = S0; ids[5, 15] = S0            # just outside [s0, s1), first[] says "none": not seen
    first_dev = torch.tensor([2, 30, 30, 30, 30, 30], dtype=torch.int32, device="cuda")
    first, live = _scan(torch.from_numpy(ids).cuda(), 10, 15, (S0, -1), first_dev)
    assert first.tolist() == [2, 30, 10, 14, 30, 30] and live == 3
    first_dev = torch.tensor([2, 30, 30, 30, 30, 30], dtype=torch.int32, device="cuda")
    first, live = _scan(torch.from_numpy(ids).cuda(), 10, 15, (S0, S1), first_dev)
    assert first.tolist() == [2, 12, 10, 14, 30, 30] and live == 2
    # both ids in one row: the earlier column wins, whichever id it holds
    ids = np.full((2, 30), 7, dtype=np.int32)
    ids[0, 4] = S1; ids[0, 5] = S0; ids[1, 4] = S0; ids[1, 5] = S1
    first, live = _scan(torch.from_numpy(ids).cuda(), 0, 30, (S0, S1), torch.zeros(2, dtype=torch.int32, device="cuda"))
    assert first.tolist() == [4, 4] and live == 0


@pytest.mark.parametrize("steps", [1, 30, 64])
@pytest.mark.parametrize("N", [1, 5, 64, 128])
def test_pad_writes_the_canonical_table_and_reads_no_column_after_the_stop(N, steps):
    ids = _table(N, steps, 4, 77 * N + steps)
    first = ec.first_stop(ids, (S0, S1))
    dev = torch.from_numpy(ids).cuda()
    for r in range(N):
        dev[r, int(first[r]) + 1:] = -123                    # what the decode never wrote: must not show
    out = _pad(dev, torch.from_numpy(first.astype(np.int32)).cuda())
    assert np.array_equal(out, ec.canon_ids(ids, (S0, S1)))


def test_hooks_refuse_out_of_contract_calls():
    lib, check, ptr = _lib()
    ids = torch.zeros(4, 30, dtype=torch.int32, device="cuda")
    f = torch.zeros(4, dtype=torch.int32, device="cuda")
    for N, steps, s0, s1 in ((0, 30, 0, 4), (257, 30, 0, 4), (4, 65, 0, 4), (4, 30, 4, 4), (4, 30, 28, 31), (4, 30, -1, 4)):
        assert lib.pio_test_dec_stop_scan(ptr(ids), N, steps, s0, s1, S0, -1, ptr(f), ptr(f), None) < 0
    assert lib.pio_test_dec_stop_pad(ptr(ids), ptr(f), 4, 30, ptr(ids), None) < 0          # in place


# ---- the engine: DeCap ------------------------------------------------------------------------------------------------------------------
def _decap_engine(gamma, max_prefixes=128):
    from patchioner_amd.engine import Engine
    e = Engine(embed_dim=768, depth=1, num_heads=12, num_registers=4, crop_dim=224, max_batch=2, max_prefixes=max_prefixes, vit_dtype="fp16")
    e.load_state_dict(ec.decap_weights(gamma))
    e.finalize()
    return e


@pytest.fixture(scope="module")
def decap_engines():
    made = {}

    def get(gamma):
        if gamma not in made:
            made[gamma] = _decap_engine(gamma)
        return made[gamma]
    yield get
    for e in made.values():
        e.close()


SEGS = (1, 4, 7, 30)


def _check_decap(e, prefix, segs=SEGS):
    """Every segment length: ids == canon(full decode) bit for bit, steps run as eos_case.steps_run says.  -> first stop columns"""
    full = e.decode_greedy(prefix)[0].cpu().numpy()
    first = ec.first_stop(full, [ec.DECAP_EOT])
    want = ec.canon_ids(full, [ec.DECAP_EOT])
    for seg in segs:
        ids, lp = e.decode_greedy(prefix, stop_id=ec.DECAP_EOT, seg=seg)
        assert lp is None and ids.shape == full.shape and ids.dtype == torch.int32
        print("N %d seg %d: first stops %s, steps run %s" % (full.shape[0], seg, first.tolist(), e.last_steps_run))
        assert np.array_equal(ids.cpu().numpy(), want), "seg %d" % seg
        assert e.last_steps_run == [ec.steps_run(first, 30, seg)], "seg %d" % seg
    return first


@pytest.mark.parametrize("N", [1, 3, 16])
@pytest.mark.parametrize("gamma", [0.3, 1.5])
def test_decap_stops_with_the_ids_of_the_full_decode_when_every_row_ends(decap_engines, gamma, N):
    e = decap_engines(gamma)
    first = _check_decap(e, ec.decap_prefixes(N))
    assert first.tolist() == ec.DECAP_FIRST[gamma][:N]                     # the fixture's own columns (margins >= 1e-3)
    if gamma == 0.3 and N == 16:
        assert [ec.steps_run(first, 30, seg) for seg in SEGS] == [19, 20, 21, 30]          # what _check_decap held last_steps_run to


@pytest.mark.parametrize("N", [1, 3, 16])
@pytest.mark.parametrize("gamma", [0.15, 0.0])
def test_decap_runs_every_step_while_a_row_has_not_ended(decap_engines, gamma, N):
    e = decap_engines(gamma)
    # rows 10 and 15 of the gamma 0.15 case do stop (columns 26 and 28): the 16-row call holds them next to rows that never do
    prefix = ec.decap_prefixes(16)[[10, 0, 15]] if (gamma == 0.15 and N == 3) else ec.decap_prefixes(N)
    first = _check_decap(e, prefix)
    assert first.max() == 30
    if gamma == 0.15 and N in (3, 16):
        assert sorted(first.tolist())[:2] == [26, 28]
    assert e.last_steps_run == [30]


def test_decap_65_rows_take_the_filtered_head_and_the_split_weight_gemms(decap_engines):
    e = decap_engines(1.5)
    prefix = torch.randn(65, 768, generator=torch.Generator().manual_seed(103))
    first = _check_decap(e, prefix, segs=(1, 4, 30))
    assert first.max() < 30
    e.decode_greedy(prefix, stop_id=ec.DECAP_EOT, seg=1)
    assert e.last_steps_run[0] < 30


def test_decap_chunks_stop_on_their_own():
    e = _decap_engine(0.3, max_prefixes=8)
    try:
        prefix = ec.decap_prefixes(16)
        full = e.decode_greedy(prefix)[0].cpu().numpy()
        ids, _ = e.decode_greedy(prefix, stop_id=ec.DECAP_EOT, seg=1)
        assert np.array_equal(ids.cpu().numpy(), ec.canon_ids(full, [ec.DECAP_EOT]))
        f = ec.DECAP_FIRST[0.3]
        assert e.last_steps_run == [max(f[:8]) + 1, max(f[8:]) + 1]
        with pytest.raises(ValueError):
            e.decode_greedy(prefix, want_logprob=True, stop_id=ec.DECAP_EOT)
    finally:
        e.close()


def test_decap_state_does_not_leak_between_stopping_and_full_length_decodes():
    """A stop decode that ended early, a full-length decode of other prefixes, the stop decode again -- and the reverse order -- on one
    handle each give what a fresh handle gives: the first call of either handle IS the fresh handle's result of the other's second."""
    p1 = ec.decap_prefixes(16)
    p2 = torch.randn(16, 768, generator=torch.Generator().manual_seed(104))
    stop = lambda e: e.decode_greedy(p1, stop_id=ec.DECAP_EOT, seg=4)[0].cpu().numpy()          # noqa: E731
    full = lambda e: e.decode_greedy(p2)[0].cpu().numpy()                                       # noqa: E731
    a, b = _decap_engine(0.3, max_prefixes=16), _decap_engine(0.3, max_prefixes=16)
    try:
        a1 = stop(a)
        assert a.last_steps_run == [20]                       # it ended early: columns 20 .. 29 of the handle's id table are not its own
        a2, a3 = full(a), stop(a)
        b1, b2, b3 = full(b), stop(b), full(b)
    finally:
        a.close()
        b.close()
    assert not np.array_equal(a1, b1)
    assert np.array_equal(a3, a1) and np.array_equal(b2, a1)
    assert np.array_equal(a2, b1) and np.array_equal(b3, b1)


def test_c_abi_refuses_out_of_contract_stop_calls(decap_engines):
    lib, check, ptr = _lib()
    e = decap_engines(1.5)
    x = ec.decap_prefixes(4).cuda()
    out = torch.empty(4, 30, dtype=torch.int32, device="cuda")
    n = ctypes.c_int32(-1)
    assert lib.pio_decode_greedy_stop(e.h, ptr(x), 4, 30, ec.DECAP_EOT, 0, ptr(out), ctypes.byref(n), None) < 0 and b"seg" in lib.pio_last_error()
    assert lib.pio_decode_greedy_stop(e.h, ptr(x), 4, 31, ec.DECAP_EOT, 4, ptr(out), ctypes.byref(n), None) < 0 and b"max_steps" in lib.pio_last_error()
    assert lib.pio_decode_greedy_stop(e.h, ptr(x), 129, 30, ec.DECAP_EOT, 4, ptr(out), ctypes.byref(n), None) < 0 and b"max_prefixes" in lib.pio_last_error()
    assert lib.pio_decode_greedy_stop(e.h, ptr(x), 4, 30, ec.DECAP_EOT, 4, ptr(out), None, None) < 0
    assert lib.pio_decode_greedy_stop(e.h, None, 4, 30, ec.DECAP_EOT, 4, ptr(out), ctypes.byref(n), None) < 0
    check(lib.pio_decode_greedy_stop(e.h, ptr(x), 4, 30, ec.DECAP_EOT, 1000, ptr(out), ctypes.byref(n), None))     # seg >= steps: one segment
    assert n.value == 30


# ---- the engine: ViECap -----------------------------------------------------------------------------------------------------------------
def _viecap_engine(gamma):
    from patchioner_amd.engine import Engine
    c = ec.VIECAP
    w = ec.viecap_case(gamma)[0]
    e = Engine(embed_dim=768, depth=1, num_heads=12, num_registers=4, crop_dim=224, max_batch=2, max_prefixes=16, vit_dtype="fp16",
               dec_layers=c["layers"], dec_heads=12, max_steps=c["Lc"] + max(c["Lt"]) + 63)
    e.load_state_dict(w)
    e.finalize()
    return e


@pytest.fixture(scope="module")
def viecap_engines():
    made = {}

    def get(gamma):
        if gamma not in made:
            made[gamma] = _viecap_engine(gamma)
        return made[gamma]
    yield get
    for e in made.values():
        e.close()


VSEGS = (1, 4, 64)


def _check_viecap(e, cont, tokens, eos):
    full = e.viecap_decode(cont.cuda(), tokens, steps=64).cpu().numpy()
    first = ec.first_stop(full, eos)
    want = ec.canon_ids(full, eos)
    for seg in VSEGS:
        ids = e.viecap_decode(cont.cuda(), tokens, steps=64, stop_ids=eos, seg=seg)
        print("N %d P %d seg %d: first stops %s, steps run %s" % (full.shape[0], 10 + tokens.shape[1], seg, first.tolist(), e.last_steps_run))
        assert np.array_equal(ids.cpu().numpy(), want), "seg %d" % seg
        assert e.last_steps_run == [ec.steps_run(first, 64, seg)], "seg %d" % seg
    return first


@pytest.mark.parametrize("N", [1, 3])
def test_viecap_stops_with_the_ids_of_the_full_decode_at_two_prompt_lengths(viecap_engines, N):
    e = viecap_engines(ec.VIECAP_GAMMA)
    for which in (0, 1, 0):                                   # the prompt length changes from call to call, and comes back
        _, cont, tokens, eos = ec.viecap_case(ec.VIECAP_GAMMA, which, n=N)
        first = _check_viecap(e, cont, tokens, eos)
        assert first.tolist() == ec.VIECAP_FIRST[which][:N]   # the fixture's own columns (margins >= 2.9e-3): _check_viecap saw it end early


@pytest.mark.parametrize("N", [1, 3])
def test_viecap_runs_every_step_while_a_row_has_not_ended(viecap_engines, N):
    e = viecap_engines(0.0)
    _, cont, tokens, eos = ec.viecap_case(0.0, 0, n=N)
    first = _check_viecap(e, cont, tokens, eos)
    assert first.max() == 64 and e.last_steps_run == [64]


def test_viecap_state_does_not_leak_between_stopping_and_full_length_decodes():
    _, c0, t0, eos = ec.viecap_case(ec.VIECAP_GAMMA, 0)
    _, c1, t1, _ = ec.viecap_case(ec.VIECAP_GAMMA, 1)
    stop = lambda e: e.viecap_decode(c0.cuda(), t0, steps=64, stop_ids=eos, seg=4).cpu().numpy()     # noqa: E731
    full = lambda e: e.viecap_decode(c1.cuda(), t1, steps=64).cpu().numpy()                           # noqa: E731
    a, b = _viecap_engine(ec.VIECAP_GAMMA), _viecap_engine(ec.VIECAP_GAMMA)
    try:
        a1 = stop(a)
        assert a.last_steps_run == [12]
        a2, a3 = full(a), stop(a)
        b1, b2, b3 = full(b), stop(b), full(b)
        with pytest.raises(ValueError):
            a.viecap_decode(c0.cuda(), t0, steps=64, stop_ids=[1, 2, 3])
    finally:
        a.close()
        b.close()
    assert np.array_equal(a3, a1) and np.array_equal(b2, a1)
    assert np.array_equal(a2, b1) and np.array_equal(b3, b1)


# ---- the model --------------------------------------------------------------------------------------------------------------------------
def _model(**over):
    from patchioner_amd import Patchioner
    c = gc.E2E
    cfg = {"decap_weights": ec.decap_weights(1.5), "prefix_size": 768, "linear_talk2dino": False, "support_memory_size": c["M"],
           "dino_model": "dinov2_vitb14_reg", "normalize": True, "resize_dim": c["crop"], "crop_dim": c["crop"],
           "dino_weights": W.synth_dinov2(c["seed_vit"], depth=c["depth"]), "memory_bank": W.synth_bank(c["seed_bank"], c["M"]), "max_batch": 4}
    cfg.update(over)
    return Patchioner.from_config(cfg, device="cuda")


def test_model_returns_the_same_strings_in_fewer_steps():
    from patchioner_amd import dist as pdist
    from patchioner_amd import engine as E
    m = _model(stop_at_eos=True, stop_segment=2)
    assert m.stop_at_eos is True and m.stop_segment == 2
    c = gc.E2E
    imgs = W.synth_images(c["seed_img"], c["B"], c["crop"]).cuda()
    traces = gc.e2e_traces()
    calls = {"cls": dict(get_cls_capt=True), "traces": dict(get_cls_capt=False, traces=traces),
             "boxes": dict(get_cls_capt=False, bboxes=None)}
    for name, kw in calls.items():
        res = {}
        for flag in (True, False):
            m.stop_at_eos = flag                                                  # may be toggled after construction
            if name == "boxes":
                kw["bboxes"] = gc.e2e_boxes()
            out = m(imgs.clone(), **kw)
            res[flag] = (out, m.last_ids.cpu().numpy(), m.last_decode_steps)
        (on, ids_on, steps_on), (off, ids_off, steps_off) = res[True], res[False]
        print("%s: steps with the flag %s, without %s" % (name, steps_on, steps_off))
        assert on == off, name
        assert ids_on.shape == ids_off.shape and ids_on.shape[1] == 30
        assert np.array_equal(ids_on, ec.canon_ids(ids_off, [ec.DECAP_EOT])), name
        assert steps_off is None and len(steps_on) == 1 and steps_on[0] < 30, name
    m.stop_at_eos = True
    # compute_scores: the score is exp of the sum of all 30 log-probabilities, so the full decode runs
    caps_on, scores_on = m.caption_tokens(gc.randn(77, 5, 768).cuda(), compute_scores=True)
    assert m.last_decode_steps is None
    m.stop_at_eos = False
    caps_off, scores_off = m.caption_tokens(gc.randn(77, 5, 768).cuda(), compute_scores=True)
    assert caps_on == caps_off and np.array_equal(np.asarray(scores_on), np.asarray(scores_off))
    # the enqueue-only paths run full length and return the same strings
    want = m(imgs.clone(), get_cls_capt=True, traces=traces)
    m.stop_at_eos = True
    got = m.forward_async(imgs.clone(), get_cls_capt=True, traces=traces).result()
    assert got == want and m.last_decode_steps is None
    caps = pdist.sharded_trace_captions(m, imgs.clone(), traces, lambda ids: m.tokenizer.batch_captions(ids))
    assert caps == want["trace_capts"] and m.last_decode_steps is not None and m.last_decode_steps[0] < 30
    # the default segment is the engine's
    m.stop_segment = 7
    assert m(imgs.clone(), get_cls_capt=True)["cls_capt"] == want["cls_capt"] and m.last_decode_steps[0] in (7, 14, 21, 28)
    m.stop_segment = None
    assert m(imgs.clone(), get_cls_capt=True)["cls_capt"] == want["cls_capt"] and m.last_decode_steps[0] % E.DEFAULT_STOP_SEGMENT == 0


def test_viecap_head_stops_with_the_same_captions_and_perplexities():
    from patchioner_amd import Patchioner
    from patchioner_amd import viecap as V
    w, (vocab, merges), ents, emb, x = gc.viecap_case()
    tok = V.ByteLevelBPE(vocab, merges)
    c = gc.VIECAP
    # the fixture's 12-layer weights with the ramp towards "." from position 30 on (the prompts are 24 positions): with ViECapOracle the six
    # rows first stop at columns [16, 18, 13, 16, 11, 15], row 1 alone at 18, at top-2 margins >= 3.0e-3
    w = ec._ramp(dict(w), "gpt.transformer.", ec.viecap_eos(tok)[0], 0.3, start=30)
    w["gpt.lm_head.weight"] = w["gpt.transformer.wte.weight"]
    vcfg = dict(clip_hidden_size=c["C"], weights=w, tokenizer=tok, entities_text=ents, texts_embeddings=emb, temperature=c["temperature"],
                top_k=c["top_k"], threshold=c["threshold"], using_hard_prompt=True, soft_prompt_first=True, using_greedy_search=True)
    cfg = {"decap_weights": None, "prefix_size": 768, "linear_talk2dino": False, "support_memory_size": 0, "dino_model": "dinov2_vitb14_reg",
           "normalize": False, "resize_dim": 224, "crop_dim": 224, "dino_weights": W.synth_dinov2(91, "dinov2_vitb14_reg", depth=1),
           "max_batch": 2, "max_prefixes": 16, "viecap": vcfg, "stop_at_eos": True}
    m = Patchioner.from_config(cfg, device="cuda")
    res = {}
    for flag in (True, False):
        m.stop_at_eos = flag
        many = m.caption_tokens(x.clone().cuda(), compute_scores=True)
        res[flag] = (many, m.last_ids.cpu().numpy(), m.last_decode_steps, m.caption_tokens(x[1:2].clone().cuda()), m.last_decode_steps)
    (on, ids_on, steps_on, one_on, steps1_on), (off, ids_off, steps_off, one_off, steps1_off) = res[True], res[False]
    print("ViECap head: steps with the flag %s / %s, first stops %s" % (steps_on, steps1_on, ec.first_stop(ids_off, m.viecap.eos).tolist()))
    assert on[0] == off[0] and isinstance(one_on, str) and one_on == one_off
    np.testing.assert_array_equal(np.asarray(on[1]), np.asarray(off[1]))          # perplexities: recomputed from the same strings
    assert ids_on.shape == (6, 64) and np.array_equal(ids_on, ec.canon_ids(ids_off, m.viecap.eos))
    assert steps_off is None and steps1_off is None and steps_on[0] < 64 and steps1_on[0] < 64
