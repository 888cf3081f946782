"""Eviction in the two bounded graph caches of a handle (api.cpp, GraphCache) on the real runtime: more prompted decodes than the 12 graphs
the prompted cache holds, more stop decodes than the 8 the stop cache holds, then an evicted key again (recaptured) and a resident one.

The case is tests/eos_case.py's ViECap one (2 GPT-2 layers) at the smallest shapes that cross both bounds: 2 rows, 4 steps, and the key
changed through the prompt length alone -- hard-prompt rows of 14 seeded tokens cut to their first Lt.  gamma 0 (no row ends) for the
full-length decodes, eos_case.VIECAP_GAMMA for the stopping ones: its ramp towards "." starts at position 13, so the short prompts run all
4 steps and the long ones end after the first segment."""
import numpy as np
import pytest
import torch

import eos_case as ec

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

N, STEPS, LT_MAX, SEG = 2, 4, 14, 2


def _engine(gamma):
    """test_gpu_stop_at_eos.py's _viecap_engine"""
    from patchioner_amd.engine import Engine
    c = ec.VIECAP
    e = Engine(embed_dim=768, depth=1, num_heads=12, num_registers=4, crop_dim=224, max_batch=2, max_prefixes=16, vit_dtype="fp16",
               dec_layers=c["layers"], dec_heads=12, max_steps=c["Lc"] + max(c["Lt"]) + 63)
    e.load_state_dict(ec.viecap_case(gamma)[0])
    e.finalize()
    return e


def _inputs(gamma):
    _, cont, _, eos = ec.viecap_case(gamma, 0, n=N)
    tokens = torch.randint(0, len(ec.viecap_tokenizer()), (N, LT_MAX), generator=torch.Generator().manual_seed(313)).to(torch.int32)
    return cont.cuda(), tokens, eos


def test_prompted_graphs_are_evicted_and_recaptured_with_the_same_ids(monkeypatch):
    """Lt = 1 .. 14 are 14 keys in a cache of 12: by the time Lt = 14 is captured, Lt = 1 and 2 are gone.  Lt = 1 again is a fresh capture
    that evicts another graph, Lt = 14 is still resident; both give the ids of their first run bit for bit, and all 14 are the ids of an
    engine that launches the same kernels without graphs (PIO_NO_GRAPH=1 when the handle is created)."""
    cont, tokens, _ = _inputs(0.0)
    decode = lambda e, Lt: e.viecap_decode(cont, tokens[:, :Lt].contiguous(), steps=STEPS).cpu().numpy()      # noqa: E731
    e = _engine(0.0)
    try:
        first = {Lt: decode(e, Lt) for Lt in range(1, LT_MAX + 1)}
        again_1, again_14 = decode(e, 1), decode(e, LT_MAX)
    finally:
        e.close()
    assert all(ids.shape == (N, STEPS) for ids in first.values())
    assert len({ids.tobytes() for ids in first.values()}) > 1                 # the prompt length does change the decode
    assert np.array_equal(again_1, first[1]) and np.array_equal(again_14, first[LT_MAX])
    monkeypatch.setenv("PIO_NO_GRAPH", "1")
    eager = _engine(0.0)
    monkeypatch.delenv("PIO_NO_GRAPH")
    try:
        for Lt in range(1, LT_MAX + 1):
            assert np.array_equal(decode(eager, Lt), first[Lt]), "Lt %d" % Lt
    finally:
        eager.close()


def test_stop_decodes_are_evicted_and_recaptured_with_the_canonical_ids():
    """Nine prompt lengths are 9 decodes in a cache of 8 (their full-length references go to the prompted cache): the ninth evicts the
    first, which then runs again.  Every time: ids == canon(full decode), steps run as eos_case.steps_run says.  With the oracle's GPT-2
    (eos_case.viecap_oracle_ids) the prompts up to Lt = 8 run all 4 steps and those from Lt = 10 on end after the first segment, at top-2
    margins of 1.3e-2 and more."""
    cont, tokens, eos = _inputs(ec.VIECAP_GAMMA)
    lengths = [1, 2, 3, 4, 6, 8, 10, 12, 14]
    e = _engine(ec.VIECAP_GAMMA)
    ran = []
    try:
        for Lt in lengths + lengths[:1]:
            tok = tokens[:, :Lt].contiguous()
            full = e.viecap_decode(cont, tok, steps=STEPS).cpu().numpy()
            ids = e.viecap_decode(cont, tok, steps=STEPS, stop_ids=eos, seg=SEG).cpu().numpy()
            first = ec.first_stop(full, eos)
            print("Lt %d: first stops %s, steps run %s" % (Lt, first.tolist(), e.last_steps_run))
            assert np.array_equal(ids, ec.canon_ids(full, eos)), "Lt %d" % Lt
            assert e.last_steps_run == [ec.steps_run(first, STEPS, SEG)], "Lt %d" % Lt
            ran.append(e.last_steps_run[0])
    finally:
        e.close()
    assert ran[0] == ran[-1]
    assert set(ran) == {SEG, STEPS}, ran            # some decodes ended after their first segment, some ran both
