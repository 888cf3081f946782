"""stop_at_eos without a GPU: the EOS-emitting fixtures against the oracle, the canonical id table against the host's own cuts, the
constructor's new keywords and the new C-ABI symbols."""
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import eos_case as ec
from patchioner_amd import viecap as V
from patchioner_amd import weights as W
from patchioner_amd.tokenizer import ClipDetokenizer

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_MARGIN = 5e-4          # the decoder's fixtures are decoded bit-exactly at 1.9e-4


@pytest.fixture(scope="module")
def O():
    from oracle import patchioner_oracle
    return patchioner_oracle


def _min_margin_to_stop(margins, first):
    return min(float(margins[r, :min(margins.shape[1], int(f) + 1)].min()) for r, f in enumerate(first))


@pytest.mark.parametrize("gamma", [0.3, 1.5, 0.15])
def test_decap_fixture_stops_where_the_table_says(O, gamma):
    orc = O.DeCapOracle(ec.decap_weights(gamma), n_head=4)
    orc.fast = True
    ids, _, margins = orc.decode_ids(ec.decap_prefixes(), ec.DECAP_STEPS)
    first = ec.first_stop(ids.numpy(), [ec.DECAP_EOT])
    print("gamma %.2f: first end-of-text columns %s, min margin up to the stop %.3e" % (gamma, first.tolist(), _min_margin_to_stop(margins, first)))
    assert first.tolist() == ec.DECAP_FIRST[gamma]
    assert _min_margin_to_stop(margins, first) >= MIN_MARGIN


def test_plain_weights_never_stop(O):
    orc = O.DeCapOracle(ec.decap_weights(0.0), n_head=4)
    orc.fast = True
    ids = orc.decode_ids(ec.decap_prefixes(), ec.DECAP_STEPS)[0]
    assert ec.first_stop(ids.numpy(), [ec.DECAP_EOT]).tolist() == [30] * 16


@pytest.mark.parametrize("which", [0, 1])
def test_viecap_fixture_stops_at_distinct_columns_before_40(O, which):
    w, cont, tokens, eos = ec.viecap_case(ec.VIECAP_GAMMA, which)
    gpt = O.DeCapOracle({("decoder." + k[4:]): v for k, v in w.items() if k.startswith("gpt.")}, n_head=12)
    ids, margins = ec.viecap_oracle_ids(gpt, cont, tokens)
    first = ec.first_stop(ids.numpy(), eos)
    print("prompt %d: first full-stop columns %s, min margin up to the stop %.3e" % (which, first.tolist(), _min_margin_to_stop(margins, first)))
    assert first.tolist() == ec.VIECAP_FIRST[which]
    assert len(set(first.tolist())) >= 2 and first.max() < 40
    assert _min_margin_to_stop(margins, first) >= MIN_MARGIN


def test_first_stop_canon_and_steps_run_on_a_constructed_table():
    ids = np.array([[5, 9, 7, 9, 1], [1, 2, 3, 4, 5], [9, 1, 1, 1, 1], [1, 1, 1, 1, 8], [3, 8, 9, 2, 2]])
    assert ec.first_stop(ids, [9, 8]).tolist() == [1, 5, 0, 4, 1]
    want = np.array([[5, 9, 9, 9, 9], [1, 2, 3, 4, 5], [9, 9, 9, 9, 9], [1, 1, 1, 1, 8], [3, 8, 8, 8, 8]])
    assert np.array_equal(ec.canon_ids(ids, [9, 8]), want)
    assert np.array_equal(ec.canon_ids(want, [9, 8]), want)                      # idempotent
    assert [ec.steps_run(ec.DECAP_FIRST[0.3], 30, s) for s in (1, 4, 7, 30)] == [19, 20, 21, 30]
    assert ec.steps_run(ec.DECAP_FIRST[0.15], 30, 4) == 30
    assert ec.steps_run([28], 30, 4) == 30 and ec.steps_run([0], 30, 4) == 4 and ec.steps_run([3], 30, 4) == 4 and ec.steps_run([4], 30, 4) == 8


def _random_tables(stops, vocab, steps, seed):
    """id tables [8, steps]: rows with a stop id in column 0, in the last column, twice, with both stop ids, and with none."""
    g = np.random.default_rng(seed)
    plain = [t for t in range(vocab) if t not in stops]
    ids = g.choice(plain, size=(8, steps))
    ids[0, 0] = stops[0]
    ids[1, steps - 1] = stops[-1]
    ids[2, 3] = ids[2, 9] = stops[0]
    ids[3, 5], ids[3, 4] = stops[0], stops[-1]
    ids[4, 11] = stops[-1]
    ids[5, 1:] = stops[0]
    return ids                                                                     # rows 6, 7: no stop


def test_canon_keeps_every_decap_caption():
    tok = ClipDetokenizer()
    assert tok.eot_id == ec.DECAP_EOT
    ids = _random_tables([ec.DECAP_EOT], 49406, 30, 5)
    full = tok.batch_captions(ids.tolist())
    assert full is not None and len(set(full)) > 1
    assert tok.batch_captions(ec.canon_ids(ids, [ec.DECAP_EOT]).tolist()) == full
    assert tok.batch_captions(ec.canon_ids(ids, [ec.DECAP_EOT]).tolist(), return_start_end_tokens=True) == \
        tok.batch_captions(ids.tolist(), return_start_end_tokens=True)


def test_canon_keeps_every_viecap_caption_and_the_single_row_str():
    tok = ec.viecap_tokenizer()
    eos = ec.viecap_eos(tok)
    head = SimpleNamespace(tokenizer=tok, eos=eos)
    ids = _random_tables(eos, len(tok), 64, 6)
    full = V.VieCapHead.captions(head, ids.tolist())
    assert isinstance(full, list) and V.VieCapHead.captions(head, ec.canon_ids(ids, eos).tolist()) == full
    for r in range(ids.shape[0]):                                                  # one row: a str, cut at the first full stop or not at all
        one = V.VieCapHead.captions(head, ids[r:r + 1].tolist())
        assert isinstance(one, str) and V.VieCapHead.captions(head, ec.canon_ids(ids[r:r + 1], eos).tolist()) == one


def _cfg(**over):
    cfg = {"decap_weights": W.synth_decap(1, n_layer=1), "prefix_size": 768, "linear_talk2dino": False, "support_memory_size": 0,
           "dino_model": "dinov2_vitb14_reg", "normalize": False, "resize_dim": 224, "crop_dim": 224,
           "dino_weights": W.synth_dinov2(91, "dinov2_vitb14_reg", depth=1), "max_batch": 2, "max_prefixes": 16}
    cfg.update(over)
    return cfg


def test_constructor_and_from_config_take_the_keys_and_reach_the_device_check():
    """Without the feature: TypeError (nn.Module.__init__ got an unexpected keyword)."""
    from patchioner_amd import Patchioner
    with pytest.raises(RuntimeError, match="MI355X"):
        Patchioner.from_config(_cfg(stop_at_eos=True, stop_segment=4), device="cpu")
    with pytest.raises(RuntimeError, match="MI355X"):
        Patchioner.from_config(_cfg(), device="cpu")
    c = _cfg()
    with pytest.raises(RuntimeError, match="MI355X"):
        Patchioner(decoder_weights=c["decap_weights"], device="cpu", prefix_size=768, linear_talk2dino=False, support_memory_size=0,
                   dino_model=c["dino_model"], dino_weights=c["dino_weights"], resize_dim=224, crop_dim=224, stop_at_eos=True, stop_segment=7)


def test_engine_argument_helpers():
    from patchioner_amd import engine as E
    assert E.DEFAULT_STOP_SEGMENT == 2                    # the measured segment table's choice
    assert E._stop_ids(None, 2) is None and E._stop_ids([13], 2) == [13, -1] and E._stop_ids([13, 764], 2) == [13, 764]
    for bad in ([], [1, 2, 3], [-1]):
        with pytest.raises(ValueError):
            E._stop_ids(bad, 2)
    with pytest.raises(ValueError):
        E._stop_ids([1, 2], 1)
    assert E._stop_seg(None) == 2 and E._stop_seg(30) == 30
    with pytest.raises(ValueError):
        E._stop_seg(0)


NEW = ["pio_decode_greedy_stop", "pio_viecap_decode_stop", "pio_test_dec_stop_scan", "pio_test_dec_stop_pad"]


def test_new_symbols_in_header_signatures_and_library():
    from patchioner_amd import _lib, build
    build.build()
    with open(os.path.join(ROOT, "include", "patchioner_hip.h")) as f:
        header = f.read()
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "patchioner_amd", "libpatchioner_hip.so")],
                          capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\b" % name, syms), name
    assert len(_lib.SIGNATURES["pio_decode_greedy_stop"][1]) == 9
    assert len(_lib.SIGNATURES["pio_viecap_decode_stop"][1]) == 13
