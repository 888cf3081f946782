"""ClipCap head, host side: strict config validation, the caption string rule, the float64 statement of the nucleus rule on cases
worked by hand, and the host copy of the Philox generator against the published known-answer vectors."""
import ctypes

import numpy as np
import pytest

import json
import os

import clipcap_case as cc
import clipcap_ref64 as R
from patchioner_amd import clipcap as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clipcap.npz")


@pytest.fixture(scope="module")
def fixture():
    g = np.load(GOLDEN)
    return g, json.loads(bytes(g["meta_json"]).decode())


# ------------------------------------------------------------------------------------------------ config
def test_unknown_key_raises_before_any_device_or_file_access():
    with pytest.raises(NotImplementedError, match="'x'"):
        C.validate_config({"x": 1})
    from patchioner_amd import Patchioner
    base = {"prefix_size": 768, "support_memory_size": 0, "synthetic_seed": 0, "dino_model": "dinov2_vitb14_reg"}
    with pytest.raises(NotImplementedError, match="'beam_width'"):       # no GPU, no weights, no tokenizer were needed to get here
        Patchioner.from_config(dict(base, clipcap={"beam_width": 3, "tokenizer_path": "/nonexistent"}), device="cuda")


def test_transformer_mapper_raises_with_the_reason():
    with pytest.raises(NotImplementedError, match="transformer"):
        C.validate_config({"mapping_type": "transformer"})


def test_missing_tokenizer_path_is_file_not_found(tmp_path):
    with pytest.raises(FileNotFoundError, match="tokenizer_path"):
        C.resolve_tokenizer(C.validate_config({}))
    with pytest.raises(FileNotFoundError, match="tokenizer_path"):
        C.resolve_tokenizer(C.validate_config({"tokenizer_path": str(tmp_path)}))


def test_defaults_are_the_references():
    cfg = C.validate_config({"top_p": 0.5})
    want = {"language_model": "gpt2", "prefix_length": 10, "clip_length": 10, "num_layers": 8, "mapping_type": "mlp", "only_prefix": True,
            "temperature": 1.0, "top_p": 0.5, "entry_length": 67, "stop_token": ".", "use_batched_generation": True, "normalize_prefix": False}
    for k, v in want.items():
        assert cfg[k] == v, k
    assert cfg["seed"] == 0
    for k in ("hf_repo_id", "weight_path_hf_repo_id", "seed", "tokenizer", "tokenizer_path", "weights"):
        C.validate_config({k: None})


# ------------------------------------------------------------------------------------------------ strings
class _Tok:
    """ids index a fixed table of strings"""
    table = ["a", " cat", ".", " on", " Mr.", " mat", "!"]

    def decode(self, ids):
        return "".join(self.table[i] for i in ids)

    def encode(self, s):
        return [self.table.index(s)]


def test_caption_strings():
    t = _Tok()
    # the stop token itself; ids after it (the frozen row's stop ids) do not show
    assert C.captions_from_ids(t, [[0, 1, 2, 2, 2]], ".") == ["a cat."]
    # a stop CHARACTER inside an earlier token cuts there
    assert C.captions_from_ids(t, [[0, 4, 1, 2]], ".") == ["a Mr."]
    # a row that never stops still gets the stop token appended
    assert C.captions_from_ids(t, [[0, 1, 3, 5]], ".") == ["a cat on mat."]
    # entry_length 0
    assert C.captions_from_ids(t, [[]], ".") == [""]
    assert C.cut_caption("", ".") == "."


def test_caption_strings_match_the_reference_fixture(fixture):
    """The reference's own cut strings (generate_batched on the stub tokenizer) from the ids it sampled: all entry_length ids of a row,
    as the reference decodes them (it keeps sampling a stopped row), and the device's form of the same rows (stop_id from the stop on)."""
    g, meta = fixture
    tok = cc.StubTokenizer(meta["stop_id"], meta["stop_token"])
    some_stop = some_run_on = False
    for ids, caps in ((g["greedy_ids"], meta["greedy_captions"]), (g["sampled0_ids"], meta["sampled0_captions"]),
                      (g["sampled1_ids"], meta["sampled1_captions"])):
        assert C.captions_from_ids(tok, ids.tolist(), meta["stop_token"]) == caps
        dev = ids.copy()
        for r in range(dev.shape[0]):
            hit = np.nonzero(dev[r] == meta["stop_id"])[0]
            if hit.size:
                dev[r, hit[0]:] = meta["stop_id"]
                some_stop = True
            else:
                some_run_on = True
        assert C.captions_from_ids(tok, dev.tolist(), meta["stop_token"]) == caps
    assert some_stop and some_run_on                     # a row that stops before the end and a row that never stops are both in there


# ------------------------------------------------------------------------------------------------ float64 statement
def test_ref64_reproduces_the_reference_fixture(fixture):
    """Ties tests/clipcap_ref64.py to the reference: from the temperature-scaled logits the reference sorted (their top 384 and the
    row's log-sum-exp, i.e. the exact probabilities of the head of the row) and the recorded uniforms, the statement gives the
    reference's kept-set size and its chosen id at every sampled (row, step) of both runs."""
    g, meta = fixture
    checked = 0
    for k in range(2):
        ids, kept, u = g["sampled%d_ids" % k], g["sampled%d_kept" % k], g["uniforms"][k]
        for r in range(ids.shape[0]):
            for t in range(ids.shape[1]):
                if kept[r, t] == 0:                      # the row had stopped: the reference samples it unfiltered, nothing to compare
                    continue
                x = g["sampled%d_top_logits" % k][r, t].astype(np.float64)
                tid = g["sampled%d_top_ids" % k][r, t]
                p = np.exp(x - g["sampled%d_lse" % k][r, t])
                km, _, _ = R.nucleus_p(x, p, meta["case"]["top_p"])
                assert km.sum() == kept[r, t] < x.shape[0], (k, r, t)
                order = np.argsort(tid)                  # the draw walks ascending token ids
                j, _, _ = R.draw(km[order], p[order], float(u[r, t]))
                assert tid[order][j] == ids[r, t], (k, r, t)
                checked += 1
    assert checked > 40


def test_ref64_nucleus_by_hand():
    # p = (0.5, 0.25, 0.125, 0.125): masses before the sorted positions: 0, 0.5, 0.75, 0.875
    s = np.log(np.array([0.125, 0.5, 0.125, 0.25]))
    kept, p, _ = R.nucleus(s, 1.0, 0.8)
    assert kept.tolist() == [True, True, True, True]     # ties at the edge: both 0.125 tokens share mass-before 0.75
    kept, p, gap = R.nucleus(s, 1.0, 0.6)
    assert kept.tolist() == [False, True, False, True] and abs(gap - 0.1) < 1e-12
    kept, _, _ = R.nucleus(s, 1.0, 0.0)
    assert kept.tolist() == [False, True, False, False]
    kept, _, _ = R.nucleus(s, 1.0, 1.0)
    assert kept.all()
    # the draw walks the kept ids in ascending id order: kept = {1: 0.5, 3: 0.25} -> CDF 2/3, 1
    kept, p, _ = R.nucleus(s, 1.0, 0.6)
    assert R.draw(kept, p, 0.0)[0] == 1 and R.draw(kept, p, 0.66)[0] == 1 and R.draw(kept, p, 0.67)[0] == 3
    assert R.draw(kept, p, np.float32(1.0) - np.float32(2.0 ** -24))[0] == 3
    # temperature sharpens: at T = 0.5 p ~ (1, 16, 1, 4) / 22: mass before the third sorted position is 20 / 22 > 0.8
    kept, _, _ = R.nucleus(s, 0.5, 0.8)
    assert kept.tolist() == [False, True, False, True]


# ------------------------------------------------------------------------------------------------ Philox
@pytest.fixture(scope="module")
def lib():
    from patchioner_amd import build
    build.build()
    from patchioner_amd import _lib
    return _lib.load()


def _philox(lib, ctr, key):
    c = (ctypes.c_uint32 * 4)(*ctr)
    o = (ctypes.c_uint32 * 4)()
    assert lib.pio_host_philox4x32(c, key[0], key[1], o) == 0
    return [int(v) for v in o]


def test_philox_known_answers(lib):
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    assert _philox(lib, [0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = 0xffffffff
    assert _philox(lib, [f, f, f, f], [f, f]) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert _philox(lib, [0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_philox_uniform_is_the_first_word_and_inside_the_unit_interval(lib):
    u = ctypes.c_float()
    seed = 0x0123456789abcdef
    for row, step in [(0, 0), (3, 7), (127, 66)]:
        assert lib.pio_host_philox_uniform(seed, row, step, ctypes.byref(u)) == 0
        w0 = _philox(lib, [row, step, 0, 0], [seed & 0xffffffff, seed >> 32])[0]
        assert u.value == (w0 >> 8) * 2.0 ** -24
        assert 0.0 <= u.value < 1.0
    # the largest value the construction can give is still below 1 in fp32
    assert np.float32((2 ** 24 - 1) * 2.0 ** -24) < np.float32(1.0)
