"""The hard prompt as device-composable fragments (viecap.PromptFragments): the table k_compose_prompts reads reproduces the
tokenizer on every ordered choice of up to top_k entities, and a tokenizer under which an entity does not decompose is caught."""
import itertools
import random
import time

import numpy as np
import pytest
import torch

from patchioner_amd import weights as W
from patchioner_amd.viecap import ByteLevelBPE, PromptFragments, compose_discrete_prompt_text


def _bpe(seed=0):
    vocab, merges = W.synth_bpe(seed)
    return ByteLevelBPE(vocab, merges)


def _every_order(tok, ents, top_k):
    frag = PromptFragments(tok, ents, top_k)
    assert frag.bad == [] and frag.empty_ok
    frag.check()
    longest = len(frag.row([]))
    assert frag.row([]) == tok.encode(compose_discrete_prompt_text([]))
    for k in range(1, top_k + 1):
        for picks in itertools.permutations(range(len(ents)), k):
            want = tok.encode(compose_discrete_prompt_text([ents[i] for i in picks]))
            assert frag.row(list(picks)) == want, [ents[i] for i in picks]
            longest = max(longest, len(want))
    assert frag.Lmax >= longest
    return frag


def test_fragments_reproduce_the_synthetic_bpe_on_every_order_of_up_to_three_entities():
    frag = _every_order(_bpe(0), list(W.SYNTH_ENTITIES), 3)
    # Lmax is exactly the bound the table states: the longest middle fragment twice, then the longest last fragment
    mids = [frag.length_host[2 * e] for e in range(len(W.SYNTH_ENTITIES))]
    lasts = [frag.length_host[2 * e + 1] for e in range(len(W.SYNTH_ENTITIES))]
    assert frag.Lmax == max(frag.head_len + 2 * max(mids) + max(lasts), frag.empty_len)


def test_fragments_reproduce_another_learnt_vocabulary():
    """The ViECap fixture (golden_cases.viecap_case) uses the tokenizer and entities above; a vocabulary learnt from another seed has other
    merges, so other fragment boundaries inside the words."""
    vocab0, _ = W.synth_bpe(0)
    vocab, merges = W.synth_bpe(5, merges=250)
    assert vocab != vocab0
    _every_order(ByteLevelBPE(vocab, merges), list(W.SYNTH_ENTITIES), 3)


def test_lmax_for_top_k_one_and_eight():
    tok, ents = _bpe(0), list(W.SYNTH_ENTITIES)
    one, eight = PromptFragments(tok, ents, 1), PromptFragments(tok, ents, 8)
    assert one.Lmax == max(one.head_len + max(one.length_host[1::2]), one.empty_len)
    assert eight.Lmax == eight.head_len + 7 * max(eight.length_host[0::2]) + max(eight.length_host[1::2])
    rng = random.Random(3)
    for _ in range(200):
        picks = rng.sample(range(len(ents)), 8)
        want = tok.encode(compose_discrete_prompt_text([ents[i] for i in picks]))
        assert eight.row(picks) == want and len(want) <= eight.Lmax


class _MergesKiteComma:
    """A tokenizer under which "kite" does not decompose: "kite, " becomes one unit, so the comma of its middle fragment takes the
    next entity's leading space with it."""

    def __init__(self, base):
        self.base, self.pad_token_id = base, None

    def encode(self, text):
        return self.base.encode(text.replace("kite, ", "kite\x01"))

    def decode(self, ids):
        return self.base.decode(ids)


def test_an_entity_that_does_not_decompose_is_named():
    ents = list(W.SYNTH_ENTITIES)
    frag = PromptFragments(_MergesKiteComma(_bpe(0)), ents, 3)
    assert frag.bad == ["kite"]
    with pytest.raises(ValueError, match="'kite'"):
        frag.check()


def test_the_check_is_fast_on_thousands_of_entities():
    rng = random.Random(7)
    letters = "abcdefghijklmnopqrstuvwxyz"
    ents = sorted({" ".join("".join(rng.choice(letters) for _ in range(rng.randint(3, 9))) for _ in range(rng.randint(1, 3)))
                   for _ in range(6000)})
    tok = _bpe(0)
    t = time.perf_counter()
    frag = PromptFragments(tok, ents, 3)
    dt = time.perf_counter() - t
    assert frag.bad == []
    assert dt < 3.0, "fragment table of %d entities took %.2f s" % (len(ents), dt)    # ~0.2 s on an idle host; the bound leaves room for a busy one
    for picks in ([0], [5, 17], [len(ents) - 1, 3, 999]):
        assert frag.row(picks) == tok.encode(compose_discrete_prompt_text([ents[i] for i in picks]))


def test_the_library_defines_the_device_prompt_launchers():
    """The library defines the launchers of the device hard prompt and of the ragged decode with the signatures that api.cpp and the host-only
    AddressSanitizer build's stubs (tests/hipstub/hip_stub.cpp) declare: a changed signature shows here by its mangled name."""
    import ctypes
    import os
    from patchioner_amd import build
    if not os.path.exists(build.LIB):
        pytest.skip("library not built")
    lib = ctypes.CDLL(build.LIB)
    for sym in ("_ZN3pio22launch_compose_promptsERKNS_11ComposeArgsEP12ihipStream_t",
                "_ZN3pio26launch_build_prompt_raggedEPKfPKiS3_S1_iiiiiiPfPiP12ihipStream_t",
                "_ZN3pio29launch_decode_prompted_raggedERKNS_11DecoderArgsEPKfiPKiiP12ihipStream_t"):
        assert getattr(lib, sym) is not None


# ------------------------------------------------------------------------------------------------ top_k_entities at its edges
# The host selection (viecap.top_k_entities, forward()'s path) against viecap_ref64.select_reference, the documented order written out
# as a sort key: NaN first, larger first, equal values by the lower index; cut at the first value below the threshold in fp32.  The
# device (k_compose_prompts) is held to the same reference in tests/test_gpu_viecap_kernels.py, so forward() and the device path pick
# the same entities.
def _names(K):
    return ["e%d" % i for i in range(K)]


def _host_vs_reference(row, top_k, threshold):
    from patchioner_amd.viecap import top_k_entities
    from viecap_ref64 import select_reference
    row = torch.as_tensor(row, dtype=torch.float32)
    names = _names(row.numel())
    want = [names[i] for i in select_reference(row, top_k, threshold)]
    got = top_k_entities(names, row, top_k, threshold)
    assert got == want, (row.tolist()[:12], top_k, threshold)
    return [int(n[1:]) for n in got]


nan = float("nan")


def test_select_reference_states_the_documented_order():
    """The reference itself, on hand-checked rows (so that host and device are not only held to each other)."""
    from viecap_ref64 import select_reference
    assert select_reference([0.1, nan, 0.3, 0.3, nan, 0.7], 4, 0.0) == [1, 4, 5, 2]
    assert select_reference([0.3, 0.3, 0.3], 2, 0.3) == [0, 1]
    assert select_reference([0.2, 0.5], 2, 0.3) == [1]
    assert select_reference([float(np.float32(0.7))], 1, 0.7) == [0]          # fp32(0.7) < 0.7 in float64, not in fp32
    assert select_reference([float(np.float32(0.2))], 1, 0.2) == [0]          # fp32(0.2) > 0.2: kept in both precisions
    assert select_reference([float(np.nextafter(np.float32(0.2), np.float32(0)))], 1, 0.2) == []     # the fp32 value below it: cut
    assert select_reference([nan, nan], 3, 0.9) == [0, 1]


def test_top_k_entities_orders_exact_ties_by_the_lower_index():
    # torch.topk (CPU) returns [1, 4, 5, 3] here: index 3 before index 2 of two equal values
    assert _host_vs_reference([0.1, nan, 0.3, 0.3, nan, 0.7], 4, 0.0) == [1, 4, 5, 2]
    assert _host_vs_reference([0.1, 0.3, 0.3, 0.2, 0.3], 3, 0.2) == [1, 2, 4]
    flat = torch.full((300,), 1.0 / 300)
    assert _host_vs_reference(flat, 8, 0.0) == list(range(8))
    assert _host_vs_reference(flat, 8, 1.0 / 300) == list(range(8))          # equal to fp32(1/300) after both round: kept
    assert _host_vs_reference(flat, 8, 0.2) == []
    two_levels = torch.full((300,), 0.001)
    two_levels[[299, 150, 7, 42]] = 0.25
    assert _host_vs_reference(two_levels, 8, 0.001) == [7, 42, 150, 299, 0, 1, 2, 3]


def test_top_k_entities_puts_nan_first_and_keeps_it():
    assert _host_vs_reference([0.5, nan, 0.2, nan], 3, 0.4) == [1, 3, 0]
    assert _host_vs_reference(torch.full((40,), nan), 8, 0.2) == list(range(8))
    assert _host_vs_reference([nan], 3, 0.99) == [0]


@pytest.mark.parametrize("threshold", [0.2, 0.4, 0.35, 0.45, 0.7])
def test_top_k_entities_cuts_in_fp32(threshold):
    """A probability equal to float32(threshold) is kept: the reference compares its fp32 tensor with the Python float in fp32.  For
    0.35, 0.45 and 0.7 fp32 rounds the threshold down, so a float64 compare (the old host path) dropped the entity."""
    t32 = float(np.float32(threshold))
    below = float(np.nextafter(np.float32(threshold), np.float32(0)))
    row = [0.01, t32, below, 0.0]
    assert _host_vs_reference(row, 3, threshold) == [1]
    row = [below, 0.9 if threshold < 0.9 else 0.95, t32, t32]
    assert _host_vs_reference(row, 4, threshold) == [1, 2, 3]


def test_top_k_entities_threshold_zero_and_top_k_above_k():
    assert _host_vs_reference([0.0, 0.5, 0.0, 0.5], 3, 0.0) == [1, 3, 0]
    assert _host_vs_reference([0.0, -0.0, 1e-45], 2, 0.0) == [2, 0]
    assert _host_vs_reference([0.2, 0.6, 0.2], 8, 0.0) == [1, 0, 2]
    assert _host_vs_reference([0.2, 0.6, 0.2], 8, 0.3) == [1]


def test_top_k_entities_matches_the_reference_on_random_tied_rows():
    """Rows drawn from a few levels (many exact ties) with NaNs sprinkled in; thresholds taken from the row's own values, so the cut
    often falls on an equality."""
    g = torch.Generator().manual_seed(11)
    for _ in range(400):
        K = int(torch.randint(1, 70, (1,), generator=g))
        levels = torch.tensor([0.0, 0.05, 0.2, 0.35, 0.4, 0.45, 0.7, nan], dtype=torch.float32)
        row = levels[torch.randint(0, 8 if torch.rand(1, generator=g) < 0.3 else 7, (K,), generator=g)]
        top_k = int(torch.randint(1, 10, (1,), generator=g))
        threshold = [0.0, 0.2, 0.35, 0.4, 0.45, 0.7][int(torch.randint(0, 6, (1,), generator=g))]
        _host_vs_reference(row, top_k, threshold)
