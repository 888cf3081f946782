"""The hard prompt as device-composable fragments (viecap.PromptFragments): the table k_compose_prompts reads reproduces the
tokenizer on every ordered choice of up to top_k entities, and a tokenizer under which an entity does not decompose is caught."""
import itertools
import random
import time

import pytest

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
    """api.cpp references the launchers of the device hard prompt and of the ragged decode weakly (its host-only AddressSanitizer build links
    without the kernels); the library itself must define them, with these signatures."""
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
