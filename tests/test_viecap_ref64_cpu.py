"""The float64 references of tests/viecap_ref64.py against the REFERENCE's own fp32 outputs (tests/golden/viecap.npz), so that the
GPU tests that hold the kernels to them hold the kernels to the right function.  The bars are the golden case's (fp32 reference
against an exact evaluation)."""
import json

import numpy as np
import torch

import golden_cases as gc
import viecap_ref64 as R
from patchioner_amd import viecap as V


def test_float64_references_reproduce_the_reference_fixture(golden):
    g = golden("viecap")
    meta = json.loads(bytes(g["meta_json"]).decode())
    w, (vocab, merges), ents, emb, x = gc.viecap_case()
    c = gc.VIECAP
    np.testing.assert_allclose(R.mapping64(w, x).numpy(), g["cont"], rtol=2e-4, atol=5e-5)
    p, logp = R.entity_probs64(x, emb, c["temperature"])
    np.testing.assert_allclose(p.numpy(), g["entity_probs"], rtol=2e-4, atol=1e-6)
    assert torch.allclose(logp.exp(), p)
    tok = V.ByteLevelBPE(vocab, merges)
    rows = [tok.encode(s) for s in meta["perplexity_sentences"]]
    nll, amax = R.gpt2_nll64(w, rows)
    ppl = [float(torch.exp(nll[i] / (len(r) - 1))) if len(r) > 1 else float("nan") for i, r in enumerate(rows)]
    np.testing.assert_allclose(ppl, g["perplexity"], rtol=5e-4)
    assert bool((amax[[len(r) > 1 for r in rows]] > 0).all())
    # the hard prompts the reference built select the entities select_reference selects (the fixture's threshold is 0.4)
    for i in range(x.shape[0]):
        picks = R.select_reference(torch.from_numpy(g["entity_probs"][i]), c["top_k"], c["threshold"])
        want = tok.encode(V.compose_discrete_prompt_text([ents[j] for j in picks]))
        assert g["prompt_tokens"][i][:len(want)].tolist() == want


def test_float64_greedy_search_follows_the_reference_ids(golden):
    """gpt2_greedy64 on the reference's own prompt (its soft prompt and hard-prompt ids): its ids equal the reference's up to the
    reference's end of sentence, or depart at a near-tie of the float64 margins."""
    g = golden("viecap")
    w, _, _, _, _ = gc.viecap_case()
    m = R.GPT2_64(w)
    emb = torch.cat([torch.from_numpy(g["cont"]).double(), m.wte[torch.from_numpy(g["prompt_tokens"]).long()]], dim=1)
    ids, margins, amax = R.gpt2_greedy64(w, emb, 64, model=m)
    ref = torch.from_numpy(g["decoded_ids"]).long()
    assert bool((amax > 0).all())
    for r in range(ref.shape[0]):
        n = int((ref[r] >= 0).sum())
        diff = (ids[r, :n] != ref[r, :n]).nonzero()
        if len(diff):
            t = int(diff[0])
            assert float(margins[r, t]) <= 1e-3, (r, t, float(margins[r, t]))
