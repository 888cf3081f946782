"""The seeded ClipCap case shared by tools/oracle/gen_golden_clipcap.py (which runs the reference on it) and the tests that read
tests/golden/clipcap.npz: weights, features and the stub tokenizer.  Only seeds and sizes live here; the weights are regenerated."""
import re

import torch

CASE = {"C": 768, "gpt_layers": 2, "weights_seed": 31, "features_seed": 32, "N": 4, "entry_length": 12, "prefix_length": 10,
        "head_scale": 8.0, "wpe_scale": 100.0, "top_p": 0.8, "temperatures": (1.0, 0.7), "top_k_recorded": 384}


def weights():
    """synth_clipcap with the tied embedding scaled up: random 0.02-std embeddings give logits of spread ~0.5, a nucleus of ~40 000
    tokens of ~2e-5 mass each, where every row is a boundary case; x 8 gives spread ~4, nuclei of a few to a few hundred tokens.  The
    position table is scaled further, so that a token's own embedding does not dominate the residual stream: with a tied head it
    would predict itself with mass ~1 and every nucleus would hold one token."""
    from patchioner_amd import weights as W
    sd = W.synth_clipcap(CASE["weights_seed"], C=CASE["C"], prefix_length=CASE["prefix_length"], n_layer=CASE["gpt_layers"])
    wte = sd["gpt.transformer.wte.weight"] * CASE["head_scale"]
    sd["gpt.transformer.wte.weight"] = wte
    sd["gpt.lm_head.weight"] = wte
    sd["gpt.transformer.wpe.weight"] = sd["gpt.transformer.wpe.weight"] * CASE["wpe_scale"]
    return sd


def features():
    return torch.randn(CASE["N"], CASE["C"], generator=torch.Generator().manual_seed(CASE["features_seed"]))


class StubTokenizer:
    """Token i is the string ' w<i>', except ``stop_id``, which is ``stop_token``.  ``encode`` inverts ``decode``; with
    ``return_tensors='pt'`` it gives the [1, L] tensor the reference's scoring asks for."""
    pad_token_id = None
    eos_token_id = 50256

    def __init__(self, stop_id: int, stop_token: str = "."):
        self.stop_id, self.stop_token = int(stop_id), stop_token

    def decode(self, ids):
        return "".join(self.stop_token if int(i) == self.stop_id else " w%d" % int(i) for i in ids)

    def encode(self, text, return_tensors=None):
        ids = [self.stop_id if m.group(1) is None else int(m.group(1)) for m in re.finditer(r" w(\d+)|" + re.escape(self.stop_token), text)]
        if return_tensors == "pt":
            return torch.tensor([ids], dtype=torch.long)
        return ids

    def __len__(self):
        return 50257
