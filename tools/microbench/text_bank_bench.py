"""Throughput of a memory-bank build on the device text tower: N seeded synthetic captions with a COCO-like length spread
(8-20 words) through the host BPE, the CLIP text tower at the real ViT-B/16 shapes (width 512, 8 heads, 12 layers; synthetic
weights) and Talk2DINO's text projection (512 -> 768 -> 768, tanh).  Prints ONE JSON line:

    python tools/microbench/text_bank_bench.py [--n 591753] [--dtype fp16|fp32] [--max-texts 1024]

  tokenize_s     host tokenisation (clip_text.ClipTokenizer.tokenize; word cache warm after the first thousands)
  tower_s        device time of the text tower, HIP events around every encode launch, summed
  talk2dino_s    device time of the projection (engine.text_project), events
  texts_per_s    N / (tokenize_s + tower_s + talk2dino_s)
  tower_gemm_tflops  2 x 12 W^2 x layers FLOP per token row the launches computed (padded rows Tp counted, as the GEMMs run
                 them), over tower_s; tower_gemm_tflops_algo counts only the tokens through EOT

The kernel split:  rocprofv3 --kernel-trace --stats -d <out dir> -- python tools/microbench/text_bank_bench.py --n 65536
(the stats CSV lists k_text_attention, k_text_embed, k_text_pool, k_layernorm and the k_vit_gemm* instantiations).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from patchioner_amd import clip_text as CT  # noqa: E402
from patchioner_amd import weights as W  # noqa: E402
from patchioner_amd.engine import Engine  # noqa: E402

WORDS = ("a an the two three man woman person boy girl dog cat horse bus train truck car bike kitchen table room street field "
         "beach water grass snow plate pizza sandwich cake red blue white black green young old small large tall sitting "
         "standing riding eating holding walking looking playing parked flying next to on in of with near under top front "
         "while some several group people giraffe elephant zebra umbrella surfboard skateboard frisbee laptop phone").split()


def captions(n, seed):
    rng = np.random.RandomState(seed)
    lens = rng.randint(8, 21, size=n)
    idx = rng.randint(0, len(WORDS), size=int(lens.sum()))
    out, p = [], 0
    for L in lens:
        out.append(" ".join(WORDS[i] for i in idx[p:p + L]) + ".")
        p += L
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=591753)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "fp32"])
    ap.add_argument("--max-texts", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    texts = captions(a.n, a.seed)

    tok = CT.ClipTokenizer()
    t0 = time.perf_counter()
    ids = tok.tokenize(texts)
    tokenize_s = time.perf_counter() - t0

    name, Wd, layers = "ViT-B/16", 512, 12
    enc = CT.ClipTextEncoder(name, synthetic_seed=501, operand_type=a.dtype, max_texts=a.max_texts)
    lens = ids.argmax(1) + 1
    order = torch.argsort(lens, stable=True)
    feats = torch.empty(a.n, 512, device="cuda")
    enc.encode_ids_raw(ids[order[:a.max_texts], :int(lens[order[:a.max_texts]].max())])      # warm-up (first-launch costs)
    torch.cuda.synchronize()
    ev, rows_padded = [], 0
    ids_sorted = ids[order]
    for s in range(0, a.n, a.max_texts):
        blk = ids_sorted[s:s + a.max_texts]
        L = int(lens[order[s:s + a.max_texts]].max())
        x = blk[:, :L].to("cuda", torch.int32)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        feats[s:s + blk.shape[0]] = enc.encode_ids_raw(x)
        e1.record()
        ev.append((e0, e1))
        rows_padded += blk.shape[0] * ((L + 7) // 8 * 8)
    torch.cuda.synchronize()
    tower_s = sum(e0.elapsed_time(e1) for e0, e1 in ev) / 1e3
    enc.close()

    eng = Engine(embed_dim=768, depth=1, num_heads=12, num_registers=4, crop_dim=224, max_batch=1)
    t2d = W.synth_talk2dino(11, 512, 768)
    wdev = {k: v.cuda() for k, v in t2d.items()}
    eng.text_project(feats[:1024], wdev["linear_layer.weight"], wdev["linear_layer.bias"], wdev["hidden_layers.0.weight"],
                     wdev["hidden_layers.0.bias"], act="tanh")
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for s in range(0, a.n, 65536):
        eng.text_project(feats[s:s + 65536], wdev["linear_layer.weight"], wdev["linear_layer.bias"], wdev["hidden_layers.0.weight"],
                         wdev["hidden_layers.0.bias"], act="tanh")
    e1.record()
    torch.cuda.synchronize()
    t2d_s = e0.elapsed_time(e1) / 1e3
    eng.close()

    flop_row = 2.0 * 12 * Wd * Wd * layers
    tokens = int(lens.sum())
    out = {"tool": "text_bank_bench", "n": a.n, "dtype": a.dtype, "model": name, "max_texts": a.max_texts,
           "mean_tokens": tokens / a.n, "tokenize_s": round(tokenize_s, 3), "tower_s": round(tower_s, 3),
           "talk2dino_s": round(t2d_s, 4), "texts_per_s": round(a.n / (tokenize_s + tower_s + t2d_s), 1),
           "tower_texts_per_s": round(a.n / tower_s, 1),
           "tower_gemm_tflops": round(flop_row * rows_padded / tower_s / 1e12, 1),
           "tower_gemm_tflops_algo": round(flop_row * tokens / tower_s / 1e12, 1),
           "feats_finite": bool(torch.isfinite(feats).all())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
