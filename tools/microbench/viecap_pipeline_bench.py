"""Config 5 (ViECap head) through forward() and through TraceCaptionPipeline, on the c5_shard workload of bench.py.

    python tools/microbench/viecap_pipeline_bench.py [--batches 24] [--out FILE]

Workload as bench.py builds c5_shard: ViT-L/14-reg 224^2 at depth 24, fp16, 16 images per batch, attention-weighted traces, synthetic
GPT-2-base ViECap head with hard + soft prompt, 64 greedy steps; max_prefixes raised to 128 so that a decode group holds 8 batches.
Prints one JSON line: captions/s of forward() and of the pipeline (groups of 8 batches, with and without decoder clones) over the same
batches, whether every caption is identical, and the ragged decode of 128 rows against pio_viecap_decode of 16 rows."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=24)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import golden_cases as gc
    from patchioner_amd import Patchioner, viecap as V, weights as W
    from patchioner_amd.pipeline import TraceCaptionPipeline
    torch.set_grad_enabled(False)
    B, crop, D, K = 16, 224, 1024, args.batches
    vocab, merges = W.synth_bpe(0)
    tok = V.ByteLevelBPE(vocab, merges)
    ents = list(W.SYNTH_ENTITIES)
    vc = dict(clip_hidden_size=D, weights=W.synth_viecap(311, clip_hidden_size=D, n_layer=12, tok_vocab=len(vocab)), tokenizer=tok,
              entities_text=ents, texts_embeddings=W.synth_entity_embeddings(312, len(ents), D), temperature=gc.VIECAP["temperature"],
              top_k=gc.VIECAP["top_k"], threshold=gc.VIECAP["threshold"], using_hard_prompt=True, soft_prompt_first=True, using_greedy_search=True)
    m = Patchioner.from_config({"decap_weights": None, "prefix_size": 768, "linear_talk2dino": False, "support_memory_size": 0,
                                "dino_model": "dinov2_vitl14_reg", "normalize": False, "resize_dim": crop, "crop_dim": crop,
                                "dino_weights": W.synth_dinov2(93, "dinov2_vitl14_reg"), "max_batch": B, "max_prefixes": 128, "viecap": vc,
                                "vit_dtype": "fp16"}, device="cuda:0")
    rng = np.random.RandomState(4)
    batches = []
    for i in range(K):
        imgs = W.synth_images(8 + i % 4, B, crop).cuda()
        traces = [gc.block_trace(int(rng.randint(0, 13)), int(rng.randint(0, 13))) for _ in range(B)]
        batches.append((imgs, traces))
    rec = {"workload": "c5_shard (bench.py) with max_prefixes 128: ViT-L/14-reg depth 24 fp16, 16 images per batch, attention-weighted "
                       "traces, ViECap head (hard + soft prompt, synthetic GPT-2-base, 64 greedy steps)", "batches": K}

    def fwd(imgs, tr):
        return m(imgs, get_cls_capt=False, traces=tr, use_attention_tracing=True)["trace_capts"]

    for imgs, tr in batches[:2]:
        fwd(imgs, tr)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = [fwd(imgs, tr) for imgs, tr in batches]
    dt = time.perf_counter() - t0
    rec["forward"] = {"captions_per_s": K * B / dt, "ms_per_batch": dt * 1e3 / K}
    for clones in (0, 2):
        pipe = TraceCaptionPipeline(m, group_batches=8, vit_batches=2, use_attention_tracing=True, decode_clones=clones)
        list(pipe.run(batches, total=K))                         # warm: every decoder's graphs of the group sizes, workspaces
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = list(pipe.run(batches, total=K))
        dt = time.perf_counter() - t0
        pipe.close()
        rec["pipeline_clones%d" % clones] = {"captions_per_s": K * B / dt, "ms_per_batch": dt * 1e3 / K, "group_batches": 8,
                                             "vit_batches": 2, "identical_to_forward": got == want}
    # decode alone: the ragged decode of 128 rows against pio_viecap_decode of 16 rows (same soft prompts / token rows)
    eng, head = m.engine, m.viecap
    feats = torch.randn(128, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    cont, tokens, lens = head.stage(feats)
    Lb = int(lens[:16].max().item())

    def timed(fn, reps=5):
        fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / reps

    rec["decode_ms"] = {
        "uniform_16_rows": timed(lambda: eng.viecap_decode(cont[:16], tokens[:16, :Lb], soft_first=True, steps=64)),
        "ragged_16_rows": timed(lambda: eng.viecap_decode_ragged(cont[:16], tokens[:16], lens[:16], soft_first=True, steps=64)),
        "ragged_128_rows": timed(lambda: eng.viecap_decode_ragged(cont, tokens, lens, soft_first=True, steps=64)),
        "Pmax": int(cont.shape[1] + tokens.shape[1]), "P_16_rows": int(cont.shape[1]) + Lb}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
