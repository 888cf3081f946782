"""Config 5 (ViECap head) with BEAM search (width 5, the reference VieCap's default) three ways, on the c5_shard workload of bench.py:
forward() (one beam_search per image, host bookkeeping between device steps), forward_async (one batched device beam search per
batch, pio_lm_beam_search) and TraceCaptionPipeline(beam_search=True) (one batched search per group).

    python tools/microbench/viecap_beam_bench.py [--batches 6] [--width 5] [--out FILE]

Workload as viecap_pipeline_bench.py: ViT-L/14-reg 224^2 at depth 24, fp16, 16 images per batch, attention-weighted traces, synthetic
GPT-2-base ViECap head with hard + soft prompt, 64 steps; max_prefixes 128.  Prints one JSON line: captions/s of each way over the
same batches, whether every caption equals forward()'s, and the batched search alone (ms per search and per step) at 16 and at
128 // W images."""
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
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--width", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import golden_cases as gc
    from patchioner_amd import Patchioner, viecap as V, weights as W
    from patchioner_amd.pipeline import TraceCaptionPipeline
    torch.set_grad_enabled(False)
    B, crop, D, K, BW = 16, 224, 1024, args.batches, args.width
    vocab, merges = W.synth_bpe(0)
    tok = V.ByteLevelBPE(vocab, merges)
    ents = list(W.SYNTH_ENTITIES)
    vc = dict(clip_hidden_size=D, weights=W.synth_viecap(311, clip_hidden_size=D, n_layer=12, tok_vocab=len(vocab)), tokenizer=tok,
              entities_text=ents, texts_embeddings=W.synth_entity_embeddings(312, len(ents), D), temperature=gc.VIECAP["temperature"],
              top_k=gc.VIECAP["top_k"], threshold=gc.VIECAP["threshold"], using_hard_prompt=True, soft_prompt_first=True,
              using_greedy_search=False, beam_width=BW)
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
                       "traces, ViECap head (hard + soft prompt, synthetic GPT-2-base, beam search width %d, 64 steps)" % BW,
           "batches": K, "beam_width": BW}
    kw = dict(get_cls_capt=False, use_attention_tracing=True)

    fwd = lambda imgs, tr: m(imgs, traces=tr, **kw)["trace_capts"]
    fwd(*batches[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = [fwd(imgs, tr) for imgs, tr in batches]
    dt = time.perf_counter() - t0
    rec["forward"] = {"captions_per_s": K * B / dt, "ms_per_batch": dt * 1e3 / K}

    m.forward_async(batches[0][0], traces=batches[0][1], **kw).result()          # warm: workspaces and the graph
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pend = [m.forward_async(imgs, traces=tr, **kw) for imgs, tr in batches]
    got = [p.result()["trace_capts"] for p in pend]
    dt = time.perf_counter() - t0
    rec["forward_async"] = {"captions_per_s": K * B / dt, "ms_per_batch": dt * 1e3 / K, "identical_to_forward": got == want}

    pipe = TraceCaptionPipeline(m, group_batches=1, use_attention_tracing=True, beam_search=True)
    list(pipe.run(batches, total=K))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = list(pipe.run(batches, total=K))
    dt = time.perf_counter() - t0
    pipe.close()
    rec["pipeline"] = {"captions_per_s": K * B / dt, "ms_per_batch": dt * 1e3 / K, "group_batches": 1, "identical_to_forward": got == want}

    # the batched search alone, on staged prompts
    eng, head = m.engine, m.viecap
    feats = torch.randn(128, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    cont, tokens, lens = head.stage(feats)

    def timed(n, reps=3):
        f = lambda: eng.viecap_beam_ragged(cont[:n], tokens[:n], lens[:n], BW, head.eos, soft_first=True, steps=64)
        f()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / reps

    rec["search_ms"] = {}
    for n in sorted({16, 128 // BW}):
        ms = timed(n)
        rec["search_ms"]["%d_images" % n] = {"ms": ms, "ms_per_step": ms / 64, "captions_per_s": n * 1e3 / ms}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
