"""ClipCap head: the sampler beside the decode step it follows, and the head through forward() (diagnostic).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/microbench/clipcap_probe.py steps N
    python3 tools/microbench/clipcap_probe.py --summarise OUT/.../*_kernel_trace.csv
    python3 tools/microbench/clipcap_probe.py forward [--batches 12] [--entry-length 64]

``steps N``: synthetic GPT-2-base (12 layers, vocabulary 50 257), N rows: prefill of the mapped prefix, then 20 rounds of
pio_nucleus_sample (top_p 0.8, temperature 1) and pio_lm_advance with the drawn tokens; device-event time of either call.  Under
rocprofv3 ``--summarise`` gives, from the kernel trace, k_nucleus_sample per launch and the kernels of one pio_lm_advance (all that
run between two sampler launches).  ``forward``: the c5_shard workload of bench.py (ViT-L/14-reg depth 24 fp16, 16 images per batch,
attention-weighted traces, max_prefixes 128) with the ClipCap head in place of the ViECap one: captions/s of forward()."""
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ROUNDS = 20


def summarise(path):
    rows = sorted((r for r in csv.DictReader(open(path)) if "at::native" not in r["Kernel_Name"]),      # torch's fills and copies
                  key=lambda r: int(r["Start_Timestamp"]))
    at = [i for i, r in enumerate(rows) if "k_nucleus_sample" in r["Kernel_Name"]][-ROUNDS:]
    dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    samp = [dur(rows[i]) for i in at]
    steps, names = [], {}
    for a, b in zip(at[:-1], at[1:]):
        steps.append(sum(dur(r) for r in rows[a + 1:b]))
        for r in rows[a + 1:b]:
            k = r["Kernel_Name"].split("(")[0][:60]
            names[k] = names.get(k, 0) + dur(r)
    rec = {"k_nucleus_sample_us": sum(samp) / len(samp) / 1e3, "k_nucleus_sample_min_max_us": [min(samp) / 1e3, max(samp) / 1e3],
           "lm_advance_kernels_us": sum(steps) / len(steps) / 1e3, "launches_per_advance": (at[-1] - at[0]) / (len(at) - 1) - 1,
           "advance_by_kernel_us": {k: v / len(steps) / 1e3 for k, v in sorted(names.items(), key=lambda kv: -kv[1])}}
    rec["sampler_over_advance"] = rec["k_nucleus_sample_us"] / rec["lm_advance_kernels_us"]
    print(json.dumps(rec))


def model(dino, C_depth, entry_length, max_batch):
    import torch
    import clipcap_case as cc
    from patchioner_amd import Patchioner, weights as W
    torch.set_grad_enabled(False)
    # a stub tokenizer over all 50 257 ids (tests/clipcap_case.py), so that the synthetic checkpoint has GPT-2's vocabulary: the
    # sampler's row is as wide as a real one
    return Patchioner.from_config({"decap_weights": None, "prefix_size": 768, "linear_talk2dino": False, "support_memory_size": 0,
                                   "dino_model": dino, "normalize": False, "resize_dim": 224, "crop_dim": 224,
                                   "dino_weights": W.synth_dinov2(93, dino, **C_depth), "max_batch": max_batch, "max_prefixes": 128,
                                   "vit_dtype": "fp16", "synthetic_seed": 5,
                                   "clipcap": {"tokenizer": cc.StubTokenizer(13), "entry_length": entry_length}}, device="cuda:0")


def steps(N):
    import torch
    m = model("dinov2_vitb14_reg", {"depth": 1}, 64, 2)
    eng, head = m.engine, m.clipcap
    assert eng.cfg.dec_layers == 12 and eng.cfg.dec_vocab == 50257
    g = torch.Generator(device="cuda").manual_seed(N)
    prefix = eng.clipcap_mapping(torch.randn(N, 768, device="cuda", generator=g), normalize=False)
    u = torch.rand(ROUNDS, N, device="cuda", generator=g)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for rep in range(2):                     # the second pass is the one the trace summary reads
        logp = eng.lm_prefill(prefix)
        ts, ta, kept_all = [], [], []
        for j in range(ROUNDS):
            a, b, c = ev(), ev(), ev()
            a.record()
            tok, act, kept = eng.nucleus_sample(logp, u[j], 1.0, 0.8, -1)
            b.record()
            logp = eng.lm_advance(tok, None, pos=prefix.shape[1] + j)
            c.record()
            ts.append((a, b)); ta.append((b, c)); kept_all.append(kept)
        torch.cuda.synchronize()
    med = lambda v: sorted(v)[len(v) // 2]
    print(json.dumps({"N": N, "vocab": int(eng.cfg.dec_vocab), "nucleus_sample_call_us": med([a.elapsed_time(b) for a, b in ts]) * 1e3,
                      "lm_advance_call_us": med([a.elapsed_time(b) for a, b in ta]) * 1e3,
                      "kept_median": int(torch.stack(kept_all).float().median().item())}), flush=True)


def forward(batches, entry_length):
    import numpy as np
    import torch
    import golden_cases as gc
    from patchioner_amd import weights as W
    B = 16
    m = model("dinov2_vitl14_reg", {}, entry_length, B)
    rng = np.random.RandomState(4)
    work = []
    for i in range(batches):
        imgs = W.synth_images(8 + i % 4, B, 224).cuda()
        work.append((imgs, [gc.block_trace(int(rng.randint(0, 13)), int(rng.randint(0, 13))) for _ in range(B)]))
    fwd = lambda imgs, tr: m(imgs, get_cls_capt=False, traces=tr, use_attention_tracing=True)["trace_capts"]
    for imgs, tr in work[:2]:
        fwd(imgs, tr)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for imgs, tr in work:
        fwd(imgs, tr)
    dt = time.perf_counter() - t0
    print(json.dumps({"workload": "c5_shard with the ClipCap head (synthetic GPT-2-base, vocabulary %d, prefix 10, %d sampled steps, top_p 0.8)"
                                  % (int(m.engine.cfg.dec_vocab), entry_length), "batches": batches,
                      "captions_per_s": batches * B / dt, "ms_per_batch": dt * 1e3 / batches}), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    elif sys.argv[1] == "steps":
        steps(int(sys.argv[2]))
    else:
        import argparse
        ap = argparse.ArgumentParser()
        ap.add_argument("mode")
        ap.add_argument("--batches", type=int, default=12)
        ap.add_argument("--entry-length", type=int, default=64)
        a = ap.parse_args()
        forward(a.batches, a.entry_length)
