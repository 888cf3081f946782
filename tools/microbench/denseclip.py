"""DenseCLIP tower time, dense against the sparse tail, and the exact-fp32 head alone.

    python tools/microbench/denseclip.py [--batch 16] [--iters 5] [--repeats 7] [--patches 16 64 256]

ViT-B/16 at 640^2 (40 x 40 patches, T = 1601), full depth 12, synthetic weights, fp16 operands, at the launch the workspace is sized for
(max_batch, default 16).  ONE engine serves every variant (the sparse tail is a second entry point of the same handle, so the variants
share weights, workspaces and clocks); the timed rounds ALTERNATE between them (dense, sparse 16, sparse 64, sparse 256, dense, ...),
`repeats` rounds of `iters` forwards each after a warm-up round, HIP events around Engine.trace_grids + Engine.vit_forward (dense) and
Engine.trace_grids(select_rows=True) + Engine.vit_forward_rows (sparse): what a traces call runs up to its tokens, the host's row
selection included (it is also timed on its own, in wall-clock time).
A sparse variant selects a square block of p patches per image (4 x 4, 8 x 8, 16 x 16), at a different place in every image.  Per
variant: median, minimum and maximum ms per forward over the rounds -- two variants differ when their ranges do not overlap.  Then the
head alone, k_sgemm_tn at the dense M = batch x 1601, K = 768, N = 512 (through pio_text_project, which is that launch plus a bias),
and from the engine's per-class event timers (a separate pass: they serialise the launches) the GEMM / attention / LayerNorm ms per
dense forward, one twelfth of which is a block.  One JSON line per measurement."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from patchioner_amd import weights as W  # noqa: E402


def time_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def block(cx, cy, side, n=40):
    return [dict(x=(cx + i + 0.5) / n, y=(cy + j + 0.5) / n) for j in range(side) for i in range(side)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--patches", type=int, nargs="+", default=[16, 64, 256])
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    from patchioner_amd.engine import Engine
    B, depth = args.batch, args.depth
    vis = {"image_resolution": 640, "vision_layers": depth, "vision_width": 768, "vision_patch_size": 16, "embed_dim": 512}
    e = Engine(embed_dim=768, depth=depth, num_heads=12, num_registers=0, crop_dim=640, patch_size=16, pretrain_grid=40, prefix_size=512,
               max_batch=B, vit_dtype="fp16", vit_arch="clip", vit_out_dim=512, vit_ln_eps=1e-5, sparse_clip_tail=True)
    e.load_state_dict(W.denseclip_to_engine(W.synth_denseclip_vit(1, 640, depth), vis), strict=True)
    e.finalize()
    imgs = W.synth_images(0, B, 640).cuda()
    first = [block((7 * b) % 37, (11 * b) % 37, 4) for b in range(B)]

    def dense():
        e.trace_grids(first)                            # what a traces call does in front of either tower path
        return e.vit_forward(imgs, want_qkv=False)

    variants = {"dense": dense}
    for p in args.patches:
        side = math.isqrt(p)
        traces = [block((7 * b) % (41 - side), (11 * b) % (41 - side), side) for b in range(B)]
        t0 = time.perf_counter()
        for _ in range(20):
            _, sel = e.trace_grids(traces, select_rows=True)
        torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) / 20 * 1e3
        assert sel is not None, "selection above the cut-over share"
        print(json.dumps(dict(measure="row_selection", patches_per_image=side * side, batch=B, selected_rows=4 * sel["nq"],
                              share_of_rows=4 * sel["nq"] / (B * e.Tp), trace_grids_select_wall_ms=host_ms)), flush=True)

        def run(traces=traces):
            _, s = e.trace_grids(traces, select_rows=True)
            return e.vit_forward_rows(imgs, s)

        variants["sparse_%d" % (side * side)] = run
    rounds = {k: [] for k in variants}
    for r in range(args.repeats + 1):
        for k, fn in variants.items():
            ms = time_ms(fn, args.iters)
            if r > 0:                                   # round 0 warms every shape up
                rounds[k].append(ms)
    dense_med = statistics.median(rounds["dense"])
    for k, v in rounds.items():
        print(json.dumps(dict(measure="tower_ms_per_forward", model="ViT-B/16@640", depth=depth, batch=B, variant=k,
                              median=statistics.median(v), min=min(v), max=max(v), rounds=len(v), iters_per_round=args.iters,
                              median_over_dense=statistics.median(v) / dense_med,
                              ranges_apart_from_dense=(k != "dense" and (max(v) < min(rounds["dense"]) or min(v) > max(rounds["dense"]))))),
              flush=True)
    # the head alone at the dense M
    M = B * e.T
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(M, 768, generator=g, device="cuda")
    w = torch.randn(512, 768, generator=g, device="cuda") * 0.03
    b0 = torch.zeros(512, device="cuda")
    head = []
    for r in range(args.repeats + 1):
        ms = time_ms(lambda: e.text_project(x, w, b0), 10)
        if r > 0:
            head.append(ms)
    print(json.dumps(dict(measure="head_alone_ms", kernel="k_sgemm_tn", M=M, K=768, N=512, median=statistics.median(head), min=min(head),
                          max=max(head), share_of_dense_forward=statistics.median(head) / dense_med)), flush=True)
    e.profile_enable(True)
    for _ in range(3):
        e.vit_forward(imgs, want_qkv=False)
    torch.cuda.synchronize()
    p = e.profile_read()
    e.profile_enable(False)
    cls = {c: p[c]["ms"] / 3 for c in ("vit_gemm", "vit_attention", "vit_layernorm")}
    print(json.dumps(dict(measure="per_class_ms_per_dense_forward", batch=B, depth=depth, **cls,
                          one_block_ms=sum(cls.values()) / depth, one_block_share_of_serialised_sum=1.0 / depth)), flush=True)
    e.close()


if __name__ == "__main__":
    main()
