"""INViTE tower time against the number of self-only blocks, and the V-only GEMM beside the qkv GEMM it replaces.

    python tools/microbench/invite.py [--batch 80] [--iters 20] [--repeats 7] [--ks 0 1 12]

ViT-B/16 at 224^2, full depth 12, synthetic weights, fp16 operands.  One engine per k (vit_self_only_layers), all alive at once; the
timed rounds ALTERNATE between them (k0, k1, k12, k0, ...), `repeats` rounds of `iters` forwards each after a warm-up round, HIP events
around Engine.vit_forward.  Per k: median, minimum and maximum tower ms per image over the rounds -- the spread of k = 0 is what a
difference has to exceed.  Then, from the engine's own per-class event timers (a separate pass: they serialise the launches), the GEMM
/ attention / LayerNorm ms per forward; and through the test hooks the V-only GEMM and the qkv GEMM alone at the same M = batch x 200
rows, in microseconds.  One JSON line per measurement."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from patchioner_amd import _lib  # noqa: E402
from patchioner_amd import weights as W  # noqa: E402


def time_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def gemm_alone_us(B, iters):
    """(V-only us, qkv us, path of each) at M = B * 200, D = 768, fp16, on the dispatch's own choice of kernel."""
    L = _lib.load()
    D, Tp, H, Tk = 768, 200, 12, 256
    M = B * Tp
    g = torch.Generator(device="cuda").manual_seed(1)
    A = torch.randn(M, D, generator=g, device="cuda").half()
    Wf = (torch.randn(3 * D, D, generator=g, device="cuda") * 0.05).half()
    bf = torch.randn(3 * D, generator=g, device="cuda") * 0.1
    out = torch.empty(M, D, dtype=torch.float16, device="cuda")
    q = torch.empty(B, H, Tk, 64, dtype=torch.float16, device="cuda")
    k, vT = torch.empty_like(q), torch.empty(B, H, 64, Tk, dtype=torch.float16, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    tv, tq = ctypes.c_int32(-1), ctypes.c_int32(-1)
    args = _lib.PioTestGemmArgs(A.data_ptr(), Wf.data_ptr(), bf.data_ptr(), M, 3 * D, D, D, None, None, None, q.data_ptr(), k.data_ptr(),
                                vT.data_ptr(), None, 197, Tp, Tk, 1, 196, D, H, 0, None, 0)

    def vonly():
        _lib.check(L.pio_test_vit_vonly(0, 0, A.data_ptr(), Wf.data_ptr(), bf.data_ptr(), out.data_ptr(), M, D, ctypes.byref(tv), s))

    def qkv():
        _lib.check(L.pio_test_vit_gemm(0, 1, 0, ctypes.byref(args), ctypes.byref(tq), s))

    res = {}
    for name, fn in (("v_only", vonly), ("qkv", qkv), ("v_only", vonly), ("qkv", qkv)):       # alternated; the second pair is kept
        time_ms(fn, 20)
        res[name] = time_ms(fn, iters) * 1e3
    return res["v_only"], res["qkv"], tv.value, tq.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=80)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--ks", type=int, nargs="+", default=[0, 1, 12])
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    from patchioner_amd.engine import Engine
    B = args.batch
    sd = W.invite_to_engine(W.synth_invite_vit(1, "ViT-B/16"))
    imgs = W.synth_images(0, B, 224).cuda()
    engines = {}
    for k in args.ks:
        e = Engine(embed_dim=768, depth=12, num_heads=12, num_registers=0, crop_dim=224, patch_size=16, pretrain_grid=14, prefix_size=512,
                   max_batch=B, vit_dtype="fp16", vit_arch="clip", vit_out_dim=512, vit_ln_eps=1e-5, vit_self_only_layers=k)
        e.load_state_dict(sd, strict=True)
        e.finalize()
        engines[k] = e
    rounds = {k: [] for k in args.ks}
    for r in range(args.repeats + 1):
        for k in args.ks:
            ms = time_ms(lambda: engines[k].vit_forward(imgs, want_qkv=False), args.iters)
            if r > 0:                                   # round 0 warms every shape up
                rounds[k].append(ms / B)
    for k in args.ks:
        v = rounds[k]
        print(json.dumps(dict(measure="tower_ms_per_image", model="ViT-B/16@224", depth=12, batch=B, self_only_layers=k,
                              median=statistics.median(v), min=min(v), max=max(v), rounds=len(v), iters_per_round=args.iters)), flush=True)
    for k in args.ks:
        e = engines[k]
        e.profile_enable(True)
        for _ in range(5):
            e.vit_forward(imgs, want_qkv=False)
        torch.cuda.synchronize()
        p = e.profile_read()
        e.profile_enable(False)
        print(json.dumps(dict(measure="per_class_ms_per_forward", batch=B, self_only_layers=k,
                              **{c: p[c]["ms"] / 5 for c in ("vit_gemm", "vit_attention", "vit_layernorm")},
                              **{c + "_launches": p[c]["launches"] // 5 for c in ("vit_gemm", "vit_attention", "vit_layernorm")})), flush=True)
    for e in engines.values():
        e.close()
    v_us, q_us, pv, pq = gemm_alone_us(B, 200)
    print(json.dumps(dict(measure="gemm_alone_us", M=B * 200, D=768, v_only_us=v_us, qkv_us=q_us, v_only_path=pv, qkv_path=pq)), flush=True)


if __name__ == "__main__":
    main()
