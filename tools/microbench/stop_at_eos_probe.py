"""stop_at_eos: what the synchronous forward() costs with and without it ("Stopping a greedy decode at the end of every caption").

    python3 tools/microbench/stop_at_eos_probe.py                 every step below, each in a process of its own under its own time limit,
                                                                  chained: the first step that fails ends the run
    python3 tools/microbench/stop_at_eos_probe.py forward         the segment table (below)
    python3 tools/microbench/stop_at_eos_probe.py viecap          the ViECap head at 16 rows, full length against stopping
    python3 tools/microbench/stop_at_eos_probe.py flagoff [--root CHECKOUT]
                                                                  forward() with the flag off, through the package of CHECKOUT (default: this
                                                                  tree): run it on two checkouts in turn to compare the default path with
                                                                  another commit's

``forward``: bench.py's workload -- 16 images, ViT-B/14 at 224 x 224, the 591 753-row bank, one trace per image, 4-layer DeCap -- with the
decoder of tests/eos_case.py at gamma 1.5 / 0.6 / 0.3 / 0 (with seeded prefixes its rows end by columns 4 / 9 / 18 / never; the columns of
THIS workload's prefixes are printed).  Per gamma one model; per segment length in 1 / 2 / 4 / 8 / 30, CALLS calls with the flag and CALLS
without, alternating in one process after every graph has been captured.  A call is timed on the host clock around forward(), which returns
strings and so ends in a device synchronise.  One JSON line per (gamma, seg): median / min / max of either, the steps run, and for the
never-stops case the per-segment round trip (t_on - t_off) / (segments - 1).
"""
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CALLS = 24
SEGS = (1, 2, 4, 8, 30)
GAMMAS = (1.5, 0.6, 0.3, 0.0)
# (mode, seconds): the four models with their banks are built once per step; the rest is a few thousand calls of some milliseconds
STEPS = (("forward", 420), ("viecap", 240), ("flagoff", 180))


def _paths(root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tests"))              # eos_case / golden_cases: this tree's


def _stat(ms):
    return {"n": len(ms), "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def _bench_model(decap_weights, **over):
    import torch
    from patchioner_amd import Patchioner, weights as W
    rows = 591753
    g = torch.Generator(device="cuda").manual_seed(6)
    bank = torch.empty(rows, 768, device="cuda", dtype=torch.float32)
    for s in range(0, rows, 65536):
        e = min(rows, s + 65536)
        bank[s:e] = torch.randn(e - s, 768, device="cuda", generator=g)
    cfg = {"decap_weights": decap_weights, "dino_weights": W.synth_dinov2(1), "memory_bank": bank, "prefix_size": 768,
           "linear_talk2dino": False, "support_memory_size": rows, "dino_model": "dinov2_vitb14_reg", "normalize": True, "resize_dim": 224,
           "crop_dim": 224, "max_batch": 16, "max_prefixes": 64}
    cfg.update(over)
    m = Patchioner.from_config(cfg, device="cuda:0")
    del bank
    torch.cuda.empty_cache()
    return m


def _inputs():
    import numpy as np
    import golden_cases as gc
    from patchioner_amd import weights as W
    rng = np.random.RandomState(2)
    return W.synth_images(1, 16, 224).cuda(), [gc.block_trace(int(rng.randint(0, 13)), int(rng.randint(0, 13))) for _ in range(16)]


def forward():
    import torch
    import eos_case as ec
    torch.set_grad_enabled(False)
    imgs, traces = _inputs()
    for gamma in GAMMAS:
        m = _bench_model(ec.decap_weights(gamma), stop_at_eos=False)
        call = lambda: m(imgs, get_cls_capt=False, traces=traces)["trace_capts"]                   # noqa: E731
        want = call()
        first = ec.first_stop(m.last_ids.cpu().numpy(), [ec.DECAP_EOT]).tolist()
        for seg in SEGS:                                             # every graph captured, every string checked, before anything is timed
            m.stop_at_eos, m.stop_segment = True, seg
            for _ in range(3):
                assert call() == want, "the strings changed (gamma %s, seg %d)" % (gamma, seg)
            m.stop_at_eos = False
            call()
        for seg in SEGS:
            on, off, ran = [], [], None
            m.stop_segment = seg
            for _ in range(CALLS):
                m.stop_at_eos = False
                off.append(_timed(call)[0])
                m.stop_at_eos = True
                on.append(_timed(call)[0])
                ran = m.last_decode_steps
            rec = {"probe": "forward", "gamma": gamma, "first_stop_columns": first, "seg": seg, "steps_run": ran, "stop": _stat(on), "full": _stat(off)}
            nseg = -(-30 // seg)
            if max(first) >= 30 and nseg > 1:
                rec["round_trip_us"] = round((rec["stop"]["median_ms"] - rec["full"]["median_ms"]) * 1e3 / (nseg - 1), 2)
            print(json.dumps(rec), flush=True)
        m.engine.close()
        del m
        torch.cuda.empty_cache()


def viecap():
    """The greedy ViECap head alone (caption_tokens on 16 feature rows; 12-layer GPT-2, hard prompts): 64 steps against stopping where
    the rows of tests/test_gpu_stop_at_eos.py's head fixture end (ramp 0.3 from position 30)."""
    import torch
    import eos_case as ec
    import golden_cases as gc
    from patchioner_amd import Patchioner, viecap as V, weights as W
    torch.set_grad_enabled(False)
    w, (vocab, merges), ents, emb, x = gc.viecap_case()
    tok = V.ByteLevelBPE(vocab, merges)
    c = gc.VIECAP
    w = ec._ramp(dict(w), "gpt.transformer.", ec.viecap_eos(tok)[0], 0.3, start=30)
    w["gpt.lm_head.weight"] = w["gpt.transformer.wte.weight"]
    vcfg = dict(clip_hidden_size=c["C"], weights=w, tokenizer=tok, entities_text=ents, texts_embeddings=emb, temperature=c["temperature"],
                top_k=c["top_k"], threshold=c["threshold"], using_hard_prompt=True, soft_prompt_first=True, using_greedy_search=True)
    m = Patchioner.from_config({"decap_weights": None, "prefix_size": 768, "linear_talk2dino": False, "support_memory_size": 0,
                                "dino_model": "dinov2_vitb14_reg", "normalize": False, "resize_dim": 224, "crop_dim": 224,
                                "dino_weights": W.synth_dinov2(91, "dinov2_vitb14_reg", depth=1), "max_batch": 2, "max_prefixes": 16,
                                "viecap": vcfg}, device="cuda:0")
    feats = torch.cat([x, x[:4] + 0.001 * gc.randn(5, 4, c["C"]), x]).cuda()               # 16 rows
    call = lambda: m.caption_tokens(feats.clone())                                           # noqa: E731
    want = call()
    first = ec.first_stop(m.last_ids.cpu().numpy(), m.viecap.eos).tolist()
    for seg in (2, 4, 8, 16):
        m.stop_at_eos, m.stop_segment = True, seg
        for _ in range(3):
            assert call() == want
        m.stop_at_eos = False
        call()
    for seg in (2, 4, 8, 16):
        on, off, ran = [], [], None
        m.stop_segment = seg
        for _ in range(CALLS):
            m.stop_at_eos = False
            off.append(_timed(call)[0])
            m.stop_at_eos = True
            on.append(_timed(call)[0])
            ran = m.last_decode_steps
        print(json.dumps({"probe": "viecap", "rows": 16, "first_stop_columns": first, "seg": seg, "steps_run": ran, "stop": _stat(on),
                          "full": _stat(off)}), flush=True)


def flagoff():
    """forward() as a caller that never heard of the flag makes it (plain seeded decoder: no row ends)."""
    import torch
    from patchioner_amd import weights as W
    torch.set_grad_enabled(False)
    m = _bench_model(W.synth_decap(3))
    imgs, traces = _inputs()
    call = lambda: m(imgs, get_cls_capt=False, traces=traces)["trace_capts"]                       # noqa: E731
    for _ in range(8):
        call()
    ms = [_timed(call)[0] for _ in range(4 * CALLS)]
    import patchioner_amd
    print(json.dumps({"probe": "flagoff", "package": os.path.dirname(patchioner_amd.__file__), "full": _stat(ms)}), flush=True)


def main(argv):
    if not argv:
        for mode, limit in STEPS:                                   # a step that fails, faults or runs out of time ends the run
            rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), mode]).returncode
            if rc != 0:
                print("step %r ended with status %d: stopping" % (mode, rc), flush=True)
                return rc
        return 0
    root = ROOT
    if "--root" in argv:
        root = os.path.abspath(argv[argv.index("--root") + 1])
    _paths(root)
    {"forward": forward, "viecap": viecap, "flagoff": flagoff}[argv[0]]()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
