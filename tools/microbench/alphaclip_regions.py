"""AlphaCLIP region captions per second on one MI355X: 16 images x 8 boxes at full depth (ViT-B/16, 12 blocks, synthetic weights),

* batched: one forward(bboxes=...) -- every region rasterised in one launch, the tower over the regions max_batch at a time, one
  caption call for all 128 regions;
* one region per forward: the reference's call pattern (forward_alphaclip_with_regions runs a batch-1 tower pass and a caption call per
  box), as 128 forward(bboxes=[1, 1, 4]) calls;

and the ViT GEMMs' share of the MFMA peak during the batched run (pio_profile_*).  Prints one JSON line.

    python tools/microbench/alphaclip_regions.py [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from patchioner_amd import Patchioner, weights as W  # noqa: E402

MFMA_PEAK_TFLOPS = 2500.0       # dense fp16 MFMA, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--boxes", type=int, default=8)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    m = Patchioner.from_config({"prefix_size": 512, "support_memory_size": 16384, "dino_model": "AlphaClip", "normalize": False,
                                "resize_dim": 224, "crop_dim": 224, "clip_model_name": "ViT-B/16", "use_talk2dino_project": False,
                                "synthetic_seed": 5, "max_batch": 16, "max_prefixes": 128,
                                "alphaclip_config": {"patch_size": 16, "name": "ViT-B/16", "use_cls_for_localized_captions": True,
                                                     "embed_dim": 512}}, device="cuda")
    B, NB = a.images, a.boxes
    imgs = W.synth_images(1, B, 224).cuda()
    g = torch.Generator().manual_seed(2)
    xy = torch.rand(B, NB, 2, generator=g) * 160
    wh = 16 + torch.rand(B, NB, 2, generator=g) * 100
    boxes = torch.cat([xy, wh], -1)
    R = B * NB

    def batched():
        return m(imgs, get_cls_capt=False, bboxes=boxes)

    def looped():
        for i in range(B):
            for j in range(NB):
                m(imgs[i:i + 1], get_cls_capt=False, bboxes=boxes[i:i + 1, j:j + 1])

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        return best

    tb = timed(batched)
    tl = timed(looped)
    m.engine.profile_enable(True)
    batched()
    torch.cuda.synchronize()
    prof = m.engine.profile_read()
    m.engine.profile_enable(False)
    gm = prof["vit_gemm"]
    tflops = gm["flops"] / (gm["ms"] * 1e-3) / 1e12 if gm["ms"] > 0 else 0.0
    print(json.dumps({"bench": "alphaclip_regions", "images": B, "boxes": NB, "regions": R,
                      "batched_captions_per_s": round(R / tb, 1), "one_region_per_forward_captions_per_s": round(R / tl, 1),
                      "speedup": round(tl / tb, 2), "vit_gemm_ms": round(gm["ms"], 3), "vit_gemm_tflops": round(tflops, 1),
                      "vit_gemm_frac_of_peak": round(tflops / MFMA_PEAK_TFLOPS, 3), "decode_ms": round(prof["decode"]["ms"], 3)}))


if __name__ == "__main__":
    main()
