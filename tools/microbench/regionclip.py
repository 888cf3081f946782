"""RegionCLIP tower throughput: the HIP tower (vit_arch 3) against the same network through torch's MIOpen convolutions in fp16.

    python tools/microbench/regionclip.py [--batches 16 64] [--iters 10] [--configs RN50@224 RN50@512 RN50x4@288]

Per configuration and batch size: tower ms per image (HIP events around Engine.vit_forward, full-depth synthetic weights), captions / s
through Patchioner.forward (cls captions, 30-step greedy decode; B = the batch), the conv FLOPs per image computed from the shapes
and the tower's rate as a fraction of the 2.5 PFLOP/s fp16 MFMA peak, and the MIOpen yardstick (F.conv2d on NCHW fp16 with the BN
folded, plus torch's MultiheadAttention for the attnpool).  One JSON line per measurement."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from patchioner_amd import weights as W  # noqa: E402

PEAK = 2.5e15


def flops(layers, width, res, out_dim):
    """(conv FLOPs, attnpool FLOPs) per image: 2 x MACs of every convolution and of the attnpool's GEMMs and attention."""
    conv = 0
    h = res // 2
    conv += 2 * h * h * (width // 2) * 3 * 9
    conv += 2 * h * h * (width // 2) * (width // 2) * 9 + 2 * h * h * width * (width // 2) * 9
    h //= 2
    inp = width
    for L in range(4):
        p = width << L
        for i in range(layers[L]):
            s = 2 if (L > 0 and i == 0) else 1
            conv += 2 * h * h * p * inp + 2 * h * h * p * p * 9
            ho = h // s
            conv += 2 * ho * ho * 4 * p * p
            if i == 0:
                conv += 2 * ho * ho * 4 * p * inp
            h, inp = ho, 4 * p
    C, T = inp, h * h + 1
    attn = 2 * T * C * 3 * C + 4 * T * T * C + 2 * T * C * out_dim
    return conv, attn


def time_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def miopen_tower(sd, layers, width, heads, B, res):
    """The same network as torch ops in fp16 NCHW (BN folded into a per-channel scale / shift after each conv)."""
    e = W.regionclip_to_engine(sd)
    dev = {k: v.cuda().half() for k, v in e.items()}
    mha = torch.nn.MultiheadAttention(32 * width, heads).cuda().half().eval()

    def cbn(x, c, b, stride=1, res=None, relu=True):
        k = dev[c + ".weight"].shape[-1]
        y = F.conv2d(x, dev[c + ".weight"], stride=stride, padding=k // 2)
        y = y * dev[b + ".scale"][None, :, None, None] + dev[b + ".shift"][None, :, None, None]
        if res is not None:
            y = y + res
        return F.relu(y) if relu else y

    def run(x):
        x = cbn(x, "rn.conv1", "rn.bn1", 2)
        x = cbn(x, "rn.conv2", "rn.bn2")
        x = F.avg_pool2d(cbn(x, "rn.conv3", "rn.bn3"), 2)
        for L in range(4):
            for i in range(layers[L]):
                p = "rn.layer%d.%d." % (L + 1, i)
                s = 2 if (L > 0 and i == 0) else 1
                o = cbn(cbn(x, p + "conv1", p + "bn1"), p + "conv2", p + "bn2")
                if s > 1:
                    o = F.avg_pool2d(o, 2)
                idn = cbn(F.avg_pool2d(x, 2) if s > 1 else x, p + "downsample.0", p + "downsample.1", relu=False) if i == 0 else x
                x = cbn(o, p + "conv3", p + "bn3", res=idn)
        t = x.flatten(2).permute(2, 0, 1)
        t = torch.cat([t.mean(0, keepdim=True), t]) + dev["rn.attnpool.positional_embedding"][:, None]
        return mha(t, t, t, need_weights=False)[0]

    x = torch.randn(B, 3, res, res, device="cuda").half()
    return lambda: run(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--configs", nargs="+", default=["RN50@224", "RN50@512", "RN50x4@288"])
    ap.add_argument("--no-captions", action="store_true")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    from patchioner_amd.engine import Engine
    for spec in args.configs:
        name, res = spec.split("@")
        res = int(res)
        layers, width, embed, heads, out_dim = W.regionclip_arch(name)
        sd = W.synth_regionclip_rn(1, name, image_resolution=res)
        cf, af = flops(layers, width, res, out_dim)
        for B in args.batches:
            eng = Engine(embed_dim=embed, depth=sum(layers), num_heads=heads, num_registers=0, crop_dim=res, patch_size=32,
                         pretrain_grid=res // 32, max_batch=B, vit_arch="regionclip", vit_out_dim=out_dim, rn_layers=layers,
                         rn_width=width)
            eng.load_state_dict(W.regionclip_to_engine(sd), strict=True)
            eng.finalize()
            imgs = W.synth_images(0, B, res).cuda()
            ms = time_ms(lambda: eng.vit_forward(imgs, want_qkv=False), args.iters)
            eng.close()
            ms_mi = time_ms(miopen_tower(sd, layers, width, heads, B, res), args.iters)
            rec = dict(config=spec, B=B, tower_ms_per_image=ms / B, miopen_ms_per_image=ms_mi / B,
                       conv_gflop_per_image=cf / 1e9, attnpool_gflop_per_image=af / 1e9,
                       tower_fraction_of_fp16_peak=(cf + af) * B / (ms * 1e-3) / PEAK)
            if not args.no_captions and name == "RN50" and res == 224:
                from patchioner_amd import Patchioner
                rc = {"patch_size": 32, "embed_dim": 1024, "checkpoint": sd,
                      "MODEL": {"RESNETS": {"OUT_FEATURES": ["res4", "res5"], "IMAGE_RESOLUTION": res}}}
                m = Patchioner.from_config({"prefix_size": 1024, "support_memory_size": 4096, "normalize": False, "resize_dim": res,
                                            "crop_dim": res, "dino_model": "regionclip_resnet50_p32.k", "regionclip_config": rc,
                                            "synthetic_seed": 3, "max_batch": B, "use_talk2dino_project": False}, device="cuda")
                cms = time_ms(lambda: m(imgs, get_cls_capt=True), max(2, args.iters // 2))
                rec["captions_per_s"] = B / (cms * 1e-3)
                m.engine.close()
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
