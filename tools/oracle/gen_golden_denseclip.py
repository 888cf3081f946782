"""Generate ``tests/golden/denseclip.npz`` by running the REFERENCE's DenseCLIP path (through ``refshim``) on the CPU:

    python tools/oracle/gen_golden_denseclip.py

* towers: the reference's own ``load_denseclip`` -> ``DenseCLIPModel`` (denseclip/loader.py, clip_loader/denseclip_loader.py) on a
  synthetic checkpoint (weights.synth_denseclip_vit, written to a temporary .pth) and a temporary YAML of the cases of
  tests/denseclip_ref.py (TOWERS).  The reference takes a config NAME and joins it to the folder beside its loader; an ABSOLUTE path
  without the extension passes through both of its os.path.join calls unchanged.  Kept: the fp32 tokens of
  ``visual.forward(imgs, get_patches=True)``, strided rows;
* captions: ``Patchioner.from_config`` with ``denseclip_config`` = that path, then ``forward`` for the cls token, one gaussian box set
  and traces: the greedy ids of every caption call and the strings, and the constructor's attributes;
* the bank file names ``Im2TxtProjector.get_memory_bank_filename_and_path`` gives for the two config names the reference ships;
* the seeds of denseclip_ref.TOWERS must leave no greedy step a near-tie: the smallest top-2 margin of every forward case, measured
  with the float driver on the reference's own prefixes, has to exceed parity_helpers.MARGIN_BOUND (asserted here).

Build container only; the fixture holds the reference's outputs (data), never its source."""
import copy
import json
import os
import sys
import tempfile

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import denseclip_ref as DR  # noqa: E402
import refshim  # noqa: E402
from gen_golden import make_projector, save  # noqa: E402
from parity_helpers import MARGIN_BOUND  # noqa: E402

torch.set_grad_enabled(False)


def main():
    ref = refshim.load()
    sys.modules.setdefault("src", sys.modules["refsrc"])
    c = DR.CASE
    arrs, meta = {}, {}
    dec_w, bank = DR.decoder_and_bank()
    work = tempfile.mkdtemp(prefix="denseclip_golden_")
    dec_path = os.path.join(work, "decap.pt")
    torch.save(dec_w, dec_path)
    calls = []

    def capture(ids):
        calls[-1].append([int(t) for t in ids])
        return ref.decap._Tokenizer.decode(ids)

    for tag, t in DR.TOWERS.items():
        ck_path = os.path.join(work, tag + ".pth")
        torch.save(DR.checkpoint(tag), ck_path)
        cfg_base = os.path.join(work, "denseclip_" + tag)          # the "name": absolute, no extension
        with open(cfg_base + ".yaml", "w") as f:
            yaml.safe_dump(DR.config(tag, checkpoint_path=ck_path), f)
        res = t["resolution"]
        model = ref.model.Patchioner.from_config(
            {"decap_weights": dec_path, "prefix_size": 512, "support_memory_size": 0, "dino_model": "INViTE_B16", "normalize": False,
             "resize_dim": res, "crop_dim": res, "clip_model_name": "ViT-B/16", "use_talk2dino_project": False, "linear_talk2dino": False,
             "denseclip_config": cfg_base}, device="cpu")
        model.eval()
        toks = model.dino.visual.forward(DR.images(tag), get_patches=True)
        assert toks.dtype == torch.float32 and toks.shape == (c["B"], 1 + (res // c["patch"]) ** 2, c["embed_dim"])
        arrs[tag + "__tokens"] = toks[:, ::t["stride"]].numpy().astype(np.float32)
        print(tag, tuple(toks.shape), float(toks.abs().max()))
        model.decoding_method = capture
        model.im_proj = make_projector(ref, bank / bank.norm(dim=-1, keepdim=True))
        meta[tag] = dict(backbone_type=model.backbone_type, patch_size=model.patch_size, embed_dim=model.embed_dim,
                         num_tokens=model.num_tokens, num_patch_tokens=model.num_patch_tokens, num_global_tokens=model.num_global_tokens,
                         num_attn_heads=model.num_attn_heads, vision=model.denseclip_config["model"]["vision"],
                         has_blocks=hasattr(model.dino, "blocks"))
        orc, dec = DR.driver(tag)
        for name, kw in DR.FORWARD_CASES:
            calls.clear()
            orig = ref.model.decoding_batched

            def wrapped(*a, **k):
                calls.append([])
                return orig(*a, **k)

            ref.model.decoding_batched = wrapped
            try:
                outs = model(DR.images(tag).clone(), **copy.deepcopy(DR.forward_args(kw, res)))
            finally:
                ref.model.decoding_batched = orig
            key = tag + "__" + name
            meta[key] = outs
            ids = np.asarray([r for call in calls for r in call], dtype=np.int64).reshape(-1, 30)
            arrs[key + "__ids"] = ids
            # no near-tie among the reference's greedy steps: the float driver's prefixes are the reference's to fp32 rounding, and its
            # ids must be the reference's for the margin to speak about the reference's steps
            orc.call_log, orc.prefix_log = [], []
            orc.forward(DR.images(tag), **DR.forward_args(kw, res))
            assert np.array_equal(torch.cat(orc.call_log).numpy(), ids), key
            P = torch.cat(orc.prefix_log)
            _, _, margin = dec.decode_ids(P[torch.isfinite(P).all(1)], cached=True)
            print(key, outs, "smallest top-2 margin %.3e" % float(margin.min()))
            assert float(margin.min()) > MARGIN_BOUND, (key, float(margin.min()))
    P = ref.im2txt.Im2TxtProjector
    names = {}
    for cfg_name in DR.SHIPPED_CONFIG_NAMES:
        for t2d in (False, True):
            fn, _ = P.get_memory_bank_filename_and_path("coco_captions", clip_modelname="ViT-B/16", support_memory_size=500000,
                                                        use_talk2dino=t2d, denseclip_config=cfg_name, im2txt_memory_path="/banks")
            names["%s|%d" % (cfg_name, int(t2d))] = fn
    meta["bank_filenames"] = names
    print(names)
    arrs["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    save("denseclip", **arrs)
    for f in os.listdir(work):
        os.unlink(os.path.join(work, f))
    os.rmdir(work)


if __name__ == "__main__":
    main()
