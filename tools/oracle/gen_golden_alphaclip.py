"""Generate ``tests/golden/alphaclip.npz`` by running the REFERENCE's AlphaCLIP path (through ``refshim``):

    python tools/oracle/gen_golden_alphaclip.py

* masks: alpha_mask_utils.bbox_to_alpha_mask / trace_to_alpha_mask at pixel level (grid = crop, divisor 1) and patch level (grid =
  crop / p, divisor p) for the box / trace table of tests/alphaclip_ref.py (np.packbits);
* tower tokens: the reference's own ``VisionTransformer`` (alpha_clip/model.py) built from weights.synth_alphaclip_vit at depth 2, for a
  few regions' masks;
* captions: ``Patchioner.forward`` with ``alphaclip_config`` (``load_alphaclip`` monkeypatched to hand over that tower; ``loralib``,
  used only with lora_adapt=True, stubbed) for boxes with dummies, traces, controllable sets, the whole image and
  use_cls_for_localized_captions False, with compute_scores: the greedy ids of every caption call and the outputs.

Build container only; the fixture holds the reference's outputs (data), never its source."""
import copy
import importlib
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import alphaclip_ref as AR  # noqa: E402
import refshim  # noqa: E402
from gen_golden import make_projector, save  # noqa: E402
from patchioner_amd import weights as W  # noqa: E402

torch.set_grad_enabled(False)


def load_alpha_modules(ref):
    """The reference's alpha_clip/model.py and alpha_mask_utils.py, imported as they import themselves (``src.`` absolute names)."""
    if "loralib" not in sys.modules:
        refshim._stub("loralib", MergedLinear=None, Linear=None)
    sys.modules.setdefault("src", sys.modules["refsrc"])
    pkg = types.ModuleType("src.alphaclip")
    pkg.__path__ = [os.path.join(refshim.REF_SRC, "alphaclip")]
    sys.modules["src.alphaclip"] = pkg
    spec = importlib.util.spec_from_file_location("alphaclip_model", os.path.join(refshim.REF_SRC, "alphaclip", "alpha_clip", "model.py"))
    model = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(model)
    masks = importlib.import_module("src.alphaclip.alpha_mask_utils")
    return model, masks


def build_tower(amodel, sd, depth):
    D, _, heads, p, out, crop = W.alphaclip_arch(AR.CASE["name"])
    vt = amodel.VisionTransformer(crop, p, D, depth, heads, out)
    missing, unexpected = vt.load_state_dict(sd, strict=True)
    return vt.eval()


def main():
    ref = refshim.load()
    amodel, amu = load_alpha_modules(ref)
    c = AR.CASE
    arrs, meta = {}, {}
    crop, p = c["crop"], c["patch"]
    n = crop // p
    # ---- masks
    pix, cell = [], []
    for b in AR.MASK_BOXES:
        bt = torch.tensor(b, dtype=torch.float32)
        pix.append(amu.bbox_to_alpha_mask(bt, crop, 1, crop).numpy() > 0)
        cell.append(amu.bbox_to_alpha_mask(bt, n, p, crop).numpy() > 0)
    for tr in AR.MASK_TRACES:
        pix.append(amu.trace_to_alpha_mask(tr, crop).numpy() > 0)
        cell.append(amu.trace_to_alpha_mask(tr, n).numpy() > 0)
    arrs["mask_pix"] = np.packbits(np.stack(pix).reshape(len(pix), -1), axis=1)
    arrs["mask_cell"] = np.packbits(np.stack(cell).reshape(len(cell), -1), axis=1)
    # the controllable path with the points of ONE trace per image (traces_to_alpha_mask walks a list of traces)
    try:
        amu.traces_to_alpha_mask(AR.MASK_TRACES[0], crop)
        meta["traces_of_points_error"] = None
    except Exception as ex:  # noqa: BLE001
        meta["traces_of_points_error"] = type(ex).__name__
    # ---- the tower
    sd = W.synth_alphaclip_vit(c["seed_vit"], c["name"], depth=c["depth"])
    vt = build_tower(amodel, sd, c["depth"])
    imgs = W.synth_images(c["seed_img"], c["B"], crop)
    tok_masks = [AR.box_mask([10.5, 20.25, 100.0, 60.0], crop, 1), AR.trace_mask(AR.MASK_TRACES[2], crop), torch.zeros(crop, crop, dtype=torch.uint8)]
    toks = []
    for i, m in enumerate(tok_masks):
        toks.append(vt(imgs[i % c["B"]][None], alpha=m.float()[None], return_patches=True)[0])
    toks.append(vt(imgs[:1], alpha=torch.ones(1, 1, crop, crop), return_patches=True)[0])       # the whole-image forward
    arrs["tok_masks"] = np.packbits(torch.stack(tok_masks).numpy().reshape(len(tok_masks), -1) > 0, axis=1)
    arrs["tok_img"] = np.array([0, 1, 0, 0])
    arrs["tokens"] = torch.stack(toks)[:, ::4].numpy().astype(np.float32)      # every 4th token row (the CLS row first): the size limit
    # ---- captions through the reference's Patchioner
    dec_w = W.synth_decap(c["seed_dec"], prefix_size=512)
    bank = W.synth_bank(c["seed_bank"], c["bank_rows"], 512) * 2.0
    holder = torch.nn.Module()
    holder.visual = vt
    loader = types.ModuleType("src.alphaclip.alphaclip_loader")
    loader.load_alphaclip = lambda **k: (None, holder, None)
    sys.modules["src.alphaclip.alphaclip_loader"] = loader
    tmp = tempfile.NamedTemporaryFile(suffix=".pt", delete=False)
    torch.save(dec_w, tmp.name)
    models = {}
    try:
        for use_cls in (True, False):
            models[use_cls] = ref.model.Patchioner.from_config(
                {"decap_weights": tmp.name, "prefix_size": 512, "support_memory_size": 0, "dino_model": "AlphaClip", "normalize": False,
                 "resize_dim": crop, "crop_dim": crop, "clip_model_name": "ViT-B/16", "use_talk2dino_project": False,
                 "alphaclip_config": {"patch_size": p, "name": c["name"], "alpha_vision_checkpoint": "synthetic",
                                      "use_cls_for_localized_captions": use_cls, "embed_dim": 512}}, device="cpu")
    finally:
        os.unlink(tmp.name)
    calls = []

    def capture(ids):
        calls[-1].append([int(t) for t in ids])
        return ref.decap._Tokenizer.decode(ids)

    def run(tag, model, **kw):
        model.eval()
        model.decoding_method = capture
        model.im_proj = make_projector(ref, bank / bank.norm(dim=-1, keepdim=True))     # normalize_memory_embs: not a dinov2 name
        calls.clear()
        orig = ref.model.decoding_batched

        def wrapped(*a, **k):
            calls.append([])
            return orig(*a, **k)

        ref.model.decoding_batched = wrapped
        try:
            outs = model(imgs.clone(), **copy.deepcopy(kw))
        except Exception as ex:  # noqa: BLE001
            outs = {"__error__": type(ex).__name__}
        finally:
            ref.model.decoding_batched = orig
        meta[tag] = outs
        arrs[tag + "__ids"] = np.asarray([r for call in calls for r in call], dtype=np.int64).reshape(-1, 30)
        print(tag, {k: v for k, v in outs.items()})

    boxes, traces = AR.region_boxes(), AR.region_traces()
    m = models[True]
    run("boxes", m, get_cls_capt=True, bboxes=boxes.clone(), compute_scores=True)
    kept = boxes.clone()
    m(imgs.clone(), bboxes=kept)
    meta["boxes_untouched"] = bool(torch.equal(kept, boxes))
    run("traces", m, get_cls_capt=False, traces=traces, compute_scores=True)
    run("boxes_traces", m, bboxes=boxes.clone(), traces=traces)
    run("controllable", m, get_cls_capt=False, bboxes=boxes.clone(), get_controllable_capts=True, compute_scores=True)
    run("controllable_traces", m, get_cls_capt=False, traces=traces, get_controllable_capts=True)
    run("controllable_trace_lists", m, get_cls_capt=False, traces=[[tr] for tr in traces], get_controllable_capts=True)
    run("whole", m, get_cls_capt=True, get_avg_patch_capt=True, compute_scores=True)
    run("patches_boxes_traces", models[False], bboxes=boxes.clone(), traces=traces, compute_scores=True)
    run("patches_controllable", models[False], get_cls_capt=False, bboxes=boxes.clone(), get_controllable_capts=True)
    arrs["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    save("alphaclip", **arrs)


if __name__ == "__main__":
    main()
