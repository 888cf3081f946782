"""Generate ``tests/golden/invite.npz`` by running the REFERENCE's INViTE path (through ``refshim``) on the CPU:

    python tools/oracle/gen_golden_invite.py

* towers: the reference's own ``build_model`` (INViTE/clipfolder/model.py: CLIP -> VisionTransformer, convert_weights,
  resize_pos_embed) on a full CLIP state dict -- weights.synth_invite_vit under ``visual.`` beside a one-layer synthetic text tower --
  then ``.float()`` as clip.load does on the CPU, for the cases of tests/invite_ref.py (TOWERS): the fp32 tokens of
  ``visual(imgs, get_all_last=True)``, strided rows; for the resized case a sample of the resampled position table.
  ``Transformer.__init__`` calls ``mask.cuda()``: ``torch.Tensor.cuda`` is the identity while the model is built;
* captions: ``Patchioner.forward`` with ``invite_config`` (``load_invite_clip`` replaced by a function that hands over that tower) for
  the cls token, one gaussian box set and traces: the greedy ids of every caption call and the strings.

Build container only; the fixture holds the reference's outputs (data), never its source."""
import copy
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

import invite_ref as IR  # noqa: E402
import refshim  # noqa: E402
from gen_golden import make_projector, save  # noqa: E402
from patchioner_amd import weights as W  # noqa: E402

torch.set_grad_enabled(False)


def load_invite_model():
    spec = importlib.util.spec_from_file_location("invite_clip_model", os.path.join(refshim.REF_SRC, "INViTE", "clipfolder", "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_tower(imodel, tag):
    """The reference's CLIP for tower case ``tag``, as clip.load(..., jit=False) leaves it on the CPU."""
    t, c = IR.TOWERS[tag], IR.CASE
    sd = {"visual." + k: v for k, v in W.synth_invite_vit(c["seed_vit"], t["name"], depth=c["depth"]).items()}
    sd.update(W.synth_clip_text(c["seed_text"], t["name"], layers=1))
    sd["logit_scale"] = torch.tensor(4.6052)
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        model = imodel.build_model(sd, t["k"], False, image_resolution=t["resolution"])
    finally:
        torch.Tensor.cuda = cuda
    return model.float()


def main():
    ref = refshim.load()
    imodel = load_invite_model()
    c = IR.CASE
    arrs, meta = {}, {}
    towers = {}
    for tag, t in IR.TOWERS.items():
        towers[tag] = m = build_tower(imodel, tag)
        toks = m.visual(IR.images(tag), get_all_last=True)
        arrs[tag + "__tokens"] = toks[:, ::t["stride"]].numpy().astype(np.float32)
        print(tag, tuple(toks.shape), float(toks.abs().max()))
        if t["resolution"] is not None:
            arrs[tag + "__pos"] = m.visual.positional_embedding.detach()[IR.POS_SAMPLE].numpy().astype(np.float32)
    # ---- captions through the reference's Patchioner
    dec_w = W.synth_decap(c["seed_dec"], prefix_size=512)
    bank = W.synth_bank(c["seed_bank"], c["bank_rows"], 512)
    sys.modules.setdefault("src", sys.modules["refsrc"])
    pkg = types.ModuleType("src.INViTE")
    pkg.__path__ = []
    sys.modules["src.INViTE"] = pkg
    loader = types.ModuleType("src.INViTE.loader")
    sys.modules["src.INViTE.loader"] = loader
    tmp = tempfile.NamedTemporaryFile(suffix=".pt", delete=False)
    torch.save(dec_w, tmp.name)
    calls = []

    def capture(ids):
        calls[-1].append([int(t) for t in ids])
        return ref.decap._Tokenizer.decode(ids)

    try:
        for tag in IR.FORWARD_TOWERS:
            t = IR.TOWERS[tag]
            loader.load_invite_clip = lambda cfg, device=None, _m=towers[tag]: (_m, refshim._Callable(), None)
            model = ref.model.Patchioner.from_config(
                {"decap_weights": tmp.name, "prefix_size": 512, "support_memory_size": 0, "dino_model": "INViTE_" + tag, "normalize": False,
                 "resize_dim": t["crop"], "crop_dim": t["crop"], "clip_model_name": t["name"], "use_talk2dino_project": False,
                 "invite_config": {"name": t["name"], "jit": False, "extract_last_k_th_token": t["k"], "viz": False}}, device="cpu")
            model.eval()
            model.decoding_method = capture
            model.im_proj = make_projector(ref, bank / bank.norm(dim=-1, keepdim=True))
            meta[tag] = dict(backbone_type=model.backbone_type, patch_size=model.patch_size, embed_dim=model.embed_dim,
                             num_tokens=model.num_tokens, num_global_tokens=model.num_global_tokens)
            for name, kw in IR.FORWARD_CASES:
                calls.clear()
                orig = ref.model.decoding_batched

                def wrapped(*a, **k):
                    calls.append([])
                    return orig(*a, **k)

                ref.model.decoding_batched = wrapped
                try:
                    outs = model(IR.images(tag).clone(), **copy.deepcopy(IR.forward_args(kw, t["crop"])))
                finally:
                    ref.model.decoding_batched = orig
                key = tag + "__" + name
                meta[key] = outs
                arrs[key + "__ids"] = np.asarray([r for call in calls for r in call], dtype=np.int64).reshape(-1, 30)
                print(key, outs)
    finally:
        os.unlink(tmp.name)
    arrs["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    save("invite", **arrs)


if __name__ == "__main__":
    main()
