"""AlphaCLIP backbone on the MI355X: the region-mask kernel and the alpha-channel tower against the reference's own outputs
(tests/golden/alphaclip.npz), region captions against the float region driver (tests/alphaclip_ref.py) and the reference's ids, the
output structure of forward_alphaclip_with_regions, and the launch invariance of the batched region forwards."""
import json
import math
import os

import numpy as np
import pytest
import torch

import alphaclip_ref as AR
from parity_helpers import assert_ids_explained
from patchioner_amd import weights as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
C = AR.CASE


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "alphaclip.npz"))
    return {k: d[k] for k in d.files}


def _unpack(packed, n, grid):
    return np.unpackbits(packed, axis=1)[:, :grid * grid].reshape(n, grid, grid)


def _model(vit_dtype="fp16", use_cls=True, max_batch=4):
    from patchioner_amd import Patchioner
    bank = W.synth_bank(C["seed_bank"], C["bank_rows"], 512) * 2.0
    cfg = {"decap_weights": W.synth_decap(C["seed_dec"], prefix_size=512), "prefix_size": 512, "support_memory_size": C["bank_rows"],
           "dino_model": "AlphaClip", "normalize": False, "resize_dim": 224, "crop_dim": 224, "clip_model_name": "ViT-B/16",
           "use_talk2dino_project": False, "memory_bank": bank, "max_batch": max_batch, "vit_dtype": vit_dtype,
           "alphaclip_config": {"patch_size": 16, "name": C["name"], "use_cls_for_localized_captions": use_cls, "embed_dim": 512,
                                "alpha_vision_checkpoint": W.synth_alphaclip_vit(C["seed_vit"], C["name"], depth=C["depth"])}}
    return Patchioner.from_config(cfg, device="cuda")


def _imgs():
    return W.synth_images(C["seed_img"], C["B"], C["crop"]).cuda()


def _args(bboxes=False, traces=False, **kw):
    if bboxes:
        kw["bboxes"] = AR.region_boxes()
    if traces:
        kw["traces"] = AR.region_traces()
    return kw


@pytest.fixture(scope="module")
def m16():
    return _model("fp16")


@pytest.fixture(scope="module")
def m32():
    return _model("fp32")


def test_device_masks_match_the_reference_bitwise(m16, gold):
    eng = m16.engine
    regions = [([b], []) for b in AR.MASK_BOXES] + [([], [(p["x"], p["y"]) for p in t]) for t in AR.MASK_TRACES]
    for key, grid, div in (("mask_pix", 224, 1), ("mask_cell", 14, 16)):
        want = _unpack(gold[key], len(regions), grid)
        got = eng.region_masks(regions, grid, div).cpu().numpy()
        assert np.array_equal(got, want), key
    # a union of boxes and points is the OR of the single masks
    union = eng.region_masks([(AR.MASK_BOXES[1:4], [(0.9, 0.1), (0.5, 0.5)])], 224, 1)[0].cpu()
    want = AR.region_mask(AR.MASK_BOXES[1:4], [{"x": 0.9, "y": 0.1}, {"x": 0.5, "y": 0.5}], 224, 1)
    assert torch.equal(union, want)


@pytest.mark.parametrize("dtype,bound", [("fp16", 4e-3), ("fp32", 2e-5)])
def test_tower_tokens_match_the_reference(gold, dtype, bound, m16, m32):
    m = m16 if dtype == "fp16" else m32
    imgs = _imgs()
    masks = torch.from_numpy(_unpack(gold["tok_masks"], 3, 224)).cuda()
    tok = m.engine.vit_forward_regions(imgs, torch.tensor(gold["tok_img"][:3], dtype=torch.int32), masks)
    whole, _ = m.engine.vit_forward(imgs[:1], want_qkv=False)
    got = torch.cat([tok, whole]).cpu()[:, ::4].numpy()
    for r in range(4):
        err = np.abs(got[r] - gold["tokens"][r]).max() / np.abs(gold["tokens"][r]).max()
        print("AlphaCLIP %s tokens region %d: rel-max-err %.2e" % (dtype, r, err))
        assert err <= bound, (dtype, r, err)
    # the alpha channel is visible: the same image with an empty and a full mask gives different tokens
    zero = m.engine.vit_forward_regions(imgs, torch.tensor([0], dtype=torch.int32), torch.zeros(1, 224, 224, dtype=torch.uint8))
    d = float((zero[0] - whole[0]).abs().max() / whole[0].abs().max())
    assert d > 1e-2, d


def test_im2col_alpha_patch_embed_against_float64():
    """conv1(x) + conv1_alpha(alpha) through the alpha im2col and the patch-embed GEMM, in the fp32 parity mode: a one-block tower whose
    block is an identity (zero attention and MLP outputs) returns ln_post(ln_pre(patch embed + positions)) @ proj, restated in float64
    on the [x; alpha] columns."""
    sd = W.synth_alphaclip_vit(3, "ViT-B/16", depth=1)
    for k in ("attn.out_proj.weight", "attn.out_proj.bias", "mlp.c_proj.weight", "mlp.c_proj.bias"):
        sd["transformer.resblocks.0." + k] = torch.zeros_like(sd["transformer.resblocks.0." + k])
    from patchioner_amd.engine import Engine
    eng = Engine(embed_dim=768, depth=1, num_heads=12, num_registers=0, crop_dim=224, patch_size=16, pretrain_grid=14, prefix_size=512,
                 max_batch=2, vit_dtype="fp32", vit_arch="alphaclip", vit_out_dim=512, vit_ln_eps=1e-5)
    eng.load_state_dict(W.alphaclip_to_engine(sd))
    eng.finalize()
    imgs = W.synth_images(4, 2, 224)
    masks = torch.stack([AR.box_mask([30.5, 40.0, 90.0, 70.25], 224, 1), AR.trace_mask(AR.MASK_TRACES[2], 224)])
    got = eng.vit_forward_regions(imgs.cuda(), torch.tensor([1, 0], dtype=torch.int32), masks.cuda()).cpu().double()
    x = torch.cat([imgs[[1, 0]].double(), masks[:, None].double()], 1)
    w = torch.cat([sd["conv1.weight"], sd["conv1_alpha.weight"]], 1).double()
    e = torch.nn.functional.conv2d(x, w, stride=16).flatten(2).transpose(1, 2)
    e = torch.cat([sd["class_embedding"].double().expand(2, 1, -1), e], 1) + sd["positional_embedding"].double()
    ln = lambda t, p: torch.nn.functional.layer_norm(t, (768,), sd[p + ".weight"].double(), sd[p + ".bias"].double(), 1e-5)
    want = ln(ln(e, "ln_pre"), "ln_post") @ sd["proj"].double()
    err = float((got - want).abs().max() / want.abs().max())
    print("alpha patch embed (fp32 mode) vs float64: %.2e" % err)
    assert err <= 1e-5, err


def _alpha_rows_host(imgs, idx, masks, p, Kpad):
    """The four-channel patch rows restated with F.unfold: column c p^2 + py p + px, alpha as channel 3, zeros from 4 p^2 on."""
    x = torch.cat([imgs[idx.long()].float(), masks[:, None].float()], 1)
    rows = torch.nn.functional.unfold(x, kernel_size=p, stride=p).transpose(1, 2).reshape(-1, 4 * p * p)
    return torch.nn.functional.pad(rows, (0, Kpad - 4 * p * p))


# (tower, D, H, T, Tp, Tk, p, Kpad): ViT-B/16 (K 1024) and ViT-L/14 (4 p^2 = 784, padded to 896: the GEMMs take K in steps of 128)
ALPHA_SHAPES = [("B16", 768, 12, 197, 200, 256, 16, 1024), ("L14", 1024, 16, 257, 264, 320, 14, 896)]


@pytest.mark.parametrize("op", [0, 1], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", ALPHA_SHAPES, ids=[s[0] for s in ALPHA_SHAPES])
def test_alpha_im2col_and_patch_embed_gemm_against_float64(op, shape):
    """k_im2col_alpha in the operand type (pio_test_im2col_alpha): its rows carry exactly the operand-type values of the F.unfold
    restatement (images by index, the mask as channel 3, the pad columns untouched); then the patch-embed GEMM on those rows through every
    path that takes it, held to test_gpu_vit_kernels' float64 bar (vit_ref64.patch_embed64 on the [x; alpha] columns)."""
    import ctypes
    import test_gpu_vit_kernels as VK
    from patchioner_amd import _lib
    name, D, H, T, Tp, Tk, p, Kpad = shape
    S, R = 224, 3
    n2 = (S // p) ** 2
    dt = VK.OPS[op]
    imgs = W.synth_images(11 + op, 2, S).cuda()
    idx = torch.tensor([1, 0, 1], dtype=torch.int32, device="cuda")
    masks = torch.stack([AR.box_mask([30.5, 40.0, 90.0, 70.25], S, 1), AR.trace_mask(AR.MASK_TRACES[2], S),
                         torch.zeros(S, S, dtype=torch.uint8)]).cuda()
    A = torch.full((R * n2, Kpad), 0.0, dtype=dt, device="cuda")
    A[:, 4 * p * p:] = 7.0                                  # sentinel: the pad columns are not the kernel's
    L = _lib.load()
    _lib.check(L.pio_test_im2col_alpha(op, imgs.data_ptr(), idx.data_ptr(), masks.data_ptr(), R, S, p, Kpad, A.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    want = _alpha_rows_host(imgs, idx, masks, p, Kpad).to(dt)
    assert torch.equal(A[:, :4 * p * p], want[:, :4 * p * p]) and bool((A[:, 4 * p * p:] == 7.0).all())
    A[:, 4 * p * p:] = 0.0
    # conv1 | conv1_alpha as finalize_vit packs them, rounded once to the operand type
    g = torch.Generator().manual_seed(5 + op)
    w = torch.cat([torch.randn(D, 3 * p * p, generator=g), 2.0 * torch.randn(D, p * p, generator=g)], 1) / math.sqrt(4 * p * p)
    Wop = torch.nn.functional.pad(w, (0, Kpad - 4 * p * p)).to(dt).cuda().contiguous()
    bias = torch.zeros(D, device="cuda")                    # CLIP's conv1 has no bias
    c = VK.Case(op, VK.PE, R * n2, D, Kpad, D, H, T, Tp, Tk, 1, n2)
    c.pos = 0.1 * torch.randn(1 + n2, D, generator=g).cuda()
    label = "%s alpha patch embed %s" % (VK.OPN[op], name)
    first = None
    for path in c.paths():
        if not VK._fits(c, path):
            continue
        _, outs = c.run(path, A, Wop, bias)
        if first is None:
            first = (path, outs)
            VK._check_against(label + " " + VK.PN[path], outs, VK._reference(c, A, Wop, bias))
        else:
            assert VK._same_bits(outs["x"], first[1]["x"]) == 0, (label, path)
    assert first is not None, label + ": no GEMM path takes K = %d" % Kpad


def test_alpha_im2col_fp32_rows_are_exact():
    S, p, Kpad, R = 224, 16, 1024, 2
    from patchioner_amd import _lib
    imgs = W.synth_images(13, 2, S).cuda()
    masks = torch.stack([AR.box_mask([3.0, 5.0, 150.0, 70.0], S, 1), AR.trace_mask(AR.MASK_TRACES[0], S)]).cuda()
    out = torch.zeros(R * (S // p) ** 2, Kpad, device="cuda")
    for idx, m in ((None, masks), (torch.tensor([1, 1], dtype=torch.int32, device="cuda"), None)):
        _lib.check(_lib.load().pio_test_im2col_alpha(2, imgs.data_ptr(), idx.data_ptr() if idx is not None else None,
                                                     m.data_ptr() if m is not None else None, R, S, p, Kpad, out.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        ii = idx if idx is not None else torch.arange(R, dtype=torch.int32, device="cuda")
        mm = m if m is not None else torch.ones(R, S, S, dtype=torch.uint8, device="cuda")
        assert torch.equal(out, _alpha_rows_host(imgs, ii, mm, p, Kpad))


@pytest.mark.parametrize("dtype,bound", [("fp16", 4e-3), ("bf16", 3e-2)])
def test_vit_l14_alphaclip_runs(dtype, bound):
    """ViT-L/14 AlphaCLIP (D 1024, 16 heads, 4 p^2 = 784 alpha-embed columns) at depth 1: tokens of masked regions and of the whole
    image against the float tower, and a box / trace forward end to end."""
    from patchioner_amd import Patchioner
    sd = W.synth_alphaclip_vit(21, "ViT-L/14", depth=1)
    cfg = {"decap_weights": W.synth_decap(23, prefix_size=768), "prefix_size": 768, "support_memory_size": 1024, "dino_model": "AlphaClip",
           "normalize": False, "resize_dim": 224, "crop_dim": 224, "clip_model_name": "ViT-L/14", "use_talk2dino_project": False,
           "memory_bank": W.synth_bank(25, 1024, 768), "max_batch": 4, "vit_dtype": dtype,
           "alphaclip_config": {"name": "ViT-L/14", "patch_size": 14, "alpha_vision_checkpoint": sd, "embed_dim": 768}}
    m = Patchioner.from_config(cfg, device="cuda")
    assert (m.patch_size, m.num_tokens, m.token_dim) == (14, 257, 768)
    vit = AR.AlphaClipViTOracle(W.alphaclip_to_engine(sd), num_heads=16, patch_size=14)
    imgs = W.synth_images(27, 2, 224)
    masks = torch.stack([AR.box_mask([20.0, 30.0, 120.5, 90.0], 224, 1), AR.trace_mask(AR.MASK_TRACES[2], 224)])
    got = m.engine.vit_forward_regions(imgs.cuda(), torch.tensor([1, 0], dtype=torch.int32), masks.cuda()).cpu()
    whole, _ = m.engine.vit_forward(imgs.cuda(), want_qkv=False)
    for g_, ref in ((got, vit.tokens(imgs[[1, 0]], masks[:, None].float())), (whole.cpu(), vit.tokens(imgs))):
        err = float((g_ - ref).abs().max() / ref.abs().max())
        print("AlphaCLIP ViT-L/14 %s tokens: rel-max-err %.2e" % (dtype, err))
        assert err <= bound, err
    out = m(imgs.cuda(), bboxes=AR.region_boxes(), traces=AR.region_traces())
    assert [len(r) for r in out["bbox_capts"]] == [5, 5] and len(out["trace_capts"]) == 2
    assert all(isinstance(t, str) for r in out["bbox_capts"] for t in r)


CASES = [("boxes", True, dict(bboxes=True, get_cls_capt=True, compute_scores=True)),
         ("traces", True, dict(traces=True, get_cls_capt=False, compute_scores=True)),
         ("controllable", True, dict(bboxes=True, get_cls_capt=False, get_controllable_capts=True, compute_scores=True)),
         ("whole", True, dict(get_cls_capt=True, get_avg_patch_capt=True, compute_scores=True)),
         ("patches_boxes_traces", False, dict(bboxes=True, traces=True, compute_scores=True))]


@pytest.mark.parametrize("tag,use_cls,kw", CASES, ids=[c[0] for c in CASES])
def test_fp32_mode_ids_equal_the_reference(gold, tag, use_cls, kw, m32):
    m = m32 if use_cls else _model("fp32", use_cls=False)
    m.call_log = []
    outs = m(_imgs(), **_args(**kw))
    ids = torch.cat([i for _, i in m.call_log]).cpu().numpy()
    assert np.array_equal(ids, gold[tag + "__ids"]), tag
    meta = json.loads(bytes(gold["meta_json"]).decode())[tag]
    assert set(outs) == set(meta), (tag, set(outs), set(meta))
    for k in outs:
        if "capt" in k and "score" not in k:
            assert outs[k] == meta[k], (tag, k)


@pytest.mark.parametrize("tag,use_cls,kw", CASES, ids=[c[0] for c in CASES])
def test_fp16_ids_are_explained_by_the_float_driver(tag, use_cls, kw, m16):
    from oracle import patchioner_oracle as O
    from patchioner_amd.tokenizer import ClipDetokenizer
    m = m16 if use_cls else _model("fp16", use_cls=False)
    vit = AR.AlphaClipViTOracle(W.alphaclip_to_engine(W.synth_alphaclip_vit(C["seed_vit"], C["name"], depth=C["depth"])))
    bank = W.synth_bank(C["seed_bank"], C["bank_rows"], 512) * 2.0
    dec = O.DeCapOracle(W.synth_decap(C["seed_dec"], prefix_size=512))
    orc = O.PatchionerOracle(vit, dec, bank / bank.norm(dim=-1, keepdim=True), ClipDetokenizer().decode, normalize=False, crop_dim=224)
    ref = AR.AlphaClipRef(vit, orc, use_cls=use_cls)
    m.call_log, orc.call_log, orc.prefix_log = [], [], []
    a = _args(**kw)
    m(_imgs(), **a)
    if tag == "whole":
        orc.forward(_imgs().cpu(), get_cls_capt=True, get_avg_patch_capt=True)
    else:
        ref.forward(_imgs().cpu(), **{k: v for k, v in a.items() if k in ("bboxes", "traces", "get_controllable_capts")})
    assert_ids_explained(dec, m.call_log, orc.call_log, "AlphaCLIP %s" % tag, ref_prefixes=orc.prefix_log)


def test_output_structure_matches_the_reference(m16, gold):
    meta = json.loads(bytes(gold["meta_json"]).decode())
    boxes = AR.region_boxes()
    mine = boxes.clone()
    out = m16(_imgs(), bboxes=mine, traces=AR.region_traces(), compute_scores=True)
    assert torch.equal(mine, boxes) and meta["boxes_untouched"]             # the caller's boxes are not floor-divided
    assert list(out) == ["bbox_capts", "bbox_scores", "trace_capts", "trace_scores"]
    assert [len(r) for r in out["bbox_capts"]] == [5, 5] and len(out["trace_capts"]) == 2
    assert out["bbox_capts"][0][1] == "" and out["bbox_capts"][1][2] == ""
    assert out["bbox_scores"][0][1] == 0.0 and out["bbox_scores"][1][2] == 0.0
    assert set(m16(_imgs(), bboxes=boxes.clone(), traces=AR.region_traces())) == set(meta["boxes_traces"])
    with pytest.raises(TypeError):                   # traces_to_alpha_mask over the points of one trace (the reference fails the same way)
        m16(_imgs(), traces=AR.region_traces(), get_controllable_capts=True)
    assert meta["controllable_traces"] == {"__error__": "TypeError"}
    got = m16(_imgs(), traces=[[t] for t in AR.region_traces()], get_controllable_capts=True)
    assert len(got["set_controllable_capts"]) == len(meta["controllable_trace_lists"]["set_controllable_capts"]) == 2
    with pytest.raises(UnboundLocalError):
        m16(_imgs(), get_cls_capt=False, get_avg_self_attn_capt=True)
    with pytest.raises(NotImplementedError):
        m16.forward_async(_imgs(), traces=AR.region_traces())


def test_region_features_are_launch_invariant():
    """The features of a region do not depend on how the regions are split into launches: one call of 16 regions, one region per launch
    (max_batch 1) and launches of 3 give the same bits, on the CLS row and on the patch average."""
    imgs = W.synth_images(C["seed_img"], 4, 224).cuda()
    rng = np.random.RandomState(3)
    regions = []
    for r in range(16):
        xy = rng.uniform(-10, 200, size=2)
        wh = rng.uniform(0, 120, size=2)
        regions.append((r % 4, [[float(xy[0]), float(xy[1]), float(wh[0]), float(wh[1])]], [(0.1 * (r % 9), 0.5)]))
    feats = {}
    for mb in (16, 1, 3):
        for use_cls in (True, False):
            m = _model("fp16", use_cls=use_cls, max_batch=mb)
            feats[(mb, use_cls)] = m._alphaclip_region_feats(imgs, regions).cpu()
            m.engine.close()
    for use_cls in (True, False):
        for mb in (1, 3):
            assert torch.equal(feats[(16, use_cls)], feats[(mb, use_cls)]), (use_cls, mb)
