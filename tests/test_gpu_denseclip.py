"""DenseCLIP backbone on the MI355X: the plain CLIP ViT on the checkpoint's fp32 values against the reference's own fp32 tokens and
captions (tests/golden/denseclip.npz), the tower's true shape -- 640 x 640, 40 x 40 patches, T = 1601 -- against the float tower and
the region kernels at the grid of 40 against tests/region_ref64.py, and what must not move: an image's tokens do not depend on the
launch, and the asynchronous entry points caption what forward() captions."""
import json
import os

import numpy as np
import pytest
import torch

import denseclip_ref as DR
from parity_helpers import assert_ids_explained
from patchioner_amd import weights as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
C = DR.CASE
TAGS = list(DR.TOWERS)
FWD = [(tag, name) for tag in TAGS for name, _ in DR.FORWARD_CASES]


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "denseclip.npz"))
    return {k: d[k] for k in d.files}


def _engine(sd, res, dtype, max_batch=2):
    from patchioner_amd.engine import Engine
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    eng = Engine(embed_dim=C["width"], depth=depth, num_heads=C["width"] // 64, num_registers=0, crop_dim=res, patch_size=C["patch"],
                 pretrain_grid=res // C["patch"], prefix_size=512, max_batch=max_batch, vit_dtype=dtype, vit_arch="clip",
                 vit_out_dim=C["embed_dim"], vit_ln_eps=1e-5, sparse_clip_tail=True)
    eng.load_state_dict(sd)
    eng.finalize()
    return eng


_MODELS = {}


def _model(tag, dtype="fp16", max_batch=4):
    """Patchioner.from_config with the keys of configs/denseclip_B16_seg_40patches.k.yaml (the config as a dict, the checkpoint as a state
    dict, the bank as a tensor)."""
    key = (tag, dtype, max_batch)
    if key not in _MODELS:
        from patchioner_amd import Patchioner
        res = DR.TOWERS[tag]["resolution"]
        dec, bank = DR.decoder_and_bank()
        cfg = {"decap_weights": dec, "prefix_size": 512, "support_memory_size": C["bank_rows"], "dino_model": "INViTE_B16",
               "normalize": False, "resize_dim": res, "crop_dim": res, "clip_model_name": "ViT-B/16", "use_talk2dino_project": False,
               "linear_talk2dino": False, "memory_bank": bank, "max_batch": max_batch, "vit_dtype": dtype,
               "denseclip_config": DR.config(tag), "denseclip_checkpoint": DR.checkpoint(tag)}
        _MODELS[key] = Patchioner.from_config(cfg, device="cuda")
    return _MODELS[key]


@pytest.mark.parametrize("tag", TAGS)
def test_fp32_mode_tokens_within_four_times_the_references_own_distance_from_float64(gold, tag):
    """The reference's fp32 tokens sit this far from a float64 evaluation of the same tower (tests/denseclip_ref.py in float64, measured on
    the CPU by tests/test_denseclip_cpu.py and recorded as denseclip_ref.REF_FP32_VS_F64, relative to max |ref|):
        r128 7.25e-7   r224 6.91e-7
    The HIP fp32 mode computes the same sums in another fp32 order, so its bar -- against float64, and against the fixture -- is that
    distance times 4:
        r128 2.90e-6   r224 2.76e-6"""
    t = DR.TOWERS[tag]
    eng = _engine(DR.tower_weights(tag), t["resolution"], "fp32")
    tok, _ = eng.vit_forward(DR.images(tag).cuda(), want_qkv=False)
    got = tok.cpu()[:, ::t["stride"]].double().numpy()
    eng.close()
    ref = gold[tag + "__tokens"]
    t64 = DR.tower(tag, torch.float64).tokens(DR.images(tag))[:, ::t["stride"]].numpy()
    bar = 4.0 * DR.REF_FP32_VS_F64[tag]
    e64, eref = np.abs(got - t64).max() / np.abs(ref).max(), np.abs(got - ref).max() / np.abs(ref).max()
    print("DenseCLIP %s fp32 mode: vs float64 %.3e, vs the reference's fp32 %.3e (bar %.3e)" % (tag, e64, eref, bar))
    assert e64 <= bar and eref <= bar, (tag, e64, eref, bar)


@pytest.mark.parametrize("tag,name", FWD, ids=["%s-%s" % f for f in FWD])
def test_fp32_mode_ids_and_strings_equal_the_reference(gold, tag, name):
    """No near-tie clause: the fp32 mode reproduces the reference's greedy ids and its strings."""
    m = _model(tag, "fp32")
    m.call_log = []
    outs = m(DR.images(tag).cuda(), **DR.forward_args(dict(DR.FORWARD_CASES)[name], DR.TOWERS[tag]["resolution"]))
    ids = torch.cat([i for _, i in m.call_log]).cpu().numpy()
    key = tag + "__" + name
    assert np.array_equal(ids, gold[key + "__ids"]), key
    assert outs == json.loads(bytes(gold["meta_json"]).decode())[key], key


@pytest.mark.parametrize("dtype,bound", [("fp16", 4e-3), ("bf16", 3e-2)])
@pytest.mark.parametrize("tag", TAGS)
def test_tower_tokens_match_the_reference(gold, tag, dtype, bound):
    """The project's CLIP-ViT bars: fp16 <= 4e-3, bf16 <= 3e-2 of max |ref|."""
    t = DR.TOWERS[tag]
    eng = _engine(DR.tower_weights(tag), t["resolution"], dtype)
    tok, _ = eng.vit_forward(DR.images(tag).cuda(), want_qkv=False)
    got, ref = tok.cpu()[:, ::t["stride"]].numpy(), gold[tag + "__tokens"]
    eng.close()
    assert got.shape == ref.shape
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("DenseCLIP %s %s tokens: rel-max-err %.2e (bar %.0e)" % (tag, dtype, err, bound))
    assert err <= bound, (tag, dtype, err)


@pytest.mark.parametrize("tag,name", FWD, ids=["%s-%s" % f for f in FWD])
def test_fp16_ids_are_explained_by_the_float_driver(tag, name):
    m = _model(tag, "fp16")
    orc, dec = DR.driver(tag)
    kw = dict(DR.FORWARD_CASES)[name]
    res = DR.TOWERS[tag]["resolution"]
    m.call_log, orc.call_log, orc.prefix_log = [], [], []
    m(DR.images(tag).cuda(), **DR.forward_args(kw, res))
    orc.forward(DR.images(tag), **DR.forward_args(kw, res))
    assert_ids_explained(dec, m.call_log, orc.call_log, "DenseCLIP %s %s" % (tag, name), ref_prefixes=orc.prefix_log)


def test_model_attributes_and_transforms():
    """P/src/model.py:230-234, 277-283, 302-304, 497-513, 639-641, 864-865."""
    m = _model("r224", "fp16")
    assert (m.backbone_type, m.patch_size, m.embed_dim, m.token_dim, m.num_global_tokens, m.num_tokens, m.num_attn_heads) == \
        ("DenseClip", 16, 512, 512, 1, 197, 16)
    assert m.denseclip_config == DR.config("r224")
    assert (m.image_transforms.resize_dim, m.image_transforms.crop_dim, m.image_transforms_no_crop.resize_dim) == (224, 224, 224)
    assert tuple(float(v) for v in m.image_transforms.mean.reshape(-1)) == pytest.approx((0.48145466, 0.4578275, 0.40821073))
    cfg = m.engine.cfg
    assert (cfg.vit_arch, cfg.vit_self_only_layers, cfg.pretrain_grid, cfg.vit_out_dim, cfg.embed_dim) == (1, 0, 14, 512, 768)
    assert m.engine.sparse_ok and m.sparse_last_block
    imgs = DR.images("r224").cuda()
    for flag in ("get_avg_self_attn_capt", "get_attn_heads_capt"):          # no attention hook: as on the CLIP path
        with pytest.raises(UnboundLocalError):
            m(imgs, get_cls_capt=False, **{flag: True})
    with pytest.raises(UnboundLocalError):
        m(imgs, get_cls_capt=False, traces=DR.traces(), use_attention_tracing=True)
    with pytest.raises(AttributeError):
        m(imgs, bboxes=DR.boxes(224), double_DINO_for_bboxes=True)
    out = m(imgs, get_cls_capt=True, bboxes=DR.boxes(224), traces=DR.traces())
    assert len(out["cls_capt"]) == 2 and [len(r) for r in out["bbox_capts"]] == [4, 4] and len(out["trace_capts"]) == 2


# ---- the true shape: 640 x 640, 40 x 40 patches, T = 1601, Tp = 1608, Tk = 1664 ------------------------------------------------
@pytest.fixture(scope="module")
def tower640():
    ck = W.synth_denseclip_vit(311, 640, 2)
    vis = DR.vision(resolution=640, depth=2)
    eng = _engine(W.denseclip_to_engine(ck, vis), 640, "fp16", max_batch=3)
    yield eng, ck, vis
    eng.close()


def test_true_shape_tokens_against_the_float_tower(tower640):
    """The longest sequence any configuration asks of the ViT kernels: 26 key tiles, the last holding ONE real key.  Depth 2, B = 2, fp16,
    under the CLIP-ViT bar of 4e-3 of max |ref| against the fp32 float tower; every one of the 1601 tokens is compared."""
    eng, ck, vis = tower640
    assert (eng.n, eng.T, eng.Tp, eng.G, eng.D) == (40, 1601, 1608, 1, 512)
    imgs = W.synth_images(C["seed_img"] + 2, 2, 640)
    tok, _ = eng.vit_forward(imgs.cuda(), want_qkv=False)
    ref = DR.tower_from(ck, vis).tokens(imgs)
    assert tok.shape == ref.shape == (2, 1601, 512) and bool(torch.isfinite(tok).all())
    err = float((tok.cpu() - ref).abs().max() / ref.abs().max())
    print("DenseCLIP 640^2 fp16 tokens vs the float tower: %.2e (bar 4e-3)" % err)
    assert err <= 4e-3, err
    last = float((tok.cpu()[:, -1] - ref[:, -1]).abs().max() / ref.abs().max())          # the row that is the last tile's only key
    assert last <= 4e-3, last


def test_region_kernels_at_the_grid_of_40_against_float64(tower640):
    """trace_grids, region_reduce, the box weights in all four modes (and the single map) and the gaussian map at 40 x 40 = 1600 cells
    with G = 1 and 512-wide tokens, by the checks and under the operation-count bars of tests/test_gpu_region_kernels.py /
    tests/region_ref64.py, which this test runs on this engine.  (At 1600 cells the first 64 threads of the weight kernels hold a 7th
    cell: one serial add more than the 6 that region_ref64.SUM_DEPTH counts; the bars hold as they stand.)"""
    import test_gpu_region_kernels as RK
    eng = tower640[0]

    def get(name, *a, **k):
        return eng

    RK.test_trace_grids_at_cell_borders(get, "DenseCLIP640")
    RK.test_region_reduce_against_float64(get, "DenseCLIP640")
    RK.test_bbox_weights_against_float64(get, "DenseCLIP640")
    RK.test_gaussian_map_against_float64(get, "DenseCLIP640")


def test_the_clip_tower_is_refused_from_the_grid_of_43_without_a_launch():
    """1849 cells are above the 1792 the region kernels hold: an error before anything is launched, the output buffers keep their bits.
    (The other tower families keep their refusal above 1536 cells: tests/test_gpu_region_kernels.py.)"""
    import ctypes
    from patchioner_amd._lib import PioError, ptr
    from patchioner_amd.engine import Engine
    eng = Engine(embed_dim=768, depth=1, num_heads=12, num_registers=0, crop_dim=688, patch_size=16, pretrain_grid=43, prefix_size=512,
                 max_batch=1, vit_arch="clip", vit_out_dim=512, vit_ln_eps=1e-5)
    try:
        assert eng.n == 43
        lib, n2 = eng.lib, 1849
        boxes = torch.zeros(1, 1, 4, dtype=torch.int32, device="cuda")
        out, single = torch.full((n2,), 7.0, device="cuda"), torch.full((n2,), 7.0, device="cuda")
        tokens = torch.zeros(1, eng.T, 512, device="cuda")
        feat = torch.full((512,), 7.0, device="cuda")
        rm = torch.zeros(1, n2, dtype=torch.int32, device="cuda")
        assert lib.pio_bbox_weights(eng.h, ptr(boxes), 1, 1, 0, ctypes.c_float(0.5), None, None, ptr(out), 1, ptr(single), None) < 0
        assert b"grid of 43" in lib.pio_last_error()
        assert lib.pio_gaussian_map(eng.h, ctypes.c_float(0.5), ptr(out), None) < 0
        assert lib.pio_region_reduce(eng.h, ptr(tokens), 1, ptr(single), None, 1, ctypes.c_float(1.0), ptr(feat), None) < 0
        assert lib.pio_region_reduce_rows(eng.h, ptr(tokens), ptr(rm), ptr(single), None, 1, ctypes.c_float(1.0), ptr(feat), None) < 0
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((single == 7.0).all()) and bool((feat == 7.0).all())
        with pytest.raises(PioError):
            eng.gaussian_map(0.5)
    finally:
        eng.close()


def test_true_shape_tokens_do_not_depend_on_the_launch(tower640):
    """The same 640^2 image alone and at position 1 of a 3-image launch: the same bits."""
    eng = tower640[0]
    imgs = W.synth_images(C["seed_img"] + 3, 3, 640).cuda()
    three, _ = eng.vit_forward(imgs, want_qkv=False)
    one, _ = eng.vit_forward(imgs[1:2].contiguous(), want_qkv=False)
    assert torch.equal(one[0], three[1])


def test_forward_async_and_the_pipeline_caption_what_forward_captions():
    from patchioner_amd.pipeline import TraceCaptionPipeline
    m = _model("r224", "fp16")
    imgs, traces = DR.images("r224").cuda(), DR.traces()
    want = m(imgs, get_cls_capt=False, traces=traces)["trace_capts"]
    assert m.forward_async(imgs, traces=traces).result()["trace_capts"] == want
    want_cls = m(imgs, get_cls_capt=True)["cls_capt"]
    assert m.forward_async(imgs, get_cls_capt=True).result()["cls_capt"] == want_cls
    batches = []
    for i, b in enumerate([2, 4, 3, 4, 1]):
        bi = W.synth_images(300 + i, b, 224).cuda()
        batches.append((bi, [DR.traces()[j % 2] for j in range(b)]))
    want = [m(bi, get_cls_capt=False, traces=tr)["trace_capts"] for bi, tr in batches]
    assert list(TraceCaptionPipeline(m, group_batches=2).run(batches)) == want
    assert list(TraceCaptionPipeline(m, group_batches=3, vit_batches=2).run(batches)) == want
    want = [m(bi, get_cls_capt=True)["cls_capt"] for bi, _ in batches]
    assert list(TraceCaptionPipeline(m, group_batches=2).run((bi, None) for bi, _ in batches)) == want
