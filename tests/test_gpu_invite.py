"""INViTE backbone on the MI355X: the tower with self-only last blocks against the reference's own fp32 tokens and captions
(tests/golden/invite.npz), the V-only GEMM on its own against float64, and what must not move: k <= 0 is the CLIP engine bit for bit,
an image's tokens do not depend on the launch, and the asynchronous entry points caption what forward() captions."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import invite_ref as IR
import vit_ref64 as R
from parity_helpers import assert_ids_explained
from patchioner_amd import _lib
from patchioner_amd import weights as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
C = IR.CASE
TAGS = list(IR.TOWERS)
FWD = [(tag, name) for tag in IR.FORWARD_TOWERS for name, _ in IR.FORWARD_CASES]


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "invite.npz"))
    return {k: d[k] for k in d.files}


def _engine(tag, dtype, max_batch=2, self_only=None, sd=None):
    """The CLIP engine of tower case ``tag`` with its self-only count (``self_only`` overrides it: 0 = the plain CLIP tower)."""
    from patchioner_amd.engine import Engine
    t = IR.TOWERS[tag]
    D, _, heads, p, out, _ = W.invite_arch(t["name"])
    sd = sd if sd is not None else IR.tower_weights(tag)
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    k = IR.self_only_layers(t["k"], depth) if self_only is None else self_only
    eng = Engine(embed_dim=D, depth=depth, num_heads=heads, num_registers=0, crop_dim=t["crop"], patch_size=p,
                 pretrain_grid=t["crop"] // p, prefix_size=512, max_batch=max_batch, vit_dtype=dtype, vit_arch="clip", vit_out_dim=out,
                 vit_ln_eps=1e-5, vit_self_only_layers=k)
    eng.load_state_dict(sd)
    eng.finalize()
    return eng


_MODELS = {}


def _model(tag, dtype="fp16", max_batch=4):
    """Patchioner.from_config with the keys of configs/INViTE_B16_1layer.k.yaml (a state dict as checkpoint, the bank as a tensor)."""
    key = (tag, dtype, max_batch)
    if key not in _MODELS:
        from patchioner_amd import Patchioner
        t = IR.TOWERS[tag]
        ic = {"name": t["name"], "jit": False, "extract_last_k_th_token": t["k"], "viz": False,
              "checkpoint": W.synth_invite_vit(C["seed_vit"], t["name"], depth=C["depth"])}
        if t["resolution"] is not None:
            ic["resolution"] = t["resolution"]
        cfg = {"decap_weights": W.synth_decap(C["seed_dec"], prefix_size=512), "prefix_size": 512, "support_memory_size": C["bank_rows"],
               "dino_model": "INViTE_B16", "normalize": False, "resize_dim": t["crop"], "crop_dim": t["crop"], "clip_model_name": t["name"],
               "use_talk2dino_project": False, "linear_talk2dino": False, "memory_bank": W.synth_bank(C["seed_bank"], C["bank_rows"], 512),
               "max_batch": max_batch, "vit_dtype": dtype, "invite_config": ic}
        _MODELS[key] = Patchioner.from_config(cfg, device="cuda")
    return _MODELS[key]


@pytest.mark.parametrize("dtype,bound", [("fp16", 4e-3), ("bf16", 3e-2)])
@pytest.mark.parametrize("tag", TAGS)
def test_tower_tokens_match_the_reference(gold, tag, dtype, bound):
    """The project's CLIP-ViT bars: fp16 <= 4e-3, bf16 <= 3e-2 of max |ref|, for all four tower cases."""
    t = IR.TOWERS[tag]
    eng = _engine(tag, dtype)
    tok, _ = eng.vit_forward(IR.images(tag).cuda(), want_qkv=False)
    got, ref = tok.cpu()[:, ::t["stride"]].numpy(), gold[tag + "__tokens"]
    eng.close()
    assert got.shape == ref.shape
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("INViTE %s %s tokens: rel-max-err %.2e (bar %.0e)" % (tag, dtype, err, bound))
    assert err <= bound, (tag, dtype, err)


@pytest.mark.parametrize("tag", TAGS)
def test_fp32_mode_tokens_within_four_times_the_references_own_distance_from_float64(gold, tag):
    """The reference's fp32 tokens sit this far from a float64 evaluation of the same tower (tests/invite_ref.py in float64, measured on
    the CPU by tests/test_invite_cpu.py and recorded as invite_ref.REF_FP32_VS_F64, relative to max |ref|):
        b16_k1 6.58e-7   b16_r288_k1 9.36e-7   b32_k2 1.11e-6   b16_km1 6.66e-7
    The HIP fp32 mode computes the same sums in another fp32 order, so its bar -- against float64, and against the fixture -- is that
    distance times 4:
        b16_k1 2.63e-6   b16_r288_k1 3.74e-6   b32_k2 4.44e-6   b16_km1 2.66e-6
    Both comparisons need the same weights on both sides: the synthetic checkpoint is drawn with weights._cn, whose values do not depend
    on the host (trunc_normal_'s do, in the last bit, and behind the loader's fp16 rounding that bit moved these tokens by 1.8e-5)."""
    t = IR.TOWERS[tag]
    eng = _engine(tag, "fp32")
    tok, _ = eng.vit_forward(IR.images(tag).cuda(), want_qkv=False)
    got = tok.cpu()[:, ::t["stride"]].double().numpy()
    eng.close()
    ref = gold[tag + "__tokens"]
    t64 = IR.tower(tag, torch.float64).tokens(IR.images(tag))[:, ::t["stride"]].numpy()
    bar = 4.0 * IR.REF_FP32_VS_F64[tag]
    e64, eref = np.abs(got - t64).max() / np.abs(ref).max(), np.abs(got - ref).max() / np.abs(ref).max()
    print("INViTE %s fp32 mode: vs float64 %.3e, vs the reference's fp32 %.3e (bar %.3e)" % (tag, e64, eref, bar))
    assert e64 <= bar and eref <= bar, (tag, e64, eref, bar)


@pytest.mark.parametrize("tag,name", FWD, ids=["%s-%s" % f for f in FWD])
def test_fp32_mode_ids_and_strings_equal_the_reference(gold, tag, name):
    """No near-tie clause: the fp32 mode reproduces the reference's greedy ids and its strings."""
    m = _model(tag, "fp32")
    m.call_log = []
    outs = m(IR.images(tag).cuda(), **IR.forward_args(dict(IR.FORWARD_CASES)[name], IR.TOWERS[tag]["crop"]))
    ids = torch.cat([i for _, i in m.call_log]).cpu().numpy()
    key = tag + "__" + name
    assert np.array_equal(ids, gold[key + "__ids"]), key
    assert outs == json.loads(bytes(gold["meta_json"]).decode())[key], key


@pytest.mark.parametrize("tag,name", FWD, ids=["%s-%s" % f for f in FWD])
def test_fp16_ids_are_explained_by_the_float_driver(tag, name):
    m = _model(tag, "fp16")
    orc, dec = IR.driver(tag)
    kw = dict(IR.FORWARD_CASES)[name]
    crop = IR.TOWERS[tag]["crop"]
    m.call_log, orc.call_log, orc.prefix_log = [], [], []
    m(IR.images(tag).cuda(), **IR.forward_args(kw, crop))
    orc.forward(IR.images(tag), **IR.forward_args(kw, crop))
    assert_ids_explained(dec, m.call_log, orc.call_log, "INViTE %s %s" % (tag, name), ref_prefixes=orc.prefix_log)


def test_model_attributes_and_transforms():
    """P/src/model.py:217-229, 264-301, 459-485, 637-638: attributes from the model name, clip._transform(input_resolution)."""
    m = _model("b16_r288_k1", "fp16")
    assert (m.backbone_type, m.patch_size, m.embed_dim, m.token_dim, m.num_global_tokens, m.num_tokens) == ("INViTE", 16, 512, 512, 1, 325)
    assert (m.image_transforms.resize_dim, m.image_transforms.crop_dim) == (288, 288)
    assert m.image_transforms_no_crop.resize_dim == 288
    assert m.engine.cfg.vit_self_only_layers == 1 and m.engine.cfg.vit_arch == 1 and m.engine.cfg.pretrain_grid == 18
    assert tuple(float(v) for v in m.image_transforms.mean.reshape(-1)) == pytest.approx((0.48145466, 0.4578275, 0.40821073))
    imgs = IR.images("b16_r288_k1").cuda()
    for flag in ("get_avg_self_attn_capt", "get_attn_heads_capt"):          # no attention hook: as on the CLIP path
        with pytest.raises(UnboundLocalError):
            m(imgs, get_cls_capt=False, **{flag: True})
    with pytest.raises(UnboundLocalError):
        m(imgs, get_cls_capt=False, traces=IR.traces(), use_attention_tracing=True)
    with pytest.raises(AttributeError):
        m(imgs, bboxes=IR.boxes(288), double_DINO_for_bboxes=True)
    out = m(imgs, get_cls_capt=True, bboxes=IR.boxes(288), traces=IR.traces())
    assert len(out["cls_capt"]) == 2 and [len(r) for r in out["bbox_capts"]] == [4, 4] and len(out["trace_capts"]) == 2
    # the bigResize configuration: 592^2, 37 x 37 patches, T = 1370, the table resampled from the checkpoint's 14 x 14
    from patchioner_amd import Patchioner
    cfg = {"decap_weights": W.synth_decap(C["seed_dec"], prefix_size=512), "prefix_size": 512, "support_memory_size": 1024,
           "dino_model": "INViTE_B16", "normalize": False, "resize_dim": 592, "crop_dim": 592, "clip_model_name": "ViT-B/16",
           "use_talk2dino_project": False, "linear_talk2dino": False, "memory_bank": W.synth_bank(C["seed_bank"], 1024, 512), "max_batch": 2,
           "invite_config": {"name": "ViT-B/16", "jit": False, "extract_last_k_th_token": 1, "viz": False, "resolution": 592,
                             "checkpoint": W.synth_invite_vit(C["seed_vit"], "ViT-B/16", depth=2)}}
    big = Patchioner.from_config(cfg, device="cuda")
    assert big.num_tokens == 1370 and big.engine.T == 1370
    imgs = W.synth_images(C["seed_img"], 2, 592)
    tok, _ = big.engine.vit_forward(imgs.cuda(), want_qkv=False)
    tw = IR.InviteViTOracle(W.invite_to_engine(cfg["invite_config"]["checkpoint"], resolution=592), 12, 16, 1)
    ref = tw.tokens(imgs)
    err = float((tok.cpu() - ref).abs().max() / ref.abs().max())
    print("INViTE B/16 at 592^2 fp16 tokens vs the float tower: %.2e" % err)
    assert err <= 4e-3, err
    out = big(imgs.cuda(), get_cls_capt=True, bboxes=IR.boxes(592), traces=IR.traces())
    assert len(out["cls_capt"]) == 2 and [len(r) for r in out["bbox_capts"]] == [4, 4] and len(out["trace_capts"]) == 2
    big.engine.close()


# ---- the V-only GEMM on its own ------------------------------------------------------------------------------------------------
AUTO, NARROW, RES128, WIDE128, K256, ROLL = 0, 1, 2, 3, 4, 5
# (D, rows per image Tp): ViT-B/16 at 224^2 and ViT-L/14 at 224^2
VONLY_SHAPES = [(768, 200), (1024, 264)]


def _vonly(op, path, A, Wf, bf, out, M, D):
    taken = ctypes.c_int32(-7)
    rc = _lib.load().pio_test_vit_vonly(op, path, A.data_ptr(), Wf.data_ptr(), bf.data_ptr(), out.data_ptr(), M, D, ctypes.byref(taken),
                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, taken.value


@pytest.mark.parametrize("op", [0, 1], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D,Tp", VONLY_SHAPES, ids=["B16", "L14"])
def test_v_only_gemm_against_float64(op, D, Tp):
    """out = A Wv^T + bv through pio_test_vit_vonly, which is handed the FUSED in_proj and slices rows [2D, 3D) as the engine does, at
    16, 80 and 160 images' worth of rows (the dispatch takes the 128-wide kernel at 16 and the 256 x 256 kernel at 80 and 160) and at a
    row count that is no multiple of any tile, on every kernel that has the epilogue; the others refuse it.

    Bar, as tests/test_gpu_vit_kernels.py derives it for the GEMM family (u = 2^-24, K / 16 MFMA steps, two roundings per step, factor 2
    for the MFMA's internal order, two for the epilogue): c = 2 (2 K / 16 + 2), |got - ref| <= c u (sum_k |a||w| + |b|) + 1 ulp of the
    output type.  The q and k thirds of the fused weight are NaN: a kernel that read them could not pass.  Every path gives the same bits,
    and the guard bands around the output stay untouched."""
    import test_gpu_vit_kernels as VK
    dt = VK.OPS[op]
    g = torch.Generator(device="cuda").manual_seed(100 * op + D)
    Wf = torch.full((3 * D, D), float("nan"), dtype=dt, device="cuda")
    Wf[2 * D:] = (torch.randn(D, D, generator=g, device="cuda") * 0.05).to(dt)
    bf = torch.full((3 * D,), float("nan"), device="cuda")
    bf[2 * D:] = torch.randn(D, generator=g, device="cuda") * 0.1
    Wv, bv = Wf[2 * D:], bf[2 * D:]
    cK = 2.0 * (2.0 * D / 16 + 2)
    want_auto = {16: WIDE128, 80: K256, 160: K256}
    for imgs, M in ((16, 16 * Tp), (80, 80 * Tp), (160, 160 * Tp), (None, 16 * Tp - 8 * 13)):
        A = torch.randn(M, D, generator=g, device="cuda").to(dt)
        ref = R.gemm64(A, Wv) + bv.to(VK.F64)
        bar = cK * VK.U * (R.mag64(A, Wv) + bv.to(VK.F64).abs()) + VK._ulp(ref, op)
        first = None
        for path in (AUTO, WIDE128, K256):
            out = VK.Guarded((M, D), dt)
            rc, taken = _vonly(op, path, A, Wf, bf, out.t, M, D)
            _lib.check(rc)
            assert taken == (path if path != AUTO else taken) and taken in (WIDE128, K256)
            if path == AUTO and imgs is not None:
                assert taken == want_auto[imgs], (imgs, taken)
            label = "V-only %s D=%d M=%d %s" % (VK.OPN[op], D, M, VK.PN[taken])
            out.check(label, torch.ones(M, D, dtype=torch.bool, device="cuda"))
            got = out.t.clone()
            assert not bool(torch.isnan(got.float()).any()), label + ": NaN (the q / k thirds were read?)"
            VK._report(label + " (max err / bar)", float(((got.to(VK.F64) - ref).abs() / bar).max()), 1.0)
            if first is None:
                first = got
            else:
                assert VK._same_bits(got, first) == 0, label + ": bits differ between kernels"
        for path in (NARROW, RES128, ROLL):
            out = torch.zeros(M, D, dtype=dt, device="cuda")
            rc, _ = _vonly(op, path, A, Wf, bf, out, M, D)
            assert rc == -1 and b"WIDE128" in _lib.load().pio_last_error() and not bool(out.any()), (path, rc)
    assert _vonly(op, AUTO, A, Wf, bf, out, 64, 384)[0] == -1             # D % 256 != 0: nothing launched


def test_k_below_one_is_the_clip_engine_bit_for_bit():
    """extract_last_k_th_token = -1: no self-only block.  The tokens equal the existing vit_arch = 1 engine's, loaded with the same
    already-rounded weights and the same table, bit for bit; with k = 1 they do not."""
    sd = IR.tower_weights("b16_km1")
    imgs = IR.images("b16_km1").cuda()
    from patchioner_amd.engine import Engine
    clip = Engine(embed_dim=768, depth=C["depth"], num_heads=12, num_registers=0, crop_dim=224, patch_size=16, pretrain_grid=14,
                  prefix_size=512, max_batch=2, vit_dtype="fp16", vit_arch="clip", vit_out_dim=512, vit_ln_eps=1e-5)
    clip.load_state_dict(sd)
    clip.finalize()
    want, _ = clip.vit_forward(imgs, want_qkv=False)
    m = _model("b16_km1", "fp16")
    assert m.engine.cfg.vit_self_only_layers == 0
    got, _ = m.engine.vit_forward(imgs, want_qkv=False)
    assert torch.equal(got, want)
    k1, _ = _model("b16_k1", "fp16").engine.vit_forward(imgs, want_qkv=False)
    assert float((k1 - want).abs().max()) > 1e-2
    clip.close()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_tokens_do_not_depend_on_the_launch(dtype):
    """An image's tokens are the same bits in a launch of 16 and of 80 images (the V-only GEMM runs on the 128-wide kernel at 16 images
    and on the 256 x 256 kernel at 80, the other GEMMs change kernels too), and at any position in the batch."""
    eng = _engine("b16_k1", dtype, max_batch=80)
    imgs = W.synth_images(C["seed_img"] + 1, 80, 224).cuda()
    all80, _ = eng.vit_forward(imgs, want_qkv=False)
    first16, _ = eng.vit_forward(imgs[:16], want_qkv=False)
    assert torch.equal(first16, all80[:16])
    perm = torch.roll(torch.arange(80), 37).cuda()
    moved, _ = eng.vit_forward(imgs[perm].contiguous(), want_qkv=False)
    assert torch.equal(moved, all80[perm])
    late16, _ = eng.vit_forward(imgs[61:77].contiguous(), want_qkv=False)
    assert torch.equal(late16, all80[61:77])
    one, _ = eng.vit_forward(imgs[5:6].contiguous(), want_qkv=False)
    assert torch.equal(one[0], all80[5])
    eng.close()


def test_forward_async_and_the_pipeline_caption_what_forward_captions():
    from patchioner_amd.pipeline import TraceCaptionPipeline
    m = _model("b16_k1", "fp16")
    imgs, traces = IR.images("b16_k1").cuda(), IR.traces()
    want = m(imgs, get_cls_capt=False, traces=traces)["trace_capts"]
    assert m.forward_async(imgs, traces=traces).result()["trace_capts"] == want
    want_cls = m(imgs, get_cls_capt=True)["cls_capt"]
    assert m.forward_async(imgs, get_cls_capt=True).result()["cls_capt"] == want_cls
    batches = []
    for i, b in enumerate([2, 4, 3, 4, 1]):
        bi = W.synth_images(300 + i, b, 224).cuda()
        batches.append((bi, [IR.traces()[j % 2] for j in range(b)]))
    want = [m(bi, get_cls_capt=False, traces=tr)["trace_capts"] for bi, tr in batches]
    assert list(TraceCaptionPipeline(m, group_batches=2).run(batches)) == want
    assert list(TraceCaptionPipeline(m, group_batches=3, vit_batches=2).run(batches)) == want
    want = [m(bi, get_cls_capt=True)["cls_capt"] for bi, _ in batches]
    assert list(TraceCaptionPipeline(m, group_batches=2).run((bi, None) for bi, _ in batches)) == want
