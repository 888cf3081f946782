"""RegionCLIP ModifiedResNet backbone on the MI355X: the convolution, pool and attnpool-input kernels against float64
(tests/regionclip_ref.py), the whole tower against the reference's fixture (tests/golden/regionclip.npz), launch invariance and the
captioning entry points."""
import os

import numpy as np
import pytest
import torch

import regionclip_ref as RR
from patchioner_amd import _lib
from patchioner_amd import weights as W

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "regionclip.npz")
LAYERS = (1, 1, 1, 1)
DT = {0: torch.float16, 1: torch.bfloat16, 2: torch.float32}
# unit roundoff of the operand type: the kernel's result is the float64 value up to one rounding per stored step
U = {0: 2.0 ** -11, 1: 2.0 ** -8, 2: 2.0 ** -24}


def _lib_():
    return _lib.load()


def _nhwc(x, cin_pad, dt):
    B, C, H, Wd = x.shape
    out = torch.zeros(B, H, Wd, cin_pad, dtype=dt)
    out[..., :C] = x.permute(0, 2, 3, 1).to(dt)
    return out.cuda()


def _wpack(w, cin_pad, dt):
    co, ci, k, _ = w.shape
    out = torch.zeros(co, k, k, cin_pad, dtype=dt)
    out[..., :ci] = w.permute(0, 2, 3, 1).to(dt)
    return out.cuda()


# (B, H, W, Cin, Cout, ks, stride, residual): Cin 3 (padded to 8) and 40 (K tails of 8 / 24), borders, stride 2, M not a tile multiple
CONV_SHAPES = [(2, 9, 7, 3, 40, 3, 2, False), (1, 13, 11, 40, 80, 3, 1, False), (3, 7, 7, 80, 40, 1, 1, True),
               (2, 14, 14, 64, 256, 1, 1, True), (1, 5, 5, 16, 33, 3, 1, False), (16, 7, 7, 512, 2048, 1, 1, True)]


@pytest.mark.parametrize("op", [0, 1, 2])
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv_kernel_against_float64(op, shape):
    B, H, Wd, cin, cout, ks, stride, resid = shape
    g = torch.Generator().manual_seed(hash(shape) % 1000 + op)
    dt, rnd = DT[op], (DT[op] if op < 2 else None)
    x = torch.randn(B, cin, H, Wd, generator=g).to(dt).double()
    x[:, :, 0, :] += 3.0                                             # asymmetric data: the borders are not like the middle
    x = x.to(dt).double()                                            # ... and still values of the operand type
    w = (torch.randn(cout, cin, ks, ks, generator=g) * (1.0 / (cin * ks * ks)) ** 0.5).to(dt).double()
    sc, sh = torch.rand(cout, generator=g) + 0.5, 0.3 * torch.randn(cout, generator=g)
    Ho, Wo = (H + 2 * (ks // 2) - ks) // stride + 1, (Wd + 2 * (ks // 2) - ks) // stride + 1
    res = torch.randn(B, cout, Ho, Wo, generator=g).to(dt).double() if resid else None
    want = RR.conv_ref(x, w, sc, sh, stride, res, True, rnd).permute(0, 2, 3, 1).numpy()
    cp = (cin + 7) // 8 * 8
    xd, wd = _nhwc(x, cp, dt), _wpack(w, cp, dt)
    rd = res.permute(0, 2, 3, 1).to(dt).contiguous().cuda() if resid else None
    scd, shd = sc.cuda(), sh.cuda()
    lib = _lib_()
    outs = []
    for tile in ([1, 2] if op < 2 else [0]):
        y = torch.full((B, Ho, Wo, cout), float("nan"), dtype=dt, device="cuda")
        _lib.check(lib.pio_test_conv(op, _lib.ptr(xd), _lib.ptr(wd), _lib.ptr(scd), _lib.ptr(shd), _lib.ptr(rd), _lib.ptr(y), None, B, H, Wd,
                                     cp, cout, ks, stride, 1, tile, None))
        torch.cuda.synchronize()
        outs.append(y.cpu())
    for y in outs[1:]:
        assert torch.equal(y, outs[0]), "the tile size changed bits"
    got = outs[0].double().numpy()
    # derived bound: the conv sum is exact-product fp32 accumulation (K <= 720 terms: <= K 2^-24 sum|x w|), then <= 3 roundings to the
    # operand type on values of size |y|, each half an ulp; and the float64 statement may sit across one rounding boundary
    # on values of the size of each intermediate (the conv times the scale, the shift, the residual: a BN shift can cancel most of them)
    sumabs = torch.nn.functional.conv2d(x.abs(), w.abs(), stride=stride, padding=ks // 2).permute(0, 2, 3, 1).numpy()
    pre = torch.nn.functional.conv2d(x, w, stride=stride, padding=ks // 2).permute(0, 2, 3, 1).abs().numpy() * sc.numpy()
    mag = pre + np.abs(sh.numpy()) + (res.permute(0, 2, 3, 1).abs().numpy() if resid else 0) + np.abs(want)
    bound = (cin * ks * ks * 2.0 ** -24 * sumabs * (np.abs(sc.numpy()) + 1)) + 4 * U[op] * mag + 1e-30   # one ulp (2U) per rounding
    assert np.isfinite(got).all()
    assert (np.abs(got - want) <= bound).all(), float((np.abs(got - want) / bound).max())


@pytest.mark.parametrize("op", [0, 1, 2])
def test_avgpool_and_attnpool_input_against_float64(op):
    dt, rnd = DT[op], (DT[op] if op < 2 else None)
    g = torch.Generator().manual_seed(7 + op)
    x = torch.randn(3, 40, 10, 6, generator=g).to(dt).double()
    lib = _lib_()
    xd = x.permute(0, 2, 3, 1).to(dt).contiguous().cuda()
    y = torch.empty(3, 5, 3, 40, dtype=dt, device="cuda")
    _lib.check(lib.pio_test_avgpool(op, _lib.ptr(xd), 3, 10, 6, 40, _lib.ptr(y), None))
    want = RR.avgpool_ref(x, rnd if op < 2 else torch.float32).permute(0, 2, 3, 1)      # fp32 mode: one fp32 rounding
    if op < 2:
        assert torch.equal(y.cpu().double(), want)    # fp16 / bf16 inputs: the fp32 sum of 4 is exact, one rounding -- the same bits
    else:                                             # fp32: three fp32 additions against one float64 rounding
        assert ((y.cpu().double() - want).abs() <= 4 * U[2] * x.abs().max()).all()
    HW, C, Tp = 15, 40, 24
    x5 = torch.randn(2, C, 5, 3, generator=g).to(dt).double()
    pos = torch.randn(HW + 1, C, generator=g) / 7
    x5d = x5.reshape(2, C, HW).permute(0, 2, 1).to(dt).contiguous().cuda()
    out = torch.full((2, Tp, C), float("nan"), dtype=dt, device="cuda")
    _lib.check(lib.pio_test_attnpool_in(op, _lib.ptr(x5d), _lib.ptr(pos.cuda()), 2, HW, C, Tp, _lib.ptr(out), None))
    torch.cuda.synchronize()
    got = out.cpu().double()
    want = RR.attnpool_in_ref(x5, pos, rnd if op < 2 else torch.float32)
    assert torch.equal(got[:, 1 + HW:], torch.zeros(2, Tp - 1 - HW, C, dtype=torch.float64))
    assert torch.equal(got[:, 1:1 + HW], want[:, 1:])        # one rounding of x + rnd(pos)
    # the mean row: a sum of 15 in fp32 (order may differ from float64 by 15 2^-24), then two roundings
    assert (got[:, 0] - want[:, 0]).abs().max() <= 2 * U[op] * (want[:, 0].abs().max() + 1) + 1e-6


def _engine(name, res, op, max_batch=4, spatial=True, seed=None):
    from patchioner_amd.engine import Engine
    seed = {"RN50": 11, "RN50x4": 12}[name] if seed is None else seed
    sd = W.synth_regionclip_rn(seed, name, layers=LAYERS, image_resolution=res)
    _, width, embed, heads, out_dim = W.regionclip_arch(name)
    eng = Engine(embed_dim=embed, depth=4, num_heads=heads, num_registers=0, crop_dim=res, patch_size=32, pretrain_grid=res // 32,
                 max_batch=max_batch, vit_dtype={0: "fp16", 1: "bf16", 2: "fp32"}[op], vit_arch="regionclip", vit_out_dim=out_dim,
                 rn_layers=LAYERS, rn_width=width, rn_attnpool_spatial=spatial)
    eng.load_state_dict(W.regionclip_to_engine(sd), strict=True)
    eng.finalize()
    return eng, sd


@pytest.mark.parametrize("name,res", [("RN50", 224), ("RN50x4", 288)])
def test_tower_tokens_against_the_reference_fixture(name, res):
    g = np.load(GOLD)
    seed = {"RN50": 11, "RN50x4": 12}[name]
    imgs = W.synth_images(seed + 100, 1, res)
    r16, r32 = g["%s_%d_tok16" % (name, res)].astype(np.float64), g["%s_%d_tok32" % (name, res)].astype(np.float64)
    gap = np.abs(r16 - r32).max()            # what fp16 rounding alone moves the reference's own tokens
    eng, _ = _engine(name, res, 0)
    t16 = eng.vit_forward(imgs, want_qkv=False)[0].cpu().double().numpy()
    e16 = np.abs(t16 - r16).max()
    # both are fp16 towers rounding at the same places; they differ by the order of the sums (and the MFMA's fp32 partial sums
    # against the CPU's): stated bound 4 x the fp16-vs-fp32 gap
    assert t16.shape == r16.shape and e16 < 4 * gap, (e16, gap)
    eng.close()
    eng, _ = _engine(name, res, 2)
    t32 = eng.vit_forward(imgs, want_qkv=False)[0].cpu().double().numpy()
    e32 = np.abs(t32 - r32).max()
    # exact fp32 operands against the reference's fp32 run: only the order of fp32 sums differs (see test_regionclip_cpu's float64 bar)
    assert e32 < 2e-5 and e32 < gap / 4, (e32, gap)
    eng.close()
    print("regionclip %s@%d: fp16 %.2e, fp32 %.2e (fp16-vs-fp32 gap of the reference %.2e)" % (name, res, e16, e32, gap))


def test_cproj_patch_rows_without_attention():
    g = np.load(GOLD)
    imgs = W.synth_images(111, 1, 224)
    eng, _ = _engine("RN50", 224, 0, spatial=False)
    t = eng.vit_forward(imgs, want_qkv=False)[0].cpu().double().numpy()
    gap = np.abs(g["RN50_224_tok16"].astype(np.float64) - g["RN50_224_tok32"]).max()
    assert np.abs(t - g["RN50_224_cproj_tok16"]).max() < 4 * gap
    eng.close()


@pytest.mark.parametrize("op", [0, 2])
def test_tokens_are_bitwise_launch_invariant(op):
    imgs = W.synth_images(5, 7, 224)
    eng, _ = _engine("RN50", 224, op, max_batch=3)
    full = eng.vit_forward(imgs, want_qkv=False)[0]                         # launches of 3, 3, 1
    singles = torch.cat([eng.vit_forward(imgs[i:i + 1], want_qkv=False)[0] for i in range(7)])
    rev = eng.vit_forward(imgs.flip(0), want_qkv=False)[0].flip(0)
    assert torch.equal(full, singles) and torch.equal(full, rev)
    eng.close()


def _model(vit_dtype="fp16", **kw):
    from patchioner_amd import Patchioner
    rc = {"patch_size": 32, "use_attnpool_for_spatial_feats": True, "embed_dim": 1024,
          "checkpoint": W.synth_regionclip_rn(11, "RN50", layers=LAYERS),
          "MODEL": {"RESNETS": {"OUT_FEATURES": ["res4", "res5"], "IMAGE_RESOLUTION": 224}}}
    cfg = {"prefix_size": 1024, "support_memory_size": 2048, "normalize": False, "resize_dim": 224, "crop_dim": 224,
           "dino_model": "regionclip_resnet50_p32.k", "regionclip_config": rc, "synthetic_seed": 3, "max_batch": 2,
           "vit_dtype": vit_dtype, "use_talk2dino_project": False}
    cfg.update(kw)
    return Patchioner.from_config(cfg, device="cuda")


def test_patchioner_structure_and_captions():
    m = _model()
    assert m.backbone_type == 'RegionCLIP' and m.num_global_tokens == 5 and m.num_tokens == 5 + 49 and m.patch_size == 32
    assert m.embed_dim == 1024 and m.engine.T == 50
    imgs = W.synth_images(0, 3, 224)
    traces = [[{"x": 0.1, "y": 0.2}, {"x": 0.6, "y": 0.7}], [{"x": 0.9, "y": 0.1}], [{"x": 0.5, "y": 0.5}]]
    out = m(imgs.cuda(), get_cls_capt=True, get_patch_capts=True, traces=traces)
    assert len(out["cls_capt"]) == 3 and all(isinstance(c, str) for c in out["cls_capt"])
    assert [len(p) for p in out["patch_tokens_capts"]] == [49, 49, 49]       # 1 cls row + 49 patches: no patch dropped
    assert len(out["trace_capts"]) == 3
    # the cls caption of one image does not depend on the others in the call
    one = m(imgs[1:2].cuda(), get_cls_capt=True)
    assert one["cls_capt"][0] == out["cls_capt"][1]
    boxes = torch.tensor([[[10, 20, 100, 80], [0, 0, 224, 224]]] * 3, dtype=torch.float32)
    from PIL import Image
    pil = [Image.fromarray(np.random.RandomState(i).randint(0, 255, (240, 260, 3), dtype=np.uint8)) for i in range(3)]
    caps = m.caption_bboxes(pil, boxes, "cls_capt")      # the main table's dense row: crop, preprocess, cls caption per box
    caps = caps["bbox_capts"]
    assert len(caps) == 3 and all(len(c) == 2 and all(isinstance(t, str) for t in c) for c in caps)
    # no attention hook: the options that read it fail as they do on the reference's CLIP backbones
    with pytest.raises(UnboundLocalError):
        m(imgs.cuda(), get_cls_capt=False, get_avg_self_attn_capt=True)
    with pytest.raises(AttributeError):
        m(imgs.cuda(), get_cls_capt=False, bboxes=boxes, double_DINO_for_bboxes=True)


# the reference's Patchioner.forward ids recorded by tools/oracle/gen_golden_regionclip.py (its CAPTION_CASES / caption_inputs)
CAPTION_RUNS = [("RN50", 224, 11, "cls_traces"), ("RN50", 224, 11, "boxes"), ("RN50x4", 288, 12, "cls_traces"), ("RN50", 512, 13, "cls_traces")]
BANK_ROWS = 2048


def _caption_inputs(name, res, seed):
    out_dim = W.regionclip_arch(name)[4]
    imgs = W.synth_images(seed + 200, 2, res)
    traces = [[{"x": 0.1, "y": 0.2}, {"x": 0.55, "y": 0.6}, {"x": 0.8, "y": 0.3}], [{"x": 0.9, "y": 0.85}, {"x": 0.3, "y": 0.7}]]
    q = res // 8
    boxes = torch.tensor([[[q, q, 3 * q, 2 * q], [0, 0, res, res], [4 * q, 2 * q, 2 * q, 5 * q]],
                          [[2 * q, 3 * q, 4 * q, 4 * q], [q, 0, q, q], [0, 5 * q, 7 * q, 2 * q]]], dtype=torch.float32)
    return imgs, traces, boxes, W.synth_decap(seed + 300, prefix_size=out_dim), W.synth_bank(seed + 400, BANK_ROWS, out_dim)


def _case_model(name, res, seed, vit_dtype):
    from patchioner_amd import Patchioner
    out_dim = W.regionclip_arch(name)[4]
    _, _, _, dec, bank = _caption_inputs(name, res, seed)
    rc = {"patch_size": 32, "embed_dim": out_dim, "checkpoint": W.synth_regionclip_rn(seed, name, layers=LAYERS, image_resolution=res),
          "MODEL": {"RESNETS": {"OUT_FEATURES": ["res4", "res5"], "IMAGE_RESOLUTION": res}}}
    return Patchioner.from_config({"decap_weights": dec, "prefix_size": out_dim, "support_memory_size": BANK_ROWS, "memory_bank": bank,
                                   "normalize": False, "resize_dim": res, "crop_dim": res, "dino_model": "regionclip_resnet50_p32.k",
                                   "regionclip_config": rc, "max_batch": 2, "vit_dtype": vit_dtype, "use_talk2dino_project": False},
                                  device="cuda")


def _kw(tag, traces, boxes):
    return dict(get_cls_capt=True, traces=traces) if tag == "cls_traces" else dict(get_cls_capt=False, bboxes=boxes.clone())


@pytest.mark.parametrize("name,res,seed,tag", CAPTION_RUNS, ids=["%s@%d-%s" % (c[0], c[1], c[3]) for c in CAPTION_RUNS])
def test_fp32_mode_ids_equal_the_reference(name, res, seed, tag):
    """exact fp32 operands: the tower, the 640 / 1024-wide projection and the decoder's prefix projection give the reference's ids"""
    ref = np.load(GOLD)["ids_%s_%d_%s" % (name, res, tag)]
    imgs, traces, boxes, _, _ = _caption_inputs(name, res, seed)
    m = _case_model(name, res, seed, "fp32")
    m.call_log = []
    m(imgs.cuda(), **_kw(tag, traces, boxes))
    ids = torch.cat([i for _, i in m.call_log]).cpu().numpy()
    assert ids.shape == ref.shape and np.array_equal(ids, ref)
    m.engine.close()


class _TowerOracle:
    """the float64 restatement (tests/regionclip_ref.py) as the PatchionerOracle's backbone: no attention hook, no registers"""
    has_attention = False
    R = 0
    patch_size = 32

    def __init__(self, sd, heads, out_dim):
        self.sd, self.heads, self.D, self.last_qkv = sd, heads, out_dim, None

    def __call__(self, imgs):
        t = RR.tokens64(self.sd, imgs, LAYERS, self.heads).float()
        return {"x_norm_clstoken": t[:, 0], "x_norm_regtokens": t[:, 1:1], "x_norm_patchtokens": t[:, 1:]}


@pytest.mark.parametrize("name,res,seed,tag", CAPTION_RUNS, ids=["%s@%d-%s" % (c[0], c[1], c[3]) for c in CAPTION_RUNS])
def test_fp16_ids_are_explained_by_the_float_driver(name, res, seed, tag):
    from oracle import patchioner_oracle as O
    from parity_helpers import assert_ids_explained
    from patchioner_amd.tokenizer import ClipDetokenizer
    _, _, _, heads, out_dim = W.regionclip_arch(name)
    imgs, traces, boxes, dec_w, bank = _caption_inputs(name, res, seed)
    sd = W.regionclip_to_engine(W.synth_regionclip_rn(seed, name, layers=LAYERS, image_resolution=res))
    dec = O.DeCapOracle(dec_w)
    orc = O.PatchionerOracle(_TowerOracle(sd, heads, out_dim), dec, bank / bank.norm(dim=-1, keepdim=True), ClipDetokenizer().decode,
                             normalize=False, crop_dim=res)
    m = _case_model(name, res, seed, "fp16")
    m.call_log, orc.call_log, orc.prefix_log = [], [], []
    m(imgs.cuda(), **_kw(tag, traces, boxes))
    orc.forward(imgs, **_kw(tag, traces, boxes))
    assert_ids_explained(dec, m.call_log, orc.call_log, "RegionCLIP %s@%d %s" % (name, res, tag), ref_prefixes=orc.prefix_log)
    m.engine.close()


def test_forward_async_and_pipeline_equal_forward():
    from patchioner_amd.pipeline import TraceCaptionPipeline
    m = _model()
    batches = []
    for i, b in enumerate([2, 1, 2]):
        imgs = W.synth_images(40 + i, b, 224).cuda()
        batches.append((imgs, [[{"x": 0.1 + 0.2 * j, "y": 0.3}, {"x": 0.8, "y": 0.9 - 0.1 * j}] for j in range(b)]))
    want = [m(imgs, get_cls_capt=False, traces=tr)["trace_capts"] for imgs, tr in batches]
    pend = [m.forward_async(imgs, get_cls_capt=False, traces=tr) for imgs, tr in batches]
    assert [p.result()["trace_capts"] for p in pend] == want
    assert list(TraceCaptionPipeline(m, group_batches=2).run(batches)) == want
    want_cls = [m(imgs, get_cls_capt=True)["cls_capt"] for imgs, _ in batches]
    assert list(TraceCaptionPipeline(m, group_batches=2).run((imgs, None) for imgs, _ in batches)) == want_cls
