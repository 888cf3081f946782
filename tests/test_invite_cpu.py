"""INViTE backbone, host side: the float tower (tests/invite_ref.py) against the reference's own fp32 tokens and captions
(tests/golden/invite.npz), the loader's rounding and position resampling, the identity the self-only block rests on, and every refusal
and default of ``invite_config`` -- all without a GPU."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import invite_ref as IR
from patchioner_amd import weights as W

torch.set_grad_enabled(False)
TAGS = list(IR.TOWERS)


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "invite.npz"))
    return {k: d[k] for k in d.files}


@pytest.mark.parametrize("tag", TAGS)
def test_float_tower_matches_the_reference_tokens(gold, tag):
    """Both are fp32 evaluations of the same weights: <= 1e-5 of max |ref|.  Also the distance of the REFERENCE's fp32 tokens from a
    float64 evaluation, which the GPU test of the fp32 mode takes its bar from (IR.REF_FP32_VS_F64: the recorded value holds)."""
    t = IR.TOWERS[tag]
    ref = gold[tag + "__tokens"]
    imgs = IR.images(tag)
    got = IR.tower(tag).tokens(imgs)[:, ::t["stride"]].numpy()
    assert got.shape == ref.shape
    err = np.abs(got - ref).max() / np.abs(ref).max()
    t64 = IR.tower(tag, torch.float64).tokens(imgs)[:, ::t["stride"]].numpy()
    d64 = np.abs(ref - t64).max() / np.abs(ref).max()
    print("INViTE %s: float tower vs reference %.2e; reference fp32 vs float64 %.3e (recorded %.3e)" % (tag, err, d64, IR.REF_FP32_VS_F64[tag]))
    assert err <= 1e-5, (tag, err)
    assert d64 <= IR.REF_FP32_VS_F64[tag] * 1.0001, (tag, d64)


def test_loader_rounds_exactly_what_convert_weights_names():
    sd = W.synth_invite_vit(5, "ViT-B/32", depth=2)
    eng = W.invite_to_engine(sd)
    rounded = {"patch_embed.proj.weight": "conv1.weight", "head.weight": "proj"}
    kept = {"cls_token": "class_embedding", "pos_embed": "positional_embedding", "norm_pre.weight": "ln_pre.weight",
            "norm_pre.bias": "ln_pre.bias", "norm.weight": "ln_post.weight", "norm.bias": "ln_post.bias"}
    for i in range(2):
        src, dst = "transformer.resblocks.%d." % i, "blocks.%d." % i
        for a, b in (("attn.in_proj_weight", "attn.qkv.weight"), ("attn.in_proj_bias", "attn.qkv.bias"), ("attn.out_proj.weight", "attn.proj.weight"),
                     ("attn.out_proj.bias", "attn.proj.bias"), ("mlp.c_fc.weight", "mlp.fc1.weight"), ("mlp.c_fc.bias", "mlp.fc1.bias"),
                     ("mlp.c_proj.weight", "mlp.fc2.weight"), ("mlp.c_proj.bias", "mlp.fc2.bias")):
            rounded[dst + b] = src + a
        for ln, nm in (("ln_1", "norm1"), ("ln_2", "norm2")):
            for leaf in ("weight", "bias"):
                kept["%s%s.%s" % (dst, nm, leaf)] = "%s%s.%s" % (src, ln, leaf)
    assert set(eng) == set(rounded) | set(kept)
    for k, s in rounded.items():
        want = sd[s].t() if s == "proj" else sd[s]
        assert torch.equal(eng[k].reshape(want.shape), want.half().float()), k
        assert not torch.equal(eng[k].reshape(want.shape), want), k + ": the synthetic values must not be fp16 already"
    for k, s in kept.items():
        assert torch.equal(eng[k].reshape(sd[s].shape), sd[s]), k
    # a full CLIP state dict: visual.* beside the text tower's keys, which are dropped
    full = {"visual." + k: v for k, v in sd.items()}
    full.update(W.synth_clip_text(7, "ViT-B/32", layers=1))
    full["logit_scale"] = torch.tensor(4.6)
    eng2 = W.invite_to_engine(full)
    assert set(eng2) == set(eng) and all(torch.equal(eng[k], eng2[k]) for k in eng)
    assert W.invite_dims(full) == (768, 2, 12, 32, 512, 7)
    with pytest.raises(NotImplementedError):
        W.invite_to_engine({"visual.layer1.0.conv1.weight": torch.zeros(1), "visual.attnpool.positional_embedding": torch.zeros(50, 8)})


def test_arch_table():
    assert W.invite_arch("ViT-B/32") == (768, 12, 12, 32, 512, 224)
    assert W.invite_arch("ViT-B/16") == (768, 12, 12, 16, 512, 224)
    assert W.invite_arch("ViT-L/14") == (1024, 24, 16, 14, 768, 224)
    assert W.invite_arch("ViT-L/14@336px") == (1024, 24, 16, 14, 768, 336)
    with pytest.raises(RuntimeError):
        W.invite_arch("ViT-H/14")
    sd = W.synth_invite_vit(1, "ViT-B/16", depth=1)
    assert sd["positional_embedding"].shape == (197, 768) and sd["proj"].shape == (768, 512) and sd["conv1.weight"].shape == (768, 3, 16, 16)
    assert "transformer.resblocks.0.attn.in_proj_weight" in sd and "transformer.resblocks.1.ln_1.weight" not in sd


def test_resized_position_table_matches_the_reference(gold):
    """resize_pos_embed: bicubic, align_corners=False, no antialias, the class row apart; the table arrives at the tower's own grid."""
    eng = IR.tower_weights("b16_r288_k1")
    pos = eng["pos_embed"][0]
    assert pos.shape == (1 + 18 * 18, 768)
    ref = gold["b16_r288_k1__pos"]
    got = pos[IR.POS_SAMPLE].numpy()
    assert got.shape == ref.shape
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("resampled position table vs reference: %.2e" % err)
    assert err <= 1e-6, err
    raw = W.synth_invite_vit(IR.CASE["seed_vit"], "ViT-B/16", depth=1)["positional_embedding"]
    assert torch.equal(pos[0], raw[0])                         # the class row is not resampled
    # the native resolution leaves the table alone
    assert torch.equal(IR.tower_weights("b16_k1")["pos_embed"][0], raw)
    assert torch.equal(W.invite_to_engine(W.synth_invite_vit(IR.CASE["seed_vit"], "ViT-B/16", depth=1), resolution=224)["pos_embed"][0], raw)


@pytest.mark.parametrize("tag", ["b16_k1", "b32_k2"])
def test_masked_attention_block_equals_the_v_only_form_bitwise(tag):
    """The reference's block -- torch.nn.MultiheadAttention under the mask that is -inf off the diagonal -- and
    x + out_proj(W_v ln_1(x) + b_v) are the same BITS in fp32, in the reference's own (sequence-first) layout: every softmax row is
    exactly one-hot, its product with V adds exact zeros to one V row, and the V third of the fused projection is the same sums."""
    tw = IR.tower(tag)
    x = tw.embed(IR.images(tag)).permute(1, 0, 2).contiguous()           # NLD -> LND, as VisionTransformer.forward does
    for i in range(tw.depth - tw.self_only, tw.depth):
        s = tw._ln(x, "blocks.%d.norm1" % i)
        masked, v_only = tw.masked_block_attention(i, s), tw.v_only_attention(i, s)
        assert masked.dtype == torch.float32 and torch.equal(masked, v_only), (tag, i, float((masked - v_only).abs().max()))
        assert torch.equal(x + masked, x + v_only)
        x = x + v_only
    # and it is not the unmasked block
    q = tw.attention(0, tw._ln(tw.embed(IR.images(tag)), "blocks.0.norm1"))
    D = tw.Dv
    v = F.linear(tw._ln(tw.embed(IR.images(tag)), "blocks.0.norm1"), tw.w["blocks.0.attn.qkv.weight"][2 * D:], tw.w["blocks.0.attn.qkv.bias"][2 * D:])
    assert float((q - v).abs().max()) > 1e-3


def test_float_driver_reproduces_the_reference_captions_without_near_ties(gold):
    """The float driver gives the reference's ids and strings for every forward() case, and no greedy step of them is a near-tie: the
    smallest top-2 margin stays above parity_helpers.MARGIN_BOUND, so that the fp32 mode can be held to exact ids and a departure of
    the fp16 mode can only be explained by its own perturbation (the seeds of invite_ref.CASE were chosen for that)."""
    from parity_helpers import MARGIN_BOUND
    meta = json.loads(bytes(gold["meta_json"]).decode())
    for tag in IR.FORWARD_TOWERS:
        t = IR.TOWERS[tag]
        assert meta[tag]["backbone_type"] == "INViTE" and meta[tag]["num_global_tokens"] == 1
        assert meta[tag]["num_tokens"] == 1 + (t["crop"] // meta[tag]["patch_size"]) ** 2 and meta[tag]["embed_dim"] == 512
        orc, dec = IR.driver(tag)
        for name, kw in IR.FORWARD_CASES:
            orc.call_log, orc.prefix_log = [], []
            outs = orc.forward(IR.images(tag), **IR.forward_args(kw, t["crop"]))
            key = tag + "__" + name
            assert np.array_equal(torch.cat(orc.call_log).numpy(), gold[key + "__ids"]), key
            assert outs == meta[key], key
            P = torch.cat(orc.prefix_log)
            _, _, margin = dec.decode_ids(P[torch.isfinite(P).all(1)], cached=True)
            print("INViTE %s: smallest top-2 margin of the reference's greedy steps %.3e" % (key, float(margin.min())))
            assert float(margin.min()) > MARGIN_BOUND, (key, float(margin.min()))


# ---- invite_config: refusals and defaults (P/src/model.py:217-229, 264-301, 459-485; INViTE/loader.py:44-45) -----------------
def _cfg(**ic):
    return {"decap_weights": None, "prefix_size": 512, "support_memory_size": 0, "dino_model": "INViTE_B16", "normalize": False,
            "resize_dim": 224, "crop_dim": 224, "clip_model_name": "ViT-B/16", "use_talk2dino_project": False, "synthetic_seed": 3,
            "invite_config": ic}


def _build(cfg):
    from patchioner_amd import Patchioner
    return Patchioner.from_config(cfg, device="cpu")


def test_refusals_come_before_the_device_is_touched():
    with pytest.raises(KeyError, match="name"):
        _build(_cfg(jit=False))
    with pytest.raises(NotImplementedError, match="jit"):
        _build(_cfg(name="ViT-B/16", jit=True))
    for rn in ("RN50", "RN101", "RN50x4"):
        with pytest.raises(NotImplementedError, match="ResNet"):
            _build(_cfg(name=rn))
    with pytest.raises(AttributeError, match="MultiheadAttentionViz"):
        _build(_cfg(name="ViT-B/16", viz=True))
    cfg = _cfg(name="ViT-B/16")
    cfg["synthetic_seed"] = None
    cfg["decap_weights"] = W.synth_decap(1, prefix_size=512, n_layer=1)
    with pytest.raises(FileNotFoundError, match="download"):
        _build(cfg)
    with pytest.raises(FileNotFoundError):
        _build(_cfg(name="ViT-B/16", checkpoint="/nonexistent/ViT-B-16.pt"))
    # crop_dim against the tower's grid: the reference's tensor-size error
    cfg = _cfg(name="ViT-B/16")
    cfg["crop_dim"] = cfg["resize_dim"] = 592
    with pytest.raises(RuntimeError, match=r"size of tensor a \(1370\) must match the size of tensor b \(197\)"):
        _build(cfg)
    with pytest.raises(RuntimeError, match=r"size of tensor a \(197\) must match the size of tensor b \(1370\)"):
        _build(_cfg(name="ViT-B/16", resolution=592))
    # with everything in order the constructor gets as far as the device, and says that there is no CPU path
    with pytest.raises(RuntimeError, match="MI355X"):
        _build(_cfg(name="ViT-B/16", extract_last_k_th_token=1))
    # DenseCLIP and ProxyCLIP keep raising
    cfg = _cfg(name="ViT-B/16")
    cfg["denseclip_config"] = {"x": 1}
    with pytest.raises(NotImplementedError):
        _build(cfg)


def test_setup_attributes_defaults_and_self_only_count(capsys):
    from patchioner_amd.backbones import _invite_setup
    sd16 = W.synth_invite_vit(1, "ViT-B/16", depth=3)
    s = _invite_setup({"name": "ViT-B/16", "checkpoint": sd16, "extract_last_k_th_token": 1}, 224, 224, None)
    assert (s.patch_size, s.embed_dim, s.token_dim, s.width, s.heads, s.depth, s.transform_resolution, s.engine_kw["vit_self_only_layers"]) == \
        (16, 512, 512, 768, 12, 3, 224, 1)
    assert capsys.readouterr().out == ""
    for k, want in ((-1, 0), (0, 0), (2, 2), (3, 3), (7, 3)):           # k <= 0: none; k >= layers: all of them
        assert _invite_setup({"name": "ViT-B/16", "checkpoint": sd16, "extract_last_k_th_token": k}, 224, 224, None).engine_kw["vit_self_only_layers"] == want
    assert _invite_setup({"name": "ViT-B/16", "checkpoint": sd16}, 224, 224, None).engine_kw["vit_self_only_layers"] == 0        # the default is -1
    # resolution: the table is resampled to the new grid and the transforms follow the tower
    s = _invite_setup({"name": "ViT-B/16", "checkpoint": sd16, "resolution": 288}, 288, 288, None)
    assert s.transform_resolution == 288 and s.state_dict["pos_embed"].shape == (1, 325, 768)
    # an unknown name: the reference's defaults, 32 / 512, each with its printed warning; the B/32 tower agrees with them
    sd32 = {"visual." + k: v for k, v in W.synth_invite_vit(2, "ViT-B/32", depth=1).items()}
    s = _invite_setup({"name": "my-clip", "checkpoint": sd32}, 224, 224, None)
    out = capsys.readouterr().out
    assert "Unknown INViTE model my-clip, using default patch size 32" in out
    assert "Unknown INViTE model my-clip, using default embedding dimension 512" in out
    assert (s.patch_size, s.embed_dim) == (32, 512)
    with pytest.raises(ValueError, match="patch_size 32"):              # ... a B/16 tower does not
        _invite_setup({"name": "my-clip", "checkpoint": sd16}, 224, 224, None)
    assert _invite_setup({"name": "ViT-L/14", "synthetic": 1, "checkpoint": W.synth_invite_vit(3, "ViT-L/14", depth=1)}, 224, 224, None).embed_dim == 768
    with pytest.raises(RuntimeError, match="not found"):                # synthetic weights need a name of the table
        _invite_setup({"name": "my-clip"}, 224, 224, 5)


def test_pio_create_rejects_a_bad_self_only_count():
    """The check sits in front of the device query, so it is reachable here."""
    from patchioner_amd import _lib
    lib = _lib.load()

    def create(arch, depth, k):
        cfg = _lib.PioConfig(embed_dim=768, depth=depth, num_heads=12, patch_size=16, num_registers=0, pretrain_grid=14, crop_dim=224,
                             vit_ln_eps=1e-5, readout_heads=16, readout_scale=0.125, dec_layers=4, dec_heads=4, dec_embd=768,
                             dec_vocab=50257, dec_positions=1024, prefix_size=512, dec_ln_eps=1e-5, max_batch=1, max_prefixes=8,
                             max_steps=30, vit_operand_type=0, device=0, vit_arch=arch, vit_out_dim=512, vit_self_only_layers=k)
        h = ctypes.c_void_p()
        rc = lib.pio_create(ctypes.byref(cfg), ctypes.byref(h))
        msg = lib.pio_last_error().decode()
        if rc == 0:
            lib.pio_destroy(h)
        return rc, msg

    for arch, depth, k in ((1, 12, 13), (1, 12, -1), (0, 12, 1), (2, 12, 1), (1, 3, 4)):
        rc, msg = create(arch, depth, k)
        assert rc == -1 and "vit_self_only_layers" in msg, (arch, depth, k, rc, msg)
    for arch, depth, k in ((1, 12, 12), (1, 12, 0), (1, 12, 1)):      # valid: whatever comes back is not this refusal
        rc, msg = create(arch, depth, k)
        assert rc == 0 or "vit_self_only_layers" not in msg, (arch, depth, k, rc, msg)
    assert ctypes.sizeof(_lib.PioConfig) == 4 * 31
