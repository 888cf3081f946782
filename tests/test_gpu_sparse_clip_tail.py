"""The sparse tail of the CLIP towers (pio_vit_forward_rows on ``vit_arch = 1``): for trace regions the last block's query rows, attention
output, proj, ln_2, fc1 + QuickGELU, fc2, then ln_post and the exact-fp32 768 -> 512 head run only on the rows whose patches a trace
touches.  The invariant is SAME BITS: every selected token is the dense forward's -- the head included, whose k_sgemm_tn output row is a
function of its own input row alone -- so region embeddings, prefixes, ids and captions are too.  With G = 1 the patch p sits at row
1 + p: a quad holds the class row and three patches, and the tokens are Dout = 512 wide behind a D = 768 tower.  All comparisons here
are torch.equal; the checks are those of tests/test_gpu_sparse_last_block.py, whose helpers this file uses."""
import numpy as np
import pytest
import torch

import denseclip_ref as DR
import golden_cases as gc
from patchioner_amd import weights as W
from test_gpu_sparse_last_block import _check_sparse_equals_dense, _selected_rows

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _engine(crop=224, patch=16, depth=2, max_batch=3, dtype="fp16", seed=17, sparse=True, self_only=0):
    """A CLIP-arch tower of width 768 with the 512-wide head, synthetic fp32 weights, the table at its own grid."""
    from patchioner_amd.engine import Engine
    n = crop // patch
    e = Engine(embed_dim=768, depth=depth, num_heads=12, num_registers=0, crop_dim=crop, patch_size=patch, pretrain_grid=n, prefix_size=512,
               max_batch=max_batch, vit_dtype=dtype, vit_arch="clip", vit_out_dim=512, vit_ln_eps=1e-5, vit_self_only_layers=self_only,
               sparse_clip_tail=sparse)
    e.load_state_dict(W._openai_visual_to_engine(W.synth_invite_tower(seed, 768, depth, patch, 512, n)))
    e.finalize()
    return e


def _edge_traces(n):
    """two launches of three images on an n x n grid: blocks at patch column 0 and ending at column n - 1, a block whose runs straddle
    quad boundaries ((1 + gx + n gy) % 4 != 0 with G = 1), a single point; points outside [0, 1] (and on its closed ends), an image without
    points, an inner block.  Blocks are 2 x 2 on the grid of 8, so that the selection stays under the cut-over share."""
    side = 2 if n <= 8 else 4
    a = [gc.block_trace(0, 1, n=n, side=side) + gc.block_trace(n - side, n - side - 1, n=n, side=side),
         gc.block_trace(2, 3, n=n, side=side), [dict(x=0.53, y=0.41)]]
    b = [gc.trace_cases()[0][1], [], gc.block_trace(n // 2 - 1, n // 2, n=n, side=side)]
    return a, b


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("crop", [128, 224], ids=["grid8-T65", "grid14-T197"])
def test_compact_tokens_are_the_dense_tokens_bit_for_bit(crop, dtype):
    e = _engine(crop=crop, dtype=dtype, seed=91)
    n = e.n
    assert e.sparse_ok and (e.G, e.D, e.Dv) == (1, 512, 768) and e.T == 1 + n * n
    imgs = W.synth_images(5, 3, crop).cuda()
    for traces in _edge_traces(n):
        emb, g = _check_sparse_equals_dense(e, imgs, traces)
        for bi in range(3):
            if not (g[bi] != 0).any():
                assert (emb[bi] == 0).all()                # an empty trace: a zero embedding, as on the dense path
    # the straddling block really straddles, the edge blocks reach both edges, and the class row rides in the first quad
    side = 2 if n <= 8 else 4
    _, sel = e.trace_grids(_edge_traces(n)[0], select_rows=True)
    rows, img_off = _selected_rows(sel, 3)
    t1 = rows[4 * img_off[1]:4 * img_off[2]] % e.Tp
    assert len(t1) == 4 * 2 * side                         # `side` runs, each over two quads
    t0 = rows[4 * img_off[0]:4 * img_off[1]] % e.Tp
    assert 1 + 1 * n + 0 in t0 and 1 + (n - side - 1) * n + (n - 1) in t0
    _, sel = e.trace_grids([[dict(x=0.0, y=0.0)], [], []], select_rows=True)
    rows, _ = _selected_rows(sel, 3)
    assert rows.tolist() == [0, 1, 2, 3]                   # patch 0 is row 1: its quad starts at the class row
    e.close()


def test_the_true_shape_640_squared_two_images():
    """DenseCLIP's own sequence: 40 x 40 patches, T = 1601, Tp = 1608, Tk = 1664 -- 26 key tiles, the last holding one real key."""
    e = _engine(crop=640, depth=2, max_batch=2, seed=23)
    assert (e.n, e.T, e.Tp) == (40, 1601, 1608)
    imgs = W.synth_images(9, 2, 640).cuda()
    traces = [gc.block_trace(0, 3, n=40) + gc.block_trace(36, 9, n=40) + gc.block_trace(17, 36, n=40),
              [dict(x=1.0, y=1.0), dict(x=0.31, y=0.77), dict(x=1.5, y=0.2), dict(x=0.0, y=0.0)]]
    _check_sparse_equals_dense(e, imgs, traces)
    _, sel = e.trace_grids(traces, select_rows=True)
    rows, img_off = _selected_rows(sel, 2)
    t1 = rows[4 * img_off[1]:] % e.Tp
    assert 1600 in t1 and 1 in t1                          # the last patch (row 1600, the last real key) and the first
    e.close()


def test_a_vit_b32_shaped_tower():
    e = _engine(crop=224, patch=32, depth=2, max_batch=2, seed=29)
    assert (e.n, e.T, e.Tp) == (7, 50, 56)
    imgs = W.synth_images(10, 2, 224).cuda()
    _check_sparse_equals_dense(e, imgs, [gc.block_trace(0, 1, n=7, side=2) + gc.block_trace(5, 4, n=7, side=2), [dict(x=0.99, y=0.99)]])
    e.close()


def test_same_images_in_a_16_and_inside_a_48_image_launch_give_identical_embeddings():
    rng = np.random.RandomState(11)
    traces = [gc.block_trace(int(rng.randint(0, 11)), int(rng.randint(0, 11)), n=14) for _ in range(48)]
    imgs = W.synth_images(8, 48, 224).cuda()
    big, small = _engine(max_batch=48), _engine(max_batch=16)
    g_b, sel_b = big.trace_grids(traces, select_rows=True)
    comp_b, map_b = big.vit_forward_rows(imgs, sel_b)
    emb_b = big.region_reduce_rows(comp_b, map_b, g_b.view(48, -1), 1.0 / big.n2)
    dense_b, _ = big.vit_forward(imgs, want_qkv=False)
    assert torch.equal(emb_b, big.region_reduce(dense_b, g_b.view(48, -1), None, 1.0 / big.n2))
    for s in (0, 16, 32):                                  # the middle 16 sit INSIDE the 48-image launch
        g_s, sel_s = small.trace_grids(traces[s:s + 16], select_rows=True)
        comp_s, map_s = small.vit_forward_rows(imgs[s:s + 16], sel_s)
        emb_s = small.region_reduce_rows(comp_s, map_s, g_s.view(16, -1), 1.0 / small.n2)
        assert torch.equal(emb_s, emb_b[s:s + 16]), s
        assert torch.equal(big.region_reduce_rows(comp_b, map_b[s:s + 16], g_b[s:s + 16].view(16, -1), 1.0 / big.n2), emb_b[s:s + 16])
    comp_b2, _ = big.vit_forward_rows(imgs, big.trace_grids(traces, select_rows=True)[1])     # and the same bits again
    assert torch.equal(comp_b, comp_b2)
    big.close(); small.close()


def test_a_trace_over_more_than_the_cut_over_share_takes_the_dense_path():
    e = _engine(max_batch=2)
    wide = [dict(x=(i + 0.5) / 14, y=(j + 0.5) / 14) for j in range(14) for i in range(0, 14, 2)]    # every second column: every quad
    grids, sel = e.trace_grids([wide, wide], select_rows=True)
    assert sel is None and (grids != 0).sum().item() == 2 * 98
    # the library refuses such a list as well (its workspace is sized by the same share)
    quads = np.arange(0, 2 * e.Tp, 4, dtype=np.int32)
    img_off = np.array([0, e.Tp // 4, e.Tp // 2], dtype=np.int32)
    tok = torch.empty(2 * e.Tp, e.D, device="cuda")
    rm = torch.empty(2, e.n2, device="cuda", dtype=torch.int32)
    imgs = W.synth_images(3, 2, 224).cuda()
    rc = e.lib.pio_vit_forward_rows(e.h, imgs.data_ptr(), 2, quads.ctypes.data, img_off.ctypes.data, tok.data_ptr(), rm.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
    assert rc < 0 and b"pio_vit_forward" in e.lib.pio_last_error()
    e.close()


def test_towers_without_a_sparse_tail_stay_dense():
    """A self-only last block is row-local and wants another cut; the fp32 mode is the parity mode; and a CLIP tower nobody asked for."""
    tr = [gc.block_trace(1, 1, n=14), gc.block_trace(2, 2, n=14)]
    for kw in (dict(self_only=1), dict(dtype="fp32"), dict(sparse=False)):
        e = _engine(max_batch=2, **kw)
        assert not e.sparse_ok, kw
        grids, sel = e.trace_grids(tr, select_rows=True)
        assert sel is None and (grids != 0).sum().item() == 32
        if "sparse" not in kw:                             # the library refuses them too, before anything is launched
            quads, img_off = np.array([0], dtype=np.int32), np.array([0, 1, 1], dtype=np.int32)
            tok = torch.full((4, e.D), 7.0, device="cuda")
            rm = torch.empty(2, e.n2, device="cuda", dtype=torch.int32)
            imgs = W.synth_images(3, 2, 224).cuda()
            rc = e.lib.pio_vit_forward_rows(e.h, imgs.data_ptr(), 2, quads.ctypes.data, img_off.ctypes.data, tok.data_ptr(), rm.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert rc < 0 and bool((tok == 7.0).all()), kw
        e.close()


def _count(eng, name, calls):
    real = getattr(eng, name)
    setattr(eng, name, lambda *a, **k: calls.append(name) or real(*a, **k))
    return real


def _denseclip(**over):
    from patchioner_amd import Patchioner
    dec, bank = DR.decoder_and_bank()
    cfg = {"decap_weights": dec, "prefix_size": 512, "support_memory_size": DR.CASE["bank_rows"], "dino_model": "INViTE_B16", "normalize": False,
           "resize_dim": 224, "crop_dim": 224, "clip_model_name": "ViT-B/16", "use_talk2dino_project": False, "linear_talk2dino": False,
           "memory_bank": bank, "max_batch": 8, "denseclip_config": DR.config("r224", depth=2),
           "denseclip_checkpoint": W.synth_denseclip_vit(91, 224, 2)}
    cfg.update(over)
    return Patchioner.from_config(cfg, device="cuda")


def test_denseclip_forward_and_pipeline_give_the_same_ids_and_strings_with_the_path_on_and_off():
    from patchioner_amd.pipeline import TraceCaptionPipeline
    m = _denseclip()
    assert m.backbone_type == "DenseClip" and m.sparse_last_block and m.engine.sparse_ok
    rng = np.random.RandomState(4)
    batches = []
    for i in range(2):                                     # 2 batches of 4 images, one decode group, one ViT launch
        traces = [gc.block_trace(int(rng.randint(0, 11)), int(rng.randint(0, 11)), n=14) for _ in range(4)]
        batches.append((W.synth_images(300 + i, 4, 224).cuda(), traces))
    res = {}
    for on in (True, False):
        pipe = TraceCaptionPipeline(m, group_batches=2, vit_batches=2, sparse_last_block=on)
        caps = list(pipe.run(batches))
        res[on] = (caps, pipe.last_ids.clone())
        pipe.close()
        m.sparse_last_block = on
        fw = []
        for imgs, traces in batches:
            out = m(imgs, get_cls_capt=False, traces=traces)
            fw.append((out["trace_capts"], m.last_ids.clone()))
        res[on] += (fw,)
    m.sparse_last_block = True
    assert res[True][0] == res[False][0] and torch.equal(res[True][1], res[False][1])
    for (c1, i1), (c0, i0) in zip(res[True][2], res[False][2]):
        assert c1 == c0 and torch.equal(i1, i0)
    assert res[True][0] == [fw[0] for fw in res[True][2]]  # and the pipeline's captions are the forward's
    # the sparse path really ran: a traces-only forward leaves the dense entry point alone
    calls = []
    real = _count(m.engine, "vit_forward", calls)
    real_rows = _count(m.engine, "vit_forward_rows", calls)
    m(batches[0][0], get_cls_capt=False, traces=batches[0][1])
    assert calls == ["vit_forward_rows"]
    m(batches[0][0], get_cls_capt=True, traces=batches[0][1])       # a CLS caption needs the dense tokens
    assert calls == ["vit_forward_rows", "vit_forward"]
    m.engine.vit_forward, m.engine.vit_forward_rows = real, real_rows
    # asked not to: the engine never offers the path
    off = _denseclip(sparse_last_block=False)
    assert not off.sparse_last_block and not off.engine.sparse_ok
    assert off(batches[0][0], get_cls_capt=False, traces=batches[0][1])["trace_capts"] == res[True][2][0][0]


def test_the_timm_clip_backbone_stays_dense_unless_asked():
    """No existing default moves: the timm OpenAI-CLIP backbone built as before runs the dense forward for traces (counted), and takes the
    sparse tail, with the same ids and strings, only when built with sparse_last_block=True."""
    from patchioner_amd import Patchioner
    name = "vit_base_patch16_clip_224.openai"
    cfg = {"decap_weights": W.synth_decap(33, prefix_size=512), "prefix_size": 512, "support_memory_size": 2048, "dino_model": name,
           "normalize": False, "resize_dim": 224, "crop_dim": 224, "clip_model_name": "ViT-B/16", "use_talk2dino_project": False,
           "dino_weights": W.synth_clip_vit(31, name, depth=2), "memory_bank": W.synth_bank(35, 2048, 512), "max_batch": 4}
    imgs = W.synth_images(300, 2, 224).cuda()
    traces = [gc.block_trace(3, 5, n=14), gc.block_trace(9, 1, n=14)]
    out = {}
    for asked in (None, True):
        m = Patchioner.from_config(dict(cfg, sparse_last_block=asked), device="cuda")
        assert m.engine.sparse_ok == bool(asked)
        calls = []
        _count(m.engine, "vit_forward", calls)
        _count(m.engine, "vit_forward_rows", calls)
        caps = m(imgs, get_cls_capt=False, traces=traces)["trace_capts"]
        assert calls == (["vit_forward_rows"] if asked else ["vit_forward"])
        out[asked] = (caps, m.last_ids.clone())
    assert out[None][0] == out[True][0] and torch.equal(out[None][1], out[True][1])
