"""The sparse last ViT block (pio_vit_forward_rows): for trace regions the last block's query rows, attention output, proj, LayerNorm 2,
fc1, fc2 and the final LayerNorm run only on the rows whose patches a trace touches.  The invariant is SAME BITS: every selected token
is the dense forward's, so region embeddings, prefixes, ids and captions are too.  All comparisons here are torch.equal."""
import numpy as np
import pytest
import torch

import golden_cases as gc
from patchioner_amd import weights as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _engine(dino="dinov2_vitb14_reg", depth=2, crop=224, max_batch=4, dtype="fp16", seed=17):
    from patchioner_amd.engine import Engine
    dims = {"dinov2_vits14_reg": (384, 6), "dinov2_vitb14_reg": (768, 12), "dinov2_vitl14_reg": (1024, 16)}[dino]
    e = Engine(embed_dim=dims[0], depth=depth, num_heads=dims[1], num_registers=4, crop_dim=crop, max_batch=max_batch, vit_dtype=dtype,
               readout_heads=6 if dims[0] == 384 else 16)
    e.load_state_dict(W.synth_dinov2(seed, dino, depth=depth))
    e.finalize()
    return e


def _selected_rows(sel, B):
    """the padded-matrix rows (b * Tp + t) of the compact rows, from the staged host list"""
    import ctypes
    nq = sel["nq"]
    quads = np.ctypeslib.as_array(ctypes.cast(sel["quads"], ctypes.POINTER(ctypes.c_int32)), shape=(nq,)).copy()
    img_off = np.ctypeslib.as_array(ctypes.cast(sel["img_off"], ctypes.POINTER(ctypes.c_int32)), shape=(B + 1,)).copy()
    return (quads[:, None] + np.arange(4)[None, :]).reshape(-1), img_off


def _check_sparse_equals_dense(e, imgs, traces):
    """compact tokens == dense tokens at the selected rows, row map consistent, region embeddings equal; returns the embeddings"""
    B = imgs.shape[0]
    dense, _ = e.vit_forward(imgs, want_qkv=False)
    grids, sel = e.trace_grids(traces, select_rows=True)
    assert sel is not None
    rows, img_off = _selected_rows(sel, B)
    comp, row_map = e.vit_forward_rows(imgs, sel)
    torch.cuda.synchronize()
    assert comp.shape == (4 * sel["nq"], e.D) and torch.isfinite(comp).all()
    b, t = rows // e.Tp, rows % e.Tp
    valid = t < e.T                                        # pad rows of a quad are computed too and mean nothing
    idx = torch.from_numpy(np.nonzero(valid)[0]).cuda()
    want = dense[torch.from_numpy(b[valid]).cuda(), torch.from_numpy(t[valid]).cuda()]
    assert torch.equal(comp[idx], want)
    # every patch with a non-zero count has a row, and that row is its token
    g = grids.view(B, -1)
    rm = row_map.cpu().numpy()
    nz = (g != 0).cpu().numpy()
    assert (rm[nz] >= 0).all()
    for bi, p in zip(*np.nonzero(nz)):
        assert rows[rm[bi, p]] == bi * e.Tp + e.G + p
    for bi in range(B):                                    # an image without points selects nothing
        if not nz[bi].any():
            assert img_off[bi + 1] == img_off[bi] and (rm[bi] == -1).all()
    emb_d = e.region_reduce(dense, g, None, 1.0 / e.n2)
    emb_s = e.region_reduce_rows(comp, row_map, g, 1.0 / e.n2)
    assert torch.equal(emb_d, emb_s)
    return emb_s, g


def _edge_traces():
    """two launches of three images: blocks at patch column 0 and ending at column 15, a block whose runs straddle quad boundaries
    ((5 + gx) % 4 != 0), a single point; points outside [0, 1] (and on its closed ends), an image without points, an inner block"""
    a = [gc.block_trace(0, 3) + gc.block_trace(12, 9), gc.block_trace(5, 6), [dict(x=0.53, y=0.41)]]
    b = [gc.trace_cases()[0][1], [], gc.block_trace(7, 7)]
    return a, b


@pytest.fixture(scope="module", params=["fp16", "bf16"])
def vitb12(request):
    e = _engine(depth=12, max_batch=3, dtype=request.param, seed=91)
    yield e
    e.close()


def test_compact_tokens_are_the_dense_tokens_bit_for_bit_depth12(vitb12):
    e = vitb12
    imgs = W.synth_images(5, 3, 224).cuda()
    for traces in _edge_traces():
        emb, g = _check_sparse_equals_dense(e, imgs, traces)
        for bi in range(3):
            if not (g[bi] != 0).any():
                assert (emb[bi] == 0).all()                # an empty trace: a zero embedding, as today
    # the straddling block really straddles, and the edge blocks reach both edges
    _, sel = e.trace_grids(_edge_traces()[0], select_rows=True)
    rows, img_off = _selected_rows(sel, 3)
    t1 = rows[4 * img_off[1]:4 * img_off[2]] % e.Tp
    assert len(t1) == 32                                   # 4 runs of 4 patches, each over two quads
    t0 = rows[4 * img_off[0]:4 * img_off[1]] % e.Tp
    assert e.G + 3 * 16 + 0 in t0 and e.G + 9 * 16 + 15 in t0


def test_same_images_in_a_16_and_inside_a_48_image_launch_give_identical_embeddings():
    rng = np.random.RandomState(11)
    traces = [gc.block_trace(int(rng.randint(0, 13)), int(rng.randint(0, 13))) for _ in range(48)]
    imgs = W.synth_images(8, 48, 224).cuda()
    big, small = _engine(depth=3, max_batch=48), _engine(depth=3, max_batch=16)
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
        # the per-batch reduction over a slice of the launch's map (what the pipeline does)
        assert torch.equal(big.region_reduce_rows(comp_b, map_b[s:s + 16], g_b[s:s + 16].view(16, -1), 1.0 / big.n2), emb_b[s:s + 16])
    comp_b2, _ = big.vit_forward_rows(imgs, big.trace_grids(traces, select_rows=True)[1])     # and the same bits again
    assert torch.equal(comp_b, comp_b2)
    big.close(); small.close()


def test_a_trace_over_more_than_the_cut_over_share_takes_the_dense_path():
    e = _engine(depth=2, max_batch=2)
    wide = [dict(x=(i + 0.5) / 16, y=(j + 0.5) / 16) for j in range(16) for i in range(0, 16, 2)]    # every second column: all 64 patch quads
    grids, sel = e.trace_grids([wide, wide], select_rows=True)
    assert sel is None                                     # 2 x 65 quads of 2 x 66: above one half
    assert (grids != 0).sum().item() == 2 * 128
    # the library refuses such a list as well (its workspace is sized by the same share)
    quads = np.arange(0, 2 * e.Tp, 4, dtype=np.int32)
    img_off = np.array([0, e.Tp // 4, e.Tp // 2], dtype=np.int32)
    tok = torch.empty(2 * e.Tp, e.D, device="cuda")
    rm = torch.empty(2, e.n2, device="cuda", dtype=torch.int32)
    imgs = W.synth_images(3, 2, 224).cuda()
    rc = e.lib.pio_vit_forward_rows(e.h, imgs.data_ptr(), 2, quads.ctypes.data, img_off.ctypes.data, tok.data_ptr(), rm.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
    assert rc < 0 and b"pio_vit_forward" in e.lib.pio_last_error()
    # a list that is not ascending multiples of 4 inside its image is refused before anything is launched
    bad = np.array([8, 6], dtype=np.int32)
    rc = e.lib.pio_vit_forward_rows(e.h, imgs.data_ptr(), 2, bad.ctypes.data, np.array([0, 2, 2], dtype=np.int32).ctypes.data,
                                    tok.data_ptr(), rm.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc < 0
    e.close()


def test_host_selection_matches_the_device_grids_on_the_golden_trace_cases():
    cases = gc.trace_cases()
    for n, crop in ((16, 224), (37, 518), (10, 140)):
        traces = [tr for nn, tr in cases if nn == n]
        e = _engine(depth=1, crop=crop, max_batch=len(traces))
        assert e.n == n
        grids, sel = e.trace_grids(traces, select_rows=True)
        nz = (grids.view(len(traces), -1) != 0).cpu().numpy()
        want = sorted({b * e.Tp + 4 * ((e.G + p) // 4) for b, p in zip(*np.nonzero(nz))})
        if sel is None:                                    # nothing selected, or above the cut-over: only possible when that is so
            assert not want or 4 * len(want) * e.SPARSE_SHARE_DEN >= len(traces) * e.Tp
        else:
            rows, _ = _selected_rows(sel, len(traces))
            assert rows[::4].tolist() == want
        e.close()


def _model(**over):
    from patchioner_amd import Patchioner
    cfg = {"decap_weights": W.synth_decap(3), "prefix_size": 768, "linear_talk2dino": False, "support_memory_size": 2048,
           "dino_model": "dinov2_vitb14_reg", "normalize": True, "resize_dim": 224, "crop_dim": 224,
           "dino_weights": W.synth_dinov2(91, "dinov2_vitb14_reg", depth=2), "memory_bank": W.synth_bank(61, 2048), "max_batch": 8}
    cfg.update(over)
    return Patchioner.from_config(cfg, device="cuda")


def test_pipeline_and_forward_give_the_same_ids_and_strings_with_the_sparse_path_on_and_off():
    from patchioner_amd.pipeline import TraceCaptionPipeline
    m = _model()
    rng = np.random.RandomState(4)
    batches = []
    for i in range(2):                                     # 2 batches of 4 images, one decode group, one ViT launch
        traces = [gc.block_trace(int(rng.randint(0, 13)), int(rng.randint(0, 13))) for _ in range(4)]
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
    # a trace over more than the cut-over share of the grid: dense either way, identical outputs
    wide = [dict(x=(i + 0.5) / 16, y=(j + 0.5) / 16) for j in range(16) for i in range(0, 16, 2)]
    wide_out = {}
    for on in (True, False):
        m.sparse_last_block = on
        wide_out[on] = (m(batches[0][0], get_cls_capt=False, traces=[wide] * 4)["trace_capts"], m.last_ids.clone())
    assert wide_out[True][0] == wide_out[False][0] and torch.equal(wide_out[True][1], wide_out[False][1])
    m.sparse_last_block = True
    assert res[True][0] == res[False][0] and torch.equal(res[True][1], res[False][1])
    for (c1, i1), (c0, i0) in zip(res[True][2], res[False][2]):
        assert c1 == c0 and torch.equal(i1, i0)
    assert res[True][0] == [fw[0] for fw in res[True][2]]  # and the pipeline's captions are the forward's
    # the sparse path really ran: a traces-only forward leaves the dense entry point alone
    calls = []
    real = m.engine.vit_forward
    m.engine.vit_forward = lambda *a, **k: calls.append(1) or real(*a, **k)
    m(batches[0][0], get_cls_capt=False, traces=batches[0][1])
    assert not calls
    m(batches[0][0], get_cls_capt=True, traces=batches[0][1])       # a CLS caption needs the dense tokens
    assert calls
    m.engine.vit_forward = real


@pytest.mark.parametrize("dino,crop", [("dinov2_vits14_reg", 224), ("dinov2_vitl14_reg", 224), ("dinov2_vitb14_reg", 518)])
def test_other_widths_and_resolutions_are_bit_identical_too(dino, crop):
    e = _engine(dino=dino, depth=2, crop=crop, max_batch=2, seed=23)
    n = e.n
    imgs = W.synth_images(9, 2, crop).cuda()
    traces = [gc.block_trace(0, 1, n=n) + gc.block_trace(n - 4, n - 5, n=n), [dict(x=1.0, y=1.0), dict(x=0.31, y=0.77), dict(x=1.5, y=0.2)]]
    _check_sparse_equals_dense(e, imgs, traces)
    e.close()


def test_towers_without_a_sparse_path_stay_dense():
    from patchioner_amd.engine import Engine
    e = Engine(embed_dim=768, depth=1, num_heads=12, num_registers=4, crop_dim=224, max_batch=2, vit_dtype="fp32")
    assert not e.sparse_ok
    e.load_state_dict(W.synth_dinov2(17, depth=1))
    e.finalize()
    grids, sel = e.trace_grids([gc.block_trace(1, 1), gc.block_trace(2, 2)], select_rows=True)
    assert sel is None and (grids != 0).sum().item() == 32
    e.close()
