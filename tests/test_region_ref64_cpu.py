"""The float64 statements of tests/region_ref64.py against the REFERENCE's own fp32 outputs (tests/golden/attn_readout*.npz,
bbox_feats.npz, region_means.npz, ctx_cleaner.npz, pinv.npz) and against this repository's oracle on the edge-case boxes of
tests/test_gpu_region_kernels.py, so that the GPU tests that hold the kernels to them hold the kernels to the right function -- and
a wrong edge expectation (clamping, negative wrap, the NaN row, the in-place renormalisation) shows here, without a GPU.  The bars
are the ones tests/test_gpu_parity.py and tests/test_gpu_configs.py use for the same vectors (fp32 reference against an exact
evaluation)."""
import numpy as np
import pytest
import torch

import golden_cases as gc
import region_ref64 as R
from oracle import patchioner_oracle as O

torch.set_grad_enabled(False)


def close(a, b, rtol, atol):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)), "NaN positions differ"
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, equal_nan=True)


@pytest.mark.parametrize("name,case,inputs,maps_atol", [("attn_readout", gc.ATTN, gc.attn_inputs, 2e-5),
                                                        ("attn_readout_vits", gc.ATTN_VITS, gc.attn_vits_inputs, 1e-4)])
def test_readout_reproduces_the_reference_fixture(golden, name, case, inputs, maps_atol):
    g = golden(name)
    c = case
    qkv, patches = inputs()
    T = c["G"] + c["n"] ** 2
    tokens = torch.cat([torch.zeros(c["B"], c["G"], c["D"]), patches], dim=1)
    sa, maps, avg, dis = R.cls_readout64(qkv, T, c["G"], c["D"], c["heads"], c["scale"], tokens)
    close(sa, g["self_attn"], rtol=2e-5 if name == "attn_readout" else 1e-4, atol=1e-7)
    close(maps, g["maps"], rtol=1e-4, atol=maps_atol)
    close(avg, g["avg_self_attn_token"], rtol=1e-4, atol=1e-6)
    close(dis, g["disentangled"], rtol=1e-4, atol=1e-6)
    assert float(R.softmax_rel64(maps, torch.zeros_like(maps[..., :1])).min()) >= R.E_EXP + R.SUM_DEPTH + 2


BOX_RUNS = [
    ("uniform", gc.boxes_regular, dict(mode=0)),
    ("gauss05", gc.boxes_regular, dict(mode=1, variance=0.5)),
    ("gauss10", gc.boxes_regular, dict(mode=1, variance=1.0)),
    ("attnmap", gc.boxes_regular, dict(mode=3)),
    ("dummy_nan", gc.boxes_with_dummies, dict(mode=1, variance=0.5)),
    ("single_uniform", gc.boxes_with_dummies, dict(mode=0, single=True)),
    ("single_gauss", gc.boxes_with_dummies, dict(mode=1, variance=0.5, single=True)),
    ("single_attn", gc.boxes_with_dummies, dict(mode=3, single=True)),
]


def _feats(patches, res, single):
    """The features the weights give: per box, or of the single map."""
    N = patches.shape[0]
    if single:
        return R.region_reduce64(patches, res.single.float(), None, 1.0)[0]
    NB = res.weights.shape[1]
    idx = torch.arange(N).repeat_interleave(NB)
    w = res.weights.reshape(N * NB, -1)
    return R.region_reduce64(patches, w, idx, 1.0)[0].view(N, NB, -1)


@pytest.mark.parametrize("tag,mk,kw", BOX_RUNS, ids=[r[0] for r in BOX_RUNS])
def test_bbox_weights_reproduce_the_reference_fixture(golden, tag, mk, kw):
    g = golden("bbox_feats")
    boxes = mk()
    boxes //= gc.BOX["patch_size"]
    assert np.array_equal(boxes.numpy(), g[tag + "__boxes_after"])
    attn = gc.box_attn() if kw["mode"] == 3 else None
    single = kw.get("single", False)
    res = R.bbox_weights64(boxes.long(), gc.BOX["n"], kw["mode"], kw.get("variance", 0.5), None, attn, single)
    close(_feats(gc.box_patches(), res, single), g[tag], rtol=2e-5, atol=2e-6)
    if attn is not None:
        close(res.attn_after, g[tag + "__attn_after"], rtol=2e-6, atol=1e-9)


def test_center_pick_reproduces_the_reference_fixture(golden):
    """variance == 0 on boxes with odd spans: the one-hot sits on the middle cell."""
    g = golden("bbox_feats")
    boxes = gc.boxes_odd_spans()
    boxes //= gc.BOX["patch_size"]
    sp = R.box_spans(boxes.long(), gc.BOX["n"])
    centre = torch.stack([(sp[..., 1] - sp[..., 0]) // 2, (sp[..., 3] - sp[..., 2]) // 2], dim=-1)
    res = R.bbox_weights64(boxes.long(), gc.BOX["n"], 2, center=centre)
    close(_feats(gc.box_patches(), res, False), g["center_odd"], rtol=1e-6, atol=1e-7)


def test_gaussian_map_ctx_cleaner_and_revert_reproduce_the_reference_fixtures(golden):
    g = golden("region_means")
    patches = gc.box_patches()
    for v in gc.REGION_VARIANCES:
        wmap = R.gaussian_map64(gc.BOX["n"], v)[0].reshape(1, -1).expand(patches.shape[0], -1)
        close(R.region_reduce64(patches, wmap, None, 1.0)[0], g["var_%s" % v], rtol=2e-5, atol=2e-6)
    g = golden("ctx_cleaner")
    dirty, ctx = gc.ctx_inputs()
    for mode, ct in enumerate(("orthogonal_projection", "contrastive_mask")):
        for alpha in (1.0, 0.35):
            close(R.ctx_clean64(dirty, ctx, mode, alpha), g["%s_%g" % (ct, alpha)], rtol=1e-5, atol=1e-6)
        dn, cn = dirty / dirty.norm(dim=-1, keepdim=True), ctx / ctx.norm(dim=-1, keepdim=True)
        close(R.ctx_clean64(dirty, ctx, mode, 0.7, normalize_inputs=True), O.ctx_cleaner(dn, cn, cleaning_type=ct, alpha=0.7),
              rtol=1e-5, atol=1e-6)
    g = golden("pinv")
    A, b, x = gc.randn(71, 768, 512) * 0.05, gc.randn(72, 768) * 0.02, gc.randn(73, 6, 768)
    close(R.revert64(x, O.get_pseudo_inverse(A), b)[0], g["y"], rtol=1e-4, atol=1e-4)


EDGE_RUNS = [(0, 0.5, False), (1, 0.05, False), (1, 0.5, False), (1, 1.0, False), (1, 10.0, False), (3, 0.5, False),
             (0, 0.5, True), (1, 0.05, True), (1, 0.5, True), (3, 0.5, True)]


@pytest.mark.parametrize("n", [7, 9, 16, 37])
def test_edge_case_boxes_against_the_oracle(n):
    """The edge-case boxes of the GPU test through oracle.extract_bboxes_feats (fp32, python slices on the real grid) and through
    bbox_weights64: same features, NaN rows in the same places -- exactly the uniform-mode rows of the empty slices and of the dummy --
    and the same attention map after the in-place renormalisation; cells no box covers keep their bits."""
    boxes = R.edge_boxes(n)
    sp = R.box_spans(boxes, n)
    empty = ((sp[..., 1] - sp[..., 0]) * (sp[..., 3] - sp[..., 2])) == 0
    assert int(empty.sum()) == 5                                   # start beyond, end at 0, below -n, the dummy, start at n
    assert (sp[1, 4].tolist(), sp[2, 0].tolist(), sp[2, 5].tolist()) == ([1, 4, n - 3, n - 1], [1, 4, n - 5, n - 3], [n - 4, n - 2, 1, 4])
    assert sp[1, 2].tolist() == [n - 2, n, n - 3, n]               # the end clamps
    patches = gc.randn(100 + n, 3, n * n, 24)
    for mode, var, single in EDGE_RUNS:
        attn0 = torch.softmax(gc.randn(200 + n, 3, n * n) * 2.0, dim=-1) if mode == 3 else None
        attn_o = attn0.clone() if mode == 3 else None
        want = O.extract_bboxes_feats(patches.clone(), boxes.float(), gaussian_avg=(mode == 1), gaussian_bbox_variance=var,
                                      get_single_embedding_per_image=single, patch_size=1, attention_map=attn_o)
        res = R.bbox_weights64(boxes, n, mode, var, None, attn0, single)
        got = _feats(patches, res, single)
        close(got, want, rtol=2e-5, atol=2e-6)
        nan_rows = torch.isnan(got).any(dim=-1)
        if single:
            assert not bool(nan_rows.any())
        else:
            assert torch.equal(nan_rows, empty if mode == 0 else torch.zeros_like(empty)), (mode, var)
        if mode == 3:
            close(res.attn_after, attn_o, rtol=2e-6, atol=1e-9)
            covered = torch.zeros(3, n, n, dtype=torch.bool)
            for i in range(3):
                for j in range(boxes.shape[1]):
                    if single and int(boxes[i, j].sum()) < 0:
                        continue
                    ys, ye, xs, xe = sp[i, j].tolist()
                    covered[i, ys:ye, xs:xe] = True
            assert torch.equal(res.attn_after.view(3, n, n)[~covered], attn0.double().view(3, n, n)[~covered])
            assert bool(covered.view(3, -1).any(dim=1).all()) and not bool(covered[1].all())
        assert bool((res.rel >= 0).all()) and bool(torch.isfinite(res.rel).all())


@pytest.mark.parametrize("n", [7, 9, 16, 37])
def test_gaussian_map_against_the_oracle(n):
    patches = gc.randn(300 + n, 2, n * n, 24)
    for v in (0.05, 0.5, 2.5, 99.9, 100, 1000):
        m, rel = R.gaussian_map64(n, v)
        assert abs(float(m.sum()) - 1.0) < 1e-12 and torch.equal(m, m.flip(0)) and torch.equal(m, m.flip(1))
        wmap = m.reshape(1, -1).expand(2, -1)
        close(R.region_reduce64(patches, wmap, None, 1.0)[0], O.compute_region_means(patches, v), rtol=2e-5, atol=2e-6)
        assert bool(torch.isfinite(rel).all())


def test_box_sequences_follow_the_oracle_slices():
    """box_sequences64 / box_seq_reduce64 on an identity 'block': the rows the oracle's double-DINO path would feed its block, and
    its two read-outs of them (row 0; the mean of the region rows, NaN for an empty region)."""
    n, G, D = 7, 5, 8
    tokens = gc.randn(9, 2, G + n * n, D)
    sl = torch.tensor([[[1, 4, 2, 5], [0, 7, 0, 7]], [[3, 4, 3, 4], [2, 2, 1, 3]]])
    for use_cls in (True, False):
        seqs = R.box_sequences64(tokens, sl, G, n, use_cls)
        Gs = G if use_cls else 0
        assert [s.shape[0] for s in seqs] == [Gs + 9, Gs + 49, Gs + 1, Gs]
        pe = tokens[:, G:].view(2, n, n, D)
        assert torch.equal(seqs[0][Gs:], pe[0, 1:4, 2:5].reshape(-1, D)) and torch.equal(seqs[2][Gs:], pe[1, 3:4, 3:4].reshape(-1, D))
        if use_cls:
            assert torch.equal(seqs[3], tokens[1, :G]) and torch.equal(R.box_seq_reduce64(seqs[3], Gs, "cls"), tokens[1, 0].double())
        assert bool(torch.isnan(R.box_seq_reduce64(seqs[3], Gs, "avg")).all())
        assert torch.allclose(R.box_seq_reduce64(seqs[1], Gs, "avg"), pe[0].double().mean(dim=(0, 1)))
