"""The projection references and bars of tests/project_ref64.py have teeth.  Emulations of k_project2 + k_project_combine in fp32 numpy, in
the kernel's order of operations (four channel slices summed in turn, tiles of 16 rows, the online rescale, and for the split form the
fp16 hi / lo pairs of bank, query and P with fp32 accumulation), stay inside every bar at the shapes and inputs the GPU file runs
(project_ref64.hook_cases); emulations of WRONG kernels leave a bar by a factor of at least 4 (the factor of tests/test_decoder_ref64_cpu.py).
The structural errors (a row lost, doubled, read with another row's inv_norm, a rescale or a combine weight missing) are caught by the
T = 1 cases, the precision errors (an operand without its low half) by the T = 0.01 and the one-signed ("biased") cases."""
import os
import re

import numpy as np
import pytest

import project_ref64 as P
from conftest import ROOT

FACTOR = 4.0
f32 = np.float32


def emulate(bank, inv, q, T, bounds, split, S, wrong=None, at=(0, 1)):
    """(m, l [parts][N], acc [parts][N][D]) as k_project2 leaves them.  ``wrong``: one of the faults below, in workgroup at[0] (tile at[1])."""
    bank, inv, q = np.asarray(bank, f32), np.asarray(inv, f32), np.asarray(q, f32)
    M, D = bank.shape
    N = q.shape[0]
    T = f32(T)
    sl = [slice(w * D // 4, (w + 1) * D // 4) for w in range(4)]
    if split:
        bh, bl = (x.astype(f32) for x in P.split16(bank * f32(S)))
        qh, ql = (x.astype(f32) for x in P.split16(q * f32(P.P_SCALE)))
        unscale = f32(1.0 / (S * P.P_SCALE))
        bl1 = np.zeros_like(bl) if wrong == "no_lo_bank" else bl          # GEMM1's view of the low plane
        bl2 = np.zeros_like(bl) if wrong == "no_lo_bank_gemm2" else bl    # GEMM2's (the transposing read at + 2 D)
        if wrong == "no_lo_q":
            ql = np.zeros_like(ql)
    if wrong == "neighbour_inv":
        inv = np.roll(inv, -1)
    m_all, l_all, acc_all = np.full((len(bounds), N), -np.inf, f32), np.zeros((len(bounds), N), f32), np.zeros((len(bounds), N, D), f32)
    for p, (r0, r1, tiles) in enumerate(bounds):
        here = p == at[0]
        m, l, acc = np.full(N, -np.inf, f32), np.zeros(N, f32), np.zeros((N, D), f32)
        for t in range(tiles):
            rows = r0 + 16 * t + np.arange(16)
            valid = rows < M
            if wrong == "tail_mask_off":
                valid[:] = True
            if wrong == "drop_last_row" and here:
                valid &= rows != r1 - 1
            idx = np.minimum(rows, M - 1)
            data = np.minimum(idx - 16, M - 1) if (wrong == "tile_twice" and here and t == at[1]) else idx     # the buffer still holds tile t - 1
            if split:
                s = np.zeros((16, N), f32)
                for w in sl:
                    s = s + ((bh[data][:, w] @ qh[:, w].T) + (bh[data][:, w] @ ql[:, w].T + bl1[data][:, w] @ qh[:, w].T))
                z = (s * (inv[idx] * unscale)[:, None]) / T
            else:
                s = np.zeros((16, N), f32)
                for w in sl:
                    s = s + bank[data][:, w] @ q[:, w].T
                z = (s * inv[idx][:, None]) / T
            z[~valid] = -np.inf
            m_new = np.maximum(m, z.max(0))
            with np.errstate(invalid="ignore"):
                alpha = np.where(np.isinf(m_new), f32(1), np.exp(m - m_new)).astype(f32)
                pw = np.where(np.isinf(m_new)[None, :], f32(0), np.exp(z - m_new[None, :])).astype(f32)
            l = l * alpha + pw.sum(0, dtype=f32)
            if not (wrong == "skip_rescale" and here and t == at[1]):
                acc = acc * alpha[:, None]
            if split:
                ph, pl = (x.astype(f32) for x in P.split16(pw * f32(P.P_SCALE)))
                if wrong == "no_lo_p":
                    pl = np.zeros_like(pl)
                acc = acc + ((ph.T @ bh[data] + ph.T @ bl2[data]) + (pl.T @ bh[data] + pl.T @ bl2[data]))
            else:
                acc = acc + pw.T @ bank[data]
            m = m_new
        m_all[p], l_all[p], acc_all[p] = m, l, acc * unscale if split else acc
    return m_all, l_all, acc_all


def combine(m, l, acc, wrong=None):
    """k_project_combine in fp32.  wrong: "no_weights"; "empty_merged": an empty workgroup's partial still holds what the buffer held
    before the pass (the GPU test fills it with ones) and is merged with weight 1."""
    top = m.max(0)
    with np.errstate(invalid="ignore"):
        w = np.where(np.isinf(m), f32(0), np.exp(m - top[None, :])).astype(f32)
    if wrong == "no_weights":
        w = np.where(np.isinf(m), f32(0), f32(1))
    if wrong == "empty_merged":
        empty = np.isinf(m)
        w, l, acc = np.where(empty, f32(1), w), np.where(empty, f32(1), l), np.where(empty[:, :, None], f32(1), acc)
    return ((w[:, :, None] * acc).sum(0, dtype=f32) / (w * l).sum(0, dtype=f32)[:, None]).astype(f32)


def ratios(c, D, groups, split, wrong=None, at=(0, 1), combine_wrong=None, queries=None):
    """Worst observed / bar of (m, l, Acc, out) for the queries of the pass (``queries``: only those of its queries)."""
    bank, inv, q, bounds, S = P.build_case(c, D, groups)
    qs = q[c["q0"]:]
    ref = P.partials64(bank, inv, qs, c["T"], bounds, split, S)
    out, bar = P.merged64(bank, inv, qs, c["T"], bounds, split, S)
    m, l, acc = emulate(bank, inv, qs, c["T"], bounds, split, S, wrong, at)
    got = combine(m, l, acc, combine_wrong)
    k = slice(None) if queries is None else list(queries)
    return (P.worst(m[:, k], ref["m"][:, k], ref["bar_m"][:, k]), P.worst(l[:, k], ref["l"][:, k], ref["bar_l"][:, k]),
            P.worst(acc[:, k], ref["acc"][:, k], ref["bar_acc"][:, k]), P.worst(got[k], out[k], bar[k]))


def case_of(D, groups, family, T):
    return next(c for c in P.hook_cases(D, groups) if c["family"] == family and c["T"] == T and c["M"] == P.families_geometry(groups)[0])


FORMS = [False, True]
IDS = ["exact", "split"]


@pytest.mark.parametrize("split", FORMS, ids=IDS)
@pytest.mark.parametrize("D", P.WIDTHS)
def test_emulations_pass_every_bar_at_the_gpu_cases(D, split):
    worst = [0.0] * 4
    for groups in (1, 2, 3) if D == 768 else (1, 2):
        for c in P.hook_cases(D, groups):
            r = ratios(c, D, groups, split)
            assert max(r) <= 1.0, (c, groups, r)
            worst = [max(a, b) for a, b in zip(worst, r)]
    print("D %4d %s  emulation / bar  m %.3f  l %.3f  Acc %.3f  out %.3f" % ((D, "split" if split else "exact") + tuple(worst)))


@pytest.mark.parametrize("split", FORMS, ids=IDS)
@pytest.mark.parametrize("D,groups", [(384, 1), (768, 2), (768, 3), (1024, 1), (640, 2)])
def test_structural_faults_leave_the_bars_at_T_1(D, groups, split):
    """Every family at T = 1 sees a row dropped, the tail counted, a neighbour's inv_norm, a tile consumed twice, a skipped rescale; the
    combine faults are seen wherever the slabs' maxima differ."""
    for family in ("gauss", "scales", "planted"):
        c = case_of(D, groups, family, 1.0)
        last = len(P.slab_bounds(c["M"], c["parts"], 16 if groups == 1 else 32)) - 1
        for wrong, at in (("drop_last_row", (0, 0)), ("drop_last_row", (last, 0)), ("tail_mask_off", (0, 0)), ("neighbour_inv", (0, 0)),
                          ("tile_twice", (0, 1)), ("tile_twice", (1, 2))):
            r = ratios(c, D, groups, split, wrong, at)
            assert max(r[:3]) >= FACTOR, (family, wrong, at, r)             # a bar of the partials sees every one of them
            if family != "gauss":                                          # ... and the merged result wherever rows differ in size or weight
                assert r[3] >= FACTOR, (family, wrong, at, r)
    # the rescale skipped where ONE query's maximum moved (the ballot family: query q0 + 5 meets its row in the third tile of slab 0)
    c = case_of(D, groups, "ballot", 1.0)
    r = ratios(c, D, groups, split, "skip_rescale", (0, 2))
    assert r[2] >= FACTOR and r[3] >= FACTOR, ("skip_rescale", r)
    assert max(ratios(c, D, groups, split)) <= 1.0
    # the sorted bank: at T = 1 a tile raises the maximum by 1e-3 or so, a skipped rescale is a 1e-3 error of a fraction of Acc and stays
    # near the bar; at T = 0.01 the same step is 0.1 or more and the family guards against it -- in a slab's last tiles: what a rescale
    # skipped earlier leaves wrong is e^-(the rise since) of the final Acc
    c = case_of(D, groups, "rising", 0.01)
    tiles = P.slab_bounds(c["M"], c["parts"], 16 if groups == 1 else 32)[1][2]
    assert ratios(c, D, groups, split, "skip_rescale", (1, tiles - 1))[2] >= FACTOR
    for family in ("planted", "rising", "scales"):
        c = case_of(D, groups, family, 1.0)
        assert ratios(c, D, groups, split, combine_wrong="no_weights")[3] >= FACTOR, (family, "combine without weights")
    # more workgroups than units: the empty ones must not count
    c = dict(family="gauss", M=33, parts=8, nq=16 * groups, q0=3, T=1.0)
    assert max(ratios(c, D, groups, split)) <= 1.0
    assert ratios(c, D, groups, split, combine_wrong="empty_merged")[3] >= FACTOR


@pytest.mark.parametrize("D,groups", [(384, 1), (768, 2), (768, 3), (1024, 2), (512, 1), (640, 1)])
def test_split_form_without_a_low_half_leaves_the_bars(D, groups):
    """Bank and query: the one-signed family at T = 0.01 (every element of the bank, and of the query, loses the same 4.3e-4 with its low
    half, so every logit -- 70 or so -- drops by 0.03: the bar of m sees it; l, Acc and out cannot, the shift is common to all rows).
    P: the family whose weights all sit 0.45 of an fp16 step above a grid point, at T = 1."""
    c = case_of(D, groups, "biased", 0.01)
    assert max(ratios(c, D, groups, True)) <= 1.0
    for wrong in ("no_lo_bank", "no_lo_q"):
        r = ratios(c, D, groups, True, wrong)
        print("D %d groups %d %s: m %.1f l %.1f Acc %.1f out %.1f" % ((D, groups, wrong) + r))
        assert r[0] >= FACTOR, (wrong, r)
    # the low plane missing from GEMM2 alone: every element of Acc loses 4.3e-4 of itself, whatever the weights -- seen where the weight
    # bar is narrow: one-hot queries at T = 1 (under the positive queries of "biased" the weight bar alone is 1e-4 and the factor is 3 .. 7)
    c = case_of(D, groups, "biased_onehot", 1.0)
    assert max(ratios(c, D, groups, True)) <= 1.0
    r = ratios(c, D, groups, True, "no_lo_bank_gemm2")
    print("D %d groups %d no_lo_bank_gemm2: m %.1f l %.1f Acc %.1f out %.1f" % ((D, groups) + r))
    assert r[2] >= FACTOR and r[3] >= FACTOR, r
    c = case_of(D, groups, "biased_p", 1.0)
    assert max(ratios(c, D, groups, True)) <= 1.0
    r = ratios(c, D, groups, True, "no_lo_p")
    print("D %d groups %d no_lo_p: m %.1f l %.1f Acc %.1f out %.1f" % ((D, groups) + r))
    assert r[2] >= FACTOR, r                                         # Acc's bar; the merged bar (|b| + |out| for |b - out|) is twice as wide


@pytest.mark.parametrize("split", FORMS, ids=IDS)
def test_T_001_hides_a_row_only_where_its_weight_is_below_the_bar(split):
    """What T = 0.01 can and cannot see, on the file's own cases (D = 768, one group, M = 300 in slabs of 80 rows).
    The planted case: query j of the pass equals row planted[(j + 3) % 5], whose logit is 100 against |z| < 15 for every other row.  Row
    79, the last of slab 0, is no planted row: dropped, it stays INSIDE the merged bar of every query, and inside the m, l and Acc bars of
    the queries whose own row (40) lies in slab 0 -- a structural fault the T = 0.01 cases do not see.  The same fault on a row that
    carries the weight (159, the last of slab 1) leaves the bars, and so does row 79 at T = 1.
    The Gaussian case has no dominant row: among 16 queries and 80 rows some row of the slab weighs enough, and the dropped row IS seen at
    T = 0.01 too.  A wrong inv_norm is a 2.5 % error of a cosine, 2.5 in the logit: seen at any temperature."""
    D, groups = 768, 1
    c = case_of(D, groups, "planted", 0.01)
    assert P.planted_rows(c["M"], c["parts"], groups) == (80, 159, 240, 299, 40)
    own = [j for j in range(c["nq"]) if (j + c["q0"]) % 5 == 4]                  # the queries equal to row 40
    assert own == [1, 6, 11]
    r = ratios(c, D, groups, split, "drop_last_row", (0, 0))
    assert r[3] <= 1.0, r
    assert max(ratios(c, D, groups, split, "drop_last_row", (0, 0), queries=own)) <= 1.0
    assert min(ratios(c, D, groups, split, "drop_last_row", (1, 0))) >= FACTOR    # row 159: the whole weight of three queries
    assert max(ratios(case_of(D, groups, "planted", 1.0), D, groups, split, "drop_last_row", (0, 0))) >= FACTOR
    assert max(ratios(case_of(D, groups, "gauss", 0.01), D, groups, split, "drop_last_row", (1, 0))) >= FACTOR
    assert max(ratios(case_of(D, groups, "gauss", 1.0), D, groups, split, "drop_last_row", (1, 0))) >= FACTOR
    assert max(ratios(case_of(D, groups, "gauss", 0.01), D, groups, split, "neighbour_inv")) >= FACTOR


def test_split_bank_bits_and_slab_bounds():
    x = np.array([[1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, -1.0 - 2.0 ** -12, 65504.0 / 2]], f32)
    img = P.split_bank64(np.tile(x, (1, 48)), 1.0).reshape(2, -1)[:, :8]
    hi, lo = img[0].view(np.float16).astype(f32), img[1].view(np.float16).astype(f32)
    assert hi.tolist() == [1.0, 1.0, 1.0 + 2.0 ** -9, 2.0 ** -14, 2.0 ** -24, 0.0, -1.0, 32752.0]       # ties to even, subnormals kept
    assert lo.tolist() == [0.0, 2.0 ** -11, -(2.0 ** -11), 0.0, 0.0, 0.0, -(2.0 ** -12), 0.0]            # 2^-25 is below half a subnormal step
    assert P.slab_bounds(33, 8, 16) == [(0, 16, 1), (16, 32, 1), (32, 33, 1)] + [(48, 48, 0)] * 5
    assert P.slab_bounds(33, 2, 32) == [(0, 32, 2), (32, 33, 2)]               # the second unit's second tile lies wholly past M
    assert P.slab_bounds(300, 4, 16) == [(0, 80, 5), (80, 160, 5), (160, 240, 5), (240, 300, 4)]
    assert P.abs_max_bits(np.array([0.5, -3.0, -0.0], f32)) == 0x40400000 and P.bank_scale(np.array([3.9], f32)) == 2.0 ** 13


def test_topk_rule_rejects_ties_highest_index_first():
    rng = np.random.default_rng(5)
    bank = rng.standard_normal((70, 384)).astype(f32)
    bank[40], bank[55], bank[9] = bank[12], bank[12], bank[12]
    q = np.stack([bank[12], rng.standard_normal(384).astype(f32)])
    c, bar = P.sims64(bank, q)
    vals, rows = P.topk64(c, 5)
    assert rows[0, :4].tolist() == [9, 12, 40, 55]
    assert P.topk_violations(c, bar, bank, vals, rows, 5) == []
    swapped = rows.copy()
    swapped[0, :4] = [55, 40, 12, 9]
    assert any("ascending" in v for v in P.topk_violations(c, bar, bank, vals, swapped, 5))
    other = rows.copy()
    other[1, 0], other[1, 4] = rows[1, 4], rows[1, 0]                                       # the fifth best and the best change places: a gap far outside the bar
    assert any("float64 gap" in v for v in P.topk_violations(c, bar, bank, np.take_along_axis(c, other, 1), other, 5))
    off = vals.copy()
    off[1, 2] += 4 * bar[1, rows[1, 2]]
    assert any("similarity" in v for v in P.topk_violations(c, bar, bank, off, rows, 5))


def test_k_project2_is_launched_from_one_place():
    """The hook tests the pass the projection runs: launch_mem_project's loop and pio_test_project_pass both call launch_project_pass,
    and k_project2 is launched nowhere else."""
    csrc = os.path.join(ROOT, "patchioner_amd", "csrc")
    launches = {f: len(re.findall(r"hipLaunchKernelGGL\(\(?k_project2\b", open(os.path.join(csrc, f)).read())) for f in os.listdir(csrc)}
    assert {f: n for f, n in launches.items() if n} == {"project.hip": 1}
    src = open(os.path.join(csrc, "project.hip")).read()
    loop = src[src.index("hipError_t launch_mem_project("):src.index("hipError_t launch_mem_topk(")]
    assert "launch_project_pass(a, groups, q0," in loop and "k_project_combine" not in loop and "project_pass_d<" not in loop
    hook = open(os.path.join(csrc, "test_hooks.cpp")).read()
    assert "launch_project_pass(a, groups, q0, parts" in hook[hook.index("int pio_test_project_pass("):]
