"""The memory-bank projection's kernels (csrc/project.hip) against the float64 statements and derived bars of tests/project_ref64.py (the
derivation is in that module's docstring; tests/test_project_ref64_cpu.py shows that the bars reject wrong kernels, on these very cases).

  k_project2 + k_project_combine   one bank pass through pio_test_project_pass -- the function launch_mem_project's loop calls -- in both
                forms (exact fp32, split fp16), at every bank width, with one and two query groups (three at D = 768), on slab geometries
                chosen through `parts` (project_ref64.GEOMETRY: slabs of 1, 2, 3 and 5 tiles, partial and empty slabs, M = 1 .. 33, the 32-row
                unit whose second tile lies past M, parts = 1 and 1024), N - q0 = 1 .. 48 with q0 = 3, T = 1, 0.01 and 1e-3, and the input
                families of project_ref64.make_case.  EVERY workgroup's (m, l, Acc) is held to partials64, the merged rows to merged64; the
                rows of `out` outside the pass and the guard rows of every buffer keep their sentinel; two calls give the same bits
  the split form's range   rows whose largest element is 2^-k of max|bank|, k = 0 .. 30: held to the bar with its magnitude term; the first k
                that leaves the bar of k = 0 is reported
  k_row_inv_norm, k_abs_max, k_split_bank   through pio_test_bank_prep: float64, exact bits, exact bits
  k_project_sims + k_topk_desc    through Engine.topk_rows and Engine.project(n_best = k)
  the whole call   Engine.project at M = 2049, D = 768 for N = 1 .. 128 in both forms against project64: the decomposition into passes of 48,
                32 and 16 queries, the in-place normalisation of q, the loader's inv_norm and the final normalisation

Each test prints observed / bar of its worst element."""
import os
import re

import numpy as np
import pytest
import torch

import project_ref64 as P
from patchioner_amd import _lib
from conftest import ROOT
from patchioner_amd._lib import check, ptr

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
SENT = 12345.678
FORMS = [False, True]
IDS = ["exact", "split"]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _prep(bank_d, S=None, want_inv=False, want_max=False):
    """pio_test_bank_prep on a device bank -> (inv_norm or None, abs-max bits or None, split image [M][2][D] int16 or None)."""
    lib = _lib.load()
    M, D = bank_d.shape
    inv = torch.full((M + 2,), SENT, device="cuda") if want_inv else None
    mx = torch.full((3,), -1, dtype=torch.int32, device="cuda") if want_max else None
    img = torch.full((M + 2, 2, D), 0x5555, dtype=torch.int16, device="cuda") if S else None
    check(lib.pio_test_bank_prep(ptr(bank_d), M, D, float(S or 0.0), inv[1:].data_ptr() if want_inv else None,
                                 mx[1:].data_ptr() if want_max else None, img[1:].data_ptr() if S else None, _stream()))
    if want_inv:
        assert float(inv[0]) == np.float32(SENT) and float(inv[-1]) == np.float32(SENT), "inv_norm: guard written"
    if want_max:
        assert int(mx[0]) == -1 and int(mx[2]) == -1, "abs max: guard written"
    if S:
        assert bool((img[0] == 0x5555).all()) and bool((img[-1] == 0x5555).all()), "split image: guard rows written"
    return (inv[1:-1] if want_inv else None), (int(mx[1]) & 0xFFFFFFFF if want_max else None), (img[1:-1] if S else None)


def _pass(bank_d, img_d, S, inv_d, q_d, q0, T, groups, parts, split):
    """One pio_test_project_pass, twice (same bits).  The partial buffers start as ones between sentinel rows, `out` as sentinels.
    -> (m, l [parts][16 groups], acc [parts][16 groups][D], out [N][D]) as float64 numpy."""
    lib = _lib.load()
    M, D = bank_d.shape
    N = q_d.shape[0]
    rows = parts * 16 * groups
    res = []
    for _ in range(2):
        acc = torch.ones(rows + 2, D, device="cuda")
        ml = torch.ones(rows + 2, 2, device="cuda")
        out = torch.full((N + 2, D), SENT, device="cuda")
        acc[0], acc[-1], ml[0], ml[-1] = SENT, SENT, SENT, SENT
        check(lib.pio_test_project_pass(groups, int(split), ptr(bank_d), ptr(img_d) if split else None, float(S) if split else 0.0, ptr(inv_d), M, D,
                                        ptr(q_d), N, q0, float(T), parts, acc[1:].data_ptr(), ml[1:].data_ptr(), rows, out.data_ptr(), _stream()))
        res.append((acc, ml, out))
    (acc, ml, out), (acc2, ml2, out2) = res
    assert torch.equal(acc, acc2) and torch.equal(ml, ml2) and torch.equal(out, out2), "two calls differ"
    s = np.float32(SENT)
    assert bool((acc[0] == s).all() and (acc[-1] == s).all() and (ml[0] == s).all() and (ml[-1] == s).all()), "partial buffers: guard rows written"
    nq = min(N - q0, 16 * groups)
    keep = torch.cat([out[:q0], out[q0 + nq:]])
    assert bool((keep == s).all()), "rows of out outside the pass written"
    ml = ml[1:-1].view(parts, 16 * groups, 2).double().cpu().numpy()
    return ml[:, :, 0], ml[:, :, 1], acc[1:-1].view(parts, 16 * groups, D).double().cpu().numpy(), out[:N].double().cpu().numpy()


def _case_ratios(c, D, groups, split, magnitude=True):
    bank, inv, q, bounds, S = P.build_case(c, D, groups)
    bank_d = _dev(bank)
    img = _prep(bank_d, S)[2] if split else None
    m, l, acc, out = _pass(bank_d, img, S, _dev(inv), _dev(q), c["q0"], c["T"], groups, c["parts"], split)
    nq, q0 = c["nq"], c["q0"]
    qs = q[q0:]
    ref = P.partials64(bank, inv, qs, c["T"], bounds, split, S, magnitude)
    want, bar = P.merged64(bank, inv, qs, c["T"], bounds, split, S, magnitude)
    assert np.isfinite(out[q0:q0 + nq]).all()
    return (P.worst(m[:, :nq], ref["m"], ref["bar_m"]), P.worst(l[:, :nq], ref["l"], ref["bar_l"]),
            P.worst(acc[:, :nq], ref["acc"], ref["bar_acc"]), P.worst(out[q0:q0 + nq], want, bar))


# ------------------------------------------------------------------------------------------------ one bank pass
@pytest.mark.parametrize("split", FORMS, ids=IDS)
@pytest.mark.parametrize("D,groups", [(D, g) for D in P.WIDTHS for g in ((1, 2, 3) if D == 768 else (1, 2))])
def test_pass_partials_and_merge_vs_float64(D, groups, split):
    """Every workgroup's m, l and Acc and the merged rows within their bars on every case of project_ref64.hook_cases; empty workgroups
    report m = -inf, l = 0, Acc = 0 (the buffers held ones); finite output at T = 1e-3, where logits differ by hundreds."""
    worst = [(0.0, None)] * 4
    for c in P.hook_cases(D, groups):
        r = _case_ratios(c, D, groups, split)
        worst = [max(w, (x, "%s M %d parts %d nq %d T %g" % (c["family"], c["M"], c["parts"], c["nq"], c["T"])), key=lambda t: t[0])
                 for w, x in zip(worst, r)]
    print("\nD %4d groups %d %s  observed / bar:" % (D, groups, "split" if split else "exact"))
    for name, (x, what) in zip(("m", "l", "Acc", "out"), worst):
        print("    %-4s %.3f  (%s)" % (name, x, what))
    assert max(x for x, _ in worst) <= 1.0, worst


def test_hook_refuses_what_the_kernel_does_not_cover():
    lib = _lib.load()
    D, M = 768, 40
    bank = torch.randn(M, D, device="cuda")
    inv = 1.0 / bank.norm(dim=-1)
    q = torch.nn.functional.normalize(torch.randn(20, D, device="cuda"), dim=-1)
    img = _prep(bank, 4096.0)[2]
    acc, ml, out = torch.zeros(4096, D, device="cuda"), torch.zeros(4096, 2, device="cuda"), torch.full((20, D), SENT, device="cuda")

    def call(groups=1, split=1, image=img, S=4096.0, D_=D, N=20, q0=0, T=1.0, parts=4, rows=4096):
        return lib.pio_test_project_pass(groups, split, ptr(bank), ptr(image) if image is not None else None, S, ptr(inv), M, D_, ptr(q), N, q0, T,
                                         parts, ptr(acc), ptr(ml), rows, ptr(out), _stream())

    assert call() == 0
    for kw in (dict(D_=256), dict(D_=896), dict(groups=0), dict(groups=4), dict(split=2), dict(image=None), dict(S=0.0), dict(S=-4096.0),
               dict(S=3000.0), dict(S=float("inf")), dict(S=float("nan")), dict(parts=0), dict(parts=1025), dict(rows=63), dict(groups=2, rows=127),
               dict(q0=20), dict(q0=21), dict(q0=-1), dict(T=0.0), dict(T=float("nan"))):
        out.fill_(SENT)
        assert call(**kw) == -1, kw                                      # PIO_ERR_INVALID_ARG
        assert b"pio_test_project_pass" in lib.pio_last_error()
        torch.cuda.synchronize()
        assert bool((out == np.float32(SENT)).all()), kw                  # refused before any launch
    bank384 = torch.randn(M, 384, device="cuda")
    assert lib.pio_test_project_pass(3, 0, ptr(bank384), None, 0.0, ptr(inv), M, 384, ptr(q), 20, 0, 1.0, 4, ptr(acc), ptr(ml), 4096, ptr(out),
                                     _stream()) == -1                  # three query groups exist at D = 768 only
    assert lib.pio_test_bank_prep(ptr(bank), M, 100, 1.0, None, None, None, _stream()) == -1
    assert lib.pio_test_bank_prep(ptr(bank), M, D, 0.0, None, None, ptr(img), _stream()) == -1


# ------------------------------------------------------------------------------------------------ the split form's range
LADDER = tuple(range(0, 32, 2))


def _ladder_case(k, D=768, M=48, N=16):
    """Row 0 carries max|bank| and is nearly orthogonal to the queries; the other rows are Gaussians scaled so that their largest element is
    2^-k of it; query n equals row 1 + n, so m of the slab IS the logit of a small row (100 at T = 0.01) and its error the logit's."""
    rng = np.random.default_rng(900 + k)
    bank = rng.standard_normal((M, D))
    bank[0] *= 8.0 / np.abs(bank[0]).max()
    for r in range(1, M):
        bank[r] *= 8.0 * 2.0 ** -k / np.abs(bank[r]).max()
    bank = bank.astype(np.float32)
    return bank, P._unit(bank[1:1 + N].astype(np.float64))


@pytest.mark.parametrize("groups", [1, 2])
def test_split_form_ladder_of_row_magnitudes(groups):
    """Rows at 2^-k of max|bank|: the split pass stays inside the bar WITH its magnitude term at every k (the term assumes that conversion
    and matrix instruction keep fp16 subnormals); printed: the logit error (|m - m64| at T = 0.01) per k, and the first k at which the
    pass leaves the bar that holds at k = 0 (the bar without the term) -- the measured range of the split form."""
    D, T, parts = 768, 0.01, 2
    onset, lines = None, []
    for k in LADDER:
        bank, q = _ladder_case(k, N=16 * groups)
        inv = P.inv_norm64(bank).astype(np.float32)
        S = P.bank_scale(bank)
        bounds = P.slab_bounds(bank.shape[0], parts, 16 if groups == 1 else 32)
        bank_d = _dev(bank)
        img = _prep(bank_d, S)[2]
        m, l, acc, out = _pass(bank_d, img, S, _dev(inv), _dev(q), 0, T, groups, parts, True)
        with_term = P.partials64(bank, inv, q, T, bounds, True, S, True)
        plain = P.partials64(bank, inv, q, T, bounds, True, S, False)
        want, bar = P.merged64(bank, inv, q, T, bounds, True, S, True)
        r_term = max(P.worst(m, with_term["m"], with_term["bar_m"]), P.worst(l, with_term["l"], with_term["bar_l"]),
                     P.worst(acc, with_term["acc"], with_term["bar_acc"]), P.worst(out, want, bar))
        r_plain = max(P.worst(m, plain["m"], plain["bar_m"]), P.worst(l, plain["l"], plain["bar_l"]), P.worst(acc, plain["acc"], plain["bar_acc"]))
        ok = np.isfinite(with_term["m"])
        err = float(np.abs(m - with_term["m"])[ok].max())
        lines.append("    2^-%-2d  logit error %.2e   / bar with term %.3f   / bar of k = 0 %.3f" % (k, err, r_term, r_plain))
        if onset is None and r_plain > 1.0:
            onset = k
        assert r_term <= 1.0, lines
    print("\nsplit form, groups %d, rows at 2^-k of max|bank| (T = 0.01):" % groups)
    print("\n".join(lines))
    print("    first k outside the bar of k = 0: %s" % ("none up to %d" % LADDER[-1] if onset is None else onset))
    # the loader's rule rests on this measurement: the split form is chosen down to 2^-kSplitRangeBinades, two binades above the onset
    K = int(re.search(r"kSplitRangeBinades = (\d+);", open(os.path.join(ROOT, "patchioner_amd", "csrc", "api.cpp")).read()).group(1))
    assert onset is None or onset >= K + 2, "the split form leaves its plain bar at 2^-%d, inside the range the loader gives it (2^-%d)" % (onset, K)


# ------------------------------------------------------------------------------------------------ what loading a bank computes
@pytest.mark.parametrize("D", P.WIDTHS)
def test_bank_prep_inv_norm_split_image_and_abs_max(D):
    rng = np.random.default_rng(D)
    M = 67                                                        # not a multiple of the 4 rows per workgroup
    bank = rng.standard_normal((M, D)).astype(np.float32)
    bank[3] *= 1e15
    bank[4] *= 1e-15                                              # every square still a normal fp32
    bank[5] *= 3.0
    bank[6] *= 1e-3
    inv, _, _ = _prep(_dev(bank), want_inv=True)
    r = P.worst(inv.double().cpu().numpy(), P.inv_norm64(bank), P.inv_norm_bar(bank))
    print("\nD %4d  inv_norm observed / bar %.3f" % (D, r))
    assert r <= 1.0
    # the split image, bit for bit: ordinary rows, rows down the ladder (low halves, then high halves, subnormal and zero), ties, -0.0
    bank = rng.standard_normal((M, D)).astype(np.float32)
    for r_, k in enumerate(range(0, 40, 2)):
        bank[10 + r_] *= np.float32(2.0 ** -k)
    bank[0, :8] = [1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -1.0 - 2.0 ** -11, 2.0 ** -26, 2.0 ** -27 * 1.5, -0.0, 0.0, 2.0 ** -12]
    bank[1, 5] = -7.5                                             # the extreme is negative
    S = P.bank_scale(bank)
    assert S == 2.0 ** 12
    _, bits, img = _prep(_dev(bank), S, want_max=True)
    assert bits == P.abs_max_bits(bank) == int(np.float32(7.5).view(np.uint32))
    want = P.split_bank64(bank, S)
    got = img.cpu().numpy().view(np.uint16)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "split image differs at %d places, first [row, plane, channel] %s: %04x for %04x (x S = %r)" % (
        len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])], float(bank[bad[0][0], bad[0][2]]) * S)
    zero = np.zeros((5, D), np.float32)
    zero[2, 7] = -0.0
    assert _prep(_dev(zero), want_max=True)[1] == 0               # nothing above zero: -0.0 is no maximum
    zero[4, D - 1] = -2.0 ** -140                                 # a subnormal, negative, in the last element
    assert _prep(_dev(zero), want_max=True)[1] == P.abs_max_bits(zero) != 0


# ------------------------------------------------------------------------------------------------ top-k
def _engine(D, **kw):
    from patchioner_amd.engine import Engine
    dims = {768: (768, 12), 384: (384, 6)}[D]
    return Engine(embed_dim=dims[0], depth=1, num_heads=dims[1], num_registers=4, crop_dim=224, max_batch=1, max_prefixes=128, **kw)


@pytest.mark.parametrize("M", [16, 70, 1027])
def test_topk_rows_and_best_sims(M):
    """k = 1, 5, 16 (M = k at M = 16), M no multiple of 4 or 256, N = 17 (two batches of the similarity scratch), duplicate rows, queries
    that equal a row: similarities within their bar, an index away from float64's only inside it, equal rows in ascending order."""
    D, N = 384, 17
    rng = np.random.default_rng(M)
    bank = rng.standard_normal((M, D)).astype(np.float32)
    bank[::9] *= 3.0
    for dup in (3, 7, M - 1):
        bank[dup] = bank[11]                                      # four equal rows: 3, 7, 11, M - 1
    q = rng.standard_normal((N, D)).astype(np.float32)
    q[0], q[5], q[16] = bank[11], 2.5 * bank[M // 2], bank[3]     # queries that equal a (multiple) row: the ties lead the list
    c, bar = P.sims64(bank, q)
    e = _engine(D)
    try:
        assert e.set_memory_bank(torch.from_numpy(bank)) == M
        worst = 0.0
        for k in (1, 5, 16):
            sims, rows = e.topk_rows(_dev(q), k)
            sims, rows = sims.double().cpu().numpy(), rows.cpu().numpy()
            bad = P.topk_violations(c, bar, bank, sims, rows, k)
            assert not bad, bad[:5]
            if k >= 4:
                assert rows[0, :4].tolist() == [3, 7, 11, M - 1] and rows[16, :4].tolist() == [3, 7, 11, M - 1]
            _, best = e.project(_dev(q), n_best=k)
            vals, _ = P.topk64(c, k)
            ref_bar = np.take_along_axis(bar, P.topk64(c, k)[1], 1)
            worst = max(worst, P.worst(best.double().cpu().numpy(), vals, ref_bar), P.worst(sims, vals, ref_bar))
            assert torch.equal(best.cpu(), torch.from_numpy(sims).float()), "project(n_best) and topk_rows disagree"
        print("\nM %4d  top-k similarities observed / bar %.3f" % (M, worst))
        assert worst <= 1.0
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ the whole call
@pytest.mark.parametrize("split", FORMS, ids=IDS)
def test_whole_call_vs_float64(split):
    """Engine.project at M = 2049, D = 768: N = 1 .. 128 takes passes of 16, 32, 48, 48 + 16 (65), 48 + 32 (80), 32 + 32 (64), 48 + 48 + 32 (128);
    raw queries of any length (normalised in place), the loader's own inv_norm and split image, with and without the final normalisation."""
    M, D = 2049, 768
    rng = np.random.default_rng(2049)
    bank = rng.standard_normal((M, D)).astype(np.float32)
    bank[::97] *= 3.0
    bank[3::101] *= 1e-3
    old = os.environ.get("PIO_PROJECT_EXACT")
    if not split:
        os.environ["PIO_PROJECT_EXACT"] = "1"                   # read when the bank is loaded
    e = _engine(D)
    try:
        e.set_memory_bank(torch.from_numpy(bank))
    finally:
        if not split:
            if old is None:
                del os.environ["PIO_PROJECT_EXACT"]
            else:
                os.environ["PIO_PROJECT_EXACT"] = old
    S = P.bank_scale(bank)
    try:
        worst = {}
        for N in (1, 17, 33, 49, 64, 65, 80, 128):
            q = (rng.standard_normal((N, D)) * rng.uniform(0.1, 30.0, size=(N, 1))).astype(np.float32)
            for T, normalize in ((0.01, True), (0.01, False), (1.0, False)):
                qd = _dev(q)
                got = e.project(qd, temperature=T, normalize=normalize)
                again = e.project(_dev(q), temperature=T, normalize=normalize)
                assert torch.equal(got, again) and bool(torch.isfinite(got).all())
                want, bar = P.project64(bank, q, T, normalize, split, S)
                key = "T %g%s" % (T, " normalised" if normalize else "")
                worst[key] = max(worst.get(key, 0.0), P.worst(got.double().cpu().numpy(), want, bar))
                qn = q.astype(np.float64) / np.sqrt((q.astype(np.float64) ** 2).sum(-1, keepdims=True))
                assert float(np.abs(qd.double().cpu().numpy() - qn).max()) <= 8 * P.U32, "q is normalised in place"
        print("\nwhole call, %s  observed / bar: %s" % ("split" if split else "exact", ", ".join("%s %.3f" % kv for kv in worst.items())))
        assert max(worst.values()) <= 1.0, worst
    finally:
        e.close()


def test_exact_form_is_what_the_environment_variable_selects():
    """The two whole-call cases above must not silently run the same form: with PIO_PROJECT_EXACT the call equals, bit for bit, the hook's
    exact pass on the same operands; without it the hook's split pass."""
    M, D, N = 300, 768, 16
    rng = np.random.default_rng(7)
    bank = rng.standard_normal((M, D)).astype(np.float32)
    q = P._unit(rng.standard_normal((N, D)))
    outs = {}
    for split in FORMS:
        old = os.environ.get("PIO_PROJECT_EXACT")
        if not split:
            os.environ["PIO_PROJECT_EXACT"] = "1"
        e = _engine(D)
        try:
            e.set_memory_bank(torch.from_numpy(bank))
            assert e.bank_form() == ("split" if split else "exact")
            qd = _dev(q)
            outs[split] = e.project(qd, temperature=0.01)
            bank_d = _dev(bank)
            inv, _, img = _prep(bank_d, P.bank_scale(bank), want_inv=True)
            _, _, _, hook = _pass(bank_d, img, P.bank_scale(bank), inv.contiguous(), qd, 0, 0.01, 1, 512, split)
            assert np.array_equal(hook, outs[split].double().cpu().numpy()), "split" if split else "exact"
        finally:
            if not split:
                if old is None:
                    del os.environ["PIO_PROJECT_EXACT"]
                else:
                    os.environ["PIO_PROJECT_EXACT"] = old
            e.close()
    assert not torch.equal(outs[False], outs[True])


@pytest.mark.parametrize("outlier", [2.0 ** 16, 2.0 ** 30, -2.0 ** 40])
def test_bank_with_one_outlier_element_stays_inside_the_bar(outlier):
    """One huge element sets max|bank|, and with it the scale of the split image, for every other row.  The loader keeps the split form
    only while the smallest row norm is at or above sqrt(D) 2^-26 max|bank| (csrc/api.cpp: bank_common; the measured range is in DESIGN
    section 3): at 2^16 the split form still holds its plain bar (the bar of k = 0, no magnitude term); at 2^30 and 2^40 the rows would sit
    28 and 38 binades down -- the call must take the exact form and is held to the exact form's bar.  Which form the loader took is not
    this test's guess: Engine.bank_form() says it, and the call's bits are those of the hook's pass in that form and not of the other."""
    M, D, N = 300, 768, 17
    rng = np.random.default_rng(11)
    bank = rng.standard_normal((M, D)).astype(np.float32)
    bank[123, 45] = outlier
    q = rng.standard_normal((N, D)).astype(np.float32)
    q[0], q[1] = bank[7], bank[123]
    norms = np.sqrt((bank.astype(np.float64) ** 2).sum(-1))
    in_range = norms.min() >= np.sqrt(D) * 2.0 ** -26 * np.abs(bank).max()          # the loader's rule, restated
    assert in_range == (abs(outlier) < 2.0 ** 20)
    S = P.bank_scale(bank)
    e = _engine(D)
    try:
        e.set_memory_bank(torch.from_numpy(bank))
        assert e.bank_form() == ("split" if in_range else "exact")
        bank_d = _dev(bank)
        inv, _, img = _prep(bank_d, S, want_inv=True)
        worst = 0.0
        for T in (0.01, 1.0):
            qd = _dev(q)
            got = e.project(qd, temperature=T)                                    # 17 queries: one pass of two groups on parts / 2 workgroups
            want, bar = P.project64(bank, q, T, False, in_range, S, magnitude=False)
            assert bool(torch.isfinite(got).all())
            worst = max(worst, P.worst(got.double().cpu().numpy(), want, bar))
            same = {f: np.array_equal(_pass(bank_d, img, S, inv.contiguous(), qd, 0, T, 2, 256, f)[3], got.double().cpu().numpy()) for f in FORMS}
            assert same == {in_range: True, (not in_range): False}, same
        print("\noutlier %g: observed / bar of the %s form %.3f" % (outlier, e.bank_form(), worst))
        assert worst <= 1.0
    finally:
        e.close()
