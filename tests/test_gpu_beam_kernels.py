"""The device beam search against float64 and against a constructed statement of its selection and bookkeeping
(tests/beam_ref64.py), kernel by kernel and then whole:

  selection       k_beam_select through pio_test_beam_select at any V: dyadic inputs (fp32 arithmetic exact, so values and indices are held
                  bit for bit) at the edges of the per-thread top-8 lists and their merge -- ties across beams and inside one thread, all
                  winners owned by one thread, the last column and the last flat index, stopped beams, -inf and NaN columns; then random
                  fp32 inputs within the rounding of the candidate formula
  bookkeeping     ONE k_beam_step launch (pio_test_beam_step) against step_spec, every field bit for bit, the cells it must not write
                  holding sentinels
  head            lm_head_rows (pio_test_lm_head_rows): k_lm_logits_full and k_lm_logits_rows give the same bits, both within a
                  per-element bar of LN(x) wte^T in float64 from the UNFOLDED parameters; k_log_softmax_rows against log_softmax64
  per-image path  pio_lm_prefill / pio_lm_advance / pio_beam_select teacher-forced along the float64 search: all V log-probabilities of
                  all W rows at every step
  whole search    pio_lm_beam_search and VieCapHead.beam_search against beam64

Bars are derived, never fitted (u = 2^-24, SAFETY = 8 as in tests/decoder_ref64.py), functions of float64 quantities only:
  logits          decoder_ref64.layer_gemm64's bar of the LayerNorm form: the dot product, the mean, the one-pass variance, rsqrtf, the
                  epilogue (k_row_stats takes its statistics in one pass, as the layer GEMMs do)
  log-softmax     lp_v = d_v - log sum_w exp(d_w), d = logit - max.  The logit's own bar, the maximum's bar (the subtraction moves every d by
                  the error of the row's largest logit), the normaliser's: sum_w p_w (bar_w + bar_max) -- the relative error of a sum of
                  exponentials is the probability-weighted error of their arguments -- then the roundings: SAFETY u (|d_v| + 1) for the
                  subtraction, expf (whose argument's rounding error u |d| becomes a relative error of its value), the division and logf;
                  SAFETY u (sum_w p_w |d_w| + 1) for the same inside the sum; and the fp32 sum itself in the kernel's shape -- ceil(V /
                  1024) terms per thread in sequence, 6 levels of the wave tree, 16 wave partials in sequence: SAFETY u (ceil(V / 1024) + 22)
  with layers     test_gpu_viecap_kernels._nll_bar(layers, max |logit|) per log-probability; twice that on a margin between two candidates
Below a float64 log-probability of -80, expf(d) leaves the normal range and logf(expf(d) / s) has no relative accuracy: such an element only
has to be <= -80 + its bar, or -inf, never NaN.  Inputs drawn like model logits leave out no element (asserted); one constructed case
with logits spanning +-120 does, and asserts how many."""
import math

import numpy as np
import pytest
import torch

import beam_ref64 as B
import decoder_ref64 as D
import viecap_ref64 as R
from parity_helpers import MARGIN_BOUND
from patchioner_amd import _lib
from patchioner_amd import weights as W
from patchioner_amd._lib import check, ptr
from test_gpu_viecap_kernels import _model, _nll_bar, _report

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

F64 = torch.float64
U32, SAFETY = D.U32, D.SAFETY
E = D.E
NEG_INF, NAN = float("-inf"), float("nan")
SENT_F, SENT_I = 12345.678, -77
Q = 1024.0                                    # inputs are multiples of 2^-10


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ selection, exact
def _select(lp, scores, lens, stopped, W_, V_):
    """pio_test_beam_select on host tensors -> (values [W] float64 list, indices [W] list); the outputs sit between sentinels."""
    lib = _lib.load()
    val = torch.full((W_ + 4,), SENT_F, device="cuda")
    idx = torch.full((W_ + 4,), SENT_I, device="cuda", dtype=torch.int64)
    dev = [None if t is None else t.cuda().contiguous() for t in (lp, scores, lens, stopped)]
    check(lib.pio_test_beam_select(ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), ptr(dev[3]), W_, V_, val[2:].data_ptr(), idx[2:].data_ptr(), _stream()))
    val, idx = val.cpu(), idx.cpu()
    assert bool((val[:2] == np.float32(SENT_F)).all() and (val[W_ + 2:] == np.float32(SENT_F)).all()), "values written outside [0, W)"
    assert bool((idx[:2] == SENT_I).all() and (idx[W_ + 2:] == SENT_I).all()), "indices written outside [0, W)"
    return val[2:W_ + 2].double().tolist(), idx[2:W_ + 2].tolist()


def _dyadic_state(g, W_, V_):
    """lp in [-16, -1), scores in [-8, 0], multiples of 2^-10; lens in {1, 3, 7}; nothing stopped.  15360 distinct lp values: from V =
    50257 on, equal candidates across and inside beams arise by themselves as well."""
    lp = -(torch.randint(1024, 16 * 1024, (W_, V_), generator=g).float() / Q)
    scores = -(torch.randint(0, 8 * 1024, (W_,), generator=g).float() / Q)
    lens = torch.tensor([1.0, 3.0, 7.0])[torch.randint(0, 3, (W_,), generator=g)]
    return lp, scores, lens, torch.zeros(W_, dtype=torch.int32)


def _plant(lp, scores, lens, b, v, target):
    """Makes candidate (b, v) of a live beam exactly ``target`` (a multiple of 2^-10): lp = target (lens + 1) - scores, all dyadic."""
    lp[b, v] = target * (float(lens[b]) + 1.0) - float(scores[b])


def _stop(scores, lens, stopped, b, target):
    """Beam b stopped with scores / lens exactly ``target``: scores = target lens (a multiple of 2^-10 times 1, 3 or 7: exact in fp32)."""
    stopped[b] = 1
    scores[b] = target * float(lens[b])


def _selection_cases(W_, V_):
    """(label, lp, scores, lens, stopped, flat indices that must be among the winners) -- the expectation itself is select_spec's."""
    g = torch.Generator().manual_seed(1000 * W_ + V_)
    total = W_ * V_
    out = []
    # first selection: row 0 only.  The last column wins; a pair of equal values in one thread's list (v, v + 1024) or in neighbours
    lp, _, _, _ = _dyadic_state(g, W_, V_)
    v1 = 17 % V_
    v2 = v1 + 1024 if v1 + 1024 < V_ else (v1 + 1) % V_
    lp[0, V_ - 1] = 5.0
    if len({v1, v2, V_ - 1}) == 3:
        lp[0, v1] = lp[0, v2] = 4.0
    lp[1:] = 9.0                                                   # rows the first selection must not read
    out.append(("first", lp, None, None, None, [V_ - 1] + ([min(v1, v2)] if W_ >= 2 and len({v1, v2, V_ - 1}) == 3 else [])))
    # first selection, every winner owned by one thread: ids congruent to 7 mod 1024, equal values (ascending ids) and then a larger one last
    lp, _, _, _ = _dyadic_state(g, W_, V_)
    own = [v for v in range(7 % V_, V_, 1024)][:W_]
    for k, v in enumerate(own):
        lp[0, v] = 3.0
    lp[0, own[-1]] = 3.5
    out.append(("first, one thread", lp, None, None, None, own))
    # later selection: the same value at (0, v) and (W - 1, v); winners at flat index W V - 1 and in the last column of beam 0
    lp, sc, ln, st = _dyadic_state(g, W_, V_)
    _plant(lp, sc, ln, W_ - 1, V_ - 1, 3.0)
    want = [total - 1]
    if V_ >= 3:
        _plant(lp, sc, ln, 0, v1, 2.0)
        _plant(lp, sc, ln, W_ - 1, v1, 2.0)
        if W_ >= 2:
            _plant(lp, sc, ln, 0, V_ - 1, 1.5)
        want += [v1] if W_ >= 2 else []
    out.append(("later, ties across beams", lp, sc, ln, st, want))
    # later selection, every winner owned by one thread of k_beam_select (flat index congruent to 5 mod 1024) -- two children of one
    # parent among them wherever V > 1029 -- and by one thread of beam_topw (the same v in every beam)
    lp, sc, ln, st = _dyadic_state(g, W_, V_)
    own = [c for c in range(5 % total, total, 1024)][:W_]
    for c in own:
        _plant(lp, sc, ln, c // V_, c % V_, 2.0)
    out.append(("later, one thread (flat)", lp, sc, ln, st, own))
    lp, sc, ln, st = _dyadic_state(g, W_, V_)
    v3 = 1029 % V_
    for b in range(W_):
        _plant(lp, sc, ln, b, v3, 2.0 + (b % 2))
    out.append(("later, one column", lp, sc, ln, st, [b * V_ + v3 for b in range(W_)]))
    # stopped beams mixed in: odd beams stopped, their one live candidate v = 0 at the top; beam 0's (0, 1) ties with beam 1's (1, 0)
    lp, sc, ln, st = _dyadic_state(g, W_, V_)
    for b in range(1, W_, 2):
        _stop(sc, ln, st, b, 2.0 - b / Q)
        lp[b] = 9.0                                                # a stopped beam's log-probabilities must not be read as candidates
    if W_ >= 2 and V_ >= 2:
        _plant(lp, sc, ln, 0, 1, 2.0 - 1 / Q)
    out.append(("stopped beams mixed in", lp, sc, ln, st, [b * V_ for b in range(1, W_, 2)] + ([1] if W_ >= 2 and V_ >= 2 else [])))
    # all beams stopped: W candidates in all, equal pairs among them
    lp, sc, ln, st = _dyadic_state(g, W_, V_)
    for b in range(W_):
        _stop(sc, ln, st, b, -1.0 - (b // 2) / Q)
    out.append(("all stopped", lp, sc, ln, st, [b * V_ for b in range(W_)]))
    # -inf columns: the first 9300 flat candidates are -inf, so every thread's list is full of -inf (9 candidates per thread) before
    # its first finite value arrives; fewer finite candidates than W at the small sizes: -inf wins, by index
    for first in (True, False):
        lp, sc, ln, st = _dyadic_state(g, W_, V_)
        n = (V_ if first else total)
        cut = max(0, min(n - 3, 9300))
        lp.view(-1)[:cut] = NEG_INF
        if not first and W_ >= 3:
            _stop(sc, ln, st, W_ - 1, -20.0)                        # below every live candidate, above -inf
        out.append(("-inf columns, %s" % ("first" if first else "later"), lp, None if first else sc, None if first else ln,
                    None if first else st, []))
    # NaN columns: a third of the columns, column 0 among them; a NaN is never selected, whatever stands next to it
    for first in (True, False):
        lp, sc, ln, st = _dyadic_state(g, W_, V_)
        cols = (torch.rand(V_, generator=g) < 0.34).nonzero().flatten()
        lp[:, cols] = NAN
        lp[0, 0] = NAN
        if not first and W_ >= 2:
            _stop(sc, ln, st, 1, -0.5)
            lp[1] = NAN
        out.append(("NaN columns, %s" % ("first" if first else "later"), lp, None if first else sc, None if first else ln,
                    None if first else st, []))
    return out


@pytest.mark.parametrize("V_", [37, 1023, 1024, 1025, 2049, 50257])
def test_selection_exact(V_):
    """Every case at W = 1, 2, 5, 8: values and indices equal select_spec on candidates64, bit for bit (dyadic inputs)."""
    _check_selection_exact([(W_, V_) for W_ in (1, 2, 5, 8)])


def test_selection_exact_at_a_vocabulary_of_w():
    """V = W: the first selection takes the whole row, a later one W of W^2 candidates."""
    _check_selection_exact([(W_, W_) for W_ in (1, 2, 5, 8)])


def _check_selection_exact(sizes):
    n = 0
    for W_, V_ in sizes:
        for label, lp, sc, ln, st, planted in _selection_cases(W_, V_):
            cand = B.candidates64(lp[0] if sc is None else lp, sc, ln, None if st is None else st.tolist())
            vals, idx = B.select_spec(cand, W_)
            assert set(planted[:W_]) <= set(idx), ("the case is not what it claims", label, W_, V_, planted, idx)
            got_v, got_i = _select(lp, sc, ln, st, W_, V_)
            assert got_i == idx, (label, W_, V_, got_i, idx)
            assert got_v == vals, (label, W_, V_, got_v, vals)
            n += 1
    print("selection exact: %d cases at (W, V) = %s equal to select_spec bit for bit" % (n, sizes))


# ------------------------------------------------------------------------------------------------ selection, rounded
@pytest.mark.parametrize("V_", [37, 1025, 50257])
def test_selection_rounded(V_):
    """Random fp32 inputs.  A candidate is two roundings away from its float64 value (the sum, the quotient; lens + 1 is exact), one on
    the first selection and for a stopped beam: each returned value within 3 u |value64| of the float64 value of the candidate it names,
    and rank r's candidate no more than twice that below the float64 rank-r value (both may have moved, toward each other)."""
    worst_v, worst_r = 0.0, 0.0
    for W_ in (1, 5, 8):
        g = torch.Generator().manual_seed(31 * W_ + V_)
        for first in (True, False):
            lp = torch.log_softmax(3.0 * torch.randn(W_, V_, generator=g), dim=-1)
            sc = -(torch.rand(W_, generator=g) * 30.0 + 0.1)
            ln = torch.randint(1, 21, (W_,), generator=g).float()
            st = torch.zeros(W_, dtype=torch.int32)
            if W_ >= 5:
                st[1], st[3] = 1, 1
            cand = B.candidates64(lp[0] if first else lp, None if first else sc, None if first else ln, None if first else st.tolist()).reshape(-1)
            ref_v, _ = B.select_spec(cand, W_)
            got_v, got_i = _select(lp, None if first else sc, None if first else ln, None if first else st, W_, V_)
            assert len(set(got_i)) == W_ and all(0 <= i < cand.numel() for i in got_i), got_i
            for r in range(W_):
                c = float(cand[got_i[r]])
                tol = 3 * U32 * abs(c)
                worst_v = max(worst_v, abs(got_v[r] - c) / abs(c))
                assert abs(got_v[r] - c) <= tol, (W_, V_, first, r, got_v[r], c)
                tol_r = 2 * 3 * U32 * abs(ref_v[r])
                worst_r = max(worst_r, (ref_v[r] - c) / abs(ref_v[r]))
                assert ref_v[r] - c <= tol_r, (W_, V_, first, r, c, ref_v[r])
                assert r == 0 or got_v[r] <= got_v[r - 1]
    _report("selection V=%d: returned value against its candidate (relative)" % V_, worst_v, 3 * U32)
    _report("selection V=%d: rank r's candidate below the float64 rank r (relative)" % V_, worst_r, 6 * U32)


# ------------------------------------------------------------------------------------------------ k_beam_step
def _mul32(a, b):
    return float(np.float32(a) * np.float32(b))


SCENARIOS = ("identity", "swap", "one parent", "stopped parent", "frozen", "eos", "reverse")


def _image_case(g, kind, W_, V_, step, P, r0, steps, tstride):
    """State of one image before selection ``step`` and its log-probabilities, built so that the selection does what ``kind`` says."""
    lp, sc, ln, st = _dyadic_state(g, W_, V_)
    state = B.new_state(W_, P, steps, r0=r0, tstride=tstride)
    eos = []
    if step == 0:
        toks = torch.randperm(V_, generator=g)[:W_].tolist()
        for k, t in enumerate(toks):
            lp[0, t] = 3.0 - (k // 2) / Q                               # pairs of equal values: the lower id first
        if kind == "eos":
            eos = [sorted(toks)[0]]
        return state, lp[:1], eos
    pos = P + step - 1
    state["scores"], state["lens"] = sc.tolist(), ln.tolist()
    state["tok"] = torch.randint(0, V_, (W_,), generator=g).tolist()
    state["hist"] = [[1000 * b + k if k < step else SENT_I for k in range(steps)] for b in range(W_)]
    state["tab"] = [[100 * (r0 + b) + j if j <= pos else SENT_I - j for j in range(tstride)] for b in range(W_)]
    v = torch.randperm(V_, generator=g)[:W_].tolist()
    if W_ == 1 and kind in ("swap", "one parent", "stopped parent", "reverse"):
        kind = "identity"
    if kind == "identity":
        for b in range(W_):
            _plant(lp, sc, ln, b, v[b], 3.0 - b / Q)
    elif kind == "swap":                                                # rank 0 from beam 1, rank 1 from beam 0, the others in place
        order = [1, 0] + list(range(2, W_))
        for r, b in enumerate(order):
            _plant(lp, sc, ln, b, v[b], 3.0 - r / Q)
    elif kind == "reverse":                                             # rank r from beam W - 1 - r: every row's source is overwritten
        for r in range(W_):                                             # before or after it is read, whichever order the rows are written in
            _plant(lp, sc, ln, W_ - 1 - r, v[r], 3.0 - r / Q)
    elif kind == "one parent":                                          # W children of the last beam, equal values in pairs
        for r in range(W_):
            _plant(lp, sc, ln, W_ - 1, v[r], 3.0 - (r // 2) / Q)
    elif kind == "stopped parent":                                      # beam 0 stopped and chosen through v = 0; the other winners are children of beam 1
        _stop(sc, ln, st, 0, 3.0)
        lp[0] = 9.0
        for r in range(1, W_):
            _plant(lp, sc, ln, 1, v[r], 3.0 - r / Q)
    elif kind == "frozen":
        for b in range(W_):
            _stop(sc, ln, st, b, -1.0 - b / Q)
    elif kind == "eos":
        for b in range(W_):
            _plant(lp, sc, ln, b, v[b], 3.0 - b / Q)
        eos = [v[W_ // 2]]
    state["scores"], state["lens"], state["stopped"] = sc.tolist(), ln.tolist(), st.tolist()
    return state, lp, eos


def _launch_step(lp, N, W_, V_, step, eos, st, steps, tstride, wte, wpe, npos, E_):
    """One pio_test_beam_step on device tensors; st: the state arrays by name (views past their guard rows)."""
    check(_lib.load().pio_test_beam_step(ptr(lp), N, W_, V_, step, eos[0], eos[1], st["prow"].data_ptr(), st["scores"].data_ptr(),
                                         st["lens"].data_ptr(), st["stopped"].data_ptr(), st["tok"].data_ptr(), st["hist"].data_ptr(), steps,
                                         st["tab"].data_ptr(), tstride, ptr(wte), ptr(wpe), npos, E_, st["x"].data_ptr(), _stream()))


def _run_step(N, W_, V_, step, steps, P_of, tstride, npos, kinds=SCENARIOS, seed=0):
    """N images, image n of scenario kinds[n % len]: one launch, every field against step_spec, sentinels around and inside."""
    g = torch.Generator().manual_seed(7 * N + 13 * W_ + V_ + 101 * step + seed)
    R_, E8, G = N * W_, 8, 2                                         # G guard rows in front of and behind every array
    wte = torch.randn(V_, E8, generator=g)
    wpe = torch.randn(npos, E8, generator=g)
    states, lps, eos = [], [], []
    for n in range(N):
        s, lp, e = _image_case(g, kinds[n % len(kinds)], W_, V_, step, P_of(n), n * W_, steps, tstride)
        states.append(s)
        lps.append(lp)
        eos += e
    eos = (eos + [-5, -5])[:2]                                       # two ids; -5 matches no token
    lp_all = torch.cat(lps).contiguous()                             # step 0: [N][V]; later: [N W][V]

    def guarded(cols, dtype, fill):
        return torch.full((R_ + 2 * G, cols), fill, dtype=dtype) if cols else torch.full((R_ + 2 * G,), fill, dtype=dtype)

    sent_f, sent_i = float(np.float32(SENT_F)), SENT_I
    bufs = {"scores": guarded(0, torch.float32, sent_f), "lens": guarded(0, torch.float32, sent_f),
            "stopped": guarded(0, torch.int32, sent_i), "tok": guarded(0, torch.int32, sent_i),
            "hist": guarded(steps, torch.int32, sent_i), "tab": guarded(tstride, torch.int32, sent_i),
            "x": guarded(E8, torch.float32, sent_f), "prow": guarded(0, torch.int32, sent_i)}
    for n, s in enumerate(states):
        for b in range(W_):
            r = G + n * W_ + b
            bufs["prow"][r] = s["P"]
            if step > 0:
                bufs["scores"][r], bufs["lens"][r], bufs["stopped"][r], bufs["tok"][r] = s["scores"][b], s["lens"][b], s["stopped"][b], s["tok"][b]
                bufs["hist"][r] = torch.tensor(s["hist"][b], dtype=torch.int32)
                bufs["tab"][r] = torch.tensor(s["tab"][b], dtype=torch.int32)
    if step == 0:                                                    # what step 0 must not read or write stays a sentinel
        for n, s in enumerate(states):
            s["scores"], s["lens"], s["stopped"], s["tok"] = [sent_f] * W_, [sent_f] * W_, [sent_i] * W_, [sent_i] * W_
            s["hist"] = [[sent_i] * steps for _ in range(W_)]
            s["tab"] = [[sent_i] * tstride for _ in range(W_)]
    dev = {k: t.cuda() for k, t in bufs.items()}
    wte_d, wpe_d, lp_d = wte.cuda(), wpe.cuda(), lp_all.cuda()
    _launch_step(lp_d, N, W_, V_, step, eos, {k: t[G:] for k, t in dev.items()}, steps, tstride, wte_d, wpe_d, npos, E8)
    got = {k: t.cpu() for k, t in dev.items()}
    for k, t in got.items():
        fill = sent_f if t.dtype == torch.float32 else sent_i
        assert bool((t[:G] == fill).all() and (t[G + R_:] == fill).all()), "guard rows of %s written" % k
    seen = {"frozen": 0, "dup": 0, "stopped src": 0, "eos": 0}
    for n, s in enumerate(states):
        rows = slice(G + n * W_, G + (n + 1) * W_)
        frozen = step > 0 and all(s["stopped"])
        if frozen:
            new = B.step_spec(s, step, None, None, V_, eos, npos, mul=_mul32)
        else:
            lp = lps[n]
            cand = B.candidates64(lp[0]) if step == 0 else B.candidates64(lp, s["scores"], s["lens"], s["stopped"])
            vals, flat = B.select_spec(cand, W_)
            new = B.step_spec(s, step, vals, flat, V_, eos, npos, mul=_mul32)
        label = (kinds[n % len(kinds)], n, W_, V_, step)
        assert got["scores"][rows].double().tolist() == [float(np.float32(v)) for v in new["scores"]], ("scores",) + label
        assert got["lens"][rows].double().tolist() == [float(np.float32(v)) for v in new["lens"]], ("lens",) + label
        assert got["stopped"][rows].tolist() == new["stopped"], ("stopped",) + label
        assert got["tok"][rows].tolist() == new["tok"], ("tok",) + label
        assert got["hist"][rows].tolist() == new["hist"], ("hist",) + label
        assert got["tab"][rows].tolist() == new["tab"], ("tab",) + label
        assert got["prow"][rows].tolist() == [s["P"]] * W_
        tok = torch.tensor(new["tok"]).clamp(0, V_ - 1)
        want_x = wte[tok] + wpe[new["xpos"]]
        assert torch.equal(got["x"][rows], want_x), ("x",) + label
        seen["frozen"] += new["frozen"]
        if new["src"] is not None:
            seen["dup"] += len(set(new["src"])) < W_
            seen["stopped src"] += any(s["stopped"][b] for b in new["src"])
        seen["eos"] += any(t in eos for t in new["tok"])
    return seen


@pytest.mark.parametrize("N,W_,V_", [(1, 1, 37), (16, 5, 1500), (16, 8, 37), (1, 8, 1500), (16, 1, 37)])
def test_beam_step_first_selection(N, W_, V_):
    """Step 0: the W largest of row n (equal values in pairs), scores = values, lens = 1, the stop flag of an eos among the winners,
    the token into hist[.][0]; tab and the rest of hist are not touched."""
    seen = _run_step(N, W_, V_, 0, 16, lambda n: 1 + 3 * n, 64, 128, kinds=("identity", "eos"))
    assert N == 1 or seen["eos"] >= 1


@pytest.mark.parametrize("N,W_,V_", [(1, 1, 37), (16, 5, 1500), (16, 8, 37), (16, 8, 1500), (1, 5, 37), (16, 1, 1500)])
def test_beam_step_later_selection(N, W_, V_):
    """A later step with, image by image: src = identity, a swap, one parent with W children, a stopped parent chosen through v = 0, a
    frozen image (nothing but x changes) beside live ones, an eos among the winners, the beams in reverse order."""
    seen = _run_step(N, W_, V_, 5, 16, lambda n: 1 + 2 * n, 64, 128)
    if N == 16:
        assert seen["frozen"] >= 2 and seen["eos"] >= 2
        if W_ > 1:
            assert seen["dup"] >= 2 and seen["stopped src"] >= 2


@pytest.mark.parametrize("W_", [1, 5, 8])
def test_beam_step_at_its_limits(W_):
    """P + step = npos (the next input's position is clamped to the last row of wpe); P + step - 1 = 255 with a table of 256 columns;
    steps = 64 at step 63."""
    _run_step(3, W_, 37, 6, 16, lambda n: 10, 64, 16)                       # P + step = 16 = npos
    _run_step(3, W_, 37, 6, 16, lambda n: 12, 64, 16, seed=1)               # beyond it
    _run_step(3, W_, 1500, 6, 16, lambda n: 250 - n, 256, 1024)             # image 0: P + step - 1 = 255
    _run_step(7, W_, 37, 63, 64, lambda n: 1 + n, 128, 1024)


def test_beam_hooks_refuse_what_the_kernels_do_not_hold():
    """Only arguments the hooks reject before launching anything: every call returns PIO_ERR_INVALID_ARG (-1), buffers keep their sentinels."""
    lib = _lib.load()
    W_, V_, steps, ts = 2, 16, 8, 32
    f = torch.full((64,), 3.0, device="cuda")
    i32 = torch.full((512,), 4, device="cuda", dtype=torch.int32)
    i64 = torch.full((16,), 5, device="cuda", dtype=torch.int64)
    prow = torch.tensor([10, 10, 28, 28], device="cuda", dtype=torch.int32)

    def step(N=2, W=W_, V=V_, step=1, steps=steps, ts=ts, prow=prow, lp=f):
        return lib.pio_test_beam_step(ptr(lp), N, W, V, step, -1, -1, ptr(prow), ptr(f), ptr(f), ptr(i32), ptr(i32), ptr(i32), steps, ptr(i32), ts,
                                      ptr(f), ptr(f), 4, 2, ptr(f), _stream())

    for kw in (dict(W=0), dict(W=9), dict(V=1), dict(steps=0), dict(steps=65), dict(step=8), dict(step=-1), dict(ts=257), dict(ts=0),
               dict(N=0), dict(N=129), dict(lp=None), dict(step=6), dict(prow=torch.zeros(4, device="cuda", dtype=torch.int32))):
        assert step(**kw) == -1, kw                                  # step = 6: image 1 has P + step - 1 = 33 >= tstride
    assert lib.pio_test_beam_select(ptr(f), None, None, None, 9, 16, ptr(f), ptr(i64), _stream()) == -1
    assert lib.pio_test_beam_select(ptr(f), None, None, None, 0, 16, ptr(f), ptr(i64), _stream()) == -1
    assert lib.pio_test_beam_select(ptr(f), None, None, None, 5, 4, ptr(f), ptr(i64), _stream()) == -1
    assert lib.pio_test_beam_select(ptr(f), ptr(f), None, None, 2, 16, ptr(f), ptr(i64), _stream()) == -1
    assert lib.pio_test_beam_select(None, None, None, None, 2, 16, ptr(f), ptr(i64), _stream()) == -1
    for kw in (dict(kind=2), dict(kind=-1), dict(rows=0), dict(rows=257), dict(V=0), dict(eps=0.0)):
        a = dict(kind=0, rows=1, V=4, eps=1e-5)
        a.update(kw)
        assert lib.pio_test_lm_head_rows(a["kind"], ptr(f), ptr(f), ptr(f), a["eps"], ptr(f), a["rows"], a["V"], 0, ptr(f), ptr(f), _stream()) == -1, kw
    torch.cuda.synchronize()
    assert bool((f == 3.0).all() and (i32 == 4).all() and (i64 == 5).all())


# ------------------------------------------------------------------------------------------------ head
HEAD_ROWS = (1, 16, 17, 128)
WIDE_RANGE_LEFT_OUT = 10877          # of 17 x 1025 float64 log-probabilities of the constructed case, those below -80


def _head_x():
    """128 rows: scales 1e-3 .. 1e3 by row, every fourth row three massive channels (1e2, 3e2, -1e3), every eighth a common offset of
    10 standard deviations."""
    x = D.x_family("scales", 128, E, seed=3)
    m = D.x_family("massive", 128, E, seed=3)
    x[3::4] = m[0:64:2]
    x[5::8] = m[1:32:2]
    return x.contiguous()


def _head_case(V_, gain=1.0):
    """wte as the seeded models draw it (std 0.02: logits of a few units) times ``gain``, a LayerNorm with gains around 1."""
    g = torch.Generator().manual_seed(50 + V_)
    wte = (0.02 * gain * torch.randn(V_, E, generator=g)).contiguous()
    wte[:1] = wte[:1].abs()
    return {"name": "head", "Nout": V_, "K": E, "epi": D.STORE, "ln": True, "eps": 1e-5, "W": wte, "b": torch.zeros(V_),
            "ln_w": (1.0 + 0.2 * torch.randn(E, generator=g)).contiguous(), "ln_b": (0.1 * torch.randn(E, generator=g)).contiguous()}


def _fold(c):
    lib = _lib.load()
    V_ = c["Nout"]
    w, cv, dv = torch.empty(V_, E), torch.empty(V_), torch.empty(V_)
    check(lib.pio_host_ln_fold(c["W"].data_ptr(), 0, E, V_, c["ln_w"].data_ptr(), c["ln_b"].data_ptr(), None, w.data_ptr(), cv.data_ptr(), dv.data_ptr()))
    return w.cuda(), cv.cuda(), dv.cuda()


def _head(kind, ops, c, x, rows, log_softmax):
    lib = _lib.load()
    V_ = c["Nout"]
    buf = torch.full((rows + 4, V_), SENT_F, device="cuda")
    stats = torch.full((rows + 2, 2), SENT_F, device="cuda")
    check(lib.pio_test_lm_head_rows(kind, ptr(ops[0]), ptr(ops[1]), ptr(ops[2]), c["eps"], ptr(x), rows, V_, int(log_softmax), ptr(stats),
                                    buf[2:].data_ptr(), _stream()))
    assert bool((buf[:2] == SENT_F).all() and (buf[rows + 2:] == SENT_F).all()), "guard rows written (rows = %d, V = %d)" % (rows, V_)
    assert bool((stats[rows:] == SENT_F).all()), "statistics written past the rows"
    return buf[2:rows + 2]


def _lp_reference(logits64, bar_logit, V_):
    """(log-probabilities, their bar) from float64 logits and the logits' bar; see the module docstring."""
    lp = B.log_softmax64(logits64)
    p = lp.exp()
    top = logits64.argmax(dim=-1, keepdim=True)
    d = logits64 - logits64.gather(1, top)
    bar_max = bar_logit.gather(1, top)
    inside = (p * (bar_logit + bar_max)).sum(-1, keepdim=True) + SAFETY * U32 * ((p * d.abs()).sum(-1, keepdim=True) + 1.0)
    bar = bar_logit + bar_max + inside + SAFETY * U32 * (d.abs() + 1.0) + SAFETY * U32 * (math.ceil(V_ / 1024) + 22)
    return lp, bar


def _check_lp(got, lp64, bar, label):
    """-> (worst observed / bar over the elements at or above -80, elements left out)."""
    assert not bool(torch.isnan(got).any()), label + ": NaN"
    keep = lp64 >= -80.0
    g = got.double()
    err = (g - lp64).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    worst = float((err[keep] / bar[keep]).max())
    low = ~keep
    assert bool((g[low] <= -80.0 + bar[low]).all()), label + ": an element whose float64 log-probability is below -80 came out above it"
    return worst, int(low.sum())


@pytest.mark.parametrize("V_", [1, 7, 8, 9, 31, 33, 1025, 50257])
def test_head_vs_float64(V_):
    """rows in 1, 16, 17, 128: k_lm_logits_full and k_lm_logits_rows give the same bits (logits and log-probabilities), and both sit
    within the per-element bars of the float64 head on the unfolded parameters.  V = 1: the log-probability is exactly 0."""
    c = _head_case(V_)
    x = _head_x()
    ref, bar_fn = D.layer_gemm64(c, x)
    bar = bar_fn(U32)
    lp64, bar_lp = _lp_reference(ref, bar, V_)
    assert float(lp64.min()) >= -80.0
    ops, xd = _fold(c), x.cuda()
    ref_d, bar_d, lp_d, barlp_d = ref.cuda(), bar.cuda(), lp64.cuda(), bar_lp.cuda()
    worst, worst_lp = 0.0, 0.0
    for rows in HEAD_ROWS:
        full, each = _head(0, ops, c, xd, rows, False), _head(1, ops, c, xd, rows, False)
        assert torch.equal(full, each), "logits differ between the two kernels (rows %d, V %d)" % (rows, V_)
        worst = max(worst, D.worst_ratio(full, ref_d[:rows], bar_d[:rows]))
        full, each = _head(0, ops, c, xd, rows, True), _head(1, ops, c, xd, rows, True)
        assert torch.equal(full, each), "log-probabilities differ between the two kernels (rows %d, V %d)" % (rows, V_)
        r, left_out = _check_lp(full, lp_d[:rows], barlp_d[:rows], "rows %d V %d" % (rows, V_))
        assert left_out == 0
        worst_lp = max(worst_lp, r)
        if V_ == 1:
            assert bool((full == 0.0).all())
    print("head V=%d: max |logit| %.2f, min float64 log-probability %.2f" % (V_, float(ref.abs().max()), float(lp64.min())))
    _report("head V=%d logits, rows 1..128 (observed / bar)" % V_, worst, 1.0)
    _report("head V=%d log-probabilities, rows 1..128 (observed / bar)" % V_, worst_lp, 1.0)


def test_head_log_softmax_over_a_wide_range():
    """The one constructed case: wte 48 times larger, logits from -125 to 128.  Elements at or above -80 are held to their bars; the
    others only have to stay below -80 (+ bar) or be -inf, and are counted."""
    V_ = 1025
    c = _head_case(V_, gain=48.0)
    x = _head_x()[:17].contiguous()
    ref, bar_fn = D.layer_gemm64(c, x)
    lp64, bar_lp = _lp_reference(ref, bar_fn(U32), V_)
    assert float(ref.max()) > 100.0 and float(ref.min()) < -100.0, (float(ref.min()), float(ref.max()))
    ops, xd = _fold(c), x.cuda()
    full, each = _head(0, ops, c, xd, 17, True), _head(1, ops, c, xd, 17, True)
    assert torch.equal(full, each)
    worst, left_out = _check_lp(full, lp64.cuda(), bar_lp.cuda(), "wide range")
    print("wide range: logits %.1f .. %.1f, %d of %d elements below -80" % (float(ref.min()), float(ref.max()), left_out, lp64.numel()))
    assert left_out == WIDE_RANGE_LEFT_OUT
    _report("head log-probabilities over +-120 (observed / bar, elements >= -80)", worst, 1.0)




# ------------------------------------------------------------------------------------------------ per-image path and whole search
LAYERS = 2


class _IdTokenizer:
    """Token strings are their ids: lets the host loop take eos ids the seeded model emits (its own vocabulary has 471 entries)."""
    pad_token_id = 0

    def encode(self, s):
        return [int(s)]

    def decode(self, ids):
        return " ".join(str(int(i)) for i in ids)


@pytest.fixture(scope="module")
def beam_case():
    """The 2-layer head on which every wte row is live, its float64 model, the eight prompts of the recipe (0.3 randn, seed 7, lengths
    1, 5, 16, 17, 24, 3, 10, 31) and two eos ids the float64 search emits."""
    vocab, merges = W.synth_bpe(0)
    from patchioner_amd import viecap as VC
    tok = VC.ByteLevelBPE(vocab, merges)
    w = W.synth_viecap(491, clip_hidden_size=768, n_layer=LAYERS, tok_vocab=50257, map_layers=1)
    ents = list(W.SYNTH_ENTITIES)
    m = _model(w, tok, ents, W.synth_entity_embeddings(7, len(ents), 768), 768, max_prefixes=128, using_greedy_search=False, beam_width=5)
    ref = R.GPT2_64(w)
    assert ref.live.numel() == ref.V == 50257
    g = torch.Generator().manual_seed(7)
    prompts = [torch.randn(P, 768, generator=g) * 0.3 for P in (1, 5, 16, 17, 24, 3, 10, 31)]
    eos = (B.beam64(ref, prompts[2], 5, 16, (-1, -1))["ids"][0][4], B.beam64(ref, prompts[5], 5, 16, (-1, -1))["ids"][1][6])
    yield m, ref, prompts, eos
    m.engine.close()


def _cand32(lp, scores, lens, stopped):
    """k_beam_select's candidates from fp32 inputs in fp32 arithmetic (IEEE sum and quotient: the kernel's own values)."""
    if scores is None:
        return lp[:1].clone()
    out = (scores[:, None] + lp) / (lens[:, None] + 1.0)
    for b in range(lp.shape[0]):
        if int(stopped[b]):
            out[b] = NEG_INF
            out[b, 0] = scores[b] / lens[b]
    return out


@pytest.mark.parametrize("P,W_,pick,stop_steps", [(1, 5, (0, 3, 4, 8), 2), (5, 1, (0, 3, 0, 8), 1), (16, 8, (0, 3, 7, 8), 2), (17, 16, (0, 3, 15, 8), 1),
                                                  (24, 5, (0, 3, 0, 9), 2), (31, 8, (0, 3, 7, 8), 2), (241, 5, (0, 3, 4, 8), 2)])
def test_per_image_path_teacher_forced(beam_case, P, W_, pick, stop_steps):
    """beam64 first; the device follows ITS tokens and source rows, so no departure accumulates: at every step all V log-probabilities
    of all W rows within _nll_bar of the float64 ones, and (W <= 8: the selection kernel's limit) the device's selection on its own
    log-probabilities equal to select_spec on them.  P = 241: the last of the 16 steps writes position max_steps - 1 = 255.
    The eos ids are tokens this very search emits without any (beam pick[0] at step pick[1], beam pick[2] at step pick[3]), so that beams
    stop, at ``stop_steps`` different steps at least (checked here on the float64 search; at W = 16 a stopped beam is soon dropped and
    only one step stops any)."""
    m, ref, prompts, eos = beam_case
    eng = m.engine
    g = torch.Generator().manual_seed(1000 + P)
    emb = next((p for p in prompts if p.shape[0] == P), None)
    if emb is None:
        emb = torch.randn(P, 768, generator=g) * 0.3
    free = B.beam64(ref, emb, W_, 16, (-1, -1))               # eos ids this very search emits: its beams stop at different steps
    eos_ = (free["ids"][pick[0]][pick[1]], free["ids"][pick[2]][pick[3]])
    worst, dup, stops, nsel, prev, count = (0.0, 0.0, 1.0), 0, [], 0, None, 0
    for rec in B.beam64_steps(ref, emb, W_, 16, eos_):
        i = rec["step"]
        if i == 0:
            lp = eng.lm_prefill(emb[None].expand(W_, -1, -1).contiguous())
        else:
            src = None if prev["src"] is None else torch.tensor(prev["src"], dtype=torch.int32)
            lp = eng.lm_advance(torch.tensor(prev["tok"], dtype=torch.int32), src, pos=P + i - 1)
        lp = lp.cpu()
        assert bool(torch.isfinite(lp).all())
        bar = float(_nll_bar(LAYERS, rec["amax"]))
        err = float((lp.double() - rec["lp"]).abs().max())                       # step 0: W identical rows against the one float64 row
        worst = max(worst, (err / bar, err, bar))
        assert err <= bar, "step %d: a log-probability is %.3e from float64, bar %.3e" % (i, err, bar)
        if W_ <= 8:
            if i == 0:
                sc = ln = st = None
            else:
                sc = torch.tensor(prev["scores"], dtype=torch.float32)
                ln = torch.tensor(prev["lens"], dtype=torch.float32)
                st = torch.tensor(prev["stopped"], dtype=torch.int32)
            val, idx = eng.beam_select(lp.cuda(), sc, ln, st)
            want_v, want_i = B.select_spec(_cand32(lp, sc, ln, st), W_)
            assert idx.tolist() == want_i and val.double().tolist() == want_v, "step %d: the selection on the device's own log-probabilities" % i
            nsel += 1
        prev = rec["state"]
        if prev["src"] is not None:
            dup += len(set(prev["src"])) < W_
        if sum(prev["stopped"]) > count:
            stops.append(i)
        count = sum(prev["stopped"])
    assert W_ == 1 or dup >= 1, "no selection took two children of one parent"
    assert len(stops) >= stop_steps, "beams should stop at %d different steps: %s" % (stop_steps, stops)
    print("per-image P=%d W=%d: %d selections equal to select_spec, %d with duplicate sources, beams stop at steps %s" % (P, W_, nsel, dup, stops))
    _report("per-image P=%d W=%d log-probabilities (step nearest its bar)" % (P, W_), worst[1], worst[2])


def _first_departure(ids, ref_ids):
    """The first selection at which any beam's history differs (None: identical)."""
    t = None
    for a, b in zip(ids, ref_ids):
        n = min(len(a), len(b))
        d = next((k for k in range(n) if a[k] != b[k]), n if len(a) != len(b) else None)
        if d is not None:
            t = d if t is None else min(t, d)
    return t


def test_whole_search_vs_float64(beam_case, monkeypatch):
    """pio_lm_beam_search (one call, eight images) and VieCapHead.beam_search (image by image) against beam64: ids per beam, lengths
    and order equal, scores / length within _nll_bar -- or the first departing selection is one whose smallest float64 margin is below
    twice _nll_bar (two candidates, each an average of log-probabilities within the bar; never above MARGIN_BOUND).  At most 1 image
    of 8 may depart."""
    m, ref, prompts, eos = beam_case
    eng, head = m.engine, m.viecap
    Wd, steps, N = 5, 16, len(prompts)
    refs = [B.beam64(ref, p, Wd, steps, eos) for p in prompts]
    Pmax = max(p.shape[0] for p in prompts)
    embeds = torch.zeros(N, Pmax, 768)
    for n, p in enumerate(prompts):
        embeds[n, :p.shape[0]] = p
    plen = torch.tensor([p.shape[0] for p in prompts], dtype=torch.int32)
    ids, lens, scores = (t.cpu() for t in eng.lm_beam_search(embeds.cuda(), plen.cuda(), Wd, eos, steps=steps))
    batched = [([ids[n, b, :min(int(lens[n, b]), steps)].tolist() for b in range(Wd)], lens[n].tolist(), scores[n].double().tolist()) for n in range(N)]
    monkeypatch.setattr(head, "tokenizer", _IdTokenizer())
    per_image = []
    for p in prompts:
        head.beam_search(p[None].cuda().contiguous(), Wd, max_len=steps, end_of_sentences=(str(eos[0]), str(eos[1])))
        per_image.append(([list(b[0]) for b in head.last_beams], [int(b[1]) for b in head.last_beams], [float(b[2]) for b in head.last_beams]))
    smallest = min(min(min(r) for r in x["margins"]) for x in refs)
    print("float64 search: %d selections, smallest margin %.3e, stopped beams per image %s"
          % (sum(len(x["flat"]) for x in refs) * Wd, smallest, [sum(l < steps for l in x["lens"]) for x in refs]))
    assert sum(sum(l < steps for l in x["lens"]) for x in refs) >= 3, "the eos ids should stop some beams early"
    assert any(len(x["flat"]) < steps for x in refs), "one image should freeze before the last step"
    for name, got in (("pio_lm_beam_search", batched), ("VieCapHead.beam_search", per_image)):
        departed, worst, worst_m = 0, (0.0, 0.0, 1.0), 0.0
        for n, (x, (g_ids, g_lens, g_scores)) in enumerate(zip(refs, got)):
            bar = float(_nll_bar(LAYERS, max(x["amax"])))
            t = _first_departure(g_ids, x["ids"])
            if t is None and g_lens == x["lens"]:
                for b in range(Wd):
                    err = abs(g_scores[b] - x["scores"][b])
                    worst = max(worst, (err / bar, err, bar))
                    assert err <= bar, "%s image %d beam %d: score %.3e from float64, bar %.3e" % (name, n, b, err, bar)
                continue
            assert t is not None and t < len(x["margins"]), (name, n, g_ids, x["ids"], g_lens, x["lens"])
            mg = min(x["margins"][t])
            departed += 1
            worst_m = max(worst_m, mg)
            assert mg <= min(2 * bar, MARGIN_BOUND), "%s image %d departs at selection %d whose smallest float64 margin is %.3e (bar %.3e)" % (
                name, n, t, mg, 2 * bar)
        print("%s: %d of %d images equal to float64; departures at margins <= %.3e" % (name, N - departed, N, worst_m))
        assert departed <= 1, "%s: %d of %d images depart" % (name, departed, N)
        _report("%s scores / length (beam nearest its bar)" % name, worst[1], worst[2])
