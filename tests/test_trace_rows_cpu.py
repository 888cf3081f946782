"""The host row selection of the sparse last ViT block (csrc/trace_rows.h through pio_host_trace_quads), without a GPU: the quads it
lists are exactly those holding a patch whose cell map_traces_to_grid gives a non-zero count, for every case of
golden_cases.trace_cases() -- closed interval ends, points outside [0, 1], the clamp to n - 1, n = 37 where 1 / n is inexact."""
import numpy as np
import pytest

import golden_cases as gc


@pytest.fixture(scope="module")
def lib():
    from patchioner_amd import build
    build.build()
    from patchioner_amd import _lib
    return _lib.load()


def host_quads(lib, traces, n, G):
    """-> (quads, img_off) of pio_host_trace_quads for a batch of traces on an n x n grid with G leading tokens"""
    B = len(traces)
    T = G + n * n
    Tp = (T + 7) // 8 * 8
    xy = np.array([(p["x"], p["y"]) for tr in traces for p in tr], dtype=np.float64).reshape(-1, 2)
    offs = np.zeros(B + 1, dtype=np.int32)
    np.cumsum([len(tr) for tr in traces], out=offs[1:])
    cap = B * Tp // 4
    quads = np.full(cap, -1, dtype=np.int32)
    img_off = np.full(B + 1, -1, dtype=np.int32)
    nq = lib.pio_host_trace_quads(xy.ctypes.data if len(xy) else None, offs.ctypes.data, B, n, G, Tp, quads.ctypes.data, cap,
                                  img_off.ctypes.data)
    assert nq >= 0, lib.pio_last_error()
    assert img_off[0] == 0 and img_off[B] == nq and (quads[nq:] == -1).all()
    return quads[:nq], img_off, Tp


def quads_of_counts(counts, G, Tp):
    """the quads that hold a patch with a non-zero count; counts [B, n * n]"""
    want = []
    for b in range(counts.shape[0]):
        rows = G + np.nonzero(counts[b])[0]
        want += [b * Tp + 4 * q for q in sorted(set((rows // 4).tolist()))]
    return np.array(want, dtype=np.int32)


@pytest.mark.parametrize("G", [5, 1])
def test_host_quads_are_the_nonzero_cells_of_the_reference_grid(lib, G):
    from oracle import patchioner_oracle as O
    cases = gc.trace_cases()
    for n in sorted({n for n, _ in cases}):
        traces = [tr for nn, tr in cases if nn == n]
        quads, img_off, Tp = host_quads(lib, traces, n, G)
        counts = np.stack([O.map_traces_to_grid(tr, n).reshape(-1).numpy() for tr in traces])
        want = quads_of_counts(counts, G, Tp)
        assert np.array_equal(quads, want), (n, G)
        per_img = [len(quads_of_counts(counts[b:b + 1], G, Tp)) for b in range(len(traces))]
        assert np.array_equal(np.diff(img_off), per_img)
        assert (quads % 4 == 0).all() and (np.diff(quads) > 0).all()


def test_a_block_that_straddles_quad_boundaries_takes_both_quads(lib):
    # 5 leading tokens, a 4-patch run from column 5: rows 5 + 16 gy + 5 .. + 8 = 10 .. 13 of row gy = 0 -> quads 8 and 12
    quads, img_off, Tp = host_quads(lib, [[dict(x=(5 + i + 0.5) / 16, y=0.5 / 16) for i in range(4)], []], 16, 5)
    assert Tp == 264 and quads.tolist() == [8, 12] and img_off.tolist() == [0, 2, 2]


def test_bad_arguments_are_refused(lib):
    offs = np.array([0, 1], dtype=np.int32)
    xy = np.array([[0.5, 0.5]], dtype=np.float64)
    q = np.zeros(4, dtype=np.int32)
    io = np.zeros(2, dtype=np.int32)
    assert lib.pio_host_trace_quads(xy.ctypes.data, offs.ctypes.data, 1, 16, 5, 264, q.ctypes.data, 0, io.ctypes.data) < 0      # cap too small
    assert lib.pio_host_trace_quads(xy.ctypes.data, offs.ctypes.data, 1, 16, 5, 261, q.ctypes.data, 4, io.ctypes.data) < 0      # Tp % 8 != 0
    assert lib.pio_host_trace_quads(None, offs.ctypes.data, 1, 16, 5, 264, q.ctypes.data, 4, io.ctypes.data) < 0               # points missing
    assert lib.pio_host_trace_quads(xy.ctypes.data, offs.ctypes.data, 1, 16, 5, 264, q.ctypes.data, 4, io.ctypes.data) == 1
