"""Float64 statement of the ClipCap head's sampling rule (P/src/clipcap/entrypoint.py:244-276) and of its MLP mapper.

``nucleus(scores, temperature, top_p)``: the reference sorts descending, keeps sorted position 0 and every position whose cumulative
probability BEFORE it is <= top_p (the shifted mask), and renormalises over the kept set.  Ties at the edge: all kept (the kernel's
rule; the reference's unstable sort keeps an arbitrary subset).  ``draw``: the smallest kept id whose kept-mass prefix sum in
ascending id order exceeds u x (kept mass).  ``edge_gap`` / ``cdf_gap`` are the distances the tests' boundary rule reads.
"""
import numpy as np


def softmax64(scores, temperature):
    x = np.asarray(scores, dtype=np.float64) / (temperature if temperature > 0 else 1.0)
    p = np.exp(x - x.max())
    return p / p.sum()


def nucleus(scores, temperature, top_p):
    """-> (kept mask [V] bool, p [V] float64, edge_gap): edge_gap = the smallest |cumulative mass before a sorted position - top_p| over
    the two positions that decide the edge (the last kept group and the first dropped one)."""
    return nucleus_p(scores, softmax64(scores, temperature), top_p)


def nucleus_p(scores, p, top_p):
    """The rule on given probabilities ``p`` of the tokens with ``scores`` (which only order them and define ties); the tokens may be
    the top of a longer row, as long as the kept set ends inside them."""
    p = np.asarray(p, dtype=np.float64)
    x = np.asarray(scores, dtype=np.float64)
    order = np.argsort(-x, kind="stable")
    ps = p[order]
    before = np.concatenate([[0.0], np.cumsum(ps)[:-1]])            # mass strictly before each sorted position
    xs = x[order]
    # ties: a position's "mass above" is the mass before the FIRST member of its tie group
    first = np.concatenate([[True], xs[1:] != xs[:-1]])
    grp_before = np.maximum.accumulate(np.where(first, before, -1.0))
    keep_sorted = grp_before <= top_p
    keep_sorted[0] = True
    keep_sorted |= xs == xs[0]
    kept = np.zeros(p.shape[0], dtype=bool)
    kept[order[keep_sorted]] = True
    cand = grp_before[first]
    edge_gap = float(np.min(np.abs(cand[1:] - top_p))) if cand.shape[0] > 1 else np.inf
    return kept, p, edge_gap


def draw(kept, p, u):
    """-> (token, cdf_gap, neighbours): cdf_gap = min |u - CDF step| relative to the kept mass; neighbours = the kept ids next to token."""
    ids = np.nonzero(kept)[0]
    pk = p[ids]
    Z = pk.sum()
    cdf = np.cumsum(pk) / Z
    j = int(np.searchsorted(cdf, u, side="right"))
    j = min(j, ids.shape[0] - 1)
    gap = float(np.min(np.abs(cdf[max(j - 1, 0):j + 1] - u)))
    nb = {int(ids[k]) for k in (j - 1, j, j + 1) if 0 <= k < ids.shape[0]}
    return int(ids[j]), gap, nb


def mlp_mapper(feats, w1, b1, w2, b2, normalize):
    x = np.asarray(feats, dtype=np.float64)
    if normalize:
        x = x / np.linalg.norm(x, axis=-1, keepdims=True)
    h = np.tanh(x @ np.asarray(w1, np.float64).T + np.asarray(b1, np.float64))
    return h @ np.asarray(w2, np.float64).T + np.asarray(b2, np.float64)
