"""numpy restatement of ``recommend_k_items``' selection: the K best candidates of every request in the strict total order

    a before b  iff  score_a > score_b,  or  score_a == score_b (IEEE: -0.0 ties with +0.0) and item_a < item_b,

seen candidates masked out first, the tail padded with (-inf, -1).  A score of -0.0 is returned as +0.0, as the kernel returns
it (csrc/reco.hip keeps one canonical zero in its keys)."""
import numpy as np


def topk(scores, ids, K, seen=None):
    """``scores`` [N, M] float32 and ``ids`` [M] (or [N, M]) int -> ``(items [N, K] int32, scores [N, K] float32)``.
    ``seen``: None, or one iterable of ids per request whose members are never returned."""
    scores = np.asarray(scores, dtype=np.float32)
    N, M = scores.shape
    ids = np.broadcast_to(np.asarray(ids, dtype=np.int64), (N, M))
    out_i = np.full((N, K), -1, dtype=np.int32)
    out_s = np.full((N, K), -np.inf, dtype=np.float32)
    for n in range(N):
        s = scores[n] + np.float32(0.0)         # -0.0 + 0.0 = +0.0
        i = ids[n]
        if seen is not None:
            ok = ~np.isin(i, np.asarray(list(seen[n]), dtype=np.int64))
            s, i = s[ok], i[ok]
        order = np.lexsort((i, -s))[:K]
        out_i[n, :len(order)] = i[order]
        out_s[n, :len(order)] = s[order]
    return out_i, out_s


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
