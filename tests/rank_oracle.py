"""numpy restatement of ``run_catalogue_eval``: the rank of a request's target among the catalogue,

    rank = 1 + #{ candidates c left : c before the target },

where the candidates are the catalogue's items except the one whose id equals the target's and, with ``seen``, except those
whose id the request has seen (the target itself is never dropped), and

    a before b  iff  score_a > score_b,  or  score_a == score_b (IEEE: -0.0 ties with +0.0) and item_a < item_b

-- the order of tests/reco_oracle.py.  The zeros are canonicalised as ``reco_oracle.topk`` does it.  ``metrics`` restates the
dict ``run_catalogue_eval`` returns, from integer ranks in float64."""
import math

import numpy as np


def ranks(scores, ids, target_scores, target_ids, seen=None):
    """``scores`` [N, M] float32, ``ids`` [M] (or [N, M]) int, ``target_scores`` [N] float32, ``target_ids`` [N] int ->
    ``ranks`` [N] int32.  ``seen``: None, or one iterable of ids per request whose members are no candidates."""
    scores = np.asarray(scores, dtype=np.float32)
    N, M = scores.shape
    ids = np.broadcast_to(np.asarray(ids, dtype=np.int64), (N, M))
    ts = np.asarray(target_scores, dtype=np.float32) + np.float32(0.0)         # -0.0 + 0.0 = +0.0
    ti = np.asarray(target_ids, dtype=np.int64)
    out = np.zeros(N, dtype=np.int32)
    for n in range(N):
        s = scores[n] + np.float32(0.0)
        i = ids[n]
        left = i != ti[n]
        if seen is not None:
            left &= ~np.isin(i, np.asarray(list(seen[n]), dtype=np.int64))
        before = (s > ts[n]) | ((s == ts[n]) & (i < ti[n]))
        out[n] = 1 + int(np.count_nonzero(left & before))
    return out


def metrics(ranks, ks, candidates=None):
    """``hit@k``, ``ndcg@k`` for every k of ``ks``, ``mean_mrr``, ``mean_rank``, ``requests`` (and ``candidates`` when given):
    plain python floats summed request by request."""
    r = [int(x) for x in np.asarray(ranks).reshape(-1)]
    N = len(r)
    res = {}
    for k in ks:
        res["hit@%d" % k] = sum(1.0 for x in r if x <= k) / N
        res["ndcg@%d" % k] = sum(1.0 / math.log2(1.0 + x) for x in r if x <= k) / N
    res["mean_mrr"] = sum(1.0 / x for x in r) / N
    res["mean_rank"] = sum(float(x) for x in r) / N
    res["requests"] = N
    if candidates is not None:
        res["candidates"] = int(candidates)
    return res
