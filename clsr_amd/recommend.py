"""``recommend_k_items``: the K best catalogue items of every request, selected on the device.

A request is a kept line of a data file (its user, history and time features); the catalogue is scored against a batch of
``n`` requests in chunks of ``g`` candidates through the scoring pass that exists -- ``net.forward`` on a compact scoring
feed (``hist_group = g``: history-level tensors one row per request, ``items`` / ``cates`` one per row).  The feed's
history-level tensors are uploaded once per request batch; per chunk there are three steps on the model's stream,

    clsr_reco_fill_candidates   the chunk's ids into the feed's items / cates (id 0 past the catalogue's end),
    net.forward(f, False)       the logits, from the recorded launch plan of the feed,
    clsr_reco_topk_merge        the chunk's valid columns into the running list of every request (csrc/reco.hip),

and one synchronisation per request batch fetches the lists.  No score crosses PCIe and no [requests, catalogue] matrix
exists.  The encoders run again for every chunk, also for the kinds whose user state does not depend on the target.

``run_catalogue_eval`` (``rank_targets``) runs the same loop to say where a request's true next item lands in that order: the
feed's group is the target in column 0 plus the chunk's candidates, ``clsr_reco_fill_ranked`` and ``clsr_reco_rank_count``
take the places of fill and merge, and the rank is one plus a sum of counts -- nothing is sorted.
"""
import collections

import numpy as np
import torch

from clsr_amd import _lib, ops

__all__ = ["Recommendations", "CatalogueRanks", "ROW_BUDGET", "plan", "plan_ranked", "merge_catalogue", "count_catalogue",
           "recommend", "rank_targets", "rank_metrics", "write_tsv"]

Recommendations = collections.namedtuple("Recommendations", "users items scores")
CatalogueRanks = collections.namedtuple("CatalogueRanks", "users items scores ranks")

#: rows (requests x candidates) of one scoring pass: the size ``run_eval`` gathers its chunks to by default -- the
#: row-level buffers of the attention kinds (T x 80 floats a row) stay at half a gigabyte at T = 50
ROW_BUDGET = 32768


def plan(n_requests, n_candidates, max_chunk, row_budget=ROW_BUDGET, chunk=None):
    """``(n, g)``: requests per batch and candidates per chunk.  The encoders run per request and the logit MLP per row, so
    a pass over few requests and many candidates is the cheap one: ``g`` first -- as large as ``max_chunk`` and the row
    budget allow, evened out over the chunks so that the ragged last one is nearly full -- then ``n`` from what the budget
    leaves.  ``chunk`` pins ``g`` (refused by name outside ``1 .. max_chunk``).  Always ``n g <= max(row_budget, g)``."""
    N, M, cap, budget = int(n_requests), int(n_candidates), int(max_chunk), int(row_budget)
    if N < 1 or M < 1 or cap < 1 or budget < 1:
        raise ValueError("plan: requests, candidates, max_chunk and row_budget must be positive, got %r"
                         % ((N, M, cap, budget),))
    if chunk is None:
        top = min(M, cap, budget)
        g = -(-M // (-(-M // top)))
    else:
        g = int(chunk)
        if not 1 <= g <= cap:
            raise ValueError("chunk must lie in 1 .. %d (clsr_reco_max_chunk()), got %r" % (cap, chunk))
    return max(1, min(N, budget // g)), g


def _request_feed(cols, sel, g):
    """The compact scoring feed of the lines ``sel`` against ``g`` candidates a request (ids filled on the device)."""
    n = len(sel)
    feed = {k: cols[k][sel] for k in ("item_history", "item_cate_history", "mask", "time_from_first_action", "time_to_now")}
    feed["users"] = cols["users"][sel].astype(np.float32)      # (as ``predict`` feeds them: through float32)
    feed["items"] = feed["cates"] = np.zeros(n * g, dtype=np.int32)
    feed["labels"] = np.zeros(n * g, dtype=np.float32)
    feed["hist_group"] = g
    return feed


def merge_catalogue(net, f, cand_items, cand_cates, M, g, K, remove_seen, best_s, best_i):
    """The chunk loop of one request batch on the current stream: ``f`` is the batch's uploaded compact scoring feed of
    ``g`` candidates a request, ``cand_items`` / ``cand_cates`` the catalogue's ``M`` device ids; chunks in ascending order,
    each fill -> ``net.forward(f, False)`` -> merge into ``best_s`` / ``best_i`` ``[requests, K]``.  Nothing synchronises."""
    nb, T = f["B"] // g, f["T"]
    stride = T if f["compact"] else g * T      # (no shared histories -- g = 1, dedup_histories=False: a history row per row)
    for c0 in range(0, M, g):
        ops.call("clsr_reco_fill_candidates", cand_items, cand_cates, M, c0, g, nb, f["items"], f["cates"])
        logit = net.forward(f, False)["logit"]
        ops.call("clsr_reco_topk_merge", logit, f["items"], nb, g, min(g, M - c0), f["item_history"], stride, T,
                 int(bool(remove_seen)), K, best_s, best_i, int(c0 == 0))


def recommend(model, infile, catalogue, top_k=10, remove_seen=True, chunk=None):
    """See ``SequentialBaseModel.recommend_k_items``."""
    net, it = model.net, model.iterator
    kmax, gmax = ops.query("clsr_reco_max_k"), ops.query("clsr_reco_max_chunk")
    if not isinstance(top_k, (int, np.integer)) or not 1 <= int(top_k) <= kmax:
        raise ValueError("top_k must be an integer in 1 .. %d, got %r" % (kmax, top_k))
    K = int(top_k)
    catalogue.check_vocabulary(net.dims["Vi"], net.dims["Vc"])
    cols, keep = it.eval_lines(infile)
    N, M, T = len(keep), len(catalogue), int(cols["item_history"].shape[1])
    users = torch.from_numpy(np.ascontiguousarray(cols["users"][keep], dtype=np.int32))
    if N == 0:
        return Recommendations(users, torch.empty(0, K, dtype=torch.int32), torch.empty(0, K, dtype=torch.float32))
    n, g = plan(N, M, gmax, chunk=chunk)
    if not ops.query("clsr_reco_topk_supported", n, g, T, K):
        raise ValueError("recommend_k_items: %d requests x chunk = %d candidates, histories of %d steps, top_k = %d is not a "
                         "shape clsr_reco_topk_merge takes" % (n, g, T, K))
    items, scores = [], []
    with model._stream_ctx():
        cand_items, cand_cates = catalogue.device(net.device)
        for a in range(0, N, n):
            sel = keep[a:a + n]
            nb = len(sel)
            key = ("recommend", nb, T, g)
            f = model._static[key] = net.upload(_request_feed(cols, sel, g), False, into=model._static.get(key))
            best_s = torch.empty(nb, K, dtype=torch.float32, device=net.device)
            best_i = torch.empty(nb, K, dtype=torch.int32, device=net.device)
            try:
                merge_catalogue(net, f, cand_items, cand_cates, M, g, K, remove_seen, best_s, best_i)
            except _lib.ClsrLibraryError as e:
                if "unsupported shape" not in str(e):
                    raise
                raise ValueError("chunk = %d: the scoring pass of %s does not take %d requests in groups of %d (%s)"
                                 % (g, type(model).__name__, nb, g, e))
            items.append(best_i.cpu())      # the one synchronisation of the request batch
            scores.append(best_s.cpu())
    return Recommendations(users, torch.cat(items), torch.cat(scores))


def plan_ranked(n_requests, n_candidates, max_group, row_budget=ROW_BUDGET, chunk=None):
    """``(n, c)`` for ``rank_targets``: requests per batch and CANDIDATES per chunk; the feed's group is ``c + 1`` (the target
    rides in column 0).  ``c`` as ``plan`` chooses it with ``max_group - 1`` as the largest chunk -- the group stays within
    ``max_group`` -- and ``chunk`` pins it (refused by name outside ``1 .. max_group - 1``); then ``n`` from what the budget
    leaves for groups of ``c + 1``.  Always ``n (c + 1) <= max(row_budget, c + 1)``."""
    cap = int(max_group) - 1
    if chunk is not None and not 1 <= int(chunk) <= cap:
        raise ValueError("chunk must lie in 1 .. %d (clsr_reco_max_chunk() - 1: the target takes one row of the group), got %r"
                         % (cap, chunk))
    _, c = plan(n_requests, n_candidates, cap, row_budget, chunk)
    return max(1, min(int(n_requests), int(row_budget) // (c + 1))), c


def count_catalogue(net, f, cand_items, cand_cates, M, g, target_items, target_cates, remove_seen, partial, target_score):
    """The chunk loop of one request batch of ``rank_targets`` on the current stream: ``f`` is the batch's uploaded compact
    scoring feed of groups of ``g`` = 1 target + ``g - 1`` candidates; per chunk fill -> ``net.forward(f, False)`` -> count into
    ``partial`` ``[requests, slabs]`` (the first chunk overwrites it and writes ``target_score``).  Nothing synchronises."""
    nb, T = f["B"] // g, f["T"]
    stride = T if f["compact"] else g * T
    for c0 in range(0, M, g - 1):
        ops.call("clsr_reco_fill_ranked", cand_items, cand_cates, M, c0, g, target_items, target_cates, nb, f["items"], f["cates"])
        logit = net.forward(f, False)["logit"]
        ops.call("clsr_reco_rank_count", logit, f["items"], nb, g, min(g - 1, M - c0), f["item_history"], stride, T,
                 int(bool(remove_seen)), partial, target_score, int(c0 == 0))


def rank_targets(model, infile, catalogue, remove_seen=True, chunk=None):
    """See ``SequentialBaseModel.run_catalogue_eval``: ``CatalogueRanks(users, items, scores, ranks)`` of the positive lines of
    ``infile``, CPU tensors."""
    net, it = model.net, model.iterator
    catalogue.check_vocabulary(net.dims["Vi"], net.dims["Vc"])
    cols, keep = it.eval_lines(infile)
    keep = keep[cols["labels"][keep] == 1]
    N, M, T = len(keep), len(catalogue), int(cols["item_history"].shape[1])
    if N == 0:
        raise ValueError("infile %r holds no kept line with label 1: there is no target to rank" % (infile,))
    n, c = plan_ranked(N, M, ops.query("clsr_reco_max_chunk"), chunk=chunk)
    g = c + 1
    if not ops.query("clsr_reco_rank_supported", n, g, T):
        raise ValueError("run_catalogue_eval: %d requests x (1 + chunk = %d candidates), histories of %d steps is not a shape "
                         "clsr_reco_rank_count takes" % (n, c, T))
    slabs = -(-c // ops.query("clsr_reco_rank_slab"))
    users = torch.from_numpy(np.ascontiguousarray(cols["users"][keep], dtype=np.int32))
    items = torch.from_numpy(np.ascontiguousarray(cols["items"][keep], dtype=np.int32))
    cates = torch.from_numpy(np.ascontiguousarray(cols["cates"][keep], dtype=np.int32))
    scores, ranks = [], []
    with model._stream_ctx():
        cand_items, cand_cates = catalogue.device(net.device)
        items_d, cates_d = items.to(net.device), cates.to(net.device)
        for a in range(0, N, n):
            sel = keep[a:a + n]
            nb = len(sel)
            key = ("recommend", nb, T, g)
            f = model._static[key] = net.upload(_request_feed(cols, sel, g), False, into=model._static.get(key))
            t_items, t_cates = items_d[a:a + nb], cates_d[a:a + nb]
            partial = torch.empty(nb, slabs, dtype=torch.int32, device=net.device)
            t_score = torch.empty(nb, dtype=torch.float32, device=net.device)
            try:
                count_catalogue(net, f, cand_items, cand_cates, M, g, t_items, t_cates, remove_seen, partial, t_score)
            except _lib.ClsrLibraryError as e:
                if "unsupported shape" not in str(e):
                    raise
                raise ValueError("chunk = %d: the scoring pass of %s does not take %d requests in groups of %d (%s)"
                                 % (c, type(model).__name__, nb, g, e))
            rank = partial.sum(1, dtype=torch.int32) + 1
            ranks.append(rank.cpu())        # the one synchronisation of the request batch
            scores.append(t_score.cpu())
    return CatalogueRanks(users, items, torch.cat(scores), torch.cat(ranks))


def rank_metrics(ranks, ks, n_candidates):
    """The dict of ``run_catalogue_eval`` from integer ranks, in float64 on the host, unrounded."""
    r = np.asarray(ranks, dtype=np.float64)
    res = {}
    for k in ks:
        hit = r <= k
        res["hit@%d" % k] = float(hit.mean())
        res["ndcg@%d" % k] = float(np.where(hit, 1.0 / np.log2(1.0 + r), 0.0).mean())
    res["mean_mrr"] = float((1.0 / r).mean())
    res["mean_rank"] = float(r.mean())
    res["requests"] = int(r.shape[0])
    res["candidates"] = int(n_candidates)
    return res


def write_tsv(outfile, reco, userdict, itemdict):
    """``user \\t item \\t rank \\t score`` per filled slot: raw strings through the inverse vocabularies, ranks from 1, the
    score as ``repr`` of the float32 logit (it parses back to the same bits).  An id outside a vocabulary (0: a token the
    vocabulary did not hold) is written as its number."""
    inv_u = {v: k for k, v in userdict.items()}
    inv_i = {v: k for k, v in itemdict.items()}
    users, items, scores = reco.users.numpy(), reco.items.numpy(), reco.scores.numpy()
    with open(outfile, "w") as wt:
        for r in range(items.shape[0]):
            u = inv_u.get(int(users[r]), str(int(users[r])))
            for k in range(items.shape[1]):
                if items[r, k] < 0:
                    break       # (the list is sorted: empty slots are its tail)
                wt.write("%s\t%s\t%d\t%s\n" % (u, inv_i.get(int(items[r, k]), str(int(items[r, k]))), k + 1, repr(float(scores[r, k]))))
