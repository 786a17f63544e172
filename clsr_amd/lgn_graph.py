"""The user-item graph of LGN (models/sequential/lgn.py: get_R, creat_item2cate, create_adj_mat_ui), as CSR arrays.

``build_graph`` reads ``dirname(user_vocab)/train_data`` and the three vocabularies and returns

  A_hat = D^-1 (A + I)   over the bipartite graph, [Vu + Vi] square: row-normalised (not symmetric), every row holds its
                         diagonal entry, float32 values cast from the float64 quotient (as the reference casts its matrix),
  its transpose          (the backward pass gathers over it: never a scatter),
  item2cate [Vi]         item2cate[0] = 0, items the events never name -> category 0.

Which lines count is the reference's: only a line whose user differs from the previous line's, and the last line of the
file.  At a change the PREVIOUS line's history (and target, for item2cate) is attributed to the NEW line's user
(lgn.py:187-191) -- kept, since the reference's checkpoints were trained on that graph; tests/golden/lgn_graph.npz pins it.
Nothing is written beside the data: the reference's .npz / item2cate caches are not reproduced.

numpy only.  Token parsing is per selected line; everything over edges and entries is vectorised.
"""
import collections
import os

import numpy as np

from clsr_amd.deeprec_utils import load_dict

Graph = collections.namedtuple("Graph", "n_users n_items indptr indices values t_indptr t_indices t_values item2cate")


def _events(train_file):
    """[(line whose user the event is attributed to, line whose history / target it takes)] in file order."""
    with open(train_file) as f:
        lines = [ln.rstrip("\n").strip().split("\t") for ln in f.read().split("\n") if ln]
    users = np.asarray([u[1] for u in lines])
    n = len(lines)
    change = 1 + np.flatnonzero(users[1:] != users[:-1])
    ev = [(int(i), int(i) - 1) for i in change]
    if n:
        ev.append((n - 1, n - 1))       # (a change on the last line comes first, as in the reference's loop body)
    return lines, ev


def _ids(vocab, tokens, what):
    try:
        return [vocab[t] for t in tokens]
    except KeyError as e:
        raise ValueError("train_data names %s %s, which the vocabulary does not hold" % (what, e))


def csr_transpose(indptr, indices, values, ncols):
    """CSR of the transpose; indices ascend in every row when they do in the input."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices)
    rows = np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))
    order = np.argsort(indices, kind="stable")
    t_indptr = np.zeros(ncols + 1, dtype=np.int64)
    np.cumsum(np.bincount(indices, minlength=ncols), out=t_indptr[1:])
    return t_indptr, rows[order].astype(np.int32), np.asarray(values)[order]


def normalised_adjacency(n_users, n_items, edge_users, edge_items):
    """CSR of D^-1 (A + I) for the bipartite edges (user u, item i), duplicates merged."""
    Vu, Vi = int(n_users), int(n_items)
    N = Vu + Vi
    if N >= 2 ** 31:
        raise ValueError("user + item vocabulary (%d rows) must fit int32" % N)
    key = np.unique(np.asarray(edge_users, dtype=np.int64) * Vi + np.asarray(edge_items, dtype=np.int64))
    u, i = key // Vi, key % Vi + Vu
    diag = np.arange(N, dtype=np.int64)
    rows, cols = np.concatenate([u, i, diag]), np.concatenate([i, u, diag])
    if len(rows) >= 2 ** 31:
        raise ValueError("adjacency entries (%d) must fit int32" % len(rows))
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    count = np.bincount(rows, minlength=N)
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(count, out=indptr[1:])
    # rowsum of A + I = entries of the row; the reference divides in float64 and casts the matrix to float32
    values = (1.0 / count.astype(np.float64))[rows].astype(np.float32)
    return indptr, cols.astype(np.int32), values


def build_graph(hparams):
    """``Graph`` for the data set ``hparams.user_vocab`` lies in (``hparams``: anything with the three vocabulary paths)."""
    userdict, itemdict, catedict = (load_dict(getattr(hparams, k)) for k in ("user_vocab", "item_vocab", "cate_vocab"))
    Vu, Vi = len(userdict), len(itemdict)
    lines, events = _events(os.path.join(os.path.dirname(hparams.user_vocab), "train_data"))
    eu, ei, pi, pc = [], [], [], []
    for to, src in events:
        uid = _ids(userdict, [lines[to][1]], "user")[0]
        hist = _ids(itemdict, lines[src][5].split(","), "item")
        eu.append(np.full(len(hist), uid, dtype=np.int64))
        ei.append(np.asarray(hist, dtype=np.int64))
        # creat_item2cate's order of assignment: the target, then the history pairs (zip: the shorter list ends it)
        cates = _ids(catedict, lines[src][6].split(","), "category")
        m = min(len(hist), len(cates))
        pi.append(np.asarray(_ids(itemdict, [lines[src][2]], "item") + hist[:m], dtype=np.int64))
        pc.append(np.asarray(_ids(catedict, [lines[src][3]], "category") + cates[:m], dtype=np.int64))
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, dtype=np.int64)
    indptr, indices, values = normalised_adjacency(Vu, Vi, cat(eu), cat(ei))
    t_indptr, t_indices, t_values = csr_transpose(indptr, indices, values, Vu + Vi)
    # a later assignment to an item wins: the first occurrence in the reversed list
    pi, pc = cat(pi)[::-1], cat(pc)[::-1]
    item2cate = np.zeros(Vi, dtype=np.int32)
    items, first = np.unique(pi, return_index=True)
    item2cate[items] = pc[first]
    item2cate[0] = 0
    return Graph(Vu, Vi, indptr, indices, values, t_indptr, t_indices, t_values, item2cate)


def split_plan(indptr, chunk):
    """Rows longer than ``chunk`` entries (clsr_lgn_row_chunk()), for the kernels' split path: ``long_rows`` ascending
    (int32) and ``long_off`` (int32, one more): row long_rows[q] owns the chunks long_off[q] .. long_off[q + 1], chunk c of
    a row covering its entries c * chunk .. min((c + 1) * chunk, degree)."""
    deg = np.diff(np.asarray(indptr, dtype=np.int64))
    rows = np.flatnonzero(deg > chunk)
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum((deg[rows] + chunk - 1) // chunk, out=off[1:])
    return rows.astype(np.int32), off.astype(np.int32)
