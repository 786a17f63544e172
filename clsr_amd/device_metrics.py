"""Evaluation metrics computed on the device (csrc/metrics.hip) -- the scores of a whole validation / test file stay
in HBM, no per-batch synchronisation, and a handful of doubles comes back at the end.

Mirrors ``cal_metric`` / ``cal_weighted_metric`` / ``cal_mean_alpha_metric`` of the reference (deeprec_utils.py:621-813)
as ``SequentialBaseModel.run_eval`` / ``run_weighted_eval`` call them (sequential_base_model.py:204-292): same keys,
same 4-decimal rounding, same ``ValueError`` when an AUC is undefined, NaN where the reference divides 0 by 0 (``wmrr`` /
``wndcg@k`` with a user who has no positive line).  Supported: ``auc``, ``logloss``, ``rmse``, ``acc``, ``f1`` (all
lines); ``mean_mrr``, ``ndcg@k``, ``hit@k``, ``group_auc`` (groups of 1 + num_ngs consecutive lines); ``wauc``, ``wmrr``,
``whit@k``, ``wndcg@k`` (per user: any non-negative int32 id, any number of users -- the lines are grouped with the stable
radix sort of csrc/segsum.hip); ``mean_alpha``.  Rank ties break towards the later line of the file, in groups and in
users alike.  What stays on the host (:func:`supported` returns False, the caller keeps clsr_amd/deeprec_utils.py): more
than 8 distinct k over the pairwise or over the weighted metrics, and groups of more than ``MAX_GROUP`` lines.

Sharded over data-parallel ranks (``SequentialBaseModel(shard_eval=True)``): :func:`plan_chunks` spreads the scoring
chunks over the ranks, :meth:`DeviceScores.merge` gives every rank all lines in file order, and
``compute(part=(rank, world), reduce=...)`` has every rank run its share of each metric kernel (the ``clsr_eval_*_part``
entries), sums the raw integer accumulators across the ranks and converts them once: the same bits as one process."""
import ctypes
import math

import torch

from clsr_amd import ops
from clsr_amd.deeprec_utils import _ks

_POINT = {"auc", "logloss", "rmse", "acc", "f1"}
MAX_GROUP = 4096      # clsr_eval_group_metrics: one wave per group, the group's scores and labels in LDS (csrc/metrics.hip)
MAX_K = 8             # distinct k of one kernel launch (GM_MAXK, csrc/metrics.hip)


def _weighted_ks(wm):
    """Sorted distinct k over the whit@ / wndcg@ entries of ``wm``; None when an entry has no device form."""
    ks = set()
    for m in wm:
        if m.startswith("whit") or m.startswith("wndcg"):
            ks.update(_ks(m))
        elif m not in ("wauc", "wmrr"):
            return None
    return sorted(ks)


def supported(hp, n_users, group):
    """``group``: lines per group of the pairwise metrics (1 + num_ngs).  ``n_users`` does not matter any more (the
    user grouping is exact for every id); the argument stays for the callers."""
    if any(m not in _POINT for m in (hp.metrics or [])):
        return False
    ks = set()
    for m in (hp.pairwise_metrics or []):
        if m.startswith("ndcg") or m.startswith("hit"):
            ks.update(_ks(m))
        elif m not in ("mean_mrr", "group_auc"):
            return False
    if len(ks) > MAX_K:
        return False
    if (hp.pairwise_metrics or []) and group > MAX_GROUP:
        return False
    wks = _weighted_ks(getattr(hp, "weighted_metrics", None) or [])
    return wks is not None and len(wks) <= MAX_K and all(k > 0 for k in wks)


def chunk_owner(loads):
    """The rank that scores the next chunk, given the lines every rank has been handed so far: the one with the
    fewest, the lowest rank on a tie.  The ranks iterate the same file, so they agree without talking."""
    return min(range(len(loads)), key=lambda r: (loads[r], r))


def plan_chunks(sizes, world):
    """[(offset, size, owner)] for scoring chunks of ``sizes`` lines in file order: offsets are the chunks' global line
    offsets, every chunk has one owner (:func:`chunk_owner`, applied chunk by chunk as the evaluation loop does)."""
    loads, off, plan = [0] * world, 0, []
    for n in sizes:
        r = chunk_owner(loads)
        plan.append((off, n, r))
        loads[r] += n
        off += n
    return plan


class DeviceScores(object):
    """Growing device buffers of (pred, label, user[, alpha]) per scored line; appends are stream-ordered copies.  The
    alpha column (the long / short fusion weight, for ``mean_alpha``) is allocated only when the batches carry one."""

    def __init__(self, device):
        self.device, self.n, self.cap = device, 0, 0
        self.pred = self.labels = self.users = self.alpha = None

    @property
    def has_alpha(self):
        return self.alpha is not None

    def _grow(self, need, with_alpha):
        cap = max(need, 2 * self.cap, 1 << 16)
        new = [torch.empty(cap, dtype=torch.float32, device=self.device),
               torch.empty(cap, dtype=torch.float32, device=self.device),
               torch.empty(cap, dtype=torch.int32, device=self.device),
               torch.empty(cap, dtype=torch.float32, device=self.device) if with_alpha else None]
        if self.n:
            for dst, src in zip(new, (self.pred, self.labels, self.users, self.alpha)):
                if dst is not None:
                    dst[: self.n].copy_(src[: self.n])
        self.pred, self.labels, self.users, self.alpha = new
        self.cap = cap

    def append(self, pred, labels, users, alpha=None):
        b = pred.numel()
        if self.n and (alpha is not None) != self.has_alpha:
            raise ValueError("either every appended batch carries an alpha column or none does")
        if self.n + b > self.cap or (alpha is not None and self.alpha is None):
            self._grow(self.n + b, alpha is not None)
        self.pred[self.n:self.n + b].copy_(pred.reshape(-1))
        self.labels[self.n:self.n + b].copy_(labels.reshape(-1))
        if users is not None:
            self.users[self.n:self.n + b].copy_(users.reshape(-1))
        if alpha is not None:
            self.alpha[self.n:self.n + b].copy_(alpha.reshape(-1))
        self.n += b

    def append_zeros(self, b, with_alpha=False):
        """``b`` lines that another rank scores: all-zero bits in every column, filled in by :meth:`merge`."""
        if self.n and with_alpha != self.has_alpha:
            raise ValueError("either every appended batch carries an alpha column or none does")
        if self.n + b > self.cap or (with_alpha and self.alpha is None):
            self._grow(self.n + b, with_alpha)
        for col in (self.pred, self.labels, self.users, self.alpha):
            if col is not None:
                col[self.n:self.n + b].zero_()
        self.n += b

    def merge(self, reduce):
        """Every line was appended by ONE rank and as zeros (:meth:`append_zeros`) by the others: ``reduce`` (sums a list
        of integer device tensors across the ranks, in place) leaves all lines on every rank.  The columns travel as
        int32 bit patterns in one buffer: a pattern plus zeros is that pattern, whatever float it encodes."""
        cols = [c[:self.n] for c in (self.pred, self.labels, self.users, self.alpha) if c is not None]
        packed = torch.cat([c.view(torch.int32) for c in cols])
        reduce([packed])
        for i, c in enumerate(cols):
            c.view(torch.int32).copy_(packed[i * self.n:(i + 1) * self.n])


# the partial forms' accumulators in ONE int64 buffer (one small collective): the slots of outd | outw | outu | err below
_ACC_D, _ACC_W, _ACC_U, _ACC_E, _ACC_SLOTS = 0, 24, 42, 50, 53
_FX_LOGLOSS, _FX_GROUP, _FX_USER, _FX_POINT = 0, 1, 2, 3      # CLSR_EVAL_FX_* (include/clsr_hip.h)


def compute(scores, hp, group, weighted, raw=None, n_users=None, mean_alpha=False, part=None, reduce=None):
    """-> dict of metrics (the union of what cal_metric(metrics), cal_metric(pairwise_metrics), when ``weighted``
    cal_weighted_metric(weighted_metrics) and, when ``mean_alpha``, cal_mean_alpha_metric return).  Synchronises once.
    ``n_users``: None for any non-negative int32 id; otherwise a STRICT upper bound of every user id (the size of the
    user vocabulary) -- a precondition: the sort then looks at the low ``ceil(log2(n_users))`` bits only, and an id at
    or above the bound would silently be grouped with another user.  ``raw`` (a dict) receives the unrounded values (tests: a mean that sits exactly on a
    4-decimal rounding boundary may round either way); for ``rmse`` -- the root of the ROUNDED mean squared error, as in
    the reference -- it receives the unrounded root and the mean squared error itself as ``mse``.
    ``part=(rank, world)``: ``scores`` holds ALL lines on every rank (:meth:`DeviceScores.merge`); this rank runs share
    ``rank`` of ``world`` of every metric kernel into raw integer accumulators, ``reduce([acc])`` (a callable that sums
    int64 device tensors across the ranks in place; may be None for a world of one) is called once, and the sums are
    converted once -- the dict, ``raw`` included, is the one ``part=None`` gives, to the bit, on every rank."""
    N, dev = scores.n, scores.device
    if N == 0 or N % group:
        raise ValueError("%d scored lines do not divide into groups of %d" % (N, group))
    if mean_alpha and not scores.has_alpha:
        raise ValueError("mean_alpha needs scores appended with an alpha column")
    pred, labels = scores.pred[:N], scores.labels[:N]
    if part is None:
        outd = torch.zeros(24, dtype=torch.float64, device=dev)  # [0] logloss | [1..] group metrics | [20..22] point sums
        outw = torch.zeros(18, dtype=torch.float64, device=dev)  # wauc, wmrr, 8 x wndcg@k, 8 x whit@k
        outu = torch.zeros(8, dtype=torch.int64, device=dev)     # [0..2] auc pair counts | [4..7] acc, TP, FP, FN
        err = torch.zeros(3, dtype=torch.int32, device=dev)      # groups | one-class users | users without a positive
        sfx, share = "", ()
    else:
        rank, world = part
        if not 0 <= rank < world or (world > 1 and reduce is None):
            raise ValueError("part=(rank, world) with 0 <= rank < world, and a reduce for more than one rank")
        acc = torch.zeros(_ACC_SLOTS, dtype=torch.int64, device=dev)      # the same slots, raw (err: 64-bit counters)
        outd, outw, outu, err = acc[_ACC_D:_ACC_W], acc[_ACC_W:_ACC_U], acc[_ACC_U:_ACC_E], acc[_ACC_E:]
        sfx, share = "_part", (rank, world)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)           # positives of the file (every part counts them all)
    metrics = list(hp.metrics or [])
    point = mean_alpha or any(m in ("rmse", "acc", "f1") for m in metrics)
    if "logloss" in metrics:
        ops.call("clsr_eval_logloss" + sfx, pred, labels, N, *share, outd)
    if "auc" in metrics:
        pos = torch.empty(N, dtype=torch.float32, device=dev)
        ops.call("clsr_eval_compact_pos", pred, labels, N, pos, cnt)
        ops.call("clsr_eval_auc_pairs" + sfx, pred, labels, N, pos, cnt, *share, outu)
    if point:
        ops.call("clsr_eval_point_stats" + sfx, pred, labels, scores.alpha[:N] if mean_alpha else None, N, *share,
                 outd[20:], outu[4:])
    pair = list(hp.pairwise_metrics or [])
    ks = sorted({k for m in pair if m.startswith("ndcg") or m.startswith("hit") for k in _ks(m)})
    if pair:
        karr = (ctypes.c_int * max(len(ks), 1))(*ks)
        ops.call("clsr_eval_group_metrics" + sfx, pred, labels, N // group, group, ctypes.addressof(karr), len(ks),
                 1 if "group_auc" in pair else 0, *share, outd[1:], err)
    wm = list(getattr(hp, "weighted_metrics", None) or []) if weighted else []
    wks = _weighted_ks(wm)
    if wks is None or len(wks) > MAX_K:
        raise ValueError("no device form for the weighted metrics %r (see supported())" % (wm,))
    if wm:
        # lines grouped by user: keys ascending, equal keys in line order; then the list of segment starts, whose length
        # (the number of distinct users) stays on the device
        bits = 31 if n_users is None else min(31, max(1, (int(n_users) - 1).bit_length()))
        keys = torch.empty(N, dtype=torch.int32, device=dev)
        perm = torch.empty(N, dtype=torch.int32, device=dev)
        ws = torch.empty(ops.query("clsr_sort_ids_stable_workspace_bytes", N, 1), dtype=torch.uint8, device=dev)
        ops.sort_ids_stable_multi([ops.SortIdsDesc.row(ids=scores.users[:N], keys_out=keys, perm_out=perm, nrows=N, row_stride=1,
                                                       ncols=1, bits=bits)], ws)
        starts = torch.empty(N, dtype=torch.int32, device=dev)
        nseg = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.call("clsr_eval_user_segments", keys, N, starts, nseg)
        wkarr = (ctypes.c_int * max(len(wks), 1))(*wks)
        ops.call("clsr_eval_user_metrics" + sfx, pred, labels, perm, keys, starts, nseg, N, ctypes.addressof(wkarr),
                 len(wks), 1 if "wauc" in wm else 0, 1 if any(m != "wauc" for m in wm) else 0, *share, outw, err[1:])
    if part is None:
        d, w, u, c, e = (outd.cpu().tolist(), outw.cpu().tolist(), outu.cpu().tolist(), int(cnt.cpu()),
                         err.cpu().tolist())                      # the one sync
    else:
        if reduce is not None:
            reduce([acc])                                         # integer sums: the whole kernels' bits on every rank
        if "logloss" in metrics:
            ops.call("clsr_eval_finalize", outd, 1, _FX_LOGLOSS)
        if pair:
            ops.call("clsr_eval_finalize", outd[1:], 2 + 2 * len(ks), _FX_GROUP)
        if point:
            ops.call("clsr_eval_finalize", outd[20:], 3, _FX_POINT)
        if wm:
            ops.call("clsr_eval_finalize", outw, 18, _FX_USER)
        host, c = acc.cpu(), int(cnt.cpu())                       # the one sync
        d, w = host[_ACC_D:_ACC_W].view(torch.float64).tolist(), host[_ACC_W:_ACC_U].view(torch.float64).tolist()
        u, e = host[_ACC_U:_ACC_E].tolist(), host[_ACC_E:].tolist()
    res, final = {}, {}
    for m in metrics:
        if m == "auc":
            if c == 0 or u[2] == 0:
                raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
            res["auc"] = (u[0] + 0.5 * u[1]) / (float(c) * float(u[2]))
        elif m == "logloss":
            res["logloss"] = d[0] / N
        elif m == "rmse":
            mse = d[20] / N
            final["rmse"] = math.sqrt(round(mse, 4))
            if raw is not None:
                raw.update(rmse=math.sqrt(mse), mse=mse)
        elif m == "acc":
            res["acc"] = u[4] / float(N)
        elif m == "f1":
            den = 2.0 * u[5] + u[6] + u[7]
            res["f1"] = u[5] * 2.0 / den if den > 0 else 0.0
    ng = N // group
    if pair and e[0]:
        raise ValueError("%d groups without a positive (or, for group_auc, without a negative) line" % e[0])
    for m in pair:
        if m == "mean_mrr":
            res["mean_mrr"] = d[1] / ng
        elif m == "group_auc":
            res["group_auc"] = d[2] / ng
        elif m.startswith("ndcg"):
            for k in _ks(m):
                res["ndcg@{0}".format(k)] = d[3 + ks.index(k)] / ng
        elif m.startswith("hit"):
            for k in _ks(m):
                res["hit@{0}".format(k)] = d[3 + len(ks) + ks.index(k)] / ng
    nan = float("nan") if e[2] else None       # a user without a positive line: the reference's mrr / ndcg are 0 / 0 there
    for m in wm:
        if m == "wauc":
            if e[1]:
                raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
            res["wauc"] = w[0]
        elif m == "wmrr":
            res["wmrr"] = w[1] if nan is None else nan
        elif m.startswith("wndcg"):
            for k in _ks(m):
                res["wndcg@{0}".format(k)] = w[2 + wks.index(k)] if nan is None else nan
        elif m.startswith("whit"):
            for k in _ks(m):
                res["whit@{0}".format(k)] = w[2 + MAX_K + wks.index(k)]
    if mean_alpha:
        res["mean_alpha"] = d[21] / d[22] if d[22] else float("nan")
    if raw is not None:
        raw.update(res)
    final.update((k, round(v, 4)) for k, v in res.items())
    return final
