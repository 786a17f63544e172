"""Device image of an iterator's per-file column store, and the recipe checks of the resident feed path.

``SequentialIterator`` pads every line of a file once (``_columns``); a training batch is then a row gather driven by
``sel`` (the file lines drawn) and ``src`` (the in-batch line every output row takes its item / category from).  With
``resident_data=True`` a model keeps the columns the step reads in HBM -- ``item_history``, ``item_cate_history``,
``time_from_first_action``, ``time_to_now`` ``[N, T]`` and ``lens``, ``users``, ``items``, ``cates`` ``[N]``, 4-byte words all:
``N * (16 T + 16)`` bytes -- and ``clsr_feed_build`` (csrc/feed.hip) gathers the batch there; only ``sel`` and ``src`` cross
PCIe.  ``NextItNetColumnIterator`` keeps the same columns left-padded; its recipe is ``(sel, psrc)``
(:func:`check_position_recipe`) and ``clsr_feed_build_pos`` builds its batches.  The image is uploaded once per cached file
and again when the iterator re-parses the file (its column dict is a new object then).  A failed allocation surfaces as
torch raises it.

``resident_eval=True`` is a separate switch with a store of its own (:class:`ResidentEvalStore`): per evaluated file the
same columns plus ``labels``, ``N * (16 T + 20)`` bytes, and per ``min_seq_length`` the list ``keep`` of the lines a pass
yields (``4 n_keep`` bytes).  ``clsr_feed_same_rows`` marks the lines that repeat their predecessor's history once per
``keep``; :func:`eval_chunk_plan` turns the marks into the chunks ``_device_eval`` scores, and ``clsr_feed_build_eval``
builds each chunk's feed from ``(k0, n, g)``.  A file that is trained on and evaluated under both switches has two images.
"""
import numpy as np
import torch

__all__ = ["ResidentColumns", "ResidentStore", "check_recipe", "check_position_recipe", "COLUMNS", "ResidentEvalColumns",
           "ResidentEvalStore", "EvalLines", "same_rows", "eval_chunk_plan"]

_BIG = (("item_history", np.int32), ("item_cate_history", np.int32), ("time_from_first_action", np.float32),
        ("time_to_now", np.float32))
_SMALL = ("lens", "users", "items", "cates")
COLUMNS = tuple(k for k, _ in _BIG) + _SMALL


def _check(sel, name, src, N, rank, tail, G, T=None):
    """The body the two recipe checks share: ``sel`` int32 ``[n]`` in ``[0, N)`` and the ``rank``-d second array ``name``,
    int32 ``[n] + tail`` in ``[0, n)`` (``tail`` None: no batch has this shape; ``G``, ``T``: the groups as the message
    names them), both contiguous."""
    for nm, a, nd in (("sel", sel, 1), (name, src, rank)):
        if not isinstance(a, np.ndarray) or a.dtype != np.int32:
            raise TypeError("recipe %s: an int32 numpy array is required, got %s" % (nm, getattr(a, "dtype", type(a))))
        if a.ndim != nd or not a.flags.c_contiguous:
            raise ValueError("recipe %s: a contiguous %d-d array is required (shape %r)" % (nm, nd, a.shape))
    n = sel.shape[0]
    if n < 1 or tail is None or src.shape != (n,) + tail:
        raise ValueError("recipe: sel %r and %s %r do not describe a batch of groups of %s"
                         % (sel.shape, name, src.shape, "%d" % G if T is None else "%d over %d steps" % (G, T)))
    if int(sel.min()) < 0 or int(sel.max()) >= N:
        raise ValueError("recipe sel: line numbers must lie in [0, %d) (min %d, max %d)" % (N, sel.min(), sel.max()))
    if int(src.min()) < 0 or int(src.max()) >= n:
        raise ValueError("recipe %s: batch positions must lie in [0, %d) (min %d, max %d)"
                         % (name, n, src.min(), src.max()))
    return n


def check_recipe(sel, src, N, G):
    """``sel`` int32 ``[n]`` line numbers in ``[0, N)``, ``src`` int32 ``[n, G]`` batch positions in ``[0, n)`` with
    ``src[:, 0]`` the line itself (the positive row).  Raises TypeError / ValueError; returns ``n``."""
    n = _check(sel, "src", src, N, 2, (G,), G)
    if not np.array_equal(src[:, 0], np.arange(n, dtype=np.int32)):
        raise ValueError("recipe src: column 0 must be the line itself")
    return n


def check_position_recipe(sel, psrc, N, G, T):
    """The recipe of a NextItNet training feed (``NextItNetColumnIterator``): ``sel`` int32 ``[n]`` line numbers in
    ``[0, N)``, ``psrc`` int32 ``[n, G - 1, T]`` batch positions in ``[0, n)`` -- the line whose (item, cate) negative row
    ``g + 1`` of line ``i`` carries at step ``t``.  Raises TypeError / ValueError; returns ``n``."""
    return _check(sel, "psrc", psrc, N, 3, (G - 1, T) if G >= 2 else None, G, T)


class ResidentColumns(object):
    """The device image of one file's column store (``cols``: a ``SequentialIterator._columns`` entry)."""

    def __init__(self, cols, device):
        missing = [k for k in COLUMNS if k not in cols]
        if missing:
            raise NotImplementedError("the iterator keeps no padded column store (missing %s): resident_data needs "
                                      "SequentialIterator / SASequentialIterator" % ", ".join(missing))
        self.cols = cols            # identity: the iterator re-parsed the file when its entry is another object
        self.N, self.T = int(cols["item_history"].shape[0]), int(cols["item_history"].shape[1])
        self.dev = {}
        for k, dt in _BIG:
            a = np.ascontiguousarray(cols[k], dtype=dt)
            if a.shape != (self.N, self.T):
                raise ValueError("column %s: shape %r, expected %r" % (k, a.shape, (self.N, self.T)))
            self.dev[k] = torch.from_numpy(a).to(device)
        for k in _SMALL:
            a = np.asarray(cols[k])
            if a.shape != (self.N,):
                raise ValueError("column %s: shape %r, expected %r" % (k, a.shape, (self.N,)))
            if a.size and (int(a.min()) < -2 ** 31 or int(a.max()) >= 2 ** 31):
                raise ValueError("column %s does not fit int32" % k)
            self.dev[k] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)
        # sticky error words of clsr_feed_build
        self.err = torch.zeros(4, dtype=torch.int32, device=device)

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self.dev.values())


class ResidentStore(object):
    """file -> :class:`ResidentColumns` of one iterator, uploaded on first use and again after a re-parse."""

    def __init__(self, iterator, device):
        if not hasattr(iterator, "_columns"):
            raise NotImplementedError("resident_data: %s keeps no column store" % type(iterator).__name__)
        self.iterator, self.device, self.files, self.uploads = iterator, device, {}, 0

    def get(self, infile, cols=None):
        """``cols``: the column dict a feed's recipe was drawn from (default: the iterator's current one)."""
        if cols is None:
            cols = self.iterator._columns.get(infile)
        if cols is None:
            raise KeyError("resident_data: %r has not been parsed by the iterator" % (infile,))
        rc = self.files.get(infile)
        if rc is None or rc.cols is not cols:
            rc = self.files[infile] = ResidentColumns(cols, self.device)
            self.uploads += 1
        return rc

    @property
    def nbytes(self):
        return sum(rc.nbytes for rc in self.files.values())


# ---------------------------------------------------------------------------------------------------------------------
# evaluation feeds (``resident_eval=True``): an image of its own per evaluated file, never shared with the training store


def same_rows(cols, keep):
    """The rule of ``clsr_feed_same_rows`` in numpy: uint8 ``[len(keep)]``, 1 where line ``keep[i]`` agrees with line
    ``keep[i - 1]`` in ``users`` (as float32, the form evaluation feeds carry them in), ``lens`` and every word of the four
    ``[N, T]`` columns under numpy's ``==`` (``-0.0 == 0.0``, a NaN equals nothing); ``flags[0] = 0``.  ``mask`` is a
    function of ``lens``.  This is what ``SequentialBaseModel._shared_history_group`` compares on the host."""
    keep = np.asarray(keep, dtype=np.int64)
    flags = np.zeros(len(keep), dtype=np.uint8)
    if len(keep) > 1:
        a, b = keep[1:], keep[:-1]
        users = np.asarray(cols["users"]).astype(np.float32)
        same = (users[a] == users[b]) & (np.asarray(cols["lens"])[a] == np.asarray(cols["lens"])[b])
        for k, _ in _BIG:
            c = np.asarray(cols[k])
            same &= (c[a] == c[b]).all(axis=1)
        flags[1:] = same
    return flags


def eval_chunk_plan(flags, n_keep, batch_size, target_rows, dedup=True):
    """The chunks ``SequentialBaseModel._device_eval`` scores on the host path, as ``[(k0, n, g)]``: lines ``k0 .. k0 + n``
    of ``keep`` in groups of ``g`` consecutive lines with one history.  ``batch_size`` consecutive lines form a batch; its
    ``g`` is the shortest run of equal lines (``flags``: :func:`same_rows`; the first line of a batch starts a run) if that
    is above 1, divides the batch and every run, else 1 -- the rule of ``_shared_history_group``; ``dedup=False``: 1
    everywhere, ``flags`` is not read.  Consecutive batches of equal ``g`` are joined until they hold ``target_rows``
    lines."""
    plan, pend = [], None
    for a in range(0, n_keep, batch_size):
        n = min(batch_size, n_keep - a)
        g = 1
        if dedup and n > 1:
            starts = np.flatnonzero(np.concatenate(([True], np.asarray(flags[a + 1:a + n]) == 0)))
            runs = np.diff(np.concatenate((starts, [n])))
            m = int(runs.min())
            if m > 1 and n % m == 0 and bool(np.all(runs % m == 0)):
                g = m
        if pend is not None and pend[2] != g:
            plan.append(tuple(pend))
            pend = None
        if pend is None:
            pend = [a, 0, g]
        pend[1] += n
        if pend[1] >= target_rows:
            plan.append(tuple(pend))
            pend = None
    if pend is not None:
        plan.append(tuple(pend))
    return plan


class ResidentEvalColumns(ResidentColumns):
    """The device image evaluation feeds are built from: the columns of :class:`ResidentColumns` plus ``labels`` (float32
    ``[N]``), ``N * (16 T + 20)`` bytes.  ``lines``: ``min_seq_length`` -> :class:`EvalLines`."""

    def __init__(self, cols, device):
        super(ResidentEvalColumns, self).__init__(cols, device)
        labels = np.asarray(cols["labels"])
        if labels.shape != (self.N,):
            raise ValueError("column labels: shape %r, expected %r" % (labels.shape, (self.N,)))
        users = np.asarray(cols["users"])
        if users.size and int(np.abs(users).max()) >= 2 ** 31 - 64:
            raise ValueError("column users: an id this large does not survive the float32 form of evaluation feeds")
        self.dev["labels"] = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.float32)).to(device)
        self.lines = {}


class EvalLines(object):
    """One ``(file, min_seq_length)``: ``keep`` int32 ``[n_keep]`` (host, checked against ``[0, N)``; ``keep_dev`` on the
    device), ``flags`` uint8 ``[n_keep]`` (host; None until a de-duplicating pass asked for them) and the file's columns
    ``rc``.  What ``CLSRNet.build_eval_feed`` takes."""

    def __init__(self, rc, keep, device):
        keep = np.asarray(keep)
        if keep.ndim != 1:
            raise ValueError("keep: a list of lines is required (shape %r)" % (keep.shape,))
        if keep.size and (int(keep.min()) < 0 or int(keep.max()) >= rc.N):
            raise ValueError("keep: line numbers must lie in [0, %d) (min %d, max %d)" % (rc.N, keep.min(), keep.max()))
        self.rc, self.keep, self.n_keep = rc, np.ascontiguousarray(keep, dtype=np.int32), int(keep.shape[0])
        self.keep_dev = torch.from_numpy(self.keep).to(device) if self.n_keep else None
        self.flags = None

    @property
    def nbytes(self):
        return 4 * self.n_keep if self.keep_dev is not None else 0


class ResidentEvalStore(object):
    """file -> :class:`ResidentEvalColumns` of one iterator.  The image is uploaded on first use and again after a
    re-parse (the iterator's column dict is another object then); ``keep`` and its flags are rebuilt whenever the
    iterator's list of lines differs from the cached one (a training pass over the same file shuffled it)."""

    def __init__(self, iterator, device):
        if (not hasattr(iterator, "eval_lines") or not getattr(iterator, "lazy_histories", False)
                or getattr(iterator, "per_position_targets", False)):       # (NextItNet: out of this store's scope)
            raise NotImplementedError("resident_eval: %s keeps no padded column store evaluation feeds are built from"
                                      % type(iterator).__name__)
        self.iterator, self.device, self.files, self.uploads = iterator, device, {}, 0

    def get(self, infile, min_seq_length=1, flags=True):
        """The :class:`EvalLines` of ``(infile, min_seq_length)``, current with the iterator.  ``flags``: also make sure
        the run flags are there (one ``clsr_feed_same_rows`` launch on the current stream and one read-back per
        ``keep``)."""
        from clsr_amd import ops

        cols, keep = self.iterator.eval_lines(infile, min_seq_length)
        rc = self.files.get(infile)
        if rc is None or rc.cols is not cols:
            rc = self.files[infile] = ResidentEvalColumns(cols, self.device)
            self.uploads += 1
        ent = rc.lines.get(min_seq_length)
        if ent is None or not np.array_equal(keep, ent.keep):
            ent = rc.lines[min_seq_length] = EvalLines(rc, keep, self.device)
        if flags and ent.flags is None:
            if ent.n_keep:
                dev = torch.empty(ent.n_keep, dtype=torch.uint8, device=self.device)
                ops.feed_same_rows(ops.feed_eval_pointers(rc.dev), rc.N, ent.keep_dev, ent.n_keep, rc.T, dev)
                ent.flags = dev.cpu().numpy()
            else:
                ent.flags = np.zeros(0, dtype=np.uint8)
        return ent

    @property
    def nbytes(self):
        return sum(rc.nbytes + sum(e.nbytes for e in rc.lines.values()) for rc in self.files.values())
