"""Host-side batch builder for the CLSR step (numpy only).

Mirror of the reference's ``reco_utils/recommender/deeprec/io/sequential_iterator.py``
(``SequentialIterator`` ``:19-503`` and ``SASequentialIterator`` ``:506-732``):
same TSV format, same time features, same left-aligned zero padding, same
in-batch negative sampling driven by the global ``random`` module, so that for a
given ``random.seed`` the produced feeds are bit-identical to the reference's
(pinned by ``tests/golden/iterator_*.npz``, captured from the reference iterator).

Differences by design:
* feeds are keyed by field-name strings (``iterator.labels == "labels"`` ...)
  instead of TF placeholders -- ``feed[iterator.users]`` keeps working;
* the O(P*G*T) python loops of ``_convert_data`` (ref ``:588-634``) are replaced by a per-file
  column store (every line padded once) + row gathers; the negative-sampling draws
  (``random.randint`` rejection loop, ref ``:622-634``) replay the ``random`` module's
  Mersenne-Twister stream in numpy, so the RNG call sequence -- part of the observable
  behaviour -- is reproduced bit for bit.
"""
import random

import numpy as np

from clsr_amd.deeprec_utils import load_dict

__all__ = ["BaseIterator", "SequentialIterator", "SASequentialIterator", "NextItNetIterator", "NextItNetColumnIterator"]

_FIELDS = (
    "labels users items cates item_history item_cate_history mask time time_diff "
    "time_from_first_action time_to_now"
).split()


class _LazyLines(object):
    """Stand-in for ``iter_data[infile]`` (the reference caches the parsed per-line tuples there): knows its
    length, and parses the file the literal way the first time somebody actually looks at the lines."""

    def __init__(self, it, infile, n):
        self._it, self._infile, self._n, self._lines = it, infile, n, None

    def _get(self):
        if self._lines is None:
            self._lines = self._it.parse_file(self._infile)
        return self._lines

    def __len__(self):
        return self._n

    def __iter__(self):
        return iter(self._get())

    def __getitem__(self, i):
        return self._get()[i]


_NATIVE = [False, None]


def _native_lib():
    """libclsr_hip.so for the host-side MT19937 replay (clsr_host_mt_*), or None: the pure-python / numpy paths
    below produce the same streams, only slower."""
    if _NATIVE[0] is False:
        try:
            from clsr_amd import _lib

            lib = _lib.load()
            _NATIVE[1] = lib if hasattr(lib, "clsr_host_mt_shuffle") else None
        except Exception:
            _NATIVE[1] = None
        _NATIVE[0] = True
    return _NATIVE[1]


def _mt_state():
    """(key uint32[624], pos, gauss) of the global ``random`` module, or None if it is not a version-3 state."""
    version, state, gauss = random.getstate()
    if version != 3:
        return None
    return np.array(state[:-1], dtype=np.uint32), int(state[-1]), gauss


def _mt_restore(key, pos, gauss):
    random.setstate((3, tuple(key.tolist()) + (int(pos),), gauss))


def shuffle_like_random(perm):
    """In-place ``random.shuffle`` of the int64 array ``perm`` consuming exactly the random numbers the call on a
    list would (native replay when the library is built: 1M entries in ~10 ms instead of ~0.7 s)."""
    import ctypes

    lib, st = _native_lib(), _mt_state()
    if lib is not None and st is not None and perm.dtype == np.int64 and perm.flags.c_contiguous:
        key, pos, gauss = st
        cpos = ctypes.c_int(pos)
        rc = lib.clsr_host_mt_shuffle(key.ctypes.data, ctypes.byref(cpos), perm.ctypes.data, len(perm))
        if rc == 0:
            _mt_restore(key, cpos.value, gauss)
            return perm
    lst = perm.tolist()
    random.shuffle(lst)
    perm[:] = lst
    return perm


class LazyFeed(dict):
    """A feed dict whose big row-repeated arrays are built on first access.

    A training batch repeats every line's padded history ``1 + batch_num_ngs`` times
    (ref ``sequential_iterator.py:416-447``).  The CLSR device step only needs ONE copy per
    line (``feed.compact``: history-level arrays + ``hist_group``), so the repeated arrays are
    materialised only for a caller that actually reads them -- with exactly the values the
    reference produces.  Any whole-dict access (iteration, ``len``, ``in``, ``keys``/``items``/
    ``values``/``get``) materialises everything first, so this behaves like the plain dict.
    """

    #: ``(file, sel, src)`` of a training feed drawn from a column store: ``sel`` int32 ``[n]``, the file lines of the batch
    #: in batch order; ``src`` int32 ``[n, 1 + ngs]``, the batch line whose (item, cate) every output row carries.  Together
    #: with the file's columns (``_cols``) that is the whole batch: clsr_amd/resident.py rebuilds the feed on the device.
    #: (``NextItNetColumnIterator``: ``(file, sel, psrc)``, ``psrc`` int32 ``[n, ngs, T]`` -- the batch line whose (item, cate)
    #: negative row ``g + 1`` of line ``i`` carries at step ``t``.)
    recipe = None
    _cols = None

    def __init__(self, eager, thunks, compact):
        dict.__init__(self, eager)
        self._thunks = dict(thunks)
        self.compact = compact

    def __missing__(self, key):
        th = self._thunks.pop(key, None)
        if th is None:
            raise KeyError(key)
        val = th()
        dict.__setitem__(self, key, val)
        return val

    def _force(self):
        for k in list(self._thunks):
            self[k]
        return self

    def __iter__(self):
        return dict.__iter__(self._force())

    def __len__(self):
        return dict.__len__(self._force())

    def __contains__(self, key):
        return dict.__contains__(self, key) or key in self._thunks

    def keys(self):
        return dict.keys(self._force())

    def items(self):
        return dict.items(self._force())

    def values(self):
        return dict.values(self._force())

    def get(self, key, default=None):
        return self[key] if key in self else default

    def __eq__(self, other):
        return dict.__eq__(self._force(), other)

    __hash__ = None

    def __bool__(self):
        return True


class BaseIterator(object):
    """4-method contract of the reference's ``io/iterator.py:9-24``."""

    def parser_one_line(self, line):
        raise NotImplementedError

    def load_data_from_file(self, infile):
        raise NotImplementedError

    def _convert_data(self, *args, **kwargs):
        raise NotImplementedError

    def gen_feed_dict(self, data_dict):
        raise NotImplementedError


class SequentialIterator(BaseIterator):
    def __init__(self, hparams, graph=None, col_spliter="\t"):
        """Load the three vocabularies and remember batch geometry (ref ``:20-70``).

        ``graph`` is accepted and ignored (there is no TF graph).
        """
        self.col_spliter = col_spliter
        self.userdict = load_dict(hparams.user_vocab)
        self.itemdict = load_dict(hparams.item_vocab)
        self.catedict = load_dict(hparams.cate_vocab)
        self.max_seq_length = hparams.max_seq_length
        self.batch_size = hparams.batch_size
        self.iter_data = dict()
        self._columns = dict()
        self._order = dict()
        self.time_unit = hparams.time_unit
        self.graph = graph
        # feed keys (the reference exposes placeholders under these attribute names)
        for name in _FIELDS:
            setattr(self, name, name)

    # ------------------------------------------------------------------ parsing
    def parse_file(self, input_file):
        """Parse every line of ``input_file`` (ref ``:72-88``)."""
        with open(input_file, "r") as f:
            lines = f.readlines()
        return [self.parser_one_line(line) for line in lines if line]

    def parser_one_line(self, line):
        """One TSV line -> tuple of parsed fields (ref ``:90-163``).

        ``label \\t user \\t item \\t cate \\t ts \\t item_hist(csv) \\t cate_hist(csv) \\t ts_hist(csv)``
        """
        words = line.strip().split(self.col_spliter)
        label = int(words[0])
        user_id = self.userdict.get(words[1], 0)
        item_id = self.itemdict.get(words[2], 0)
        item_cate = self.catedict.get(words[3], 0)
        current_time = float(words[4])

        item_hist, cate_hist = self.get_item_cate_history_sequence(
            words[5].strip().split(","), words[6].strip().split(","), user_id
        )
        ts = np.asarray(self.get_time_history_sequence(words[7].strip().split(",")), dtype=np.float64)

        time_range = 3600 * 24 * 1000 if self.time_unit == "ms" else 3600 * 24 / 1000

        gaps = np.append(ts[1:] - ts[:-1], current_time - ts[-1]) / time_range
        time_diff = np.log(np.maximum(gaps, 0.5))
        since_first = np.append(ts[1:] - ts[0], current_time - ts[0]) / time_range
        time_from_first_action = np.log(np.maximum(since_first, 0.5))
        time_to_now = np.log(np.maximum((current_time - ts) / time_range, 0.5))

        return (
            label,
            user_id,
            item_id,
            item_cate,
            item_hist,
            cate_hist,
            current_time,
            time_diff,
            time_from_first_action,
            time_to_now,
        )

    def get_item_cate_history_sequence(self, item_history_words, cate_history_words, user_id):
        return (
            self.get_item_history_sequence(item_history_words),
            self.get_cate_history_sequence(cate_history_words),
        )

    def get_item_history_sequence(self, item_history_words):
        d = self.itemdict
        return [d.get(w, 0) for w in item_history_words]

    def get_cate_history_sequence(self, cate_history_words):
        d = self.catedict
        return [d.get(w, 0) for w in cate_history_words]

    def get_time_history_sequence(self, time_history_words):
        return [float(w) for w in time_history_words]

    # ------------------------------------------------------------------ batching
    def load_data_from_file(self, infile, batch_num_ngs=0, min_seq_length=1):
        """Generator of feed dicts, ``batch_size`` file lines each (ref ``:194-302``).

        Parsed files are cached in ``self.iter_data``; when ``batch_num_ngs > 0`` the
        cached list is shuffled in place with ``random.shuffle`` every call.  Yields
        ``None`` for a training batch the reference drops (fewer than 5 lines).

        Fast path: the padded / truncated per-line arrays are built ONCE per file
        (``self._columns``); a batch is then a row gather, and the in-batch negative
        sampling replays the global ``random`` module's Mersenne-Twister stream in numpy
        (bit-identical draws, see :func:`_sample_negatives`).
        """
        cols = self._columns.get(infile) if infile in self.iter_data else None
        if cols is None:
            cols = self._load_columns(infile)
        lines = self.iter_data[infile]
        # the reference shuffles the cached list of parsed lines in place on every training pass
        # (cumulative permutation); shuffling a persistent index list consumes the same random numbers
        # and yields the same order without touching the column store
        perm = self._order.get(infile)
        if perm is None or len(perm) != len(lines):
            perm = self._order[infile] = np.arange(len(lines), dtype=np.int64)
        if batch_num_ngs > 0:
            shuffle_like_random(perm)
        order = perm.copy()
        keep = self._kept(cols, order, min_seq_length)
        for a in range(0, len(keep), self.batch_size):
            sel = keep[a:a + self.batch_size]
            data = self._convert_rows(cols, sel, batch_num_ngs)
            feed = self.gen_feed_dict(data)
            if isinstance(data, LazyFeed) and data.recipe is not None:
                feed.recipe, feed._cols = (infile,) + data.recipe, cols
            yield feed if feed else None

    @staticmethod
    def _kept(cols, order, min_seq_length):
        return order[cols["full_len"][order] >= min_seq_length]

    def eval_lines(self, infile, min_seq_length=1):
        """``(cols, keep)``: the column store of ``infile`` and the file lines ``load_data_from_file(infile,
        batch_num_ngs=0, min_seq_length=...)`` would yield, in its order, ``batch_size`` of them a batch (the order a
        training pass left behind when the file was trained on).  Read-only: nothing is shuffled, no random number is
        drawn; a file not seen yet is parsed as ``load_data_from_file`` would parse it."""
        cols = self._columns.get(infile) if infile in self.iter_data else None
        if cols is None:
            cols = self._load_columns(infile)
        n = len(self.iter_data[infile])
        perm = self._order.get(infile)
        order = perm.copy() if perm is not None and len(perm) == n else np.arange(n, dtype=np.int64)
        return cols, self._kept(cols, order, min_seq_length)

    def _load_columns(self, infile):
        """Column store of ``infile``.  Fast path: the native tokenizer (``clsr_host_tsv_parse``: vocabulary look-ups
        and number parsing in one pass over the file bytes, ~40x faster than the per-line python parser on a 1 M-line
        file) + the time features / padding computed by the same numpy expressions as ``parser_one_line`` on the
        flattened histories.  ``iter_data[infile]`` (the reference caches the per-line tuples there) then holds a
        stand-in that parses the file the literal way only if somebody looks at the lines.  Anything irregular, a
        subclass with its own line parser, or no native library: the literal ``parse_file`` + ``_columns_of``."""
        cols = None
        try:
            cols = self._parse_columns_native(infile)
        except Exception:
            cols = None
        if cols is None:
            lines = self.parse_file(infile)
            self.iter_data[infile] = lines
            return self._columns_of(infile, lines)
        self._columns[infile] = cols
        self.iter_data[infile] = _LazyLines(self, infile, cols["n"])
        return cols

    def _native_vocab(self, which, d):
        """Native hash table of one vocabulary dict (built once per iterator)."""
        import ctypes

        cache = self.__dict__.setdefault("_nat_vocabs", {})
        if which not in cache:
            lib = _native_lib()
            keys = [k.encode("utf-8") for k in d.keys()]
            off = np.zeros(len(keys) + 1, dtype=np.int64)
            np.cumsum([len(k) for k in keys], out=off[1:])
            blob = b"".join(keys)
            ids = np.fromiter(d.values(), dtype=np.int64, count=len(keys)).astype(np.int32)
            lib.clsr_host_vocab_create.restype = ctypes.c_void_p
            lib.clsr_host_vocab_create.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
            h = lib.clsr_host_vocab_create(blob, off.ctypes.data, ids.ctypes.data, len(keys))
            if not h:
                raise RuntimeError("clsr_host_vocab_create failed")
            cache[which] = h
        return cache[which]

    def _parse_columns_native(self, infile):
        import ctypes

        lib = _native_lib()
        cls = type(self)
        if lib is None or not hasattr(lib, "clsr_host_tsv_parse") or self.col_spliter != "\t":
            return None
        for meth in ("parser_one_line", "parse_file", "get_item_cate_history_sequence", "get_item_history_sequence",
                     "get_cate_history_sequence", "get_time_history_sequence"):
            if getattr(cls, meth) is not getattr(SequentialIterator, meth):
                return None                                 # a subclass customised the parsing
        with open(infile, "rb") as f:
            buf = f.read()
        if not buf or b"\r" in buf:
            return None                                     # (universal-newline translation: leave it to python)
        vp, lp = ctypes.c_void_p, ctypes.c_long
        nl, nt = lp(0), lp(0)
        lib.clsr_host_tsv_count.argtypes = [ctypes.c_char_p, lp, ctypes.POINTER(lp), ctypes.POINTER(lp)]
        if lib.clsr_host_tsv_count(buf, len(buf), ctypes.byref(nl), ctypes.byref(nt)) != 0:
            return None
        n, ntok = nl.value, nt.value
        if n == 0:
            return None
        i32, f64 = np.int32, np.float64
        labels, users, items, cates = (np.empty(n, dtype=i32) for _ in range(4))
        cur = np.empty(n, dtype=f64)
        off = np.empty(n + 1, dtype=np.int64)
        h_items, h_cates = np.empty(ntok, dtype=i32), np.empty(ntok, dtype=i32)
        ts = np.empty(ntok, dtype=f64)
        lib.clsr_host_tsv_parse.argtypes = [ctypes.c_char_p, lp] + [vp] * 12
        rc = lib.clsr_host_tsv_parse(buf, len(buf), self._native_vocab("u", self.userdict),
                                     self._native_vocab("i", self.itemdict), self._native_vocab("c", self.catedict),
                                     labels.ctypes.data, users.ctypes.data, items.ctypes.data, cates.ctypes.data,
                                     cur.ctypes.data, off.ctypes.data, h_items.ctypes.data, h_cates.ctypes.data,
                                     ts.ctypes.data)
        if rc != 0 or off[n] != ntok:
            return None
        T = self.max_seq_length
        full = np.diff(off)
        starts, ends = off[:-1], off[1:]
        line_of = np.repeat(np.arange(n), full)
        time_range = 3600 * 24 * 1000 if self.time_unit == "ms" else 3600 * 24 / 1000
        # the same expressions as parser_one_line, on the flattened histories: next timestamp of every history
        # position (the current time after the last one), first timestamp of its line
        nxt = np.empty_like(ts)
        nxt[:-1] = ts[1:]
        nxt[ends - 1] = cur
        first = ts[starts][line_of]
        tdiff = np.log(np.maximum((nxt - ts) / time_range, 0.5))
        tfirst = np.log(np.maximum((nxt - first) / time_range, 0.5))
        tnow = np.log(np.maximum((cur[line_of] - ts) / time_range, 0.5))
        # most recent T actions, left aligned, zero padded (as _columns_of)
        lens = np.minimum(full, T)
        within = np.arange(ntok) - starts[line_of]
        skip = (full - lens)[line_of]
        keep = within >= skip
        r_idx, c_idx = line_of[keep], (within - skip)[keep]

        def scatter(vals, dtype):
            out = np.zeros((n, T), dtype=dtype)
            out[r_idx, c_idx] = vals[keep]
            return out

        mask = np.zeros((n, T), dtype=np.float32)
        mask[r_idx, c_idx] = 1.0
        return dict(
            n=n, lens=lens, full_len=full, labels=labels.astype(np.float32), users=users, items=items, cates=cates,
            time=cur.astype(np.float32), item_history=scatter(h_items, np.int32),
            item_cate_history=scatter(h_cates, np.int32), mask=mask, time_diff=scatter(tdiff, np.float32),
            time_from_first_action=scatter(tfirst, np.float32), time_to_now=scatter(tnow, np.float32))

    def _columns_of(self, infile, lines):
        """Per-file column store: every parsed line padded once (most recent T actions, left aligned)."""
        cols = self._columns.get(infile)
        if cols is not None and cols["n"] == len(lines):
            return cols
        lens, item_hist, cate_hist, mask, tdiff, tfirst, tnow = self._pad_histories(
            [l[4] for l in lines], [l[5] for l in lines], [l[7] for l in lines], [l[8] for l in lines],
            [l[9] for l in lines])
        cols = dict(
            n=len(lines), lens=lens, full_len=np.fromiter((len(l[4]) for l in lines), np.int64,
                                                                             len(lines)),
            labels=np.asarray([l[0] for l in lines], dtype=np.float32),
            users=np.asarray([l[1] for l in lines], dtype=np.int32),
            items=np.asarray([l[2] for l in lines], dtype=np.int32),
            cates=np.asarray([l[3] for l in lines], dtype=np.int32),
            time=np.asarray([l[6] for l in lines], dtype=np.float32),
            item_history=item_hist, item_cate_history=cate_hist, mask=mask, time_diff=tdiff,
            time_from_first_action=tfirst, time_to_now=tnow)
        self._columns[infile] = cols
        return cols

    def _convert_rows(self, cols, sel, batch_num_ngs):
        """Same result as ``_convert_data`` on the selected lines, from the cached columns."""
        n = len(sel)
        if batch_num_ngs and n < 5:
            return None
        items, cates = cols["items"][sel], cols["cates"][sel]
        res = {}
        if batch_num_ngs:
            G = batch_num_ngs + 1
            src = self._sample_negatives(items.tolist(), batch_num_ngs)
            flat = src.reshape(-1)
            rows = np.repeat(sel, G)
            labels = np.zeros((n, G), dtype=np.float32)
            labels[:, 0] = 1.0
            res["labels"] = labels.reshape(-1, 1)
            row_cates = cates[flat]
            if self._with_attn_labels and not self.lazy_histories:
                res["attn_labels"] = self._attn_labels(cols["item_cate_history"][rows], cols["mask"][rows],
                                                       cols["lens"][rows], row_cates)
            res["users"] = cols["users"][rows]
            res["items"] = items[flat]
            res["cates"] = row_cates
            res["time"] = cols["time"][rows]
        else:
            rows = sel
            res["labels"] = cols["labels"][sel].reshape(-1, 1)
            if self._with_attn_labels:
                res["attn_labels"] = self._attn_labels(cols["item_cate_history"][rows], cols["mask"][rows],
                                                       cols["lens"][rows], cates)
            res["users"] = cols["users"][sel].astype(np.float32)
            res["items"] = items
            res["cates"] = cates
            res["time"] = cols["time"][sel]
        big = ("item_history", "item_cate_history", "mask", "time_diff", "time_from_first_action", "time_to_now")
        if batch_num_ngs and self.lazy_histories:
            if self.defer_compact:
                # (a consumer that rebuilds the batch on the device from ``recipe`` never reads these: no work
                # proportional to n * T is left in the batch)
                ct = {k: (lambda k=k: cols[k][sel]) for k in big if k != "time_diff"}
                ct["users"] = lambda: cols["users"][sel]
                compact = LazyFeed({"hist_group": batch_num_ngs + 1}, ct, None)
            else:
                compact = {k: cols[k][sel] for k in big if k != "time_diff"}
                compact["users"] = cols["users"][sel]
                compact["hist_group"] = batch_num_ngs + 1
            thunks = {k: (lambda k=k: cols[k][rows]) for k in big}
            if self._with_attn_labels:
                thunks["attn_labels"] = lambda: self._attn_labels(
                    cols["item_cate_history"][rows], cols["mask"][rows], cols["lens"][rows], row_cates)
            out = LazyFeed(res, thunks, compact)
            if n < (1 << 31) // G and cols["n"] < (1 << 31):
                out.recipe = (np.ascontiguousarray(sel, dtype=np.int32), np.ascontiguousarray(src, dtype=np.int32))
            return out
        for k in big:
            res[k] = cols[k][rows]
        return res

    def _convert_chunk(self, chunk, batch_num_ngs):
        cols = list(zip(*chunk))
        return self._convert_data(
            list(cols[0]), list(cols[1]), list(cols[2]), list(cols[3]), list(cols[4]),
            list(cols[5]), list(cols[6]), list(cols[7]), list(cols[8]), list(cols[9]),
            batch_num_ngs,
        )

    _with_attn_labels = False
    #: training feeds defer the (1 + ngs)-fold repetition of the padded histories (see LazyFeed)
    lazy_histories = True
    #: also defer the history-level arrays of ``feed.compact`` (set by a model built with ``resident_data=True``, which
    #: reads ``feed.recipe`` instead); whoever reads them still gets today's values
    defer_compact = False

    def _pad_histories(self, item_history_batch, item_cate_history_batch, time_diff_list,
                       time_from_first_action_list, time_to_now_list):
        """Most recent ``T`` actions, left-aligned, zero padded (ref ``:353-396, 588-610``)."""
        n = len(item_history_batch)
        T = self.max_seq_length
        lens = np.fromiter((min(len(h), T) for h in item_history_batch), dtype=np.int64, count=n)
        total = int(lens.sum())
        rows = np.repeat(np.arange(n), lens)
        cols = np.arange(total) - np.repeat(np.cumsum(lens) - lens, lens)

        def scatter(seqs, dtype):
            out = np.zeros((n, T), dtype=dtype)
            if total:
                flat = np.concatenate(
                    [np.asarray(s[len(s) - l:], dtype=dtype) for s, l in zip(seqs, lens) if l > 0]
                )
                out[rows, cols] = flat
            return out

        item_hist = scatter(item_history_batch, np.int32)
        cate_hist = scatter(item_cate_history_batch, np.int32)
        tdiff = scatter(time_diff_list, np.float32)
        tfirst = scatter(time_from_first_action_list, np.float32)
        tnow = scatter(time_to_now_list, np.float32)
        mask = np.zeros((n, T), dtype=np.float32)
        mask[rows, cols] = 1.0
        return lens, item_hist, cate_hist, mask, tdiff, tfirst, tnow

    def _sample_negatives(self, item_list, batch_num_ngs):
        """In-batch negative sampling with the reference's exact RNG call sequence
        (``random.randint(0, n-1)``, reject draws whose item equals the positive;
        ref ``:398-414, 612-634``).  Returns ``src[n, 1+ngs]``: for every output row,
        the index of the batch line whose (item, cate) it carries.
        """
        n = len(item_list)
        src = np.empty((n, batch_num_ngs + 1), dtype=np.int64)
        lib, st = _native_lib(), _mt_state()
        if lib is not None and st is not None and 2 <= n < (1 << 31):
            import ctypes

            key, pos, gauss = st
            cpos = ctypes.c_int(pos)
            items64 = np.ascontiguousarray(item_list, dtype=np.int64)
            if len(np.unique(items64[:64])) > 1 or len(np.unique(items64)) > 1:   # the reference loops forever otherwise
                rc = lib.clsr_host_mt_sample_negatives(key.ctypes.data, ctypes.byref(cpos), items64.ctypes.data, n,
                                                       batch_num_ngs, src.ctypes.data)
                if rc == 0:
                    _mt_restore(key, cpos.value, gauss)
                    return src
        src[:, 0] = np.arange(n)
        # random.randint(0, n-1) == _randbelow(n): k = n.bit_length(); r = getrandbits(k) until r < n, and
        # getrandbits(k <= 32) is one MT19937 32-bit output >> (32 - k).  Replay that stream with numpy's
        # MT19937 seeded from the module's state, then put the advanced state back.
        k = n.bit_length()
        version, state, gauss = random.getstate()
        if version != 3 or k > 32 or n < 2:
            return self._sample_negatives_py(item_list, batch_num_ngs, src)
        mt = np.random.MT19937()
        mt.state = {"bit_generator": "MT19937", "state": {"key": np.asarray(state[:-1], dtype=np.uint32),
                                                          "pos": int(state[-1])}}
        need = n * batch_num_ngs
        items = np.asarray(item_list)
        consumed = 0     # raw 32-bit outputs consumed from the stream so far
        flat = np.empty(need, dtype=np.int64)
        filled = 0       # output slot ``filled`` belongs to line ``filled // batch_num_ngs``
        while filled < need:
            block = max(4096, int((need - filled) * 1.3 * (1 << k) / n) + 64)
            raw = mt.random_raw(block) >> np.uint64(32 - k)
            ok = np.flatnonzero(raw < n)
            cand = raw[ok].astype(np.int64)
            p = 0        # candidates of this block consumed so far (accepted or rejected)
            while p < len(cand) and filled < need:
                m = min(len(cand) - p, need - filled)
                c = cand[p:p + m]
                owner = (filled + np.arange(m)) // batch_num_ngs
                rej = items[c] == items[owner]
                if rej.any():            # a draw that hit the positive's own item: skip it, re-align the rest
                    m = int(np.argmax(rej))
                    flat[filled:filled + m] = c[:m]
                    p += m + 1
                else:
                    flat[filled:filled + m] = c
                    p += m
                filled += m
            used_upto = int(ok[p - 1]) if p else -1
            consumed_in_block = used_upto + 1 if filled == need else block
            if filled == need and consumed_in_block < block:
                # rewind: rebuild the generator at the exact consumed position
                mt2 = np.random.MT19937()
                mt2.state = {"bit_generator": "MT19937", "state": {"key": np.asarray(state[:-1], dtype=np.uint32),
                                                                   "pos": int(state[-1])}}
                total = consumed + consumed_in_block
                if total:
                    mt2.random_raw(total)
                mt = mt2
            consumed += consumed_in_block
        src[:, 1:] = flat.reshape(n, batch_num_ngs)
        st = mt.state["state"]
        random.setstate((3, tuple(int(x) for x in st["key"]) + (int(st["pos"]),), gauss))
        return src

    def _sample_negatives_py(self, item_list, batch_num_ngs, src):
        """Plain-python fallback with the reference's literal loop (used for degenerate batch sizes)."""
        n = len(item_list)
        randint = random.randint
        hi = n - 1
        for i in range(n):
            pos = item_list[i]
            count = 0
            while count < batch_num_ngs:
                j = randint(0, hi)
                if item_list[j] == pos:
                    continue
                count += 1
                src[i, count] = j
        return src

    def _convert_data(self, label_list, user_list, item_list, item_cate_list, item_history_batch,
                      item_cate_history_batch, time_list, time_diff_list,
                      time_from_first_action_list, time_to_now_list, batch_num_ngs):
        """Lists of parsed fields -> dict of numpy arrays (ref ``:304-478``; SA variant ``:519-704``).

        Training (``batch_num_ngs > 0``): every line becomes ``1 + batch_num_ngs`` rows
        (positive first); batches with fewer than 5 lines are dropped (returns ``None``).
        Evaluation: one row per line, ``users`` as float32 like the reference (``:462, 694``).
        """
        n = len(label_list)
        if batch_num_ngs:
            if n < 5:
                return None
        lens, item_hist, cate_hist, mask, tdiff, tfirst, tnow = self._pad_histories(
            item_history_batch, item_cate_history_batch, time_diff_list,
            time_from_first_action_list, time_to_now_list,
        )
        items = np.asarray(item_list, dtype=np.int32)
        cates = np.asarray(item_cate_list, dtype=np.int32)
        res = {}
        if batch_num_ngs:
            G = batch_num_ngs + 1
            src = self._sample_negatives(item_list, batch_num_ngs)
            flat_src = src.reshape(-1)
            labels = np.zeros((n, G), dtype=np.float32)
            labels[:, 0] = 1.0
            res["labels"] = labels.reshape(-1, 1)
            row_items = items[flat_src]
            row_cates = cates[flat_src]
            rep = np.repeat(np.arange(n), G)
            if self._with_attn_labels:
                res["attn_labels"] = self._attn_labels(cate_hist[rep], mask[rep], lens[rep], row_cates)
            res["users"] = np.repeat(np.asarray(user_list, dtype=np.int32), G)
            res["items"] = row_items
            res["cates"] = row_cates
            res["item_history"] = item_hist[rep]
            res["item_cate_history"] = cate_hist[rep]
            res["mask"] = mask[rep]
            res["time"] = np.repeat(np.asarray(time_list, dtype=np.float32), G)
            res["time_diff"] = tdiff[rep]
            res["time_from_first_action"] = tfirst[rep]
            res["time_to_now"] = tnow[rep]
            return res

        res["labels"] = np.asarray(label_list, dtype=np.float32).reshape(-1, 1)
        if self._with_attn_labels:
            res["attn_labels"] = self._attn_labels(cate_hist, mask, lens, cates)
        res["users"] = np.asarray(user_list, dtype=np.float32)
        res["items"] = items
        res["cates"] = cates
        res["item_history"] = item_hist
        res["item_cate_history"] = cate_hist
        res["mask"] = mask
        res["time"] = np.asarray(time_list, dtype=np.float32)
        res["time_diff"] = tdiff
        res["time_from_first_action"] = tfirst
        res["time_to_now"] = tnow
        return res

    @staticmethod
    def _attn_labels(cate_hist, mask, lens, row_cates):
        """Fraction of the (truncated) history whose category equals the row's target
        category (ref ``:618, 629, 677-678``).  A zero-length history gives 0/0 = nan,
        as in the reference."""
        same = ((cate_hist == row_cates[:, None]) & (mask > 0)).sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = same / lens.astype(np.float64)
        return frac.astype(np.float32).reshape(-1, 1)

    def gen_feed_dict(self, data_dict):
        """Map field names to arrays; empty dict for a dropped batch (ref ``:480-503``)."""
        if not data_dict:
            return dict()
        if isinstance(data_dict, LazyFeed):
            eager = {getattr(self, n): dict.__getitem__(data_dict, n) for n in _FIELDS
                     if dict.__contains__(data_dict, n)}
            thunks = {getattr(self, n): (lambda n=n: data_dict[n]) for n in _FIELDS
                      if not dict.__contains__(data_dict, n)}
            return LazyFeed(eager, thunks, data_dict.compact)
        return {getattr(self, name): data_dict[name] for name in _FIELDS}


class SASequentialIterator(SequentialIterator):
    """Adds ``attn_labels`` (ref ``:506-732``); the iterator CLSR is built with
    (``examples/00_quick_start/sequential.py:88-91``)."""

    _with_attn_labels = True

    def __init__(self, hparams, graph=None, col_spliter="\t"):
        super(SASequentialIterator, self).__init__(hparams, graph, col_spliter)
        self.attn_labels = "attn_labels"

    def gen_feed_dict(self, data_dict):
        if not data_dict:
            return dict()
        feed = super(SASequentialIterator, self).gen_feed_dict(data_dict)
        if isinstance(feed, LazyFeed) and not dict.__contains__(data_dict, "attn_labels"):
            feed._thunks[self.attn_labels] = lambda: data_dict["attn_labels"]
        else:
            feed[self.attn_labels] = data_dict["attn_labels"]
        return feed


class NextItNetIterator(SequentialIterator):
    """Feeds of the NextItNet model (ref ``io/nextitnet_iterator.py``): histories are LEFT-padded (the most recent action
    sits at step ``T - 1``), and a training instance carries a target per position -- ``items`` / ``cates`` / ``labels`` are
    ``[n * (1 + ngs), T]``: row 0 of a group is the history shifted by one step with the target appended, the other rows
    are negatives drawn per position from the batch's targets (``random.randint`` over the instances, a draw equal to the
    positive of that position is rejected).  Evaluation feeds are those of ``SequentialIterator`` with left padding.

    The literal conversion path: per-line tuples, no column store, no native sampler (the draws are ``random.randint``
    calls in the reference's order, so ``random.seed`` reproduces its stream)."""

    lazy_histories = False

    def _load_columns(self, infile):
        lines = self.parse_file(infile)
        self.iter_data[infile] = lines
        cols = dict(n=len(lines), lines=lines, full_len=np.fromiter((len(l[4]) for l in lines), np.int64, len(lines)))
        self._columns[infile] = cols
        return cols

    def _convert_rows(self, cols, sel, batch_num_ngs):
        return self._convert_chunk([cols["lines"][int(i)] for i in sel], batch_num_ngs)

    def _left_pad(self, seqs, dtype, repeat):
        T = self.max_seq_length
        out = np.zeros((len(seqs), T), dtype=dtype)
        for i, s in enumerate(seqs):
            n = min(len(s), T)
            if n:       # (a slice [-0:] would take the whole row)
                out[i, T - n:] = np.asarray(s[len(s) - n:], dtype=dtype)
        return np.repeat(out, repeat, axis=0) if repeat > 1 else out

    def _convert_data(self, label_list, user_list, item_list, item_cate_list, item_history_batch,
                      item_cate_history_batch, time_list, time_diff_list,
                      time_from_first_action_list, time_to_now_list, batch_num_ngs):
        n, T = len(label_list), self.max_seq_length
        if batch_num_ngs and n < 5:
            return None
        G = batch_num_ngs + 1 if batch_num_ngs else 1
        res = {}
        res["item_history"] = self._left_pad(item_history_batch, np.int32, G)
        res["item_cate_history"] = self._left_pad(item_cate_history_batch, np.int32, G)
        res["mask"] = self._left_pad([[1.0] * len(h) for h in item_history_batch], np.float32, G)
        res["time_diff"] = self._left_pad(time_diff_list, np.float32, G)
        res["time_from_first_action"] = self._left_pad(time_from_first_action_list, np.float32, G)
        res["time_to_now"] = self._left_pad(time_to_now_list, np.float32, G)
        if not batch_num_ngs:
            res["labels"] = np.asarray(label_list, dtype=np.float32).reshape(-1, 1)
            res["users"] = np.asarray(user_list, dtype=np.float32)
            res["items"] = np.asarray(item_list, dtype=np.int32).reshape(-1, 1)
            res["cates"] = np.asarray(item_cate_list, dtype=np.int32).reshape(-1, 1)
            res["time"] = np.asarray(time_list, dtype=np.float32)
            return res
        items = np.zeros((n * G, T), dtype=np.int32)
        cates = np.zeros((n * G, T), dtype=np.int32)
        labels = np.zeros((n * G, T), dtype=np.float32)
        randint = random.randint
        for i in range(n):
            r0 = i * G
            # the positive row: the history one step on, the instance's target last
            items[r0, :T - 1], items[r0, T - 1] = res["item_history"][r0, 1:], item_list[i]
            cates[r0, :T - 1], cates[r0, T - 1] = res["item_cate_history"][r0, 1:], item_cate_list[i]
            labels[r0] = 1.0
            pos = items[r0].tolist()
            for g in range(1, G):
                for t in range(T):
                    j = randint(0, n - 1)
                    while item_list[j] == pos[t]:
                        j = randint(0, n - 1)
                    items[r0 + g, t], cates[r0 + g, t] = item_list[j], item_cate_list[j]
        res["labels"], res["items"], res["cates"] = labels, items, cates
        res["users"] = np.repeat(np.asarray(user_list, dtype=np.int32), G)
        res["time"] = np.repeat(np.asarray(time_list, dtype=np.float32), G)
        return res


class NextItNetColumnIterator(NextItNetIterator):
    """The feeds of :class:`NextItNetIterator`, array for array, from a per-file column store: every line is padded once
    (left padding: the most recent action at step ``T - 1``), an evaluation batch is a row gather, and the per-position
    negative sampling of a training batch replays the ``random`` module's stream natively
    (``clsr_host_mt_sample_negatives_pos``: the draws, their order and the state ``random`` is left in are the literal
    loop's).  A training feed is a :class:`LazyFeed` with every array deferred -- work proportional to ``n * G * T`` is left to
    whoever reads it -- that carries the recipe ``(file, sel, psrc)`` and its column dict, from which
    ``clsr_feed_build_pos`` rebuilds the batch on the device (clsr_amd/resident.py).  Without the native library, with a
    ``random`` state that is not version 3, or for a batch the native sampler refuses, the draws are ``random.randint``
    calls in the literal order."""

    lazy_histories = True
    #: ``items`` / ``cates`` / ``labels`` of a training feed hold a target per position and its recipe is
    #: ``(file, sel, psrc)``: the consumers of ``(file, sel, src)`` recipes and of evaluation column stores ask for this
    per_position_targets = True

    _BIG = ("item_history", "item_cate_history", "mask", "time_diff", "time_from_first_action", "time_to_now")

    def _load_columns(self, infile):
        self._columns.pop(infile, None)
        left = SequentialIterator._load_columns(self, infile)       # left ALIGNED: the history starts at step 0
        T = self.max_seq_length
        lens = np.asarray(left["lens"])
        at = np.arange(T)[None, :] - (T - lens[:, None])            # the left-aligned step every padded step shows
        cols = dict(left)
        for k in self._BIG:
            a = np.take_along_axis(left[k], np.maximum(at, 0), axis=1)
            a[at < 0] = 0
            cols[k] = a
        self._columns[infile] = cols
        return cols

    def _convert_rows(self, cols, sel, batch_num_ngs):
        n = len(sel)
        if batch_num_ngs and n < 5:
            return None
        if not batch_num_ngs:
            res = {k: cols[k][sel] for k in self._BIG}
            res["labels"] = cols["labels"][sel].reshape(-1, 1)
            res["users"] = cols["users"][sel].astype(np.float32)
            res["items"] = cols["items"][sel].reshape(-1, 1)
            res["cates"] = cols["cates"][sel].reshape(-1, 1)
            res["time"] = cols["time"][sel]
            return res
        G, T = batch_num_ngs + 1, self.max_seq_length
        items, cates = cols["items"][sel], cols["cates"][sel]
        # the positive rows: the history one step on, the instance's target last
        pos = np.concatenate((cols["item_history"][sel][:, 1:], items[:, None]), axis=1)
        psrc = self._sample_positions(items, pos, batch_num_ngs)
        rows = np.repeat(sel, G)

        def targets(own, positive):
            out = np.empty((n, G, T), dtype=np.int32)
            out[:, 0], out[:, 1:] = positive, own[psrc]
            return out.reshape(n * G, T)

        def labels():
            out = np.zeros((n, G, T), dtype=np.float32)
            out[:, 0] = 1.0
            return out.reshape(n * G, T)

        thunks = {k: (lambda k=k: cols[k][rows]) for k in self._BIG}
        thunks["items"] = lambda: targets(items, pos)
        thunks["cates"] = lambda: targets(cates, np.concatenate((cols["item_cate_history"][sel][:, 1:], cates[:, None]),
                                                               axis=1))
        thunks["labels"] = labels
        thunks["users"] = lambda: cols["users"][rows]
        thunks["time"] = lambda: cols["time"][rows]
        out = LazyFeed({}, thunks, None)
        out.recipe = (np.ascontiguousarray(sel, dtype=np.int32), psrc)
        return out

    def _sample_positions(self, items, pos, batch_num_ngs):
        """``psrc`` int32 ``[n, ngs, T]`` with the literal loop's draws (``NextItNetIterator._convert_data``): line ``i``,
        negative ``g``, step ``t`` in that order, ``j = randint(0, n - 1)`` redrawn while ``items[j] == pos[i, t]``."""
        n, T = pos.shape
        psrc = np.empty((n, batch_num_ngs, T), dtype=np.int32)
        lib, st = _native_lib(), _mt_state()
        if (lib is not None and hasattr(lib, "clsr_host_mt_sample_negatives_pos") and st is not None
                and 2 <= n < (1 << 31)):
            import ctypes

            key, p, gauss = st
            cpos = ctypes.c_int(p)
            items = np.ascontiguousarray(items, dtype=np.int32)
            pos = np.ascontiguousarray(pos, dtype=np.int32)
            rc = lib.clsr_host_mt_sample_negatives_pos(key.ctypes.data, ctypes.byref(cpos), items.ctypes.data,
                                                       pos.ctypes.data, n, batch_num_ngs, T, psrc.ctypes.data)
            if rc == 0:
                _mt_restore(key, cpos.value, gauss)
                return psrc
            # (refused, state untouched: a position no line of the batch can serve -- the literal loop never ends on it)
        randint, item_list, hi = random.randint, items.tolist(), n - 1
        for i in range(n):
            own = pos[i].tolist()
            for g in range(batch_num_ngs):
                for t in range(T):
                    j = randint(0, hi)
                    while item_list[j] == own[t]:
                        j = randint(0, hi)
                    psrc[i, g, t] = j
        return psrc
