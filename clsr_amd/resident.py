"""Device image of an iterator's per-file column store, and the recipe checks of the resident feed path.

``SequentialIterator`` pads every line of a file once (``_columns``); a training batch is then a row gather driven by
``sel`` (the file lines drawn) and ``src`` (the in-batch line every output row takes its item / category from).  With
``resident_data=True`` a model keeps the columns the step reads in HBM -- ``item_history``, ``item_cate_history``,
``time_from_first_action``, ``time_to_now`` ``[N, T]`` and ``lens``, ``users``, ``items``, ``cates`` ``[N]``, 4-byte words all:
``N * (16 T + 16)`` bytes -- and ``clsr_feed_build`` (csrc/feed.hip) gathers the batch there; only ``sel`` and ``src`` cross
PCIe.  The image is uploaded once per cached file and again when the iterator re-parses the file (its column dict is a new
object then).  A failed allocation surfaces as torch raises it.
"""
import numpy as np
import torch

__all__ = ["ResidentColumns", "ResidentStore", "check_recipe", "COLUMNS"]

_BIG = (("item_history", np.int32), ("item_cate_history", np.int32), ("time_from_first_action", np.float32),
        ("time_to_now", np.float32))
_SMALL = ("lens", "users", "items", "cates")
COLUMNS = tuple(k for k, _ in _BIG) + _SMALL


def check_recipe(sel, src, N, G):
    """``sel`` int32 ``[n]`` line numbers in ``[0, N)``, ``src`` int32 ``[n, G]`` batch positions in ``[0, n)`` with
    ``src[:, 0]`` the line itself (the positive row).  Raises TypeError / ValueError; returns ``n``."""
    for name, a, nd in (("sel", sel, 1), ("src", src, 2)):
        if not isinstance(a, np.ndarray) or a.dtype != np.int32:
            raise TypeError("recipe %s: an int32 numpy array is required, got %s" % (name, getattr(a, "dtype", type(a))))
        if a.ndim != nd or not a.flags.c_contiguous:
            raise ValueError("recipe %s: a contiguous %d-d array is required (shape %r)" % (name, nd, a.shape))
    n = sel.shape[0]
    if n < 1 or src.shape != (n, G):
        raise ValueError("recipe: sel %r and src %r do not describe a batch of groups of %d" % (sel.shape, src.shape, G))
    if int(sel.min()) < 0 or int(sel.max()) >= N:
        raise ValueError("recipe sel: line numbers must lie in [0, %d) (min %d, max %d)" % (N, sel.min(), sel.max()))
    if int(src.min()) < 0 or int(src.max()) >= n:
        raise ValueError("recipe src: batch positions must lie in [0, %d) (min %d, max %d)" % (n, src.min(), src.max()))
    if not np.array_equal(src[:, 0], np.arange(n, dtype=np.int32)):
        raise ValueError("recipe src: column 0 must be the line itself")
    return n


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
