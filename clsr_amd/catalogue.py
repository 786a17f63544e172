"""The candidates of ``recommend_k_items``: item ids with the category each is scored with.

``Catalogue(items, cates)`` takes the arrays directly (a candidate pool); ``Catalogue.from_files(model, files)`` scans data
files in the project's line format with the model's vocabularies.  An item is paired with the FIRST category it appears
with: line by line, files in the given order, a line's target pair before its history pairs (``zip``: the shorter of the
two history lists ends it).  Items no file names are not candidates, and id 0 -- the padding row, and what a token outside
the vocabulary maps to -- never is.

(``clsr_amd/lgn_graph.py`` assigns in the same order but reads only the lines the reference's graph builder reads and lets
the LAST assignment win; where every item keeps one category, as in the data sets of the quick start, the two agree on every
item both name -- tests/test_recommend_cpu.py holds them together on the golden data.)

The device copies of the two arrays are made once per object and device and reused by every call.
"""
import numpy as np

__all__ = ["Catalogue"]


class Catalogue(object):
    def __init__(self, items, cates, n_items=None):
        """``items``: int32, ascending, unique, every id in ``1 .. n_items - 1``; ``cates``: int32, same length >= 1.
        ``n_items`` (the item vocabulary's size) may be left out: ``recommend_k_items`` checks against the model's."""
        it, ct = np.asarray(items), np.asarray(cates)
        for name, a in (("items", it), ("cates", ct)):
            if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
                raise ValueError("Catalogue: %s must be a one-dimensional integer array, got %s %r" % (name, a.dtype, a.shape))
        if it.shape[0] == 0:
            raise ValueError("Catalogue: items is empty -- a catalogue holds at least one candidate")
        if ct.shape[0] != it.shape[0]:
            raise ValueError("Catalogue: cates holds %d entries for %d items" % (ct.shape[0], it.shape[0]))
        it64 = it.astype(np.int64)
        if int(it64.min()) < 1:
            raise ValueError("Catalogue: items holds id %d -- candidates are ids from 1 on (0 is the padding row)" % int(it64.min()))
        d = np.diff(it64)
        if bool((d == 0).any()):
            raise ValueError("Catalogue: items holds id %d twice" % int(it64[1:][d == 0][0]))
        if bool((d < 0).any()):
            raise ValueError("Catalogue: items must ascend (id %d follows a larger one)" % int(it64[1:][d < 0][0]))
        if int(ct.min()) < 0:
            raise ValueError("Catalogue: cates holds the negative id %d" % int(ct.min()))
        if int(it64.max()) >= 2 ** 31 or int(ct.max()) >= 2 ** 31:
            raise ValueError("Catalogue: items / cates must fit int32")
        self.items = np.ascontiguousarray(it, dtype=np.int32)
        self.cates = np.ascontiguousarray(ct, dtype=np.int32)
        self._device = {}
        if n_items is not None:
            self.check_vocabulary(n_items)

    def __len__(self):
        return int(self.items.shape[0])

    def check_vocabulary(self, n_items, n_cates=None):
        """Raise unless every item id is a row of an item table of ``n_items`` rows (and every category of ``n_cates``)."""
        if int(self.items[-1]) >= int(n_items):
            raise ValueError("Catalogue: items holds id %d, the item vocabulary has %d rows" % (int(self.items[-1]), n_items))
        if n_cates is not None and int(self.cates.max()) >= int(n_cates):
            raise ValueError("Catalogue: cates holds id %d, the category vocabulary has %d rows" % (int(self.cates.max()), n_cates))

    def device(self, device):
        """``(items, cates)`` as int32 tensors on ``device``; copied on first use, the same tensors ever after."""
        import torch

        key = str(torch.device(device))
        dev = self._device.get(key)
        if dev is None:
            dev = self._device[key] = (torch.from_numpy(self.items).to(device), torch.from_numpy(self.cates).to(device))
        return dev

    @staticmethod
    def pairs(itemdict, catedict, files, col_spliter="\t"):
        """``(item ids, category ids)`` of every (item, category) occurrence of ``files`` in the order of assignment."""
        pi, pc = [], []
        for name in files:
            with open(name) as f:
                for line in f:
                    words = line.strip().split(col_spliter)
                    if len(words) < 7:
                        continue
                    hi, hc = words[5].strip().split(","), words[6].strip().split(",")
                    m = min(len(hi), len(hc))
                    pi.append(itemdict.get(words[2], 0))
                    pc.append(catedict.get(words[3], 0))
                    pi.extend(itemdict.get(w, 0) for w in hi[:m])
                    pc.extend(catedict.get(w, 0) for w in hc[:m])
        return np.asarray(pi, dtype=np.int64), np.asarray(pc, dtype=np.int64)

    @classmethod
    def from_files(cls, model_or_iterator, files):
        """The catalogue of the items ``files`` name, through the vocabularies of a model (or of its iterator)."""
        it = getattr(model_or_iterator, "iterator", model_or_iterator)
        if isinstance(files, str):
            files = [files]
        pi, pc = cls.pairs(it.itemdict, it.catedict, files, getattr(it, "col_spliter", "\t"))
        items, first = np.unique(pi, return_index=True)      # first occurrence of every id, ids ascending
        cates = pc[first]
        named = items > 0
        if not bool(named.any()):
            raise ValueError("Catalogue.from_files: files name no item of the vocabulary")
        return cls(items[named], cates[named], n_items=len(it.itemdict))
