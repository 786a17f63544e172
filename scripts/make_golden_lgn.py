#!/usr/bin/env python
"""Generate tests/golden/lgn_graph.npz from the REFERENCE's LGNModel graph builders.

Companion of scripts/make_golden.py (the same reference checkout, ``make_golden.REF``).  The reference's ``get_adj_mat``
(get_R + create_adj_mat_ui) and ``get_item2cate`` (creat_item2cate) are numpy / scipy / pickle only; they run here as
unbound methods on an instance made with ``object.__new__`` -- no TensorFlow graph is built.  The model MODULE imports
TensorFlow and the trunk's modules at its top, so the stub of make_golden.py is widened: any attribute it does not
have resolves to an inert placeholder, which is enough for the ``import`` lines and class statements to run.

Both methods write caches next to the vocabularies (s_*_adj_mat_*.npz, item2cate), so they are pointed at a scratch
copy of tests/golden/data, which itself stays untouched.  Output -- arrays only, no reference source is copied:

  lgn_graph.npz   indptr, indices (ascending in a row), values (float32) of norm_adj = D^-1 (A + I) over the
                  user-item graph of train_data, [Vu + Vi] square, and item2cate [Vi] as the model uses it
                  (item2cate[0] = 0, unseen items -> 0)
"""
import os
import shutil
import sys
import tempfile
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from make_golden import GOLD, REF, install_tf_stub  # noqa: E402


class _Inert(object):
    """Stands for any TensorFlow name the model modules touch while they are imported."""

    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return _Inert()

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Inert()

    def __mro_entries__(self, bases):
        return (object,)


class _WideStub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        sub = _WideStub(self.__name__ + "." + name)
        sub.__path__ = []
        sys.modules[sub.__name__] = sub
        setattr(self, name, sub)
        return sub

    def __call__(self, *a, **k):
        return _Inert()

    def __mro_entries__(self, bases):
        return (object,)


def install_wide_tf_stub():
    install_tf_stub()
    narrow = sys.modules["tensorflow"]
    wide = _WideStub("tensorflow")
    wide.__path__ = []
    for k, v in vars(narrow).items():
        if not k.startswith("__"):
            setattr(wide, k, v)
    sys.modules["tensorflow"] = wide


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, REF)
    install_wide_tf_stub()
    warnings.simplefilter("ignore")
    from reco_utils.recommender.deeprec.models.sequential import lgn as ref_lgn
    from reco_utils.recommender.deeprec.deeprec_utils import load_dict

    scratch = tempfile.mkdtemp(prefix="lgn_golden_")
    try:
        d = os.path.join(scratch, "data")
        shutil.copytree(os.path.join(GOLD, "data"), d)

        class HP(object):
            user_vocab = os.path.join(d, "user_vocab.pkl")
            item_vocab = os.path.join(d, "item_vocab.pkl")
            cate_vocab = os.path.join(d, "category_vocab.pkl")

        m = object.__new__(ref_lgn.LGNModel)
        m.hparams, m.path, m.train_file = HP, d, os.path.join(d, "train_data")
        m.n_users, m.n_items = len(load_dict(HP.user_vocab)), len(load_dict(HP.item_vocab))
        m.user_vocab_length, m.item_vocab_length = m.n_users, m.n_items
        _, norm_adj, _, _ = m.get_adj_mat()
        # the lines of LGNModel._build_embedding between get_item2cate and the lookup, restated
        i2c = m.get_item2cate()
        i2c[0] = 0
        for i in range(m.item_vocab_length):
            if i not in i2c:
                i2c[i] = 0
        sorted_cate = [v for _, v in sorted(i2c.items(), key=lambda x: x[0])]
    finally:
        shutil.rmtree(scratch)
    a = norm_adj.tocsr().astype(np.float32)
    a.sort_indices()
    N = m.n_users + m.n_items
    assert a.shape == (N, N) and len(sorted_cate) == m.n_items
    out = dict(indptr=a.indptr.astype(np.int64), indices=a.indices.astype(np.int32), values=a.data.astype(np.float32),
               item2cate=np.asarray(sorted_cate, dtype=np.int32))
    np.savez_compressed(os.path.join(GOLD, "lgn_graph.npz"), **out)
    deg = np.diff(out["indptr"])
    print("lgn_graph.npz: shape %d^2, %d entries, degrees %d..%d, n_users %d, n_items %d"
          % (N, a.nnz, deg.min(), deg.max(), m.n_users, m.n_items))


if __name__ == "__main__":
    main()
