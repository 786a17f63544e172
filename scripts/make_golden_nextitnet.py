#!/usr/bin/env python
"""Generate tests/golden/iterator_{train,eval}_nextitnet.npz from the REFERENCE's NextItNetIterator.

Companion of scripts/make_golden.py (same TensorFlow stub, the same reference checkout, ``make_golden.REF``): the reference's
``NextItNetIterator._convert_data`` is numpy + ``random`` only.  Reads the committed golden data (tests/golden/data), which
it leaves untouched, and writes data only -- no reference source is copied:

  iterator_train_nextitnet.npz   ONE training feed, random.seed(1234), batch_num_ngs = 4, max_seq_length = 10
  iterator_eval_nextitnet.npz    ONE evaluation feed of valid_data
"""
import os
import random
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from make_golden import GOLD, REF, install_tf_stub  # noqa: E402


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, REF)
    install_tf_stub()
    warnings.simplefilter("ignore")
    from reco_utils.recommender.deeprec.io import nextitnet_iterator as ref_it

    d = os.path.join(GOLD, "data")

    class HP(object):
        user_vocab = os.path.join(d, "user_vocab.pkl")
        item_vocab = os.path.join(d, "item_vocab.pkl")
        cate_vocab = os.path.join(d, "category_vocab.pkl")
        max_seq_length = 10
        batch_size = 64
        time_unit = "s"

    it = ref_it.NextItNetIterator(HP, ref_it.tf.Graph())
    # (its own __init__ does not take over time_unit, which the base class's line parser reads)
    it.time_unit = HP.time_unit
    keys = {v: k for k, v in it.__dict__.items() if isinstance(v, ref_it.tf.placeholder)}
    for fname, infile, ngs in (("iterator_train_nextitnet.npz", "train_data", 4), ("iterator_eval_nextitnet.npz", "valid_data", 0)):
        random.seed(1234)
        out = {}
        for feed in it.load_data_from_file(os.path.join(d, infile), batch_num_ngs=ngs, min_seq_length=1):
            if not feed:
                continue
            for ph, val in feed.items():
                out["b0_" + keys[ph]] = val
            break
        out["n_batches"] = np.asarray(1)
        np.savez_compressed(os.path.join(GOLD, fname), **out)
        print(fname, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
