#!/usr/bin/env python
"""Interactions/s through a model's ``fit`` training loop (TSV -> iterator -> device feed -> step) next to the model's
resident-input step rate, for CLSR and its sibling models, with the feeds uploaded from the host (default) or gathered on
the device from the resident column store (``--resident_data``): the protocol of scripts/fit_throughput.py -- a synthetic
Taobao-shaped file, batch 4096, T = 50, 4 negatives -- repeated over ``--regions`` timed regions of ``--epochs`` passes
each, so that a median and a spread (max - min) can be quoted.  Prints one JSON line.

The per-batch host times are measured on their own: the iterator alone (what the prefetch thread does per batch), and
``_to_arrays`` + ``_stage`` alone (what the main thread does per batch besides launching the step; the device is idle).
With ``--resident_data`` the builder's device time per batch is taken with events around ``build_feed``."""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import clsr_amd.clsr as M  # noqa: E402
from clsr_amd.deeprec_utils import prepare_hparams  # noqa: E402
from clsr_amd.sequential_iterator import (NextItNetColumnIterator, NextItNetIterator, SASequentialIterator,  # noqa: E402
                                           SequentialIterator)
from clsr_amd.synthetic import make_tsv_dataset  # noqa: E402

MODELS = {"clsr": ("CLSRModel", "clsr.yaml", SASequentialIterator), "a2svd": ("A2SVDModel", "asvd.yaml", SequentialIterator),
          "gru4rec": ("GRU4RecModel", "gru4rec.yaml", SequentialIterator), "ncf": ("NCFModel", "ncf.yaml", SequentialIterator),
          "lgn": ("LGNModel", "lgn.yaml", SequentialIterator), "sasrec": ("SASRecModel", "sasrec.yaml", SequentialIterator),
          # NextItNet: the column iterator (host feeds, or --resident_data) and the literal one (host feeds only; its
          # per-position sampler is a python loop of 0.4 - 0.8 s per batch: --n_train 16384 --regions 3 --epochs 1)
          "nextitnet": ("NextItNetModel", "nextitnet.yaml", NextItNetColumnIterator),
          "nextitnet_literal": ("NextItNetModel", "nextitnet.yaml", NextItNetIterator)}


def _stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "spread": max(xs) - min(xs), "all": xs}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--model", choices=sorted(MODELS), default="clsr")
    ap.add_argument("--resident_data", action="store_true")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=2, help="passes over the file per timed region")
    ap.add_argument("--n_train", type=int, default=65536)
    ap.add_argument("--batch_size", type=int, default=4096)
    ap.add_argument("--data_dir", default=os.path.join(tempfile.gettempdir(), "clsr_fit_tsv"))
    a = ap.parse_args()
    cls_name, yaml_name, it_cls = MODELS[a.model]
    paths = make_tsv_dataset(a.data_dir, n_users=20000, n_items=60000, n_cates=4000, n_train=a.n_train, n_valid=64,
                             n_test=64, max_hist=70)
    kw = dict(user_vocab=paths["user_vocab"], item_vocab=paths["item_vocab"], cate_vocab=paths["category_vocab"],
              max_seq_length=50, batch_size=a.batch_size, train_num_ngs=4, time_unit="s", is_clip_norm=1, embed_l2=1e-6,
              layer_l2=1e-6, show_step=10 ** 9, save_model=False, MODEL_DIR=None, epochs=1)
    if a.model == "clsr":
        kw.update(contrastive_loss="triplet", contrastive_length_threshold=5, discrepancy_loss_weight=0.01,
                  contrastive_loss_weight=0.1)
    hp = prepare_hparams(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "clsr_amd", "config", yaml_name), **kw)
    extra = {"resident_data": True} if a.resident_data else {}
    model = getattr(M, cls_name)(hp, it_cls, seed=0, **extra)
    train = paths["train_data"]
    G = hp.train_num_ngs + 1

    def epoch():
        model.batch_train(model.iterator.load_data_from_file(train, batch_num_ngs=hp.train_num_ngs), model.sess)

    random.seed(0)
    epoch()                                     # parse + pad (+ column upload), workspaces
    epoch()                                     # launch plans recorded
    torch.cuda.synchronize()
    n_batches = sum(1 for f in model.iterator.load_data_from_file(train, batch_num_ngs=hp.train_num_ngs) if f)
    lines = 0
    for f in model.iterator.load_data_from_file(train, batch_num_ngs=hp.train_num_ngs):
        if f:
            lines += int(f["labels"].shape[0]) // G
    fit_rate, fit_ms = [], []
    for _ in range(a.regions):
        t0 = time.perf_counter()
        for _ in range(a.epochs):
            epoch()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        fit_rate.append(a.epochs * lines / dt)
        fit_ms.append(1e3 * dt / (a.epochs * n_batches))
    # the iterator alone (the prefetch thread's work per batch)
    it_ms = []
    for _ in range(a.regions):
        t0 = time.perf_counter()
        feeds = [f for f in model.iterator.load_data_from_file(train, batch_num_ngs=hp.train_num_ngs) if f]
        it_ms.append(1e3 * (time.perf_counter() - t0) / len(feeds))
    full = [f for f in feeds if int(f["labels"].shape[0]) == a.batch_size * G]
    # _to_arrays + _stage alone (main thread, device idle between batches)
    stage_ms = []
    for _ in range(a.regions):
        tot = 0.0
        for f in full:
            t0 = time.perf_counter()
            staged = model._stage(model._to_arrays(f, True))
            tot += time.perf_counter() - t0
            torch.cuda.synchronize()
        stage_ms.append(1e3 * tot / len(full))
    # the step on a resident device feed
    key, dev_feed = staged
    step_ms = []
    with model._stream_ctx():
        for _ in range(3):
            model.net.train_step(dev_feed)
        torch.cuda.synchronize()
        for _ in range(a.regions):
            t0 = time.perf_counter()
            for _ in range(2 * n_batches):
                model.net.train_step(dev_feed)
            torch.cuda.synchronize()
            step_ms.append(1e3 * (time.perf_counter() - t0) / (2 * n_batches))
    out = {"model": a.model, "resident_data": bool(a.resident_data), "batch_size": a.batch_size, "lines_per_epoch": lines,
           "batches_per_epoch": n_batches, "regions": a.regions, "epochs_per_region": a.epochs,
           "fit_interactions_per_s": _stats(fit_rate), "fit_ms_per_step": _stats(fit_ms),
           "iterator_ms_per_batch": _stats(it_ms), "stage_host_ms_per_batch": _stats(stage_ms),
           "resident_input_step_ms": _stats(step_ms),
           "resident_input_interactions_per_s": a.batch_size / (1e-3 * statistics.median(step_ms))}
    if a.resident_data:
        infile, sel, src = full[0].recipe
        rc = model._resident.get(infile, full[0]._cols)
        out["resident_bytes"] = model._resident.nbytes
        build_us = []
        with model._stream_ctx():
            for _ in range(a.regions + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    model.net.build_feed(rc, sel, src, into=dev_feed)
                e1.record()
                e1.synchronize()
                build_us.append(1e3 * e0.elapsed_time(e1) / 20)
        out["build_feed_device_us_per_batch"] = _stats(build_us[1:])     # (recipe copy + check + gather)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
