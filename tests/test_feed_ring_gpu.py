"""The pinned ring behind ``build_feed`` and ``upload`` (``clsr_amd.feeds.PinnedRing``): more calls than the ring has
slots, queued without a synchronisation in between, each with other data; a slot rewritten while a queued transfer still
reads it, or a recipe buffer let go of too early, shows as a stale byte in the arena.  The device arena of a feed passed
back through ``into=`` never moves.  Arenas are compared over every byte of every tensor; the bytes that pad a piece to 16
are never written by a builder and belong to no tensor."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CALLS = 7       # twice the ring plus one


def _same_bytes(got, want, lay):
    """``got``: a clone of an arena, ``want``: an arena, both of layout ``lay``."""
    return all(torch.equal(got[o:o + nb], want[o:o + nb]) for o, nb in lay.values())


def _a2svd(golden_hparams, **kw):
    """(The iterator draws 4 negatives from the other lines of a batch and drops a batch of fewer than 5 lines: it is
    asked for 8.  The builder test writes its own recipes of 4 and 5 lines.)"""
    from test_resident_feed_gpu import _hp, _model

    return _model("A2SVDModel", "SequentialIterator", _hp(golden_hparams, "A2SVDModel", batch_size=8), **kw)


def test_build_feed_through_a_growing_ring(golden_dir, golden_hparams):
    from clsr_amd.feeds import PinnedRing
    from clsr_amd.resident import check_recipe

    assert CALLS == 2 * PinnedRing._STAGE_SLOTS + 1
    model = _a2svd(golden_hparams, resident_data=True)
    net, G = model.net, model.net.G_train
    path = os.path.join(golden_dir, "data", "train_data")
    random.seed(2)
    first = next(f for f in model.iterator.load_data_from_file(path, batch_num_ngs=4) if f)
    rc = model._resident.get(first.recipe[0], first._cols)
    rng = np.random.default_rng(4)
    recipes = []
    for i in range(CALLS):
        n_sel = 4 + i % 2           # the recipe buffer grows at the second call
        sel = rng.integers(0, rc.N, n_sel).astype(np.int32)
        src = rng.integers(0, n_sel, (n_sel, G)).astype(np.int32)
        src[:, 0] = np.arange(n_sel)
        assert check_recipe(sel, src, rc.N, G) == n_sel
        recipes.append((sel, src))
    assert len({sel.tobytes() for sel, _ in recipes}) == CALLS
    with model._stream_ctx():
        f, got, ptrs = None, [], set()
        for sel, src in recipes:
            f = net.build_feed(rc, sel, src, h0=0, n=4, into=f)
            got.append(f["_arena"].dev.clone())
            ptrs.add(f["_arena"].dev.data_ptr())
        torch.cuda.synchronize()
        assert len(ptrs) == 1, "the arena of a feed passed back through into= moved"
        assert f["_rbuf"].ring.nbytes >= 16 + (4 * 5 * G + 15) // 16 * 16
        for i, (sel, src) in enumerate(recipes):
            want = net.build_feed(rc, sel, src, h0=0, n=4)
            torch.cuda.synchronize()
            assert want["_arena"].dev.data_ptr() not in ptrs
            assert want["_arena"].lay == f["_arena"].lay
            assert _same_bytes(got[i], want["_arena"].dev, f["_arena"].lay), i
    model.check_resident()


def test_upload_through_the_ring(golden_dir, golden_hparams):
    model = _a2svd(golden_hparams)
    net = model.net
    path = os.path.join(golden_dir, "data", "train_data")
    random.seed(2)
    feeds = []
    for fb in model.iterator.load_data_from_file(path, batch_num_ngs=4):
        if fb and len(feeds) < CALLS:
            feeds.append(model._to_arrays(fb, True))
    assert len(feeds) == CALLS
    assert len({np.asarray(a["items"]).tobytes() + np.asarray(a["item_history"]).tobytes() for a in feeds}) == CALLS
    with model._stream_ctx():
        f, got, ptrs = None, [], set()
        for a in feeds:
            f = net.upload(a, True, into=f)
            got.append(f["_arena"].dev.clone())
            ptrs.add(f["_arena"].dev.data_ptr())
        torch.cuda.synchronize()
        assert len(ptrs) == 1, "the arena of a feed passed back through into= moved"
        for i, a in enumerate(feeds):
            want = net.upload(a, True)
            torch.cuda.synchronize()
            assert want["B"] == f["B"] and want["_arena"].lay == f["_arena"].lay
            assert _same_bytes(got[i], want["_arena"].dev, f["_arena"].lay), i
