"""The resident feed path end to end (``resident_data=True``): device feeds gathered from the resident column store are
the feeds ``upload`` makes from the host iterator's batches, tensor for tensor; a step and a whole ``fit`` from either
give bit-identical state; the iterator consumes the ``random`` stream alike on both paths."""
import copy
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TENSORS = ("users", "items", "cates", "item_history", "item_cate_history", "time_from_first_action", "time_to_now",
           "labels", "seq_len", "denom")
T = 10


@pytest.fixture(scope="module")
def train_file(golden_dir, tmp_path_factory):
    """The golden training TSV plus three lines whose histories are longer than T, exactly T and shorter: 603 lines."""
    src = os.path.join(golden_dir, "data", "train_data")
    lines = [l for l in open(src).read().split("\n") if l]
    w = lines[0].split("\t")
    hist = [x.split(",") for x in w[5:8]]
    extra = []
    for k in (T + 3, T, 2):
        cols = [",".join((h * (k // len(h) + 1))[:k]) for h in hist]
        extra.append("\t".join(w[:5] + cols))
    path = str(tmp_path_factory.mktemp("resident") / "train_data")
    with open(path, "w") as f:
        f.write("\n".join(lines + extra) + "\n")
    full = [len(l.split("\t")[5].split(",")) for l in lines + extra]
    assert any(n > T for n in full) and any(n == T for n in full) and any(n < T for n in full)
    assert len(full) == 603
    return path


def _hp(golden_hparams, model, **kw):
    from clsr_amd.deeprec_utils import prepare_hparams

    if model == "CLSRModel":
        hp = copy.deepcopy(golden_hparams)
    elif model == "NCFModel":
        hp = copy.deepcopy(golden_hparams)
        for k, v in dict(model_type="NCF", user_embedding_dim=16, ncf_layer_sizes=[80, 40]).items():
            setattr(hp, k, v)
    else:
        g = golden_hparams
        hp = prepare_hparams(os.path.join(ROOT, "clsr_amd", "config", "asvd.yaml"), user_vocab=g.user_vocab,
                             item_vocab=g.item_vocab, cate_vocab=g.cate_vocab, max_seq_length=T, batch_size=64,
                             train_num_ngs=4, time_unit="s", is_clip_norm=1, embed_l2=1e-6, layer_l2=1e-6,
                             learning_rate=0.005, show_step=10 ** 9, save_model=False, MODEL_DIR=None, SUMMARIES_DIR=None,
                             write_tfevents=False, epochs=2, EARLY_STOP=5, pairwise_metrics=g.pairwise_metrics,
                             weighted_metrics=g.weighted_metrics)
    hp.show_step = 10 ** 9
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def _model(name, it_name, hp, **kw):
    import clsr_amd.clsr as M
    import clsr_amd.sequential_iterator as I

    return getattr(M, name)(hp, getattr(I, it_name), seed=11, **kw)


def _same_feed(a, b, what):
    for k in ("B", "T", "compact", "G"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    for k in TENSORS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (what, k)


@pytest.mark.parametrize("name,it_name,dedup", [
    ("CLSRModel", "SASequentialIterator", True), ("CLSRModel", "SASequentialIterator", False),
    ("CLSRModel", "SequentialIterator", True), ("A2SVDModel", "SequentialIterator", True),
    ("A2SVDModel", "SequentialIterator", False), ("A2SVDModel", "SASequentialIterator", True)])
def test_device_feed_equals_the_uploaded_host_feed(name, it_name, dedup, golden_hparams, train_file):
    """Two passes (the shuffle is cumulative) from one seed; 64 lines a batch: a last batch of 27; 150: a last batch of 3,
    which the iterator drops.  Whole batches through the model's staging, and the shards of 2 and 3 ranks."""
    from clsr_amd.dp import shard_feed
    from clsr_amd.resident import check_recipe

    for bs in (64, 150):
        hp = _hp(golden_hparams, name, batch_size=bs)
        host = _model(name, it_name, hp, dedup_histories=dedup)
        res = _model(name, it_name, hp, dedup_histories=dedup, resident_data=True)
        net, G = res.net, hp.train_num_ngs + 1
        states, seen, dropped, sizes = [], 0, 0, set()
        for model in (host, res):
            random.seed(5)
            feeds = []
            for _ in range(2):
                feeds.append(list(model.iterator.load_data_from_file(train_file, batch_num_ngs=4, min_seq_length=1)))
                states.append(random.getstate())
            model._feeds = feeds
        assert states[0] == states[2] and states[1] == states[3], "the random stream after each pass"
        for pa, pb in zip(host._feeds, res._feeds):
            assert len(pa) == len(pb)
            for fa, fb in zip(pa, pb):
                assert (fa is None) == (fb is None)
                if fa is None:
                    dropped += 1
                    continue
                arrays = res._to_arrays(fb, True)
                assert set(arrays) == {"_recipe", "_cols"}
                with res._stream_ctx():
                    _, f = res._stage(arrays)
                    want = net.upload(host._to_arrays(fa, True), True)
                    torch.cuda.synchronize()
                    n = f["B"] // G
                    sizes.add(n)
                    _same_feed(f, want, (bs, seen))
                    if seen % 4 == 0 or n == 27:      # (64 = 3 * 21 + 1 and 27 = 2 * 13 + 1: truncated remainders)
                        infile, sel, src = fb.recipe
                        rc = res._resident.get(infile, fb._cols)
                        check_recipe(sel, src, rc.N, G)
                        for world in (2, 3):
                            for rank in range(world):
                                per = n // world
                                got = net.build_feed(rc, sel, src, rank * per, per)
                                want = net.upload(shard_feed(host._to_arrays(fa, True), rank, world, G), True)
                                torch.cuda.synchronize()
                                _same_feed(got, want, (bs, seen, world, rank))
                seen += 1
        res.check_resident()
        assert res._resident.uploads == 1 and res._resident.nbytes == 603 * (16 * T + 16)
        if bs == 64:
            assert sizes == {64, 27} and dropped == 0 and seen == 20
        else:
            assert sizes == {150} and dropped == 2 and seen == 8


@pytest.mark.parametrize("name,it_name", [("CLSRModel", "SASequentialIterator"), ("A2SVDModel", "SequentialIterator"),
                                          ("NCFModel", "SequentialIterator")])
def test_one_step_from_either_feed_gives_bit_identical_state(name, it_name, golden_hparams, train_file):
    """Parameters, batch-norm statistics and optimiser moments after one step."""
    (_, a), (_, b) = _one_step_each_way(name, it_name, golden_hparams, train_file)
    assert set(a) == set(b) and len(a) > 4
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("name,it_name", [("CLSRModel", "SASequentialIterator"), ("A2SVDModel", "SequentialIterator"),
                                          ("NCFModel", "SequentialIterator")])
def test_one_step_from_either_feed_gives_bit_identical_losses(name, it_name, golden_hparams, train_file):
    """The loss terms ``train`` returns, compared exactly.

    KNOWN TO MISS for CLSR, on either path against ITSELF: the step adds the per-workgroup shares of the regulariser and
    the discrepancy loss into their reported scalars with double-precision atomics, in arrival order.  Measured on an
    MI355X, one CLSR step from the same state and batch, sixteen runs: regular_loss 0.000653581346808891 in eleven runs
    and 0.0006535813468088909 in five (one unit in the last place), with the flag off (2 of 8) and on (3 of 8) alike; in
    an earlier run discrepancy_loss -1.5907591114448466e-06 against -1.5907591114448468e-06.  The scalars are reported
    only, nothing reads them back: parameters and moments are exact (the test above).  Every other term was equal in
    every run.  In three runs of this file the CLSR case held once and missed twice (once in
    regular_loss, 0.0006536078723520997 against ...998, once in discrepancy_loss); the A2SVD and NCF cases held."""
    (la, _), (lb, _) = _one_step_each_way(name, it_name, golden_hparams, train_file)
    print("losses, flag off:", [repr(x) for x in la], "flag on:", [repr(x) for x in lb])
    assert la == lb, (la, lb)


def _one_step_each_way(name, it_name, golden_hparams, train_file):
    hp = _hp(golden_hparams, name)
    out = []
    for flag in (False, True):
        model = _model(name, it_name, hp, resident_data=flag)
        random.seed(3)
        feed = next(f for f in model.iterator.load_data_from_file(train_file, batch_num_ngs=4) if f)
        losses = model.train(model.sess, feed)
        with model._stream_ctx():
            torch.cuda.synchronize()
            sd = {k: v.detach().cpu().clone() for k, v in model.net.state_dict().items()}
        if flag:
            assert ("resident", 64, T, True, 5) in model._static and len(model._static) == 1
        out.append((losses, sd))
    return out


@pytest.mark.parametrize("name,it_name,graph", [("CLSRModel", "SASequentialIterator", False),
                                                ("A2SVDModel", "SequentialIterator", False),
                                                ("CLSRModel", "SASequentialIterator", True)])
def test_fit_with_resident_data_is_bit_identical(name, it_name, graph, golden_dir, golden_hparams, train_file):
    """Two epochs of fit with the flag on and off: the same state_dict, the same validation metrics; also under
    ``use_graph=True`` (the builder runs outside the captured step)."""
    valid = os.path.join(golden_dir, "data", "valid_data")
    hp = _hp(golden_hparams, name, epochs=2)
    out = []
    for flag in (False, True):
        model = _model(name, it_name, hp, resident_data=flag, use_graph=graph)
        random.seed(9)
        model.fit(train_file, valid, valid_num_ngs=4, eval_metric="wauc")
        res = model.run_weighted_eval(valid, num_ngs=4)
        with model._stream_ctx():
            torch.cuda.synchronize()
            sd = {k: v.detach().cpu().clone() for k, v in model.net.state_dict().items()}
        out.append((res, sd, random.getstate()))
        if flag:
            assert model._resident.uploads == 1 and any("resident" in k for k in model._static)
        else:
            assert model._resident is None
    (ra, a, sa), (rb, b, sb) = out
    assert ra == rb, (ra, rb)
    assert sa == sb
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_a_reparsed_file_is_uploaded_again(golden_hparams, train_file):
    hp = _hp(golden_hparams, "A2SVDModel")
    model = _model("A2SVDModel", "SequentialIterator", hp, resident_data=True)
    it = model.iterator
    random.seed(1)
    feed = next(f for f in it.load_data_from_file(train_file, batch_num_ngs=4) if f)
    model.train(model.sess, feed)
    first = model._resident.files[train_file]
    it.iter_data.pop(train_file)                # the iterator parses the file again
    feed = next(f for f in it.load_data_from_file(train_file, batch_num_ngs=4) if f)
    model.train(model.sess, feed)
    assert model._resident.uploads == 2 and model._resident.files[train_file] is not first
    # a feed without a recipe (a plain dict, as a caller may build one) takes the host path
    model.train(model.sess, dict(feed))
    assert any(k[0] != "resident" for k in model._static if k[0] != "2x")


def test_nextitnet_refuses_resident_data(golden_hparams):
    from clsr_amd.clsr import NextItNetModel
    from clsr_amd.deeprec_utils import prepare_hparams
    from clsr_amd.sequential_iterator import NextItNetIterator

    g = golden_hparams
    hp = prepare_hparams(os.path.join(ROOT, "clsr_amd", "config", "nextitnet.yaml"), user_vocab=g.user_vocab,
                         item_vocab=g.item_vocab, cate_vocab=g.cate_vocab, max_seq_length=T, batch_size=64,
                         train_num_ngs=4, time_unit="s")
    with pytest.raises(NotImplementedError, match="NextItNetIterator"):
        NextItNetModel(hp, NextItNetIterator, seed=1, resident_data=True)
