"""``run_catalogue_eval`` end to end on the golden data: the 40 positives of ``test_data`` ranked against the catalogue of
``train_data`` (993 items; it names every one of the 40 targets with the category its line carries, and one target occurs in
its own fed history -- the test asserts both).  Ranks, ids and score BITS are compared with ``==``: against
tests/rank_oracle.py on logits of host-built compact feeds, between chunk sizes, against ``recommend_k_items`` and ``predict``."""
import copy
import os
import random

import numpy as np
import pytest
import torch

import rank_oracle as KO
import reco_oracle as RO

pytestmark = pytest.mark.gpu

KS = (1, 5, 10)
SIB = dict(user_embedding_dim=16, attention_size=40)
CLASSES = {
    "CLSRModel": ("SASequentialIterator", {}),
    "GRU4RecModel": ("SequentialIterator", dict(SIB, model_type="GRU4Rec")),
    "DINModel": ("SequentialIterator", dict(SIB, model_type="DIN")),
    "DIENModel": ("SequentialIterator", dict(SIB, model_type="DIEN")),
    "A2SVDModel": ("SequentialIterator", dict(SIB, model_type="A2SVD")),
    "SLI_RECModel": ("SequentialIterator", dict(SIB, model_type="sli_rec")),
    "CaserModel": ("SequentialIterator", dict(model_type="Caser", user_embedding_dim=16, L=3, n_v=16, n_h=16, T=1)),
    "SASRecModel": ("SequentialIterator", dict(model_type="SASRec", user_embedding_dim=16, num_blocks=2, num_heads=1)),
    "NCFModel": ("SequentialIterator", dict(model_type="NCF", user_embedding_dim=16, ncf_layer_sizes=[80, 40])),
    "LGNModel": ("SequentialIterator", dict(model_type="LGN", user_embedding_dim=40)),
}


def _path(golden_dir, name):
    return os.path.join(golden_dir, "data", name)


def _model(name, golden_hparams, golden_dir, steps=2, **kw):
    """The class on the golden hparams, ``seed=7``, after ``steps`` training steps (moving statistics off their start)."""
    import clsr_amd.clsr as C
    import clsr_amd.sequential_iterator as I

    it_name, over = CLASSES.get(name, ("NextItNetIterator", dict(model_type="NextItNet", user_embedding_dim=16,
                                                                 dilations=[1, 2, 4], kernel_size=3)))
    hp = copy.deepcopy(golden_hparams)
    for k, v in over.items():
        setattr(hp, k, v)
    model = getattr(C, name)(hp, getattr(I, it_name), seed=7, **kw)
    random.seed(3)
    done = 0
    for feed in model.iterator.load_data_from_file(_path(golden_dir, "train_data"), batch_num_ngs=4):
        if done == steps:
            break
        if feed:
            model.train(model.sess, feed)
            done += 1
    assert done == steps
    return model


@pytest.fixture(scope="module")
def files(golden_dir, tmp_path_factory):
    """``test``: test_data as it is (400 lines, 40 positives); ``positives``: its 40 positive lines; ``negatives``: the other
    360."""
    lines = open(_path(golden_dir, "test_data")).readlines()
    pos = [ln for ln in lines if ln.split("\t")[0] == "1"]
    assert len(lines) == 400 and len(pos) == 40
    d = tmp_path_factory.mktemp("rank_requests")
    out = {"test": _path(golden_dir, "test_data"), "positives": str(d / "positives"), "negatives": str(d / "negatives")}
    with open(out["positives"], "w") as f:
        f.writelines(pos)
    with open(out["negatives"], "w") as f:
        f.writelines(ln for ln in lines if ln.split("\t")[0] != "1")
    return out


def _catalogue(model, golden_dir):
    from clsr_amd.catalogue import Catalogue

    return Catalogue.from_files(model, [_path(golden_dir, "train_data")])


def _host_logits(model, positives, cat, chunk):
    """Of the lines of ``positives`` (one batch): logits [N, M] against the catalogue, the targets' logits [N], ids [N] and the
    fed ``item_history`` rows, from compact feeds built on the HOST with the target in column 0 of every group of ``1 + chunk``
    (``net.upload`` + ``net.forward``).  The target's logit is taken from the first pass and must have the same bits in all."""
    it = model.iterator
    batches = [b for b in it.load_data_from_file(positives, batch_num_ngs=0) if b]
    assert len(batches) == 1
    batch = batches[0]
    hist_keys = ("item_history", "item_cate_history", "mask", "time_from_first_action", "time_to_now")
    base = {k: np.asarray(batch[getattr(it, k)]) for k in hist_keys}
    base["users"] = np.asarray(batch[it.users])
    ti = np.asarray(batch[it.items]).reshape(-1).astype(np.int32)
    tc = np.asarray(batch[it.cates]).reshape(-1).astype(np.int32)
    N, g = base["mask"].shape[0], chunk + 1
    logits = np.zeros((N, len(cat)), dtype=np.float32)
    ts = None
    with model._stream_ctx():
        for c0 in range(0, len(cat), chunk):
            nv = min(chunk, len(cat) - c0)
            gi, gc = np.zeros((N, g), dtype=np.int32), np.zeros((N, g), dtype=np.int32)
            gi[:, 0], gc[:, 0] = ti, tc
            gi[:, 1:1 + nv], gc[:, 1:1 + nv] = cat.items[c0:c0 + nv], cat.cates[c0:c0 + nv]
            feed = dict(base, items=gi.reshape(-1), cates=gc.reshape(-1), labels=np.zeros(N * g, dtype=np.float32), hist_group=g)
            out = model.net.forward(model.net.upload(feed, False), False)["logit"].cpu().numpy().reshape(N, g)
            logits[:, c0:c0 + nv] = out[:, 1:1 + nv]
            if ts is None:
                ts = out[:, 0].copy()
            assert np.array_equal(RO.bits(out[:, 0]), RO.bits(ts)), "the target is re-scored to the same bits with every chunk"
    return logits, ts, ti, tc, base["item_history"]


def _same(a, b):
    return (torch.equal(a.users, b.users) and torch.equal(a.items, b.items) and torch.equal(a.ranks, b.ranks)
            and torch.equal(a.scores.view(torch.int32), b.scores.view(torch.int32)))


def _seen(hist):
    return [set(r.tolist()) for r in hist]


def _close(got, want):
    """The dicts agree: integers and hit rates (sums of ones over N) exactly, the float64 means of 40 terms to 1e-12 relative --
    the product sums pairwise in numpy, the oracle term by term, each within 40 roundings of 1.1e-16."""
    assert list(got) == list(want)
    for k in got:
        if isinstance(want[k], int) or k.startswith("hit@"):
            assert got[k] == want[k] and type(got[k]) is type(want[k]), k
        else:
            assert isinstance(got[k], float) and got[k] == pytest.approx(want[k], rel=1e-12, abs=0), k


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_every_class_equals_the_oracle_and_the_recommendations(name, golden_hparams, golden_dir, files):
    model = _model(name, golden_hparams, golden_dir)
    cat = _catalogue(model, golden_dir)
    M = len(cat)
    res, got = model.run_catalogue_eval(files["test"], cat, ks=KS, chunk=64, return_ranks=True)
    assert [t.dtype for t in got] == [torch.int32, torch.int32, torch.float32, torch.int32]
    assert all(tuple(t.shape) == (40,) and not t.is_cuda for t in got)
    logits, ts, ti, tc, hist = _host_logits(model, files["positives"], cat, 64)
    # what the module's docstring says of the data
    col = np.searchsorted(cat.items, ti)
    assert np.array_equal(cat.items[col], ti) and np.array_equal(cat.cates[col], tc)
    in_hist = np.array([int(t) in s for t, s in zip(ti, _seen(hist))])
    assert int(in_hist.sum()) == 1
    # the oracle
    want = KO.ranks(logits, cat.items, ts, ti, seen=_seen(hist))
    assert np.array_equal(got.ranks.numpy(), want)
    assert np.array_equal(got.items.numpy(), ti)
    assert np.array_equal(RO.bits(got.scores.numpy()), RO.bits(ts)) and np.isfinite(ts).all()
    assert np.array_equal(RO.bits(logits[np.arange(40), col]), RO.bits(ts)), "the target's own column is scored like column 0"
    _close(res, KO.metrics(want, KS, candidates=M))
    assert res["requests"] == 40 and res["candidates"] == M == 993
    # whatever the chunk
    for chunk in (17, 63, None):
        res2, got2 = model.run_catalogue_eval(files["test"], cat, ks=KS, chunk=chunk, return_ranks=True)
        assert _same(got2, got) and res2 == res, chunk
    assert model.run_catalogue_eval(files["positives"], cat, ks=KS) == res      # the label-0 lines are ignored
    # against recommend_k_items: rank <= K exactly when the target is entry rank - 1 of the request's row
    left_out = 0
    for K in (5, 256):
        reco = model.recommend_k_items(files["positives"], cat, top_k=K)
        assert torch.equal(reco.users, got.users)
        inside = 0
        for n in range(40):
            if in_hist[n]:
                left_out += 1       # (recommend_k_items drops the seen target; the rank never drops it)
                continue
            row, r = reco.items[n].tolist(), int(want[n])
            assert (r <= K) == (int(ti[n]) in row), (K, n)
            if r <= K:
                inside += 1
                assert row.index(int(ti[n])) == r - 1
                assert RO.bits(reco.scores[n, r - 1].numpy()) == RO.bits(ts[n] + np.float32(0.0))
        assert K == 5 or inside > 0
    assert left_out == 2            # one request, at each of the two depths


@pytest.mark.parametrize("name", ["CLSRModel", "GRU4RecModel"])
def test_scores_are_the_logits_predict_squashes(name, golden_hparams, golden_dir, files, tmp_path):
    model = _model(name, golden_hparams, golden_dir)
    cat = _catalogue(model, golden_dir)
    _, got = model.run_catalogue_eval(files["test"], cat, chunk=64, return_ranks=True)
    out = str(tmp_path / "pred")
    model.iterator.batch_size = 40      # a batch of predict: four groups of one history and ten lines (a group above 8)
    model.predict(files["test"], out)
    pred = np.asarray([np.float32(x) for x in open(out).read().split()], dtype=np.float32)
    labels = np.asarray([ln.split("\t")[0] == "1" for ln in open(files["test"])])
    assert pred.shape == (400,) and labels.sum() == 40
    with model._stream_ctx():
        squashed = torch.sigmoid(got.scores.to(model.net.device)).cpu().numpy()      # (where predict squashes)
    assert np.array_equal(RO.bits(pred[labels]), RO.bits(squashed))


def test_remove_seen_off_differs_where_the_oracle_says(golden_hparams, golden_dir, files):
    model = _model("CLSRModel", golden_hparams, golden_dir)
    cat = _catalogue(model, golden_dir)
    logits, ts, ti, _, hist = _host_logits(model, files["positives"], cat, 64)
    want_on = KO.ranks(logits, cat.items, ts, ti, seen=_seen(hist))
    want_off = KO.ranks(logits, cat.items, ts, ti)
    assert (want_on != want_off).any() and (want_on <= want_off).all()
    res_on, on = model.run_catalogue_eval(files["test"], cat, ks=KS, return_ranks=True)
    res_off, off = model.run_catalogue_eval(files["test"], cat, ks=KS, remove_seen=False, return_ranks=True)
    assert np.array_equal(on.ranks.numpy(), want_on) and np.array_equal(off.ranks.numpy(), want_off)
    assert torch.equal(on.scores.view(torch.int32), off.scores.view(torch.int32)) and torch.equal(on.items, off.items)
    _close(res_off, KO.metrics(want_off, KS, candidates=len(cat)))
    assert res_on != res_off


def test_refusals_name_the_argument(golden_hparams, golden_dir, files):
    from clsr_amd.ops import query

    model = _model("GRU4RecModel", golden_hparams, golden_dir, steps=0)
    cat = _catalogue(model, golden_dir)
    for bad in ((0,), (1, 2.5), (), (-3, 1), 5, (True,)):
        with pytest.raises(ValueError, match="^ks must be"):
            model.run_catalogue_eval(files["test"], cat, ks=bad)
    res = model.run_catalogue_eval(files["test"], cat, ks=(3, 100000))      # no upper limit: a rank is exact at any depth
    assert res["hit@100000"] == 1.0 and 0.0 <= res["hit@3"] <= 1.0 and res["ndcg@100000"] >= res["ndcg@3"]
    for bad in (0, query("clsr_reco_max_chunk")):
        with pytest.raises(ValueError, match="^chunk must lie in 1 .. 3839"):
            model.run_catalogue_eval(files["test"], cat, chunk=bad)
    with pytest.raises(ValueError, match="^infile .*negatives.* no kept line with label 1"):
        model.run_catalogue_eval(files["negatives"], cat)
    nin = _model("NextItNetModel", golden_hparams, golden_dir, steps=0)
    with pytest.raises(NotImplementedError, match="NextItNetModel.run_catalogue_eval"):
        nin.run_catalogue_eval(files["test"], cat)


def test_a_call_has_no_side_effects(golden_hparams, golden_dir, files):
    model = _model("CLSRModel", golden_hparams, golden_dir)
    twin = _model("CLSRModel", golden_hparams, golden_dir)
    cat = _catalogue(model, golden_dir)
    valid = _path(golden_dir, "valid_data")
    before_eval = model.run_eval(valid, 4)
    before = model.net.state_dict()
    model.run_catalogue_eval(files["test"], cat, chunk=64)
    model.run_catalogue_eval(files["test"], cat)
    after = model.net.state_dict()
    assert list(before) == list(after) and all(torch.equal(before[k], after[k]) for k in before)
    assert model.run_eval(valid, 4) == before_eval
    # ... and the next training step is the one a model that never ranked takes
    for m in (model, twin):
        random.seed(11)
        feed = next(f for f in m.iterator.load_data_from_file(_path(golden_dir, "train_data"), batch_num_ngs=4) if f)
        m.train(m.sess, feed)
    a, b = model.net.state_dict(), twin.net.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
