"""GPU parity of SASRec (clsr_amd/seqnet.py kind "sasrec", csrc/sasrec.hip) against its torch-CPU oracle
(tests/sasrec_oracle.py, float64, autograd), with the checks and tolerances of tests/test_nextitnet_gpu.py /
tests/test_ncf_gpu.py, unchanged: logits, loss terms, every dense and table gradient with the reference's clip norms, the
(Lazy)Adam step, the BN moving statistics -- at sasrec.yaml's widths with histories of 1, 50, 25, 33 and 12 real steps, for
1, 4 and 15 negatives, with the deterministic gradient path on and off, clip on and off, compact and replicated feeds;
bit-identical steps; evaluation with shared histories; the model API on the golden data; ``resident_data`` (also under
``use_graph``) and ``resident_eval`` against the host path."""
import copy
import os
import pickle
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sasrec_cases as K  # noqa: E402
import sasrec_oracle as O  # noqa: E402
from clsr_amd.params import SIB_TABLES  # noqa: E402
from clsr_amd.seqnet import SeqNet  # noqa: E402

YAML = dict(max_seq_length=50, item_embedding_dim=32, cate_embedding_dim=8, num_blocks=2, num_heads=1, layer_sizes=[100, 64])
DIMS = dict(Vu=8, Vi=60, Vc=9)


def _dims(hp):
    return dict(Vu=len(pickle.load(open(hp.user_vocab, "rb"))), Vi=len(pickle.load(open(hp.item_vocab, "rb"))),
                Vc=len(pickle.load(open(hp.cate_vocab, "rb"))))


def _feed(golden_dir, name, b=0):
    g = np.load(os.path.join(golden_dir, name))
    pre = "b%d_" % b
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}


def _close(got, exp, rtol, atol, name):
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    exp = torch.as_tensor(exp).detach().double().cpu().reshape(-1)
    assert got.shape == exp.shape, (name, got.shape, exp.shape)
    err = (got - exp).abs()
    excess = float((err - (atol + rtol * exp.abs())).max())
    assert excess <= 0, "%s: max abs err %.3e, max |exp| %.3e" % (name, float(err.max()), float(exp.abs().max()))


def _setup(hp, dims, det=True, dedup=True):
    params32 = O.init_params(dims, hp, **O.FIXTURE)
    net = SeqNet(hp, dims, kind="sasrec", device="cuda:0", seed=0, dedup_histories=dedup)
    net.det_grads = det
    sd = dict(params32)
    sd.update(O.init_bn_state(params32))
    net.load_state_dict(sd, strict=True)
    params64 = type(params32)((k, v.double()) for k, v in params32.items())
    return net, params64


def _step_matches_oracle(hp, dims, feed, det=True, dedup=True):
    net, params = _setup(hp, dims, det, dedup)
    tf = O.to_torch_feed(feed, dtype=torch.float64)
    bn, adam = O.init_bn_state(params), O.init_adam(params)
    lazy = str(hp.optimizer).lower() == "lazyadam"
    Gt = hp.train_num_ngs + 1
    new_p, new_bn, _, ls, grads, norms, out = O.train_step(params, bn, adam, 1, tf, hp, lazy=lazy,
                                                          dedup_group=Gt if dedup else None)
    net.capture_grads = True
    got = net.train_step(net.upload(feed, True))
    torch.cuda.synchronize()
    B, T, G, Hn = net.last_shape
    assert G == (Gt if dedup else 1) and B == Hn * G == out["logit"].numel()
    _close(got["logit"], out["logit"], 1e-4, 1e-4, "logit")
    _close(got["model_output"], out["model_output"], 1e-4, 1e-5, "model_output")
    gl = net.read_losses()
    for k in ("loss", "data_loss", "regular_loss"):
        _close([gl[k]], [float(ls[k])], 1e-5, 1e-7, k)
    cap, raw = net.captured, out["raw_grads"]
    floor = 4e-6 * max(float(raw[n].abs().max()) for n in net.dense_names)
    assert set(net.dense_names) | set(SIB_TABLES.values()) == set(raw)
    assert set(O.encoder_names(int(hp.num_blocks))) <= set(net.dense_names)
    for i, name in enumerate(net.dense_names):
        scale = float(raw[name].abs().max()) + 1e-12
        _close(cap["dense"][name], raw[name], 2e-3, 2e-4 * scale + floor, "grad " + name)
        _close([float(cap["dense_sumsq"][i]) ** 0.5], [norms[name]], 1e-3, 20 * floor, "norm " + name)
    ss = cap["table_sumsq"].cpu().numpy()
    tab_norm = dict(item=(ss[0] + ss[2] + ss[4]) ** 0.5, cate=(ss[1] + ss[3] + ss[5]) ** 0.5)
    for key, name in SIB_TABLES.items():
        scale = float(raw[name].abs().max()) + 1e-12
        _close(cap["tables"][key], raw[name], 2e-3, 2e-4 * scale + floor, "grad " + name)
        _close([tab_norm[key]], [norms[name]], 1e-3, 1e-7, "clip norm " + name)
    # the rows of pos past the longest history of the batch: no data gradient, the regulariser's alone
    longest = int(tf["mask"].sum(1).max())
    if longest < T:
        exp = float(hp.layer_l2) * params[O.POS][longest:]
        assert torch.equal(cap["dense"][O.POS][longest:].cpu().double(), exp.float().double()) or \
            float((cap["dense"][O.POS][longest:].cpu().double() - exp).abs().max()) <= 1e-7 * float(exp.abs().max())
    sd = net.state_dict()
    lr = hp.learning_rate
    for name in list(net.dense_names) + list(SIB_TABLES.values()):
        g_ = grads[name].double().reshape(-1)
        sel = g_.abs() > 100 * floor
        upd_got = (sd[name].double().reshape(-1) - params[name].reshape(-1))[sel]
        upd_exp = (new_p[name].reshape(-1) - params[name].reshape(-1))[sel]
        if upd_exp.numel():
            _close(upd_got, upd_exp, 5e-3, 0.02 * lr, "adam update " + name)
    for k, v in new_bn.items():
        _close(sd[k], v, 1e-4, 1e-6, k)
    assert torch.equal(sd["sequential/embedding/user_embedding"].double(), params["sequential/embedding/user_embedding"])
    return net, out


@pytest.mark.parametrize("ngs,optimizer,clip,det,dedup", [
    (4, "adam", 1, True, True), (4, "lazyadam", 1, True, True), (4, "adam", 0, True, True), (4, "adam", 1, False, True),
    (4, "lazyadam", 0, False, False), (4, "adam", 1, True, False), (1, "adam", 1, True, True), (15, "adam", 1, True, True)])
def test_train_step_matches_oracle(golden_hparams, ngs, optimizer, clip, det, dedup):
    hp = O.hparams(golden_hparams, train_num_ngs=ngs, optimizer=optimizer, is_clip_norm=clip, **YAML)
    feed = K.edge_feed(50, ngs + 1, DIMS["Vi"], DIMS["Vc"], K.STEP_LENS, seed=3)
    _step_matches_oracle(hp, DIMS, feed, det, dedup)


@pytest.mark.parametrize("heads,blocks", [(2, 1), (10, 4)])
def test_train_step_on_the_golden_batch(golden_dir, golden_hparams, heads, blocks):
    hp = O.hparams(golden_hparams, num_heads=heads, num_blocks=blocks)
    _step_matches_oracle(hp, _dims(hp), _feed(golden_dir, "iterator_train_sa.npz", b=1))


def test_two_steps_are_bit_identical(golden_hparams):
    hp = O.hparams(golden_hparams, **YAML)
    feed = K.edge_feed(50, 5, DIMS["Vi"], DIMS["Vc"], K.STEP_LENS, seed=3)
    runs = []
    for _ in range(2):
        net, _ = _setup(hp, DIMS)
        net.capture_grads = True
        net.train_step(net.upload(feed, True))
        torch.cuda.synchronize()
        runs.append((net.state_dict(), net.captured))
    (sd_a, cap_a), (sd_b, cap_b) = runs
    assert set(sd_a) == set(sd_b) and any(k.startswith("__adam__/") for k in sd_a)
    for k in sd_a:       # tables, dense parameters, BN statistics, Adam moments
        assert torch.equal(sd_a[k], sd_b[k]), k
    assert torch.equal(cap_a["dense_sumsq"], cap_b["dense_sumsq"])
    assert torch.equal(cap_a["table_sumsq"][:4], cap_b["table_sumsq"][:4]) and float(cap_a["table_sumsq"][2]) > 0
    for k in cap_a["dense"]:
        assert torch.equal(cap_a["dense"][k], cap_b["dense"][k]), k
    for k in cap_a["tables"]:
        assert torch.equal(cap_a["tables"][k], cap_b["tables"][k]), k


def test_eval_scores_match_oracle(golden_dir, golden_hparams):
    hp = O.hparams(golden_hparams)
    net, params = _setup(hp, _dims(hp))
    bn = O.init_bn_state(params)
    feed = _feed(golden_dir, "iterator_eval_sa.npz")
    tf = O.to_torch_feed(feed, dtype=torch.float64)
    exp = O.predict(params, bn, tf, hp)
    got = net.forward(net.upload(feed, False), False)
    torch.cuda.synchronize()
    D = hp.item_embedding_dim + hp.cate_embedding_dim
    _close(got["model_output"][:, :D], exp["s"], 1e-4, 1e-5, "s")
    _close(got["model_output"], exp["model_output"], 1e-4, 1e-5, "model_output")
    _close(got["logit"], exp["logit"], 1e-4, 1e-4, "logit")
    feed_t = _feed(golden_dir, "iterator_train_sa.npz")
    new_p, new_bn = O.train_step(params, bn, O.init_adam(params), 1, O.to_torch_feed(feed_t, dtype=torch.float64), hp)[:2]
    net.train_step(net.upload(feed_t, True))
    exp = O.predict(new_p, new_bn, tf, hp)
    got = net.forward(net.upload(feed, False), False)
    torch.cuda.synchronize()
    _close(torch.sigmoid(got["logit"]), exp["pred"], 2e-3, 2e-4, "pred")


def test_scoring_with_shared_histories(golden_dir, golden_hparams):
    """An evaluation file holds runs of lines with ONE history: the compact feed (``hist_group``) runs a history's encoder
    once and writes s to every line of the group -- the scores of the expanded feed, to the bit."""
    hp = O.hparams(golden_hparams)
    dims = _dims(hp)
    net, _ = _setup(hp, dims)
    feed, g, n = _feed(golden_dir, "iterator_eval_sa.npz"), 3, 20
    rng = np.random.RandomState(4)
    full = {k: np.repeat(v[:n], g, axis=0) for k, v in feed.items()}
    full["items"] = rng.randint(1, dims["Vi"], full["items"].shape).astype(np.int32)
    full["cates"] = rng.randint(1, dims["Vc"], full["cates"].shape).astype(np.int32)
    a = net.forward(net.upload(full, False), False)["logit"].clone()
    assert net.last_shape == (n * g, 10, 1, n * g)
    hist_keys = ("users", "item_history", "item_cate_history", "mask", "time_from_first_action", "time_to_now")
    compact = dict(full, hist_group=g, **{k: np.ascontiguousarray(full[k][::g]) for k in hist_keys})
    b = net.forward(net.upload(compact, False), False)["logit"].clone()
    torch.cuda.synchronize()
    assert net.last_shape == (n * g, 10, g, n)
    assert torch.equal(a, b) and float(a.std()) > 0


def test_keys_the_graph_never_reads_take_any_value(golden_dir, golden_hparams):
    dims = _dims(O.hparams(golden_hparams))
    feed_t, feed_e = _feed(golden_dir, "iterator_train_sa.npz"), _feed(golden_dir, "iterator_eval_sa.npz")
    got = []
    for kw in ({}, dict(hidden_size=7, attention_size=3, att_fcn_layer_sizes=[5], attention_dropout=0.5),
               dict(hidden_size=None, attention_size=None, att_fcn_layer_sizes=None)):
        net, _ = _setup(O.hparams(golden_hparams, **kw), dims)
        net.train_step(net.upload(feed_t, True))
        logit = net.forward(net.upload(feed_e, False), False)["logit"].clone()
        torch.cuda.synchronize()
        got.append((list(net.state_dict()), net.read_losses()["loss"], logit))
    for names, loss, logit in got[1:]:
        assert names == got[0][0] and loss == got[0][1] and torch.equal(logit, got[0][2])


def _model(hp, **kw):
    from clsr_amd.clsr import SASRecModel
    from clsr_amd.sequential_iterator import SequentialIterator

    return SASRecModel(copy.deepcopy(hp), SequentialIterator, seed=7, **kw)


def test_model_api(golden_dir, golden_hparams, tmp_path):
    """SASRecModel through the shared API: a few steps on one batch lower its loss, fit one epoch, every requested metric,
    a checkpoint into a fresh model with identical scores, a state_dict of exactly the listed names."""
    d = os.path.join(golden_dir, "data")
    hp = O.hparams(golden_hparams, epochs=1, MODEL_DIR=str(tmp_path / "model") + "/")
    model = _model(hp)
    random.seed(5)
    batch = next(f for f in model.iterator.load_data_from_file(os.path.join(d, "train_data"), batch_num_ngs=4) if f)
    data_loss = [model.train(None, batch)[3] for _ in range(6)]
    assert all(np.isfinite(data_loss)) and data_loss[-1] < data_loss[0], data_loss
    assert model.fit(os.path.join(d, "train_data"), os.path.join(d, "valid_data"), valid_num_ngs=4,
                     eval_metric="auc") is model
    res = model.run_weighted_eval(os.path.join(d, "test_data"), 9)
    want = {"auc", "logloss", "mean_mrr", "ndcg@2", "ndcg@4", "ndcg@6", "hit@2", "hit@4", "hit@6", "wauc"}
    assert want <= set(res) and all(np.isfinite(float(v)) for v in res.values()), res
    names = {n for n in model.net.state_dict() if not n.startswith("__") and "moving_" not in n}
    assert names == {n for n, _, _ in O.param_specs(_dims(hp), hp)}
    moving = {n for n in model.net.state_dict() if "moving_" in n}
    assert moving and all(n.startswith("sequential/logit_fcn/") for n in moving)      # (the layer norms have none)
    ckpt = str(tmp_path / "ckpt" / "sasrec")
    os.makedirs(os.path.dirname(ckpt))
    model.save_model(ckpt)
    fresh = _model(hp)
    fresh.seed = 123
    fresh.load_model(ckpt)
    a, b = tmp_path / "pred_a.txt", tmp_path / "pred_b.txt"
    model.predict(os.path.join(d, "test_data"), str(a))
    fresh.predict(os.path.join(d, "test_data"), str(b))
    assert a.read_text() == b.read_text() and len(a.read_text().split()) == sum(1 for _ in open(os.path.join(d, "test_data")))


def test_captured_step_is_bit_identical_to_the_eager_step(golden_dir, golden_hparams):
    """``use_graph=True``: the first step of a batch shape runs eagerly and is captured, the later ones replay the graph --
    after every one of six steps on the golden batches the state_dict is the eager model's, to the bit.  (A whole ``fit``
    under ``use_graph`` does not end in the eager fit's bits for any sibling model, GRU4Rec included: that is the trunk's
    pipeline, and the reason the resident test below pairs two captured fits.)"""
    hp = O.hparams(golden_hparams, save_model=False, show_step=10 ** 9, write_tfevents=False)
    runs = []
    for graph in (False, True):
        model = _model(hp, use_graph=graph)
        random.seed(9)
        feeds = (f for f in model.iterator.load_data_from_file(os.path.join(golden_dir, "data", "train_data"),
                                                               batch_num_ngs=4) if f)
        sds = []
        for _ in range(6):
            model.train(model.sess, next(feeds))
            with model._stream_ctx():
                torch.cuda.synchronize()
                sds.append({k: v.detach().cpu().clone() for k, v in model.net.state_dict().items()})
        runs.append(sds)
        assert len(model._graphs) == (1 if graph else 0)
    for i, (a, b) in enumerate(zip(*runs)):
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (i, k)
    assert not torch.equal(runs[0][0][O.POS], runs[0][5][O.POS])


def _short_fit(golden_dir, hp, **kw):
    d = os.path.join(golden_dir, "data")
    model = _model(hp, **kw)
    random.seed(9)
    model.fit(os.path.join(d, "train_data"), os.path.join(d, "valid_data"), valid_num_ngs=4, eval_metric="auc")
    res = model.run_weighted_eval(os.path.join(d, "valid_data"), num_ngs=4)
    with model._stream_ctx():
        torch.cuda.synchronize()
        sd = {k: v.detach().cpu().clone() for k, v in model.net.state_dict().items()}
    return model, res, sd


@pytest.mark.parametrize("flag,graph", [("resident_data", False), ("resident_eval", False), ("resident_data", True)])
def test_fit_is_bit_identical_with_the_flag(golden_dir, golden_hparams, flag, graph):
    """One epoch of fit on the golden data with the flag on ends in the state_dict and the metric dict of the host path:
    the iterator is SequentialIterator, so the resident stores serve SASRec without code of its own.  ``graph``: both fits
    under ``use_graph=True`` (the step captured once per batch shape and replayed), as tests/test_resident_feed_gpu.py pairs
    them for CLSR."""
    hp = O.hparams(golden_hparams, epochs=1, save_model=False, show_step=10 ** 9, write_tfevents=False)
    first, res_a, a = _short_fit(golden_dir, hp, use_graph=graph)
    model, res_b, b = _short_fit(golden_dir, hp, use_graph=graph, **{flag: True})
    if graph:
        assert len(first._graphs) >= 2 and len(model._graphs) >= 2       # (the full batches and the ragged last one)
        assert all(np.isfinite(float(v)) for v in res_a.values()) and all(bool(torch.isfinite(v).all()) for v in a.values()
                                                                            if v.is_floating_point())
    if flag == "resident_data":
        assert model._resident is not None and model._resident.uploads == 1
    if flag == "resident_eval":
        assert model._resident_eval is not None and model._resident_eval.uploads >= 1
    assert res_a == res_b, (res_a, res_b)
    assert set(a) == set(b) and any(k.startswith(O.SCOPE) for k in a)
    for k in a:
        assert torch.equal(a[k], b[k]), k
