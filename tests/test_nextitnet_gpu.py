"""GPU parity of NextItNet (clsr_amd/seqnet.py kind "nextitnet", csrc/nextitnet.hip) against its torch-CPU oracle
(tests/nextitnet_oracle.py, float64, autograd), with the checks and tolerances of tests/test_caser_gpu.py: logits, loss
terms, every dense and table gradient with the reference's clip norms, the (Lazy)Adam step, the BN moving statistics -- at
nextitnet.yaml's widths with histories of 1, 50, 25, 33 and 12 real steps, for 1, 4 and 15 negatives, with the
deterministic gradient path on and off, clip on and off; at 20 000 and 205 000 logit rows (every ``parts`` cap of the
logit-MLP path is crossed); evaluation on the last position; the model API on the golden data."""
import copy
import os
import pickle
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nextitnet_cases as K  # noqa: E402
import nextitnet_oracle as O  # noqa: E402
from clsr_amd.params import SIB_TABLES  # noqa: E402
from clsr_amd.seqnet import SeqNet  # noqa: E402

YAML = dict(max_seq_length=50, item_embedding_dim=32, cate_embedding_dim=8, dilations=[1, 2, 4, 1, 2, 4], kernel_size=3,
            layer_sizes=[100, 64])
DIMS = dict(Vu=8, Vi=60, Vc=9)


def _dims(hp):
    return dict(Vu=len(pickle.load(open(hp.user_vocab, "rb"))), Vi=len(pickle.load(open(hp.item_vocab, "rb"))),
                Vc=len(pickle.load(open(hp.cate_vocab, "rb"))))


def _feed(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name))
    return {k[3:]: g[k] for k in g.files if k.startswith("b0_")}


def _close(got, exp, rtol, atol, name):
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    exp = torch.as_tensor(exp).detach().double().cpu().reshape(-1)
    assert got.shape == exp.shape, (name, got.shape, exp.shape)
    err = (got - exp).abs()
    excess = float((err - (atol + rtol * exp.abs())).max())
    assert excess <= 0, "%s: max abs err %.3e, max |exp| %.3e" % (name, float(err.max()), float(exp.abs().max()))


def _setup(hp, dims, det=True):
    params32 = O.init_params(dims, hp, **O.FIXTURE)
    net = SeqNet(hp, dims, kind="nextitnet", device="cuda:0", seed=0)
    net.det_grads = det
    sd = dict(params32)
    sd.update(O.init_bn_state(params32))
    net.load_state_dict(sd, strict=True)
    params64 = type(params32)((k, v.double()) for k, v in params32.items())
    return net, params64


def _step_matches_oracle(hp, dims, feed, det=True, updates=True):
    net, params = _setup(hp, dims, det)
    tf = O.to_torch_feed(feed, dtype=torch.float64)
    bn, adam = O.init_bn_state(params), O.init_adam(params)
    lazy = str(hp.optimizer).lower() == "lazyadam"
    new_p, new_bn, _, ls, grads, norms, out = O.train_step(params, bn, adam, 1, tf, hp, lazy=lazy)
    net.capture_grads = True
    got = net.train_step(net.upload(feed, True))
    torch.cuda.synchronize()
    R, T, G, Hn = net.last_shape
    assert G == hp.train_num_ngs + 1 and R == Hn * T * G == out["logit"].numel()
    _close(got["logit"], out["logit"], 1e-4, 1e-4, "logit")
    _close(got["model_output"], out["model_output"], 1e-4, 1e-5, "model_output")
    gl = net.read_losses()
    for k in ("loss", "data_loss", "regular_loss"):
        _close([gl[k]], [float(ls[k])], 1e-5, 1e-7, k)
    cap, raw = net.captured, out["raw_grads"]
    floor = 4e-6 * max(float(raw[n].abs().max()) for n in net.dense_names)
    assert set(net.dense_names) | set(SIB_TABLES.values()) == set(raw)
    for i, name in enumerate(net.dense_names):
        scale = float(raw[name].abs().max()) + 1e-12
        _close(cap["dense"][name], raw[name], 2e-3, 2e-4 * scale + floor, "grad " + name)
        _close([float(cap["dense_sumsq"][i]) ** 0.5], [norms[name]], 1e-3, 20 * floor, "norm " + name)
    ss = cap["table_sumsq"].cpu().numpy()
    tab_norm = dict(item=(ss[0] + ss[2] + ss[4]) ** 0.5, cate=(ss[1] + ss[3] + ss[5]) ** 0.5)
    for key, name in SIB_TABLES.items():
        scale = float(raw[name].abs().max()) + 1e-12
        _close(cap["tables"][key], raw[name], 2e-3, 2e-4 * scale + floor, "grad " + name)
        # the norm of the un-merged slices: Hn T history rows, Hn T G target rows, the involved rows
        _close([tab_norm[key]], [norms[name]], 1e-3, 1e-7, "clip norm " + name)
    # the padded steps' gradient reaches table row 0 (no mask enters NextItNet's graph)
    assert float(raw[SIB_TABLES["item"]][0].abs().max()) > 0 and float(cap["tables"]["item"][0].abs().max()) > 0
    if not updates:
        return net, out
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


@pytest.mark.parametrize("ngs,optimizer,clip,det", [(4, "adam", 1, True), (4, "lazyadam", 1, True), (4, "adam", 0, True),
                                                    (4, "adam", 1, False), (4, "lazyadam", 0, False), (1, "adam", 1, True),
                                                    (15, "adam", 1, True)])
def test_train_step_matches_oracle(golden_hparams, ngs, optimizer, clip, det):
    hp = O.hparams(golden_hparams, train_num_ngs=ngs, optimizer=optimizer, is_clip_norm=clip, **YAML)
    feed = K.edge_feed(50, ngs + 1, DIMS["Vi"], DIMS["Vc"], K.STEP_LENS, seed=3)
    _step_matches_oracle(hp, DIMS, feed, det)


def test_train_step_on_the_golden_batch(golden_dir, golden_hparams):
    hp = O.hparams(golden_hparams)
    _step_matches_oracle(hp, _dims(hp), _feed(golden_dir, "iterator_train_nextitnet.npz"))


def test_twenty_thousand_rows(golden_hparams):
    """Hn = 80 at nextitnet.yaml's shape: 20 000 logit rows."""
    hp = O.hparams(golden_hparams, **YAML)
    lens = [1 + (7 * i) % 50 for i in range(80)]
    net, out = _step_matches_oracle(hp, DIMS, K.edge_feed(50, 5, DIMS["Vi"], DIMS["Vc"], lens, seed=5), updates=False)
    assert net.last_shape[0] == 20000


def test_two_hundred_thousand_rows(golden_hparams):
    """Hn = 820, T = 50, G = 5 with narrow tables and a narrow logit MLP: 205 000 rows, past every ``parts`` cap of the
    logit-MLP, batch-norm and softmax path."""
    from clsr_amd.ops import query

    hp = O.hparams(golden_hparams, max_seq_length=50, item_embedding_dim=4, cate_embedding_dim=4, dilations=[1, 2],
                   kernel_size=3, layer_sizes=[8, 4])
    dims = dict(Vu=8, Vi=300, Vc=20)
    lens = [1 + (7 * i) % 50 for i in range(820)]
    net, out = _step_matches_oracle(hp, dims, K.edge_feed(50, 5, dims["Vi"], dims["Vc"], lens, seed=6), updates=False)
    R = net.last_shape[0]
    assert R == 205000
    # the caps the row count crosses
    assert query("clsr_pgemm_stats_parts", R) == query("clsr_pgemm_stats_parts", 1 << 30)
    assert query("clsr_mlp_out_bwd_parts", R, 64) == query("clsr_mlp_out_bwd_parts", 1 << 30, 64)


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
    # squared norms of the un-summed slices of the four lookup sites (history and target rows of both tables); slots 4, 5
    # are the shared trunk's regulariser norms, which tests/test_det_grads_gpu.py leaves out for every model
    assert torch.equal(cap_a["table_sumsq"][:4], cap_b["table_sumsq"][:4]) and float(cap_a["table_sumsq"][2]) > 0
    for k in cap_a["dense"]:
        assert torch.equal(cap_a["dense"][k], cap_b["dense"][k]), k
    for k in cap_a["tables"]:
        assert torch.equal(cap_a["tables"][k], cap_b["tables"][k]), k


def test_eval_scores_the_last_position(golden_dir, golden_hparams):
    """model_output of a scoring feed is x_L[:, T - 1] ++ target, held at the forward tolerances on the fixture's
    parameters; after one training step (whose Adam update the step test holds to 0.02 lr) the scores, as
    tests/test_caser_gpu.py compares them."""
    hp = O.hparams(golden_hparams)
    net, params = _setup(hp, _dims(hp))
    bn = O.init_bn_state(params)
    feed = _feed(golden_dir, "iterator_eval_nextitnet.npz")
    tf = O.to_torch_feed(feed, dtype=torch.float64)
    exp = O.predict(params, bn, tf, hp)
    got = net.forward(net.upload(feed, False), False)
    torch.cuda.synchronize()
    assert got["logit"].numel() == feed["items"].shape[0] == exp["logit"].numel()
    D = hp.item_embedding_dim + hp.cate_embedding_dim
    _close(got["model_output"][:, :D], exp["xL"][:, -1], 1e-4, 1e-5, "x_L at the last position")
    _close(got["model_output"], exp["model_output"], 1e-4, 1e-5, "model_output")
    _close(got["logit"], exp["logit"], 1e-4, 1e-4, "logit")
    # an earlier position would show: the oracle's x_L differs there
    assert float((exp["xL"][:, -1] - exp["xL"][:, -2]).abs().max()) > 1e-2
    feed_t = _feed(golden_dir, "iterator_train_nextitnet.npz")
    new_p, new_bn = O.train_step(params, bn, O.init_adam(params), 1, O.to_torch_feed(feed_t, dtype=torch.float64), hp)[:2]
    net.train_step(net.upload(feed_t, True))
    exp = O.predict(new_p, new_bn, tf, hp)
    got = net.forward(net.upload(feed, False), False)
    torch.cuda.synchronize()
    _close(torch.sigmoid(got["logit"]), exp["pred"], 2e-3, 2e-4, "pred")


def test_scoring_with_shared_histories(golden_dir, golden_hparams):
    """An evaluation file holds runs of lines with ONE history: the compact feed (``hist_group``) computes a history's
    stack once and writes its last position to every line of the group -- the scores of the expanded feed, to the bit."""
    hp = O.hparams(golden_hparams)
    dims = _dims(hp)
    net, _ = _setup(hp, dims)
    feed, g, n = _feed(golden_dir, "iterator_eval_nextitnet.npz"), 3, 20
    rng = np.random.RandomState(4)
    full = {k: np.repeat(v[:n], g, axis=0) for k, v in feed.items()}
    full["items"] = rng.randint(1, dims["Vi"], (n * g, 1)).astype(np.int32)
    full["cates"] = rng.randint(1, dims["Vc"], (n * g, 1)).astype(np.int32)
    a = net.forward(net.upload(full, False), False)["logit"].clone()
    assert net.last_shape == (n * g, 10, 1, n * g)
    hist_keys = ("users", "item_history", "item_cate_history", "mask", "time_from_first_action", "time_to_now")
    compact = dict(full, hist_group=g, **{k: np.ascontiguousarray(full[k][::g]) for k in hist_keys})
    b = net.forward(net.upload(compact, False), False)["logit"].clone()
    torch.cuda.synchronize()
    assert net.last_shape == (n * g, 10, g, n)
    assert torch.equal(a, b) and float(a.std()) > 0


def test_keys_the_graph_never_reads_take_any_value(golden_dir, golden_hparams):
    """hidden_size, attention_size and att_fcn_layer_sizes are never read by NextItNet's graph: a net built with odd values
    of all three has the same variables and gives the same step and the same scores, to the bit."""
    dims = _dims(O.hparams(golden_hparams))
    feed_t, feed_e = _feed(golden_dir, "iterator_train_nextitnet.npz"), _feed(golden_dir, "iterator_eval_nextitnet.npz")
    got = []
    for kw in ({}, dict(hidden_size=7, attention_size=3, att_fcn_layer_sizes=[5]),
               dict(hidden_size=None, attention_size=None, att_fcn_layer_sizes=None)):
        net, _ = _setup(O.hparams(golden_hparams, **kw), dims)
        net.train_step(net.upload(feed_t, True))
        logit = net.forward(net.upload(feed_e, False), False)["logit"].clone()
        torch.cuda.synchronize()
        got.append((list(net.state_dict()), net.read_losses()["loss"], logit))
    for names, loss, logit in got[1:]:
        assert names == got[0][0] and loss == got[0][1] and torch.equal(logit, got[0][2])


def test_refusals_on_the_device_path(golden_dir, golden_hparams):
    hp = O.hparams(golden_hparams)
    net, _ = _setup(hp, _dims(hp))
    feed = _feed(golden_dir, "iterator_train_nextitnet.npz")
    flat = dict(feed, items=feed["items"][:, -1], cates=feed["cates"][:, -1], labels=feed["labels"][:, -1])
    with pytest.raises(ValueError, match="NextItNetIterator"):
        net.train_step(net.upload(flat, True))
    short = {k: (v[:, 2:] if v.ndim == 2 else v) for k, v in feed.items()}
    with pytest.raises(ValueError, match="max_seq_length = 10"):
        net.train_step(net.upload(short, True))
    ragged = {k: v[:-1] for k, v in feed.items()}
    with pytest.raises(ValueError, match="multiple of"):
        net.train_step(net.upload(ragged, True))
    net.train_step(net.upload(feed, True))       # (and the net still steps)
    torch.cuda.synchronize()
    assert np.isfinite(net.read_losses()["loss"])


def test_model_api(golden_dir, golden_hparams, tmp_path):
    """NextItNetModel through the shared API: a few steps on one batch lower its loss, fit one epoch, every requested
    metric, a checkpoint into a fresh model with identical scores, a state_dict of exactly the reference's names."""
    from clsr_amd.clsr import NextItNetModel
    from clsr_amd.sequential_iterator import NextItNetIterator

    d = os.path.join(golden_dir, "data")
    hp = O.hparams(golden_hparams, epochs=1, MODEL_DIR=str(tmp_path / "model") + "/")
    model = NextItNetModel(hp, NextItNetIterator, seed=7)
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
    ckpt = str(tmp_path / "ckpt" / "nextitnet")
    os.makedirs(os.path.dirname(ckpt))
    model.save_model(ckpt)
    fresh = NextItNetModel(copy.deepcopy(hp), NextItNetIterator, seed=123)
    fresh.load_model(ckpt)
    a, b = tmp_path / "pred_a.txt", tmp_path / "pred_b.txt"
    model.predict(os.path.join(d, "test_data"), str(a))
    fresh.predict(os.path.join(d, "test_data"), str(b))
    assert a.read_text() == b.read_text() and len(a.read_text().split()) == sum(1 for _ in open(os.path.join(d, "test_data")))
