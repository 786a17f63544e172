"""GPU parity of LGN (clsr_amd/seqnet.py kind "lgn", clsr_amd/lgn.py, csrc/lgn.hip) against its torch-CPU oracle
(tests/lgn_oracle.py, float64, autograd) on the committed golden batches and the reference's own graph of the golden data,
with the checks and tolerances of tests/test_ncf_gpu.py: logits, the loss terms, every dense and table gradient, the
three table clip norms (user_embedding and item_embedding: the whole dense gradient; cate_embedding: the un-deduplicated
slices of its two lookups), the Adam / LazyAdam step with the clip on and off -- plus what is LGN's own: cate rows outside
set(item2cate) | involved unchanged to the bit under LazyAdam, eval scores that fail on a stale F cache, and a step on a
synthetic graph whose longest user and item rows run through the split path.  tests/test_lgn_cpu.py holds that the fixture
leaves no pre-activation undecidable on either graph, before or after the step."""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lgn_cases as K  # noqa: E402
import lgn_oracle as O  # noqa: E402
from clsr_amd.seqnet import SeqNet  # noqa: E402


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
    print("%s: max abs err %.3e, max |exp| %.3e" % (name, float(err.max()), float(exp.abs().max())))
    assert excess <= 0, "%s: max abs err %.3e, max |exp| %.3e" % (name, float(err.max()), float(exp.abs().max()))


_A = {}


def _graph(which, dims):
    """(graph, dense float64 adjacency, dims of the case): computed once and left unchanged."""
    if which not in _A:
        d = dims if which == "golden" else K.skewed_dims(dims)
        g = K.golden_model_graph() if which == "golden" else K.skewed_model_graph(**d)
        _A[which] = (g, O.dense_adjacency(g.indptr, g.indices, g.values), d)
    return _A[which]


def _setup(hp, dims, dedup, which="golden"):
    graph, A, d = _graph(which, dims)
    params32 = O.init_params(d, hp, **O.FIXTURE)
    net = SeqNet(hp, d, kind="lgn", device="cuda:0", seed=0, dedup_histories=dedup, graph=graph)
    net.load_state_dict(dict(params32), strict=True)
    return net, type(params32)((k, v.double()) for k, v in params32.items()), graph, A


def _check_step(net, params, graph, A, hp, feed, optimizer, dedup):
    tf = O.to_torch_feed(feed, dtype=torch.float64)
    new_p, _, ls, grads, norms, out = O.train_step(params, O.init_adam(params), 1, tf, hp, A, graph.item2cate,
                                                   lazy=optimizer == "lazyadam")
    net.capture_grads = True
    got = net.train_step(net.upload(feed, True))
    torch.cuda.synchronize()
    B, T, G, Hn = net.last_shape
    assert Hn * G == B and (G > 1) == dedup
    _close(got["logit"], out["logit"], 1e-4, 1e-4, "logit")
    gl = net.read_losses()
    for k in ("loss", "data_loss", "regular_loss"):
        _close([gl[k]], [float(ls[k])], 1e-5, 1e-7, k)
    cap, raw = net.captured, out["raw_grads"]
    assert list(net.dense_names) == O.dense_names()
    assert set(net.dense_names) | set(O.TABLES.values()) == set(raw)
    floor = 4e-6 * max(float(raw[n].abs().max()) for n in net.dense_names)
    for i, name in enumerate(net.dense_names):
        scale = float(raw[name].abs().max()) + 1e-12
        _close(cap["dense"][name], raw[name], 2e-3, 2e-4 * scale + floor, "grad " + name)
        _close([float(cap["dense_sumsq"][i]) ** 0.5], [norms[name]], 1e-3, 20 * floor, "norm " + name)
    ss = cap["table_sumsq"].cpu().numpy()
    assert not ss[2:5].any() and not ss[7:].any()
    tab_norm = dict(user=ss[6] ** 0.5, item=ss[0] ** 0.5, cate=(ss[1] + ss[5]) ** 0.5)
    _close([ss[1] ** 0.5], [out["cate_slice_norms"]["cate/lookup"]], 1e-3, 1e-7, "cate item2cate-slices norm")
    _close([ss[5] ** 0.5], [out["cate_slice_norms"]["cate/involved"]], 1e-4, 1e-12, "cate involved-slice norm")
    for key, name in O.TABLES.items():
        scale = float(raw[name].abs().max()) + 1e-12
        _close(cap["tables"][key], raw[name], 2e-3, 2e-4 * scale + floor, "grad " + name)
        _close([tab_norm[key]], [norms[name]], 1e-3, 1e-7, "clip norm " + name)
    sd = net.state_dict()
    lr = hp.learning_rate
    for name in list(net.dense_names) + list(O.TABLES.values()):
        g_ = grads[name].double().reshape(-1)
        sel = g_.abs() > 100 * floor
        upd_got = (sd[name].double().reshape(-1) - params[name].reshape(-1))[sel]
        upd_exp = (new_p[name].reshape(-1) - params[name].reshape(-1))[sel]
        assert upd_exp.numel()
        _close(upd_got, upd_exp, 5e-3, 0.02 * lr, "adam update " + name)
    # cate rows outside set(item2cate) | involved: no gradient; unchanged to the bit (dense Adam: zero moments; LazyAdam: not visited)
    name = O.TABLES["cate"]
    rows = torch.ones(params[name].shape[0], dtype=torch.bool)
    rows[out["touched"][name]] = False
    assert torch.equal(sd[name][rows].double(), params[name][rows]), name
    return rows


@pytest.mark.parametrize("clip", [1, 0])
@pytest.mark.parametrize("optimizer", ["adam", "lazyadam"])
@pytest.mark.parametrize("dedup", [True, False])
def test_train_step_matches_oracle(golden_dir, golden_hparams, dedup, optimizer, clip):
    hp = O.hparams(golden_hparams, optimizer=optimizer, is_clip_norm=clip)
    feed = _feed(golden_dir, "iterator_train_plain.npz", b=0)
    net, params, graph, A = _setup(hp, _dims(hp), dedup)
    _check_step(net, params, graph, A, hp, feed, optimizer, dedup)


def test_regulariser_through_the_graph_weighs_in(golden_dir, golden_hparams):
    """embed_l2 four orders above the golden value: the regulariser's gradient -- through both layers for F's item rows, the
    usual term for the raw category rows -- is then a visible share of every table gradient and of the cate norms."""
    hp = O.hparams(golden_hparams, embed_l2=1e-2, layer_l2=1e-2)
    feed = _feed(golden_dir, "iterator_train_plain.npz", b=0)
    net, params, graph, A = _setup(hp, _dims(hp), True)
    _check_step(net, params, graph, A, hp, feed, "adam", True)


def test_untouched_cate_rows_keep_their_bits_under_lazyadam(golden_dir, golden_hparams):
    """A category table with four rows past the vocabulary: neither item2cate nor the feed names them, so they lie outside
    set(item2cate) | involved.  Two LazyAdam steps leave them and their moments alone, to the bit."""
    hp = O.hparams(golden_hparams, optimizer="lazyadam")
    dims = _dims(hp)
    graph = _graph("golden", dims)[0]
    feed = _feed(golden_dir, "iterator_train_plain.npz", b=0)
    spare = list(range(dims["Vc"], dims["Vc"] + 4))       # four more categories than the vocabulary: nobody names them
    dims = dict(dims, Vc=dims["Vc"] + 4)
    g2 = graph
    params32 = O.init_params(dims, hp, **O.FIXTURE)
    net = SeqNet(hp, dims, kind="lgn", device="cuda:0", seed=0, graph=g2)
    net.load_state_dict(dict(params32), strict=True)
    f = net.upload(feed, True)
    net.train_step(f)
    before = net.state_dict()
    net.train_step(f)
    torch.cuda.synchronize()
    after = net.state_dict()
    name = O.TABLES["cate"]
    assert torch.equal(before[name][spare], params32[name][spare].to(before[name].device)) and torch.equal(after[name][spare], before[name][spare])
    moved = [c for c in range(dims["Vc"]) if c not in spare]
    assert not torch.equal(after[name][moved], before[name][moved])
    for k in after:
        if k.startswith("__adam__/") and name in k and after[k].dim() == 2:
            assert float(after[k][spare].abs().max()) == 0.0, k


def test_step_on_a_graph_with_split_rows(golden_dir, golden_hparams):
    """``graph=`` takes a synthetic graph: user row 3 and item row 5 hold more than 2 L entries, so the split path runs
    inside a real step, forward and (transposed) backward."""
    hp = O.hparams(golden_hparams)
    feed = _feed(golden_dir, "iterator_train_plain.npz", b=0)
    net, params, graph, A = _setup(hp, _dims(hp), True, which="skewed")
    assert net.lg_prop.fwd.nlong >= 2 and net.lg_prop.bwd.nlong >= 2
    _check_step(net, params, graph, A, hp, feed, "adam", True)


def test_two_steps_are_bit_identical(golden_dir, golden_hparams):
    hp = O.hparams(golden_hparams)
    feed = _feed(golden_dir, "iterator_train_plain.npz", b=1)
    runs = []
    for _ in range(2):
        net, _, _, _ = _setup(hp, _dims(hp), True)
        net.capture_grads = True
        net.train_step(net.upload(feed, True))
        torch.cuda.synchronize()
        runs.append((net.state_dict(), net.captured))
    (sd_a, cap_a), (sd_b, cap_b) = runs
    assert set(sd_a) == set(sd_b) and any(k.startswith("__adam__/") for k in sd_a)
    for k in sd_a:       # tables, dense parameters, Adam moments
        assert torch.equal(sd_a[k], sd_b[k]), k
    assert torch.equal(cap_a["dense_sumsq"], cap_b["dense_sumsq"])
    assert torch.equal(cap_a["table_sumsq"], cap_b["table_sumsq"]) and float(cap_a["table_sumsq"][6]) > 0
    for k in cap_a["dense"]:
        assert torch.equal(cap_a["dense"][k], cap_b["dense"][k]), k
    for k in cap_a["tables"]:
        assert torch.equal(cap_a["tables"][k], cap_b["tables"][k]), k


def test_eval_scores_match_oracle_and_follow_the_parameters(golden_dir, golden_hparams):
    hp = O.hparams(golden_hparams)
    net, params, graph, A = _setup(hp, _dims(hp), True)
    feed_t = _feed(golden_dir, "iterator_train_plain.npz", b=0)
    feed = _feed(golden_dir, "iterator_eval_plain.npz", b=0)
    tfe = O.to_torch_feed(feed, dtype=torch.float64)
    new_p = O.train_step(params, O.init_adam(params), 1, O.to_torch_feed(feed_t, dtype=torch.float64), hp, A, graph.item2cate)[0]
    exp0, exp1 = O.predict(params, tfe, hp, A, graph.item2cate), O.predict(new_p, tfe, hp, A, graph.item2cate)
    assert float((exp1["logit"] - exp0["logit"]).abs().max()) > 1e-3        # (the step moves the scores: a stale F shows)
    fe = net.upload(feed, False)
    for _ in range(3):      # (eager, recorded, replayed: the same scores)
        got = net.forward(fe, False)
        torch.cuda.synchronize()
        _close(got["logit"], exp0["logit"], 1e-4, 1e-4, "logit before the step")
    net.train_step(net.upload(feed_t, True))
    for _ in range(3):
        got = net.forward(fe, False)
        torch.cuda.synchronize()
        _close(got["logit"], exp1["logit"], 1e-4, 1e-4, "logit after the step")
        _close(torch.sigmoid(got["logit"]), exp1["pred"], 2e-3, 2e-4, "pred after the step")
    # load_state_dict: back to the first parameters, the cache follows
    net.load_state_dict({k: v.float() for k, v in params.items()}, strict=False)
    got = net.forward(fe, False)
    torch.cuda.synchronize()
    _close(got["logit"], exp0["logit"], 1e-4, 1e-4, "logit after load_state_dict")


def test_model_api_roundtrip(golden_dir, golden_hparams, tmp_path):
    """LGNModel through the shared API: the graph built from train_data, fit one epoch, every requested metric, one score per
    line, a checkpoint of exactly the reference's variable names into a fresh model with identical scores; dist= is refused."""
    from clsr_amd.clsr import LGNModel
    from clsr_amd.sequential_iterator import SequentialIterator

    d = os.path.join(golden_dir, "data")
    hp = O.hparams(golden_hparams, epochs=1, MODEL_DIR=str(tmp_path / "model") + "/")
    before = sorted(os.listdir(d))
    model = LGNModel(hp, SequentialIterator, seed=7)
    z = np.load(os.path.join(golden_dir, "lgn_graph.npz"))
    assert np.array_equal(model.net.lg_prop.fwd.indices.cpu().numpy(), z["indices"])
    assert model.fit(os.path.join(d, "train_data"), os.path.join(d, "valid_data"), valid_num_ngs=4, eval_metric="auc") is model
    res = model.run_weighted_eval(os.path.join(d, "test_data"), 9)
    want = {"auc", "logloss", "mean_mrr", "ndcg@2", "ndcg@4", "ndcg@6", "hit@2", "hit@4", "hit@6", "wauc"}
    assert want <= set(res) and all(np.isfinite(float(v)) for v in res.values()), res
    names = {n for n in model.net.state_dict() if not n.startswith("__")}
    assert names == {n for n, _, _ in O.param_specs(_dims(hp), hp)}
    ckpt = str(tmp_path / "ckpt" / "lgn")
    os.makedirs(os.path.dirname(ckpt))
    model.save_model(ckpt)
    fresh = LGNModel(copy.deepcopy(hp), SequentialIterator, seed=123)
    a0 = tmp_path / "pred_0.txt"
    fresh.predict(os.path.join(d, "test_data"), str(a0))        # (fills the fresh model's F cache with ITS parameters)
    fresh.load_model(ckpt)
    a, b = tmp_path / "pred_a.txt", tmp_path / "pred_b.txt"
    model.predict(os.path.join(d, "test_data"), str(a))
    fresh.predict(os.path.join(d, "test_data"), str(b))
    assert a.read_text() == b.read_text() and a.read_text() != a0.read_text()
    assert len(a.read_text().split()) == sum(1 for _ in open(os.path.join(d, "test_data")))
    assert sorted(os.listdir(d)) == before                      # nothing written beside the data
    with pytest.raises(NotImplementedError, match="dist"):
        LGNModel(hp, SequentialIterator, dist=object())
