"""GPU parity of NCF (clsr_amd/seqnet.py kind "ncf", csrc/ncf.hip) against its torch-CPU oracle (tests/ncf_oracle.py,
float64, autograd) on the committed golden batches: the checks and tolerances of tests/test_siblings_gpu.py /
tests/test_caser_gpu.py -- logits, the loss terms, every dense and table gradient with the reference's clip norms, the
Adam / LazyAdam step -- plus what is NCF's own: the trunk's item / cate tables move by the regulariser only, user_embedding
not at all.  tests/test_ncf_cpu.py holds that the fixture leaves no tower unit undecidable on these batches."""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ncf_oracle as O  # noqa: E402
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
    assert excess <= 0, "%s: max abs err %.3e, max |exp| %.3e" % (name, float(err.max()), float(exp.abs().max()))


def _setup(hp, dims, dedup):
    params32 = O.init_params(dims, hp, **O.FIXTURE)
    net = SeqNet(hp, dims, kind="ncf", device="cuda:0", seed=0, dedup_histories=dedup)
    net.load_state_dict(dict(params32), strict=True)
    return net, type(params32)((k, v.double()) for k, v in params32.items())


@pytest.mark.parametrize("clip", [1, 0])
@pytest.mark.parametrize("optimizer", ["adam", "lazyadam"])
@pytest.mark.parametrize("dedup", [True, False])
def test_train_step_matches_oracle(golden_dir, golden_hparams, dedup, optimizer, clip):
    hp = O.hparams(golden_hparams, optimizer=optimizer, is_clip_norm=clip)
    dims = _dims(hp)
    feed = _feed(golden_dir, "iterator_train_plain.npz", b=0)
    net, params = _setup(hp, dims, dedup)
    tf = O.to_torch_feed(feed, dtype=torch.float64)
    new_p, _, ls, grads, norms, out = O.train_step(params, O.init_adam(params), 1, tf, hp, lazy=optimizer == "lazyadam")
    net.capture_grads = True
    got = net.train_step(net.upload(feed, True))
    torch.cuda.synchronize()
    B, T, G, Hn = net.last_shape
    assert Hn * G == B and (G > 1) == dedup
    _close(got["logit"], out["logit"], 1e-4, 1e-4, "logit")
    _close(got["model_output"], out["model_output"], 1e-4, 1e-5, "model_output")
    gl = net.read_losses()
    for k in ("loss", "data_loss", "regular_loss"):
        _close([gl[k]], [float(ls[k])], 1e-5, 1e-7, k)
    cap, raw = net.captured, out["raw_grads"]
    assert list(net.dense_names) == O.dense_names(hp)
    assert set(net.dense_names) | set(O.TABLES.values()) == set(raw)
    floor = 4e-6 * max(float(raw[n].abs().max()) for n in net.dense_names)
    for i, name in enumerate(net.dense_names):
        scale = float(raw[name].abs().max()) + 1e-12
        _close(cap["dense"][name], raw[name], 2e-3, 2e-4 * scale + floor, "grad " + name)
        _close([float(cap["dense_sumsq"][i]) ** 0.5], [norms[name]], 1e-3, 20 * floor, "norm " + name)
    ss = cap["table_sumsq"].cpu().numpy()
    assert not ss[:4].any() and not ss[10:].any()        # no data gradient reaches item / cate: their site slots stay zero
    tab_norm = dict(item=ss[4] ** 0.5, cate=ss[5] ** 0.5, user_gmf=ss[6] ** 0.5, user_mlp=ss[7] ** 0.5,
                    item_gmf=ss[8] ** 0.5, item_mlp=ss[9] ** 0.5)
    for key, name in O.TABLES.items():
        scale = float(raw[name].abs().max()) + 1e-12
        if key in O.NCF_KEYS:
            _close(cap["tables"][key], raw[name], 2e-3, 2e-4 * scale + floor, "grad " + name)
            # the norm of the B un-merged slices, duplicate ids not summed first
            _close([tab_norm[key]], [norms[name]], 1e-3, 1e-7, "clip norm " + name)
        else:
            # the regulariser only: embed_l2 * row on the involved rows, nothing elsewhere -- held tightly, the gradient is
            # far below the floor of the data gradients
            _close(cap["tables"][key], raw[name], 1e-5, 1e-6 * scale, "regulariser grad " + name)
            assert float(raw[name].abs().max()) > 0
            _close([tab_norm[key]], [norms[name]], 1e-4, 1e-12, "clip norm " + name)
    sd = net.state_dict()
    lr = hp.learning_rate
    for name in list(net.dense_names) + list(O.TABLES.values()):
        g_ = grads[name].double().reshape(-1)
        sel = g_.abs() > (100 * floor if name in net.dense_names or name.split("/")[-1][:-10] in O.NCF_KEYS else 0.0)
        upd_got = (sd[name].double().reshape(-1) - params[name].reshape(-1))[sel]
        upd_exp = (new_p[name].reshape(-1) - params[name].reshape(-1))[sel]
        assert upd_exp.numel()
        _close(upd_got, upd_exp, 5e-3, 0.02 * lr, "adam update " + name)
    # rows without a gradient: unchanged, to the bit (dense Adam: zero moments; LazyAdam: not visited)
    for key, name in O.TABLES.items():
        rows = torch.ones(params[name].shape[0], dtype=torch.bool)
        rows[out["touched"][name]] = False
        assert rows.any() or key == "cate"
        assert torch.equal(sd[name][rows].double(), params[name][rows]), name
    assert torch.equal(sd["sequential/embedding/user_embedding"].double(), params["sequential/embedding/user_embedding"])


def test_two_steps_are_bit_identical(golden_dir, golden_hparams):
    hp = O.hparams(golden_hparams)
    feed = _feed(golden_dir, "iterator_train_plain.npz", b=1)
    runs = []
    for _ in range(2):
        net, _ = _setup(hp, _dims(hp), True)
        net.capture_grads = True
        net.train_step(net.upload(feed, True))
        torch.cuda.synchronize()
        runs.append((net.state_dict(), net.captured))
    (sd_a, cap_a), (sd_b, cap_b) = runs
    assert set(sd_a) == set(sd_b) and any(k.startswith("__adam__/") for k in sd_a)
    for k in sd_a:       # tables, dense parameters, Adam moments
        assert torch.equal(sd_a[k], sd_b[k]), k
    assert torch.equal(cap_a["dense_sumsq"], cap_b["dense_sumsq"])
    # squared norms of the un-merged slices of NCF's four lookup sites (slots 4, 5 are the shared trunk's regulariser
    # norms, which tests/test_det_grads_gpu.py leaves out for every model)
    assert torch.equal(cap_a["table_sumsq"][6:10], cap_b["table_sumsq"][6:10]) and float(cap_a["table_sumsq"][6]) > 0
    for k in cap_a["dense"]:
        assert torch.equal(cap_a["dense"][k], cap_b["dense"][k]), k
    for k in cap_a["tables"]:
        assert torch.equal(cap_a["tables"][k], cap_b["tables"][k]), k


def test_eval_scores_match_oracle(golden_dir, golden_hparams):
    hp = O.hparams(golden_hparams)
    net, params = _setup(hp, _dims(hp), True)
    feed_t = _feed(golden_dir, "iterator_train_plain.npz", b=0)
    new_p = O.train_step(params, O.init_adam(params), 1, O.to_torch_feed(feed_t, dtype=torch.float64), hp)[0]
    net.train_step(net.upload(feed_t, True))
    feed = _feed(golden_dir, "iterator_eval_plain.npz", b=0)
    exp0 = O.predict(params, O.to_torch_feed(feed, dtype=torch.float64), hp)
    exp = O.predict(new_p, O.to_torch_feed(feed, dtype=torch.float64), hp)
    got = net.forward(net.upload(feed, False), False)
    torch.cuda.synchronize()
    _close(got["logit"], exp["logit"], 1e-4, 1e-4, "logit")
    _close(torch.sigmoid(got["logit"]), exp["pred"], 2e-3, 2e-4, "pred")
    assert float((exp["logit"] - exp0["logit"]).abs().max()) > 1e-3        # (the step moved the scores: the check above sees it)


def test_model_api_roundtrip(golden_dir, golden_hparams, tmp_path):
    """NCFModel through the shared API: fit one epoch, every requested metric, one score per line, checkpoint into a fresh
    model with identical scores, a state_dict of exactly the reference's variable names."""
    from clsr_amd.clsr import NCFModel
    from clsr_amd.sequential_iterator import SequentialIterator

    d = os.path.join(golden_dir, "data")
    hp = O.hparams(golden_hparams, epochs=1, MODEL_DIR=str(tmp_path / "model") + "/")
    model = NCFModel(hp, SequentialIterator, seed=7)
    assert model.fit(os.path.join(d, "train_data"), os.path.join(d, "valid_data"), valid_num_ngs=4,
                     eval_metric="auc") is model
    res = model.run_weighted_eval(os.path.join(d, "test_data"), 9)
    want = {"auc", "logloss", "mean_mrr", "ndcg@2", "ndcg@4", "ndcg@6", "hit@2", "hit@4", "hit@6", "wauc"}
    assert want <= set(res) and all(np.isfinite(float(v)) for v in res.values()), res
    names = {n for n in model.net.state_dict() if not n.startswith("__")}
    assert names == {n for n, _, _ in O.param_specs(_dims(hp), hp)}
    ckpt = str(tmp_path / "ckpt" / "ncf")
    os.makedirs(os.path.dirname(ckpt))
    model.save_model(ckpt)
    fresh = NCFModel(copy.deepcopy(hp), SequentialIterator, seed=123)
    fresh.load_model(ckpt)
    a, b = tmp_path / "pred_a.txt", tmp_path / "pred_b.txt"
    model.predict(os.path.join(d, "test_data"), str(a))
    fresh.predict(os.path.join(d, "test_data"), str(b))
    assert a.read_text() == b.read_text() and len(a.read_text().split()) == sum(1 for _ in open(os.path.join(d, "test_data")))
