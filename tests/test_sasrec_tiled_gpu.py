"""GPU parity of SASRec with ``long_histories=True`` (clsr_amd/seqnet.py kind "sasrec"; the tiled kernels of csrc/sasrec.hip)
against its torch-CPU oracle (tests/sasrec_oracle.py, float64, autograd), with the step check and the tolerances of
tests/test_sasrec_gpu.py, unchanged: one step past the resident kernels' limit and at the Kuaishou quick start's 250 steps,
histories of 1, T, T // 2, one tile and one tile plus one real steps, Adam and LazyAdam, clip on and off.  The dispatch rule
(a shape the resident kernels admit runs them: bit-identical nets at T = 50), evaluation with shared histories at T = 250, a
captured step against the eager one, and the model API at ``max_seq_length = 120``: fit with and without ``resident_data``,
a checkpoint from a net with the keyword into one without."""
import copy
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sasrec_cases as K  # noqa: E402
import sasrec_oracle as O  # noqa: E402
import sasrec_tiled_cases as TK  # noqa: E402
import test_sasrec_gpu as B  # noqa: E402
from clsr_amd.ops import query  # noqa: E402
from clsr_amd.seqnet import SeqNet  # noqa: E402

DIMS = B.DIMS
T_PAST = TK.T_AT_40 + 1


def _yaml(T):
    return dict(B.YAML, max_seq_length=T)


def _setup(hp, dims, det=True, dedup=True, long_histories=True):
    """tests/test_sasrec_gpu.py's ``_setup`` with the keyword"""
    params32 = O.init_params(dims, hp, **O.FIXTURE)
    net = SeqNet(hp, dims, kind="sasrec", device="cuda:0", seed=0, dedup_histories=dedup, long_histories=long_histories)
    net.det_grads = det
    sd = dict(params32)
    sd.update(O.init_bn_state(params32))
    net.load_state_dict(sd, strict=True)
    params64 = type(params32)((k, v.double()) for k, v in params32.items())
    return net, params64


def _lens(T):
    tile = TK.default_tile(T, 40)
    assert 1 < tile < T - 1
    return (1, T, T // 2, tile, tile + 1)


@pytest.mark.parametrize("T", [T_PAST, 250])
@pytest.mark.parametrize("optimizer,clip", [("adam", 1), ("lazyadam", 1), ("adam", 0), ("lazyadam", 0)])
def test_train_step_matches_oracle(golden_hparams, monkeypatch, T, optimizer, clip):
    """The whole check of tests/test_sasrec_gpu.py::_step_matches_oracle, on a net built with the keyword"""
    monkeypatch.setattr(B, "_setup", _setup)
    hp = O.hparams(golden_hparams, train_num_ngs=4, optimizer=optimizer, is_clip_norm=clip, **_yaml(T))
    feed = K.edge_feed(T, 5, DIMS["Vi"], DIMS["Vc"], _lens(T), seed=3)
    net, _ = B._step_matches_oracle(hp, DIMS, feed)
    assert net.long_histories and net._sasrec_tile(T) == TK.default_tile(T, 40) > 0
    assert query("clsr_sasrec_supported", T, T, 40, 2, 1) == 0
    assert any(k[0] == "sa.tws.train" for k in net._bufs) and not any(k[0] == "sa.ws" for k in net._bufs)


def test_two_steps_are_bit_identical(golden_hparams):
    hp = O.hparams(golden_hparams, **_yaml(250))
    feed = K.edge_feed(250, 5, DIMS["Vi"], DIMS["Vc"], _lens(250), seed=3)
    runs = []
    for _ in range(2):
        net, _ = _setup(hp, DIMS)
        net.train_step(net.upload(feed, True))
        torch.cuda.synchronize()
        runs.append(net.state_dict())
    assert set(runs[0]) == set(runs[1])
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_admitted_shapes_run_the_resident_kernels(golden_hparams):
    """T = 50: nets with and without the keyword end two steps in the same bits, and the one with it never sized a tiled
    workspace."""
    hp = O.hparams(golden_hparams, **_yaml(50))
    feed = K.edge_feed(50, 5, DIMS["Vi"], DIMS["Vc"], K.STEP_LENS, seed=3)
    sds = []
    for flag in (False, True):
        net, _ = _setup(hp, DIMS, long_histories=flag)
        assert net._sasrec_tile(50) == 0
        for _ in range(2):
            net.train_step(net.upload(feed, True))
        torch.cuda.synchronize()
        assert any(k[0] == "sa.ws" for k in net._bufs) and not any(str(k[0]).startswith("sa.tws") for k in net._bufs)
        sds.append(net.state_dict())
    assert list(sds[0]) == list(sds[1]) and any(k.startswith("__adam__/") for k in sds[0])
    for k in sds[0]:
        assert torch.equal(sds[0][k], sds[1][k]), k


def test_scoring_with_shared_histories(golden_hparams):
    """T = 250: the scores match the oracle's, and the compact feed (``hist_group``: a history's encoder runs once, s goes
    to every line of the group) gives the scores of the expanded feed, to the bit."""
    hp = O.hparams(golden_hparams, **_yaml(250))
    net, params = _setup(hp, DIMS)
    g = 5
    full = K.edge_feed(250, g, DIMS["Vi"], DIMS["Vc"], _lens(250), seed=4)
    exp = O.predict(params, O.init_bn_state(params), O.to_torch_feed(full, dtype=torch.float64), hp)
    got = net.forward(net.upload(full, False), False)
    torch.cuda.synchronize()
    a = got["logit"].clone()
    n = len(_lens(250))
    assert net.last_shape == (n * g, 250, 1, n * g)
    B._close(got["model_output"][:, :40], exp["s"], 1e-4, 1e-5, "s")
    B._close(a, exp["logit"], 1e-4, 1e-4, "logit")
    hist_keys = ("users", "item_history", "item_cate_history", "mask", "time_from_first_action", "time_to_now")
    compact = dict(full, hist_group=g, **{k: np.ascontiguousarray(full[k][::g]) for k in hist_keys})
    b = net.forward(net.upload(compact, False), False)["logit"].clone()
    torch.cuda.synchronize()
    assert net.last_shape == (n * g, 250, g, n)
    assert torch.equal(a, b) and float(a.std()) > 0
    assert any(k[0] == "sa.tws.score" for k in net._bufs)


def _hp120(golden_hparams, **kw):
    return O.hparams(golden_hparams, max_seq_length=120, save_model=False, show_step=10 ** 9, write_tfevents=False, **kw)


def _model(hp, **kw):
    return B._model(hp, long_histories=True, **kw)


def _state(model):
    with model._stream_ctx():
        torch.cuda.synchronize()
        return {k: v.detach().cpu().clone() for k, v in model.net.state_dict().items()}


def test_captured_step_is_bit_identical_to_the_eager_step(golden_dir, golden_hparams):
    """``use_graph=True`` at max_seq_length = 120 (the tiled pair): the first step runs eagerly and is captured, the later
    ones replay the graph, workspace included -- after each of three steps the state_dict is the eager model's."""
    hp = _hp120(golden_hparams)
    runs = []
    for graph in (False, True):
        model = _model(hp, use_graph=graph)
        assert model.net._sasrec_tile(120) > 0
        random.seed(9)
        feeds = (f for f in model.iterator.load_data_from_file(os.path.join(golden_dir, "data", "train_data"),
                                                               batch_num_ngs=4) if f)
        sds = []
        for _ in range(3):
            model.train(model.sess, next(feeds))
            sds.append(_state(model))
        runs.append(sds)
        assert len(model._graphs) == (1 if graph else 0)
    for i, (a, b) in enumerate(zip(*runs)):
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (i, k)
    assert not torch.equal(runs[0][0][O.POS], runs[0][2][O.POS])


def _fit(golden_dir, hp, **kw):
    d = os.path.join(golden_dir, "data")
    model = _model(hp, **kw)
    random.seed(9)
    model.fit(os.path.join(d, "train_data"), os.path.join(d, "valid_data"), valid_num_ngs=4, eval_metric="auc")
    res = model.run_weighted_eval(os.path.join(d, "valid_data"), num_ngs=4)
    return model, res, _state(model)


def test_model_api(golden_dir, golden_hparams, tmp_path):
    """Two epochs of ``SASRecModel(long_histories=True).fit`` at max_seq_length = 120, plain and with ``resident_data``:
    the same metrics and state_dict, to the bit.  A checkpoint saved at T = 50 with the keyword loads into a model without
    it and scores the same."""
    hp = _hp120(golden_hparams, epochs=2)
    plain, res_a, a = _fit(golden_dir, hp)
    assert plain.net.long_histories and plain.net._sasrec_tile(120) > 0
    assert any(k[0] == "sa.tws.train" for k in plain.net._bufs) and any(k[0] == "sa.tws.score" for k in plain.net._bufs)
    assert all(np.isfinite(float(v)) for v in res_a.values())
    resident, res_b, b = _fit(golden_dir, hp, resident_data=True)
    assert resident._resident is not None and resident._resident.uploads == 1
    assert res_a == res_b, (res_a, res_b)
    assert set(a) == set(b) and any(k.startswith(O.SCOPE) for k in a)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    names = {n for n in a if not n.startswith("__") and "moving_" not in n}
    assert names == {n for n, _, _ in O.param_specs(B._dims(hp), hp)}        # (no variable of the keyword's own)
    # a checkpoint crosses the keyword
    d = os.path.join(golden_dir, "data")
    hp50 = O.hparams(golden_hparams, max_seq_length=50, epochs=1, show_step=10 ** 9, write_tfevents=False,
                     MODEL_DIR=str(tmp_path / "model") + "/")
    with_flag = _model(hp50)
    random.seed(5)
    batch = next(f for f in with_flag.iterator.load_data_from_file(os.path.join(d, "train_data"), batch_num_ngs=4) if f)
    with_flag.train(None, batch)
    ckpt = str(tmp_path / "ckpt" / "sasrec")
    os.makedirs(os.path.dirname(ckpt))
    with_flag.save_model(ckpt)
    without = B._model(hp50)
    without.seed = 123
    without.load_model(ckpt)
    assert not without.net.long_histories
    pa, pb = tmp_path / "pred_a.txt", tmp_path / "pred_b.txt"
    with_flag.predict(os.path.join(d, "test_data"), str(pa))
    without.predict(os.path.join(d, "test_data"), str(pb))
    assert pa.read_text() == pb.read_text() and len(pa.read_text().split()) > 0
    sa, sb = _state(with_flag), _state(without)
    assert all(torch.equal(sa[k], sb[k]) for k in sa if not k.startswith("__"))
