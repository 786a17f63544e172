"""The resident evaluation path end to end (``resident_eval=True``): every chunk feed built on the device is the feed
``upload`` makes from the host iterator's batches, tensor for tensor; ``run_eval`` / ``run_weighted_eval`` / ``fit`` return
what they return with the flag off, compared with ``==``; the store follows the iterator; two ranks share a pass."""
import copy
import os
import random
import socket
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 10
WAIT_S = 120.0          # bound of the two rank processes (tests/test_shard_eval_gpu.py: start-up dominates, 2.5 - 4.3 s)
MODELS = [("CLSRModel", "SASequentialIterator"), ("A2SVDModel", "SequentialIterator"), ("NCFModel", "SequentialIterator")]


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
    assert "wauc" in hp.weighted_metrics
    return hp


def _model(name, it_name, hp, **kw):
    import clsr_amd.clsr as M
    import clsr_amd.sequential_iterator as I

    return getattr(M, name)(hp, getattr(I, it_name), seed=11, **kw)


def _pair(name, it_name, hp, **kw):
    """The same model with the flag off and on, from one state_dict."""
    off, on = _model(name, it_name, hp, **kw), _model(name, it_name, hp, resident_eval=True, **kw)
    with off._stream_ctx():
        torch.cuda.synchronize()
        sd = {k: v.detach().cpu().clone() for k, v in off.net.state_dict().items()}
    on.net.load_state_dict(sd)
    assert off._resident_eval is None and on._resident_eval is not None and on._resident is None
    return off, on


def _files(golden_dir):
    return [(os.path.join(golden_dir, "data", "valid_data"), 4), (os.path.join(golden_dir, "data", "test_data"), 9)]


def _host_chunks(model, path, m, target):
    """The feeds ``_device_eval`` uploads on the host path: ``_to_arrays`` per batch, batches of one group size joined."""
    chunks, pend, rows = [], [], 0

    def flush():
        chunks.append(pend[0] if len(pend) == 1 else {
            k: (v if k == "hist_group" else np.concatenate([np.asarray(x[k]) for x in pend], axis=0))
            for k, v in pend[0].items()})

    for batch in model.iterator.load_data_from_file(path, min_seq_length=m, batch_num_ngs=0):
        feed = model._to_arrays(batch)
        if pend and feed.get("hist_group", 0) != pend[0].get("hist_group", 0):
            flush()
            pend, rows = [], 0
        pend.append(feed)
        rows += int(np.asarray(feed["labels"]).shape[0])
        if rows >= target:
            flush()
            pend, rows = [], 0
    if pend:
        flush()
    return chunks


def _same_feed(got, want, what):
    public = lambda f: {k for k in f if not k.startswith("_")}
    assert public(got) == public(want), (what, sorted(public(got) ^ public(want)))
    for k in sorted(public(want)):
        if isinstance(want[k], torch.Tensor):
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
            assert got[k].data_ptr() % 16 == 0 and got["_arena"].lay[k] == want["_arena"].lay[k], (what, k)
            assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), (what, k)
        else:
            assert got[k] == want[k], (what, k, got[k], want[k])


@pytest.mark.parametrize("name,it_name,dedup", [m + (True,) for m in MODELS] + [MODELS[0] + (False,)])
def test_chunk_feeds_equal_the_uploaded_host_feeds(name, it_name, dedup, golden_dir, golden_hparams):
    from clsr_amd.resident import eval_chunk_plan

    model = _model(name, it_name, _hp(golden_hparams, name), dedup_histories=dedup, resident_eval=True)
    net, store = model.net, model._resident_eval
    seen, groups = 0, set()
    for path, _ in _files(golden_dir):
        for bs in (50, 64, 200):
            model.iterator.batch_size = bs
            for target in (32768, 120):
                for m in (1, 3):
                    with model._stream_ctx():
                        lines = store.get(path, m, flags=dedup)
                        plan = eval_chunk_plan(lines.flags, lines.n_keep, bs, target, dedup)
                        host = _host_chunks(model, path, m, target)
                        assert len(plan) == len(host) and plan
                        for (k0, n, g), feed in zip(plan, host):
                            want = net.upload(feed, False)
                            got = net.build_eval_feed(lines, k0, n, g)
                            torch.cuda.synchronize()
                            _same_feed(got, want, (path, bs, target, m, k0))
                            assert ("users_rows" in got) == (g > 1) and got["G"] == (g if g > 1 else 0) and got["B"] == n
                            groups.add(g)
                            seen += 1
    assert store.uploads == 2 and seen > 30
    assert groups == {1} if not dedup else groups >= {1, 5, 10}
    rc = store.files[path]
    assert rc.nbytes == rc.N * (16 * T + 20) and store.nbytes > sum(r.nbytes for r in store.files.values())


@pytest.mark.parametrize("name,it_name", MODELS)
@pytest.mark.parametrize("rows", [None, "120"])
def test_metrics_are_equal_with_the_flag_on_and_off(name, it_name, rows, golden_dir, golden_hparams, monkeypatch):
    if rows:
        monkeypatch.setenv("CLSR_EVAL_ROWS", rows)
    else:
        monkeypatch.delenv("CLSR_EVAL_ROWS", raising=False)
    off, on = _pair(name, it_name, _hp(golden_hparams, name, batch_size=50))
    kw = dict(calc_mean_alpha=True) if name == "CLSRModel" else {}
    for path, ngs in _files(golden_dir):
        a, b = off.run_eval(path, ngs), on.run_eval(path, ngs)
        assert a == b and "auc" in a, (a, b)
        assert on.eval_rows_scored == off.eval_rows_scored > 0
        a, b = off.run_weighted_eval(path, ngs, **kw), on.run_weighted_eval(path, ngs, **kw)
        assert a == b and "wauc" in a and ("mean_alpha" in a) == bool(kw), (a, b)
    # the chunks were built on the device, under a key of their own; the host path of the other model made none
    assert any(k[0] == "resident_eval" for k in on._static) and all(k[0] != "resident_eval" for k in off._static)
    assert all(k[0] == "resident_eval" for k in on._static)
    assert on._resident_eval.uploads == 2


@pytest.mark.parametrize("name,it_name,resident_data", [MODELS[0] + (False,), MODELS[0] + (True,), MODELS[1] + (False,)])
def test_fit_is_bit_identical_with_the_flag_on_and_off(name, it_name, resident_data, golden_dir, golden_hparams):
    """Two epochs: the same state_dict, the same validation dict after every epoch, the same ``random`` state."""
    train = os.path.join(golden_dir, "data", "train_data")
    valid = os.path.join(golden_dir, "data", "valid_data")
    hp = _hp(golden_hparams, name, epochs=2)
    out = []
    for flag in (False, True):
        model = _model(name, it_name, hp, resident_eval=flag, resident_data=resident_data)
        per_epoch, whole = [], model.run_weighted_eval
        model.run_weighted_eval = lambda *a, **k: (per_epoch.append(whole(*a, **k)), per_epoch[-1])[1]
        random.seed(9)
        model.fit(train, valid, valid_num_ngs=4, eval_metric="wauc")
        with model._stream_ctx():
            torch.cuda.synchronize()
            sd = {k: v.detach().cpu().clone() for k, v in model.net.state_dict().items()}
        out.append((per_epoch, sd, random.getstate()))
        assert len(per_epoch) == 2
        assert (model._resident_eval is not None) == flag and (model._resident is not None) == resident_data
        if resident_data:
            assert model._resident.uploads == 1 and model._resident.nbytes == 600 * (16 * T + 16)
        if flag:
            assert model._resident_eval.uploads == 1 and set(model._resident_eval.files) == {valid}
    (ra, a, sa), (rb, b, sb) = out
    assert ra == rb, (ra, rb)
    assert sa == sb
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_store_follows_the_iterator(golden_dir, golden_hparams, monkeypatch):
    valid = os.path.join(golden_dir, "data", "valid_data")
    off, on = _pair("A2SVDModel", "SequentialIterator", _hp(golden_hparams, "A2SVDModel"))
    store = on._resident_eval
    want = off.run_weighted_eval(valid, 4)
    assert on.run_weighted_eval(valid, 4) == want and store.uploads == 1
    lines = store.files[valid].lines[1]
    assert lines.flags is not None and lines.flags.sum() == 160
    # a second pass over an unchanged file uploads nothing and asks for no flags
    from clsr_amd import ops

    real, names = ops.call, []
    monkeypatch.setattr(ops, "call", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    assert on.run_weighted_eval(valid, 4) == want
    monkeypatch.setattr(ops, "call", real)
    assert store.uploads == 1 and store.files[valid].lines[1] is lines
    assert "clsr_feed_build_eval" in names and "clsr_feed_same_rows" not in names
    # host metrics: the host path whole, the same dict with the flag on, the store not touched
    with monkeypatch.context() as mp:
        mp.setenv("CLSR_HOST_METRICS", "1")
        names.clear()
        mp.setattr(ops, "call", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
        a, b = off.run_weighted_eval(valid, 4), on.run_weighted_eval(valid, 4)
        assert a == b and "wauc" in a and "clsr_feed_build_eval" not in names
    # a training pass over the same file leaves it shuffled: both paths score the lines in the new order (the whole file
    # as ONE group of 200 lines, so that every group still holds a positive line)
    for model in (off, on):
        random.seed(21)
        for _ in model.iterator.load_data_from_file(valid, batch_num_ngs=4):
            pass
    a, b = off.run_weighted_eval(valid, 199), on.run_weighted_eval(valid, 199)
    assert a == b and "wauc" in a, (a, b)
    shuffled = store.files[valid].lines[1]
    assert store.uploads == 1 and shuffled is not lines and not np.array_equal(shuffled.keep, lines.keep)
    assert np.array_equal(np.sort(shuffled.keep), lines.keep) and shuffled.flags.sum() < 160
    assert off.run_eval(valid, 199) == on.run_eval(valid, 199)
    # a re-parsed file is uploaded again
    on.iterator.iter_data.pop(valid)
    assert on.run_eval(valid, 199) == off.run_eval(valid, 199)
    assert store.uploads == 2


def test_nextitnet_refuses_resident_eval(golden_hparams):
    from clsr_amd.clsr import NextItNetModel
    from clsr_amd.deeprec_utils import prepare_hparams
    from clsr_amd.sequential_iterator import NextItNetIterator

    g = golden_hparams
    hp = prepare_hparams(os.path.join(ROOT, "clsr_amd", "config", "nextitnet.yaml"), user_vocab=g.user_vocab,
                         item_vocab=g.item_vocab, cate_vocab=g.cate_vocab, max_seq_length=T, batch_size=64,
                         train_num_ngs=4, time_unit="s")
    with pytest.raises(NotImplementedError, match="NextItNetIterator"):
        NextItNetModel(hp, NextItNetIterator, seed=1, resident_eval=True)


# ------------------------------------------------------------------------------ two rank processes on one GPU
def _jobs(golden_dir):
    (valid, _), (test, _) = _files(golden_dir)
    return [("run_weighted_eval", valid, 4, {}), ("run_eval", test, 9, {}),
            ("run_weighted_eval", valid, 4, dict(calc_mean_alpha=True))]


def _rank_worker(rank, world, port, hp, sd, jobs, out):
    import torch.distributed as dist

    from clsr_amd.clsr import CLSRModel
    from clsr_amd.dp import HostStagedDist
    from clsr_amd.sequential_iterator import SASequentialIterator

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model = CLSRModel(hp, SASequentialIterator, seed=100 + rank, dist=HostStagedDist(dist), device="cuda:0", shard_eval=True,
                      resident_eval=True)
    model.net.load_state_dict(sd)
    res = []
    for method, path, ngs, kw in jobs:
        res.append((getattr(model, method)(path, ngs, **kw), model.eval_rows_scored))
    out[rank] = (res, model._resident_eval.uploads, sorted(k[0] for k in model._static))
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_share_a_resident_evaluation(golden_dir, golden_hparams, monkeypatch):
    """``shard_eval=True`` with the flag on: chunks of 64 lines from batches of 12, so borders fall inside groups of 5;
    every rank returns the single-process dict of the host path and scores a share of the lines."""
    import torch.multiprocessing as mp

    monkeypatch.setenv("CLSR_EVAL_ROWS", "64")
    hp = _hp(golden_hparams, "CLSRModel", batch_size=12, weighted_metrics=["wauc", "wmrr", "whit@1;2", "wndcg@1;2"])
    jobs = _jobs(golden_dir)
    single = _model("CLSRModel", "SASequentialIterator", hp)
    with single._stream_ctx():
        torch.cuda.synchronize()
        sd = {k: v.detach().cpu().clone() for k, v in single.net.state_dict().items()}
    want = [getattr(single, method)(path, ngs, **kw) for method, path, ngs, kw in jobs]
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = mp.get_context("spawn").Manager().dict()
    pc = mp.spawn(_rank_worker, args=(2, port, hp, sd, jobs, out), nprocs=2, join=False)
    deadline = time.monotonic() + WAIT_S
    try:
        while not pc.join(timeout=max(0.1, deadline - time.monotonic())):
            if time.monotonic() >= deadline:
                pytest.fail("rank processes still running after %.0f s" % WAIT_S)
    finally:
        for p in pc.processes:
            if p.is_alive():
                p.terminate()
        for p in pc.processes:
            p.join(10)
            if p.is_alive():
                p.kill()
    ranks = [out[r] for r in range(2)]
    for j, (method, path, ngs, kw) in enumerate(jobs):
        n_lines = 400 if path.endswith("test_data") else 200
        for rank, (res, uploads, keys) in enumerate(ranks):
            got, rows = res[j]
            assert got == want[j], (method, path, rank, got, want[j])
            assert 0 < rows < n_lines
        assert sum(res[j][1] for res, _, _ in ranks) == n_lines
    for _, uploads, keys in ranks:
        assert uploads == 2 and set(keys) == {"resident_eval"}
