"""GPU tests of the data-parallel step: two ranks with sync-BN reproduce the single-process step on the global batch.

Two transports: ``nccl`` (RCCL, one GPU per rank -- runs when the box has at least two GPUs, skipped otherwise) and
``staged`` (both ranks share the one GPU of the test box; every collective is staged through gloo on the host by
``_HostStagedDist``, whose blocking device-to-host copy on the issuing stream gives the same "ordered after that
stream's work so far" semantics RCCL has).  Plus: the order in which the overlapped exchange issues its collectives,
checked against the state of the step's stream joins at issue time."""
import copy
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


from clsr_amd.dp import HostStagedDist as _HostStagedDist  # noqa: E402


def _transports():
    return [pytest.param("staged"),
            pytest.param("nccl", marks=pytest.mark.skipif(torch.cuda.device_count() < 2,
                                                          reason="RCCL with two ranks needs two GPUs"))]


def _init(transport, rank, world, port):
    """-> (dist-like object for DataParallel / CLSRModel, device of this rank)"""
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if transport == "nccl":
        torch.cuda.set_device(rank)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
        return dist, "cuda:%d" % rank
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return _HostStagedDist(dist), "cuda:0"


def _worker(rank, world, port, hp, dims, feed, sd, sparse, out, transport="staged", overlap=True, mode="allgather"):
    import torch.distributed as dist

    from clsr_amd.dp import DataParallel, shard_feed
    from clsr_amd.net import CLSRNet

    d, dev = _init(transport, rank, world, port)
    net = CLSRNet(hp, dims, device=dev, seed=rank)  # different seeds: broadcast must fix that
    if rank == 0:
        net.load_state_dict(sd)
    dp = DataParallel(net, d, sync_bn=True, sparse_tables=sparse, overlap=overlap, sparse_mode=mode)
    net.capture_grads = True
    f = dp.prepare(net.upload(shard_feed(feed, rank, world, hp.train_num_ngs + 1), True))
    dp.train_step(f)
    torch.cuda.synchronize()
    if rank == 0:
        out["state"] = {k: v.numpy() for k, v in net.state_dict().items()}
        out["grads"] = {k: v.cpu().numpy() for k, v in net.captured["dense"].items()}
        out["tgrads"] = {k: v.cpu().numpy() for k, v in net.captured["tables"].items()}
        out["losses"] = net.read_losses()
        out["sparse"] = list(dp.last_sparse)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("transport", _transports())
@pytest.mark.parametrize("sparse,overlap,mode", [("none", True, "allgather"), ("all", True, "allgather"),
                                                 ("auto", True, "allgather"), ("none", False, "allgather"),
                                                 ("all", True, "owner"), ("all", False, "owner")])
def test_two_ranks_match_single_process(golden_dir, golden_hparams, sparse, overlap, mode, transport):
    import pickle

    import torch.multiprocessing as mp

    from clsr_amd.net import CLSRNet
    from oracle import clsr_oracle as O

    hp = copy.deepcopy(golden_hparams)
    dims = dict(Vu=len(pickle.load(open(hp.user_vocab, "rb"))), Vi=len(pickle.load(open(hp.item_vocab, "rb"))),
                Vc=len(pickle.load(open(hp.cate_vocab, "rb"))))
    g = np.load(os.path.join(golden_dir, "iterator_train_sa.npz"))
    feed = {k[3:]: g[k] for k in g.files if k.startswith("b0_")}
    params = O.init_params(dims, hp, seed=5, scale_dense=8.0)
    sd = dict(params)
    sd.update(O.init_bn_state(params))
    single = CLSRNet(hp, dims, device="cuda:0", seed=0)
    single.load_state_dict(sd)
    single.capture_grads = True
    single.train_step(single.upload(feed, True))
    torch.cuda.synchronize()
    ref_state, ref_losses = single.state_dict(), single.read_losses()

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    mgr = ctx.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, port, hp, dims, feed, sd, sparse, out, transport, overlap, mode), nprocs=2, join=True)
    assert len(out["sparse"]) == {"none": 0, "all": 4}.get(sparse, len(out["sparse"]))
    for k in ("loss", "data_loss", "contrastive_loss", "regular_loss", "discrepancy_loss"):
        assert abs(out["losses"][k] - ref_losses[k]) < 1e-5 * max(1.0, abs(ref_losses[k])), (k, out["losses"], ref_losses)
    # gradients of the global batch (pre-clip, regularisers included) agree to fp32 accumulation noise
    ref_g = {k: v.cpu().numpy() for k, v in single.captured["dense"].items()}
    floor = 1e-6 * max(float(np.abs(v).max()) for v in ref_g.values())
    for k, v in ref_g.items():
        d = np.abs(out["grads"][k] - v)
        assert float(d.max()) <= 2e-3 * float(np.abs(v).max()) + floor, (k, float(d.max()), float(np.abs(v).max()))
    for k, v in single.captured["tables"].items():
        v = v.cpu().numpy()
        d = np.abs(out["tgrads"][k] - v)
        assert float(d.max()) <= 2e-3 * float(np.abs(v).max()) + floor, (k, float(d.max()))
    # BN moving statistics equal the global-batch ones
    for k, v in ref_state.items():
        if k.endswith("moving_mean") or k.endswith("moving_variance"):
            np.testing.assert_allclose(out["state"][k], v.numpy(), rtol=1e-4, atol=1e-6, err_msg=k)


@pytest.mark.parametrize("mode", ["allgather", "owner"])
def test_two_ranks_catalogue_dims_through_the_sparse_exchange(mode):
    """BASELINE configs[4] layer sizes (item 96 + category 32 = 128 = user = hidden, lazy Adam, row lists) with EVERY table
    exchanged as touched rows (sparse_tables="all": the path the 100M-item catalogue takes), two ranks on one device with
    host-staged collectives, against the single-process step on the global batch."""
    import sys

    import torch.multiprocessing as mp

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import build_hparams
    from clsr_amd.net import CLSRNet
    from clsr_amd.synthetic import synthetic_feed
    from oracle import clsr_oracle as O

    cfg = dict(Vu=300, Vi=5000, Vc=40, Di=96, Dc=32, Du=128, H=128, T=20, P=32)
    hp = build_hparams(cfg, cfg["P"], optimizer="lazyadam")
    dims = dict(Vu=cfg["Vu"], Vi=cfg["Vi"], Vc=cfg["Vc"])
    feed = synthetic_feed(cfg["P"], cfg["T"], cfg["Vu"], cfg["Vi"], cfg["Vc"], lengths="lognormal", seed=7)
    params = O.init_params(dims, hp, seed=5, scale_dense=4.0)
    sd = dict(params)
    sd.update(O.init_bn_state(params))
    single = CLSRNet(hp, dims, device="cuda:0", seed=0)
    single.rowlist_min_elems = 0          # (row lists as at the catalogue, whatever the table size)
    single.load_state_dict(sd)
    single.capture_grads = True
    single.train_step(single.upload(feed, True))
    torch.cuda.synchronize()
    ref_state, ref_losses = single.state_dict(), single.read_losses()

    s_ = socket.socket()
    s_.bind(("127.0.0.1", 0))
    port = s_.getsockname()[1]
    s_.close()
    ctx = mp.get_context("spawn")
    mgr = ctx.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, port, hp, dims, feed, sd, "all", out, "staged", True, mode), nprocs=2, join=True)
    assert len(out["sparse"]) == 4
    for k in ("loss", "data_loss", "contrastive_loss", "regular_loss", "discrepancy_loss"):
        assert abs(out["losses"][k] - ref_losses[k]) < 1e-5 * max(1.0, abs(ref_losses[k])), (k, out["losses"], ref_losses)
    ref_g = {k: v.cpu().numpy() for k, v in single.captured["dense"].items()}
    floor = 3e-6 * max(float(np.abs(v).max()) for v in ref_g.values())
    for k, v in ref_g.items():
        d = np.abs(out["grads"][k] - v)
        assert float(d.max()) <= 2e-3 * float(np.abs(v).max()) + floor, (k, float(d.max()), float(np.abs(v).max()))
    for k, v in single.captured["tables"].items():
        v = v.cpu().numpy()
        d = np.abs(out["tgrads"][k] - v)
        assert float(d.max()) <= 2e-3 * float(np.abs(v).max()) + floor, (k, float(d.max()))
    # the updated tables (lazy Adam on the exchanged rows) and the moving statistics equal the single-process ones
    for k, v in ref_state.items():
        if k.endswith("moving_mean") or k.endswith("moving_variance") or k.endswith("_embedding"):
            np.testing.assert_allclose(out["state"][k], v.numpy(), rtol=2e-4, atol=2e-6, err_msg=k)


def _model_worker(rank, world, port, hp, paths, sd, out, transport="staged"):
    import random

    import torch.distributed as dist

    from clsr_amd.clsr import CLSRModel
    from clsr_amd.sequential_iterator import SASequentialIterator

    d, dev = _init(transport, rank, world, port)
    model = CLSRModel(hp, SASequentialIterator, seed=rank, dist=d, sync_bn=True, device=dev)
    if rank == 0:
        model.net.load_state_dict(sd)
    random.seed(11)                      # same global batches (shuffle + negative sampling) on every rank
    losses = []
    for feed in model.iterator.load_data_from_file(paths, batch_num_ngs=hp.train_num_ngs):
        if feed:
            losses.append(model.train(model.sess, feed)[2])
        if len(losses) == 4:
            break
    torch.cuda.synchronize()
    out[rank] = dict(losses=losses, item=model.net.tables["item"].cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("transport", _transports())
def test_model_train_with_two_ranks_matches_single_process(golden_dir, golden_hparams, transport):
    """CLSRModel(dist=...): two ranks that iterate the same global batches and train on their halves follow the
    single-process run on the global batches (sync-BN): same loss per step, same embedding table afterwards.
    (Four steps: over a whole epoch the two runs drift apart like any two fp32 runs with Adam -- parameters whose
    gradient is analytically zero random-walk by +-lr per step on summation noise.)"""
    import random

    import torch.multiprocessing as mp

    from clsr_amd.clsr import CLSRModel
    from clsr_amd.sequential_iterator import SASequentialIterator

    hp = copy.deepcopy(golden_hparams)
    hp.batch_size = 16                   # global batch: 8 positives per rank
    train = os.path.join(golden_dir, "data", "train_data")
    single = CLSRModel(hp, SASequentialIterator, seed=0)
    sd = {k: v.clone() for k, v in single.net.state_dict().items()}
    random.seed(11)
    ref_losses = []
    for feed in single.iterator.load_data_from_file(train, batch_num_ngs=hp.train_num_ngs):
        if feed:
            ref_losses.append(single.train(single.sess, feed)[2])
        if len(ref_losses) == 4:
            break
    torch.cuda.synchronize()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    mp.spawn(_model_worker, args=(2, port, hp, train, sd, out, transport), nprocs=2, join=True)
    assert len(out[0]["losses"]) == len(ref_losses) == 4
    for a, b, c in zip(out[0]["losses"], out[1]["losses"], ref_losses):
        assert abs(a - b) < 1e-12 and abs(a - c) < 1e-4 * max(1.0, abs(c)), (a, b, c)
    # Adam divides by sqrt(v) + 1e-8: an element whose gradient is fp32 summation noise of ~1e-10 moves by a visible
    # fraction of lr, with the sign of the noise -- and two ranks sum in a different order than one process.  A handful
    # of such elements (seen: 2 of 31 808, off by 2.2e-5, one run in ~5) is not a defect; a real one (a lost shard, a
    # wrong scale) moves EVERY touched element by ~lr per step.  So: tight tolerance for all but 0.1 % of the elements,
    # and a bound of 5 % of lr * steps for those.
    a, b = out[0]["item"], single.net.tables["item"].cpu().numpy()
    bad = np.abs(a - b) > 2e-6 + 1e-3 * np.abs(b)
    assert bad.mean() < 1e-3, "%d of %d elements differ" % (bad.sum(), bad.size)
    assert float(np.abs(a - b).max()) < 0.05 * float(hp.learning_rate) * 4, float(np.abs(a - b).max())
    np.testing.assert_array_equal(out[0]["item"], out[1]["item"])      # replicas stay bit-identical


def _sibling_worker(rank, world, port, hp, dims, kind, feed, sd, out):
    import torch.distributed as dist

    from clsr_amd.dp import DataParallel, shard_feed
    from clsr_amd.seqnet import SeqNet

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    net = SeqNet(hp, dims, kind=kind, device="cuda:0", seed=rank)
    if rank == 0:
        net.load_state_dict(sd)
    dp = DataParallel(net, _HostStagedDist(dist), sync_bn=True, sparse_tables="auto")
    net.capture_grads = True
    dp.train_step(dp.prepare(net.upload(shard_feed(feed, rank, world, hp.train_num_ngs + 1), True)))
    torch.cuda.synchronize()
    if rank == 0:
        out["grads"] = {k: v.cpu().numpy() for k, v in net.captured["dense"].items()}
        out["tgrads"] = {k: v.cpu().numpy() for k, v in net.captured["tables"].items()}
        out["losses"] = net.read_losses()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("kind,model_type", [("sli_rec", "sli_rec"), ("dien", "DIEN")])
def test_sibling_models_two_ranks_match_single_process(golden_dir, golden_hparams, kind, model_type):
    """The sibling models go through the same DataParallel exchange (two trained tables instead of four)."""
    import pickle

    from oracle import sibling_oracle as O

    hp = copy.deepcopy(golden_hparams)
    hp.model_type, hp.user_embedding_dim, hp.attention_size = model_type, 16, 40
    dims = dict(Vu=len(pickle.load(open(hp.user_vocab, "rb"))), Vi=len(pickle.load(open(hp.item_vocab, "rb"))),
                Vc=len(pickle.load(open(hp.cate_vocab, "rb"))))
    _sibling_two_ranks(golden_dir, hp, dims, kind, O.init_params(dims, hp, kind, seed=5, scale_dense=8.0))


def test_caser_two_ranks_match_single_process(golden_dir, golden_hparams):
    """Caser adds only dense parameters (the convolution kernels and biases of both tables) to the same exchange: each rank
    runs the convolutions over its own histories and the weight gradients are summed by the dense all-reduce."""
    import pickle
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import caser_oracle as O

    hp = O.hparams(golden_hparams)
    dims = dict(Vu=len(pickle.load(open(hp.user_vocab, "rb"))), Vi=len(pickle.load(open(hp.item_vocab, "rb"))),
                Vc=len(pickle.load(open(hp.cate_vocab, "rb"))))
    _sibling_two_ranks(golden_dir, hp, dims, "caser", O.init_params(dims, hp, **O.FIXTURE))


def _sibling_two_ranks(golden_dir, hp, dims, kind, params):
    import torch.multiprocessing as mp

    from clsr_amd.seqnet import SeqNet
    from oracle import sibling_oracle as O

    g = np.load(os.path.join(golden_dir, "iterator_train_sa.npz"))
    feed = {k[3:]: g[k] for k in g.files if k.startswith("b0_")}
    sd = dict(params)
    sd.update(O.init_bn_state(params))
    single = SeqNet(hp, dims, kind=kind, device="cuda:0", seed=0)
    single.load_state_dict(sd)
    single.capture_grads = True
    single.train_step(single.upload(feed, True))
    torch.cuda.synchronize()
    ref_losses = single.read_losses()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    mp.spawn(_sibling_worker, args=(2, port, hp, dims, kind, feed, sd, out), nprocs=2, join=True)
    for k in ("loss", "data_loss", "regular_loss"):
        assert abs(out["losses"][k] - ref_losses[k]) < 1e-5 * max(1.0, abs(ref_losses[k])), (k, out["losses"], ref_losses)
    ref_g = {k: v.cpu().numpy() for k, v in single.captured["dense"].items()}
    floor = 4e-6 * max(float(np.abs(v).max()) for v in ref_g.values())
    for k, v in ref_g.items():
        d = np.abs(out["grads"][k] - v)
        assert float(d.max()) <= 2e-3 * float(np.abs(v).max()) + floor, (k, float(d.max()), float(np.abs(v).max()))
    for k, v in single.captured["tables"].items():
        v = v.cpu().numpy()
        assert float(np.abs(out["tgrads"][k] - v).max()) <= 2e-3 * float(np.abs(v).max()) + floor, k


def _epoch_worker(rank, world, port, hp, train, dedup, out):
    import random

    import torch.distributed as dist

    from clsr_amd.clsr import CLSRModel
    from clsr_amd.sequential_iterator import SASequentialIterator

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model = CLSRModel(hp, SASequentialIterator, seed=3, dist=_HostStagedDist(dist), sync_bn=True,
                      dedup_histories=dedup)
    random.seed(11)
    it = model.iterator.load_data_from_file(train, batch_num_ngs=hp.train_num_ngs)
    loss = model.batch_train(it, model.sess)
    torch.cuda.synchronize()
    model.net.read_losses()      # (raises if a grid barrier of the fused heads timed out)
    out[rank] = dict(loss=float(loss), item=model.net.tables["item"].cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("dedup", [True, False])
def test_two_rank_epoch_with_ragged_end(golden_dir, golden_hparams, dedup):
    """A whole data-parallel epoch whose batches do not divide by the ranks: 600 lines in batches of 85 positives
    (odd: one positive per batch is dropped by the sharding, compact and row layout alike) and a last batch of 5;
    then batches of 599, whose last batch of ONE positive cannot feed two ranks and is skipped on both."""
    import torch.multiprocessing as mp

    train = os.path.join(golden_dir, "data", "train_data")
    for bs in (85, 599):
        hp = copy.deepcopy(golden_hparams)
        hp.batch_size = bs
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        ctx = mp.get_context("spawn")
        out = ctx.Manager().dict()
        mp.spawn(_epoch_worker, args=(2, port, hp, train, dedup, out), nprocs=2, join=True)
        assert np.isfinite(out[0]["loss"]) and out[0]["loss"] == out[1]["loss"]
        np.testing.assert_array_equal(out[0]["item"], out[1]["item"])      # replicas stay bit-identical


class _RecordingDist(object):
    """Single-process torch.distributed look-alike (world 2 on paper): collectives are identities that record, at
    ISSUE time, what the step's stream bookkeeping looked like."""

    class ReduceOp(object):
        SUM, MAX = "sum", "max"

    class _Work(object):
        def __init__(self, log):
            self.log = log

        def wait(self):
            self.log.append(("wait", None))

    def __init__(self):
        self.log, self.net = [], None

    def get_world_size(self, group=None):
        return 2

    def get_rank(self, group=None):
        return 0

    def broadcast(self, t, src=0, group=None):
        pass

    def all_reduce(self, t, op=None, group=None, async_op=False):
        n = self.net
        self.log.append(("all_reduce", t.data_ptr(), t.numel(), torch.cuda.current_stream().cuda_stream,
                         [j[0] for j in n._joins], {k: len(v) for k, v in n._dw_pending.items() if v}))
        return self._Work(self.log) if async_op else None

    def all_gather(self, outs, t, group=None):
        for o in outs:
            o.copy_(t)


@pytest.mark.parametrize("coalesce", [True, False])
@pytest.mark.parametrize("planned", [False, True])
def test_overlapped_exchange_is_issued_after_the_joins_that_finish_its_data(golden_dir, golden_hparams, planned, coalesce):
    """Fails if a collective is enqueued before the stream joins / weight-gradient flush that make its buffer final:
    the dense all-reduce must see NO unjoined branch and NO pending weight-gradient partials and rides on the
    weight-gradient stream; the gradient tables go as one collective from the compute stream after the final join; the
    24 doubles and every wait come last.  Also under a replayed launch plan (the hooks are part of the plan)."""
    import pickle

    from clsr_amd.dp import DataParallel
    from clsr_amd.net import CLSRNet

    hp = copy.deepcopy(golden_hparams)
    dims = dict(Vu=len(pickle.load(open(hp.user_vocab, "rb"))), Vi=len(pickle.load(open(hp.item_vocab, "rb"))),
                Vc=len(pickle.load(open(hp.cate_vocab, "rb"))))
    g = np.load(os.path.join(golden_dir, "iterator_train_sa.npz"))
    feed = {k[3:]: g[k] for k in g.files if k.startswith("b0_")}
    net = CLSRNet(hp, dims, device="cuda:0", seed=0)
    d = _RecordingDist()
    d.net = net
    dp = DataParallel(net, d, sync_bn=False, sparse_tables="none")
    dp.coalesce = coalesce
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        f = net.upload(feed, True)
        for _ in range(3 if planned else 1):     # third occurrence = replayed plan
            d.log.clear()
            dp.trace = []
            dp.train_step(f)
        torch.cuda.synchronize()
    main = stream.cuda_stream
    ar = [e for e in d.log if e[0] == "all_reduce"]
    by_ptr = {e[1]: e for e in ar}
    if coalesce:
        # every table dense: [dense gradients | gradient tables | moving statistics (per-rank batch-norm)] = the whole flat
        # buffer in ONE collective on the compute stream, after the final join and behind a wait for the weight-gradient
        # stream (where the dense gradients became final); the byte maps before it, the 24 doubles after it
        assert net.dense_grad.data_ptr() == net.grad_flat.data_ptr()
        one = by_ptr[net.grad_flat.data_ptr()]
        assert one[2] == net.grad_flat.numel() and one[3] == main
        assert net.tab_grad_flat.data_ptr() not in by_ptr and net.bn_moving.data_ptr() not in by_ptr
        if not planned:
            assert one[4] in ([], ["@dense"]) and one[5] == {}, "issued before the joins / the dW flush: %r" % (one,)
        flags = by_ptr[net.tab_flags_flat.data_ptr()]
        assert d.log.index(flags) < d.log.index(one) and flags[3] != main
        small = by_ptr[net.stats24.data_ptr()]
        assert d.log.index(small) > d.log.index(one)
        waits = [i for i, e in enumerate(d.log) if e[0] == "wait"]
        assert len(waits) == len(ar) == 3 and min(waits) > max(d.log.index(e) for e in ar)
        return
    dense = by_ptr[net.dense_grad.data_ptr()]
    if not planned:      # (a replayed plan does not rebuild the python-side bookkeeping the recorder looks at)
        assert dense[4] in ([], ["@dense"]) and dense[5] == {}, "dense all-reduce issued before the joins / the dW flush: %r" % (dense,)
    assert dense[3] != main, "the dense path (batched reduction, all-reduce) runs on the weight-gradient stream"
    flags = by_ptr[net.tab_flags_flat.data_ptr()]
    assert d.log.index(flags) < d.log.index(dense), "the byte maps are exchanged from the start of the step"
    assert flags[3] != main, "flags ride on the side stream that marked them"
    # the four dense gradient tables travel as ONE collective, issued on the compute stream after the final join; the
    # dense gradients follow it (issue order = execution order inside a process group) on the weight-gradient stream
    tabs = by_ptr[net.tab_grad_flat.data_ptr()]
    last = list(net.tab_grad)[-1]       # (one run from the first table to the end of the last: the 256-byte padding between tables travels too)
    assert tabs[2] == net.tab_goff[last] + net.tab_grad[last].numel()
    if not planned:     # (the dense branch is independent of the tables: it is joined by the optimiser, not here)
        assert tabs[4] in ([], ["@dense"]), "table all-reduce issued before the final join"
    assert tabs[3] == main
    assert d.log.index(flags) < d.log.index(tabs) < d.log.index(dense)
    small = by_ptr[net.stats24.data_ptr()]
    assert d.log.index(small) > d.log.index(dense)
    waits = [i for i, e in enumerate(d.log) if e[0] == "wait"]
    assert len(waits) == len(ar) and min(waits) > max(d.log.index(e) for e in ar)
    assert [w for w, _ in dp.trace if w == "finish"] == ["finish"]
