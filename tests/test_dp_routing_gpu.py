"""The data-parallel exchange with per-rank batch-norm (``sync_bn=False``), for every routing of the four gradient tables.

Two ranks share the one GPU of the test box and exchange through ``HostStagedDist`` over gloo (the ``staged`` rig of
tests/test_dp_gpu.py).  ONE spawn of the two workers loops over all routings; every routing gets a fresh ``CLSRNet`` +
``DataParallel`` on the same process group (per-rank batch-norm creates no peer-to-peer communicator).

  * exchange == a hand-made accumulation of the two shards' gradient state on one device, bit for bit: with two ranks every
    dense sum is ``a + b`` (commutative), the sparse routes add ``0 + r0 + r1`` in rank order, and the step is deterministic;
  * the same over two steps with the routing changed in between (per-table buffers, byte maps and row lists carry over);
  * the step against the float64 oracle run on each shard with its own batch statistics (``O.sharded_gradients``);
  * ``DataParallel.capture()`` (two hipGraphs around the eager exchange) == ``train_step``.
"""
import copy
import os
import pickle
import socket

import numpy as np
import pytest
import torch

from clsr_amd.dp import HostStagedDist

ALL = ("item", "cate", "user_long", "user_short")

# (sparse tables, sparse_mode, overlap)
ROUTINGS = [
    ((), "allgather", True),                                     # every table dense: one collective for the flat buffer
    (("user_short",), "allgather", True),                        # dense prefix + sparse suffix: the three routings whose
    (("user_long", "user_short"), "allgather", True),            # sparse tables used to be summed twice
    (("cate", "user_long", "user_short"), "allgather", True),
    (("cate",), "allgather", True),                              # two dense runs
    (("item",), "allgather", True),                              # the catalogue case
    (ALL, "allgather", True),
    (("user_long", "user_short"), "owner", True),
    (ALL, "owner", True),
    (("user_long", "user_short"), "allgather", False),
]
# two steps, the routing changed in between (step 1 on b0, step 2 on b1)
SWAPS = [((("user_long", "user_short"), ("item",)), "allgather", True),
         ((("item",), ("user_long", "user_short")), "allgather", True)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _init(rank, world, port):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist, HostStagedDist(dist), "cuda:0"


class _RangeLog(object):
    """Passes every call on to the wrapped dist and keeps (first byte, last byte + 1, op) of every all-reduce."""

    def __init__(self, d):
        self._d, self.ReduceOp, self.log = d, d.ReduceOp, []

    def __getattr__(self, name):
        return getattr(self._d, name)

    def all_reduce(self, t, op=None, group=None, async_op=False):
        self.log.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), op))
        return self._d.all_reduce(t, op=op, group=group, async_op=async_op)


def _coverage_violations(net, log, sparse, sum_op):
    """SUM all-reduces of one step against the layout of the flat gradient buffer: the dense gradients, every DENSE table
    and the moving statistics lie in exactly one of them, a SPARSE table (merged by its row exchange) in none."""
    sums = [(a, b) for a, b, op in log if op == sum_op or op is None]
    bad = []

    def covers(t):
        lo, hi = t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()
        whole = sum(1 for a, b in sums if a <= lo and hi <= b)
        partly = sum(1 for a, b in sums if a < hi and lo < b) - whole
        return whole, partly

    pieces = [("dense_grad", net.dense_grad, 1), ("bn_moving", net.bn_moving, 1)]
    pieces += [(k, g, 0 if k in sparse else 1) for k, g in net.tab_grad.items()]
    for name, t, want in pieces:
        whole, partly = covers(t)
        if whole != want or partly:
            bad.append("%s: inside %d SUM all-reduces (expected %d), cut by %d" % (name, whole, want, partly))
    return bad


def _state(net):
    return {k: v.numpy() for k, v in net.state_dict().items()}


def _routing_worker(rank, world, port, hp, dims, feeds, sd, jobs, out):
    from clsr_amd.dp import DataParallel, shard_feed
    from clsr_amd.net import CLSRNet

    dist, staged, dev = _init(rank, world, port)
    for j, (routes, mode, overlap, grads) in enumerate(jobs):
        d = _RangeLog(staged)
        net = CLSRNet(hp, dims, device=dev, seed=rank)      # different seeds: the broadcast must fix that
        if rank == 0:
            net.load_state_dict(sd)
        dp = DataParallel(net, d, sync_bn=False, sparse_tables=routes[0], overlap=overlap, sparse_mode=mode)
        assert dp.comm is None and dp.stats_transport == "torch.distributed"
        net.capture_grads = grads
        res = dict(trace=[], sparse=[], coverage=[])
        for b, route in enumerate(routes):
            dp.sparse_tables = route
            dp.trace = []
            f = dp.prepare(net.upload(shard_feed(feeds[b], rank, world, hp.train_num_ngs + 1), True))
            del d.log[:]                                    # (prepare: the contrastive denominator)
            dp.train_step(f)
            torch.cuda.synchronize()
            res["trace"].append(list(dp.trace))
            res["sparse"].append(list(dp.last_sparse))
            res["coverage"].append(_coverage_violations(net, d.log, dp.last_sparse, d.ReduceOp.SUM))
        res["state"] = _state(net)
        if grads:
            res["grads"] = {k: v.cpu().numpy() for k, v in net.captured["dense"].items()}
            res["tgrads"] = {k: v.cpu().numpy() for k, v in net.captured["tables"].items()}
            res["losses"] = net.read_losses()
        out[(j, rank)] = res
        dp.close()
        del dp, net
    dist.barrier()
    dist.destroy_process_group()


def _accumulated_step(hp, dims, sd, feed):
    """One data-parallel step with per-rank batch-norm made by hand on ONE device: two plain nets run the backward pass on
    their shards, net 0 takes the sums ``DataParallel`` would exchange and applies the update -> its state dict."""
    from clsr_amd.dp import shard_feed
    from clsr_amd.net import CLSRNet

    nets, fs = [], []
    for r in range(2):
        net = CLSRNet(hp, dims, device="cuda:0", seed=0)
        net.load_state_dict(sd)
        net.dp_world = 2                                    # the data loss is scaled by 1 / (P * world)
        nets.append(net)
        fs.append(net.upload(shard_feed(feed, r, 2, hp.train_num_ngs + 1), True))
    denom = fs[0]["denom"] + fs[1]["denom"]                 # the contrastive denominator is global
    for net, f in zip(nets, fs):
        f["denom"].copy_(denom)
        net.train_step(f, apply=False)
        torch.cuda.synchronize()
    n0, n1 = nets
    n0.grad_flat.add_(n1.grad_flat)                         # dense gradients | gradient tables | moving statistics
    torch.maximum(n0.tab_flags_flat, n1.tab_flags_flat, out=n0.tab_flags_flat)
    n0.stats24.add_(n1.stats24)
    n0.bn_moving.mul_(0.5)
    n0._apply_updates()
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in n0.state_dict().items()}


def _jobs():
    jobs = [((tuple(s),), mode, overlap, False) for s, mode, overlap in ROUTINGS]
    jobs += [(tuple(tuple(s) for s in routes), mode, overlap, False) for routes, mode, overlap in SWAPS]
    jobs.append((("none",), "allgather", True, True))     # the oracle comparison: pre-clip gradients captured
    return jobs


def _golden_setup(golden_dir, golden_hparams):
    from oracle import clsr_oracle as O

    hp = copy.deepcopy(golden_hparams)
    dims = dict(Vu=len(pickle.load(open(hp.user_vocab, "rb"))), Vi=len(pickle.load(open(hp.item_vocab, "rb"))),
                Vc=len(pickle.load(open(hp.cate_vocab, "rb"))))
    g = np.load(os.path.join(golden_dir, "iterator_train_sa.npz"))
    feeds = [{k[3:]: g[k] for k in g.files if k.startswith("b%d_" % b)} for b in range(2)]
    params = O.init_params(dims, hp, seed=5, scale_dense=8.0)
    sd = dict(params)
    sd.update(O.init_bn_state(params))
    return hp, dims, feeds, params, sd


def _run_routings(golden_dir, golden_hparams):
    import torch.multiprocessing as mp

    hp, dims, feeds, params, sd = _golden_setup(golden_dir, golden_hparams)
    ref1 = _accumulated_step(hp, dims, sd, feeds[0])
    ref2 = _accumulated_step(hp, dims, ref1, feeds[1])
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    jobs = _jobs()
    mp.spawn(_routing_worker, args=(2, _free_port(), hp, dims, feeds, sd, jobs, out), nprocs=2, join=True)
    return dict(hp=hp, dims=dims, feeds=feeds, params=params, ref=[ref1, ref2], jobs=jobs, out=dict(out))


@pytest.fixture(scope="module")
def routed(golden_dir, golden_hparams):
    return _run_routings(golden_dir, golden_hparams)


def _assert_same_bits(got, ref, what):
    assert sorted(got) == sorted(ref), what
    for k in ref:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(np.asarray(ref[k]))
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k)
        if a.tobytes() != b.tobytes():
            af, bf = a.astype(np.float64), b.astype(np.float64)
            n = int((a.view(np.uint8) != b.view(np.uint8)).reshape(a.size, -1).any(1).sum()) if a.size else 0
            raise AssertionError("%s: %s differs in %d of %d elements, max |diff| %.3e (max |ref| %.3e)"
                                 % (what, k, n, a.size, float(np.abs(af - bf).max()), float(np.abs(bf).max())))


@pytest.mark.gpu
@pytest.mark.parametrize("j", range(len(ROUTINGS)), ids=["%s-%s-%s" % ("+".join(s) or "dense", m, "overlap" if o else "serial")
                                                         for s, m, o in ROUTINGS])
def test_exchange_equals_the_two_shard_accumulation_bit_for_bit(routed, j):
    """Parameters, Adam slots, clock and moving statistics of BOTH ranks after one step == the accumulation made by hand."""
    sparse = ROUTINGS[j][0]
    r0, r1 = routed["out"][(j, 0)], routed["out"][(j, 1)]
    assert sorted(r0["sparse"][0]) == sorted(sparse) == sorted(r1["sparse"][0])
    _assert_same_bits(r0["state"], {k: v.numpy() for k, v in routed["ref"][0].items()}, "rank 0 against the accumulation")
    _assert_same_bits(r1["state"], r0["state"], "rank 1 against rank 0")


@pytest.mark.gpu
@pytest.mark.parametrize("j", range(len(ROUTINGS) + len(SWAPS)))
def test_no_collective_covers_a_row_exchanged_table_and_every_other_piece_travels_once(routed, j):
    """Byte ranges of the SUM all-reduces of every step, on both ranks: dense gradients, dense tables and the moving
    statistics inside exactly one, the gradient table of a sparse route inside none (it is merged by its row exchange: a
    second sum doubles it, and a dense all-reduce of it is what the sparse route exists to avoid)."""
    for rank in (0, 1):
        assert routed["out"][(j, rank)]["coverage"] == [[]] * len(routed["jobs"][j][0]), (rank, routed["jobs"][j])


@pytest.mark.gpu
def test_dense_prefix_and_sparse_suffix_in_the_trace(routed):
    """{user_long, user_short} sparse: the issue order the stepper reports -- the two row exchanges, ONE collective for
    [dense gradients | item | cate], the moving statistics on their own, and no collective named after a user table."""
    j = ROUTINGS.index((("user_long", "user_short"), "allgather", True))
    for rank in (0, 1):
        trace = routed["out"][(j, rank)]["trace"][0]
        what = [d for e, d in trace if e == "collective"]
        assert sorted(w for w in what if w != "flags") == sorted(
            ["rows:user_long", "rows:user_short", "dense+tables:item+cate", "small", "bn_moving"]), what
        assert what.count("flags") == 1                      # item + cate: adjacent byte maps, one MAX all-reduce
        assert [e for e, _ in trace if e == "finish"] == ["finish"]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(SWAPS)), ids=["users-then-item", "item-then-users"])
def test_two_steps_with_the_routing_changed_in_between(routed, k):
    """``dp.sparse_tables`` reassigned between two steps on two batches: a table that was row-exchanged travels dense in the
    next step and the other way round -- against the accumulation carried over two steps, bit for bit."""
    j = len(ROUTINGS) + k
    r0, r1 = routed["out"][(j, 0)], routed["out"][(j, 1)]
    assert [sorted(s) for s in r0["sparse"]] == [sorted(s) for s in SWAPS[k][0]]
    _assert_same_bits(r0["state"], {k_: v.numpy() for k_, v in routed["ref"][1].items()}, "rank 0 against the accumulation")
    _assert_same_bits(r1["state"], r0["state"], "rank 1 against rank 0")


# ---- per-rank batch-norm against the float64 oracle
def _sharded_oracle(hp, feeds0, params, dtype):
    from clsr_amd.dp import shard_feed
    from oracle import clsr_oracle as O

    p = type(params)((k, v.to(dtype)) for k, v in params.items())
    shards = [O.to_torch_feed(shard_feed(feeds0, r, 2, hp.train_num_ngs + 1), dtype=dtype) for r in range(2)]
    return O.sharded_gradients(p, O.init_bn_state(p), shards, hp)


def _sharded_step_distances(got_losses, got_dense, got_tables, got_moving, ref, label):
    """Distances of one per-rank-BN step from the float64 sharded oracle, printed, then held to the bars of the sync-BN test
    (test_two_ranks_match_single_process): losses 1e-5 * max(1, |ref|); gradients 2e-3 * max|ref| + a floor of 1e-6 * the
    largest dense gradient; moving statistics rtol 1e-4, atol 1e-6.  -> the worst ratios distance / bar."""
    from oracle.clsr_oracle import TABLES

    ls, raw, moving = ref
    worst, worst_key = dict(loss=0.0, grad=0.0, moving=0.0), ""
    fails = []
    for k in ("loss", "data_loss", "contrastive_loss", "regular_loss", "discrepancy_loss"):
        r = float(ls[k])
        ratio = abs(float(got_losses[k]) - r) / (1e-5 * max(1.0, abs(r)))
        worst["loss"] = max(worst["loss"], ratio)
        if not ratio < 1.0:
            fails.append((k, float(got_losses[k]), r))
    dense = {k: v for k, v in raw.items() if k not in TABLES.values()}
    floor = 1e-6 * max(float(v.abs().max()) for v in dense.values())
    for k, g in list(got_dense.items()) + [(TABLES[k], g) for k, g in got_tables.items()]:
        v = raw[k].double().numpy()
        d = float(np.abs(np.asarray(g, dtype=np.float64) - v).max())
        ratio = d / (2e-3 * float(np.abs(v).max()) + floor)
        if ratio > worst["grad"]:
            worst["grad"], worst_key = ratio, "%s: %.3e of max |ref| %.3e" % (k, d, float(np.abs(v).max()))
        if not ratio <= 1.0:
            fails.append((k, d, float(np.abs(v).max())))
    assert sorted(got_dense) == sorted(dense) and len(got_tables) == 4
    for k, v in moving.items():
        v = v.double().numpy()
        d = np.abs(np.asarray(got_moving[k], dtype=np.float64) - v)
        ratio = float((d / (1e-6 + 1e-4 * np.abs(v))).max())
        worst["moving"] = max(worst["moving"], ratio)
        if not ratio <= 1.0:
            fails.append((k, float(d.max())))
    print("[%s] worst distance from the float64 sharded oracle as a fraction of its bar: losses %.3g, gradients %.3g, "
          "moving statistics %.3g; worst gradient %s" % (label, worst["loss"], worst["grad"], worst["moving"], worst_key))
    assert not fails, fails
    return worst


def test_float32_oracle_of_the_sharded_step_is_inside_the_bars(golden_dir, golden_hparams):
    """The reference alone: the sharded oracle in float32 against itself in float64 (CPU) stays inside the bars the HIP step
    is held to."""
    from oracle.clsr_oracle import TABLES

    hp, dims, feeds, params, sd = _golden_setup(golden_dir, golden_hparams)
    ref = _sharded_oracle(hp, feeds[0], params, torch.float64)
    ls, raw, moving = _sharded_oracle(hp, feeds[0], params, torch.float32)
    keys = {v: k for k, v in TABLES.items()}
    worst = _sharded_step_distances({k: float(v) for k, v in ls.items()},
                                    {k: v.numpy() for k, v in raw.items() if k not in keys},
                                    {keys[k]: v.numpy() for k, v in raw.items() if k in keys},
                                    {k: v.numpy() for k, v in moving.items()}, ref, "float32 oracle")
    assert max(worst.values()) <= 1.0


def test_sharded_oracle_of_one_shard_is_the_plain_oracle(golden_dir, golden_hparams):
    from oracle import clsr_oracle as O

    hp, dims, feeds, params, sd = _golden_setup(golden_dir, golden_hparams)
    p = type(params)((k, v.double()) for k, v in params.items())
    feed = O.to_torch_feed(feeds[0], dtype=torch.float64)
    ls, raw, moving = O.sharded_gradients(p, O.init_bn_state(p), [feed], hp)
    ls1, _, _, new_bn, out = O.gradients(p, O.init_bn_state(p), feed, hp)
    for k in ls1:
        assert abs(float(ls[k]) - float(ls1[k])) < 1e-12, k
    for k, v in out["raw_grads"].items():
        assert float((raw[k] - v).abs().max()) < 1e-12, k
    for k, v in new_bn.items():
        assert float((moving[k] - v).abs().max()) == 0.0, k


@pytest.mark.gpu
def test_per_rank_batch_norm_step_matches_the_sharded_float64_oracle(routed):
    """``sync_bn=False``: losses (data loss scaled by 1 / (P * world), global contrastive denominator, regularisers and
    discrepancy counted once over the merged rows), summed gradients and averaged moving statistics of a two-rank step
    against the float64 oracle run on each shard with its own batch statistics."""
    j = len(routed["jobs"]) - 1
    r0, r1 = routed["out"][(j, 0)], routed["out"][(j, 1)]
    assert r0["sparse"] == [[]]
    ref = _sharded_oracle(routed["hp"], routed["feeds"][0], routed["params"], torch.float64)
    moving = {k: v for k, v in r0["state"].items() if k.endswith("moving_mean") or k.endswith("moving_variance")}
    assert sorted(moving) == sorted(ref[2])
    _sharded_step_distances(r0["losses"], r0["grads"], r0["tgrads"], moving, ref, "HIP step, two ranks")
    _assert_same_bits(r1["state"], r0["state"], "rank 1 against rank 0")


# ---- capture() == train_step()
def _capture_worker(rank, world, port, hp, dims, feed, sd, out):
    from clsr_amd import ops
    from clsr_amd.dp import DataParallel, shard_feed
    from clsr_amd.net import CLSRNet

    dist, staged, dev = _init(rank, world, port)
    shard = shard_feed(feed, rank, world, hp.train_num_ngs + 1)

    def fresh(**kw):
        net = CLSRNet(hp, dims, device=dev, seed=rank)
        if rank == 0:
            net.load_state_dict(sd)
        return net, DataParallel(net, staged, **kw)

    res = {}
    for how in ("graphs", "eager"):
        net, dp = fresh(sync_bn=False, overlap=False)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            f = dp.prepare(net.upload(shard, True))
            for _ in range(2):                  # buffers allocated, weights packed: a capture must not allocate
                dp.train_step(f)
                torch.cuda.synchronize()
            if how == "graphs":
                run = dp.capture(f)             # (recorded only: nothing executes during the capture)
                assert dp._graphs is not None and len(dp._graphs) == 2
            else:
                run = lambda: dp.train_step(f)
            for _ in range(3):
                run()
                torch.cuda.synchronize()
        assert float(net.adam_state[0]) == 5.0
        res[how] = _state(net)
        dp.close()
    # with sync-BN (collectives inside the backward pass) or the overlapped exchange, capture() hands back the eager step
    begin = ops.graph_begin

    def no_graph(*a, **k):
        raise AssertionError("capture() opened a stream capture")

    ops.graph_begin = no_graph
    try:
        for kw in (dict(sync_bn=True, overlap=False, p2p_stats=False), dict(sync_bn=False, overlap=True)):
            net, dp = fresh(**kw)
            f = dp.prepare(net.upload(shard, True))
            run = dp.capture(f)
            assert dp._graphs is None
            dp.trace = []
            run()
            torch.cuda.synchronize()
            assert float(net.adam_state[0]) == 1.0 and [e for e, _ in dp.trace if e == "finish"] == ["finish"]
            dp.close()
    finally:
        ops.graph_begin = begin
    out[rank] = res
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_captured_step_equals_train_step(golden_dir, golden_hparams):
    """Per-rank batch-norm, exchange behind the backward pass: three steps through ``run = dp.capture(f)`` (backward graph |
    eager exchange | update graph) leave both ranks in the state three ``dp.train_step(f)`` leave an identically initialised
    pair in, bit for bit.  Both pairs run two eager steps first: the first steps allocate their buffers, which a stream
    capture must not do."""
    import torch.multiprocessing as mp

    hp, dims, feeds, params, sd = _golden_setup(golden_dir, golden_hparams)
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    mp.spawn(_capture_worker, args=(2, _free_port(), hp, dims, feeds[0], sd, out), nprocs=2, join=True)
    for rank in (0, 1):
        _assert_same_bits(out[rank]["graphs"], out[rank]["eager"], "rank %d: captured against eager" % rank)
    _assert_same_bits(out[1]["graphs"], out[0]["graphs"], "rank 1 against rank 0")
