"""GPU tests of the evaluation sharded over data-parallel ranks: the partial metric kernels (clsr_eval_*_part +
clsr_eval_finalize, clsr_amd/csrc/metrics.hip) against the whole ones, ``device_metrics.compute(part=..., reduce=...)``
with simulated ranks, and ``CLSRModel(dist=..., shard_eval=True)`` with two and three rank processes on one GPU
(transports as in tests/test_dp_gpu.py).  Everything is compared for EQUALITY: integer sums commute.

Wait bound of the spawned ranks: tests/test_dp_gpu.py::test_model_train_with_two_ranks_matches_single_process[staged]
(two ranks with the same start-up: spawn, import torch, load the library, gloo rendezvous) takes 3.3 s on the MI355X
box of the suite; the rank tests here (two or three ranks sharing the GPU, three evaluations of 200 - 400 lines each)
take 2.5 - 4.3 s there.  WAIT_S = 120 s is 36 times the measurement: start-up of a rank dominates and grows with a
cold file cache or a loaded box, not with this code.  When the bound expires the ranks
are ended and the test fails."""
import ctypes
import json
import os
import pickle
import socket
import time
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from clsr_amd import device_metrics as DM  # noqa: E402
from clsr_amd import ops  # noqa: E402
from clsr_amd.dp import HostStagedDist  # noqa: E402

DEV = "cuda:0"
WAIT_S = 120.0
KS = [1, 2, 3, 5, 10, 64, 100, 5000]      # GM_MAXK = 8 distinct k
I64, F64, I32, F32 = torch.int64, torch.float64, torch.int32, torch.float32
FX_LOGLOSS, FX_GROUP, FX_USER, FX_POINT = 0, 1, 2, 3


# ------------------------------------------------------------------------------ 1. partial kernels == whole kernels
def _case(name):
    """-> dict(pred, labels, users, alpha [N]; G, n_groups for the group kernel (the first n_groups * G lines);
    only: the entries to run, None = all)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    only = None
    if name in ("groups7x5", "groups2x5", "wide2x4096"):
        n_groups, G = {"groups7x5": (7, 5), "groups2x5": (2, 5), "wide2x4096": (2, 4096)}[name]
        N = n_groups * G
        labels = (rng.random(N) < 0.2).astype(np.float32)
        labels[::G] = 1.0
        labels[G - 1::G] = 0.0
        if name == "groups7x5":
            labels[5:10] = 0.0                                       # a group without a positive: err
        users = np.repeat(rng.integers(0, 3 if G == 5 else 50, n_groups * (1 if G == 5 else 64)), G if G == 5 else 64)
        preds = np.round(rng.random(N), 1 if G == 5 else 3)          # ties inside groups and users
    elif name == "heavy_user":
        # one user with ~80 % of the lines, many one- and two-line users, a user without a positive, ids above 2^18
        ids = rng.choice(np.arange(1 << 18, 1 << 30), 400, replace=False)
        users = [ids[0]] * 2400 + list(ids[1:220]) + 2 * list(ids[220:399]) + [ids[399]] * 5 + [7, 7, 7, 262143, 262144]
        labels = (rng.random(len(users)) < 0.3).astype(np.float32)
        labels[np.asarray(users) == ids[399]] = 0.0                  # (the NaN path of wmrr / wndcg)
        order = rng.permutation(len(users))
        users, labels = np.asarray(users)[order], labels[order]
        N, G = len(users), 5
        n_groups = N // G
        preds = np.round(rng.random(N), 2)
        assert N % 2 and N % 3 and N % 5 and (users == ids[0]).mean() > 0.79
    elif name == "lines70k":
        # the line loops stride more than once; 35 003 groups of 2 and ~40 000 users: more than one wave per 16 384 waves
        N, G = 70007, 2
        n_groups = N // G
        users = rng.integers(0, 40000, N) * 53687 % ((1 << 31) - 1)
        labels = (rng.random(N) < 0.3).astype(np.float32)
        preds = np.round(rng.random(N), 3)
    else:
        # 4096 blocks of the pair-count kernel cover 4 194 304 lines: beyond that its line loop strides (lines only)
        assert name == "lines4m"
        N, G, n_groups, only = 4096 * 1024 + 4099, 1, 0, ("logloss", "auc", "point")
        users = np.zeros(N, dtype=np.int64)
        labels = (rng.random(N) < 0.0006).astype(np.float32)
        preds = np.round(rng.random(N), 3)
        assert labels.sum() > 2048                                   # (more positives than one LDS tile)
    t = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt, device=DEV)
    return dict(N=N, G=G, n_groups=n_groups, only=only, pred=t(preds, F32), labels=t(labels, F32),
                users=t(np.asarray(users, dtype=np.int64), I32), alpha=t(rng.random(N), F32))


def _segments(c):
    """keys, perm (stable sort: the same every time), starts (compacted through an atomic cursor: any order), count"""
    N = c["N"]
    keys, perm = torch.empty(N, dtype=I32, device=DEV), torch.empty(N, dtype=I32, device=DEV)
    ws = torch.empty(ops.query("clsr_sort_ids_stable_workspace_bytes", N, 1), dtype=torch.uint8, device=DEV)
    ops.sort_ids_stable_multi([(c["users"].data_ptr(), keys.data_ptr(), perm.data_ptr(), N, 1, 1, 31)], ws)
    starts, nseg = torch.empty(N, dtype=I32, device=DEV), torch.zeros(1, dtype=I32, device=DEV)
    ops.call("clsr_eval_user_segments", keys, N, starts, nseg)
    return keys, perm, starts, nseg


def _positives(c):
    pos, cnt = torch.empty(c["N"], dtype=F32, device=DEV), torch.zeros(1, dtype=I32, device=DEV)
    ops.call("clsr_eval_compact_pos", c["pred"], c["labels"], c["N"], pos, cnt)
    return pos, cnt


USER_FORMS = {"user": (1, 1), "user_auc": (1, 0), "user_rank": (0, 1)}       # the three template instances


def _entries(c):
    names = ["logloss", "auc", "point", "group"] + list(USER_FORMS)
    return [n for n in names if c["only"] is None or n in c["only"]]


def _whole(c):
    """-> {entry: [int64 tensors: the bits of every output, err counters included]} of the existing entries"""
    N, pred, labels = c["N"], c["pred"], c["labels"]
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=DEV)
    karr = (ctypes.c_int * 8)(*KS)
    out = {}
    for name in _entries(c):
        if name == "logloss":
            o = z(1, F64)
            ops.call("clsr_eval_logloss", pred, labels, N, o)
            out[name] = [o.view(I64)]
        elif name == "auc":
            pos, cnt = _positives(c)
            u = z(3, I64)
            ops.call("clsr_eval_auc_pairs", pred, labels, N, pos, cnt, u)
            out[name] = [u]
        elif name == "point":
            d, u = z(3, F64), z(4, I64)
            ops.call("clsr_eval_point_stats", pred, labels, c["alpha"], N, d, u)
            out[name] = [d.view(I64), u]
        elif name == "group":
            o, e = z(18, F64), z(1, I32)
            ops.call("clsr_eval_group_metrics", pred, labels, c["n_groups"], c["G"], ctypes.addressof(karr), 8, 1, o, e)
            out[name] = [o.view(I64), e.to(I64)]
        else:
            want_auc, want_rank = USER_FORMS[name]
            keys, perm, starts, nseg = _segments(c)
            o, e = z(18, F64), z(2, I32)
            ops.call("clsr_eval_user_metrics", pred, labels, perm, keys, starts, nseg, N, ctypes.addressof(karr),
                     8 if want_rank else 0, want_auc, want_rank, o, e)
            out[name] = [o.view(I64), e.to(I64)]
    return {k: [t.cpu() for t in v] for k, v in out.items()}


def _parts(c, nparts):
    """The same through the partial entries: every part in buffers of its own and with its own compaction of the
    positives and of the segment starts (as on a rank of its own), the raw integers added, then finalized."""
    N, pred, labels = c["N"], c["pred"], c["labels"]
    z = lambda n: torch.zeros(n, dtype=I64, device=DEV)
    karr = (ctypes.c_int * 8)(*KS)
    out = {}
    for name in _entries(c):
        sums = None
        for part in range(nparts):
            if name == "logloss":
                bufs = [z(1)]
                ops.call("clsr_eval_logloss_part", pred, labels, N, part, nparts, bufs[0])
            elif name == "auc":
                pos, cnt = _positives(c)
                bufs = [z(3)]
                ops.call("clsr_eval_auc_pairs_part", pred, labels, N, pos, cnt, part, nparts, bufs[0])
            elif name == "point":
                bufs = [z(3), z(4)]
                ops.call("clsr_eval_point_stats_part", pred, labels, c["alpha"], N, part, nparts, bufs[0], bufs[1])
            elif name == "group":
                bufs = [z(18), z(1)]
                ops.call("clsr_eval_group_metrics_part", pred, labels, c["n_groups"], c["G"], ctypes.addressof(karr), 8,
                         1, part, nparts, bufs[0], bufs[1])
            else:
                want_auc, want_rank = USER_FORMS[name]
                keys, perm, starts, nseg = _segments(c)
                bufs = [z(18), z(2)]
                ops.call("clsr_eval_user_metrics_part", pred, labels, perm, keys, starts, nseg, N,
                         ctypes.addressof(karr), 8 if want_rank else 0, want_auc, want_rank, part, nparts, bufs[0],
                         bufs[1])
            sums = bufs if sums is None else [a + b for a, b in zip(sums, bufs)]
        if name != "auc":
            n, scale = {"logloss": (1, FX_LOGLOSS), "point": (3, FX_POINT), "group": (18, FX_GROUP)}.get(name, (18, FX_USER))
            ops.call("clsr_eval_finalize", sums[0], n, scale)
        out[name] = sums
    return {k: [t.cpu() for t in v] for k, v in out.items()}


CASES = ["groups7x5", "groups2x5", "wide2x4096", "heavy_user", "lines70k", "lines4m"]


@pytest.fixture(scope="module")
def kernel_cases():
    """case -> (buffers, outputs of the whole entries): built on first use, shared by the nparts of a case"""
    made = {}

    def get(name):
        if name not in made:
            c = _case(name)
            made[name] = (c, _whole(c))
        return made[name]
    return get


def _assert_same_bits(got, exp, what):
    assert set(got) == set(exp)
    for name in exp:
        for i, (a, b) in enumerate(zip(got[name], exp[name])):
            assert torch.equal(a, b), (what, name, i, a.tolist(), b.tolist())


@pytest.mark.parametrize("nparts", [1, 2, 3, 5])
@pytest.mark.parametrize("case", CASES)
def test_partial_kernels_add_up_to_the_whole_kernels(kernel_cases, case, nparts):
    c, whole = kernel_cases(case)
    _assert_same_bits(_parts(c, nparts), whole, (case, nparts))
    if case in ("heavy_user", "lines70k"):
        # the list of segment starts is compacted through an atomic cursor, in a new order every time: a share that
        # depended on a position in it would count some users twice and drop others in one run or the other
        _assert_same_bits(_parts(c, nparts), whole, (case, nparts, "second run"))


def test_cases_are_not_degenerate(kernel_cases):
    c, whole = kernel_cases("heavy_user")
    assert whole["user"][1].tolist()[1] >= 1 and whole["user"][1].tolist()[0] >= 1      # users without a positive; one-class users
    assert whole["group"][1].tolist()[0] >= 1                                               # groups without a positive
    assert all(int(v) != 0 for v in whole["user"][0].tolist()[:2]) and all(int(v) != 0 for v in whole["auc"][0].tolist())
    c, whole = kernel_cases("groups2x5")
    assert c["n_groups"] == 2 and int(whole["group"][0][0]) != 0


def test_partial_entries_check_their_share():
    c = _case("groups2x5")
    for part, nparts in [(2, 2), (-1, 2), (0, 0)]:
        with pytest.raises(Exception, match="invalid argument"):
            ops.call("clsr_eval_logloss_part", c["pred"], c["labels"], c["N"], part, nparts,
                     torch.zeros(1, dtype=I64, device=DEV))


# ------------------------------------------------------------------------------ 2. compute(part=..., reduce=...)
ALL_METRICS = dict(metrics=["auc", "logloss", "rmse", "acc", "f1"],
                   pairwise_metrics=["mean_mrr", "group_auc", "ndcg@1;2;3;5;10;64;100;5000", "hit@1;2;3;5;10;64;100;5000"],
                   weighted_metrics=["wauc", "wmrr", "whit@1;2;3;5;10;64;100;5000", "wndcg@1;2;3;5;10;64;100;5000"])


class _Captured(Exception):
    pass


def _simulated_rank(scores, hp, group, rank, world, raw, **kw):
    """compute() as rank ``rank`` sees it: ``reduce`` runs the partial computes of the other ranks (each stopped at ITS
    reduce, where its accumulators are taken) and adds their tensors, as an integer all-reduce would."""
    calls = []

    def reduce(tensors):
        calls.append(len(tensors))
        for other in range(world):
            if other == rank:
                continue

            def capture(ts):
                raise _Captured([t.clone() for t in ts])
            try:
                DM.compute(scores, hp, group, True, part=(other, world), reduce=capture, **kw)
                raise AssertionError("compute did not call reduce")
            except _Captured as c:
                theirs = c.args[0]
            assert len(theirs) == len(tensors)
            for mine, t in zip(tensors, theirs):
                assert mine.dtype == torch.int64 and t.dtype == torch.int64 and mine.is_cuda
                mine += t
    res = DM.compute(scores, hp, group, True, raw=raw, part=(rank, world), reduce=reduce, **kw)
    assert len(calls) == 1                                        # reduce is called ONCE
    return res


def _scores(preds, labels, users, alpha):
    acc = DM.DeviceScores(torch.device(DEV))
    acc.append(torch.tensor(preds, dtype=F32, device=DEV), torch.tensor(labels, dtype=F32, device=DEV),
               torch.tensor(np.asarray(users, dtype=np.int64), dtype=I32, device=DEV),
               torch.tensor(alpha, dtype=F32, device=DEV))
    return acc


@pytest.fixture(scope="module")
def metric_files(golden_dir):
    """name -> (scores, group, whole-process dict, whole-process raw dict); every metric the device computes requested"""
    hp = types.SimpleNamespace(**ALL_METRICS)
    g = json.load(open(os.path.join(golden_dir, "metrics_golden.json")))
    labels = np.asarray(g["labels"], dtype=np.float64)
    rng = np.random.default_rng(12)
    files = {"golden": (np.asarray(g["preds"], dtype=np.float64).reshape(-1), labels.reshape(-1),
                        np.asarray(g["users"]).astype(np.int64), labels.shape[1])}
    n_groups, G = 1201, 5                                           # 6005 lines: no multiple of 2 x 3 x 256
    lab = np.zeros((n_groups, G))
    lab[:, 0] = 1.0
    lab = np.maximum(lab, (rng.random((n_groups, G)) < 0.05) * (np.arange(G) < G - 1))
    files["random"] = (np.round(rng.random(n_groups * G), 2), lab.reshape(-1),
                       np.repeat(rng.integers(0, 1 << 22, 300)[rng.integers(0, 300, n_groups)], G), G)
    out = {}
    for name, (preds, labels, users, group) in files.items():
        scores = _scores(preds, labels, users, rng.random(len(preds)))
        raw = {}
        out[name] = (scores, group, DM.compute(scores, hp, group, True, raw=raw, mean_alpha=True), raw)
    return hp, out, g["expected"]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["golden", "random"])
def test_compute_with_simulated_ranks_equals_the_whole_compute(metric_files, name, world):
    hp, files, expected = metric_files
    scores, group, whole, whole_raw = files[name]
    assert len(whole) == 5 + 2 + 16 + 2 + 16 + 1
    for rank in range(world):
        raw = {}
        got = _simulated_rank(scores, hp, group, rank, world, raw, mean_alpha=True)
        # (NaN-free: every user of both files has a positive line)
        assert got == whole and raw == whole_raw, (rank, got, whole)
    if name == "golden":
        # the reference-captured answers, where tests/test_device_metrics*_gpu.py use them (tie-exact metrics)
        for k in ("auc", "logloss", "group_auc", "wauc"):
            assert abs(got[k] - expected[k]) < 1e-9, (k, got[k], expected[k])
        assert got["whit@1"] == expected["whit@1"] and got["whit@2"] == expected["whit@2"]


def test_part_of_a_world_of_one_needs_no_reduce_and_more_ranks_do(metric_files):
    hp, files, _ = metric_files
    scores, group, whole, whole_raw = files["random"]
    raw = {}
    assert DM.compute(scores, hp, group, True, raw=raw, mean_alpha=True, part=(0, 1)) == whole and raw == whole_raw
    with pytest.raises(ValueError):
        DM.compute(scores, hp, group, True, part=(0, 2))
    with pytest.raises(ValueError):
        DM.compute(scores, hp, group, True, part=(2, 2), reduce=lambda ts: None)


def test_merge_puts_every_line_on_every_rank_bit_for_bit():
    """Three simulated ranks: each appends its own chunks and zeros elsewhere; the integer sum restores all columns."""
    rng = np.random.default_rng(5)
    n = 1000
    cols = [torch.tensor(rng.standard_normal(n), dtype=F32, device=DEV), torch.tensor(rng.random(n) < 0.3, dtype=F32, device=DEV),
            torch.tensor(rng.integers(0, 1 << 31, n), dtype=I32, device=DEV), torch.tensor(-rng.random(n), dtype=F32, device=DEV)]
    cols[0][:3] = torch.tensor([float("inf"), -0.0, 1e-42], device=DEV)         # bit patterns a float sum would not keep
    sizes = [64, 64, 7, 200, 64, 1, 600]
    plan = DM.plan_chunks(sizes, 3)
    ranks = []
    for r in range(3):
        s = DM.DeviceScores(torch.device(DEV))
        for off, m, owner in plan:
            if owner == r:
                s.append(*[c[off:off + m] for c in cols])
            else:
                s.append_zeros(m, True)
        ranks.append(s)
    packed = []
    for s in ranks:                      # every rank's packed buffer, stopped at the reduce
        def capture(ts):
            raise _Captured([t.clone() for t in ts])
        with pytest.raises(_Captured) as e:
            s.merge(capture)
        packed.append(e.value.args[0])
    total = [sum(p[i] for p in packed) for i in range(len(packed[0]))]
    for s in ranks:
        s.merge(lambda ts: [t.copy_(x) for t, x in zip(ts, total)])
        for got, exp in zip((s.pred, s.labels, s.users, s.alpha), cols):
            assert torch.equal(got[:n].view(I32), exp.view(I32))


# ------------------------------------------------------------------------------ 3. rank processes
def _worlds_and_transports():
    return [p for world in (2, 3) for p in (
        pytest.param(world, "staged", id="%d-staged" % world),
        pytest.param(world, "nccl", id="%d-nccl" % world,
                     marks=pytest.mark.skipif(torch.cuda.device_count() < world, reason="RCCL needs one GPU per rank")))]


def _init(transport, rank, world, port):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if transport == "nccl":
        torch.cuda.set_device(rank)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
        return dist, "cuda:%d" % rank
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return HostStagedDist(dist), "cuda:0"


def _build(kind, hp, sd, seed, **kw):
    import clsr_amd.clsr as M
    from clsr_amd.sequential_iterator import SASequentialIterator, SequentialIterator

    model = (M.CLSRModel(hp, SASequentialIterator, seed=seed, **kw) if kind == "clsr" else
             M.SLI_RECModel(hp, SequentialIterator, seed=seed, **kw))
    model.net.load_state_dict(sd)
    return model


def _evaluate(model, jobs):
    """jobs: [(method, file, num_ngs, kwargs)] -> [(result dict, lines this rank scored, entry points called)]"""
    real, out = ops.call, []
    for method, path, ngs, kw in jobs:
        names = []

        def spy(name, *a, **k):
            names.append(name)
            return real(name, *a, **k)
        ops.call = spy
        try:
            res = getattr(model, method)(path, ngs, **kw)
        finally:
            ops.call = real
        out.append((res, model.eval_rows_scored, sorted({n for n in names if n.startswith("clsr_eval")})))
    return out


def _rank_worker(rank, world, port, transport, kind, hp, sd, jobs, shard, out):
    import torch.distributed as dist

    d, dev = _init(transport, rank, world, port)
    kw = dict(shard_eval=True) if shard else {}                   # (default behaviour: the keyword is not passed at all)
    model = _build(kind, hp, sd, 100 + rank, dist=d, device=dev, **kw)
    out[rank] = _evaluate(model, jobs)
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


def _run_ranks(world, transport, kind, hp, sd, jobs, shard=True):
    """Spawn the ranks and wait for them with a bound; on expiry they are ended and the test fails."""
    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = mp.get_context("spawn").Manager().dict()
    pc = mp.spawn(_rank_worker, args=(world, port, transport, kind, hp, sd, jobs, shard, out), nprocs=world, join=False)
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
    return [out[r] for r in range(world)]


ALL_W = ["wauc", "wmrr", "whit@1;2", "wndcg@1;2"]


@pytest.fixture(scope="module")
def eval_setup(golden_dir, golden_hparams, tmp_path_factory):
    """Models' hparams and weights, the evaluation jobs and the single-process answers (computed once, with the same
    small scoring chunks the ranks use: 64 lines, batches of 12 lines, so chunk boundaries fall inside groups of 5)."""
    from clsr_amd.deeprec_utils import HParams
    from oracle import clsr_oracle, sibling_oracle

    data = os.path.join(golden_dir, "data")
    valid, test = os.path.join(data, "valid_data"), os.path.join(data, "test_data")
    short = str(tmp_path_factory.mktemp("shard_eval") / "two_groups")      # 10 lines: one chunk
    with open(short, "w") as f:
        f.writelines(open(valid).readlines()[:10])
    base = dict(golden_hparams.values(), batch_size=12, weighted_metrics=ALL_W,
                metrics=["auc", "logloss", "rmse", "acc", "f1"])
    hps = {"clsr": HParams(**base),
           "sli_rec": HParams(**dict(base, model_type="sli_rec", user_embedding_dim=16, attention_size=40))}
    dims = dict(Vu=len(pickle.load(open(base["user_vocab"], "rb"))), Vi=len(pickle.load(open(base["item_vocab"], "rb"))),
                Vc=len(pickle.load(open(base["cate_vocab"], "rb"))))
    sds = {}
    for kind, params in (("clsr", clsr_oracle.init_params(dims, hps["clsr"], seed=5, scale_dense=8.0)),
                         ("sli_rec", sibling_oracle.init_params(dims, hps["sli_rec"], "sli_rec", seed=5, scale_dense=8.0))):
        oracle = clsr_oracle if kind == "clsr" else sibling_oracle
        sds[kind] = dict(params)
        sds[kind].update(oracle.init_bn_state(params))
    jobs = {"files": [("run_weighted_eval", valid, 4, {}), ("run_eval", test, 9, {}),
                      ("run_weighted_eval", valid, 4, dict(calc_mean_alpha=True))],
            "short": [("run_weighted_eval", short, 4, {})]}
    lines = {valid: 200, test: 400, short: 10}
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("CLSR_EVAL_ROWS", "64")
        single = {}
        for kind in hps:
            model = _build(kind, hps[kind], sds[kind], 0)
            for which in jobs:
                single[kind, which] = _evaluate(model, jobs[which])
        yield types.SimpleNamespace(hps=hps, sds=sds, jobs=jobs, lines=lines, single=single)


def _check_ranks(setup, kind, which, ranks, sharded):
    jobs, single = setup.jobs[which], setup.single[kind, which]
    for j, (method, path, ngs, kw) in enumerate(jobs):
        N, (exp, exp_rows, exp_names) = setup.lines[path], single[j]
        assert exp_rows == N and not any(n.endswith("_part") or n == "clsr_eval_finalize" for n in exp_names)
        assert ("mean_alpha" in exp) == bool(kw) and "auc" in exp and ("wmrr" in exp) == (method == "run_weighted_eval")
        for rank, res in enumerate(ranks):
            got, rows, names = res[j]
            assert got == exp, (method, path, rank, got, exp)
            if sharded:
                assert any(n.endswith("_part") for n in names) and "clsr_eval_finalize" in names
            else:
                assert rows == N and names == exp_names       # every rank scores everything, with today's launches
        if sharded:
            assert sum(res[j][1] for res in ranks) == N, [res[j][1] for res in ranks]


@pytest.mark.parametrize("world,transport", _worlds_and_transports())
def test_ranks_share_evaluation_and_get_the_single_process_metrics(eval_setup, world, transport):
    ranks = _run_ranks(world, transport, "clsr", eval_setup.hps["clsr"], eval_setup.sds["clsr"], eval_setup.jobs["files"])
    _check_ranks(eval_setup, "clsr", "files", ranks, True)
    for j, (_, path, _, _) in enumerate(eval_setup.jobs["files"]):
        for res in ranks:
            assert 0 < res[j][1] < eval_setup.lines[path]           # every rank scored a share, none the whole file


def test_fewer_chunks_than_ranks_leave_a_rank_without_lines(eval_setup):
    ranks = _run_ranks(2, "staged", "clsr", eval_setup.hps["clsr"], eval_setup.sds["clsr"], eval_setup.jobs["short"])
    _check_ranks(eval_setup, "clsr", "short", ranks, True)
    assert [res[0][1] for res in ranks] == [10, 0]


def test_sibling_model_with_an_alpha_column_shares_evaluation(eval_setup):
    ranks = _run_ranks(2, "staged", "sli_rec", eval_setup.hps["sli_rec"], eval_setup.sds["sli_rec"], eval_setup.jobs["files"])
    _check_ranks(eval_setup, "sli_rec", "files", ranks, True)
    assert all(0 < res[2][1] < 200 for res in ranks)


def test_without_the_keyword_every_rank_scores_everything(eval_setup):
    ranks = _run_ranks(2, "staged", "clsr", eval_setup.hps["clsr"], eval_setup.sds["clsr"], eval_setup.jobs["files"],
                       shard=False)
    _check_ranks(eval_setup, "clsr", "files", ranks, False)
