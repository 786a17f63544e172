"""The host side of ``run_catalogue_eval``: the rank oracle against the selection oracle and against ``cal_metric``, the chunk
choice, the new entry points of csrc/reco.hip as the header declares them, the method on every model class."""
import os

import numpy as np
import pytest

import rank_oracle as KO
import reco_oracle as RO


def _tied_case(seed, N, M, T):
    """Scores from four values (both zeros among them), distinct ascending ids, targets that are catalogue items, histories
    drawn partly from the catalogue and sometimes holding the target."""
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(np.arange(1, 4 * M + 2), size=M, replace=False)).astype(np.int32)
    scores = rng.choice(np.asarray([0.0, -0.0, 1.5, -2.0], dtype=np.float32), size=(N, M))
    col = rng.integers(0, M, N)
    hist = np.where(rng.random((N, T)) < 0.4, rng.choice(ids, size=(N, T)), 0).astype(np.int32)
    hist[::3, 0] = ids[col[::3]]        # every third request has its target in its history
    return scores, ids, col, hist


@pytest.mark.parametrize("seed", range(6))
def test_rank_is_the_place_of_the_target_in_the_full_sort(seed):
    N, M, T = 7, 61, 9
    scores, ids, col, hist = _tied_case(seed, N, M, T)
    ts, ti = scores[np.arange(N), col], ids[col]
    b = RO.bits(scores)
    assert (b == 0x80000000).any() and (b == 0).any()
    for use_seen in (False, True):
        # the target is never dropped: take it out of what the selection oracle removes
        seen = [set(r.tolist()) - {int(t)} for r, t in zip(hist, ti)] if use_seen else None
        full_i, _ = RO.topk(scores, ids, M, seen=seen)
        got = KO.ranks(scores, ids, ts, ti, seen=[set(r.tolist()) for r in hist] if use_seen else None)
        assert got.dtype == np.int32
        for n in range(N):
            assert int(got[n]) == full_i[n].tolist().index(int(ti[n])) + 1
    # many ties at the target: most candidates compare equal to some target
    assert (scores == ts[:, None]).mean() > 0.2


def test_oracle_on_a_hand_checked_case():
    ids = np.array([2, 3, 5, 7, 11, 13])
    scores = np.array([[1.0, 2.0, 2.0, -1.0, 2.0, 0.5],
                       [0.0, -0.0, -3.0, 0.0, 5.0, -0.0]], dtype=np.float32)
    # request 0: target 5 at 2.0 -- only id 3 ties below it;  request 1: target 7 at 0.0 -- 11 beats, 2 and 3 tie below
    assert KO.ranks(scores, ids, [2.0, 0.0], [5, 7]).tolist() == [2, 4]
    assert KO.ranks(scores, ids, [2.0, -0.0], [5, 7], seen=[{3, 5}, {2, 11, 0}]).tolist() == [1, 2]
    # a target outside the catalogue, and one whose id is in the catalogue with another score: that column never counts
    assert KO.ranks(scores, ids, [2.0, -10.0], [4, 11]).tolist() == [2, 6]
    m = KO.metrics([1, 2, 4], (1, 3), candidates=6)
    assert m["hit@1"] == 1 / 3 and m["hit@3"] == 2 / 3 and m["requests"] == 3 and m["candidates"] == 6
    assert m["ndcg@1"] == 1 / 3 and m["ndcg@3"] == pytest.approx((1 + 1 / np.log2(3)) / 3, rel=1e-15)
    assert m["mean_mrr"] == pytest.approx((1 + 0.5 + 0.25) / 3, rel=1e-15) and m["mean_rank"] == 7 / 3


def test_metrics_agree_with_cal_metric_on_groups_of_the_whole_catalogue():
    from clsr_amd.deeprec_utils import cal_metric
    from clsr_amd.recommend import rank_metrics

    rng = np.random.default_rng(4)
    N, M = 23, 40
    ids = np.arange(2, M + 2)
    scores = rng.choice(np.linspace(-1, 1, 9).astype(np.float32), size=(N, M))      # ties among the candidates
    ts = (rng.choice(np.linspace(-1, 1, 9), size=N) + 0.01).astype(np.float32)       # none at the positive
    ti = np.full(N, 1)
    assert not (scores == ts[:, None]).any()
    r = KO.ranks(scores, ids, ts, ti)
    assert r.min() == 1 and r.max() > 10
    labels = np.zeros((N, 1 + M))
    labels[:, 0] = 1
    preds = np.concatenate([ts[:, None], scores], axis=1).astype(np.float64)
    want = cal_metric(labels, preds, ["mean_mrr", "ndcg@1;5;10", "hit@1;5;10"])
    want_loop = cal_metric([l for l in labels], [p for p in preds], ["mean_mrr", "ndcg@1;5;10", "hit@1;5;10"])
    assert want == want_loop
    for got in (KO.metrics(r, (1, 5, 10)), rank_metrics(r, (1, 5, 10), M)):
        for k, v in want.items():
            assert abs(got[k] - v) <= 0.5e-4 + 1e-12, (k, got[k], v)       # cal_metric rounds to 4 decimals
    a, b = KO.metrics(r, (1, 5, 10), candidates=M), rank_metrics(r, (1, 5, 10), M)
    assert list(a) == list(b)
    for k in a:
        assert a[k] == pytest.approx(b[k], rel=1e-12, abs=0), k


def test_chunk_choice_keeps_the_row_bound():
    from clsr_amd.recommend import ROW_BUDGET, plan_ranked

    cap = 3840
    for N, M in [(1, 1), (40, 300), (1024, 64138), (5, 3839), (5, 3840), (100000, 7), (3, 10 ** 6)]:
        n, c = plan_ranked(N, M, cap)
        assert 1 <= c <= min(cap - 1, M) and 1 <= n <= N and n * (c + 1) <= max(ROW_BUDGET, c + 1)
        assert -(-M // c) == -(-M // min(M, cap - 1)), "no more chunks than the largest chunk needs"
        assert n == max(1, min(N, ROW_BUDGET // (c + 1)))
    assert plan_ranked(1024, 64138, cap) == (8, 3773)
    assert plan_ranked(40, 618, cap) == (40, 618)
    assert plan_ranked(10, 5000, cap, chunk=17) == (10, 17)
    assert plan_ranked(10, 5000, cap, row_budget=10, chunk=64) == (1, 64)
    assert plan_ranked(10, 5000, cap, row_budget=1000) == (1, 1000)       # a group of 1001 rows: one request always fits
    assert plan_ranked(600, 100, cap, chunk=63) == (512, 63)               # groups of 64: 512 x 64 = the budget
    assert plan_ranked(600, 100, cap, chunk=64) == (504, 64)
    for bad in (0, -1, cap):
        with pytest.raises(ValueError, match="chunk must lie in 1 .. 3839"):
            plan_ranked(10, 5000, cap, chunk=bad)


def test_new_entry_points_are_declared_and_resolve():
    from clsr_amd import _lib, build

    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    protos = _lib.parse_header()
    assert len(protos["clsr_reco_fill_ranked"][1]) == 11 and len(protos["clsr_reco_rank_count"][1]) == 13
    assert protos["clsr_reco_rank_count"][2][9:11] == ["int32", "float32"]      # partial, target_score
    lib = _lib.load()
    for name in ("clsr_reco_fill_ranked", "clsr_reco_rank_count", "clsr_reco_rank_supported", "clsr_reco_rank_slab"):
        assert name in protos and getattr(lib, name) is not None
    from clsr_amd.ops import query

    W = query("clsr_reco_rank_slab")
    assert W >= 64 and W % 64 == 0
    ok = lambda Hn, g, T: query("clsr_reco_rank_supported", Hn, g, T)
    assert ok(1, 2, 1) and ok(8, 3840, 256) and ok(100000, 17, 50)
    for bad in [(0, 2, 1), (1, 1, 1), (1, 0, 1), (1, 2, 0), (1, 2, 257), (2 ** 31, 2, 1), (2 ** 30, 2, 1), (2 ** 31 // 3840 + 1, 3840, 1)]:
        assert not ok(*bad), bad
    # the existing entry points are what they were
    assert (query("clsr_reco_max_chunk"), query("clsr_reco_max_k")) == (3840, 256)


def test_run_catalogue_eval_is_on_every_model_class():
    import inspect

    import clsr_amd.clsr as C

    names = ["CLSRModel", "GRU4RecModel", "DINModel", "DIENModel", "A2SVDModel", "SLI_RECModel", "CaserModel", "SASRecModel",
             "NCFModel", "LGNModel", "NextItNetModel"]
    for name in names:
        assert callable(getattr(getattr(C, name), "run_catalogue_eval"))
    sig = inspect.signature(C.SequentialBaseModel.run_catalogue_eval)
    assert list(sig.parameters) == ["self", "infile", "catalogue", "ks", "remove_seen", "chunk", "return_ranks"]
    assert sig.parameters["ks"].default == (1, 5, 10) and sig.parameters["remove_seen"].default is True
    nin = object.__new__(C.NextItNetModel)          # the refusal needs no net
    with pytest.raises(NotImplementedError, match="NextItNetModel.run_catalogue_eval"):
        nin.run_catalogue_eval("file", None)
