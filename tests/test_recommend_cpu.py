"""The host side of ``recommend_k_items``: the catalogue and its refusals, the chunk planner, the selection oracle on a
hand-checked case, the host queries of csrc/reco.hip."""
import os
import types

import numpy as np
import pytest

import reco_oracle as RO


def _iterator(golden_hparams):
    from clsr_amd.sequential_iterator import SequentialIterator

    return SequentialIterator(golden_hparams)


def _line(user, item, cate, hist_items, hist_cates):
    ts = ",".join(str(1000 + k) for k in range(len(hist_items)))
    return "1\t%s\t%s\t%s\t2000\t%s\t%s\t%s\n" % (user, item, cate, ",".join(hist_items), ",".join(hist_cates), ts)


def test_from_files_pairs_an_item_with_its_first_category(golden_hparams, tmp_path):
    from clsr_amd.catalogue import Catalogue

    it = _iterator(golden_hparams)
    inv_i = {v: k for k, v in it.itemdict.items()}
    inv_c = {v: k for k, v in it.catedict.items()}
    i = [inv_i[k] for k in (5, 9, 17, 33, 2)]
    A, B, C = inv_c[3], inv_c[4], inv_c[7]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    with open(a, "w") as f:
        # item 5: target with A first, later (history, then another file) with B -> A.  item 17: only ever in a history.
        # item 9: FIRST seen in a history with C, then as a target with A -> C.  "nowhere" is outside the vocabulary -> id 0.
        f.write(_line("u1", i[0], A, [i[1], i[2]], [C, B]))
        f.write(_line("u1", i[1], A, [i[0], "nowhere"], [B, B]))
    with open(b, "w") as f:
        f.write(_line("u2", i[3], B, [i[0]], [C]))
    model = types.SimpleNamespace(iterator=it)
    for source in (it, model):
        cat = Catalogue.from_files(source, [a, b])
        assert cat.items.dtype == np.int32 and cat.cates.dtype == np.int32
        assert cat.items.tolist() == [5, 9, 17, 33] and cat.cates.tolist() == [3, 7, 4, 4]      # item 2: never named
    # the files in the other order: item 5 is met with C first
    assert Catalogue.from_files(it, [b, a]).cates.tolist() == [7, 7, 4, 4]
    assert Catalogue.from_files(it, a).items.tolist() == [5, 9, 17]


def test_from_files_agrees_with_the_graph_of_lgn_on_the_golden_data(golden_hparams, golden_dir):
    from clsr_amd import lgn_graph
    from clsr_amd.catalogue import Catalogue

    train = os.path.join(golden_dir, "data", "train_data")
    cat = Catalogue.from_files(_iterator(golden_hparams), [train])
    item2cate = lgn_graph.build_graph(golden_hparams).item2cate
    assert len(cat) > 300 and np.array_equal(item2cate[cat.items], cat.cates)
    # and the graph names no item the catalogue lacks
    assert set(np.flatnonzero(item2cate).tolist()) <= set(cat.items.tolist())


@pytest.mark.parametrize("items,cates,word", [
    ([0, 3], [1, 1], "items holds id 0"),
    ([3, 3], [1, 1], "items holds id 3 twice"),
    ([4, 3], [1, 1], "items must ascend"),
    ([3, 4], [1], "cates holds 1 entries for 2 items"),
    ([], [], "items is empty"),
    ([3, 994], [1, 1], "items holds id 994, the item vocabulary has 994 rows"),
])
def test_catalogue_refuses_by_argument_name(items, cates, word):
    from clsr_amd.catalogue import Catalogue

    with pytest.raises(ValueError, match=word):
        Catalogue(np.asarray(items, dtype=np.int32), np.asarray(cates, dtype=np.int32), n_items=994)


def test_catalogue_checks_the_vocabulary_late_when_it_is_not_given():
    from clsr_amd.catalogue import Catalogue

    cat = Catalogue([3, 993], [1, 20])
    cat.check_vocabulary(994, 21)
    with pytest.raises(ValueError, match="items holds id 993, the item vocabulary has 993 rows"):
        cat.check_vocabulary(993)
    with pytest.raises(ValueError, match="cates holds id 20"):
        cat.check_vocabulary(994, 20)


def test_planner_bounds():
    from clsr_amd.recommend import ROW_BUDGET, plan

    cap = 3840
    for N, M in [(1, 1), (6, 300), (1024, 64138), (5, 3840), (5, 3841), (100000, 7), (3, 10 ** 6)]:
        n, g = plan(N, M, cap)
        chunks = -(-M // g)
        assert 1 <= g <= min(cap, M) and 1 <= n <= N and n * g <= ROW_BUDGET
        assert chunks == -(-M // min(M, cap)), "no more chunks than the largest chunk needs"
        assert chunks * g - M < chunks, "the ragged last chunk lacks less than one candidate a chunk"
        assert n == min(N, ROW_BUDGET // g), "all the requests the budget leaves room for"
    assert plan(1024, 64138, cap) == (8, 3773)
    assert plan(6, 300, cap) == (6, 300)
    # a smaller budget bounds g as well; a pinned chunk is taken as it is, and one request always fits
    assert plan(10, 5000, cap, row_budget=1000) == (1, 1000)
    assert plan(10, 5000, cap, chunk=17) == (10, 17)
    assert plan(10, 5000, cap, row_budget=10, chunk=64) == (1, 64)
    for bad in (0, -1, cap + 1):
        with pytest.raises(ValueError, match="chunk must lie in 1 .. 3840"):
            plan(10, 5000, cap, chunk=bad)
    with pytest.raises(ValueError, match="must be positive"):
        plan(0, 5, cap)


def test_oracle_on_a_hand_checked_case_with_ties():
    ids = np.array([2, 3, 5, 7, 11, 13])
    scores = np.array([[1.0, 2.0, 2.0, -1.0, 2.0, 0.5],
                       [0.0, -0.0, -3.0, 0.0, 5.0, -0.0]], dtype=np.float32)
    items, top = RO.topk(scores, ids, 4)
    assert items.tolist() == [[3, 5, 11, 2], [11, 2, 3, 7]]
    assert top.tolist() == [[2.0, 2.0, 2.0, 1.0], [5.0, 0.0, 0.0, 0.0]]
    assert RO.bits(top[1]).tolist() == [0x40A00000, 0, 0, 0]            # the zeros come back as +0.0
    # seen items are skipped; fewer than K left: (-inf, -1) in the tail
    items, top = RO.topk(scores, ids, 4, seen=[{3, 11, 0}, {2, 3, 5, 7, 13}])
    assert items.tolist() == [[5, 2, 13, 7], [11, -1, -1, -1]]
    assert top[0].tolist() == [2.0, 1.0, 0.5, -1.0] and top[1].tolist() == [5.0] + [-np.inf] * 3
    items, top = RO.topk(scores, ids, 1, seen=[set(ids.tolist()), ()])
    assert items.tolist() == [[-1], [11]] and top.tolist() == [[-np.inf], [5.0]]


def test_host_queries_of_the_selection_kernel():
    from clsr_amd import build

    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from clsr_amd.ops import query

    gmax, kmax = query("clsr_reco_max_chunk"), query("clsr_reco_max_k")
    assert (gmax, kmax) == (3840, 256) and gmax + kmax == 4096       # the list and a chunk share 4096 key slots
    ok = lambda Hn, g, T, K: query("clsr_reco_topk_supported", Hn, g, T, K)
    assert ok(1, 1, 1, 1) and ok(8, gmax, 256, kmax) and ok(100000, 17, 50, 10)
    for bad in [(0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, gmax + 1, 1, 1), (1, 1, 257, 1), (1, 1, 1, kmax + 1),
                (2 ** 31, 1, 1, 1), (2 ** 31 // gmax + 1, gmax, 1, 1)]:
        assert not ok(*bad), bad
