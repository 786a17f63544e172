"""Host side of the resident evaluation path (no GPU): the chunk plan against an independent walk over the iterator's
batches, the numpy form of the run-flag rule against ``_shared_history_group``, the iterator's ``eval_lines`` helper and
the host checks of the store."""
import copy
import os
import random

import numpy as np
import pytest

from clsr_amd.clsr import SequentialBaseModel
from clsr_amd.resident import COLUMNS, EvalLines, ResidentEvalColumns, ResidentEvalStore, eval_chunk_plan, same_rows
from clsr_amd.sequential_iterator import NextItNetIterator, SASequentialIterator, SequentialIterator

FILES = {"valid_data": (200, 5), "test_data": (400, 10)}        # lines, lines per positive


def _iterator(golden_hparams, batch_size, cls=SequentialIterator):
    hp = copy.deepcopy(golden_hparams)
    hp.batch_size = batch_size
    return cls(hp)


def _walk(it, path, m, target, dedup):
    """The chunks of ``_device_eval`` on the host path: ``_shared_history_group`` per batch, batches of one group size
    joined until they hold ``target`` lines."""
    chunks, pend, k = [], None, 0
    for feed in it.load_data_from_file(path, batch_num_ngs=0, min_seq_length=m):
        n = int(np.asarray(feed["labels"]).shape[0])
        g = SequentialBaseModel._shared_history_group(feed) if dedup else 1
        if pend is not None and pend[2] != g:
            chunks.append(tuple(pend))
            pend = None
        if pend is None:
            pend = [k, 0, g]
        pend[1] += n
        k += n
        if pend[1] >= target:
            chunks.append(tuple(pend))
            pend = None
    if pend is not None:
        chunks.append(tuple(pend))
    return chunks


def _pair_rule(arrays):
    """uint8 [n]: 1 where ``_shared_history_group`` finds rows i - 1 and i of the feed ``arrays`` to be one run (asked
    pair by pair: two equal rows are one run of 2)."""
    n = np.asarray(arrays["item_history"]).shape[0]
    out = np.zeros(n, dtype=np.uint8)
    for i in range(1, n):
        pair = {k: np.asarray(v)[i - 1:i + 1] for k, v in arrays.items()}
        out[i] = SequentialBaseModel._shared_history_group(pair) == 2
    return out


def _as_feed(cols, keep):
    """The arrays an evaluation feed of the lines ``keep`` holds (``_convert_rows``: users as float32)."""
    f = {k: np.asarray(cols[k])[keep] for k in ("item_history", "item_cate_history", "mask", "time_from_first_action",
                                               "time_to_now")}
    f["users"] = np.asarray(cols["users"])[keep].astype(np.float32)
    return f


@pytest.mark.parametrize("name", sorted(FILES))
def test_fixture_facts(name, golden_dir, golden_hparams):
    path = os.path.join(golden_dir, "data", name)
    n_lines, per = FILES[name]
    it = _iterator(golden_hparams, 50)
    cols, keep = it.eval_lines(path, 1)
    assert np.array_equal(keep, np.arange(n_lines))
    flags = same_rows(cols, keep)
    starts = np.flatnonzero(flags == 0)
    assert np.array_equal(starts, np.arange(0, n_lines, per)), "40 runs of %d lines" % per
    full = cols["full_len"]
    assert 1 <= full.min() < 3 and 10 < full.max() <= 14, "some runs fall to min_seq_length = 3, some are cut to T = 10"
    assert np.array_equal(full, np.repeat(full[::per], per)), "min_seq_length drops whole runs, never part of one"
    _, keep3 = it.eval_lines(path, 3)
    assert 0 < len(keep3) < n_lines and len(keep3) % per == 0


@pytest.mark.parametrize("name", sorted(FILES))
@pytest.mark.parametrize("batch_size", [7, 50, 64, 200])
@pytest.mark.parametrize("m", [1, 3])
def test_plan_equals_an_independent_walk(name, batch_size, m, golden_dir, golden_hparams):
    path = os.path.join(golden_dir, "data", name)
    it = _iterator(golden_hparams, batch_size)
    cols, keep = it.eval_lines(path, m)
    flags = same_rows(cols, keep)
    per = FILES[name][1]
    for target in (120, 32768):
        for dedup in (True, False):
            plan = eval_chunk_plan(flags if dedup else None, len(keep), batch_size, target, dedup)
            assert plan == _walk(it, path, m, target, dedup), (target, dedup)
            assert sum(n for _, n, _ in plan) == len(keep) and [k for k, _, _ in plan] == list(
                np.cumsum([0] + [n for _, n, _ in plan[:-1]]))
            if not dedup:
                assert all(g == 1 for _, _, g in plan)
            elif batch_size in (50, 200):
                assert all(g == per for _, _, g in plan)
            elif name == "valid_data" and batch_size == 64:
                # every batch holds whole runs of 5 and a cut one: no common group
                assert all(g == 1 for _, _, g in plan)
            else:
                # batches that cut a run have g = 1 (one that lies inside a single run still has its group)
                assert any(g == 1 for _, _, g in plan)
            if target == 32768 and (not dedup or batch_size in (50, 200)):
                assert len(plan) == 1
            if target == 120 and batch_size == 50 and m == 1:
                assert [n for _, n, _ in plan][0] == 150


def test_plan_edges():
    assert eval_chunk_plan(np.zeros(0, np.uint8), 0, 8, 100) == []
    assert eval_chunk_plan(np.zeros(1, np.uint8), 1, 8, 100) == [(0, 1, 1)]
    # a one-line last batch has g = 1 and ends the chunk of twos in front of it
    flags = np.array([0, 1, 0, 1, 0], np.uint8)
    assert eval_chunk_plan(flags, 5, 4, 100) == [(0, 4, 2), (4, 1, 1)]
    # the first line of a batch starts a run, whatever its flag says
    assert eval_chunk_plan(np.array([0, 1, 1, 1], np.uint8), 4, 2, 100) == [(0, 4, 2)]
    assert eval_chunk_plan(np.array([0, 1, 1, 0, 1, 1], np.uint8), 6, 3, 3) == [(0, 3, 3), (3, 3, 3)]
    # runs of 2 and 4: groups of 2; runs of 2 and 3: none
    assert eval_chunk_plan(np.array([0, 1, 0, 1, 1, 1], np.uint8), 6, 6, 100) == [(0, 6, 2)]
    assert eval_chunk_plan(np.array([0, 1, 0, 1, 1, 0], np.uint8), 6, 6, 100) == [(0, 6, 1)]


@pytest.mark.parametrize("name", sorted(FILES))
def test_flag_rule_is_the_rule_of_shared_history_group_on_the_fixtures(name, golden_dir, golden_hparams):
    path = os.path.join(golden_dir, "data", name)
    it = _iterator(golden_hparams, 50)
    cols, keep = it.eval_lines(path, 1)
    rng = np.random.RandomState(4)
    for lines in (keep, rng.permutation(keep), np.sort(rng.randint(0, len(keep), 90))):
        got = same_rows(cols, lines)
        assert got.dtype == np.uint8 and got[0] == 0
        assert np.array_equal(got, _pair_rule(_as_feed(cols, lines)))


def _hand_made():
    """Twelve lines, T = 4.  Lines 0/1: time_to_now -0.0 against 0.0; 2/3: a NaN in both; 4/5 and 6/7: two groups with one
    history and two users; 8/9: lens differ (a padded zero against a real zero); 10/11: item_history differs in the last
    word."""
    T, N = 4, 12
    rng = np.random.RandomState(0)
    cols = {"item_history": np.repeat(rng.randint(1, 50, (N // 2, T)), 2, axis=0).astype(np.int32),
            "item_cate_history": np.repeat(rng.randint(1, 9, (N // 2, T)), 2, axis=0).astype(np.int32),
            "time_from_first_action": np.repeat(rng.rand(N // 2, T), 2, axis=0).astype(np.float32),
            "time_to_now": np.repeat(rng.rand(N // 2, T), 2, axis=0).astype(np.float32),
            "lens": np.full(N, T, np.int64), "users": np.repeat(np.arange(1, N // 2 + 1), 2).astype(np.int32),
            "items": np.arange(N, dtype=np.int32), "cates": np.arange(N, dtype=np.int32) % 5,
            "labels": (np.arange(N) % 2 == 0).astype(np.float32)}
    cols["time_to_now"][0, 1], cols["time_to_now"][1, 1] = -0.0, 0.0
    cols["time_from_first_action"][2:4, 2] = np.nan
    for k in ("item_history", "item_cate_history", "time_from_first_action", "time_to_now"):
        cols[k][6:8] = cols[k][4:6]
    cols["lens"][8] = T - 1
    for k in ("item_history", "item_cate_history"):
        cols[k][8:10, T - 1] = 0
    cols["item_history"][11, T - 1] += 1
    cols["mask"] = (np.arange(T)[None, :] < cols["lens"][:, None]).astype(np.float32)
    return cols


def test_flag_rule_on_a_hand_made_store():
    cols = _hand_made()
    keep = np.arange(12)
    want = np.array([0, 1, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0], np.uint8)
    assert np.array_equal(same_rows(cols, keep), want)
    assert np.array_equal(_pair_rule(_as_feed(cols, keep)), want)
    for lines in (np.array([5]), np.array([4, 5, 5, 4, 6, 7, 1, 0, 3, 3]), np.array([7, 6, 5, 4])):
        got = same_rows(cols, lines)
        assert np.array_equal(got, _pair_rule(_as_feed(cols, lines))), lines
    assert same_rows(cols, np.array([5])).tolist() == [0]
    assert same_rows(cols, np.array([3, 3])).tolist() == [0, 0], "a NaN equals nothing, itself included"
    # ids that differ only below the precision of float32 are one user to an evaluation feed
    cols["users"][4:6] = (2 ** 24, 2 ** 24 + 1)
    assert same_rows(cols, keep)[5] == 1 and _pair_rule(_as_feed(cols, keep))[5] == 1


@pytest.mark.parametrize("cls", [SequentialIterator, SASequentialIterator])
def test_eval_lines_are_what_the_iterator_yields(cls, golden_dir, golden_hparams):
    path = os.path.join(golden_dir, "data", "train_data")
    it = _iterator(golden_hparams, 64, cls)

    def check(m):
        state = random.getstate()
        cols, keep = it.eval_lines(path, m)
        assert random.getstate() == state
        feeds = list(it.load_data_from_file(path, batch_num_ngs=0, min_seq_length=m))
        assert random.getstate() == state
        assert cols is it._columns[path] and sum(len(f["items"]) for f in feeds) == len(keep)
        for k in ("items", "cates", "item_history", "time_to_now"):
            assert np.array_equal(np.concatenate([f[k] for f in feeds]), cols[k][keep]), k
        assert np.array_equal(np.concatenate([f["users"] for f in feeds]), cols["users"][keep].astype(np.float32))
        return keep

    first = check(1)                                # (parses the file)
    assert np.array_equal(first, np.arange(len(first)))
    assert len(check(3)) < len(first)
    random.seed(7)
    for f in it.load_data_from_file(path, batch_num_ngs=4):     # a training pass shuffles the file
        pass
    after = check(1)
    assert not np.array_equal(after, first) and np.array_equal(np.sort(after), first)
    check(3)
    for f in it.load_data_from_file(path, batch_num_ngs=4):     # the shuffle is cumulative
        pass
    assert not np.array_equal(check(1), after)


def test_store_checks_on_the_host():
    """``keep`` is held against ``[0, N)`` before anything is uploaded; the image is ``N (16 T + 20)`` bytes."""
    cols = _hand_made()
    rc = ResidentEvalColumns(cols, "cpu")
    assert rc.nbytes == 12 * (16 * 4 + 20) and set(rc.dev) == set(COLUMNS) | {"labels"}
    ent = EvalLines(rc, np.array([3, 0, 11, 3]), "cpu")
    assert ent.keep.dtype == np.int32 and ent.n_keep == 4 and ent.flags is None and ent.nbytes == 16
    for bad in ([0, 12], [-1, 2], [2 ** 31]):
        with pytest.raises(ValueError, match="keep"):
            EvalLines(rc, np.array(bad, dtype=np.int64), "cpu")
    with pytest.raises(ValueError, match="keep"):
        EvalLines(rc, np.zeros((2, 2), np.int64), "cpu")
    assert EvalLines(rc, np.zeros(0, np.int64), "cpu").keep_dev is None
    big = dict(cols, users=cols["users"].astype(np.int64) + (2 ** 31 - 64))
    with pytest.raises(ValueError, match="users"):
        ResidentEvalColumns(big, "cpu")


def test_store_follows_the_iterator(golden_dir, golden_hparams):
    """Without flags the store needs no device code: one image per parse, ``keep`` rebuilt when the order changed."""
    path = os.path.join(golden_dir, "data", "train_data")
    it = _iterator(golden_hparams, 64)
    store = ResidentEvalStore(it, "cpu")
    a = store.get(path, 1, flags=False)
    assert store.uploads == 1 and store.get(path, 1, flags=False) is a and store.uploads == 1
    b = store.get(path, 3, flags=False)
    assert b is not a and b.rc is a.rc and store.uploads == 1
    N, T = a.rc.N, a.rc.T
    assert store.nbytes == N * (16 * T + 20) + 4 * (a.n_keep + b.n_keep)
    random.seed(1)
    for f in it.load_data_from_file(path, batch_num_ngs=4):
        pass
    c = store.get(path, 1, flags=False)
    assert c is not a and c.rc is a.rc and store.uploads == 1 and not np.array_equal(c.keep, a.keep)
    it.iter_data.pop(path)                          # the iterator parses the file again
    d = store.get(path, 1, flags=False)
    assert store.uploads == 2 and d.rc is not a.rc
    with pytest.raises(NotImplementedError, match="NextItNetIterator"):
        ResidentEvalStore(NextItNetIterator(golden_hparams), "cpu")
