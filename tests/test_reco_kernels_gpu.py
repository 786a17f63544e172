"""The two entry points of csrc/reco.hip alone, against tests/reco_oracle.py: ids and score BITS are compared with ``==``.

The shapes are the smallest at which the kernels can go wrong: one candidate, lists that fill over several chunks, fewer
candidates than slots, chunks and catalogues that are seen altogether, a ragged last chunk whose pad columns hold the launch's
largest scores, ties across the K-th place and across chunk edges, both zeros, the largest K with the largest and the
smallest chunk, histories of 1 and 256 steps.  (The merge launches one workgroup per history and clamps nothing; the fill's
grid is clamped at 4096 workgroups of 256 elements, which one case passes.)"""
import numpy as np
import pytest
import torch

import reco_oracle as RO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD_SCORE = np.float32(3.0e38)      # what the pad columns of a ragged chunk hold here: above every real score


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _merge(scores, ids, hist, K, g, remove_seen=True, stride=None, order=None):
    """Run the catalogue ``ids`` [M] with ``scores`` [Hn, M] through clsr_reco_topk_merge in chunks of ``g``; pad columns
    hold (PAD_SCORE, a real id).  ``stride``: row stride of the history array (default T).  ``order``: the chunks' order."""
    from clsr_amd.ops import call

    scores = np.asarray(scores, dtype=np.float32)
    ids = np.asarray(ids, dtype=np.int32)
    Hn, M = scores.shape
    T = hist.shape[1]
    stride = T if stride is None else stride
    wide = np.zeros((Hn, stride), dtype=np.int32)
    wide[:, :T] = hist
    wide[:, T:] = ids[0]        # what lies behind a row is not part of it
    hist_d = _dev(wide)
    best_s = torch.full((Hn, K), 7.0, dtype=torch.float32, device=DEV)      # (first = 1 must not read these)
    best_i = torch.full((Hn, K), int(ids[0]), dtype=torch.int32, device=DEV)
    starts = list(range(0, M, g))
    for n, c0 in enumerate(starts if order is None else [starts[k] for k in order]):
        nv = min(g, M - c0)
        lg = np.full((Hn, g), PAD_SCORE, dtype=np.float32)
        it = np.full((Hn, g), int(ids[-1]), dtype=np.int32)
        lg[:, :nv] = scores[:, c0:c0 + nv]
        it[:, :nv] = ids[c0:c0 + nv]
        call("clsr_reco_topk_merge", _dev(lg.reshape(-1)), _dev(it.reshape(-1)), Hn, g, nv, hist_d, stride, T, int(remove_seen),
             K, best_s, best_i, int(n == 0))
    torch.cuda.synchronize()
    return best_i.cpu().numpy(), best_s.cpu().numpy()


def _check(got, scores, ids, hist, K, remove_seen=True):
    want_i, want_s = RO.topk(scores, ids, K, seen=[set(r.tolist()) for r in hist] if remove_seen else None)
    assert np.array_equal(got[0], want_i)
    assert np.array_equal(RO.bits(got[1]), RO.bits(want_s))
    return want_i, want_s


def _case(Hn, M, T, seed, values=None, seen_frac=0.3):
    """Distinct ascending ids, scores (from ``values`` when given: ties), histories drawn partly from the catalogue."""
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(np.arange(1, 4 * M + 2), size=M, replace=False)).astype(np.int32)
    if values is None:
        scores = rng.standard_normal((Hn, M)).astype(np.float32)
    else:
        scores = rng.choice(np.asarray(values, dtype=np.float32), size=(Hn, M))
    hist = np.where(rng.random((Hn, T)) < seen_frac, rng.choice(ids, size=(Hn, T)), 0).astype(np.int32)
    return scores, ids, hist


def test_one_history_one_candidate_one_slot():
    scores, ids, hist = np.array([[0.25]], np.float32), np.array([9], np.int32), np.zeros((1, 1), np.int32)
    assert _check(_merge(scores, ids, hist, 1, 1), scores, ids, hist, 1)[0].tolist() == [[9]]
    hist[0, 0] = 9      # ... and seen: the slot stays empty
    got = _merge(scores, ids, hist, 1, 1)
    assert got[0].tolist() == [[-1]] and got[1].tolist() == [[-np.inf]]


@pytest.mark.parametrize("Hn,M,T,K,g", [(3, 20, 10, 8, 3),          # the list fills over several chunks
                                        (2, 5, 10, 8, 3),           # fewer candidates than slots: empty tail
                                        (5, 300, 1, 256, 1),        # the widest list, one candidate a launch
                                        (2, 4000, 256, 256, 3840),  # ... and the largest chunk, 256-step rows
                                        (70, 130, 50, 10, 64)])
def test_merge_equals_the_oracle(Hn, M, T, K, g):
    from clsr_amd.ops import query

    assert g <= query("clsr_reco_max_chunk")
    scores, ids, hist = _case(Hn, M, T, seed=Hn * 1000 + M)
    want_i, _ = _check(_merge(scores, ids, hist, K, g), scores, ids, hist, K)
    assert (want_i[:, -1] == -1).any() == (M < K), "empty slots exactly where the catalogue is smaller than the list"
    # the row stride is honoured: rows three times as far apart, a catalogue id behind every row
    _check(_merge(scores, ids, hist, K, g, stride=3 * T), scores, ids, hist, K)


def test_seen_chunks_and_seen_catalogues():
    scores, ids, hist = _case(3, 12, 16, seed=5, seen_frac=0.0)
    hist[0, :4] = ids[4:8]          # history 0 has seen the whole second chunk of four
    hist[1, :12] = ids              # history 1 has seen the catalogue
    got = _merge(scores, ids, hist, 5, 4)
    want_i, _ = _check(got, scores, ids, hist, 5)
    assert not set(want_i[0].tolist()) & set(ids[4:8].tolist()) and want_i[1].tolist() == [-1] * 5 and (want_i[2] > 0).all()
    # remove_seen = 0: the seen ids come back, and the history pointer is not needed
    _check(_merge(scores, ids, hist, 5, 4, remove_seen=False), scores, ids, hist, 5, remove_seen=False)


def test_pad_columns_never_enter():
    # M = 10 in chunks of 4: the last launch has two pad columns, which hold PAD_SCORE with a real, unseen id
    scores, ids, hist = _case(4, 10, 8, seed=11)
    got = _merge(scores, ids, hist, 6, 4)
    _check(got, scores, ids, hist, 6)
    assert float(got[1].max()) < 10.0


@pytest.mark.parametrize("values", [(0.5, -1.25, 2.0, 0.0), (0.0, -0.0, 1.0, -1.0)])
def test_ties_across_the_kth_place_and_the_chunk_edges(values):
    scores, ids, hist = _case(6, 97, 12, seed=23, values=values)
    if any(v == 0 and np.signbit(v) for v in values):      # both zeros are among the scores
        b = RO.bits(scores)
        assert (b == 0x80000000).any() and (b == 0).any()
    want = None
    for g in (1, 7, 64, 3840):
        got = _merge(scores, ids, hist, 9, g)
        if want is None:
            want = _check(got, scores, ids, hist, 9)
            # ties straddle the K-th place: the 9th and the 10th best of some history compare equal
            full_i, full_s = RO.topk(scores, ids, 10, seen=[set(r.tolist()) for r in hist])
            assert (full_s[:, 8] == full_s[:, 9]).any()
        assert np.array_equal(got[0], want[0]) and np.array_equal(RO.bits(got[1]), RO.bits(want[1])), g
    # the chunks in another order: the same lists
    got = _merge(scores, ids, hist, 9, 7, order=list(reversed(range(14))))
    assert np.array_equal(got[0], want[0]) and np.array_equal(RO.bits(got[1]), RO.bits(want[1]))


def test_unsupported_shapes_are_refused():
    from clsr_amd._lib import ClsrLibraryError
    from clsr_amd.ops import call

    z = torch.zeros(8, dtype=torch.float32, device=DEV)
    zi = torch.zeros(8, dtype=torch.int32, device=DEV)
    for Hn, g, T, K in [(1, 3841, 1, 1), (1, 1, 257, 1), (1, 1, 1, 257)]:
        with pytest.raises(ClsrLibraryError, match="unsupported shape"):
            call("clsr_reco_topk_merge", z, zi, Hn, g, 1, zi, T, T, 1, K, z, zi, 1)
    with pytest.raises(ClsrLibraryError, match="invalid argument"):
        call("clsr_reco_topk_merge", z, zi, 1, 4, 5, zi, 1, 1, 1, 1, z, zi, 1)        # n_valid > g


@pytest.mark.parametrize("Hn,g,M,c0", [(1, 4, 10, 8),            # c0 + g past M, one history
                                       (3, 5, 7, 5),
                                       (100, 7, 30, 28),         # past one workgroup's span of 256 elements
                                       (300, 3840, 4000, 3840)])  # past the clamped grid (4096 x 256 elements)
def test_fill_candidates(Hn, g, M, c0):
    from clsr_amd.ops import call

    rng = np.random.default_rng(M)
    ci = np.sort(rng.choice(np.arange(1, 10 * M), size=M, replace=False)).astype(np.int32)
    cc = rng.integers(1, 20, M).astype(np.int32)
    GUARD, n = 16, Hn * g
    items = torch.full((n + 2 * GUARD,), -7, dtype=torch.int32, device=DEV)
    cates = torch.full((n + 2 * GUARD,), -9, dtype=torch.int32, device=DEV)
    call("clsr_reco_fill_candidates", _dev(ci), _dev(cc), M, c0, g, Hn, items[GUARD:GUARD + n], cates[GUARD:GUARD + n])
    torch.cuda.synchronize()
    col = c0 + np.arange(g)
    want_i = np.tile(np.where(col < M, ci[np.minimum(col, M - 1)], 0), Hn)
    want_c = np.tile(np.where(col < M, cc[np.minimum(col, M - 1)], 0), Hn)
    assert (col >= M).any()
    for got, want, guard in ((items, want_i, -7), (cates, want_c, -9)):
        got = got.cpu().numpy()
        assert np.array_equal(got[GUARD:GUARD + n], want)
        assert (got[:GUARD] == guard).all() and (got[GUARD + n:] == guard).all()
