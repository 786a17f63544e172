"""``clsr_reco_fill_ranked`` and ``clsr_reco_rank_count`` (csrc/reco.hip) alone, on synthetic logits and ids: ranks are compared
with ``==`` against tests/rank_oracle.py, the target's score by its bits.

A feed group is the target in column 0 and ``g - 1`` candidate columns, of which the first ``n_valid`` count.  The shapes sit on
every boundary of the launch: one candidate, a wave (64 columns), a slab of ``W = clsr_reco_rank_slab()`` columns and one and
two past it, the largest group, ragged chunks whose pad columns hold the launch's largest scores.  Scores come from four values
(both zeros among them), so most candidates tie with the target and the id decides."""
import numpy as np
import pytest
import torch

import rank_oracle as KO
import reco_oracle as RO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD_SCORE = np.float32(3.0e38)
VALUES = np.asarray([0.0, -0.0, 1.5, -2.0], dtype=np.float32)
GUARD = 8


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _slab():
    from clsr_amd.ops import query

    return query("clsr_reco_rank_slab")


def _group_size(name):
    from clsr_amd.ops import query

    if isinstance(name, int):
        return name
    return {"W": _slab(), "W+1": _slab() + 1, "W+2": _slab() + 2, "max": query("clsr_reco_max_chunk")}[name]


class Counter(object):
    """``partial`` / ``target_score`` of ``Hn`` requests at group ``g`` with guard words on both sides, prefilled with values a
    ``first`` launch must overwrite."""

    def __init__(self, Hn, g, hist, stride=None):
        self.Hn, self.g, self.T = Hn, g, hist.shape[1]
        self.slabs = -(-(g - 1) // _slab())
        self.stride = self.T if stride is None else stride
        wide = np.full((Hn, self.stride), -5, dtype=np.int32)        # what lies behind a row is not part of it
        wide[:, :self.T] = hist
        self.hist = _dev(wide)
        self.partial = torch.full((Hn * self.slabs + 2 * GUARD,), 12345, dtype=torch.int32, device=DEV)
        self.tscore = torch.full((Hn + 2 * GUARD,), 7.0, dtype=torch.float32, device=DEV)
        self.launches = 0

    def launch(self, lg, it, n_valid, remove_seen):
        from clsr_amd.ops import call

        assert lg.shape == (self.Hn, self.g) == it.shape
        call("clsr_reco_rank_count", _dev(lg.reshape(-1)), _dev(it.reshape(-1)), self.Hn, self.g, n_valid, self.hist, self.stride,
             self.T, int(remove_seen), self.partial[GUARD:GUARD + self.Hn * self.slabs], self.tscore[GUARD:GUARD + self.Hn],
             int(self.launches == 0))
        self.launches += 1

    def result(self):
        torch.cuda.synchronize()
        p, s = self.partial.cpu().numpy(), self.tscore.cpu().numpy()
        n = self.Hn * self.slabs
        assert (p[:GUARD] == 12345).all() and (p[GUARD + n:] == 12345).all(), "a slot outside partial was written"
        assert (s[:GUARD] == 7.0).all() and (s[GUARD + self.Hn:] == 7.0).all()
        part = p[GUARD:GUARD + n].reshape(self.Hn, self.slabs)
        assert (part >= 0).all() and (part <= _slab() * self.launches).all()
        return 1 + part.sum(1), s[GUARD:GUARD + self.Hn]


def _group(rng, Hn, g, n_valid, T, target_in_history=True):
    """One launch's ``logit`` / ``items`` [Hn, g] and ``hist`` [Hn, T]: column 0 the target, the valid columns distinct ids
    above and below the target's with one column that IS the target's id (at the best score: it must not count), pad columns
    (PAD_SCORE, a real unseen id).  Half of the history slots hold ids of the valid columns."""
    lg = rng.choice(VALUES, size=(Hn, g))
    it = np.zeros((Hn, g), dtype=np.int32)
    hist = np.zeros((Hn, T), dtype=np.int32)
    for h in range(Hn):
        ids = rng.choice(np.arange(1, 3 * g + 8), size=g, replace=False).astype(np.int32)
        it[h] = ids
        valid = ids[1:1 + n_valid]
        if n_valid >= 2:
            k = 1 + int(rng.integers(0, n_valid))
            it[h, k], lg[h, k] = ids[0], 1.5
        hist[h] = np.where(rng.random(T) < 0.5, rng.choice(valid, size=T), 0)
        if target_in_history and h % 2 == 0:
            hist[h, T // 2] = ids[0]
    lg[:, 1 + n_valid:] = PAD_SCORE
    return lg.astype(np.float32), it, hist


def _want(lg, it, n_valid, hist, remove_seen):
    return KO.ranks(lg[:, 1:1 + n_valid], it[:, 1:1 + n_valid], lg[:, 0], it[:, 0],
                    seen=[set(r.tolist()) for r in hist] if remove_seen else None)


@pytest.mark.parametrize("Hn", [1, 3])
@pytest.mark.parametrize("g", [2, 3, 64, 65, 256, 257, 258, "W", "W+1", "W+2", "max"])
def test_one_launch_equals_the_oracle(g, Hn):
    g = _group_size(g)
    rng = np.random.default_rng(1000 * g + Hn)
    ties = below = above = 0
    for n_valid in sorted({1, max(1, g - 2), g - 1}):
        for T in (1, 50, 256):
            lg, it, hist = _group(rng, Hn, g, n_valid, T)
            for stride in (T, g * T):
                for remove_seen in (True, False):
                    c = Counter(Hn, g, hist, stride)
                    c.launch(lg, it, n_valid, remove_seen)
                    got, ts = c.result()
                    assert np.array_equal(got, _want(lg, it, n_valid, hist, remove_seen)), (n_valid, T, stride, remove_seen)
                    assert np.array_equal(RO.bits(ts), RO.bits(lg[:, 0]))
            tie = (lg[:, 1:1 + n_valid] == lg[:, :1]) & (it[:, 1:1 + n_valid] != it[:, :1])
            ties += int(tie.sum())
            below += int((tie & (it[:, 1:1 + n_valid] < it[:, :1])).sum())
            above += int((tie & (it[:, 1:1 + n_valid] > it[:, :1])).sum())
    if g >= 64:
        assert ties > g // 4 and below and above, "most columns tie with the target, with ids on both sides of its id"


def test_both_zeros_tie_and_the_targets_own_id_never_counts():
    # target (+0.0, id 10); candidates: -0.0 with a lower id (counts), -0.0 with a higher id (does not), the target's id at 1.5
    lg = np.array([[0.0, -0.0, -0.0, 1.5, 0.0]], dtype=np.float32)
    it = np.array([[10, 4, 12, 10, 3]], dtype=np.int32)
    hist = np.zeros((1, 1), dtype=np.int32)
    assert RO.bits(lg)[0, 1] == 0x80000000
    for flip in (False, True):      # ... and the target at -0.0 against candidates at +0.0
        l = -lg if flip else lg
        l[0, 3] = 1.5
        c = Counter(1, 5, hist)
        c.launch(l, it, 4, True)
        got, ts = c.result()
        assert got.tolist() == [3] == _want(l, it, 4, hist, True).tolist()
        assert RO.bits(ts)[0] == RO.bits(l)[0, 0], "the target's score keeps its stored bits"


@pytest.mark.parametrize("g", [5, 258])
def test_seen_candidates_and_a_target_in_its_own_history(g):
    rng = np.random.default_rng(g)
    n_valid, T = g - 1, 50
    lg, it, hist = _group(rng, 3, g, n_valid, T, target_in_history=False)
    lg[:, 1:] = 1.5
    lg[:, 0] = -2.0                                  # every candidate beats the target ...
    it[:, 1:] = np.arange(100, 100 + n_valid)
    it[:, 0] = 50
    hist[:] = 0
    hist[0, :4] = (50, 100, 101, 50)                 # request 0: its target and two candidates seen
    hist[1, :] = np.resize(np.arange(100, 100 + n_valid), T)      # request 1: 50 candidates (g = 5: every one) seen
    for remove_seen, want in ((False, [g, g, g]), (True, [g - 2, max(1, g - 50), g])):
        c = Counter(3, g, hist)
        c.launch(lg, it, n_valid, remove_seen)
        got, _ = c.result()
        assert got.tolist() == want == _want(lg, it, n_valid, hist, remove_seen).tolist()
    # nobody beats the target: rank 1 whatever is seen
    lg[:, 0] = 1.5
    it[:, 0] = 1
    c = Counter(3, g, hist)
    c.launch(lg, it, n_valid, True)
    assert c.result()[0].tolist() == [1, 1, 1]


def test_every_candidate_seen_at_the_longest_history():
    g, T = 257, 256
    rng = np.random.default_rng(9)
    lg, it, _ = _group(rng, 1, g, g - 1, T)
    lg[:, 0] = -2.0
    lg[:, 1:] = 1.5
    hist = it[:, 1:].copy()                          # 256 candidates, 256 history steps
    hist[0, 7] = it[0, 0]                            # (one slot for the target itself: at most that candidate stays)
    c = Counter(1, g, hist)
    c.launch(lg, it, g - 1, True)
    want = _want(lg, it, g - 1, hist, True)
    assert c.result()[0].tolist() == want.tolist() and int(want[0]) <= 2
    c = Counter(1, g, hist)
    c.launch(lg, it, g - 1, False)
    assert c.result()[0].tolist() == [g - 1]         # (one column holds the target's own id)


def test_pad_columns_never_count():
    g = 300
    rng = np.random.default_rng(3)
    for n_valid in (1, 255, 256, 257):
        lg, it, hist = _group(rng, 2, g, n_valid, 8)
        assert (lg[:, 1 + n_valid:] == PAD_SCORE).all() and (it[:, 1 + n_valid:] > 0).all()
        c = Counter(2, g, hist)
        c.launch(lg, it, n_valid, False)
        got, _ = c.result()
        assert np.array_equal(got, _want(lg, it, n_valid, hist, False)) and (got <= 1 + n_valid).all()


def _sweep(scores, ids, ts, ti, hist, chunk, remove_seen=True, order=None):
    """The catalogue ``ids`` [M] with ``scores`` [Hn, M] in chunks of ``chunk`` candidates, the target in column 0 of each."""
    Hn, M = scores.shape
    g = chunk + 1
    c = Counter(Hn, g, hist)
    starts = list(range(0, M, chunk))
    for c0 in (starts if order is None else [starts[k] for k in order]):
        nv = min(chunk, M - c0)
        lg = np.full((Hn, g), PAD_SCORE, dtype=np.float32)
        it = np.full((Hn, g), int(ids[-1]), dtype=np.int32)
        lg[:, 0], it[:, 0] = ts, ti
        lg[:, 1:1 + nv], it[:, 1:1 + nv] = scores[:, c0:c0 + nv], ids[c0:c0 + nv]
        c.launch(lg, it, nv, remove_seen)
    return c.result()


def test_one_catalogue_whatever_the_chunk_and_the_order():
    from clsr_amd.ops import query

    rng = np.random.default_rng(23)
    Hn, M, T = 6, 97, 12
    ids = np.sort(rng.choice(np.arange(1, 4 * M + 2), size=M, replace=False)).astype(np.int32)
    scores = rng.choice(VALUES, size=(Hn, M))
    col = rng.integers(0, M, Hn)
    ts, ti = scores[np.arange(Hn), col], ids[col]     # the targets are catalogue items: their own column never counts
    hist = np.where(rng.random((Hn, T)) < 0.3, rng.choice(ids, size=(Hn, T)), 0).astype(np.int32)
    hist[0, 0] = ti[0]
    for remove_seen in (True, False):
        want = KO.ranks(scores, ids, ts, ti, seen=[set(r.tolist()) for r in hist] if remove_seen else None)
        assert want.max() > 8 and len(set(want.tolist())) > 2
        for chunk in (1, 7, 64, query("clsr_reco_max_chunk") - 1):
            got, got_s = _sweep(scores, ids, ts, ti, hist, chunk, remove_seen)
            assert np.array_equal(got, want), chunk
            assert np.array_equal(RO.bits(got_s), RO.bits(ts))
        got, _ = _sweep(scores, ids, ts, ti, hist, 7, remove_seen, order=list(reversed(range(14))))
        assert np.array_equal(got, want)


@pytest.mark.parametrize("Hn,g,M,c0", [(1, 4, 10, 8),             # c0 + g - 1 past M, one request
                                       (3, 2, 7, 6),              # one candidate a group
                                       (3, 5, 7, 4),
                                       (100, 7, 30, 28),          # past one workgroup's span of 256 elements
                                       (300, 3840, 4000, 3839)])  # past the clamped grid (4096 x 256 elements)
def test_fill_ranked(Hn, g, M, c0):
    from clsr_amd.ops import call

    rng = np.random.default_rng(M)
    ci = np.sort(rng.choice(np.arange(1, 10 * M), size=M, replace=False)).astype(np.int32)
    cc = rng.integers(1, 20, M).astype(np.int32)
    ti = rng.integers(1, 10 * M, Hn).astype(np.int32)
    tc = rng.integers(20, 40, Hn).astype(np.int32)
    n = Hn * g
    assert (n > 4096 * 256) == (Hn == 300)
    items = torch.full((n + 2 * GUARD,), -7, dtype=torch.int32, device=DEV)
    cates = torch.full((n + 2 * GUARD,), -9, dtype=torch.int32, device=DEV)
    call("clsr_reco_fill_ranked", _dev(ci), _dev(cc), M, c0, g, _dev(ti), _dev(tc), Hn, items[GUARD:GUARD + n],
         cates[GUARD:GUARD + n])
    torch.cuda.synchronize()
    col = c0 + np.arange(g - 1)
    want_i = np.concatenate([ti[:, None], np.tile(np.where(col < M, ci[np.minimum(col, M - 1)], 0), (Hn, 1))], axis=1)
    want_c = np.concatenate([tc[:, None], np.tile(np.where(col < M, cc[np.minimum(col, M - 1)], 0), (Hn, 1))], axis=1)
    assert (col >= M).any() or g == 2
    for got, want, guard in ((items, want_i, -7), (cates, want_c, -9)):
        got = got.cpu().numpy()
        assert np.array_equal(got[GUARD:GUARD + n], want.reshape(-1))
        assert (got[:GUARD] == guard).all() and (got[GUARD + n:] == guard).all()


def test_refusals_are_error_codes():
    from clsr_amd._lib import ClsrLibraryError
    from clsr_amd.ops import call

    z = torch.zeros(8, dtype=torch.float32, device=DEV)
    zi = torch.zeros(8, dtype=torch.int32, device=DEV)
    ok = (z, zi, 1, 4, 3, zi, 1, 1, 1, zi, z, 1)
    call("clsr_reco_rank_count", *ok)
    for k in (0, 1, 9, 10, 5):      # logit, items, partial, target_score on first, the history with remove_seen
        with pytest.raises(ClsrLibraryError, match="invalid argument"):
            call("clsr_reco_rank_count", *(ok[:k] + (None,) + ok[k + 1:]))
    call("clsr_reco_rank_count", z, zi, 1, 4, 3, None, 1, 1, 0, zi, None, 0)     # ... neither is needed otherwise
    for n_valid in (0, 4, -1):       # outside 1 .. g - 1
        with pytest.raises(ClsrLibraryError, match="invalid argument"):
            call("clsr_reco_rank_count", z, zi, 1, 4, n_valid, zi, 1, 1, 1, zi, z, 1)
    with pytest.raises(ClsrLibraryError, match="invalid argument"):
        call("clsr_reco_rank_count", z, zi, 1, 4, 3, zi, 0, 1, 1, zi, z, 1)      # a row stride below T
    for Hn, g, T in [(1, 1, 1), (1, 4, 257), (1, 4, 0), (0, 4, 1)]:
        with pytest.raises(ClsrLibraryError, match="unsupported shape"):
            call("clsr_reco_rank_count", z, zi, Hn, g, 1, zi, T, T, 1, zi, z, 1)
    fill = (zi, zi, 4, 0, 2, zi, zi, 2, zi, zi)
    call("clsr_reco_fill_ranked", *fill)
    for k in (0, 1, 5, 6, 8, 9):
        with pytest.raises(ClsrLibraryError, match="invalid argument"):
            call("clsr_reco_fill_ranked", *(fill[:k] + (None,) + fill[k + 1:]))
    for M, c0, g, Hn in [(4, 0, 1, 2), (4, 4, 2, 2), (4, -1, 2, 2), (0, 0, 2, 2), (4, 0, 2, 0)]:
        with pytest.raises(ClsrLibraryError, match="invalid argument"):
            call("clsr_reco_fill_ranked", zi, zi, M, c0, g, zi, zi, Hn, zi, zi)
    torch.cuda.synchronize()
