"""clsr_feed_build_pos alone against numpy, bit for bit: NextItNet training feeds (a target per position) built from a
resident column store, ``sel`` and ``psrc`` -- every length a line can have, whole batches and the shards of 2 and 3 ranks,
both word widths, both layouts; indices that cannot be served raise the sticky error words and leave the outputs alone."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 301
OUT_KEYS = ("users", "items", "cates", "item_history", "item_cate_history", "time_from_first_action", "time_to_now", "labels",
            "seq_len", "denom")
F32 = ("time_from_first_action", "time_to_now", "labels", "denom")
SENTINEL = 0x5A5A5A5A


def _columns(T, seed=0):
    """Left-padded columns of N lines; the first lines have 0, 1, T - 1 and T real steps, item / cate ids include 0."""
    rng = np.random.RandomState(seed)
    lens = rng.randint(0, T + 1, size=N).astype(np.int32)
    lens[:4] = (0, min(1, T), max(T - 1, 0), T)
    real = np.arange(T)[None, :] >= (T - lens[:, None])
    cols = {"item_history": (rng.randint(1, 1000, size=(N, T)) * real).astype(np.int32),
            "item_cate_history": (rng.randint(1, 50, size=(N, T)) * real).astype(np.int32),
            "time_from_first_action": (rng.standard_normal((N, T)) * real).astype(np.float32),
            "time_to_now": (rng.standard_normal((N, T)) * real).astype(np.float32),
            "lens": lens, "users": rng.randint(0, 90, size=N).astype(np.int32),
            "items": rng.randint(0, 1000, size=N).astype(np.int32), "cates": rng.randint(0, 50, size=N).astype(np.int32)}
    return cols


def _recipe(n_sel, G, T, seed):
    rng = np.random.RandomState(seed)
    sel = rng.randint(0, N, size=n_sel).astype(np.int32)
    sel[:4] = (0, 1, 2, 3)                              # the lines of 0, 1, T - 1 and T real steps are in every batch
    psrc = rng.randint(0, n_sel, size=(n_sel, G - 1, T)).astype(np.int32)
    psrc[0, 0, 0], psrc[-1, -1, -1] = n_sel - 1, 0      # the ends of the batch, pointed at from its other end
    return sel, psrc


def _reference(cols, sel, psrc, h0, n, G, expanded, thr):
    T = cols["item_history"].shape[1]
    lines = sel[h0:h0 + n]
    rows = np.repeat(lines, G) if expanded else lines
    out = {k: cols[k][rows] for k in ("item_history", "item_cate_history", "time_from_first_action", "time_to_now")}
    out["users"], out["seq_len"] = cols["users"][rows], cols["lens"][rows]
    for k, hist in (("items", "item_history"), ("cates", "item_cate_history")):
        a = np.empty((n, G, T), dtype=np.int32)
        a[:, 0, :T - 1], a[:, 0, T - 1] = cols[hist][lines][:, 1:], cols[k][lines]
        a[:, 1:] = cols[k][sel][psrc[h0:h0 + n]]
        out[k] = a.reshape(n * G, T)
    labels = np.zeros((n, G, T), dtype=np.float32)
    labels[:, 0] = 1.0
    out["labels"] = labels.reshape(-1)
    out["denom"] = np.asarray([float(int((cols["lens"][lines] > thr).sum()) * G)], dtype=np.float32)
    return out


class _Call(object):
    """Device copies of the columns and the recipe, and an output arena pre-filled with a sentinel.  ``shift``: the bases
    of psrc and of every [., T] output are moved by 4 bytes (rows no longer start on 16-byte boundaries)."""

    def __init__(self, cols, sel, psrc, n, G, expanded, shift=False):
        from clsr_amd.ops import query

        T = cols["item_history"].shape[1]
        dev = "cuda"
        self.cols = {k: torch.from_numpy(v).to(dev) for k, v in cols.items()}
        self.sel, self.n_sel, self.G, self.T, self.expanded = torch.from_numpy(sel).to(dev), len(sel), G, T, expanded
        o = 1 if shift else 0
        p = torch.empty(psrc.size + 4, dtype=torch.int32, device=dev)
        assert p.data_ptr() % 16 == 0
        self.psrc = p[o:o + psrc.size]
        self.psrc.copy_(torch.from_numpy(psrc.reshape(-1)))
        R, B = (n * G if expanded else n), n * G
        shapes = {"users": (R,), "items": (B, T), "cates": (B, T), "item_history": (R, T), "item_cate_history": (R, T),
                  "time_from_first_action": (R, T), "time_to_now": (R, T), "labels": (B * T,), "seq_len": (R,), "denom": (1,)}
        self.outs, self.raw = {}, []
        for k in OUT_KEYS:
            size = int(np.prod(shapes[k]))
            raw = torch.full((size + 8,), SENTINEL, dtype=torch.int32, device=dev)
            assert raw.data_ptr() % 16 == 0
            self.raw.append(raw)
            v = raw[o:o + size].view(shapes[k])
            self.outs[k] = v.view(torch.float32) if k in F32 else v
        self.scratch = torch.full((query("clsr_feed_build_pos_scratch_ints", len(sel)),), SENTINEL, dtype=torch.int32,
                                  device=dev)
        self.err = torch.zeros(4, dtype=torch.int32, device=dev)

    def run(self, h0, n, thr=0, N_=N):
        from clsr_amd import ops

        ptrs = ops.feed_pointers(self.cols, self.outs)
        ops.feed_build_pos(ptrs, N_, self.sel, self.n_sel, self.psrc, h0, n, self.T, self.G, self.expanded, thr, self.scratch,
                           self.err)
        torch.cuda.synchronize()

    def check(self, want, what):
        for k in OUT_KEYS:
            got = self.outs[k].cpu().numpy()
            assert got.dtype == want[k].dtype and got.shape == want[k].shape, (what, k, got.shape, want[k].shape)
            assert got.tobytes() == want[k].tobytes(), (what, k)
        for raw, k in zip(self.raw, OUT_KEYS):          # nothing is written around a tensor
            size = self.outs[k].numel()
            edge = torch.cat((raw[:1], raw[size + 1:])) if self.outs[k].data_ptr() != raw.data_ptr() else raw[size:]
            assert bool((edge == SENTINEL).all()), (what, k)

    def untouched(self):
        return all(bool((raw == SENTINEL).all()) for raw in self.raw)


@pytest.mark.parametrize("G", [2, 5])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 7, 8, 50])
def test_whole_batches_and_shards_equal_numpy(T, G):
    """n = 5, 6, 64, 257 lines (257 * 5 * 50 words: more than one workgroup in every region of the grid); the whole batch in
    both layouts, then the shards (h0, per) of 2 and 3 ranks, whose psrc points anywhere in the global batch; T % 4 == 0 with
    aligned bases (16-byte words) and with every base moved by 4 bytes (4-byte words)."""
    from clsr_amd.ops import query

    cols = _columns(T, seed=T)
    for n_sel in (5, 6, 64, 257):
        assert query("clsr_feed_build_pos_supported", N, n_sel, T, G) == 1
        sel, psrc = _recipe(n_sel, G, T, seed=n_sel + G)
        for shift in ((False, True) if T % 4 == 0 else (False,)):
            for expanded in (1, 0):
                c = _Call(cols, sel, psrc, n_sel, G, expanded, shift)
                thr = 0 if expanded else T // 2
                c.run(0, n_sel, thr)
                c.check(_reference(cols, sel, psrc, 0, n_sel, G, expanded, thr), (n_sel, shift, expanded))
                assert c.err.cpu().tolist() == [0, 0, 0, 0]
            for world in (2, 3):
                per = n_sel // world
                for rank in range(world):
                    h0 = rank * per
                    p = psrc.copy()
                    p[h0, 0, 0] = (h0 + per) % n_sel    # a line of another rank's shard (or of the dropped remainder)
                    c = _Call(cols, sel, p, per, G, 1, shift)
                    c.run(h0, per)
                    c.check(_reference(cols, sel, p, h0, per, G, 1, 0), (n_sel, shift, world, rank))


@pytest.mark.parametrize("T", [4, 7])
def test_bad_indices_raise_the_error_words_and_write_nothing(T):
    from clsr_amd import ops
    from clsr_amd._lib import ClsrLibraryError

    G, n_sel = 3, 64
    cols = _columns(T)
    sel, psrc = _recipe(n_sel, G, T, seed=1)
    h0, per = 32, 32                                    # the second shard of two
    cases = []
    for v in (-1, N):
        bad = sel.copy()
        bad[7] = v                                      # (outside the shard: every sel is held, psrc may point there)
        cases.append((bad, psrc, 1, 7, v))
    for v in (-1, n_sel):
        bad = psrc.copy()
        bad[40, 1, T - 2] = v
        cases.append((sel, bad, 3, (40 * (G - 1) + 1) * T + T - 2, v))
    for s, p, code, index, value in cases:
        c = _Call(cols, s, p, per, G, 1)
        c.run(h0, per)
        assert c.err.cpu().tolist() == [code, index, value, 1]
        assert c.untouched() and bool((c.scratch[:2 * n_sel] == SENTINEL).all())      # (no target was looked up)
        with pytest.raises(ClsrLibraryError, match="psrc" if code == 3 else "sel"):
            ops.call("clsr_feed_error", c.err)
        # sticky: a good call on the same words builds its feed and clears the status of the launch, not the report
        good = _Call(cols, sel, psrc, per, G, 1)
        good.err = c.err
        good.run(h0, per)
        good.check(_reference(cols, sel, psrc, h0, per, G, 1, 0), "after an error")
        assert c.err.cpu().tolist() == [code, index, value, 0]
        with pytest.raises(ClsrLibraryError):
            ops.call("clsr_feed_error", c.err)
        ops.call("clsr_feed_clear_error", c.err)
        ops.call("clsr_feed_error", c.err)
    # the first of two bad values is the one reported (sel before psrc, then the lower index)
    bad = psrc.copy()
    bad[33, 0, 0], bad[50, 1, 1] = n_sel + 5, -3
    c = _Call(cols, sel, bad, per, G, 1)
    c.run(h0, per)
    assert c.err.cpu().tolist() == [3, 33 * (G - 1) * T, n_sel + 5, 1] and c.untouched()
    # ... also when the scan that finds them takes more than one workgroup (51 657 positions, 26 workgroups)
    cols50 = _columns(50)
    sel50, psrc50 = _recipe(257, 5, 50, seed=3)
    bad = psrc50.copy()
    bad[200, 3, 49], bad[30, 2, 7] = -1, 257
    c = _Call(cols50, sel50, bad, 257, 5, 1)
    c.run(0, 257)
    assert c.err.cpu().tolist() == [3, (30 * 4 + 2) * 50 + 7, 257, 1] and c.untouched()
    # a bad psrc OUTSIDE the shard is not this call's business: it is neither read nor reported
    bad = psrc.copy()
    bad[3, 0, 0], bad[31, 1, T - 1] = -1, n_sel
    c = _Call(cols, sel, bad, per, G, 1)
    c.run(h0, per)
    assert c.err.cpu().tolist() == [0, 0, 0, 0]
    c.check(_reference(cols, sel, psrc, h0, per, G, 1, 0), "bad psrc outside the shard")


def test_unsupported_shapes_are_refused_without_a_launch():
    from clsr_amd._lib import ClsrLibraryError
    from clsr_amd.ops import query

    ok = lambda *a: query("clsr_feed_build_pos_supported", *a)
    tmax, gmax = query("clsr_feed_build_max_steps"), query("clsr_feed_build_max_group")
    assert ok(N, 64, 50, 5) == 1 and ok(1, 1, 1, 2) == 1 and ok(2 ** 31 - 1, 64, tmax, gmax) == 1
    assert ok(0, 64, 50, 5) == 0 and ok(2 ** 31, 64, 50, 5) == 0 and ok(N, 0, 50, 5) == 0
    assert ok(N, 64, 0, 5) == 0 and ok(N, 64, tmax + 1, 5) == 0
    assert ok(N, 64, 50, 1) == 0 and ok(N, 64, 50, gmax + 1) == 0        # (G = 1: no negative row, no psrc)
    assert ok(N, 2 ** 31 // 250 - 2, 50, 5) == 1 and ok(N, 2 ** 31 // 250, 50, 5) == 0
    T, G, n_sel = 4, 3, 8
    cols = _columns(T)
    sel, psrc = _recipe(n_sel, G, T, seed=2)
    c = _Call(cols, sel, psrc, n_sel, G, 1)
    c.G = 1
    with pytest.raises(ClsrLibraryError, match="rc=-3"):
        c.run(0, n_sel)
    c.G = G
    for h0, n in ((0, 0), (-1, 4), (4, 5)):             # lines outside the batch
        with pytest.raises(ClsrLibraryError, match="rc=-1"):
            c.run(h0, n)
    with pytest.raises(ClsrLibraryError, match="rc=-3"):
        c.run(0, n_sel, N_=0)
    assert c.untouched() and c.err.cpu().tolist() == [0, 0, 0, 0]
