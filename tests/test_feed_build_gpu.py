"""clsr_feed_build alone (csrc/feed.hip) against a numpy restatement written here: every output bit for bit, on synthetic
columns -- file sizes 1 / 7 / 300, history widths 1 / 3 / 50 / 64 / 256 (4-byte and 16-byte rows), groups of 2 / 5 / 16,
batches of 5 / 63 / 64 / 65 / 257 lines (below, at and past one workgroup of the small part), compact and expanded, whole
batches and shards, and the refusal of an index that cannot be served."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG = ("item_history", "item_cate_history", "time_from_first_action", "time_to_now")


def _columns(N, T, rng):
    """Synthetic column store: lens cover 0, 1, T - 1, T; the float columns hold every kind of bit pattern."""
    lens = rng.integers(0, T + 1, N).astype(np.int32)
    for i, v in enumerate((T, 0, 1, max(T - 1, 0))):
        if i < N:
            lens[(i * 5) % N if N > 4 else i] = v
    c = dict(lens=lens)
    for k in ("users", "items", "cates"):
        c[k] = rng.integers(0, 1 << 20, N).astype(np.int32)
    for k in BIG[:2]:
        c[k] = rng.integers(0, 1 << 30, (N, T)).astype(np.int32)
    for k in BIG[2:]:
        a = rng.standard_normal((N, T)).astype(np.float32)
        flat = a.reshape(-1)
        flat[::7] = -0.0
        flat[3::11] = np.inf
        flat[5::13] = np.nan
        c[k] = a
    return c


def _expect(c, sel, src, G, expanded, thr, h0, n):
    own = sel[h0:h0 + n]
    rows = np.repeat(own, G) if expanded else own
    flat = sel[src[h0:h0 + n].reshape(-1)]
    lab = np.zeros((n, G), np.float32)
    lab[:, 0] = 1.0
    e = dict(users=c["users"][rows], items=c["items"][flat], cates=c["cates"][flat], labels=lab.reshape(-1),
             seq_len=c["lens"][rows])
    for k in BIG:
        e[k] = c[k][rows]
    rep = 1 if expanded else G
    e["denom"] = np.asarray([float(int((e["seq_len"] > thr).sum()) * rep)], dtype=np.float32)
    return e


def _outputs(n, T, G, expanded, shift=0):
    """Poisoned output tensors as views of one arena, every piece 16-byte aligned (+ ``shift`` bytes)."""
    from clsr_amd import ops

    R, B = (n * G if expanded else n), n * G
    shapes = dict(users=(R,), items=(B,), cates=(B,), item_history=(R, T), item_cate_history=(R, T),
                  time_from_first_action=(R, T), time_to_now=(R, T), labels=(B,), seq_len=(R,), denom=(1,))
    total = sum((4 * int(np.prod(s)) + 15) // 16 * 16 for s in shapes.values()) + 16
    arena = torch.full((total,), 0x5A, dtype=torch.uint8, device=DEV)
    outs, off = {}, shift
    for k in ops.FEED_OUTPUTS:
        nb = 4 * int(np.prod(shapes[k]))
        dt = torch.float32 if k in ("time_from_first_action", "time_to_now", "labels", "denom") else torch.int32
        outs[k] = arena[off:off + nb].view(dt).view(shapes[k])
        off += (nb + 15) // 16 * 16
    return arena, outs


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.int32)


def _recipes(N, n, G, rng):
    """sel ascending / reversed / shuffled with the file's last line; src rows that point at line 0, at line n - 1, at
    themselves, and anywhere."""
    base = np.sort(rng.integers(0, N, n)).astype(np.int32)
    base[-1] = N - 1
    shuffled = rng.permutation(base).astype(np.int32)
    src = rng.integers(0, n, (n, G)).astype(np.int32)
    src[:, 0] = np.arange(n)
    src[0, 1:] = 0
    src[1, 1:] = n - 1
    src[2, 1:] = 2
    src[n - 1, 1] = 0
    src[n - 2, G - 1] = n - 1
    return [(base, src), (np.ascontiguousarray(base[::-1]), src), (shuffled, src)]


def _run(cd, N, sel, src, h0, n, T, G, expanded, thr, outs, err):
    from clsr_amd import ops

    ptrs = ops.feed_pointers(cd, outs)
    ops.feed_build(ptrs, N, torch.from_numpy(sel).to(DEV), len(sel), torch.from_numpy(src).to(DEV), h0, n, T, G, expanded,
                   thr, err)
    torch.cuda.synchronize()


@pytest.mark.parametrize("expanded", [False, True])
@pytest.mark.parametrize("T", [1, 3, 50, 64, 256])
def test_feed_build_matches_numpy_bit_for_bit(T, expanded):
    from clsr_amd import ops

    rng = np.random.default_rng(100 * T + int(expanded))
    checked = 0
    for N in (1, 7, 300):
        c = _columns(N, T, rng)
        cd = {k: torch.from_numpy(v).to(DEV) for k, v in c.items()}
        err = torch.zeros(4, dtype=torch.int32, device=DEV)
        present = sorted(set(c["lens"].tolist()))
        for G in (2, 5, 16):
            for n in (5, 63, 64, 65, 257):
                assert ops.query("clsr_feed_build_supported", N, n, T, G) == 1
                recipes = _recipes(N, n, G, rng)
                # thresholds below, at and above the lengths that occur
                thrs = [present[0] - 1, present[len(present) // 2], present[-1]]
                for i, (sel, src) in enumerate(recipes):
                    thr = thrs[i % 3]
                    arena, outs = _outputs(n, T, G, expanded)
                    _run(cd, N, sel, src, 0, n, T, G, expanded, thr, outs, err)
                    exp = _expect(c, sel, src, G, expanded, thr, 0, n)
                    for k in ops.FEED_OUTPUTS:
                        assert outs[k].shape == exp[k].shape and np.array_equal(_bits(outs[k]), _bits(exp[k])), \
                            (k, N, T, G, n, i)
                    checked += 1
        ops.call("clsr_feed_error", err)        # raises if any call was refused
    assert checked == 3 * 3 * 5 * 3


@pytest.mark.parametrize("expanded", [False, True])
def test_feed_build_thresholds_shards_and_unaligned_rows(expanded):
    """denom for every threshold from below the shortest to above the longest history; lines h0 .. h0 + n - 1 of a batch
    (a data-parallel shard: src still points into the whole batch); rows of 64 words that do NOT start on 16 bytes."""
    from clsr_amd import ops

    rng = np.random.default_rng(9 + int(expanded))
    N, G, n_sel = 300, 5, 65
    err = torch.zeros(4, dtype=torch.int32, device=DEV)
    for T in (50, 64):
        c = _columns(N, T, rng)
        cd = {k: torch.from_numpy(v).to(DEV) for k, v in c.items()}
        sel, src = _recipes(N, n_sel, G, rng)[2]
        for thr in (-1, 0, 1, T - 1, T, T + 1):
            arena, outs = _outputs(n_sel, T, G, expanded)
            _run(cd, N, sel, src, 0, n_sel, T, G, expanded, thr, outs, err)
            exp = _expect(c, sel, src, G, expanded, thr, 0, n_sel)
            assert np.array_equal(_bits(outs["denom"]), _bits(exp["denom"])), (T, thr)
        for world in (2, 3):
            per = n_sel // world
            for rank in range(world):
                for shift in (0, 4):
                    arena, outs = _outputs(per, T, G, expanded, shift=shift)
                    _run(cd, N, sel, src, rank * per, per, T, G, expanded, 3, outs, err)
                    exp = _expect(c, sel, src, G, expanded, 3, rank * per, per)
                    for k in ops.FEED_OUTPUTS:
                        assert np.array_equal(_bits(outs[k]), _bits(exp[k])), (k, T, world, rank, shift)
    ops.call("clsr_feed_error", err)


@pytest.mark.parametrize("expanded", [False, True])
def test_feed_build_refuses_an_index_it_cannot_serve(expanded):
    """sel outside the file, src outside the batch: the error is reported with the index, and the poisoned outputs keep
    every byte; after clsr_feed_clear_error the same buffers serve a good call."""
    from clsr_amd import _lib, ops

    rng = np.random.default_rng(77)
    N, T, G, n = 7, 50, 5, 65
    c = _columns(N, T, rng)
    cd = {k: torch.from_numpy(v).to(DEV) for k, v in c.items()}
    sel, src = _recipes(N, n, G, rng)[0]
    cases = []
    for pos, val in ((0, N), (n - 1, -1), (33, 1 << 30)):
        bad = sel.copy()
        bad[pos] = val
        cases.append((bad, src, "sel[%d] = %d" % (pos, val)))
    for (r, g), val in (((0, 1), n), ((n - 1, G - 1), -1), ((40, 2), 1 << 30)):
        bad = src.copy()
        bad[r, g] = val
        cases.append((sel, bad, "src[%d] = %d" % (r * G + g, val)))
    for bsel, bsrc, what in cases:
        err = torch.zeros(4, dtype=torch.int32, device=DEV)
        arena, outs = _outputs(n, T, G, expanded)
        _run(cd, N, bsel, bsrc, 0, n, T, G, expanded, 3, outs, err)
        assert bool((arena == 0x5A).all()), what
        with pytest.raises(_lib.ClsrLibraryError) as ei:
            ops.call("clsr_feed_error", err)
        assert what in str(ei.value), (what, str(ei.value))
        # sticky: a good call afterwards works, the report stays until it is cleared
        _run(cd, N, sel, src, 0, n, T, G, expanded, 3, outs, err)
        exp = _expect(c, sel, src, G, expanded, 3, 0, n)
        for k in ops.FEED_OUTPUTS:
            assert np.array_equal(_bits(outs[k]), _bits(exp[k])), (k, what)
        with pytest.raises(_lib.ClsrLibraryError):
            ops.call("clsr_feed_error", err)
        ops.call("clsr_feed_clear_error", err)
        ops.call("clsr_feed_error", err)


def test_feed_build_rejects_sizes_it_does_not_serve():
    from clsr_amd import _lib, ops

    assert ops.query("clsr_feed_build_supported", 300, 64, 50, 5) == 1
    assert ops.query("clsr_feed_build_supported", 0, 64, 50, 5) == 0
    assert ops.query("clsr_feed_build_supported", 1 << 31, 64, 50, 5) == 0
    assert ops.query("clsr_feed_build_supported", 300, 64, 0, 5) == 0
    assert ops.query("clsr_feed_build_supported", 300, 64, ops.query("clsr_feed_build_max_steps") + 1, 5) == 0
    assert ops.query("clsr_feed_build_supported", 300, 64, 50, ops.query("clsr_feed_build_max_group") + 1) == 0
    assert ops.query("clsr_feed_build_supported", 300, (1 << 31) // 6 + 1, 50, 5) == 0
    rng = np.random.default_rng(1)
    c = _columns(7, 3, rng)
    cd = {k: torch.from_numpy(v).to(DEV) for k, v in c.items()}
    sel, src = _recipes(7, 5, 2, rng)[0]
    err = torch.zeros(4, dtype=torch.int32, device=DEV)
    arena, outs = _outputs(5, 3, 2, False)
    for h0, n in ((-1, 2), (0, 0), (3, 3)):             # a shard that is not inside the batch
        with pytest.raises(_lib.ClsrLibraryError):
            _run(cd, 7, sel, src, h0, n, 3, 2, False, 0, outs, err)
    with pytest.raises(TypeError):
        ops.feed_pointers(dict(cd, lens=cd["lens"].long()), outs)
    torch.cuda.synchronize()
    assert bool((arena == 0x5A).all())
