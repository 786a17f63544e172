"""clsr_feed_same_rows and clsr_feed_build_eval alone (csrc/feed.hip) on synthetic columns, bit for bit: the run flags
against the numpy rule of clsr_amd/resident.py (held to ``_shared_history_group`` in tests/test_resident_eval_cpu.py), the
scoring feed against numpy indexing of the same columns inside an arena of canary bytes, and the refusals."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG = ("item_history", "item_cate_history", "time_from_first_action", "time_to_now")
F32 = ("time_from_first_action", "time_to_now", "labels", "denom")
N = 1200
RUN = 6
#: what one line of a run is made to differ in from the line before it (``same``: expected flag)
KINDS = (("first word", 0), ("last word", 0), ("users", 0), ("lens", 0), ("signed zero", 1), ("nan", 0), ("cate last", 0),
         ("time first", 0), ("users beyond float32", 1))


def _columns(T, rng):
    """1200 lines in runs of 6 with one history and one user; line 2 of run j differs from line 1 in ``KINDS[j % 9]``."""
    base = N // RUN
    rows = np.repeat(np.arange(base), RUN)
    c = {}
    for k in BIG[:2]:
        c[k] = rng.integers(0, 1 << 30, (base, T)).astype(np.int32)[rows]
    for k in BIG[2:]:
        a = rng.standard_normal((base, T)).astype(np.float32)
        a.reshape(-1)[::7] = -0.0
        a.reshape(-1)[3::11] = np.inf
        c[k] = a[rows]
    c["users"] = rng.integers(0, 1 << 20, base).astype(np.int32)[rows]
    c["lens"] = rng.integers(0, T + 1, base).astype(np.int32)[rows]
    c["items"] = rng.integers(0, 1 << 20, N).astype(np.int32)
    c["cates"] = rng.integers(0, 1 << 12, N).astype(np.int32)
    c["labels"] = (rng.random(N) < 0.3).astype(np.float32)
    want = {}
    for j in range(base):
        kind, same = KINDS[j % len(KINDS)]
        p = j * RUN + 2
        if kind == "first word":
            c["item_history"][p, 0] ^= 1
        elif kind == "last word":
            c["time_to_now"][p, T - 1] = c["time_to_now"][p - 1, T - 1] + 1.0 if np.isfinite(c["time_to_now"][p - 1, T - 1]) else 0.0
        elif kind == "users":
            c["users"][p] += 1
        elif kind == "lens":
            c["lens"][p] = (c["lens"][p] + 1) % (T + 1)
        elif kind == "signed zero":
            c["time_from_first_action"][p - 1, T // 2], c["time_from_first_action"][p, T // 2] = 0.0, -0.0
        elif kind == "nan":
            c["time_from_first_action"][p - 1:p + 1, T - 1] = np.nan
        elif kind == "cate last":
            c["item_cate_history"][p, T - 1] ^= 1 << 29
        elif kind == "time first":
            c["time_from_first_action"][p, 0] = 7.5 if c["time_from_first_action"][p - 1, 0] != 7.5 else 8.5
        else:
            c["users"][p - 1], c["users"][p] = 2 ** 24, 2 ** 24 + 1
        want[p] = same
    return c, want


def _to_device(c, shift=False):
    """The columns on the device; ``shift``: the [N, T] columns start 4 bytes past a 16-byte boundary."""
    cd = {}
    for k, v in c.items():
        t = torch.from_numpy(np.ascontiguousarray(v))
        if shift and k in BIG:
            buf = torch.empty(v.size + 1, dtype=t.dtype, device=DEV)
            buf[1:].copy_(t.reshape(-1))
            cd[k] = buf[1:].view(v.shape)
            assert cd[k].data_ptr() % 16 == 4 and cd[k].is_contiguous()
        else:
            cd[k] = t.to(DEV)
    return cd


def _flags(cd, keep, T):
    from clsr_amd import ops

    flags = torch.full((len(keep) + 16,), 0x5A, dtype=torch.uint8, device=DEV)
    ops.feed_same_rows(ops.feed_eval_pointers(cd), N, torch.from_numpy(keep).to(DEV), len(keep), T, flags)
    torch.cuda.synchronize()
    out = flags.cpu().numpy()
    assert (out[len(keep):] == 0x5A).all(), "bytes behind flags[n_keep]"
    return out[:len(keep)]


@pytest.mark.parametrize("T", [1, 3, 8, 50])
def test_same_rows_matches_the_numpy_rule(T):
    from clsr_amd.resident import same_rows

    rng = np.random.default_rng(T)
    c, want = _columns(T, rng)
    whole = same_rows(c, np.arange(N))
    for p, same in want.items():        # the rule itself sees every planted difference (and the two planted equalities)
        assert whole[p] == same and whole[p + 2] == 1, (p, KINDS[(p // RUN) % len(KINDS)])
    for shift in ((False, True) if T == 8 else (False,)):
        cd = _to_device(c, shift)
        for n_keep in (1, 2, 257, 1000):
            rising = (N - n_keep + np.arange(n_keep)).astype(np.int32)          # (ends on the file's last line)
            keeps = [rising, np.arange(n_keep, dtype=np.int32), rng.permutation(rising).astype(np.int32),
                     np.sort(rng.integers(0, N, n_keep)).astype(np.int32)]      # (non-decreasing, with repeats)
            for i, keep in enumerate(keeps):
                exp = same_rows(c, keep)
                got = _flags(cd, keep, T)
                assert np.array_equal(got, exp), (T, shift, n_keep, i, np.flatnonzero(got != exp)[:8])
                if n_keep >= 257 and i != 2:
                    assert 0 < exp.sum() < n_keep - 1


def test_same_rows_refuses_bad_sizes():
    from clsr_amd import _lib, ops

    c, _ = _columns(3, np.random.default_rng(0))
    cd = _to_device(c)
    keep = torch.arange(5, dtype=torch.int32, device=DEV)
    flags = torch.full((16,), 0x5A, dtype=torch.uint8, device=DEV)
    ptrs = ops.feed_eval_pointers(cd)
    for Nn, n_keep, T in ((0, 5, 3), (1 << 31, 5, 3), (N, 0, 3), (N, 1 << 31, 3), (N, 5, 0),
                          (N, 5, ops.query("clsr_feed_build_max_steps") + 1)):
        with pytest.raises(_lib.ClsrLibraryError, match="rc=-1"):
            ops.feed_same_rows(ptrs, Nn, keep, n_keep, T, flags)
    with pytest.raises(_lib.ClsrLibraryError, match="rc=-1"):
        ops.feed_same_rows(ptrs, N, None, 5, 3, flags)
    torch.cuda.synchronize()
    assert bool((flags == 0x5A).all())


def _arena(n, g, T, shift=0):
    """(device arena of canary bytes, output views, {name: (offset, shape, dtype)}): every piece 16-byte aligned (+ shift)
    with 16 canary bytes or more behind it; ``users_rows`` only when g > 1."""
    from clsr_amd import ops

    H = n // g
    shapes = dict(users=(H,), items=(n,), cates=(n,), item_history=(H, T), item_cate_history=(H, T),
                  time_from_first_action=(H, T), time_to_now=(H, T), labels=(n,), users_rows=(n,), seq_len=(H,), denom=(1,))
    if g == 1:
        del shapes["users_rows"]
    lay, off = {}, 16 + shift
    for k in ops.FEED_EVAL_OUTPUTS:
        if k in shapes:
            nb = 4 * int(np.prod(shapes[k]))
            lay[k] = (off, shapes[k], np.float32 if k in F32 else np.int32)
            off += (nb + 15) // 16 * 16 + 16
    arena = torch.full((off + 16,), 0x5A, dtype=torch.uint8, device=DEV)
    outs = {}
    for k, (o, shape, dt) in lay.items():
        nb = 4 * int(np.prod(shape))
        outs[k] = arena[o:o + nb].view(torch.float32 if k in F32 else torch.int32).view(shape)
    return arena, outs, lay


def _expect_arena(c, keep, k0, n, g, thr, lay, nbytes):
    lines = keep[k0:k0 + n]
    heads = lines[::g]
    as_fed = lambda u: u.astype(np.float32).astype(np.int32)        # (the float32 form of evaluation user ids)
    e = dict(users=as_fed(c["users"][heads]), items=c["items"][lines], cates=c["cates"][lines], labels=c["labels"][lines],
             users_rows=as_fed(c["users"][lines]), seq_len=c["lens"][heads])
    for k in BIG:
        e[k] = c[k][heads]
    e["denom"] = np.asarray([float(g * int((e["seq_len"] > thr).sum()))], dtype=np.float32)
    host = np.full(nbytes, 0x5A, dtype=np.uint8)
    for k, (o, shape, dt) in lay.items():
        a = np.ascontiguousarray(e[k], dtype=dt)
        assert a.shape == shape, k
        host[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    return host


CASES = ((1, 1), (5, 5), (257, 1), (300, 100), (1000, 2))


@pytest.mark.parametrize("T", [1, 3, 8, 50])
def test_build_eval_matches_numpy_indexing_inside_canaries(T):
    from clsr_amd import ops

    rng = np.random.default_rng(50 + T)
    c, _ = _columns(T, rng)
    c["users"][::17] = 2 ** 24 + 1          # survives int32, not float32
    c["users"][5::29] = -(2 ** 24 + 3)
    cd = _to_device(c)
    checked = 0
    for n, g in CASES:
        n_keep = n + 7
        keep = rng.integers(0, N, n_keep).astype(np.int32)
        keep[0], keep[-1], keep[n_keep // 2] = N - 1, 0, 17
        kd = torch.from_numpy(keep).to(DEV)
        for k0 in (0, 3, n_keep - n):
            for thr in (0, 5):
                for shift in ((0, 4) if T == 8 and k0 == 3 else (0,)):
                    arena, outs, lay = _arena(n, g, T, shift)
                    assert ("users_rows" in outs) == (g > 1)
                    assert ops.query("clsr_feed_build_eval_supported", N, n_keep, k0, n, g, T) == 1
                    ops.feed_build_eval(ops.feed_eval_pointers(cd, outs), N, kd, n_keep, k0, n, g, T, thr)
                    torch.cuda.synchronize()
                    got = arena.cpu().numpy()
                    exp = _expect_arena(c, keep, k0, n, g, thr, lay, arena.numel())
                    bad = np.flatnonzero(got != exp)
                    assert bad.size == 0, (T, n, g, k0, thr, shift, bad[:8])
                    checked += 1
    assert checked == 5 * 3 * 2 + (10 if T == 8 else 0)


def test_build_eval_refusals_leave_the_canaries_alone():
    from clsr_amd import _lib, ops

    T, n_keep = 8, 40
    c, _ = _columns(T, np.random.default_rng(3))
    cd = _to_device(c)
    kd = torch.arange(n_keep, dtype=torch.int32, device=DEV)
    arena, outs, _ = _arena(20, 5, T)
    ptrs = ops.feed_eval_pointers(cd, outs)
    steps = ops.query("clsr_feed_build_max_steps")
    #        N        n_keep   k0   n   g  T
    bad = [(N, n_keep, 0, 20, 0, T), (N, n_keep, 0, 20, -5, T),             # g < 1
           (N, n_keep, 0, 0, 5, T), (N, n_keep, 0, -20, 5, T),              # n < 1
           (N, n_keep, 0, 20, 3, T), (N, n_keep, 0, 20, 40, T),             # n % g != 0
           (N, n_keep, -1, 20, 5, T),                                       # k0 < 0
           (N, n_keep, 21, 20, 5, T), (N, n_keep, n_keep, 20, 5, T), (N, n_keep, 1 << 40, 20, 5, T),     # past keep
           (0, n_keep, 0, 20, 5, T), (1 << 31, n_keep, 0, 20, 5, T), (N, 1 << 31, 0, 20, 5, T),         # past int32
           (N, n_keep, 0, 20, 5, 0), (N, n_keep, 0, 20, 5, steps + 1)]
    for args in bad:
        assert ops.query("clsr_feed_build_eval_supported", *args) == 0, args
        Nn, nk, k0, n, g, Tt = args
        with pytest.raises(_lib.ClsrLibraryError, match="rc=-1"):
            ops.feed_build_eval(ptrs, Nn, kd, nk, k0, n, g, Tt, 0)
    assert ops.query("clsr_feed_build_eval_supported", N, n_keep, 20, 20, 5, T) == 1
    assert ops.query("clsr_feed_build_eval_supported", 1 << 30, (1 << 31) - 1, 0, (1 << 31) - 1, 1, steps) == 0   # rows * T
    # groups without a users_rows tensor, a missing output, a missing column, a null keep
    no_rows = {k: v for k, v in outs.items() if k != "users_rows"}
    with pytest.raises(_lib.ClsrLibraryError, match="rc=-1"):
        ops.feed_build_eval(ops.feed_eval_pointers(cd, no_rows), N, kd, n_keep, 0, 20, 5, T, 0)
    with pytest.raises(KeyError):
        ops.feed_eval_pointers(cd, {k: v for k, v in outs.items() if k != "denom"})
    with pytest.raises(KeyError):
        ops.feed_eval_pointers({k: v for k, v in cd.items() if k != "labels"}, outs)
    with pytest.raises(TypeError):
        ops.feed_eval_pointers(dict(cd, labels=cd["labels"].double()), outs)
    with pytest.raises(_lib.ClsrLibraryError, match="rc=-1"):
        ops.feed_build_eval(ptrs, N, None, n_keep, 0, 20, 5, T, 0)
    torch.cuda.synchronize()
    assert bool((arena == 0x5A).all())
    ops.feed_build_eval(ptrs, N, kd, n_keep, 20, 20, 5, T, 0)       # the same buffers serve a good call
    torch.cuda.synchronize()
    assert not bool((outs["items"].view(torch.uint8) == 0x5A).all())
