"""CPU tests of the dropout generator (clsr_amd/csrc/philox.h) through the host entry points of the C ABI: Philox4x32-10
known answers, the mask rule against a numpy restatement written here, and the kept fraction (no kernel is launched)."""
import ctypes

import numpy as np
import pytest

from clsr_amd import _lib

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(ctr, key):
    """numpy restatement: ``ctr`` [..., 4] and ``key`` [..., 2] uint32 -> [..., 4] uint32."""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k = [np.asarray(key[..., i], dtype=np.uint64) for i in range(2)]
    mask = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(W0)) & mask, (k[1] + np.uint64(W1)) & mask]
    return np.stack(c, -1).astype(np.uint32)


def threshold(keep):
    return int(round(keep * (1 << 24)))


def mask_np(seed, draw, layer, row0, B, C, thr):
    """The mask rule: counter (global row, column / 4, layer, draw), key (seed low, seed high), word k of the block serves
    column 4 (c / 4) + k, kept <=> (word >> 8) < thr."""
    Q = (C + 3) // 4
    ctr = np.zeros((B, Q, 4), dtype=np.uint32)
    ctr[..., 0] = ((row0 + np.arange(B, dtype=np.int64)) & 0xffffffff).astype(np.uint32)[:, None]
    ctr[..., 1] = np.arange(Q, dtype=np.uint32)[None, :]
    ctr[..., 2] = layer
    ctr[..., 3] = draw
    key = np.zeros((B, Q, 2), dtype=np.uint32)
    key[..., 0], key[..., 1] = seed & 0xffffffff, (seed >> 32) & 0xffffffff
    words = philox4x32_10(ctr, key).reshape(B, 4 * Q)[:, :C]
    return ((words >> np.uint32(8)) < np.uint32(thr)).astype(np.uint8)


def mask_lib(seed, draw, layer, row0, B, C, thr):
    lib = _lib.load()
    out = np.full((B, C), 7, dtype=np.uint8)
    assert lib.clsr_dropout_mask_host(seed, draw, layer, row0, B, C, thr, out.ctypes.data) == 0
    return out


KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,exp", KAT)
def test_philox_known_answers(ctr, key, exp):
    lib = _lib.load()
    c, k, o = (ctypes.c_uint32 * 4)(*ctr), (ctypes.c_uint32 * 2)(*key), (ctypes.c_uint32 * 4)()
    assert lib.clsr_philox4x32_10_host(c, k, o) == 0
    assert tuple(o) == exp
    # ... and the restatement the other tests compare against gives the same words
    assert tuple(int(v) for v in philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))) == exp


CASES = [(1, 4, 0), (5, 8, 0), (37, 100, 0), (3, 1024, 0), (257, 64, 1000003)]


@pytest.mark.parametrize("B,C,row0", CASES)
def test_mask_matches_restatement(B, C, row0):
    seed = 0x1234567890abcdef
    for keep, layer, draw in ((0.7, 0, 1), (0.5, 1, 3), (1.0, 1, 2)):
        thr = threshold(keep)
        got = mask_lib(seed, draw, layer, row0, B, C, thr)
        assert np.array_equal(got, mask_np(seed, draw, layer, row0, B, C, thr))
        if keep == 1.0:
            assert got.all()
    # every coordinate of the counter and both key words matter
    base = mask_lib(seed, 1, 0, row0, 64, 64, threshold(0.7))
    for other in (mask_lib(seed, 2, 0, row0, 64, 64, threshold(0.7)), mask_lib(seed, 1, 1, row0, 64, 64, threshold(0.7)),
                  mask_lib(seed + 1, 1, 0, row0, 64, 64, threshold(0.7)),
                  mask_lib(seed + (1 << 32), 1, 0, row0, 64, 64, threshold(0.7))):
        assert not np.array_equal(base, other)


def test_mask_is_a_function_of_the_global_row():
    thr = threshold(0.7)
    whole = mask_lib(11, 5, 1, 0, 300, 64, thr)
    for r, B in ((0, 300), (1, 7), (150, 150), (293, 7)):
        assert np.array_equal(whole[r:r + B], mask_lib(11, 5, 1, r, B, 64, thr))


def test_kept_fraction():
    frac = float(mask_lib(2024, 1, 0, 0, 1024, 64, threshold(0.7)).mean())
    # binomial: sigma = sqrt(0.7 * 0.3 / 65536) ~ 0.0018, five sigma
    assert abs(frac - 0.7) < 0.009, frac


def test_host_entry_points_reject_null():
    lib = _lib.load()
    assert lib.clsr_dropout_mask_host(0, 0, 0, 0, 4, 4, 1 << 23, None) == -1
    assert lib.clsr_philox4x32_10_host(None, None, None) == -1
