"""Shapes and inputs of the kernel-level Caser tests (tests/test_caser_kernels_gpu.py, checked on the CPU by
tests/test_caser_cpu.py)  --  TEST INFRASTRUCTURE ONLY.

Inputs sit on a dyadic grid: history rows are multiples of 1/4 in [-1, 1], kernels multiples of 1/8 in [-1/2, 1/2], biases
multiples of 1/32 in [-2, 2].  Every product is then a multiple of 1/32 and every partial sum of at most 256 * 252 of them
stays below 2^24 / 32, so ANY fp32 summation order gives the exact pre-activation: the forward is compared bit for bit, and
no pool sits at a near-tie.  Ties themselves are plentiful, as in training: the histories are gathered by id from a small
table, left-aligned and padded with id 0 (whose row is NOT zero)."""
import functools
from collections import namedtuple

import numpy as np
import torch

import caser_oracle as O

Case = namedtuple("Case", "Hn T Di Dc L n_v n_h seed what")

# (Hn, T, Di, Dc, L, n_v, n_h), the seed of its inputs (chosen on the CPU so that the three conditions of
# ``conditions`` hold on the reference), what it reaches in csrc/caser.hip
CASES = [
    Case(5, 50, 32, 8, 3, 128, 128, 0, "config shape, PW = 512: the d hist column loop strides twice, LDS holds 1280 words"),
    Case(17, 24, 8, 4, 3, 4, 8, 0, "16 weight-gradient slices of 2 histories, the last seven empty"),
    Case(37, 16, 4, 8, 2, 8, 4, 0, "slices of 3, the last one a single history; Dc > Di"),
    Case(1, 9, 4, 4, 9, 4, 4, 0, "L = T: one window; one slice writes the gradient block itself (4-float workspace)"),
    Case(3, 120, 252, 4, 3, 4, 4, 0, "chunk of 56: boundaries at 56 and 112 fall inside mask words"),
    Case(2, 64, 4, 252, 58, 4, 4, 0, "chunk of 8 with 57 overlap rows, forward LDS at its limit (65 520 B), cate is the wide table"),
    Case(2, 256, 8, 4, 5, 4, 4, 0, "four full chunks, 9 tie words"),
    Case(2, 129, 8, 4, 5, 4, 4, 0, "third chunk of one position"),
    Case(2, 72, 8, 4, 10, 4, 4, 0, "second chunk in which the widest filters have no whole window"),
    Case(3, 70, 8, 4, 70, 4, 4, 0, "L = T > chunk"),
    Case(2, 8, 4, 4, 5, 1024, 1024, 0, "n_v + 3 L n_h = 16 384: backward LDS exactly 64 KB"),
    Case(4, 256, 128, 4, 2, 512, 4, 0, "the workspace caps the slices at 3, the third is empty"),
]
CONFIG, SLICES_17, SLICES_37, CHUNK_56, LDS_BWD, WS_CAPPED = (CASES[i] for i in (0, 1, 2, 4, 10, 11))
GATES = Case(3, 12, 4, 4, 2, 4, 4, 0, "a pooled maximum of exactly 0 and a filter negative everywhere")

SMALL_IDS, LARGE_IDS = 6, 4096      # ids 0 .. 5 repeat (ties); ids 6 .. 4101 give rows that are all different


def case_id(c):
    return "Hn%d-T%d-Di%d-Dc%d-L%d-nv%d-nh%d" % tuple(c[:7])


def lengths(c):
    """Real steps per history and whether its ids come from the large range: length 1, length T, a length that ends inside
    a mask word, and a full row of the large id range (single-winner pools); cases of fewer histories keep the first and
    the last kinds; further histories draw their length."""
    mid = c.T // 2 + 1
    mid += mid % 32 == 0
    kinds = [(1, False), (c.T, False), (mid, False), (c.T, True)]
    if c.Hn < 4:
        kinds = {1: [(c.T, True)], 2: [(1, False), (c.T, True)], 3: [(1, False), (mid, False), (c.T, True)]}[c.Hn]
    return kinds


def _grid(rng, shape, step, lim):
    k = int(round(lim / step))
    return torch.from_numpy(rng.randint(-k, k + 1, size=shape).astype(np.float64) * step)


def _ids(rng, c):
    ids = np.zeros((c.Hn, c.T), np.int64)
    kinds = lengths(c)
    for r in range(c.Hn):
        n, large = kinds[r] if r < len(kinds) else (int(rng.randint(1, c.T + 1)), False)
        ids[r, :n] = rng.randint(SMALL_IDS, SMALL_IDS + LARGE_IDS, n) if large else rng.randint(1, SMALL_IDS, n)
    return torch.from_numpy(ids)


def _block(rng, T, Dx, L, n_v, n_h):
    blk = dict(Wv=_grid(rng, (Dx, T, n_v), 0.125, 0.5), bv=_grid(rng, (n_v,), 1 / 32, 2.0), Wh=[], bh=[])
    for h in range(1, L + 1):
        blk["Wh"].append(_grid(rng, (h, Dx, n_h), 0.125, 0.5))
        blk["bh"].append(_grid(rng, (n_h,), 1 / 32, 2.0))
    return blk


def make_inputs(c, n_v=None):
    """float64 on the grid: X / blk per table ("item", "cate"); dpool [Hn, 2 PW] and the prior content of d hist
    [Hn, T, Di + Dc]: ordinary float32 normal data.  ``n_v`` overrides the case's (the CPU test of the widest case)."""
    n_v = c.n_v if n_v is None else n_v
    rng = np.random.RandomState(1000 + c.seed)
    inp = dict(X={}, blk={})
    for key, Dx in (("item", c.Di), ("cate", c.Dc)):
        table = _grid(rng, (SMALL_IDS + LARGE_IDS, Dx), 0.25, 1.0)
        table[0, 0] = 0.75        # (the padding row is not zero, whatever was drawn)
        inp["X"][key] = table[_ids(rng, c)]
        inp["blk"][key] = _block(rng, c.T, Dx, c.L, n_v, c.n_h)
    gen = torch.Generator().manual_seed(2000 + c.seed)
    inp["dpool"] = torch.randn(c.Hn, 2 * (n_v + c.L * c.n_h), generator=gen, dtype=torch.float32)
    inp["prior"] = torch.randn(c.Hn, c.T, c.Di + c.Dc, generator=gen, dtype=torch.float32)
    return inp


def make_gate_inputs():
    """GATES with the biases moved so that, per table and path, filter 0 has a maximum of EXACTLY 0 in history 0 (the gate
    ``pooled > 0`` is closed there) and filter 1 is negative at every position of every history."""
    inp = make_inputs(GATES)
    for key in ("item", "cate"):
        X, blk = inp["X"][key], inp["blk"][key]
        blk["bv"][0] -= O.vertical_pre(X, blk["Wv"], blk["bv"])[0, 0]
        blk["bv"][1] = -64.0
        for W, b in zip(blk["Wh"], blk["bh"]):
            b[0] -= O.horizontal_pre(X, W, b)[0, :, 0].max()
            b[1] = -64.0
    return inp


def reference(inp):
    """The float64 reference of a case: pooled / masks per table, the explicit backward and its |.| evaluation S."""
    ref = dict(pooled={}, masks={}, dX={}, dblk={}, SX={}, Sblk={})
    PW = inp["dpool"].shape[1] // 2
    for i, key in enumerate(("item", "cate")):
        X, blk = inp["X"][key], inp["blk"][key]
        dp = inp["dpool"][:, i * PW:(i + 1) * PW].double()
        ref["pooled"][key], m = O.block_forward(X, blk)
        ref["masks"][key] = m
        ref["dX"][key], ref["dblk"][key] = O.explicit_backward(X, blk, dp, m)
        ref["SX"][key], ref["Sblk"][key] = O.explicit_backward(X.abs(), O.map_block(blk, torch.abs), dp.abs(), m)
    return ref


@functools.lru_cache(maxsize=None)
def case_data(c):
    """(inputs, reference) of a case of the table, computed once and shared by the tests (never modified)."""
    inp = make_inputs(c)
    return inp, reference(inp)


def conditions(c, masks):
    """What the inputs of a case must offer, counted on the REFERENCE's masks of both tables: open pools with one winner,
    open pools whose tied positions span two mask words (asked for when T > 32), closed gates."""
    single = spanning = closed = 0
    for m in masks.values():
        closed += int((~m["gate_v"]).sum())
        for M, n, gate in zip(m["M"], m["n"], m["gate"]):
            closed += int((~gate).sum())
            single += int((gate & (n == 1)).sum())
            pos = torch.arange(M.shape[1]).view(1, -1, 1)
            lo = torch.where(M, pos, torch.full_like(pos, 1 << 20)).amin(1)
            hi = torch.where(M, pos, torch.full_like(pos, -1)).amax(1)
            spanning += int((gate & (n > 1) & (lo // 32 != hi // 32)).sum())
    return dict(single=single, spanning=spanning, closed=closed)


def conditions_hold(c, masks):
    k = conditions(c, masks)
    return k["single"] > 0 and k["closed"] > 0 and (c.T <= 32 or k["spanning"] > 0), k


def edge_feed(T, G, Vi, Vc, lens=None, seed=11):
    """A training feed of a few histories -- by default one real step, a full one, one that ends mid-way -- each repeated for
    its 1 + (G - 1) candidate rows; left-aligned, padded with id 0."""
    rng = np.random.RandomState(seed)
    lens = [1, T, 33] if lens is None else list(lens)
    Hn, B = len(lens), len(lens) * G
    ih, ch, mask = (np.zeros((Hn, T), np.int32) for _ in range(3))
    for r, n in enumerate(lens):
        ih[r, :n], ch[r, :n], mask[r, :n] = rng.randint(1, Vi, n), rng.randint(1, Vc, n), 1
    t = np.cumsum(rng.rand(Hn, T).astype(np.float32), 1) * mask
    rep = lambda a: np.repeat(a, G, axis=0)
    labels = np.zeros((B, 1), np.float32)
    labels[::G] = 1
    return dict(users=rep(np.arange(1, Hn + 1, dtype=np.int32)), items=rng.randint(1, Vi, B).astype(np.int32),
                cates=rng.randint(1, Vc, B).astype(np.int32), item_history=rep(ih), item_cate_history=rep(ch),
                mask=rep(mask), time_from_first_action=rep(t), time_to_now=rep(t[:, ::-1].copy()), labels=labels,
                time=np.zeros(B, np.float32), time_diff=rep(t))


# the training step at caser.yaml's widths and length (tests/test_caser_gpu.py): five histories of 1, 50 and mid-way steps;
# tests/test_caser_cpu.py pins that with this seed the float32 and the float64 oracle select alike
CONFIG_STEP = dict(T=50, lens=(1, 50, 25, 33, 12), dims=dict(Vu=8, Vi=30, Vc=7), seed=11)
