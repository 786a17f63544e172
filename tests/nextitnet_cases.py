"""Shapes, inputs and float64 reference of the kernel-level NextItNet tests (tests/test_nextitnet_kernels_gpu.py; checked on
the CPU by tests/test_nextitnet_cpu.py)  --  TEST INFRASTRUCTURE ONLY.

The slice, workgroup and LDS figures come from the kernels' own host-side queries (csrc/nextitnet.hip), never from literals
here.  Every case carries the seed of its inputs: tests/test_nextitnet_cpu.py holds that with it the float64 reference alone
meets the conditions the comparisons rest on -- every layer-norm row has variance >= 1e-4 (outside the gate case), no ReLU
input lies within 2^-16 of zero (outside the gate case's designed zeros), and a float32 evaluation opens the same gates."""
import functools
from collections import namedtuple

import numpy as np
import torch

import nextitnet_oracle as O
from clsr_amd.ops import query

Case = namedtuple("Case", "Hn T Di Dc k dilations seed what")

BUDGET = query("clsr_nextitnet_lds_budget_bytes")
POOL = 67            # distinct histories of the persistent-loop case (tiled over its history count)


def lds_bytes(T, C):
    return query("clsr_nextitnet_lds_bytes", T, C, 1)


def t_limit(C):
    """Longest history the backward's LDS slice admits at width C, by the kernel's own count."""
    T = 1
    while T < 256 and lds_bytes(T + 1, C) <= BUDGET:
        T += 1
    return T


T_AT_128, T_AT_40 = t_limit(128), t_limit(40)
SLICE_4_8 = query("clsr_nextitnet_slice", 4, 8, 1)
PARTS_MAX = query("clsr_nextitnet_parts", 1 << 30, 4, 8, 3, 1)

# (Hn, T, Di, Dc, k, dilations, seed, what the case reaches)
CASES = [
    Case(5, 50, 32, 8, 3, (1, 2, 4, 1, 2, 4), 0, "nextitnet.yaml's shape"),
    Case(2, 1, 4, 4, 3, (1, 2), 1, "T = 1: every older tap reads padding"),
    Case(3, 9, 4, 4, 3, (4,), 0, "(k - 1) d = T - 1: exactly one position sees the oldest tap"),
    Case(3, 9, 4, 4, 3, (64,), 0, "only the current tap is live"),
    Case(3, 12, 4, 4, 1, (1, 3), 0, "k = 1"),
    Case(3, 12, 4, 12, 8, (1,), 0, "k at its maximum, Dc > Di"),
    Case(1, 7, 4, 4, 2, (1,) * 16, 0, "16 blocks, one history"),
    Case(4, 16, 124, 4, 3, (1, 2), 0, "C = 128"),
    Case(PARTS_MAX * SLICE_4_8 + SLICE_4_8 + 3, 4, 4, 4, 3, (1, 2), 0,
         "more slices than workgroups: workgroup 0 walks a second slice, workgroup 1 a ragged one of 3 histories"),
    Case(2, T_AT_128, 124, 4, 2, (1,), 0, "C = 128 at the LDS limit: %d of %d bytes" % (lds_bytes(T_AT_128, 128), BUDGET)),
    Case(2, T_AT_40, 32, 8, 3, (1, 5), 1, "C = 40 at the LDS limit: %d of %d bytes" % (lds_bytes(T_AT_40, 40), BUDGET)),
    Case(1, 256, 4, 4, 2, (3,), 0, "T = 256, the trunk's longest history: %d bytes" % lds_bytes(256, 8)),
]
CONFIG, LIVE_TAP, MULTI = CASES[0], CASES[3], CASES[8]
# one step past each boundary of clsr_nextitnet_supported: (T, C, k, blocks) and what is past
PAST = [((T_AT_128 + 1, 128, 2, 1), "C = 128: %d bytes" % lds_bytes(T_AT_128 + 1, 128)),
        ((T_AT_40 + 1, 40, 3, 2), "C = 40: %d bytes" % lds_bytes(T_AT_40 + 1, 40)),
        ((257, 8, 2, 1), "T past 256"), ((8, 136, 2, 1), "C past 128"), ((8, 12, 2, 1), "C no multiple of 8"),
        ((8, 8, 9, 1), "k past 8"), ((8, 8, 2, 17), "17 blocks")]
GATE = Case(2, 3, 4, 4, 2, (1,), 0, "a position with variance exactly 0; beta = 0 in one channel")


def case_id(c):
    return "Hn%d-T%d-D%d+%d-k%d-d%s" % (c.Hn, c.T, c.Di, c.Dc, c.k, "x".join(map(str, c.dilations[:6])))


def _f32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32))


def _blocks(rng, C, k, n):
    h, out = C // 2, []
    u = lambda fan, *shape: _f32(rng.uniform(-1, 1, size=shape) * (6.0 / fan) ** 0.5)
    for _ in range(n):
        out.append(dict(be1=_f32(rng.randn(C) * 0.2), g1=_f32(1 + rng.randn(C) * 0.2), W1=u(C + h, C, h),
                        b1=_f32(rng.randn(h) * 0.1), be2=_f32(rng.randn(h) * 0.2), g2=_f32(1 + rng.randn(h) * 0.2),
                        Wd=u(k * h + h, k, h, h), bd=_f32(rng.randn(h) * 0.1), be3=_f32(rng.randn(h) * 0.2),
                        g3=_f32(1 + rng.randn(h) * 0.2), W2=u(h + C, h, C), b2=_f32(rng.randn(C) * 0.1)))
    return out


@functools.lru_cache(maxsize=None)
def make_inputs(c):
    """fp32 history rows x [Hn, T, C] (left-padded: the first steps of a history hold ONE non-zero row, the table's row 0),
    the blocks' variables and d x_L.  The persistent-loop case tiles POOL distinct histories."""
    rng = np.random.RandomState(2000 + c.seed)
    C = c.Di + c.Dc
    n = min(c.Hn, POOL)
    x = rng.randn(n, c.T, C) * 0.5
    row0 = rng.randn(C) * 0.5
    for h_ in range(n):
        x[h_, :rng.randint(0, c.T)] = row0
    dout = rng.randn(n, c.T, C)
    idx = np.arange(c.Hn) % n
    return dict(x=_f32(x)[idx], dout=_f32(dout)[idx], blocks=_blocks(rng, C, c.k, len(c.dilations)), pool=n)


def make_gate_inputs():
    """Everything on a dyadic grid (multiples of 1/8 for x, 1/16 for the variables).  Position (0, 1) holds the same value
    in every channel: its variance is exactly 0, LN1 gives exactly beta1 there, and beta1[2] = 0 -- a ReLU input of exactly
    zero, whose gate is closed.  beta1[0] > 0 and beta1[1] < 0 are an open and a closed gate beside it."""
    c = GATE
    rng = np.random.RandomState(77)
    C = c.Di + c.Dc
    q = lambda a, s: _f32(np.round(np.asarray(a) * s) / s)
    x = q(rng.randn(c.Hn, c.T, C) * 0.75, 8)
    x[0, 1, :] = 0.625
    blocks = [{k_: q(v.numpy(), 16) for k_, v in _blocks(rng, C, c.k, 1)[0].items()}]
    blocks[0]["be1"][:3] = torch.tensor([0.25, -0.25, 0.0])
    return dict(x=x, dout=q(rng.randn(c.Hn, c.T, C), 8), blocks=blocks, pool=c.Hn)


def reference(c, inp, dtype=torch.float64):
    """forward, the explicit backward and the conditions' figures in ``dtype``; in float64 also the bounds of x_L and of
    every block's input: four times what a float32 restatement measures on these inputs (nextitnet_oracle.fp32_bounds)"""
    blocks = [{k_: v.to(dtype) for k_, v in p.items()} for p in inp["blocks"]]
    x, dout = inp["x"].to(dtype), inp["dout"].to(dtype)
    xL, caches = O.stack_forward(x, blocks, c.dilations)
    dx, grads = O.stack_backward(caches, blocks, c.dilations, dout)
    v, y = O.conditions(caches)
    e_xL, e_in, ms = (None, None, None)
    if dtype == torch.float64:
        e_xL, e_in, ms = O.fp32_bounds(x, xL, caches, blocks, c.dilations, c.Di + c.Dc, c.k)
    return dict(xL=xL, e_xL=e_xL, e_inputs=e_in, fp32_measured=ms, dx=dx, dblock=O.pack_blocks(grads), grads=grads, min_var=v, min_pre=y,
                gates=O.gates(caches), caches=caches)


@functools.lru_cache(maxsize=None)
def case_data(c):
    inp = make_inputs(c)
    return inp, reference(c, inp)


# ------------------------------------------------------------------------------------------ step-level feeds
STEP_LENS = (1, 50, 25, 33, 12)          # real steps of the five histories of the step tests (T = 50)


def edge_feed(T, G, Vi, Vc, lens, seed=0, Vu=8):
    """A training feed in NextItNetIterator's layout without the iterator: ``len(lens)`` histories of the given real
    lengths, LEFT-padded with id 0, each repeated for its G rows; items / cates / labels [n G, T] -- row 0 of a group is the
    history one step on with a drawn target appended, the others are negatives that differ from the positive."""
    rng = np.random.RandomState(seed)
    n = len(lens)
    ih, ch = np.zeros((n, T), dtype=np.int32), np.zeros((n, T), dtype=np.int32)
    mask = np.zeros((n, T), dtype=np.float32)
    for i, ln in enumerate(lens):
        ih[i, T - ln:], ch[i, T - ln:], mask[i, T - ln:] = rng.randint(1, Vi, ln), rng.randint(1, Vc, ln), 1.0
    items, cates = np.zeros((n, G, T), dtype=np.int32), np.zeros((n, G, T), dtype=np.int32)
    items[:, 0, :-1], cates[:, 0, :-1] = ih[:, 1:], ch[:, 1:]
    items[:, 0, -1], cates[:, 0, -1] = rng.randint(1, Vi, n), rng.randint(1, Vc, n)
    neg = rng.randint(1, Vi - 1, (n, G - 1, T))
    items[:, 1:] = neg + (neg >= items[:, :1])          # (never the positive of its position)
    cates[:, 1:] = rng.randint(1, Vc, (n, G - 1, T))
    labels = np.zeros((n, G, T), dtype=np.float32)
    labels[:, 0] = 1.0
    rep = lambda a: np.repeat(a, G, axis=0)
    z = np.zeros((n * G, T), dtype=np.float32)
    return dict(labels=labels.reshape(n * G, T), users=rep(rng.randint(1, Vu, n).astype(np.int32)),
                items=items.reshape(n * G, T), cates=cates.reshape(n * G, T), item_history=rep(ih),
                item_cate_history=rep(ch), mask=rep(mask), time=np.zeros(n * G, dtype=np.float32), time_diff=z,
                time_from_first_action=z, time_to_now=z)
