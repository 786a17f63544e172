"""Shapes, inputs and float64 reference of the kernel-level SASRec tests (tests/test_sasrec_kernels_gpu.py; checked on the CPU
by tests/test_sasrec_cpu.py)  --  TEST INFRASTRUCTURE ONLY.

The slice, workgroup and LDS figures come from the kernels' own host-side queries (csrc/sasrec.hip), never from literals
here.  Every case carries the seed of its inputs: tests/test_sasrec_cpu.py holds that with it the float64 reference alone
meets the conditions the comparisons rest on -- every layer-norm row of a valid step has variance >= 1e-4, no ReLU input
lies within 2^-16 of zero, and a float32 evaluation opens the same gates.  The rows of padding hold drawn values, not
zeros: a kernel that read them would show."""
import functools
from collections import namedtuple

import numpy as np
import torch

import sasrec_oracle as O
from clsr_amd.ops import query

Case = namedtuple("Case", "Hn T Tmax Di Dc nb nh lens seed what")

BUDGET = query("clsr_sasrec_lds_budget_bytes")
C_MAX, NB_MAX, T_MAX = (query("clsr_sasrec_max_" + n) for n in ("channels", "blocks", "steps"))
POOL = 67            # distinct histories of the persistent-loop case (tiled over its history count)


def lds_bytes(T, C):
    return query("clsr_sasrec_lds_bytes", T, C, 1)


def lds_formula(T, C):
    """The README's formula of the backward's one-history slice, in bytes"""
    return 4 * (9 * T * (C + 1) + T * (C // 2 + 1) + 2)


def t_limit(C):
    """Longest history the backward's LDS slice admits at width C, by the kernel's own count."""
    T = 1
    while T < T_MAX and lds_bytes(T + 1, C) <= BUDGET:
        T += 1
    return T


T_AT_MAX, T_AT_40 = t_limit(C_MAX), t_limit(40)
SLICE_4_8, SLICE_9_8 = query("clsr_sasrec_slice", 4, 8, 1), query("clsr_sasrec_slice", 9, 8, 1)
PARTS_MAX = query("clsr_sasrec_parts", 1 << 30, 4, 4, 8, 1)

# (Hn, T, rows of pos, Di, Dc, blocks, heads, lengths (cycled over the histories), seed, what the case reaches)
CASES = [
    Case(3, 50, 50, 32, 8, 2, 1, (1, 50, 25), 0, "sasrec.yaml's shape"),
    Case(2, 1, 1, 4, 4, 2, 1, (1,), 0, "T = 1"),
    Case(3, 9, 12, 4, 4, 1, 2, (1,), 0, "len = 1 inside T = 9; three rows of pos past T"),
    Case(2, 9, 9, 4, 4, 1, 1, (9,), 0, "len = T"),
    Case(5, 6, 6, 4, 4, 2, 2, (3, 0, 6, 1, 5), 0, "mixed lengths in one slice, one history of len = 0; dh = 4 at C = 8"),
    Case(2, 8, 8, C_MAX - 4, 4, 1, C_MAX // 4, (8, 5), 0, "the widest C with the most heads (dh = 4)"),
    Case(2, 8, 8, 4, C_MAX - 4, 2, 1, (7, 2), 0, "the widest C with one head, Dc > Di"),
    Case(2, 7, 7, 4, 4, NB_MAX, 1, (7, 3), 0, "the most blocks"),
    Case(SLICE_9_8 + 1, 9, 9, 4, 4, 1, 1, (4, 9, 1, 6), 0, "one history past a slice: the second workgroup holds one"),
    Case(PARTS_MAX * SLICE_4_8 + SLICE_4_8 + 3, 4, 4, 4, 4, 2, 1, (2, 4, 1, 3, 4, 0, 1), 0,
         "the cap of the partial rows: workgroup 0 walks a second slice, workgroup 1 a ragged one of 3 histories"),
    Case(2, T_AT_MAX, T_AT_MAX, 32, C_MAX - 32, 1, 2, (T_AT_MAX, 11), 0,
         "C = %d at the LDS limit: %d of %d bytes" % (C_MAX, lds_bytes(T_AT_MAX, C_MAX), BUDGET)),
    Case(2, T_AT_40, T_AT_40, 32, 8, 1, 1, (T_AT_40, 40), 0,
         "C = 40 at the LDS limit: %d of %d bytes" % (lds_bytes(T_AT_40, 40), BUDGET)),
    Case(3, 64, 64, 32, 8, 2, 2, (64, 33, 1), 1, "T = 64 at C = 40: %d bytes" % lds_bytes(64, 40)),
]
CONFIG, MIXED, POS_PAST_T, MULTI = CASES[0], CASES[4], CASES[2], CASES[9]
# one step past each boundary of clsr_sasrec_supported: (T, Tmax, C, blocks, heads) and what is past
PAST = [((T_AT_MAX + 1, T_AT_MAX + 1, C_MAX, 1, 1), "C = %d: %d bytes" % (C_MAX, lds_bytes(T_AT_MAX + 1, C_MAX))),
        ((T_AT_40 + 1, T_AT_40 + 1, 40, 1, 1), "C = 40: %d bytes" % lds_bytes(T_AT_40 + 1, 40)),
        ((T_MAX + 1, T_MAX + 1, 8, 1, 1), "T past %d" % T_MAX), ((8, 7, 8, 1, 1), "fewer rows of pos than steps"),
        ((8, 8, C_MAX + 8, 1, 1), "C past %d" % C_MAX), ((8, 8, 12, 1, 1), "C no multiple of 8"),
        ((8, 8, 8, NB_MAX + 1, 1), "%d blocks" % (NB_MAX + 1)), ((8, 8, 8, 0, 1), "no block"),
        ((8, 8, 24, 1, 4), "heads that do not divide C"), ((8, 8, 8, 1, 4), "dh = 2")]


def case_id(c):
    return "Hn%d-T%d-D%d+%d-b%d-h%d" % (c.Hn, c.T, c.Di, c.Dc, c.nb, c.nh)


def _f32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32))


def _encoder(rng, Tmax, C, nb):
    u = lambda: _f32(rng.uniform(-1, 1, size=(C, C)) * (3.0 / C) ** 0.5)
    gain, bias = (lambda: _f32(1 + rng.randn(C) * 0.2)), (lambda: _f32(rng.randn(C) * 0.2))
    blocks = []
    for _ in range(nb):
        blocks.append(dict(g1=gain(), be1=bias(), Wq=u(), bq=bias(), Wk=u(), bk=bias(), Wv=u(), bv=bias(), Wo=u(), bo=bias(),
                           g2=gain(), be2=bias(), W1=u(), b1=bias(), W2=u(), b2=bias()))
    return dict(pos=_f32(rng.randn(Tmax, C) * 0.3), blocks=blocks, gf=gain(), bef=bias())


@functools.lru_cache(maxsize=None)
def make_inputs(c):
    """fp32 history rows hist [Hn, T, C] (every row drawn, the padding too), the lengths, the encoder's variables and d s.
    A case of more than POOL histories tiles POOL distinct ones."""
    rng = np.random.RandomState(3000 + c.seed)
    C = c.Di + c.Dc
    n = min(c.Hn, POOL)
    hist, ds = _f32(rng.randn(n, c.T, C) * 0.5), _f32(rng.randn(n, C))
    enc = _encoder(rng, c.Tmax, C, c.nb)
    idx = np.arange(c.Hn) % n
    lens = torch.tensor([c.lens[i % len(c.lens)] for i in idx], dtype=torch.int64)
    return dict(hist=hist[idx], ds=ds[idx], lens=lens, enc=enc)


def reference(c, inp, dtype=torch.float64):
    """forward, the explicit backward and the conditions' figures in ``dtype``; in float64 also the bounds of s and of every
    saved tensor: four times what a float32 restatement measures on these inputs (sasrec_oracle.fp32_bounds)"""
    enc = O.cast(inp["enc"], dtype)
    hist, ds, lens = inp["hist"].to(dtype), inp["ds"].to(dtype), inp["lens"]
    s, cache = O.encoder_forward(hist, lens, enc, c.nh)
    dhist, grads = O.encoder_backward(cache, enc, c.nh, ds)
    v, z = O.conditions(cache)
    bounds, errs = (None, None)
    if dtype == torch.float64:
        n = min(c.Hn, POOL)         # (the tiled histories repeat the pool's: the same errors)
        bounds, errs = O.fp32_bounds(hist[:n], lens[:n], enc, c.nh)
    return dict(s=s, cache=cache, dhist=dhist, grads=grads, dblock=O.pack(grads), bounds=bounds, fp32_errors=errs, min_var=v,
                min_pre=z, gates=O.gates(cache))


@functools.lru_cache(maxsize=None)
def case_data(c):
    inp = make_inputs(c)
    return inp, reference(c, inp)


# ------------------------------------------------------------------------------------------ step-level feeds
STEP_LENS = (1, 50, 25, 33, 12)          # real steps of the five histories of the step tests (T = 50)


def edge_feed(T, G, Vi, Vc, lens, seed=0, Vu=8):
    """A training feed in SequentialIterator's layout without the iterator: ``len(lens)`` histories of the given real
    lengths, LEFT aligned and padded with id 0, each repeated for its G rows; row 0 of a group is the positive, the others
    are negatives that differ from it."""
    rng = np.random.RandomState(seed)
    n = len(lens)
    ih, ch = np.zeros((n, T), dtype=np.int32), np.zeros((n, T), dtype=np.int32)
    mask = np.zeros((n, T), dtype=np.float32)
    for i, ln in enumerate(lens):
        ih[i, :ln], ch[i, :ln], mask[i, :ln] = rng.randint(1, Vi, ln), rng.randint(1, Vc, ln), 1.0
    items, cates = np.zeros((n, G), dtype=np.int32), rng.randint(1, Vc, (n, G)).astype(np.int32)
    items[:, 0] = rng.randint(1, Vi, n)
    neg = rng.randint(1, Vi - 1, (n, G - 1))
    items[:, 1:] = neg + (neg >= items[:, :1])
    labels = np.zeros((n, G), dtype=np.float32)
    labels[:, 0] = 1.0
    rep = lambda a: np.repeat(a, G, axis=0)
    z = np.zeros((n * G, T), dtype=np.float32)
    return dict(labels=labels.reshape(n * G, 1), users=rep(rng.randint(1, Vu, n).astype(np.int32)),
                items=items.reshape(n * G), cates=cates.reshape(n * G), item_history=rep(ih), item_cate_history=rep(ch),
                mask=rep(mask), time=np.zeros(n * G, dtype=np.float32), time_diff=z, time_from_first_action=z, time_to_now=z)
