"""Shapes, inputs and float64 reference of the kernel-level NCF tests (tests/test_ncf_kernels_gpu.py; checked on the CPU
by tests/test_ncf_cpu.py)  --  TEST INFRASTRUCTURE ONLY.

The tile and limit figures come from the kernel's own host-side queries (csrc/ncf.hip), never from literals here.  Every
case carries the seed of its inputs: tests/test_ncf_cpu.py holds that with it NO tower unit is undecidable (float64
pre-activation within its propagated fp32 bound of zero), so no gradient comparison hangs on a ReLU gate."""
import functools
from collections import namedtuple

import numpy as np
import torch

import ncf_oracle as O
from clsr_amd.ops import query

Case = namedtuple("Case", "B G Du widths ids seed what")


def tile(G):
    return query("clsr_ncf_tile_lines", G)


def w4(widths):
    return tuple((list(widths) + [0, 0, 0, 0])[:4])


def lds_limit_widths(Du, w0):
    """Second-layer widths (w at the LDS limit, first w past it) of the family (Du, [w0, w]), by the kernel's own count."""
    budget, w = query("clsr_ncf_lds_budget_floats"), 4
    while query("clsr_ncf_lds_floats", Du, 2, w0, w + 4, 0, 0) <= budget:
        w += 4
    return w, w + 4


WMAX = query("clsr_ncf_max_width")
T5, T2 = tile(5), tile(2)
LDS_AT, LDS_PAST = lds_limit_widths(40, WMAX)
PARTS_MAX = query("clsr_ncf_parts", 1 << 30, 2)

# (B, G, Du, tower widths, id pattern, seed, what the case reaches)
CASES = [
    Case(5, 5, 8, (4,), "edge", 0, "one group only; one layer"),
    Case(T5 - 5, 5, 4, (36,), "edge", 0, "one group short of a line tile"),
    Case(T5, 5, 8, (40, 36), "edge", 0, "exactly one line tile; two layers"),
    Case(T5 + 5, 5, 44, (80, 40, 4), "edge", 0, "one group past a tile: two workgroups; three layers; Du = 44"),
    Case(3 * T2, 2, 40, (80, 40), "edge", 0, "ncf.yaml's shape, three workgroups, G = 2"),
    Case((PARTS_MAX + 2) * T2, 2, 4, (4, 4), "rand", 0, "more tiles than workgroups: two of them add a second tile to their row"),
    Case(10, 5, 8, (WMAX,), "edge", 0, "the maximum width"),
    Case(10, 5, 40, (WMAX, LDS_AT), "edge", 0, "at the LDS limit"),
    Case(20, 5, 8, (36, 4), "same", 0, "every line the same user and item"),
    Case(20, 5, 8, (36, 4), "distinct", 0, "all ids distinct"),
]
MULTI = CASES[5]
SCORE = [Case(T5 + 2, 1, 40, (80, 40), "edge", 0, "scoring (G = 1): a partial second tile"),
         Case(7, 1, 4, (4,), "edge", 0, "scoring: less than a tile")]
PAST_LDS = (40, (WMAX, LDS_PAST))


def case_id(c):
    return "B%d-G%d-Du%d-%s-%s" % (c.B, c.G, c.Du, "x".join(map(str, c.widths)), c.ids)


@functools.lru_cache(maxsize=None)
def make_inputs(c):
    """fp32 tables, parameter block pieces, ids and labels of a case (labels: the first line of every group)."""
    rng = np.random.RandomState(1000 + c.seed)
    Vu, Vi = (c.B + 3, c.B + 5) if c.ids == "distinct" else (11, 13)
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    tabs = [f32(rng.randn(V, c.Du) * 0.5) for V in (Vu, Vu, Vi, Vi)]          # user_gmf, user_mlp, item_gmf, item_mlp
    Ws, bs, K = [], [], 2 * c.Du
    for n in c.widths:
        lim = (6.0 / (K + n)) ** 0.5
        Ws.append(f32(rng.uniform(-lim, lim, size=(K, n))))
        bs.append(f32(rng.randn(n) * 0.1))
        K = n
    wout = f32(rng.uniform(-0.5, 0.5, size=(c.Du + K,)))
    if c.ids == "same":
        users, items = np.full(c.B, 3), np.full(c.B, 7)
    elif c.ids == "distinct":
        users, items = rng.permutation(Vu)[:c.B], rng.permutation(Vi)[:c.B]
    else:
        users, items = rng.randint(0, Vu, size=c.B), rng.randint(0, Vi, size=c.B)
        if c.ids == "edge":       # the first and the last row of both vocabularies
            users[0], users[-1], items[0], items[-1] = 0, Vu - 1, Vi - 1, 0
    labels = np.zeros(c.B, dtype=np.float32)
    labels[::c.G] = 1.0
    return dict(tabs=tabs, Ws=Ws, bs=bs, wout=wout, users=torch.from_numpy(users.astype(np.int32)),
                items=torch.from_numpy(items.astype(np.int32)), labels=torch.from_numpy(labels))


def block(inp):
    """The flat parameter block of csrc/ncf.hip: W_1 | b_1 | ... | w_out."""
    return torch.cat([t.reshape(-1) for W, b in zip(inp["Ws"], inp["bs"]) for t in (W, b)] + [inp["wout"].reshape(-1)])


@functools.lru_cache(maxsize=None)
def reference(c):
    """float64: forward with its propagated bounds, loss, dlogit, the un-merged slices, the dense gradient block and the
    slices' sums of squares -- computed once per case and shared by the tests that need it."""
    inp = make_inputs(c)
    u, i = inp["users"].long(), inp["items"].long()
    d = lambda t: t.double().clone().requires_grad_(True)
    Ws, bs, wout = [d(W) for W in inp["Ws"]], [d(b) for b in inp["bs"]], d(inp["wout"])
    sl = [t.double()[u if k < 2 else i].clone().requires_grad_(True) for k, t in enumerate(inp["tabs"])]
    t = O.tower(sl[0], sl[1], sl[2], sl[3], Ws, bs, wout, bound=True)
    scale = 1.0 / (c.B // c.G)
    lg = t["logit"].reshape(-1, c.G)
    lg.retain_grad()
    y = inp["labels"].double().reshape(-1, c.G)
    loss = -scale * (torch.log_softmax(lg, -1) * y).sum()
    dense = [p for W, b in zip(Ws, bs) for p in (W, b)] + [wout]
    cancel = None
    if c.ids == "same":
        # Identical lines: every dense gradient is sum_l dlogit[l] * J[l] with one J and sum_l dlogit[l] = 0 per group -- an
        # exact zero, so the relative tolerances have nothing to scale with.  What fp32 may leave is the error of the
        # terms: dlogit[l] = scale * (npos * exp(x - lse) - y) is off by at most scale * npos * sm * (2 e_logit + 8 * 2^-23
        # * (1 + |lse|)) (the logits' own bound through exp, exp and log to 2 ulp each), and the products and sums of the
        # backward chain add at most K * 2^-23 per term with K = B + 2 * (2 Du + sum of widths) roundings on any path.
        J = [torch.autograd.grad(t["logit"][l], dense, retain_graph=True) for l in range(c.B)]
        with torch.no_grad():
            sm, lse = torch.softmax(lg, -1), torch.logsumexp(lg, -1, keepdim=True)
            dl = scale * (y.sum(-1, keepdim=True) * sm - y)
            e_dl = scale * y.sum(-1, keepdim=True) * sm * (2 * t["e_logit"].reshape(-1, c.G).amax(-1, keepdim=True)
                                                          + 8 * O.EPS * (1 + lse.abs()))
            Kr = c.B + 2 * (2 * c.Du + sum(c.widths))
            wgt = (e_dl + Kr * O.EPS * dl.abs()).reshape(-1)
            cancel = torch.cat([sum(wgt[l] * J[l][k].abs() for l in range(c.B)).reshape(-1) for k in range(len(dense))])
    loss.backward()
    det = lambda x: x.detach()
    dblock = torch.cat([det(p.grad).reshape(-1) for W, b in zip(Ws, bs) for p in (W, b)] + [det(wout.grad).reshape(-1)])
    return dict(logit=det(t["logit"]), e_logit=det(t["e_logit"]), model_output=det(t["model_output"]),
                e_model_output=det(t["e_model_output"]), undecidable=O.undecidable({k: [det(x) for x in t[k]] for k in ("pre", "e_pre")}),
                units=sum(int(p.numel()) for p in t["pre"]), loss=float(loss.detach()), dlogit=det(lg.grad).reshape(-1),
                slices=[det(s.grad) for s in sl], dblock=dblock, cancel_bound=cancel, sumsq=[float((s.grad ** 2).sum()) for s in sl], scale=scale)
