#!/usr/bin/env python
"""Time of LGN's propagation launches (csrc/lgn.hip through clsr_amd/lgn.py) on synthetic user-item graphs at the
vocabulary sizes scripts/ncf_step_time.py uses (CONFIGS["taobao"]: 36 915 users, 64 138 items), width 40 (lgn.yaml: 32 + 8).

Two graphs with the SAME entry count (``--degree`` edges a user on average; entries = 2 edges + one diagonal entry a row):

  even    every user holds ``--degree`` items dealt round robin: user rows of --degree + 1 entries, item rows within one of
          each other
  skewed  item popularity follows a Zipf law (clsr_amd.synthetic.zipf_sampler) and one hub user holds ``--hub`` items, so a
          few item rows and the hub row hold thousands of entries against a median of tens: the split path carries them

Per graph, medians of ``--repeats`` regions taken in turn (even, skewed, even, ...), device events around ``--iters``
launches each, on an otherwise idle device: the forward layer (training form: S is stored), the forward layer (scoring
form), the backward layer, the gate, and the whole pass (2 forward + gate + 2 backward + the partial-sum reduction).
Each propagation launch is set beside its gathered bytes (entries x C x 4: every entry fetches one row of C floats;
the 12 bytes of index, value and the row's own output are left out) and the rates the guide gives for rows served from
an XCD's L2 and from the Infinity Cache.  The node table is 16 MB here: past the 4 MiB L2, inside the Infinity Cache.

    python scripts/lgn_propagation_time.py [--degree 50] [--hub 20000] [--iters 30] [--repeats 7]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import time_kernel  # noqa: E402
from clsr_amd import lgn_graph, ops  # noqa: E402
from clsr_amd.lgn import Propagation  # noqa: E402
from clsr_amd.ops import call, query  # noqa: E402
from clsr_amd.synthetic import CONFIGS, zipf_sampler  # noqa: E402

L2_TBS, MALL_TBS = 16.8, 8.6        # indexed rows gathered from the XCD's L2 / the Infinity Cache, chip-wide lower bounds


def even_edges(Vu, Vi, degree):
    u = np.repeat(np.arange(Vu, dtype=np.int64), degree)
    return u, np.arange(Vu * degree, dtype=np.int64) % Vi


def skewed_edges(Vu, Vi, n_edges, hub, seed):
    """``n_edges`` distinct (user, item) pairs: a hub user with ``hub`` items, the rest Zipf over items, uniform over users."""
    rng = np.random.default_rng(seed)
    draw = zipf_sampler(rng, Vi)
    keys = np.arange(1, hub + 1, dtype=np.int64)                  # user 0 x items 1 .. hub
    while len(keys) < n_edges:
        m = int(1.2 * (n_edges - len(keys))) + 1024
        keys = np.unique(np.concatenate([keys, rng.integers(1, Vu, m) * Vi + draw(m)]))
    rest = keys[keys >= Vi]
    keep = rng.permutation(len(rest))[:n_edges - hub]
    keys = np.concatenate([keys[keys < Vi], rest[np.sort(keep)]])
    assert len(keys) == n_edges
    return keys // Vi, keys % Vi


def build(Vu, Vi, u, i):
    a = lgn_graph.normalised_adjacency(Vu, Vi, u, i)
    t = lgn_graph.csr_transpose(*a, Vu + Vi)
    return lgn_graph.Graph(Vu, Vi, *a, *t, None)


class Runner(object):
    def __init__(self, graph, C):
        self.p = p = Propagation(graph, C)
        g = torch.Generator().manual_seed(1)
        dev = lambda t: t.to(p.device)
        self.E0 = dev(torch.randn(p.N, C, generator=g) * 0.1)
        self.Ws = [dev(torch.randn(C, C, generator=g) * 0.02) for _ in range(2)]
        self.bs = [dev(torch.randn(C, generator=g) * 0.1) for _ in range(2)]
        self.dF = dev(torch.randn(p.N, C, generator=g))
        self.whole()
        self.S, self.E1, self.P, self.out = p._bufs["S0"], p._bufs["E1"], p._bufs["P1"], p._bufs["P0"]
        self.part = p._bufs["part0"]

    def whole(self):
        self.p.forward(self.E0, self.Ws, self.bs, training=True)
        self.p.backward(self.dF)

    def fwd_train(self):
        f = self.p.fwd
        call("clsr_lgn_layer_fwd", *f.head(), self.p.C, self.E0, self.Ws[0], self.bs[0], self.S, self.E1, None, None, f.ws)

    def fwd_score(self):
        f = self.p.fwd
        call("clsr_lgn_layer_fwd", *f.head(), self.p.C, self.E0, self.Ws[0], self.bs[0], None, self.E1, None, None, f.ws)

    def bwd(self):
        b = self.p.bwd
        call("clsr_lgn_layer_bwd", *b.head(), self.p.C, self.P, self.Ws[1], self.dF, self.S, self.E1, self.out, self.part, b.ws)

    def gate(self):
        call("clsr_lgn_gate", self.dF, self.E1, self.p.N * self.p.C, 1.0 / 3.0, self.P)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degree", type=int, default=50)
    ap.add_argument("--hub", type=int, default=20000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--width", type=int, default=40)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a launch time is a measurement on the device")
    cfg = CONFIGS["taobao"]
    Vu, Vi, C = cfg["Vu"], cfg["Vi"], a.width
    n_edges = Vu * a.degree
    graphs = dict(even=build(Vu, Vi, *even_edges(Vu, Vi, a.degree)),
                  skewed=build(Vu, Vi, *skewed_edges(Vu, Vi, n_edges, a.hub, 7)))
    out = dict(Vu=Vu, Vi=Vi, C=C, chunk=query("clsr_lgn_row_chunk"))
    runners = {}
    for name, g in graphs.items():
        deg = np.diff(g.indptr)
        entries = len(g.indices)
        assert entries == 2 * n_edges + Vu + Vi
        runners[name] = r = Runner(g, C)
        out[name] = dict(entries=entries, degree_median=int(np.median(deg)), degree_max=int(deg.max()),
                         long_rows=r.p.fwd.nlong, chunks=r.p.fwd.nchunks)
        print("%-7s %d rows, %d entries, degree median %d max %d, %d rows past the chunk of %d in %d chunks"
              % (name, r.p.N, entries, np.median(deg), deg.max(), r.p.fwd.nlong, out["chunk"], r.p.fwd.nchunks))
    what = ("fwd_train", "fwd_score", "bwd", "gate", "whole")
    times = {n: {w: [] for w in what} for n in runners}
    for _ in range(a.repeats):
        for n, r in runners.items():
            for w in what:
                times[n][w].append(1e6 * time_kernel(getattr(r, w), iters=a.iters))
    for n in runners:
        gathered = out[n]["entries"] * C * 4.0
        for w in what:
            t = times[n][w]
            med = statistics.median(t)
            out[n][w + "_us"] = dict(median=round(med, 1), min=round(min(t), 1), max=round(max(t), 1))
            extra = ""
            if w in ("fwd_train", "fwd_score", "bwd"):
                rate = gathered / med / 1e6
                out[n][w + "_gathered_TBs"] = round(rate, 3)
                extra = "   %.0f MB gathered: %.2f TB/s (L2 rows %.1f, Infinity Cache rows %.1f TB/s: %.0f / %.0f us)" % (
                    gathered / 1e6, rate, L2_TBS, MALL_TBS, gathered / L2_TBS / 1e6, gathered / MALL_TBS / 1e6)
            print("%-7s %-10s median %8.1f us (min %.1f, max %.1f over %d regions of %d)%s"
                  % (n, w, med, min(t), max(t), a.repeats, a.iters, extra))
    out["skewed_over_even"] = {w: round(out["skewed"][w + "_us"]["median"] / out["even"][w + "_us"]["median"], 3) for w in what}
    print("skewed / even:", out["skewed_over_even"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
