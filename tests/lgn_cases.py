"""Fixtures of the LGN propagation tests: graph, parameters and the float64 reference with its fp32 bounds, computed once
and shared by tests/test_lgn_cpu.py (which holds that no unit is undecidable) and tests/test_lgn_propagation_gpu.py.

  golden   the reference's own graph (tests/golden/lgn_graph.npz: 1184 rows, 9940 entries, degrees 1 .. 75), width 40
  skewed   a synthetic user-item graph in which one user row and one item row hold more than 2 L entries (L: the kernels'
           chunk, clsr_lgn_row_chunk()), so that the split path runs in both directions, width 8
"""
import collections
import functools
import os

import numpy as np
import torch

import lgn_oracle as O
from clsr_amd import lgn_graph
from clsr_amd.ops import query

HERE = os.path.dirname(os.path.abspath(__file__))
Csr = collections.namedtuple("Csr", "indptr indices values t_indptr t_indices t_values")
SEEDS = dict(golden=11, skewed=12)


def golden_graph():
    z = np.load(os.path.join(HERE, "golden", "lgn_graph.npz"))
    t = lgn_graph.csr_transpose(z["indptr"], z["indices"], z["values"], len(z["indptr"]) - 1)
    return Csr(z["indptr"], z["indices"], z["values"], *t), 40


def skewed_graph():
    L = query("clsr_lgn_row_chunk")
    Vu = Vi = 2 * L + 43
    rng = np.random.default_rng(3)
    u = np.concatenate([rng.integers(0, Vu, 900), np.full(2 * L + 5, 3), rng.choice(Vu, 2 * L + 7, replace=False)])
    i = np.concatenate([rng.integers(0, Vi, 900), rng.choice(Vi, 2 * L + 5, replace=False), np.full(2 * L + 7, 5)])
    a = lgn_graph.normalised_adjacency(Vu, Vi, u, i)
    g = Csr(*a, *lgn_graph.csr_transpose(*a, Vu + Vi))
    deg, deg_t = np.diff(g.indptr), np.diff(g.t_indptr)
    assert deg[3] > 2 * L and deg[Vu + 5] > 2 * L and deg_t[3] > 2 * L and deg_t[Vu + 5] > 2 * L
    return g, 8


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(graph, C, E0, Ws, bs, dF (fp32), A, fwd (forward(bound=True)), bwd (explicit backward with bounds))."""
    graph, C = dict(golden=golden_graph, skewed=skewed_graph)[name]()
    N = len(graph.indptr) - 1
    E0, Ws, bs, dF = O.fixture_params(N, C, SEEDS[name])
    A = O.dense_adjacency(graph.indptr, graph.indices, graph.values)
    d = lambda t: t.double()
    fwd = O.forward(A, d(E0), [d(W) for W in Ws], [d(b) for b in bs], bound=True)
    bwd = O.backward(A, fwd, [d(W) for W in Ws], d(dF), bs=[d(b) for b in bs], parts=query("clsr_lgn_parts", N))
    return dict(graph=graph, C=C, N=N, E0=E0, Ws=Ws, bs=bs, dF=dF, A=A, fwd=fwd, bwd=bwd)


# ------------------------------------------------------------------ the model's fixtures
def golden_model_graph():
    """The reference's graph of the golden data with its item2cate, as SeqNet(kind="lgn", graph=...) takes it."""
    z = np.load(os.path.join(HERE, "golden", "lgn_graph.npz"))
    g, _ = golden_graph()
    return lgn_graph.Graph(None, None, *g, z["item2cate"])


SKEWED_USERS = 300      # an item row past 2 L entries needs more users than the golden vocabulary's 190: the table is larger


def skewed_dims(dims):
    return dict(dims, Vu=SKEWED_USERS)


def skewed_model_graph(Vu, Vi, Vc):
    """A synthetic graph over the golden item / category vocabularies and SKEWED_USERS users (the feeds' ids all lie below
    that) in which user 3 and item 5 hold more than 2 L entries."""
    L = query("clsr_lgn_row_chunk")
    n = 2 * L + 9
    assert n <= min(Vu, Vi)
    rng = np.random.default_rng(8)
    u = np.concatenate([rng.integers(0, Vu, 1500), np.full(n, 3), rng.choice(Vu, n, replace=False) if n < Vu else np.arange(Vu)])
    i = np.concatenate([rng.integers(0, Vi, 1500), rng.choice(Vi, n, replace=False), np.full(len(u) - 1500 - n, 5)])
    a = lgn_graph.normalised_adjacency(Vu, Vi, u, i)
    i2c = rng.integers(0, Vc, Vi).astype(np.int32)
    i2c[0] = 0
    g = lgn_graph.Graph(Vu, Vi, *a, *lgn_graph.csr_transpose(*a, Vu + Vi), i2c)
    assert np.diff(g.indptr)[3] > 2 * L and np.diff(g.indptr)[Vu + 5] > 2 * L
    return g
