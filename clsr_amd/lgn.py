"""LGN's propagation (models/sequential/lgn.py: _create_lightgcn_embed_ui) on the HIP kernels of csrc/lgn.hip.

    E_0 = the node rows [N, C];   E_{k+1} = leaky_relu((A_hat E_k) W_k + b_k), slope 0.2;   F = mean of E_0 .. E_K

``Propagation`` owns the device image of the graph (CSR of A_hat and of its transpose, clsr_amd/lgn_graph.py), the split plan
of the rows longer than clsr_lgn_row_chunk() entries and the buffers of a pass.  ``forward`` is one launch a layer (plus
one over the chunks of the long rows, when there are any); ``backward`` one gate launch, one launch a layer over the
TRANSPOSED graph -- a gather like the forward, never a scatter -- and one fixed-order reduction of the workgroups' partial
rows of d W_k | d b_k.  No float atomics: two passes give the same bits.  The reference builds K = 2 layers (lgn.py:67);
the kernel that writes F takes the mean of exactly three tables, so other depths are refused.
"""
import numpy as np
import torch

from clsr_amd import ops
from clsr_amd.lgn_graph import split_plan
from clsr_amd.ops import call, query

N_LAYERS = 2


def check_limits(N, entries, C):
    """What the kernels take, by name: -> list of complaints (empty: supported)."""
    bad = []
    cmax = query("clsr_lgn_max_width")
    if C <= 0 or C % 4 or C > cmax:
        bad.append("item_embedding_dim + cate_embedding_dim must be a positive multiple of 4, at most %d, got %d" % (cmax, C))
    if not 0 < N < 2 ** 31:
        bad.append("user + item vocabulary (%d rows) must fit int32" % N)
    if not 0 <= entries < 2 ** 31:
        bad.append("adjacency entries (%d) must fit int32" % entries)
    if not bad and not query("clsr_lgn_supported", N, entries, C):
        bad.append("graph of %d rows, %d entries at width %d" % (N, entries, C))
    return bad


class _Csr(object):
    def __init__(self, indptr, indices, values, C, device):
        rows, off = split_plan(indptr, query("clsr_lgn_row_chunk"))
        i32 = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32), device=device)
        self.N, self.nlong, self.nchunks = len(indptr) - 1, len(rows), int(off[-1])
        self.indptr, self.indices = i32(indptr), i32(indices)
        # (values None: every entry 1 -- the category segments of clsr_lgn_rows_sum)
        self.values = None if values is None else torch.as_tensor(np.ascontiguousarray(values, dtype=np.float32), device=device)
        self.long_rows, self.long_off = (i32(rows), i32(off)) if self.nlong else (None, None)
        n = query("clsr_lgn_workspace_floats", self.nchunks, C)
        self.ws = torch.empty(n, dtype=torch.float32, device=device) if n else None

    def head(self):
        return (self.indptr, self.indices, self.values, self.long_rows, self.long_off, self.nlong, self.nchunks, self.N)


class Propagation(object):
    def __init__(self, graph, C, device="cuda:0"):
        """``graph``: anything with indptr / indices / values and t_indptr / t_indices / t_values (lgn_graph.Graph)."""
        N, entries = len(graph.indptr) - 1, len(graph.indices)
        bad = check_limits(N, entries, int(C))
        if bad:
            raise NotImplementedError("lgn HIP path does not support: " + "; ".join(bad))
        if len(graph.t_indptr) - 1 != N or len(graph.t_indices) != entries:
            raise ValueError("the transposed graph must hold the same %d rows and %d entries" % (N, entries))
        self.N, self.C, self.entries, self.device = N, int(C), entries, torch.device(device)
        self.fwd, self.bwd = _Csr(graph.indptr, graph.indices, graph.values, self.C, device), \
            _Csr(graph.t_indptr, graph.t_indices, graph.t_values, self.C, device)
        self.parts, self.part_floats = query("clsr_lgn_parts", N), query("clsr_lgn_part_floats", self.C)
        self._bufs, self._saved = {}, None

    def _buf(self, name, *shape):
        b = self._bufs.get(name)
        if b is None or tuple(b.shape) != shape:
            b = self._bufs[name] = torch.empty(shape, dtype=torch.float32, device=self.device)
        return b

    def _check(self, E0, Ws, bs):
        N, C = self.N, self.C
        if len(Ws) != N_LAYERS or len(bs) != N_LAYERS:
            raise ValueError("LGN propagates through %d layers, got %d" % (N_LAYERS, len(Ws)))
        for t, shape in [(E0, (N, C))] + [(W, (C, C)) for W in Ws] + [(b, (C,)) for b in bs]:
            if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("expected a contiguous fp32 tensor of shape %r, got %r %s" % (shape, tuple(t.shape), t.dtype))

    def forward(self, E0, Ws, bs, training=False):
        """-> F [N, C] (a buffer of this object: the next pass overwrites it).  ``training`` keeps S_k and E_k for ``backward``."""
        self._check(E0, Ws, bs)
        N, C, g = self.N, self.C, self.fwd
        E, F = [E0], self._buf("F", N, C)
        S = []
        for k in range(N_LAYERS):
            last = k == N_LAYERS - 1
            S.append(self._buf("S%d" % k, N, C) if training else None)
            E.append(self._buf("E%d" % (k + 1), N, C))
            call("clsr_lgn_layer_fwd", *g.head(), C, E[k], Ws[k], bs[k], S[k], E[k + 1], E0 if last else None,
                 F if last else None, g.ws)
        self._saved = (E, S, list(Ws)) if training else None
        return F

    def backward(self, dF, reduce=True):
        """``dF`` [N, C]: the gradient with respect to F of the last training ``forward``.  -> (d E_0 [N, C], [d W_k], [d b_k]);
        ``reduce=False``: -> (d E_0, [partial rows of layer k: ``parts`` x ``part_floats``, d W_k | d b_k]) for a caller that
        reduces them with its other partial sums."""
        if self._saved is None:
            raise ValueError("backward needs the state of a forward pass with training=True")
        E, S, Ws = self._saved
        N, C, g = self.N, self.C, self.bwd
        if tuple(dF.shape) != (N, C) or dF.dtype != torch.float32 or not dF.is_contiguous():
            raise ValueError("dF must be a contiguous fp32 tensor of shape %r" % ((N, C),))
        P = self._buf("P%d" % (N_LAYERS - 1), N, C)
        call("clsr_lgn_gate", dF, E[N_LAYERS], N * C, 1.0 / (N_LAYERS + 1), P)
        dW, rows = [None] * N_LAYERS, []
        for k in range(N_LAYERS - 1, -1, -1):
            out = self._buf("P%d" % (k - 1) if k else "dE0", N, C)
            part = self._buf("part%d" % k, self.parts, self.part_floats)
            call("clsr_lgn_layer_bwd", *g.head(), C, P, Ws[k], dF, S[k], E[k] if k else None, out, part, g.ws)
            if not reduce:
                dW[k], P = part, out
                continue
            dW[k] = self._buf("dWb%d" % k, self.part_floats)
            rows.append(ops.RpDesc.row(partial=part, out=dW[k], scale=1.0, nparts=self.parts, stride=self.part_floats,
                                       n=self.part_floats))
            P = out
        if not reduce:
            return P, dW
        ops.multi("clsr_reduce_parts_multi", ops.RpDesc, rows)
        return P, [d[:C * C].view(C, C) for d in dW], [d[C * C:] for d in dW]
