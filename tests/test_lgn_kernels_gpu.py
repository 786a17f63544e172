"""The LGN entry points alone (csrc/lgn.hip) against a float64 reference on synthetic CSR matrices.

With L = clsr_lgn_row_chunk(): rows of 0, 1, L - 1, L, L + 1 and 2 L + 3 entries, a long row first and a long row last
(the SAME entries: their sums must agree to the bit wherever the rows sit), a row count that is no multiple of a tile, widths
4, 40 and 128.  Tolerance -- no measured number: an output that is a sum of products reached through n additions is held to

    SLACK * gamma_n * sum |terms|,    gamma_n = n u / (1 - n u),  u = 2^-24,  SLACK = 2

(n counts every addition between the inputs and that output: the row's entries, the dense layer's C columns and bias, the
three terms of F; the float64 sum of |terms| is formed from the absolute values of the same inputs).  The leaky ReLU is
1-Lipschitz, so the bound of a pre-activation holds for the activation whichever side of zero either value lies on."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from clsr_amd import _lib, ops  # noqa: E402
from clsr_amd.lgn_graph import csr_transpose, split_plan  # noqa: E402
from clsr_amd.ops import call, query  # noqa: E402

DEV = "cuda:0"
U = 2.0 ** -24
SLACK = 2.0
WIDTHS = (4, 40, 128)


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


@functools.lru_cache(maxsize=None)
def matrix():
    """A square CSR matrix of 267 rows (16 tiles of 16 and one of 11) with every degree the split path distinguishes."""
    L = _chunk()
    N = 2 * L + 11
    rng = np.random.default_rng(20)
    long_cols = np.sort(rng.choice(N, 2 * L + 3, replace=False))
    deg = {0: None, 1: 0, 2: 1, 3: L - 1, 4: L, 5: L + 1, 6: 2 * L + 3, 40: L + 1, N - 1: None}
    indptr, indices = [0], []
    for r in range(N):
        if r in (0, N - 1):
            cols = long_cols
        elif r in deg:
            cols = np.sort(rng.choice(N, deg[r], replace=False))
        else:
            cols = np.sort(rng.choice(N, int(rng.integers(1, 12)), replace=False))
        indices.append(cols)
        indptr.append(indptr[-1] + len(cols))
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.concatenate(indices).astype(np.int32)
    values = rng.uniform(0.05, 1.0, len(indices)).astype(np.float32)
    # rows 0 and N - 1: the same entries
    values[indptr[N - 1]:indptr[N]] = values[indptr[0]:indptr[1]]
    return N, indptr, indices, values


def _chunk():
    return query("clsr_lgn_row_chunk")


def dense(N, indptr, indices, values, ncols=None):
    A = np.zeros((N, ncols or N), dtype=np.float64)
    rows = np.repeat(np.arange(N), np.diff(indptr))
    A[rows, indices] = values
    return A


class Csr(object):
    """Device arrays and the split plan of a CSR matrix, in the order the entry points take them."""

    def __init__(self, indptr, indices, values, width):
        rows, off = split_plan(indptr, _chunk())
        self.nlong, self.nchunks = len(rows), int(off[-1])
        i32 = lambda x: torch.as_tensor(np.asarray(x, dtype=np.int32), device=DEV)
        self.indptr, self.indices = i32(indptr), i32(indices)
        self.values = None if values is None else torch.as_tensor(values, device=DEV)
        self.long_rows, self.long_off = (i32(rows), i32(off)) if self.nlong else (None, None)
        n = query("clsr_lgn_workspace_floats", self.nchunks, width)
        self.ws = torch.full((n,), float("nan"), device=DEV) if n else None
        self.N = len(indptr) - 1

    def head(self):
        return (self.indptr, self.indices, self.values, self.long_rows, self.long_off, self.nlong, self.nchunks, self.N)


def _within(got, exp, bound, name):
    got = got.detach().double().cpu().numpy().reshape(-1)
    err = np.abs(got - np.asarray(exp).reshape(-1))
    bound = np.asarray(bound).reshape(-1)
    assert not np.isnan(got).any(), "%s: an element nobody wrote" % name
    print("%s: max err %.3e, bound there %.3e" % (name, err.max(), bound[err.argmax()]))
    assert (err <= bound).all(), "%s: error exceeds the summation bound by %.3e" % (name, (err - bound).max())


@functools.lru_cache(maxsize=None)
def layer_case(C):
    N, indptr, indices, values = matrix()
    rng = np.random.default_rng(100 + C)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    d = dict(E=f32(N, C), E0=f32(N, C), W=(f32(C, C) / np.sqrt(C)).astype(np.float32), b=f32(C) * np.float32(0.1),
             P=f32(N, C), dF=f32(N, C), S=f32(N, C), Eg=f32(N, C))
    d["Eg"][::7, ::3] = 0.0        # zeros among the gate's inputs: the derivative there is the slope
    return d


def _fwd(C, save_S, last, poison):
    N, indptr, indices, values = matrix()
    d, g = layer_case(C), Csr(indptr, indices, values, C)
    t = {k: torch.as_tensor(v, device=DEV) for k, v in d.items()}
    full = lambda: torch.full((N, C), poison, device=DEV)
    S, E1, F = (full() if save_S else None), full(), (full() if last else None)
    call("clsr_lgn_layer_fwd", *g.head(), C, t["E"], t["W"], t["b"], S, E1, t["E0"] if last else None, F, g.ws)
    torch.cuda.synchronize()
    return S, E1, F


@pytest.mark.parametrize("C", WIDTHS)
def test_forward_layer_matches_reference(C):
    N, indptr, indices, values = matrix()
    d = {k: v.astype(np.float64) for k, v in layer_case(C).items()}
    A, deg = dense(N, indptr, indices, values), np.diff(indptr)[:, None]
    S, E1, F = _fwd(C, True, True, float("nan"))
    S_ref, S_abs = A @ d["E"], np.abs(A) @ np.abs(d["E"])
    _within(S, S_ref, SLACK * gamma(deg + 1) * S_abs, "S")
    Z = S_ref @ d["W"] + d["b"]
    Z_abs = S_abs @ np.abs(d["W"]) + np.abs(d["b"])
    e_Z = SLACK * gamma(deg + C + 3) * Z_abs
    E1_ref = np.where(Z > 0, Z, 0.2 * Z)
    _within(E1, E1_ref, e_Z, "E_out")
    F_ref = (d["E0"] + d["E"] + E1_ref) / 3.0
    _within(F, F_ref, e_Z + SLACK * gamma(deg + C + 6) * (np.abs(d["E0"]) + np.abs(d["E"]) + Z_abs) / 3.0, "F")
    # the rows without entries: S = 0, E_out = lrelu(b)
    assert float(S[1].abs().max()) == 0.0
    # rows 0 and N - 1 hold the same entries: the same sums to the bit, in different tiles (one of them a partial tile)
    assert torch.equal(S[0], S[N - 1]) and torch.equal(E1[0], E1[N - 1])
    # without S, without F: the same E_out
    S2, E2, F2 = _fwd(C, False, False, 3.0)
    assert torch.equal(E1, E2)


@functools.lru_cache(maxsize=None)
def _transposed():
    N, indptr, indices, values = matrix()
    return csr_transpose(indptr, indices, values, N)


def _bwd(C, gate, poison):
    N = matrix()[0]
    t_indptr, t_indices, t_values = _transposed()
    d, g = layer_case(C), Csr(t_indptr, t_indices, t_values, C)
    t = {k: torch.as_tensor(v, device=DEV) for k, v in d.items()}
    parts, pf = query("clsr_lgn_parts", N), query("clsr_lgn_part_floats", C)
    out = torch.full((N, C), poison, device=DEV)
    part = torch.full((parts, pf), poison, device=DEV)
    call("clsr_lgn_layer_bwd", *g.head(), C, t["P"], t["W"], t["dF"], t["S"], t["Eg"] if gate else None, out, part, g.ws)
    red = torch.full((pf,), poison, device=DEV)
    ops.multi("clsr_reduce_parts_multi", ops.RpDesc,
              [ops.RpDesc.row(partial=part, out=red, scale=1.0, nparts=parts, stride=pf, n=pf)])
    torch.cuda.synchronize()
    return out, part, red


@pytest.mark.parametrize("C", WIDTHS)
def test_backward_layer_matches_reference(C):
    N, indptr, indices, values = matrix()
    d = {k: v.astype(np.float64) for k, v in layer_case(C).items()}
    t_indptr = _transposed()[0]
    assert np.diff(t_indptr).max() > 0
    At, deg = dense(N, indptr, indices, values).T, np.diff(t_indptr)[:, None]
    out, part, red = _bwd(C, True, float("nan"))
    T_ref, T_abs = At @ d["P"], np.abs(At) @ np.abs(d["P"])
    pre = d["dF"] / 3.0 + T_ref @ d["W"].T
    pre_abs = np.abs(d["dF"]) / 3.0 + T_abs @ np.abs(d["W"]).T
    gate = np.where(d["Eg"] > 0, 1.0, 0.2)
    _within(out, pre * gate, SLACK * gamma(deg + C + 4) * pre_abs, "d_out (gated)")
    out2, _, _ = _bwd(C, False, 5.0)
    _within(out2, pre, SLACK * gamma(deg + C + 3) * pre_abs, "d_out")
    parts = query("clsr_lgn_parts", N)
    dW, dW_abs = d["S"].T @ d["P"], np.abs(d["S"]).T @ np.abs(d["P"])
    _within(red[:C * C], dW, SLACK * gamma(N + parts) * dW_abs, "dW")
    _within(red[C * C:], d["P"].sum(0), SLACK * gamma(N + parts) * np.abs(d["P"]).sum(0), "db")
    # a workgroup's row of the partial buffer is the sum over ITS tiles: tile t belongs to workgroup t mod parts
    tr = query("clsr_lgn_tile_rows")
    rows = [r for t in range(1, (N + tr - 1) // tr, parts) for r in range(t * tr, min(N, (t + 1) * tr))]
    _within(part[1, :C * C], d["S"][rows].T @ d["P"][rows], SLACK * gamma(len(rows) + 1) * (np.abs(d["S"][rows]).T @ np.abs(d["P"][rows])),
            "dW, partial row 1")


@pytest.mark.parametrize("C", (40,))
def test_two_launches_are_bit_identical(C):
    a, b = _fwd(C, True, True, 7.0), _fwd(C, True, True, float("nan"))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    a, b = _bwd(C, True, 7.0), _bwd(C, True, -1.0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_unnamed_long_rows_are_still_summed():
    """Without a plan the long rows are summed whole by their owner: the same bound holds."""
    C = 40
    N, indptr, indices, values = matrix()
    d, g = layer_case(C), Csr(indptr, indices, values, C)
    g.long_rows = g.long_off = g.ws = None
    g.nlong = g.nchunks = 0
    S, E1 = torch.full((N, C), float("nan"), device=DEV), torch.full((N, C), float("nan"), device=DEV)
    call("clsr_lgn_layer_fwd", *g.head(), C, torch.as_tensor(d["E"], device=DEV), torch.as_tensor(d["W"], device=DEV),
         torch.as_tensor(d["b"], device=DEV), S, E1, None, None, None)
    torch.cuda.synchronize()
    A = dense(N, indptr, indices, values)
    _within(S, A @ d["E"].astype(np.float64), SLACK * gamma(np.diff(indptr)[:, None] + 1) * (np.abs(A) @ np.abs(d["E"]).astype(np.float64)), "S")


def test_unsupported_width_is_refused_and_writes_nothing():
    N, indptr, indices, values = matrix()
    lib, s = _lib.load(), ops.stream_ptr()
    assert query("clsr_lgn_supported", N, len(indices), 40) == 1
    for C in (6, 0, query("clsr_lgn_max_width") + 4):
        assert query("clsr_lgn_supported", N, len(indices), C) == 0 and query("clsr_lgn_lds_floats", C, 1) == 0
        W = max(C, 8)
        g = Csr(indptr, indices, values, W)
        E, Wt, b = (torch.ones(N, W, device=DEV), torch.ones(W, W, device=DEV), torch.ones(W, device=DEV))
        out = [torch.full((N, W), 9.0, device=DEV) for _ in range(3)]
        part = torch.full((query("clsr_lgn_parts", N), W * W + W), 9.0, device=DEV)
        p = lambda x: None if x is None else x.data_ptr()
        head = [p(x) if isinstance(x, torch.Tensor) or x is None else x for x in g.head()]
        rc = lib.clsr_lgn_layer_fwd(*head, C, p(E), p(Wt), p(b), p(out[0]), p(out[1]), p(E), p(out[2]), p(g.ws), s)
        assert rc == -1 and "lgn" in _lib.last_error()
        rc = lib.clsr_lgn_layer_bwd(*head, C, p(E), p(Wt), p(E), p(E), None, p(out[0]), p(part), p(g.ws), s)
        assert rc == -1
        torch.cuda.synchronize()
        assert all(float((o - 9.0).abs().max()) == 0.0 for o in out + [part])
        with pytest.raises(_lib.ClsrLibraryError):
            call("clsr_lgn_layer_fwd", *g.head(), C, E, Wt, b, out[0], out[1], E, out[2], g.ws)
    assert query("clsr_lgn_supported", 1 << 31, 10, 40) == 0 and query("clsr_lgn_supported", 10, 1 << 31, 40) == 0


def test_rows_sum_gate_score_and_logit_backward():
    """The small launches: the product alone over a strided slice with unit values (the category gradient's shape: a
    few segments, one of them long), the gate, scoring and the un-merged rows of the logit backward."""
    L = _chunk()
    rng = np.random.default_rng(5)
    Vu, Vi, Di, Dc = 7, 2 * L + 30, 32, 8
    C, Vc = Di + Dc, 5
    dE0 = rng.standard_normal((Vu + Vi, C)).astype(np.float32)
    cate = rng.integers(1, Vc, Vi)
    cate[:2 * L + 5] = 0                      # a segment past two chunks
    perm = np.argsort(cate, kind="stable").astype(np.int32)
    seg = np.zeros(Vc + 1, dtype=np.int64)
    np.cumsum(np.bincount(cate, minlength=Vc), out=seg[1:])
    g = Csr(seg, perm, None, Dc)
    assert g.nlong == 1
    X = torch.as_tensor(dE0, device=DEV)
    out = torch.full((Vc, Dc), float("nan"), device=DEV)
    call("clsr_lgn_rows_sum", *g.head(), Vi, X[Vu:, Di:], C, Dc, out, Dc, g.ws)
    torch.cuda.synchronize()
    ref, ref_abs = np.zeros((Vc, Dc)), np.zeros((Vc, Dc))
    np.add.at(ref, cate, dE0[Vu:, Di:].astype(np.float64))
    np.add.at(ref_abs, cate, np.abs(dE0[Vu:, Di:]).astype(np.float64))
    _within(out, ref, SLACK * gamma(np.diff(seg)[:, None] + 1) * ref_abs, "category sums")
    # gate
    E = rng.standard_normal((Vu + Vi, C)).astype(np.float32)
    E[::5] = 0.0
    P = torch.empty(Vu + Vi, C, device=DEV)
    call("clsr_lgn_gate", X, torch.as_tensor(E, device=DEV), X.numel(), 1.0 / 3.0, P)
    exp = dE0.astype(np.float64) / 3.0 * np.where(E > 0, 1.0, 0.2)
    _within(P, exp, SLACK * gamma(3) * np.abs(exp), "gate")
    # scoring and its backward; one user per group of 3 lines as well
    B = 50 * 3 + 0
    users, items = rng.integers(0, Vu, B).astype(np.int32), rng.integers(0, Vi, B).astype(np.int32)
    users = np.repeat(users[::3], 3)
    F = torch.as_tensor(E, device=DEV)
    tu, ti = torch.as_tensor(users, device=DEV), torch.as_tensor(items, device=DEV)
    logit = torch.full((B,), float("nan"), device=DEV)
    call("clsr_lgn_score", tu, 1, ti, F, Vu, Vi, C, B, logit)
    Ed = E.astype(np.float64)
    fu, fi = Ed[users], Ed[Vu + items]
    _within(logit, (fu * fi).sum(1), SLACK * gamma(C) * (np.abs(fu) * np.abs(fi)).sum(1), "logit")
    logit3 = torch.full((B,), float("nan"), device=DEV)
    call("clsr_lgn_score", tu[::3].contiguous(), 3, ti, F, Vu, Vi, C, B, logit3)
    assert torch.equal(logit, logit3)
    dl = rng.standard_normal(B).astype(np.float32)
    du, di = torch.full((B, C), float("nan"), device=DEV), torch.full((B, C), float("nan"), device=DEV)
    uid = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    call("clsr_lgn_logit_bwd", tu[::3].contiguous(), 3, ti, F, Vu, Vi, C, B, torch.as_tensor(dl, device=DEV), du, di, uid)
    torch.cuda.synchronize()
    assert np.array_equal(uid.cpu().numpy(), users)
    _within(du, dl[:, None] * fi, SLACK * gamma(1) * np.abs(dl[:, None] * fi), "d user rows")
    _within(di, dl[:, None] * fu, SLACK * gamma(1) * np.abs(dl[:, None] * fu), "d item rows")


def test_out_of_range_entries_and_ids_are_skipped_not_read():
    """Column entries outside the matrix contribute nothing; a user or item id outside its table scores 0 and gives zero
    rows in the logit backward -- the documented behaviour, and no read past a buffer."""
    C, N = 8, 40
    rng = np.random.default_rng(9)
    indptr = np.arange(0, 4 * N + 1, 4)
    indices = rng.integers(0, N, 4 * N).astype(np.int32)
    values = rng.uniform(0.1, 1.0, 4 * N).astype(np.float32)
    bad = indices.copy()
    bad[::5] = N + 7
    bad[2::11] = -3
    ok = (bad >= 0) & (bad < N)
    X = rng.standard_normal((N, C)).astype(np.float32)
    g = Csr(indptr, bad, values, C)
    out = torch.full((N, C), float("nan"), device=DEV)
    call("clsr_lgn_rows_sum", *g.head(), N, torch.as_tensor(X, device=DEV), C, C, out, C, None)
    A = np.zeros((N, N))
    np.add.at(A, (np.repeat(np.arange(N), 4)[ok], bad[ok]), values[ok].astype(np.float64))
    _within(out, A @ X.astype(np.float64), SLACK * gamma(5) * (np.abs(A) @ np.abs(X).astype(np.float64)), "rows with skipped entries")
    Vu, Vi = 10, 30
    users = np.array([0, 9, 10, -1, 3, 3], dtype=np.int32)
    items = np.array([0, 29, 5, 5, 30, -2], dtype=np.int32)
    F, tu, ti = torch.as_tensor(X, device=DEV), torch.as_tensor(users, device=DEV), torch.as_tensor(items, device=DEV)
    logit = torch.full((6,), float("nan"), device=DEV)
    call("clsr_lgn_score", tu, 1, ti, F, Vu, Vi, C, 6, logit)
    du, di = torch.full((6, C), float("nan"), device=DEV), torch.full((6, C), float("nan"), device=DEV)
    uid = torch.zeros(6, dtype=torch.int32, device=DEV)
    call("clsr_lgn_logit_bwd", tu, 1, ti, F, Vu, Vi, C, 6, torch.ones(6, device=DEV), du, di, uid)
    torch.cuda.synchronize()
    assert logit[2:].abs().max().item() == 0.0 and du[2:].abs().max().item() == 0.0 and di[2:].abs().max().item() == 0.0
    Xd = X.astype(np.float64)
    _within(logit[:2], (Xd[users[:2]] * Xd[Vu + items[:2]]).sum(1), SLACK * gamma(C) * (np.abs(Xd[users[:2]]) * np.abs(Xd[Vu + items[:2]])).sum(1), "logit")
    assert torch.equal(du[:2].cpu(), torch.as_tensor(X[Vu + items[:2]])) and torch.equal(di[:2].cpu(), torch.as_tensor(X[users[:2]]))


def test_regulariser_rows_and_gradient_norms():
    """clsr_lgn_reg_rows and clsr_lgn_grad_sumsq against float64, twice to the same bits."""
    rng = np.random.default_rng(10)
    V, C, l2 = 333, 40, 0.25
    F = rng.standard_normal((V, C)).astype(np.float32)
    dF0 = rng.standard_normal((V, C)).astype(np.float32)
    flags = (rng.random(V) < 0.4).astype(np.uint8)
    ws = torch.zeros(query("clsr_lgn_stats_workspace_doubles"), dtype=torch.float64, device=DEV)
    res = []
    for _ in range(2):
        dF = torch.as_tensor(dF0, device=DEV).clone()
        loss, ss = torch.full((1,), 2.0, dtype=torch.float64, device=DEV), torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
        call("clsr_lgn_reg_rows", torch.as_tensor(flags, device=DEV), torch.as_tensor(F, device=DEV), dF, V, C, l2, ws, loss, ss)
        n3 = torch.full((3,), -1.0, dtype=torch.float64, device=DEV)
        call("clsr_lgn_grad_sumsq", dF, 100, V, C, 32, ws, n3[0:], n3[1:], n3[2:])
        torch.cuda.synchronize()
        res.append((dF, loss, ss, n3))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    dF, loss, ss, n3 = res[0]
    Fd, m = F.astype(np.float64), flags.astype(bool)
    exp = dF0.astype(np.float64)
    exp[m] += l2 * Fd[m]
    _within(dF, exp, SLACK * gamma(2) * (np.abs(dF0) + l2 * np.abs(Fd)), "dF with the regulariser")
    assert abs(float(loss) - 2.0 - 0.5 * l2 * (Fd[m] ** 2).sum()) < 1e-9 and abs(float(ss) - l2 * l2 * (Fd[m] ** 2).sum()) < 1e-9
    got = dF.double().cpu().numpy()
    for q, e in enumerate(((got[:100] ** 2).sum(), (got[100:, :32] ** 2).sum(), (got[100:, 32:] ** 2).sum())):
        assert abs(float(n3[q]) - e) < 1e-9 * e
