"""The four kernels of csrc/caser.hip, called through the C ABI with raw parameter blocks, against the explicit float64
reference of tests/caser_oracle.py, at the shapes of tests/caser_cases.py: every chunk, tile, mask-word and slice boundary
of the kernels, both LDS limits, padded leading dimensions, prior content of d hist, gates at the edge.

The inputs sit on a dyadic grid on which any fp32 summation order is exact (caser_cases.py), so the forward is compared
bit for bit: pooled values, first maxima, tie counts, and the mask bits from the first maximum up to T - h (bits below it
are documented stale; words past T - h are never written).  The backward is held, element by element, to the running-sum
bound N * 2^-23 * S: S is the sum of the absolute addends of the element (the reference evaluated on |g|, |W|, |X| with the
same masks), N the number of addends of its longest chain (caser_oracle.chain_lengths).  The bound is derived, not measured;
a dropped or misplaced addend costs about S / N, far outside it while N^2 << 2^23.  tests/test_caser_cpu.py shows that the
comparator rejects a reference with one tied position's share removed and one with a window shifted by one."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import caser_cases as K  # noqa: E402
import caser_oracle as O  # noqa: E402
from clsr_amd._lib import ClsrLibraryError  # noqa: E402
from clsr_amd.ops import call, query  # noqa: E402

SENT = -7.5          # output padding and guard elements: must survive
GUARD = 8
KEYS = ("item", "cate")


def _shape(c):
    return (c.Hn, c.T, c.Di, c.Dc, c.L, c.n_v, c.n_h)


class _Run(object):
    """Device buffers of one case.  Padded leading dimensions: input padding holds NaN, output padding a sentinel."""

    def __init__(self, c, inp, padded):
        self.c, self.inp = c, inp
        D, self.PW = c.Di + c.Dc, c.n_v + c.L * c.n_h
        PW2 = 2 * self.PW
        self.ldh, self.ldp, self.ldd = (D + 4, PW2 + 4, PW2 + 8) if padded else (D, PW2, PW2)
        self.TS = 1 + (c.T + 31) // 32
        hist = torch.full((c.Hn * c.T, self.ldh), float("nan"))
        hist[:, :c.Di] = inp["X"]["item"].reshape(-1, c.Di).float()
        hist[:, c.Di:D] = inp["X"]["cate"].reshape(-1, c.Dc).float()
        self.hist = hist.cuda()
        self.W = {k: O.pack_block(inp["blk"][k]).float().cuda() for k in KEYS}
        self.S = {k: self.W[k].numel() for k in KEYS}
        assert self.S["item"] == query("clsr_caser_param_floats", c.T, c.Di, c.L, c.n_v, c.n_h)
        assert self.S["cate"] == query("clsr_caser_param_floats", c.T, c.Dc, c.L, c.n_v, c.n_h)
        self.pooled = torch.full((c.Hn + 1, self.ldp), SENT).cuda()          # (one guard row)
        pools = c.Hn * c.L * c.n_h
        self.argmax = {k: torch.full((pools + GUARD,), -77, dtype=torch.int32).cuda() for k in KEYS}
        # every bit set: nothing may depend on the tie record being cleared beforehand
        self.ties = {k: torch.full((pools * self.TS + GUARD,), -1, dtype=torch.int32).cuda() for k in KEYS}

    def forward(self):
        c = self.c
        call("clsr_caser_hconv_fwd", self.hist, self.ldh, c.Hn, c.T, c.Di, c.Dc, self.W["item"], self.W["cate"], c.L,
             c.n_v, c.n_h, self.pooled, self.ldp, self.argmax["item"], self.argmax["cate"], self.ties["item"],
             self.ties["cate"])
        torch.cuda.synchronize()

    def backward(self, dpool=None):
        """-> (d hist buffer, its initial content, d Wi, d Wc) on the host.  d hist starts from random content."""
        c, PW2 = self.c, 2 * self.PW
        dp = torch.full((c.Hn, self.ldd), float("nan"))
        dp[:, :PW2] = self.inp["dpool"] if dpool is None else dpool
        gen = torch.Generator().manual_seed(77)
        before = torch.randn(c.Hn * c.T + 3, self.ldh, generator=gen)        # (three guard rows)
        before[:c.Hn * c.T, :c.Di + c.Dc] = self.inp["prior"].reshape(-1, c.Di + c.Dc)
        dhist = before.cuda()
        dW = {k: torch.full((self.S[k] + GUARD,), SENT).cuda() for k in KEYS}
        nws = query("clsr_caser_hconv_bwd_workspace_floats", *_shape(c))
        ws = torch.full((nws + GUARD,), float("nan"))
        ws[nws:] = SENT
        ws = ws.cuda()
        pooled = self.pooled.clone()
        pooled[:c.Hn, PW2:] = float("nan")       # (an input now: its padding must not be read)
        call("clsr_caser_hconv_bwd", dp.cuda(), self.ldd, pooled, self.ldp, self.argmax["item"], self.argmax["cate"],
             self.ties["item"], self.ties["cate"], self.hist, self.ldh, c.Hn, c.T, c.Di, c.Dc, self.W["item"],
             self.W["cate"], c.L, c.n_v, c.n_h, dhist, dW["item"], dW["cate"], ws)
        torch.cuda.synchronize()
        assert torch.equal(ws[nws:].cpu(), torch.full((GUARD,), SENT)), "written past the workspace"
        return dhist.cpu(), before, dW["item"].cpu(), dW["cate"].cpu()


def _check_forward(run, ref):
    c, PW = run.c, run.PW
    pooled = run.pooled.cpu()
    assert torch.equal(pooled[:c.Hn, 2 * PW:], torch.full((c.Hn, run.ldp - 2 * PW), SENT)), "pooled: padding written"
    assert torch.equal(pooled[c.Hn], torch.full((run.ldp,), SENT)), "pooled: written past the last history"
    pools = c.Hn * c.L * c.n_h
    shifts = torch.arange(32, dtype=torch.int64)
    for i, key in enumerate(KEYS):
        m = ref["masks"][key]
        assert torch.equal(pooled[:c.Hn, i * PW:(i + 1) * PW], ref["pooled"][key].float()), key + ": pooled values"
        am = run.argmax[key].cpu()
        assert torch.equal(am[pools:], torch.full((GUARD,), -77, dtype=torch.int32)), key + ": argmax guard"
        assert torch.equal(am[:pools].reshape(c.Hn, c.L, c.n_h).long(), torch.stack(m["first"], 1)), key + ": first maxima"
        ti = run.ties[key].cpu()
        assert torch.equal(ti[pools * run.TS:], torch.full((GUARD,), -1, dtype=torch.int32)), key + ": ties guard"
        ti = ti[:pools * run.TS].reshape(c.Hn, c.L, c.n_h, run.TS).long()
        assert torch.equal(ti[..., 0], torch.stack(m["n"], 1)), key + ": tie counts"
        bits = ((ti[..., 1:] & 0xFFFFFFFF).unsqueeze(-1) >> shifts) & 1        # [Hn, L, n_h, words, 32]
        bits = bits.reshape(c.Hn, c.L, c.n_h, -1).bool()
        for h0 in range(c.L):
            P = c.T - h0                     # positions 0 .. T - h
            M = m["M"][h0].transpose(1, 2)   # [Hn, n_h, P]
            stale = torch.arange(P).view(1, 1, P) < m["first"][h0].unsqueeze(-1)
            same = (bits[:, h0, :, :P] == M) | stale
            assert bool(same.all()), "%s width %d: %d mask bits at or after the first maximum differ" % (
                key, h0 + 1, int((~same).sum()))


def _check_backward(run, ref, got, parts):
    c, D = run.c, run.c.Di + run.c.Dc
    dhist, before, dWi, dWc = got
    rows = c.Hn * c.T
    # outside the two tables' columns and past the last history: bit-unchanged
    assert torch.equal(dhist[:rows, D:], before[:rows, D:]), "d hist: padding columns changed"
    assert torch.equal(dhist[rows:], before[rows:]), "d hist: rows past the last history changed"
    N = O.chain_lengths(c.Hn, c.T, c.L, c.n_v, c.n_h, parts)

    def hold(name, g, r, S, n):
        ex, at = O.bar_excess(g, r, S, n)
        bar = n * O.EPS32 * S.double()
        ratio = float(((g.double() - r.double()).abs()[bar > 0] / bar[bar > 0]).max()) if bool((bar > 0).any()) else 0.0
        print("%s: worst |err| / (N eps S) = %.4f  (N = %d)" % (name, ratio, n))
        assert ex <= 0, "%s: element %d is %.3e outside N * 2^-23 * S (N = %d)" % (name, at, ex, n)

    for key, c0, Dx, dW in (("item", 0, c.Di, dWi), ("cate", c.Di, c.Dc, dWc)):
        prior = before[:rows, c0:c0 + Dx].reshape(c.Hn, c.T, Dx).double()
        hold("d hist " + key, dhist[:rows, c0:c0 + Dx].reshape(c.Hn, c.T, Dx), prior + ref["dX"][key],
             prior.abs() + ref["SX"][key], N["dhist"])
        assert torch.equal(dW[run.S[key]:], torch.full((GUARD,), SENT)), key + ": written past the gradient block"
        g = O.unpack_block(dW[:run.S[key]], c.T, Dx, c.L, c.n_v, c.n_h)
        r, S = ref["dblk"][key], ref["Sblk"][key]
        hold("d Wv " + key, g["Wv"], r["Wv"], S["Wv"], N["Wv"])
        hold("d bv " + key, g["bv"], r["bv"], S["bv"], N["bv"])
        for h0 in range(c.L):
            hold("d Wh_%d %s" % (h0 + 1, key), g["Wh"][h0], r["Wh"][h0], S["Wh"][h0], N["Wh"][h0])
            hold("d bh_%d %s" % (h0 + 1, key), g["bh"][h0], r["bh"][h0], S["bh"][h0], N["bh"][h0])


def _compare(c, inp, ref, padded):
    ok, found = K.conditions_hold(c, ref["masks"])
    assert ok, found
    parts = query("clsr_caser_hconv_bwd_parts", *_shape(c))
    assert query("clsr_caser_supported", *_shape(c)[1:]) == 1 and parts >= 1
    run = _Run(c, inp, padded)
    run.forward()
    _check_forward(run, ref)
    got = run.backward()
    _check_backward(run, ref, got, parts)
    return run, got


def _cases():
    out = []
    for c in K.CASES:
        out.append(pytest.param(c, False, id=K.case_id(c)))
        if c in (K.SLICES_17, K.CHUNK_56):
            out.append(pytest.param(c, True, id=K.case_id(c) + "-padded"))
    return out


@pytest.mark.parametrize("c,padded", _cases())
def test_kernels_match_explicit_reference(c, padded):
    inp, ref = K.case_data(c)
    _compare(c, inp, ref, padded)


def test_slice_counts():
    """The cases that are about the slices of the weight gradients reach them: a change of a constant in caser.hip fails
    here instead of leaving a case blind."""
    assert query("clsr_caser_hconv_bwd_parts", *_shape(K.SLICES_17)) == 16       # slices of 2: nine used, seven empty
    assert query("clsr_caser_hconv_bwd_parts", *_shape(K.SLICES_37)) == 16       # slices of 3: the thirteenth holds one
    assert query("clsr_caser_hconv_bwd_parts", *_shape(K.WS_CAPPED)) == 3        # slices of 2: the third is empty
    one = K.CASES[3]
    assert query("clsr_caser_hconv_bwd_parts", *_shape(one)) == 1
    assert query("clsr_caser_hconv_bwd_workspace_floats", *_shape(one)) == 4


def test_gates_at_the_edge():
    """A pooled maximum of exactly 0 closes the gate (pooled > 0), a filter negative everywhere takes the closed-pool path:
    both contribute nothing anywhere -- the backward does not change by a bit when d pooled of the closed gates does."""
    c = K.GATES
    inp = K.make_gate_inputs()
    ref = K.reference(inp)
    PW = c.n_v + c.L * c.n_h
    cols0 = [0] + [c.n_v + h0 * c.n_h for h0 in range(c.L)]        # filter 0 of the vertical path and of every width
    for key in KEYS:
        m, p = ref["masks"][key], ref["pooled"][key]
        assert not bool(m["gate_v"][0, 0]) and not bool(m["gate_v"][:, 1].any())
        for h0 in range(c.L):
            assert not bool(m["gate"][h0][0, 0]) and not bool(m["gate"][h0][:, 1].any())
        assert all(float(p[0, col]) == 0.0 and float(p[:, col + 1].max()) == 0.0 for col in cols0)
    run, got = _compare(c, inp, ref, False)
    dpool = inp["dpool"].clone()
    for i in range(2):
        for col in cols0:
            dpool[0, i * PW + col] = 1e6
            dpool[:, i * PW + col + 1] = -1e6
    again = run.backward(dpool)
    for a, b, name in zip(got, again, ("d hist", "d hist before", "d Wi", "d Wc")):
        assert torch.equal(a, b), name + ": a closed gate contributed"
    for key, dW in (("item", got[2]), ("cate", got[3])):
        Dx = c.Di if key == "item" else c.Dc
        g = O.unpack_block(dW[:run.S[key]], c.T, Dx, c.L, c.n_v, c.n_h)
        assert float(g["Wv"][:, :, 1].abs().max()) == 0.0 and float(g["bv"][1]) == 0.0
        for h0 in range(c.L):
            assert float(g["Wh"][h0][:, :, 1].abs().max()) == 0.0 and float(g["bh"][h0][1]) == 0.0


def test_backward_twice_is_bit_identical():
    c = K.SLICES_17
    inp, _ = K.case_data(c)
    run = _Run(c, inp, False)
    run.forward()
    a, b = run.backward(), run.backward()
    for x, y, name in zip(a, b, ("d hist", "d hist before", "d Wi", "d Wc")):
        assert torch.equal(x, y), name


def test_lds_limits():
    """Each side of both LDS limits; the forward refuses the shape past its limit and leaves its outputs alone."""
    assert query("clsr_caser_supported", 64, 4, 252, 58, 4, 4) == 1          # 65 rows of 252 floats: 65 520 B
    assert query("clsr_caser_supported", 64, 4, 252, 59, 4, 4) == 0
    assert query("clsr_caser_supported", 64, 252, 4, 59, 4, 4) == 0
    assert query("clsr_caser_supported", 8, 4, 4, 5, 1024, 1024) == 1        # 1024 + 3 * 5 * 1024 = 16 384 words
    assert query("clsr_caser_supported", 8, 4, 4, 6, 1024, 1024) == 0
    assert query("clsr_caser_hconv_bwd_parts", 2, 64, 4, 252, 59, 4, 4) == 0
    c = K.Case(2, 64, 4, 252, 59, 4, 4, 0, "one overlap row past the forward's LDS limit")
    run = _Run(c, K.make_inputs(c), False)
    with pytest.raises(ClsrLibraryError):
        run.forward()
    torch.cuda.synchronize()
    assert bool((run.pooled == SENT).all())
    for key in KEYS:
        assert bool((run.argmax[key] == -77).all()) and bool((run.ties[key] == -1).all())
