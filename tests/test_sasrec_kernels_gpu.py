"""The entry points of csrc/sasrec.hip alone (clsr_sasrec_fwd, clsr_sasrec_bwd), called through the C ABI with raw parameter
blocks, against the float64 reference of tests/sasrec_cases.py.

s and every saved tensor (each block's input, x_L[len - 1]) are held, element by element, to FOUR TIMES the largest error of
a float32 restatement of the oracle against the float64 one on the same inputs (tests/sasrec_oracle.py: ``fp32_bounds``),
measured per case and per tensor on the CPU over nine summation orders, each one term at a time and with torch's float32
operators: the rule DESIGN.md section 9d gives for a factor that has to move; never a figure from the kernels.  The test
prints the measured errors and where the kernels sit against the bound.  d hist, d pos and the reduced gradient block are
held to the relative tolerances and floor of tests/test_nextitnet_kernels_gpu.py, unchanged.  No element is left out:
tests/test_sasrec_cpu.py holds that no ReLU input of any case lies within 2^-16 of zero and that every layer-norm row of a
valid step has variance >= 1e-4.  Exact: padding rows and unreached rows of pos are 0.0, two launches are bit-identical, a
refused shape leaves the outputs alone."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import sasrec_cases as K  # noqa: E402
import sasrec_oracle as O  # noqa: E402
from clsr_amd import _lib, ops  # noqa: E402
from clsr_amd.ops import call, query  # noqa: E402

DEV = "cuda:0"
SENT = -7.5
GUARD = 8


def _within(got, exp, bound, name):
    err = (got.detach().double().cpu().reshape(-1) - exp.reshape(-1)).abs()
    print("%s: worst |err| / (4 x the float32 restatement's) = %.4f" % (name, float(err.max()) / bound))
    assert float(err.max()) <= bound, "%s: error %.3e exceeds four times the float32 restatement's, %.3e" % (
        name, float(err.max()), bound)


def _close(got, exp, rtol, atol, name):
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    exp = torch.as_tensor(exp).detach().double().cpu().reshape(-1)
    assert got.shape == exp.shape, (name, got.shape, exp.shape)
    err = (got - exp).abs()
    print("%s: max abs err %.3e, max |exp| %.3e" % (name, float(err.max()), float(exp.abs().max())))
    excess = float((err - (atol + rtol * exp.abs())).max())
    assert excess <= 0, "%s: max abs err %.3e, max |exp| %.3e" % (name, float(err.max()), float(exp.abs().max()))


class _Run(object):
    """Device buffers of one case.  Outputs start from NaN (an element nobody wrote shows), with a guard behind each.  The
    lengths sit ``stride`` entries apart, as the rows of a replicated feed do."""

    def __init__(self, c, inp, stride=1):
        self.c, self.C, self.stride = c, c.Di + c.Dc, stride
        self.hist = inp["hist"].contiguous().to(DEV)
        self.ds = inp["ds"].contiguous().to(DEV)
        lens = torch.full((c.Hn * stride,), 10 ** 6, dtype=torch.int32)
        lens[::stride] = inp["lens"].to(torch.int32)
        self.lens = lens.to(DEV)
        self.W = O.pack(inp["enc"]).float().to(DEV)
        self.P = self.W.numel()
        assert self.P == query("clsr_sasrec_param_floats", c.Tmax, self.C, c.nb)
        self.n = c.Hn * c.T * self.C
        self.nsaved = query("clsr_sasrec_saved_floats", c.Hn, c.T, self.C, c.nb)
        assert self.nsaved == c.nb * self.n + c.Hn * self.C

    def _buf(self, n):
        t = torch.full((n + GUARD,), float("nan"), device=DEV)
        t[n:] = SENT
        return t

    def forward(self, training=True, rep=1, ldo=None):
        c = self.c
        ldo = ldo or self.C
        rows = c.Hn * rep
        self.saved = self._buf(self.nsaved) if training else None
        self.out = torch.full((rows + 1, ldo), SENT, device=DEV)
        call("clsr_sasrec_fwd", self.hist, self.lens, self.stride, c.Hn, c.T, c.Tmax, self.C, self.W, c.nb, c.nh, self.saved,
             self.out, ldo, rep)
        torch.cuda.synchronize()
        if training:
            assert bool((self.saved[self.nsaved:] == SENT).all()), "written past the saved tensors"
        assert bool((self.out[rows] == SENT).all()), "written past the last output row"
        return self.out[:rows].cpu()

    def backward(self):
        c = self.c
        shape = (c.Hn, c.T, c.Tmax, self.C, c.nb)
        parts, nws = query("clsr_sasrec_parts", *shape), query("clsr_sasrec_workspace_floats", *shape)
        assert nws == parts * self.P
        ws, dhist, dblock = self._buf(nws), self._buf(self.n), self._buf(self.P)
        call("clsr_sasrec_bwd", self.ds, self.saved, self.lens, self.stride, c.Hn, c.T, c.Tmax, self.C, self.W, c.nb, c.nh,
             dhist, ws)
        ops.multi("clsr_reduce_parts_multi", ops.RpDesc,
                  [ops.RpDesc.row(partial=ws, out=dblock, scale=1.0, nparts=parts, stride=self.P, n=self.P)])
        torch.cuda.synchronize()
        for t, n, name in ((ws, nws, "workspace"), (dhist, self.n, "d hist"), (dblock, self.P, "gradient block")):
            assert bool((t[n:] == SENT).all()), "written past the " + name
        return dhist[:self.n].cpu(), dblock[:self.P].cpu(), ws[:nws].cpu()


def _compare(c, inp, ref, stride=1):
    run = _Run(c, inp, stride)
    C, nb = run.C, c.nb
    print("float32 restatement, largest |err| per tensor: " + " ".join("%.3e" % e for e in ref["fp32_errors"]))
    s = run.forward()
    exp = O.checked_tensors(ref["s"], ref["cache"])
    _within(s, exp[0], ref["bounds"][0], "s")
    saved = run.saved[:run.nsaved].cpu()
    blocks = saved[:nb * run.n].reshape(nb, c.Hn, c.T, C)
    for l in range(nb):
        _within(blocks[l], exp[1 + l], ref["bounds"][1 + l], "saved input of block %d" % l)
    _within(saved[nb * run.n:], exp[nb + 1], ref["bounds"][nb + 1], "saved x_L[len - 1]")
    valid = ref["cache"]["valid"]
    assert float(blocks[:, ~valid].abs().max() if not bool(valid.all()) else 0.0) == 0.0, "saved rows of padding"
    none = inp["lens"] == 0
    if bool(none.any()):
        assert float(s[none].abs().max()) == 0.0 and float(saved[nb * run.n:].reshape(c.Hn, C)[none].abs().max()) == 0.0
    dhist, dblock, _ = run.backward()
    assert bool(torch.isfinite(dhist).all()) and bool(torch.isfinite(dblock).all())
    floor = 4e-6 * float(ref["dblock"].abs().max())
    _close(dhist, ref["dhist"], 2e-3, 2e-4 * float(ref["dhist"].abs().max()), "d hist")
    got, r = O.unpack(dblock, c.Tmax, C, nb), ref["grads"]
    _close(got["pos"], r["pos"], 2e-3, 2e-4 * float(r["pos"].abs().max()) + floor, "d pos")
    for key in ("gf", "bef"):
        _close(got[key], r[key], 2e-3, 2e-4 * float(r[key].abs().max()) + floor, "d " + key)
    for l in range(nb):
        for key in O.BLOCK_KEYS:
            rk = r["blocks"][l][key]
            _close(got["blocks"][l][key], rk, 2e-3, 2e-4 * float(rk.abs().max()) + floor, "block %d d %s" % (l, key))
    # exactly zero: the padding's gradient, the rows of pos past the longest history
    dh = dhist.reshape(c.Hn, c.T, C)
    assert float(dh[~valid].abs().max() if not bool(valid.all()) else 0.0) == 0.0, "d hist of padding"
    longest = int(inp["lens"].max())
    if longest < c.Tmax:
        assert float(got["pos"][longest:].abs().max()) == 0.0, "d pos past the longest history"
    return run, dhist, dblock


@pytest.mark.parametrize("c", K.CASES, ids=K.case_id)
def test_kernels_match_reference(c):
    inp, ref = K.case_data(c)
    assert query("clsr_sasrec_supported", c.T, c.Tmax, c.Di + c.Dc, c.nb, c.nh) == 1
    _compare(c, inp, ref)


def test_lengths_are_read_at_their_stride():
    """A replicated feed holds a history's length in every G-th entry: the entries between are never read."""
    c = K.MIXED
    inp, ref = K.case_data(c)
    _compare(c, inp, ref, stride=5)


def test_scoring_outputs():
    """Scoring saves nothing and writes s straight into rows of a wider buffer, ``rep`` copies of each -- the bits of the
    training forward; the columns past C stay untouched."""
    c = K.MIXED
    inp, _ = K.case_data(c)
    run = _Run(c, inp)
    C = run.C
    s = run.forward()
    wide = run.forward(training=False, rep=3, ldo=2 * C)
    assert run.saved is None
    assert torch.equal(wide[:, :C], s.repeat_interleave(3, 0)) and bool((wide[:, C:] == SENT).all())


def test_two_launches_are_bit_identical():
    c = K.MULTI
    inp, _ = K.case_data(c)
    run = _Run(c, inp)
    s_a = run.forward()
    saved_a = run.saved.clone()
    s_b = run.forward()
    assert torch.equal(s_a, s_b) and torch.equal(saved_a[:run.nsaved], run.saved[:run.nsaved])
    a, b = run.backward(), run.backward()
    for x, y, name in zip(a, b, ("d hist", "gradient block", "partial sums")):
        assert torch.equal(x, y), name


@pytest.mark.parametrize("shape,what", K.PAST, ids=[w for _, w in K.PAST])
def test_one_step_past_a_limit_is_refused(shape, what):
    """The entry points refuse the shape and leave their outputs alone."""
    T, Tmax, C, nb, nh = shape
    assert query("clsr_sasrec_supported", T, Tmax, C, nb, nh) == 0
    n = 2 * T * C
    W = torch.zeros(max(Tmax, T) * C + max(nb, 1) * (6 * C * C + 10 * C) + 2 * C + 16, device=DEV)
    x, lens = torch.zeros(n, device=DEV), torch.ones(2, dtype=torch.int32, device=DEV)
    out = torch.full((n,), SENT, device=DEV)
    saved = torch.full((max(nb, 1) * n + 2 * C,), SENT, device=DEV)
    with pytest.raises(_lib.ClsrLibraryError):
        call("clsr_sasrec_fwd", x, lens, 1, 2, T, Tmax, C, W, nb, nh, saved, out, C, 1)
    with pytest.raises(_lib.ClsrLibraryError):
        call("clsr_sasrec_bwd", x, saved, lens, 1, 2, T, Tmax, C, W, nb, nh, out, W)
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((saved == SENT).all()) and float(W.abs().max()) == 0.0
