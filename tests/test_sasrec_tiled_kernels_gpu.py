"""The tiled entry points of csrc/sasrec.hip alone (clsr_sasrec_tiled_fwd, clsr_sasrec_tiled_bwd), called through the C ABI
with raw parameter blocks, against the float64 reference of tests/sasrec_cases.py on the shapes of
tests/sasrec_tiled_cases.py.

The rule and the tolerances are those of tests/test_sasrec_kernels_gpu.py, unchanged at every T up to 256: s and every saved
tensor within FOUR TIMES the largest error of the float32 restatement (sasrec_oracle.fp32_bounds, measured per case on the
CPU, never a figure from the kernels), d hist, d pos and the reduced gradient block within that file's relative tolerances and
floor.  Exact: padding rows and unreached rows of pos are 0.0, scoring writes the bits of the training forward, two launches
are bit-identical, a refused shape or tile leaves the outputs alone.  Tiles of 1, 4 and 64 rows over the same T = 9 agree
within the forward bound."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import sasrec_cases as K  # noqa: E402
import sasrec_oracle as O  # noqa: E402
import sasrec_tiled_cases as TK  # noqa: E402
import test_sasrec_kernels_gpu as B  # noqa: E402
from clsr_amd import _lib, ops  # noqa: E402
from clsr_amd.ops import call, query  # noqa: E402

DEV, SENT = B.DEV, B.SENT


class _Run(B._Run):
    """Device buffers of one case under one tile (tests/test_sasrec_kernels_gpu.py: outputs start from NaN, a guard behind
    each).  The workspace is sized by the query and guarded too."""

    def __init__(self, tc, inp, stride=1):
        super(_Run, self).__init__(tc.case, inp, stride)
        self.tile = tc.tile
        c = tc.case
        self.shape = (c.Hn, c.T, c.Tmax, self.C, c.nb)
        self.parts = query("clsr_sasrec_tiled_parts", *self.shape)
        assert 1 <= self.parts <= min(c.Hn, query("clsr_sasrec_max_parts"))

    def _ws(self, training):
        n = query("clsr_sasrec_tiled_workspace_floats", *(self.shape + (self.tile, int(training))))
        assert n > 0
        return self._buf(n), n

    def forward(self, training=True, rep=1, ldo=None):
        c = self.c
        ldo = ldo or self.C
        rows = c.Hn * rep
        self.saved = self._buf(self.nsaved) if training else None
        self.out = torch.full((rows + 1, ldo), SENT, device=DEV)
        ws, nws = self._ws(training)
        call("clsr_sasrec_tiled_fwd", self.hist, self.lens, self.stride, c.Hn, c.T, c.Tmax, self.C, self.W, c.nb, c.nh,
             self.saved, self.out, ldo, rep, self.tile, ws)
        torch.cuda.synchronize()
        if training:
            assert bool((self.saved[self.nsaved:] == SENT).all()), "written past the saved tensors"
        assert bool((ws[nws:] == SENT).all()), "written past the workspace"
        assert bool((self.out[rows] == SENT).all()), "written past the last output row"
        return self.out[:rows].cpu()

    def backward(self):
        c = self.c
        ws, nws = self._ws(True)
        assert nws >= self.parts * self.P
        dhist, dblock = self._buf(self.n), self._buf(self.P)
        call("clsr_sasrec_tiled_bwd", self.ds, self.saved, self.lens, self.stride, c.Hn, c.T, c.Tmax, self.C, self.W, c.nb,
             c.nh, dhist, self.tile, ws)
        ops.multi("clsr_reduce_parts_multi", ops.RpDesc,
                  [ops.RpDesc.row(partial=ws, out=dblock, scale=1.0, nparts=self.parts, stride=self.P, n=self.P)])
        torch.cuda.synchronize()
        for t, n, name in ((ws, nws, "workspace"), (dhist, self.n, "d hist"), (dblock, self.P, "gradient block")):
            assert bool((t[n:] == SENT).all()), "written past the " + name
        return dhist[:self.n].cpu(), dblock[:self.P].cpu(), ws[:self.parts * self.P].cpu()


def _compare(tc, inp, ref, stride=1):
    c = tc.case
    run = _Run(tc, inp, stride)
    C, nb = run.C, c.nb
    print("float32 restatement, largest |err| per tensor: " + " ".join("%.3e" % e for e in ref["fp32_errors"]))
    s = run.forward()
    exp = O.checked_tensors(ref["s"], ref["cache"])
    B._within(s, exp[0], ref["bounds"][0], "s")
    saved = run.saved[:run.nsaved].cpu()
    blocks = saved[:nb * run.n].reshape(nb, c.Hn, c.T, C)
    for l in range(nb):
        B._within(blocks[l], exp[1 + l], ref["bounds"][1 + l], "saved input of block %d" % l)
    B._within(saved[nb * run.n:], exp[nb + 1], ref["bounds"][nb + 1], "saved x_L[len - 1]")
    valid = ref["cache"]["valid"]
    assert float(blocks[:, ~valid].abs().max() if not bool(valid.all()) else 0.0) == 0.0, "saved rows of padding"
    none = inp["lens"] == 0
    if bool(none.any()):
        assert float(s[none].abs().max()) == 0.0 and float(saved[nb * run.n:].reshape(c.Hn, C)[none].abs().max()) == 0.0
    dhist, dblock, _ = run.backward()
    assert bool(torch.isfinite(dhist).all()) and bool(torch.isfinite(dblock).all())
    floor = 4e-6 * float(ref["dblock"].abs().max())
    B._close(dhist, ref["dhist"], 2e-3, 2e-4 * float(ref["dhist"].abs().max()), "d hist")
    got, r = O.unpack(dblock, c.Tmax, C, nb), ref["grads"]
    B._close(got["pos"], r["pos"], 2e-3, 2e-4 * float(r["pos"].abs().max()) + floor, "d pos")
    for key in ("gf", "bef"):
        B._close(got[key], r[key], 2e-3, 2e-4 * float(r[key].abs().max()) + floor, "d " + key)
    for l in range(nb):
        for key in O.BLOCK_KEYS:
            rk = r["blocks"][l][key]
            B._close(got["blocks"][l][key], rk, 2e-3, 2e-4 * float(rk.abs().max()) + floor, "block %d d %s" % (l, key))
    # exactly zero: the padding's gradient, the rows of pos past the longest history
    dh = dhist.reshape(c.Hn, c.T, C)
    assert float(dh[~valid].abs().max() if not bool(valid.all()) else 0.0) == 0.0, "d hist of padding"
    longest = int(inp["lens"].max())
    if longest < c.Tmax:
        assert float(got["pos"][longest:].abs().max()) == 0.0, "d pos past the longest history"
    return run, s


@pytest.mark.parametrize("tc", TK.CASES, ids=TK.case_id)
def test_tiled_kernels_match_reference(tc):
    c = tc.case
    inp, ref = K.case_data(c)
    assert query("clsr_sasrec_tiled_supported", c.T, c.Tmax, c.Di + c.Dc, c.nb, c.nh, tc.tile) == 1
    _compare(tc, inp, ref)


def test_lengths_are_read_at_their_stride():
    tc = TK.MIXED
    inp, ref = K.case_data(tc.case)
    _compare(tc, inp, ref, stride=5)


@pytest.mark.parametrize("tc", [TK.MIXED, TK.FIRST_PAST], ids=TK.case_id)
def test_scoring_outputs(tc):
    """Scoring saves nothing, keeps the rows of x between blocks in the workspace and writes s straight into rows of a wider
    buffer, ``rep`` copies of each -- the bits of the training forward; the columns past C stay untouched."""
    inp, _ = K.case_data(tc.case)
    run = _Run(tc, inp)
    C = run.C
    s = run.forward()
    wide = run.forward(training=False, rep=3, ldo=2 * C)
    assert run.saved is None
    assert torch.equal(wide[:, :C], s.repeat_interleave(3, 0)) and bool((wide[:, C:] == SENT).all())


@pytest.mark.parametrize("tc", [TK.MULTI, TK.KUAISHOU], ids=TK.case_id)
def test_two_launches_are_bit_identical(tc):
    inp, _ = K.case_data(tc.case)
    run = _Run(tc, inp)
    s_a = run.forward()
    saved_a = run.saved.clone()
    s_b = run.forward()
    assert torch.equal(s_a, s_b) and torch.equal(saved_a[:run.nsaved], run.saved[:run.nsaved])
    a, b = run.backward(), run.backward()
    for x, y, name in zip(a, b, ("d hist", "gradient block", "partial sums")):
        assert torch.equal(x, y), name


def test_tiles_agree_with_each_other():
    """T = 9 under tiles of 4, 64 and 1 rows: s and the saved tensors of any two lie within the forward bound of each other
    (each lies within it of the reference: at most twice the bound apart; here they are held to ONE bound), the gradients
    within the gradient tolerances."""
    assert sorted(tc.tile for tc in TK.TILES_OF_NINE) == [1, 4, TK.TILE_MAX]
    inp, ref = K.case_data(TK.NINE)
    runs = []
    for tc in TK.TILES_OF_NINE:
        run = _Run(tc, inp)
        s = run.forward()
        saved = run.saved[:run.nsaved].cpu()
        dhist, dblock, _ = run.backward()
        runs.append((s, saved, dhist, dblock))
    nb, n = TK.NINE.nb, runs[0][2].numel()
    for other in runs[1:]:
        B._within(other[0], runs[0][0].double(), ref["bounds"][0], "s across tiles")
        for l in range(nb):
            B._within(other[1][l * n:(l + 1) * n], runs[0][1][l * n:(l + 1) * n].double(), ref["bounds"][1 + l], "saved")
        B._within(other[1][nb * n:], runs[0][1][nb * n:].double(), ref["bounds"][nb + 1], "x_L[len - 1]")
        B._close(other[2], runs[0][2], 2e-3, 2e-4 * float(runs[0][2].abs().max()), "d hist across tiles")
        B._close(other[3], runs[0][3], 2e-3, 2e-4 * float(runs[0][3].abs().max()), "gradient block across tiles")


@pytest.mark.parametrize("shape,what", TK.PAST, ids=[w for _, w in TK.PAST])
def test_past_a_limit_is_refused(shape, what):
    """The entry points refuse the shape or the tile and leave their outputs alone."""
    T, Tmax, C, nb, nh, tile = shape
    assert query("clsr_sasrec_tiled_supported", *shape) == 0
    assert query("clsr_sasrec_tiled_workspace_floats", 2, T, Tmax, C, nb, tile, 1) == 0
    n = 2 * T * C
    W = torch.zeros(Tmax * C + nb * (6 * C * C + 10 * C) + 2 * C + 16, device=DEV)
    x, lens = torch.zeros(n, device=DEV), torch.ones(2, dtype=torch.int32, device=DEV)
    out = torch.full((n,), SENT, device=DEV)
    saved = torch.full((nb * n + 2 * C,), SENT, device=DEV)
    ws = torch.full((2 * (W.numel() + 4 * n),), SENT, device=DEV)
    with pytest.raises(_lib.ClsrLibraryError):
        call("clsr_sasrec_tiled_fwd", x, lens, 1, 2, T, Tmax, C, W, nb, nh, saved, out, C, 1, tile, ws)
    with pytest.raises(_lib.ClsrLibraryError):
        call("clsr_sasrec_tiled_bwd", x, saved, lens, 1, 2, T, Tmax, C, W, nb, nh, out, tile, ws)
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((saved == SENT).all()) and bool((ws == SENT).all())
    assert float(W.abs().max()) == 0.0
