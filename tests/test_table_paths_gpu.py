"""Every launch path of the embedding-table Adam update stores the same bits (csrc/tableopt.h: one element update and one
set of loops for the three storage formats -- fp32, bf16 ``_h``, bf16 + 16-bit residual ``_hm``).

The same inputs go through the row-list entry, the single-table sweep and the multi-table sweep (as the only table of a
launch and as the second of two), twice in a row with fresh gradients so that the second update starts from moments that are
no longer zero-extended by luck; table, residual, moments, cleared gradient rows and cleared flags are compared with
``torch.equal``.  The norm slots are written by the host: no atomic order enters the comparison.  The ``_hm`` moments equal
the fp32 moments and merge(hi, lo) equals the fp32 table (both start from the same master).

Shapes: the three of tests/test_bf16_master_gpu.py (777 pieces and 5000 * 24 chunks are no multiples of the unrolled
strides: the clamped-address tails run); C = 6 takes the scalar sweep and the one-value row-list kernel; C = 32 with every
operand viewed at a 4-byte offset takes the scalar sweep at a width that otherwise takes the 16-byte one, and is compared
with the aligned run."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from clsr_amd import ops  # noqa: E402
from clsr_amd.ops import call  # noqa: E402
from test_bf16_master_gpu import BF, DEV, I16, SHAPES, _case, merge, split  # noqa: E402

SFX = {"f": "", "h": "_h", "hm": "_hm"}
B1, B2, EPS = 0.9, 0.999, 1e-8
# clip_norm, nsum, stride of the norm slots
VARIANTS = {"plain": (2.0, 1, 1), "clip": (0.01, 1, 1), "nsum2": (2.0, 2, 2)}
CASES = [(s, 0) for s in SHAPES] + [((37, 6, 5), 0), ((300, 32, 300), 4)]      # (V, C, rows), byte offset of the operands


def _inputs(shape, variant, seed=None):
    """_case plus a second gradient on the same rows, the host-written norm slots and the Adam state of both steps."""
    c = _case(*shape, seed=seed)
    clip, nsum, stride = VARIANTS[variant]
    g = torch.Generator().manual_seed(1000 + c["V"])
    grad2 = torch.zeros_like(c["grad"])
    grad2[c["ids"].long()] = torch.randn(c["nrows"], c["C"], generator=g).to(DEV) * 2e-2
    c["grads"] = [c["grad"], grad2]
    c["sumsqs"], c["states"] = [], []
    for k, gr in enumerate(c["grads"]):
        tot = float((gr.double() ** 2).sum())
        slots = [tot] if nsum == 1 else [0.3 * tot, 99.0, 0.7 * tot]       # (99: between the strided slots, not read)
        c["sumsqs"].append(torch.tensor(slots, dtype=torch.float64, device=DEV))
        t = 3 + k
        c["states"].append(torch.tensor([t, B1 ** t, B2 ** t, 1e-3 * (1 - B2 ** t) ** 0.5 / (1 - B1 ** t), 0.0],
                                        dtype=torch.float64, device=DEV))
    c["clip"], c["nsum"], c["stride"] = clip, nsum, stride
    return c


def _at(t, off):
    """A copy of ``t`` that starts ``off`` bytes behind an allocation."""
    k = off // t.element_size()
    buf = torch.empty(t.numel() + k, dtype=t.dtype, device=DEV)
    out = buf[k:].view(t.shape)
    out.copy_(t)
    return out


def _fresh(fmt, c, off=0):
    tab = {"f": (c["w"],), "h": (c["w"].to(BF),), "hm": split(c["w"])}[fmt]
    return dict(tab=tuple(_at(t, off) for t in tab), grad=_at(torch.zeros_like(c["grad"]), off), m=_at(c["m"], off),
                v=_at(c["v"], off), fl=_at(torch.zeros_like(c["flags"]), off))


def _desc(s, c, k):
    # clsr_table_desc: table, partner, grad, m, v, flags, sumsq_reg, disc_loss, sumsq_adam, V, C, nsum, sumsq_stride, ...
    return (s["tab"][0].data_ptr(), None, s["grad"].data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), s["fl"].data_ptr(),
            None, None, c["sumsqs"][k].data_ptr(), c["V"], c["C"], c["nsum"], c["stride"], 0.0, 0.0, 0)


def _run(fmt, path, lazy, c, off=0, first=None):
    """Two updates of one table through ``path``; ``first``: (inputs, state) of the table in front of it in a 'second' launch.
    Returns the state after each update."""
    s = _fresh(fmt, c, off)
    snaps = []
    for k in range(2):
        for st, ci in ((s, c),) + ((first[::-1],) if path == "second" else ()):
            st["grad"].copy_(ci["grads"][k])
            st["fl"].copy_(ci["flags"])
        tail = (c["sumsqs"][k], c["stride"], c["nsum"], c["clip"], c["states"][k], B1, B2, EPS)
        if path == "rows":
            call("clsr_table_adam_rows" + SFX[fmt], *s["tab"], s["grad"], s["m"], s["v"], s["fl"], c["ids"], c["count"],
                 c["nrows"], c["C"], *tail)
        elif path == "single":
            call("clsr_table_adam" + SFX[fmt], *s["tab"], s["grad"], s["m"], s["v"], s["fl"], c["V"], c["C"], *tail, lazy)
        else:
            tabs = [(first[1], first[0])] if path == "second" else []
            tabs.append((s, c))
            ops.multi("clsr_tables_adam_multi" + SFX[fmt], ops.TableDesc, [_desc(st, ci, k) for st, ci in tabs], c["clip"],
                      c["states"][k], B1, B2, EPS, lazy, lo=[st["tab"][1].data_ptr() for st, _ in tabs] if fmt == "hm" else None)
        torch.cuda.synchronize()
        snaps.append({key: tuple(t.clone() for t in val) if key == "tab" else val.clone() for key, val in s.items()})
    return snaps


def _bits(t):
    return t.view(I16) if t.dtype == BF else t


def _same(got, ref, what):
    for k, (a, b) in enumerate(zip(got, ref)):
        for x, y in zip(a["tab"], b["tab"]):
            assert torch.equal(_bits(x), _bits(y)), "%s, update %d: table" % (what, k + 1)
        assert torch.equal(a["m"], b["m"]) and torch.equal(a["v"], b["v"]), "%s, update %d: moments" % (what, k + 1)
        assert torch.equal(a["grad"], b["grad"]), "%s, update %d: cleared gradient rows" % (what, k + 1)
        assert torch.equal(a["fl"], b["fl"]) and int(a["fl"].sum()) == 0, "%s, update %d: cleared flags" % (what, k + 1)


_FP32 = {}


def _fp32_sweep(shape, variant, lazy):
    """The fp32 single-table sweep of a case, computed once (what the `_hm` runs have to equal)."""
    key = (shape, variant, lazy)
    if key not in _FP32:
        _FP32[key] = _run("f", "single", lazy, _inputs(shape, variant))
    return _FP32[key]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("fmt", ["f", "h", "hm"])
@pytest.mark.parametrize("shape,off", CASES)
def test_every_launch_path_stores_the_same_bits(shape, off, fmt, variant):
    V, C, nrows = shape
    c = _inputs(shape, variant)
    c0 = _inputs(SHAPES[0], variant, seed=100)      # the table in front of it in a two-table launch (its own norm slots)
    c0["clip"], c0["states"] = c["clip"], c["states"]

    def second(lazy, o):
        return _run(fmt, "second", lazy, c, o, first=(c0, _fresh(fmt, c0)))

    for lazy in (1, 0):
        runs = [("single", _run(fmt, "single", lazy, c)), ("multi", _run(fmt, "multi", lazy, c)), ("second", second(lazy, 0))]
        if lazy and not off and (C % 4 == 0 or fmt == "f"):
            runs.append(("rows", _run(fmt, "rows", lazy, c)))
        if off:     # the same width on the scalar forms
            runs += [("single+%d" % off, _run(fmt, "single", lazy, c, off)), ("multi+%d" % off, _run(fmt, "multi", lazy, c, off)),
                     ("second+%d" % off, second(lazy, off))]
        for name, r in runs[1:]:
            _same(r, runs[0][1], "%s %r lazy=%d %s: %s against the single-table sweep" % (fmt, shape, lazy, variant, name))
        last = runs[0][1][-1]
        touched = c["flags"].bool() if lazy else torch.ones(V, dtype=torch.bool, device=DEV)
        assert float(last["grad"][touched].abs().max()) == 0.0
        start = _fresh(fmt, c)
        for x, y in zip(last["tab"], start["tab"]):
            assert torch.equal(_bits(x)[~touched], _bits(y)[~touched]) and not torch.equal(_bits(x)[touched], _bits(y)[touched])
        assert torch.equal(last["m"][~touched], c["m"][~touched]) and torch.equal(last["v"][~touched], c["v"][~touched])
        if fmt == "hm":
            for k, (a, b) in enumerate(zip(runs[0][1], _fp32_sweep(shape, variant, lazy))):
                assert torch.equal(a["m"], b["m"]) and torch.equal(a["v"], b["v"]), "update %d: _hm moments == fp32 moments" % (k + 1)
                assert torch.equal(merge(*a["tab"]), b["tab"][0]), "update %d: merge(hi, lo) == the fp32 table" % (k + 1)
