"""The training / scoring step against the float64 oracles on both sides of every dispatch boundary: the committed
boundary cases of scripts/fuzz_step.py (boundary_cases(): tiny shapes, one width at a time on the last value a fused kernel
admits and on the first it refuses; tests/test_boundaries_cpu.py holds the list to that rule by the kernels' own queries and
admits every case on the float32 oracle alone).

Each case is the full comparison of fuzz_step.run_case, unchanged, at the bars of tests/test_fuzz_gpu.py: logits in scoring
and training, the five losses, every dense gradient, the gradient tables, the IndexedSlices clip norms, the (lazy-)Adam
updates, idle rows bit for bit, the moving statistics, with de-duplicated histories and without; a non-finite value on
either side is a failure.  precision="fp32" runs every case, "fp32x3" the CLSR cases at a boundary of a kernel with a
two-piece instance; the siblings' model API admits fp32 only.  The bf16 speed mode is not covered here: its rounding oracle
takes its own shapes (tests/test_bf16_gpu.py).

test_both_sides_launched reads, from the launches one more training step of a case RECORDS (ops.record_begin), which
entry point ran: for every two-sided branch (BRANCHES), per precision, the cases on the last admitted value launched the
fused entry and the cases on the first refused value the other side -- so a sweep cannot silently run one side only, and a
changed predicate cannot silently un-cover a kernel.  No predicate is evaluated here.  DESIGN.md section 6 has the table,
the ratios and the wall time."""
import collections
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import fuzz_step  # noqa: E402

CASES = fuzz_step.boundary_cases()
CHUNK = 8


def _chunks(cases):
    """Cases of one axis and model family, eight to a test."""
    groups = collections.OrderedDict()
    for c in cases:
        groups.setdefault((c.axis, "clsr" if c.kind == "clsr" else "siblings"), []).append(c)
    out = []
    for (axis, fam), cs in groups.items():
        for i in range(0, len(cs), CHUNK):
            out.append(pytest.param(cs[i:i + CHUNK], id="%s-%s-%d" % (fam, axis, i // CHUNK)))
    return out


def _guarded(c, fn, *args):
    """``fn(*args)``; a host error that leaves the device unusable ends the whole session: nothing more is started on a
    GPU that has faulted."""
    try:
        return fn(*args)
    except RuntimeError as exc:
        try:
            torch.cuda.synchronize()
        except Exception:
            pytest.exit("device fault at %s (%s): %s" % (c.id, c.desc, exc), returncode=70)
        raise


def _run(chunk, precision):
    fuzz_step.PRECISION = precision
    fuzz_step.STATS.clear()
    failures = []
    try:
        for c in chunk:
            problems = _guarded(c, fuzz_step.run_case, c)
            if problems:
                failures.append((c.id, c.desc, problems[:8]))
    finally:
        fuzz_step.PRECISION = "fp32"
    print("%s: %s" % (precision, " ".join(c.id for c in chunk)))
    fuzz_step.print_stats()
    fuzz_step.STATS.clear()
    assert not failures, failures


@pytest.mark.parametrize("chunk", _chunks(CASES))
def test_boundary_step(chunk):
    _run(chunk, "fp32")


@pytest.mark.parametrize("chunk", _chunks([c for c in CASES if c.x3]))
def test_boundary_step_fp32x3(chunk):
    """The two-piece split-bf16 products, held to the same bars as the fp32 products."""
    _run(chunk, "fp32x3")


# ---------------------------------------------------------------------------------------------- the path taken
def _launches(c, precision):
    """What ONE training step of the case launches (de-duplicated histories, the product default): entry name -> count,
    and (fused input projection?, products code) of every recurrence descriptor of the forward launch."""
    from clsr_amd import ops
    from clsr_amd.net import CLSRNet
    from clsr_amd.seqnet import SeqNet

    if c.kind == "clsr":
        orc, extra = fuzz_step.O, ()
        net = CLSRNet(c.hp, c.dims, device="cuda:0", seed=0, precision=precision)
    else:
        orc, extra = fuzz_step.SO, (c.kind,)
        net = SeqNet(c.hp, c.dims, kind=c.kind, device="cuda:0", seed=0)
    params32 = orc.init_params(c.dims, c.hp, *extra, seed=c.idx, scale_dense=8.0)
    sd = dict(params32)
    sd.update(orc.init_bn_state(params32))
    net.load_state_dict(sd, strict=True)
    f = net.upload(fuzz_step.make_feed(c), True)
    plan = ops.record_begin()
    try:
        net.train_step(f, apply=False)
    finally:
        ops.record_end()
    torch.cuda.synchronize()
    names = collections.Counter(getattr(fn, "__name__", "") for fn, _ in plan.ops)
    descs = [d for k in plan.keep for d in (k if isinstance(k, list) else [k]) if isinstance(d, (ops.GruDesc, ops.T4Desc))]
    rnn = [(bool(d.X), int(d.products)) for d in descs if not d.dPin]          # (dPin: a descriptor of the backward launch)
    return names, rnn


def _has(*entries):
    return lambda names, rnn: any(names[e] for e in entries)


def _lacks(*entries, **kw):
    need = kw.get("need", ())
    return lambda names, rnn: not any(names[e] for e in entries) and all(names[e] for e in need)


def _count(k, *entries):
    return lambda names, rnn: sum(names[e] for e in entries) == k


L0X = ("clsr_att_l0_bwd_x3", "clsr_att_l0_bwd_x6")
L1X = ("clsr_att_l1_bwd_x3", "clsr_att_l1_bwd_x6")
ENCB = ("clsr_enc_bwd_fused", "clsr_enc_bwd_fused_fold", "clsr_enc_bwd_fused_x3", "clsr_enc_bwd_fused_x6")
TILED = ("clsr_att_prod_bwd", "clsr_att_prod_bwd_ld")
ATT = ("clsr_att_out_fwd",)      # an attention block ran at all
BOTH = ("fp32", "fp32x3")
Branch = collections.namedtuple("Branch", "name precisions fused other inside outside")
# The branch table: branch (clsr_amd/net.py line of its predicate), the precisions it is two-sided in, what shows the fused
# entry / the other side in the recorded launches, and the cases that sit on the last admitted value (``inside``: they must
# show the fused entry) and on the first refused one (``outside``: they must show the other side), pairwise along one swept
# width.  The sides come from the limits the kernels document (csrc/*.hip, the ``*_supported`` functions); what is asserted
# is read from the launches alone.
BRANCHES = [
    Branch("att_hist_fwd_x3 (net.py:1422)", BOTH, _has("clsr_att_hist_fwd_x3"), _lacks("clsr_att_hist_fwd_x3", need=ATT),
           ["clsr-D64-gru", "clsr-A0_80", "dien-Q80", "dien-H64"], ["clsr-D68-gru", "clsr-A0_84", "dien-Q84", "dien-H68"]),
    Branch("att_hist_bwd_x3 (net.py:1733, 1754)", BOTH, _has("clsr_att_hist_bwd_x3"), _lacks("clsr_att_hist_bwd_x3", need=ATT),
           ["clsr-D48-gru", "clsr-A0_96", "clsr-A0_8", "dien-Q80"], ["clsr-D52-gru", "clsr-A0_100", "clsr-A0_4", "dien-Q84"]),
    Branch("att_l0_fwd (net.py:1485)", BOTH, _has("clsr_att_l0_fwd", "clsr_att_l0_fwd_x6"),
           _lacks("clsr_att_l0_fwd", "clsr_att_l0_fwd_x6", need=ATT),
           ["clsr-A0_80", "din-Q128"], ["clsr-A0_84", "din-Q132"]),
    # wide product terms outside "fp32" (K > 80) take the three-piece forward form
    Branch("att_l0_fwd_x6 for K > 80 (net.py:1722)", ("fp32x3",), _has("clsr_att_l0_fwd_x6"), _lacks("clsr_att_l0_fwd_x6", need=("clsr_att_l0_fwd",)),
           ["clsr-D84-gru"], ["clsr-D80-gru"]),
    # precision="fp32" runs layer 0 of the backward on fp32-input MFMAs (att_bwd_l0 = "fp32"): clsr_att_l0_bwd or the tiled chain
    Branch("att_l0_bwd (net.py:1611)", ("fp32",), _has("clsr_att_l0_bwd"), _lacks("clsr_att_l0_bwd", need=TILED[:1]),
           ["clsr-D80-gru", "clsr-A0_80", "din-Q80"], ["clsr-D84-gru", "clsr-A0_84", "din-Q84"]),
    Branch("att_l0_bwd_x3 (net.py:1592)", ("fp32x3",), _has(*L0X), _lacks(*L0X, need=ATT),
           ["clsr-D80-gru", "clsr-A0_80", "clsr-A0_8"], ["clsr-D84-gru", "clsr-A0_84", "clsr-A0_4"]),
    # rows per positive: the long-term attention runs ONE row per history whatever G is, so its launch stays; the short-term
    # attention's launch is the second one
    Branch("att_l0_fwd, G rows (net.py:1485)", BOTH, _count(2, "clsr_att_l0_fwd"), _count(1, "clsr_att_l0_fwd"),
           ["clsr-D24-G8", "clsr-golden-G8"], ["clsr-D24-G9", "clsr-golden-G9"]),
    Branch("att_l0_bwd, G rows (net.py:1611)", ("fp32",), _count(2, "clsr_att_l0_bwd"), _count(1, "clsr_att_l0_bwd"),
           ["clsr-D24-G8", "clsr-golden-G8"], ["clsr-D24-G9", "clsr-golden-G9"]),
    Branch("att_l0_bwd_x3, G rows (net.py:1592)", ("fp32x3",), _count(2, *L0X), _count(1, *L0X),
           ["clsr-D24-G8", "clsr-golden-G8"], ["clsr-D24-G9", "clsr-golden-G9"]),
    # two column halves: four launches for the two attentions, where one launch each serves up to 80 columns
    Branch("att_l0_bwd_x3 in two column halves (net.py:1698)", ("fp32x3",), lambda n, r: sum(n[e] for e in L0X) >= 3,
           lambda n, r: not any(n[e] for e in L0X) and any(n[e] for e in TILED), ["clsr-D88-gru", "clsr-D128-gru"], ["clsr-D84-gru"]),
    Branch("att_l1_fwd (net.py:1446)", BOTH, _has("clsr_att_l1_fwd"), _lacks("clsr_att_l1_fwd", need=ATT),
           ["clsr-A0_96", "clsr-A0_8", "clsr-A1_48"], ["clsr-A0_100", "clsr-A0_4", "clsr-A1_52"]),
    Branch("att_l1_bwd_x3 (net.py:1575)", BOTH, _has(*L1X), _lacks(*L1X, need=ATT),
           ["clsr-A1_48", "clsr-A1_8", "clsr-A0_80"], ["clsr-A1_52", "clsr-A1_4", "clsr-A0_84"]),
    # (reached where the split-product kernel refuses)
    Branch("att_l1_bwd (net.py:1578)", BOTH, _has("clsr_att_l1_bwd"), _has("clsr_att_dy1_apply"),
           ["clsr-A0_128", "clsr-A1_44"], ["clsr-A0_132", "clsr-A1_52"]),
    Branch("proj_x3 (net.py:2142, 2191)", BOTH, _has("clsr_proj_x3"), _has("clsr_proj_x3_wide"),
           ["clsr-D12-time4lstm", "clsr-D64-gru"], ["clsr-D44-time4lstm", "clsr-D48-time4lstm"]),
    Branch("proj_x3_tt (net.py:2179)", BOTH, _has("clsr_proj_x3_tt"), _lacks("clsr_proj_x3_tt", need=("clsr_t4_time_inputs_fwd2",)),
           ["clsr-golden-G2", "clsr-D24-G2"], ["clsr-D44-time4lstm", "clsr-D48-time4lstm"]),
    Branch("enc_bwd_fused (net.py:1986)", BOTH, _has(*ENCB), _lacks(*ENCB, need=("clsr_t4_time_inputs_fwd2",)),
           ["clsr-golden-G2", "clsr-golden-G16"], ["clsr-D24-G2", "clsr-D44-time4lstm"]),
    Branch("mlp_tail_softmax (net.py:2470)", BOTH, _has("clsr_mlp_tail_softmax"), _has("clsr_softmax_loss"),
           ["clsr-L100x64", "clsr-D24-G8"], ["clsr-L100x68", "clsr-D24-G9"]),
    Branch("heads_fused (net.py:2301)", BOTH, _has("clsr_heads_fused_step1"), _lacks("clsr_heads_fused_step1", "clsr_heads_fused_step2"),
           ["clsr-golden-G8"], ["clsr-golden-G9", "clsr-D24-G8"]),
    # the recurrences: read from the descriptors of the forward launch
    Branch("fused input projection (net.py:1916)", BOTH, lambda n, r: bool(r) and all(x for x, _ in r),
           lambda n, r: bool(r) and not any(x for x, _ in r), ["clsr-D48-gru", "clsr-D48-time4lstm"], ["clsr-D52-gru", "clsr-D52-time4lstm"]),
    Branch("three-piece recurrence products (net.py:212)", ("fp32",), lambda n, r: bool(r) and all(p == 3 for _, p in r),
           lambda n, r: bool(r) and all(p == 1 for _, p in r), ["clsr-D48-gru", "clsr-D48-lstm"], ["clsr-D52-gru", "clsr-D52-lstm"]),
]
# One-sided from the step, with the reason (tests/test_boundaries_cpu.py ONE_SIDED lists the same rows):
#   recurrences, n % 4 in 4 .. 128       -- no fallback: _shape_limits refuses the other side at construction
#   recurrence tile instance <3> / <8>   -- chosen inside the launch from n (csrc/rnn.hip): n = 48 / 52 run, nothing to read here
#   enc_back_x3 (net.py:2060)            -- reached only inside the fused encoder tail, i.e. at D = 40 alone, where it admits
#   att_l0_bwd_x3 under precision="fp32" -- off by mode (att_bwd_l0 = "fp32"), whatever the shape


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_both_sides_launched(precision):
    by_id = {c.id: c for c in CASES}
    rows = [b for b in BRANCHES if precision in b.precisions]
    wanted = sorted({i for b in rows for i in b.inside + b.outside if by_id[i].kind == "clsr" or precision == "fp32"})
    seen = {i: _guarded(by_id[i], _launches, by_id[i], precision) for i in wanted}
    wrong = []
    for b in rows:
        inside, outside = [i for i in b.inside if i in seen], [i for i in b.outside if i in seen]
        assert inside and outside, b.name
        for i in inside:
            if not b.fused(*seen[i]):
                wrong.append("%s: %s did not launch the fused entry" % (b.name, i))
        for i in outside:
            if not b.other(*seen[i]):
                wrong.append("%s: %s did not launch the other side" % (b.name, i))
        print("%-52s fused: %-48s other: %s" % (b.name, " ".join(inside), " ".join(outside)))
    assert not wrong, wrong
