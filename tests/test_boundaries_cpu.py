"""The committed dispatch-boundary cases (scripts/fuzz_step.py boundary_cases()) without a GPU:

* admission -- the float32 ORACLE, in the place of the HIP step, stays within fuzz_step.LONG_ADMIT (half) of every gradient /
  clip-norm / update bar against the float64 oracle on every case; a draw that does not is replaced from the case's own
  stream (BOUNDARY_REDRAWN, at most one case in twenty, same kind and pinned shape).  The device plays no part in it.
* the rule of the list -- for every shape-dependent branch of the step (BRANCHES: the kernels' own ``clsr_*_supported``
  queries, and the net's own predicates where net.py decides by a literal) and every swept hyper-parameter, the list holds
  the last value the branch admits and the first it refuses, at both ends of the admitted range.  The admitted range is
  FOUND by asking the query on every value the constructor accepts; no limit is written down here.
* the older lists (16 + 30 committed fuzz seeds, long_cases()) describe the same cases as before the pin repair of
  draw_case.
* widths past the recurrences' range, which has no fallback, are refused by key name at construction."""
import collections
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import fuzz_step  # noqa: E402
from clsr_amd.net import CLSRNet  # noqa: E402
from clsr_amd.ops import query  # noqa: E402
from clsr_amd.seqnet import SeqNet  # noqa: E402


@pytest.fixture(autouse=True)
def plain_draws(monkeypatch):
    for k in ("FUZZ_LONG", "FUZZ_CASE", "FUZZ_OVERRIDE"):      # (they would change what draw_case draws)
        monkeypatch.delenv(k, raising=False)


CASES = fuzz_step.boundary_cases()
AXES = sorted({c.axis for c in CASES})


# ------------------------------------------------------------------------------------------------- admission
@pytest.mark.parametrize("axis", AXES)
def test_float32_oracle_within_half_of_every_bar(axis, monkeypatch):
    monkeypatch.setenv("FUZZ_F32", "cpu")
    worst = {}
    for c in fuzz_step.boundary_cases(axes=[axis]):
        fuzz_step.STATS.clear()
        problems = fuzz_step.run_case(c)
        assert not problems, (c.id, c.desc, problems[:6])
        assert fuzz_step.STATS, c.id                      # (the comparisons ran)
        worst[c.id] = fuzz_step.worst_ratio()
    fuzz_step.STATS.clear()
    print(axis, "worst err / bar %.3f at %s" % max((v, k) for k, v in worst.items()))
    over = {k: round(v, 3) for k, v in worst.items() if not v <= fuzz_step.LONG_ADMIT}
    assert not over, over


def test_shape_of_the_list():
    assert len({c.idx for c in CASES}) == len({c.id for c in CASES}) == len(CASES)
    assert [c.idx for c in CASES] == list(range(len(CASES)))
    tiny = fuzz_step.BOUNDARY_TINY
    for c in CASES:
        assert (c.T, c.P, c.lengths) == (tiny["T"], tiny["P"], tiny["lengths"]) and c.P >= 2, c.id
        assert c.G == tiny["G"] or c.axis == "G", c.id
        assert all(getattr(c, k) == v for k, v in c.pin.items() if k in ("D", "Dc", "T", "P", "G")), c.id
        hyper = {k: v for k, v in c.pin.items() if k not in ("D", "Dc", "T", "P", "G", "lengths")}
        assert hyper and all(getattr(c.hp, k) == v for k, v in hyper.items()), (c.id, hyper)
        assert c.hp.item_embedding_dim + c.hp.cate_embedding_dim == c.D
    # at most one case in twenty is a replaced draw; it keeps its kind and its pinned shape, and moves no other
    redrawn = fuzz_step.BOUNDARY_REDRAWN
    assert 20 * len(redrawn) <= len(CASES) and set(redrawn) <= {c.idx for c in CASES}
    assert {c.idx for c in CASES if c.attempt} == set(redrawn)
    plain = {c.idx: c for c in fuzz_step.boundary_cases(redrawn={})}
    for c in CASES:
        p = plain[c.idx]
        assert (c.kind, c.pin, c.id) == (p.kind, p.pin, p.id)
        assert (c.desc == p.desc) == (not c.attempt), c.id
    # the swept values the issue of this list names
    d = collections.defaultdict(set)
    for c in CASES:
        if c.axis == "D":
            d[c.hp.sequential_model].add(c.D)
    assert set().union(*d.values()) == set(range(8, 129, 4))
    assert all(set(fuzz_step.BOUNDARY_D_EVERY_ENC) <= d[e] for e in fuzz_step.BOUNDARY_ENC)
    assert {c.Dc for c in CASES if c.axis == "D"} > {4}
    assert {c.kind for c in CASES} == {"clsr"} | set(fuzz_step.BOUNDARY_SIBLINGS)
    # the fp32x3 subset: CLSR only (the siblings' model API admits nothing else)
    assert all(c.kind == "clsr" for c in CASES if c.x3) and sum(1 for c in CASES if c.x3) >= 80


# ------------------------------------------------------------------------- the older lists are what they were
OLD_LISTS = dict(clsr="edb85bb29d5ef6dda8228ffb480ace3ae3e595b71d90500c39f4d83322e2afd9",
                 siblings="5117eeaa068cb6db9131b7d7597e661f5337985ac3c4b27d549d5608b3838be9",
                 long="9e84c0564e397546222a56aa50cb472d45cad538bae037d9443f0108812a616b")


def test_older_lists_unchanged():
    """sha256 of the descriptions (shape + every hyper-parameter) of the 16 + 30 committed fuzz cases of
    tests/test_fuzz_gpu.py and of long_cases(), taken before draw_case's sibling overrides followed a pinned D."""
    got = {}
    for name, n, seed, kinds in (("clsr", 16, 0, ["clsr"]), ("siblings", 30, 7, ["gru4rec", "din", "sli_rec", "a2svd", "dien"])):
        rng = np.random.default_rng(seed)
        got[name] = "\n".join(fuzz_step.draw_case(rng, i, kinds[i % len(kinds)]).desc for i in range(n))
    got["long"] = "\n".join(c.desc for c in fuzz_step.long_cases())
    assert {k: hashlib.sha256(v.encode()).hexdigest() for k, v in got.items()} == OLD_LISTS


def test_pinned_width_reaches_the_sibling_overrides():
    for kind in ("sli_rec", "a2svd"):
        c = fuzz_step.draw_case(np.random.default_rng(3), 0, kind, pin=dict(D=44, Dc=4))
        assert c.hp.attention_size == 44 and (kind != "sli_rec" or c.hp.hidden_size == 44)


# --------------------------------------------------------------------------------------- the rule of the list
def _net(c, precision="fp32"):
    if c.kind == "clsr":
        return CLSRNet(c.hp, c.dims, device="cpu", seed=0, precision=precision)
    return SeqNet(c.hp, c.dims, kind=c.kind, device="cpu", seed=0)


def _attentions(net, c):
    """(key, key width Dk, query width Q, history-level query columns qh) of the attention-MLP blocks of the graph, as
    net.py:1186 / seqnet.py:436, 466, 511 call them."""
    if c.kind == "clsr":
        return [("lt", net.D, net.Du, 0), ("st", net.H, net.Du + net.D, net._att_qh("st"))]
    return {"din": [("st", net.D, net.D, 0)], "dien": [("st", net.H, net.D, 0)], "sli_rec": [("st", net.H, net.D, 0)]}.get(c.kind, [])


def branches(c):
    """branch -> admitted?, for the shapes this case produces, by the kernels' own queries (and the net's own predicates).
    Rows of DESIGN.md section 6 / tests/test_boundaries_gpu.py BRANCHES."""
    net = _net(c)
    G, M = net.G_train, c.P * c.T
    A0, A1, L1 = net.A0, net.A1, net.L1
    out = collections.OrderedDict()
    for key, Dk, Q, qh in _attentions(net, c):
        Qe = Q - qh
        out["att_hist_fwd_x3." + key] = query("clsr_att_hist_fwd_x3_supported", Dk, Q, A0, qh)
        out["att_hist_bwd_x3." + key] = query("clsr_att_hist_bwd_x3_supported", Dk, Q, A0, qh)
        out["att_l0_fwd." + key] = query("clsr_att_l0_fwd_supported", G, Qe, A0)
        out["att_l0_bwd." + key] = query("clsr_att_l0_bwd_supported", G, Qe, A0)
        if c.kind == "clsr":          # (the two-piece instances: precision="fp32x3", CLSR only)
            out["att_l0_bwd_x3." + key] = query("clsr_att_l0_bwd_x3_supported", G, Qe, A0)
            out["att_l0_bwd_x3 halves." + key] = _net(c, "fp32x3")._l0_bwd_halves_ok(G, Qe)
    if net.A0:
        out["att_l1_fwd"] = query("clsr_att_l1_fwd_supported", A0, A1)
        out["att_l1_bwd_x3"] = query("clsr_att_l1_bwd_x3_supported", A1, A0)
        out["att_l1_bwd"] = query("clsr_att_l1_bwd_supported", A1, A0)
    out["mlp_tail_softmax"] = query("clsr_mlp_tail_softmax_supported", G, L1)
    if c.kind == "clsr":
        D, H = net.D, net.H
        NX = net._xw_blocks()[1]
        out["rnn three-piece products"] = net.rnn_products == "x6"
        out["rnn fused input projection"] = net._rnn_fp_on()
        out["rnn fused input projection (fp32x3)"] = _net(c, "fp32x3")._rnn_fp_on()
        out["proj_x3 (K = D)"] = query("clsr_proj_x3_supported", M, net.enc_in, NX)
        if c.hp.sequential_model == "time4lstm":
            Dp = 16 * ((D + 15) // 16)
            out["proj_x3 (K = Dp + 2H)"] = query("clsr_proj_x3_supported", M, Dp + 2 * H, 3 * H)
            out["proj_x3_tt"] = query("clsr_proj_x3_tt_supported", M, D, Dp, H, 3 * H)
            out["enc_bwd_fused"] = query("clsr_enc_bwd_fused_supported", D, H, NX)
    return collections.OrderedDict((k, bool(v)) for k, v in out.items())


# swept hyper-parameter of an axis: (value of a case, pin with another value, finest step)
SWEPT = {
    "D": (lambda c: c.D, lambda pin, v: dict(pin, D=v, Dc=4), 4),
    "A0": (lambda c: c.hp.att_fcn_layer_sizes[0], lambda pin, v: dict(pin, att_fcn_layer_sizes=[v, pin["att_fcn_layer_sizes"][1]]), 4),
    "A1": (lambda c: c.hp.att_fcn_layer_sizes[1], lambda pin, v: dict(pin, att_fcn_layer_sizes=[pin["att_fcn_layer_sizes"][0], v]), 4),
    "L": (lambda c: c.hp.layer_sizes[1], lambda pin, v: dict(pin, layer_sizes=[pin["layer_sizes"][0], v]), 4),
    "G": (lambda c: c.G, lambda pin, v: dict(pin, G=v), 1),
    "Q": (lambda c: c.D, lambda pin, v: dict(pin, D=v, Dc=4), 4),
    "H": (lambda c: c.hp.hidden_size, lambda pin, v: dict(pin, D=v) if "hidden_size" not in pin else dict(pin, hidden_size=v), 4),
}
GRID_END = {"G": 32}          # (rows per positive have no limit of their own; widths: whatever the constructor accepts)
# Branches whose other side no hyper-parameter reaches, with the reason (the GPU test lists the same):
ONE_SIDED = {
    "recurrences, n % 4 in 4 .. 128": "no fallback: _shape_limits refuses the other side at construction (test_refusals)",
    "recurrence tile instance <3> / <8>": "chosen inside the launch from n (csrc/rnn.hip); n = 48 and 52 run in every encoder",
    "enc_back_x3": "reached only inside the fused encoder tail, i.e. at D = n = 40, where it admits (net.py:2060)",
    "heads_fused": "admits the golden widths only and asks the device for its CU count: its two sides are the golden and "
                   "the D = 24 cases of the G axis, told apart on the device (tests/test_boundaries_gpu.py)",
    "att_hist_*_x3: qh <= 48": "qh = Du = D = Q / 2 in the CLSR graph, and Q <= 80 binds first",
    "att_l1_fwd: M A1 4 < 2^30, att_l1_bwd_x3: (M A0 + 80) 4 < 2^31, proj_x3_wide / pgemm_dw_wide: M >= 32768":
        "bounds on the row count, not on a width: out of reach of a tiny shape (tests/test_fullsize_gpu.py runs past them)",
    "att_l0_bwd_x3 halves: Qw / 2 <= 80": "Q = D <= 128 in the CLSR graph; the siblings, whose Q reaches 160 / 164, run fp32 only",
}


def _template(c, axis):
    return (c.kind, repr(sorted((k, v) for k, v in SWEPT[axis][1](c.pin, 0).items())))


def _grid(c, axis):
    """Every value of the swept hyper-parameter the constructor accepts around this case (the rest of the pin kept)."""
    _, repin, step = SWEPT[axis]
    out = []
    for v in range(step, GRID_END.get(axis, 1100), step):
        try:
            h = fuzz_step.draw_case(np.random.default_rng(0), c.idx, c.kind, pin=repin(c.pin, v))
            _net(h)
        except (NotImplementedError, ValueError):
            continue
        out.append((v, h))
    return out


@pytest.mark.parametrize("axis", sorted(SWEPT))
def test_both_sides_of_every_boundary(axis):
    value = SWEPT[axis][0]
    groups = collections.OrderedDict()
    for c in CASES:
        if c.axis == axis:
            groups.setdefault(_template(c, axis), []).append(c)
    edges, held = set(), set()         # (branch, "upper" | "lower") that exist along this axis / that some group holds
    for cs in groups.values():
        listed = {value(c) for c in cs}
        if len(listed) < 2:           # (a group of one value holds no pair; its branches are some larger group's)
            continue
        grid = _grid(cs[0], axis)
        vals = [v for v, _ in grid]
        table = [branches(h) for _, h in grid]
        for name in table[0]:
            adm = [v for v, t in zip(vals, table) if t.get(name)]
            if not adm or len(adm) == len(vals):
                continue
            for end, inside in (("upper", max(adm)), ("lower", min(adm))):
                i = vals.index(inside) + (1 if end == "upper" else -1)
                if 0 <= i < len(vals):
                    edges.add((name, end))
                    if {inside, vals[i]} <= listed:
                        held.add((name, end))
    print(axis, "edges held:", sorted(held))
    assert edges, axis            # (an axis none of whose values moves a branch would not belong in the list)
    assert not edges - held, sorted(edges - held)


def test_every_branch_has_both_sides_in_the_list():
    """Across the whole list every two-sided branch is admitted by some case and refused by some case."""
    seen = collections.defaultdict(set)
    for c in CASES:
        for name, ok in branches(c).items():
            seen[name.split(".")[0]].add(ok)
    assert all(v == {True, False} for v in seen.values()), {k: v for k, v in seen.items() if v != {True, False}}
    assert len(seen) >= 16


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    """What has no fallback is refused by key name at construction (CLSRNet._shape_limits)."""
    base = [c for c in CASES if c.id == "clsr-D24-G2"][0]
    for pin, word in ((dict(D=132, Dc=4), "hidden_size"), (dict(att_fcn_layer_sizes=[260, 8]), "att_fcn_layer_sizes"),
                      (dict(att_fcn_layer_sizes=[16, 6]), "MLP layer widths"), (dict(layer_sizes=[1028, 8]), "MLP layer widths"),
                      (dict(D=22, Dc=4), "embedding dims")):
        c = fuzz_step.draw_case(np.random.default_rng(0), 0, "clsr", pin=dict(base.pin, **pin))
        with pytest.raises(NotImplementedError, match=word):
            _net(c)
    sib = [c for c in CASES if c.id == "dien-H128"][0]
    c = fuzz_step.draw_case(np.random.default_rng(0), 0, "dien", pin=dict(sib.pin, hidden_size=132))
    with pytest.raises(NotImplementedError, match="hidden_size"):
        _net(c)
