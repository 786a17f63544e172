"""The committed long-history cases (scripts/fuzz_step.py long_cases(): T = 63 .. 256, the edges of the 64-step chunks of
the attention tail) are well-conditioned in float32: the float32 ORACLE, in the place of the HIP step, meets every
gradient / clip-norm / update bar of the step comparison against the float64 oracle, and stays within half of each.  That
is the rule a draw is admitted by (a draw that misses it is replaced from a stream of its own, fuzz_step.LONG_REDRAWN,
DESIGN.md); what computes the step on the device plays no part in it.  The factor of two is what another summation
order may use.

The second condition of admission, also on the reference alone: the float64 step with the ReLU kinks of the hidden MLP
layers moved by +-2^-20 (fuzz_step.kink_case, KINK: the float32 noise of a batch-norm output) keeps every gradient within half of the
same bars.  A hidden unit that close to its kink with a gradient through it makes the case a coin toss for ANY float32
computation; one float32 run of the oracle cannot show that, it only shows the side IT fell on (the first replacement of
case A 43 had one unit at 4.2e-7 carrying 1.36e-6 of a gradient whose tensor maximum is 6.5e-6).  Both conditions are
read from STATS by the same ratio.  No GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import fuzz_step  # noqa: E402


@pytest.fixture
def float32_oracle_as_step(monkeypatch):
    monkeypatch.setenv("FUZZ_F32", "cpu")
    for k in ("FUZZ_LONG", "FUZZ_CASE", "FUZZ_OVERRIDE"):      # (they would change what draw_case draws)
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("kind", fuzz_step.LONG_KINDS)
def test_float32_oracle_within_half_of_every_bar(kind, float32_oracle_as_step):
    cases = fuzz_step.long_cases([kind])
    assert len(cases) == len(fuzz_step.LONG_T) + len(fuzz_step.LONG_FULL_T)
    worst = {}
    for c in cases:
        fuzz_step.STATS.clear()
        problems = fuzz_step.run_case(c)
        assert not problems, (c.id, c.desc, problems[:6])
        assert fuzz_step.STATS, c.id                      # (the comparisons ran)
        worst[c.id] = fuzz_step.worst_ratio()
    fuzz_step.STATS.clear()
    over = {k: round(v, 3) for k, v in worst.items() if not v <= fuzz_step.LONG_ADMIT}
    assert not over, over


def test_shape_of_the_lists(float32_oracle_as_step):
    cases = fuzz_step.long_cases()
    assert len({c.idx for c in cases}) == len(cases) == 96
    for which, Ts, cap in (("A", fuzz_step.LONG_T, 8), ("B", fuzz_step.LONG_FULL_T, 4)):
        part = [c for c in cases if c.which == which]
        # every kind x every T, once -- a replaced draw keeps its kind and its T
        assert sorted((c.kind, c.T) for c in part) == sorted((k, T) for k in fuzz_step.LONG_KINDS for T in Ts)
        assert sum(1 for c in part if c.attempt) == len(fuzz_step.LONG_REDRAWN[which]) <= cap
        assert set(fuzz_step.LONG_REDRAWN[which]) <= {c.idx for c in part}
    assert fuzz_step.LONG_T == (63, 64, 65, 127, 128, 129, 191, 192, 193, 250, 255, 256)
    assert all(c.P in (2, 3, 5) for c in cases if c.which == "A")
    for kind in fuzz_step.LONG_KINDS:
        mine = [c for c in cases if c.kind == kind]
        assert max(c.G for c in mine) >= 5
        # every chunk full: a history exactly T long (which the lengths drawn for list A need not give)
        for T in fuzz_step.LONG_FULL_T:
            full = [c for c in mine if c.which == "B" and c.T == T]
            assert len(full) == 1 and full[0].lengths == "full" and full[0].P == 3
            feed = fuzz_step.make_feed(full[0])
            assert int(feed["mask"].sum(1).max()) == T
    # a replaced draw moves no other: the rest equals the un-replaced stream
    plain = {c.idx: c.desc for c in fuzz_step.long_cases(redrawn=dict(A={}, B={}))}
    assert all(c.desc == plain[c.idx] for c in cases if not c.attempt)
