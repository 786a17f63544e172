"""The committed sequences of scripts/fuzz_sequence.py (one long-lived net, seven training steps and two scorings over
shapes A A B E A C E A B, teacher-forced against the float64 oracle) on the CPU: what the list holds, the input conditions
of its feeds, and the float32 ORACLE in the net's place, which must meet every bar of every step of every sequence -- a
sequence it misses would be ill-conditioned in float32 whatever the kernels do (DESIGN.md has its worst ratio to each
bar).  No GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import fuzz_sequence as Q  # noqa: E402
import fuzz_step  # noqa: E402

GROUPS = dict(clsr=Q.CLSR_KINDS, siblings=Q.SIB_KINDS, caser_ncf_nextitnet=Q.OWN_KINDS)


@pytest.fixture(autouse=True)
def plain_draws(monkeypatch):
    for k in ("FUZZ_LONG", "FUZZ_CASE", "FUZZ_OVERRIDE", "FUZZ_F32"):      # (they would change what draw_case draws)
        monkeypatch.delenv(k, raising=False)


def test_the_committed_list():
    seqs = Q.sequences()
    assert len(seqs) == len({s.id for s in seqs}) == 22
    assert [w for w, _, _ in Q.SCHEDULE].count("train") == 7 and [w for w, _, _ in Q.SCHEDULE].count("score") == 2
    clsr = [s for s in seqs if s.kind == "clsr"]
    assert sorted(s.hp.sequential_model for s in clsr) == ["gru"] * 2 + ["lstm"] * 2 + ["time4lstm"] * 2
    for attr, want in (("lazy", {True: 3, False: 3}), ("dedup", {True: 3, False: 3})):
        assert {v: sum(1 for s in clsr if getattr(s, attr) == v) for v in want} == want
    assert sorted(s.hp.contrastive_loss for s in clsr) == ["bpr"] * 3 + ["triplet"] * 3
    assert sum(1 for s in clsr if s.hp.is_clip_norm and s.hp.max_grad_norm == 0.01) == 3
    assert {s.hp.item_embedding_dim + s.hp.cate_embedding_dim for s in clsr} == {16, 40, 52}
    assert [s.shapes["B"] for s in clsr if s.shapes["B"]["T"] == 65] == [dict(P=3, T=65, G=2)]
    for s in clsr:
        assert s.shapes["A"]["P"] == 7 and s.shapes["A"]["T"] == 10 and s.shapes["C"]["P"] == 1 and s.shapes["C"]["T"] == 2
        assert s.hp.contrastive_length_threshold >= s.shapes["C"]["T"]           # step 6 has no long history
        assert s.shapes["B"] in (dict(P=33, T=17, G=s.shapes["A"]["G"]), dict(P=3, T=65, G=2))
    for kind in Q.SIB_KINDS + Q.OWN_KINDS:
        assert sorted(s.lazy for s in seqs if s.kind == kind) == [False, True], kind
    for s in seqs:
        assert s.shapes["E"]["G"] != s.shapes["A"]["G"] and s.shapes["E"]["P"] != s.shapes["A"]["P"]
        assert s.dims["Vu"] == 50 and s.dims["Vc"] == 12 and s.dims["Vi"] == (4000 if s.kind == "nextitnet" else 200)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_input_conditions_hold_for_every_sequence(group):
    """Properties of the feeds alone: from the second training step on, the item table and every user table see a row that
    is new and leave out a row touched before -- otherwise the row checks of a step would have nothing to look at.  (By
    group: only NextItNet's feeds, tests/nextitnet_cases.py, ask the built library for anything.)"""
    seqs = Q.sequences(GROUPS[group])
    assert seqs
    problems = [p for s in seqs for p in Q.input_conditions(s)]
    assert not problems, problems


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_float32_oracle_meets_every_bar(group):
    failures, worst = [], {}
    fuzz_step.STATS.clear()
    for s in Q.sequences(GROUPS[group]):
        problems = Q.run_sequence(s, cpu=True)
        if problems:
            failures.append((s.desc, problems[:6]))
    for tag, st in fuzz_step.STATS.items():
        if not tag[0].endswith(" rows"):
            worst[tag[0]] = max(worst.get(tag[0], 0.0), st[0])
    rows = {tag: st[2] for tag, st in fuzz_step.STATS.items() if tag[0].endswith(" rows")}
    fuzz_step.STATS.clear()
    print("worst err / bar per check:", {k: round(v, 3) for k, v in sorted(worst.items())})
    assert not failures, failures
    # the comparisons ran: every bar was reached, and rows of both kinds were there to be looked at
    assert {"logit", "model_output", "loss", "grad", "norm", "update", "slot m", "slot v", "eval logit"} <= set(worst)
    assert rows[("never rows", "item")] > 0 and rows[("stale rows", "item")] > 0
