"""One long-lived net held to the float64 oracle across steps of changing shape (scripts/fuzz_sequence.py): seven training
steps and two scorings over shapes A A B E A C E A B, the oracle stepped from the net's own ``state_dict()`` before every
step (teacher forcing), so the single-step bars of tests/test_step_gpu.py / test_siblings_gpu.py hold at every step --
logits, model output, every loss term, the update of every dense variable and table, the Adam moments and clock, the
batch-norm moving statistics, never-touched rows bit-identical to the loaded state, rows touched earlier and not now frozen
under lazyadam and decayed under adam.  What a fresh net per case cannot show: a workspace relied on to be zero, a flag
table or row list not cleared, a stale scalar in a replayed launch plan, dense Adam skipping decayed rows.

Every sequence runs twice: pass 1 with launch plans and one persistent uploaded feed object per shape (at least one
training and one scoring plan must have been replayed), pass 2 on a new net without plans and with the captured gradients
held to the oracle too.  tests/test_sequence_cpu.py holds the feeds to their input conditions and the float32 oracle to
the same bars."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(kinds, precision="fp32"):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import fuzz_sequence as Q

    failures = []
    for s in Q.sequences(kinds):
        problems = Q.run_sequence(s, precision, cpu=False)
        if problems:
            failures.append((s.desc, problems[:6]))
    assert not failures, failures


@pytest.fixture(autouse=True)
def plain_draws(monkeypatch):
    for k in ("FUZZ_LONG", "FUZZ_CASE", "FUZZ_OVERRIDE", "FUZZ_F32"):      # (they would change what draw_case draws)
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_clsr_sequences(precision):
    _run(["clsr"], precision)


def test_sibling_sequences():
    _run(["gru4rec", "din", "sli_rec", "a2svd", "dien"])


def test_caser_ncf_nextitnet_sequences():
    _run(["caser", "ncf", "nextitnet"])
