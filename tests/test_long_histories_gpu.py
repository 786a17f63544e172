"""Histories of 63 .. 256 steps: the training / scoring step against the float64 oracles on the committed long cases of
scripts/fuzz_step.py (long_cases()).  The attention tail works in 64-step chunks, at most four: T = 63 / 64 / 65, 127 / 128 /
129, 191 / 192 / 193 and 250 / 255 / 256 are where a lane mask, a chunk count or an LDS extent is off by one, for CLSR and
the five sibling models (list A); list B has every history exactly 64 / 128 / 192 / 256 long.

One pytest case per committed case, so a failure names its shape.  Each is the full comparison of fuzz_step.run_case at the
bars of the random-shape tests (tests/test_fuzz_gpu.py): logits in training and scoring, the loss terms, every dense
gradient, every gradient table, the IndexedSlices clip norms of the replicated computation, the Adam / lazy-Adam update,
idle rows bit-equal, the batch-norm moving statistics, a non-finite value on either side a failure -- with de-duplicated
histories and without.  What is in the lists is decided by the float32 oracle alone
(tests/test_long_histories_cpu.py), never by what the device computes."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import fuzz_step  # noqa: E402

CASES = fuzz_step.long_cases()


def _run(case, precision):
    fuzz_step.PRECISION = precision
    try:
        problems = fuzz_step.run_case(case)
    finally:
        fuzz_step.PRECISION = "fp32"
    assert not problems, (case.desc, problems[:8])


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_long_step(case):
    """[din-T250-A33] found the fp32 partial sums of the batch-norm statistics of small batches (1.89 of the gradient-table
    bar; with the double sums 0.62).  DESIGN.md section 6 has the worst distance per check."""
    _run(case, "fp32")


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "clsr"], ids=[c.id for c in CASES if c.kind == "clsr"])
def test_long_step_clsr_fp32x3(case):
    """The two-piece split-bf16 products, held to the same bars as the fp32 products."""
    _run(case, "fp32x3")
