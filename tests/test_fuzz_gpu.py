"""Random small shapes of the training / scoring step against the oracles (scripts/fuzz_step.py): widths that are
not the golden 40, lengths 1..50 (63..256: tests/test_long_histories_gpu.py), 1..64 positives, 2..10 rows per positive,
all encoders and sibling models.  The
seeds below include the cases that exposed real limits (groups of more than 8 rows in the attention backward, bpr on
wide embeddings, DIN with D > T).

Every case also holds the embedding-table side of the step to the oracle (fuzz_step.table_checks): the gradient table of
every embedding (item widths 4 .. 124, where the sorted segmented sums change instantiation), the IndexedSlices clip norms
of the replicated computation, the (lazy-)Adam update of the tables with the clip active (max_grad_norm 0.01) and not, and,
under lazyadam, bit equality of every row the step does not involve.  The float32 ORACLE meets all of these bars on all 16
+ 30 committed cases (``FUZZ_F32=cpu python scripts/fuzz_step.py 16 0 clsr`` / ``... 30 7 gru4rec,din,sli_rec,a2svd,dien``,
worst distances in DESIGN.md): no case is ill-conditioned there, no seed was replaced.  A non-finite value on either
side of a comparison is a failure (cases 2, 7, 8 and 12 of seed 0 have no history longer than
contrastive_length_threshold: the oracle used to expect NaN gradients there, which every bar passed)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(n, seed, kinds, precision="fp32"):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import fuzz_step

    fuzz_step.PRECISION = precision
    rng = np.random.default_rng(seed)
    failures = []
    for i in range(n):
        desc, problems = fuzz_step.one_case(rng, i, kinds[i % len(kinds)])
        if problems:
            failures.append((desc, problems[:6]))
    assert not failures, failures


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_clsr_random_shapes(precision):
    """precision="fp32": every product at fp32 accuracy (the reference's arithmetic); "fp32x3": the two-piece split products,
    held to the same tolerances."""
    _run(16, 0, ["clsr"], precision)


def test_sibling_random_shapes():
    _run(30, 7, ["gru4rec", "din", "sli_rec", "a2svd", "dien"])


def test_model_api_random_batch_shapes(tmp_path):
    """fit / run_weighted_eval / predict with random batch sizes, negatives per positive and file sizes (ragged last
    batches, evaluation batches that cut groups apart): the product defaults (de-duplicated histories, compact feeds,
    launch plans, look-ahead staging) against the plain row-by-row configuration."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import fuzz_model

    rng = np.random.default_rng(0)
    failures = []
    for i in range(12):
        desc, problems = fuzz_model.one_case(rng, i, str(tmp_path))
        if problems:
            failures.append((desc, problems[:6]))
    assert not failures, failures
