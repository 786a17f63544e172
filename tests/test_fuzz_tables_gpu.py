"""The embedding-table modes of CLSRNet against each other at random shapes (scripts/fuzz_tables.py): fp32 tables, bf16
tables and bf16 tables with an fp32 master, each through the sweep launches and through the row-list optimizer entries
(``rowlist_min_elems = 0``), on the same bf16-representable tables -- what tests/test_bf16_master_gpu.py,
tests/test_bf16_tables_gpu.py and test_row_list_optimizer_path_equals_sweep hold at the golden shape only.  Item widths
8 .. 120, histories of 1 .. 50 steps, 1 .. 64 positives, 2 .. 10 rows per positive, adam and lazyadam, the clip active and not;
a second step starts from residuals that are no longer zero."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import fuzz_tables  # noqa: E402


# case 0 is a regression case (FUZZ_CASE 16,8,1,64,2,time4lstm, dense adam): on its second step the master net through the
# sweep launches and the one through the single-table / row-list launches stored item masters one ulp apart -- the Adam
# moment updates were contracted into fused multiply-adds differently from kernel to kernel (csrc/tableopt.h: adam_elem)
IDS = ["regression_16_8_1_64_2_time4lstm_adam_second_step"] + ["case%d" % i for i in range(1, len(fuzz_tables.CASES))]


@pytest.mark.parametrize("case", range(len(fuzz_tables.CASES)), ids=IDS)
def test_table_modes_agree_at_random_shapes(case):
    pin, seed = fuzz_tables.CASES[case]
    c = fuzz_tables.one_case(pin, seed, case)
    for k, v in pin.items():
        assert getattr(c, k, None) == v or getattr(c.hp, k, None) == v, (k, v)


def test_the_pinned_shapes_are_among_the_cases():
    drawn = [fuzz_tables.draw(pin, seed, i) for i, (pin, seed) in enumerate(fuzz_tables.CASES)]
    assert all(fuzz_tables.accepts_bf16(c) and c.P <= 64 and c.T <= 50 for c in drawn)
    assert any((c.D, c.Dc, c.T) == (16, 8, 1) for c in drawn)
    assert any((c.D, c.Dc, c.T, c.lengths) == (64, 8, 50, "lognormal") for c in drawn)
    assert any((c.D, c.Dc) == (128, 8) for c in drawn)
    assert any(c.P == 1 for c in drawn) and any(c.G == 10 for c in drawn)
    assert {c.hp.optimizer for c in drawn} == {"adam", "lazyadam"}
    assert any(c.hp.is_clip_norm and c.hp.max_grad_norm == 0.01 for c in drawn)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_widths_bf16_tables_do_not_take_are_refused_before_any_launch(seed, monkeypatch):
    """A draw with category width 4, or an item width that is no multiple of 8: NotImplementedError from the constructor,
    before anything is allocated or launched."""
    from clsr_amd import net as N
    from clsr_amd import ops

    c = fuzz_tables.draw_rejected(seed)
    assert c.Dc == 4 or (c.D - c.Dc) % 8

    def launched(*a, **kw):
        raise AssertionError("a launch before the shape check")

    for mod, names in ((ops, ("call", "multi", "query", "sort_ids_multi")), (N, ("call", "query"))):
        for name in names:
            monkeypatch.setattr(mod, name, launched)
    for kw in (dict(table_dtype="bf16"), dict(table_dtype="bf16", table_master=True)):
        with pytest.raises(NotImplementedError):
            N.CLSRNet(c.hp, c.dims, device="cuda:0", seed=0, **kw)
    monkeypatch.undo()
    N.CLSRNet(c.hp, c.dims, device="cuda:0", seed=0)      # (the same draw is a valid fp32 net)


def test_the_rejected_draws_cover_both_reasons():
    drawn = [fuzz_tables.draw_rejected(seed) for seed in (0, 1, 2, 3)]
    assert any(c.Dc == 4 for c in drawn) and any(c.Dc == 8 and (c.D - c.Dc) % 8 for c in drawn), \
        [(c.D, c.Dc) for c in drawn]
