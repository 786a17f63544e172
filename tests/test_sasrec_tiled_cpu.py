"""The tiled SASRec kernels without a GPU: the host-side queries of csrc/sasrec.hip against the case table's claims and the
formula DESIGN.md section 9f states, the conditions the kernel cases' comparisons rest on (which pins their seeds), and the
``long_histories`` keyword through ``SeqNet._check_supported``."""
import pytest
import torch

import sasrec_cases as K
import sasrec_oracle as O
import sasrec_tiled_cases as TK
from clsr_amd.ops import query


def _shape(tc):
    c = tc.case
    return c.T, c.Tmax, c.Di + c.Dc, c.nb, c.nh


def test_cases_are_admitted_and_past_is_refused():
    for tc in TK.CASES:
        assert query("clsr_sasrec_tiled_supported", *(_shape(tc) + (tc.tile,))) == 1, TK.case_id(tc)
        assert 1 <= tc.tile <= TK.TILE_MAX
    assert len(TK.PAST) >= 3
    for shape, what in TK.PAST:
        assert query("clsr_sasrec_tiled_supported", *shape) == 0, what
        assert query("clsr_sasrec_tiled_workspace_floats", 2, shape[0], shape[1], shape[2], shape[3], shape[5], 1) == 0, what
    assert query("clsr_sasrec_tiled_default_tile", TK.T_MAX + 1, 8) == 0
    # every refusal of clsr_sasrec_supported that is not about LDS is one of the tiled query too
    for shape, what in K.PAST[2:]:
        assert query("clsr_sasrec_tiled_supported", *(shape + (4,))) == 0, what


def test_lds_stays_within_the_budget_and_equals_the_formula():
    for tc in TK.CASES:
        T, _, C, _, _ = _shape(tc)
        for training in (1, 0):
            n = TK.lds_bytes(T, C, tc.tile, training)
            assert 0 < n <= TK.BUDGET and n == TK.lds_formula(T, C, tc.tile, training), TK.case_id(tc)
        assert TK.lds_bytes(T, C, tc.tile, 0) < TK.lds_bytes(T, C, tc.tile, 1)
    assert TK.BUDGET == 160 * 1024
    assert TK.lds_bytes(250, 40, 64) == 4 * (2 * 250 * 41 + 64 * (7 * 41 + 21))
    assert TK.lds_bytes(9, 8, 64) == TK.lds_bytes(9, 8, 9)          # (a tile past T holds T rows)
    # the default tile is the largest the budget holds
    for T, C in ((250, 40), (TK.T_MAX, 48), (TK.T_MAX, TK.C_MAX), (TK.T_AT_40 + 1, 40)):
        tile = TK.default_tile(T, C)
        assert 1 <= tile <= TK.TILE_MAX and TK.lds_bytes(T, C, tile) <= TK.BUDGET
        assert tile == TK.TILE_MAX or TK.lds_bytes(T, C, tile + 1) > TK.BUDGET


def test_boundary_cases_are_refused_resident_and_admitted_tiled():
    assert len(TK.BOUNDARY) == 2
    for tc in TK.BOUNDARY:
        assert query("clsr_sasrec_supported", *_shape(tc)) == 0
        assert query("clsr_sasrec_tiled_supported", *(_shape(tc) + (tc.tile,))) == 1
        assert tc.tile == TK.default_tile(tc.case.T, tc.case.Di + tc.case.Dc)
    assert TK.FIRST_PAST.case.T == TK.T_AT_40 + 1 and query("clsr_sasrec_supported", TK.T_AT_40, TK.T_AT_40, 40, 1, 1) == 1


def test_every_length_is_admitted_at_40_channels():
    for C in (8, 16, 24, 32, 40):
        assert all(TK.default_tile(T, C) > 0 for T in range(1, TK.T_MAX + 1)), C
    assert all(query("clsr_sasrec_tiled_supported", T, T, 40, 2, 1, TK.default_tile(T, 40)) for T in range(1, TK.T_MAX + 1))


def test_case_table_reaches_what_it_says():
    m = TK.MULTI.case
    shape = (m.Hn, m.T, m.Tmax, 8, m.nb)
    assert query("clsr_sasrec_tiled_parts", *shape) == TK.PARTS_CAP <= query("clsr_sasrec_max_parts") and m.Hn == TK.PARTS_CAP + 3
    P = query("clsr_sasrec_param_floats", m.Tmax, 8, m.nb)
    assert query("clsr_sasrec_tiled_workspace_floats", *(shape + (2, 1))) == TK.PARTS_CAP * (P + m.T * (3 * 8 + 4))
    assert query("clsr_sasrec_tiled_workspace_floats", *(shape + (2, 0))) == TK.PARTS_CAP * m.T * 8
    assert query("clsr_sasrec_tiled_parts", 3, 9, 9, 8, 1) == 3
    lens = K.make_inputs(TK.MIXED.case)["lens"].tolist()
    assert lens == [8, 4, 5, 0, 1] and TK.MIXED.tile == 4 and TK.MIXED.case.T == 8
    k = TK.KUAISHOU
    assert (k.case.T, k.case.Tmax, k.case.Di + k.case.Dc, k.case.nb, k.case.Hn, k.case.lens) == (250, 250, 40, 2, 2, (250, 131))
    assert [tc.case.T for tc in TK.CASES[:1]] == [1] and TK.CASES[5].case.Tmax > TK.CASES[5].case.T
    assert TK.CASES[6].case.nb == TK.NB_MAX and TK.CASES[12].case.T == TK.T_MAX
    assert TK.NINE.T % 4 and TK.NINE.nh == 2 and (TK.NINE.Di + TK.NINE.Dc) // TK.NINE.nh == 4


@pytest.mark.parametrize("tc", [tc for i, tc in enumerate(TK.CASES) if tc.case not in [o.case for o in TK.CASES[:i]]],
                         ids=TK.case_id)
def test_tiled_cases_meet_their_conditions(tc):
    """The check of tests/test_sasrec_cpu.py::test_kernel_cases_meet_their_conditions on the tiled cases: with the committed
    seed (the first from 0 upward that does) the float64 reference alone has every layer-norm variance of a valid step
    >= 1e-4 and no ReLU input within 2^-16 of zero, and a float32 evaluation opens the same gates."""
    c = tc.case
    inp, ref = K.case_data(c)
    assert ref["min_var"] >= 1e-4, ref["min_var"]
    assert ref["min_pre"] > 2.0 ** -16, ref["min_pre"]
    r32 = K.reference(c, inp, torch.float32)
    assert all(torch.equal(a, b) for a, b in zip(ref["gates"], r32["gates"]))
    print("float32 restatement, largest |err| per tensor: " + " ".join("%.3e" % e for e in ref["fp32_errors"]))
    assert len(ref["bounds"]) == c.nb + 2 and all(0 < e < 1e-4 for e in ref["fp32_errors"])
    got, exp = O.checked_tensors(r32["s"], r32["cache"]), O.checked_tensors(ref["s"], ref["cache"])
    for g, e, b in zip(got, exp, ref["bounds"]):
        assert float((g.double() - e).abs().max()) <= b
    valid = ref["cache"]["valid"]
    if not bool(valid.all()):           # (the padding holds drawn values, the reference zeros)
        assert float(inp["hist"][~valid].abs().min()) > 0 and float(ref["cache"]["xL"][~valid].abs().max()) == 0.0


class _Passed(Exception):
    pass


def _past_check_supported(hp, kind, **kw):
    """Build the net up to the step behind ``_check_supported`` (no device is touched before it)."""
    from clsr_amd.seqnet import SeqNet

    class Probe(SeqNet):
        def _dropout_setup(self, seed):
            raise _Passed()

    with pytest.raises(_Passed):
        Probe(hp, dict(Vu=7, Vi=11, Vc=5), kind=kind, **kw)


def test_long_histories_keyword(golden_hparams):
    from clsr_amd.seqnet import SeqNet

    dims = dict(Vu=7, Vi=11, Vc=5)
    for T in (250, TK.T_AT_40 + 1, TK.T_MAX, 50):
        _past_check_supported(O.hparams(golden_hparams, max_seq_length=T), "sasrec", long_histories=True)
    _past_check_supported(O.hparams(golden_hparams, max_seq_length=50), "sasrec")
    # without the keyword the documented refusal stands, and names what lifts it
    with pytest.raises(NotImplementedError, match="max_seq_length 250") as e:
        SeqNet(O.hparams(golden_hparams, max_seq_length=250), dims, kind="sasrec")
    assert "long_histories=True" in str(e.value)
    with pytest.raises(NotImplementedError, match="max_seq_length 250"):
        SeqNet(O.hparams(golden_hparams, max_seq_length=250), dims, kind="sasrec", long_histories=False)
    # the trunk's limit and the other keys stay
    for kw, needle in ((dict(max_seq_length=TK.T_MAX + 1), "max_seq_length"), (dict(num_heads=3), "num_heads"),
                       (dict(item_embedding_dim=TK.C_MAX, cate_embedding_dim=8), "item_embedding_dim")):
        with pytest.raises(NotImplementedError, match=needle):
            SeqNet(O.hparams(golden_hparams, **kw), dims, kind="sasrec", long_histories=True)
    # the other kinds refuse the keyword by name
    hp = O.hparams(golden_hparams)
    hp.model_type = "GRU4Rec"
    with pytest.raises(NotImplementedError, match="long_histories"):
        SeqNet(hp, dims, kind="gru4rec", long_histories=True)


def test_model_takes_the_keyword(golden_hparams):
    import copy

    from clsr_amd.clsr import GRU4RecModel, SASRecModel
    from clsr_amd.sequential_iterator import SequentialIterator

    hp = O.hparams(golden_hparams, max_seq_length=250)
    with pytest.raises(NotImplementedError, match="max_seq_length 250"):
        SASRecModel(copy.deepcopy(hp), SequentialIterator, long_histories=False)
    assert SASRecModel._net_keywords is not GRU4RecModel._net_keywords
    with pytest.raises(TypeError, match="long_histories"):
        GRU4RecModel(copy.deepcopy(hp), SequentialIterator, long_histories=True)
