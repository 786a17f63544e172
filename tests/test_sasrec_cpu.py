"""SASRec without a GPU: the oracle's pieces against torch's own operators, its explicit backward against autograd, the
variable inventory and flat layout, the yaml, the refusals by key name, the case table's own claims, and the conditions that
the kernel cases' comparisons rest on (tests/sasrec_cases.py), which pins their seeds."""
import copy
import math
import os

import numpy as np
import pytest
import torch

import sasrec_cases as K
import sasrec_oracle as O
from clsr_amd.ops import query
from clsr_amd.params import init_tensor, sibling_kind, sibling_specs


@pytest.mark.parametrize("nh,lens", [(1, (5, 7, 1)), (2, (7, 3, 0)), (4, (2, 6, 7))])
def test_attention_equals_torch(nh, lens):
    gen = torch.Generator().manual_seed(nh)
    T, C = 7, 16
    q, k, v = (torch.randn(3, T, C, generator=gen, dtype=torch.float64) for _ in range(3))
    valid, attend = O.masks(torch.tensor(lens), T)
    got, a = O.attention(q, k, v, attend, nh)
    # torch's own attention with the same mask; a row that sees no key is defined as zero here and NaN there
    seen = attend.any(-1)
    safe = attend | ~seen.unsqueeze(-1)
    exp = torch.nn.functional.scaled_dot_product_attention(O.heads(q, nh), O.heads(k, nh), O.heads(v, nh),
                                                           attn_mask=safe[:, None])
    exp = exp.transpose(1, 2).reshape(3, T, C)
    assert float((got - exp)[seen].abs().max()) < 1e-13
    assert float(got[~seen].abs().max() if bool((~seen).any()) else 0.0) == 0.0
    # a valid query sees exactly the keys s <= t, and they are all valid; its weights sum to one
    for h, n in enumerate(lens):
        for t in range(T):
            assert attend[h, t].tolist() == [t < n and s <= t for s in range(T)]
    assert float((a.sum(-1)[seen[:, None].expand(-1, nh, -1)] - 1).abs().max()) < 1e-13
    assert float(a[~attend[:, None].expand(-1, nh, -1, -1)].abs().max()) == 0.0


def test_layer_norm_equals_torch():
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(4, 7, 12, generator=gen, dtype=torch.float64)
    g, b = torch.randn(12, generator=gen, dtype=torch.float64), torch.randn(12, generator=gen, dtype=torch.float64)
    y, xhat, rstd, var = O.layer_norm(x, g, b)
    assert float((y - torch.layer_norm(x, (12,), g, b, eps=1e-8)).abs().max()) < 1e-13
    assert float((var - x.var(-1, unbiased=False, keepdim=True)).abs().max()) < 1e-14
    y2 = O.seq_layer_norm(x, g, b)[0]
    assert float((y - y2).abs().max()) < 1e-13
    W, c = torch.randn(12, 12, generator=gen, dtype=torch.float64), torch.randn(12, generator=gen, dtype=torch.float64)
    assert float((O.seq_linear(x, W, c) - O.linear(x, W, c)).abs().max()) < 1e-13


def test_position_counts_back_from_the_most_recent_action():
    """The encoder sees a history the same wherever its padding is: s depends on the valid steps alone."""
    c = K.MIXED
    inp = K.make_inputs(c)
    enc = O.cast(inp["enc"], torch.float64)
    hist, lens = inp["hist"].double(), inp["lens"]
    s, cache = O.encoder_forward(hist, lens, enc, c.nh)
    other = hist.clone()
    other[~cache["valid"]] = 123.0
    assert torch.equal(O.encoder_forward(other, lens, enc, c.nh)[0], s)
    for h, n in enumerate(lens.tolist()):
        for t in range(n):
            assert torch.equal(cache["x0"][h, t], hist[h, t] + enc["pos"][n - 1 - t])
        assert float(cache["x0"][h, n:].abs().max() if n < c.T else 0.0) == 0.0
    assert float(s[lens == 0].abs().max()) == 0.0 and bool(torch.isfinite(s).all())
    # a history alone gives what it gives in the batch, and cut to its valid steps too
    h, n = 0, int(lens[0])
    alone = O.encoder_forward(hist[h:h + 1, :n], lens[h:h + 1], enc, c.nh)[0]
    assert float((alone[0] - s[h]).abs().max()) < 1e-13


@pytest.mark.parametrize("c", [K.MIXED, K.POS_PAST_T, K.CASES[5]], ids=K.case_id)
def test_explicit_backward_equals_autograd(c):
    inp = K.make_inputs(c)
    enc = O.cast(inp["enc"], torch.float64)
    leaves = [enc["pos"], enc["gf"], enc["bef"]] + [p[k] for p in enc["blocks"] for k in O.BLOCK_KEYS]
    for t in leaves:
        t.requires_grad_(True)
    hist = inp["hist"].double().requires_grad_(True)
    s, _ = O.encoder_forward(hist, inp["lens"], enc, c.nh)
    (s * inp["ds"].double()).sum().backward()
    ref = K.case_data(c)[1]
    assert float((hist.grad - ref["dhist"]).abs().max()) < 1e-12
    g = ref["grads"]
    assert float((enc["pos"].grad - g["pos"]).abs().max()) < 1e-12
    assert float((enc["gf"].grad - g["gf"]).abs().max()) < 1e-12 and float((enc["bef"].grad - g["bef"]).abs().max()) < 1e-12
    for l, p in enumerate(enc["blocks"]):
        for key in O.BLOCK_KEYS:
            assert float((p[key].grad - g["blocks"][l][key]).abs().max()) < 1e-12, (l, key)
    # padding: exactly zero gradient, and so are the rows of pos that no history reaches
    valid = ref["cache"]["valid"]
    assert float(ref["dhist"][~valid].abs().max() if bool((~valid).any()) else 0.0) == 0.0
    longest = int(inp["lens"].max())
    assert float(g["pos"][longest:].abs().max() if longest < c.Tmax else 0.0) == 0.0 and float(g["pos"][:longest].abs().min()) > 0


def test_variable_inventory(golden_hparams):
    hp = O.hparams(golden_hparams, num_blocks=2, num_heads=2)
    assert sibling_kind("SASRec") == "sasrec" and sibling_kind(hp.model_type) == "sasrec"
    dims = dict(Vu=7, Vi=11, Vc=5)
    specs = sibling_specs(dims, hp, "sasrec")
    assert [(n, tuple(s)) for n, s, _ in specs] == [(n, tuple(s)) for n, s, _ in O.param_specs(dims, hp)]
    enc = [(n, tuple(s), k) for n, s, k in specs if n.startswith(O.SCOPE)]
    assert [n for n, _, _ in enc] == O.encoder_names(2)
    assert not any(n.startswith("sequential/embedding") for n, _, _ in enc)
    b = O.SCOPE + "block_1/"
    assert [n[len(b):] for n, _, _ in enc if n.startswith(b)] == list(O.BLOCK_NAMES)
    kinds = {n[len(O.SCOPE):]: (s, k) for n, s, k in enc}
    assert kinds["position_embedding"] == ((hp.max_seq_length, 40), "w")
    assert kinds["block_0/attention/query/kernel"] == ((40, 40), "tnormal_0.02") and kinds["block_1/ffn_2/kernel"][1] == "tnormal_0.02"
    assert kinds["block_0/layer_norm1/gain"] == ((40,), "one") and kinds["layer_norm_final/bias"] == ((40,), "zero")
    assert kinds["block_1/attention/output/bias"] == ((40,), "zero")
    # (a name ending in /gamma would be taken for a batch-norm layer by the trunk)
    assert not any(n.endswith(("/gamma", "/beta")) for n, _, _ in enc)
    w = init_tensor("tnormal_0.02", (40, 40), hp, torch.Generator().manual_seed(0))
    assert float(w.abs().max()) <= 0.04 and 0.015 < float(w.std()) < 0.02
    n = sum(int(np.prod(s)) for _, s, _ in enc)
    assert n == query("clsr_sasrec_param_floats", hp.max_seq_length, 40, 2) == hp.max_seq_length * 40 + 2 * (6 * 1600 + 400) + 80
    # the flat layout of the kernels is the creation order
    e = O.encoder_of(O.init_params(dims, hp, seed=1, perturb=0.1), hp)
    back = O.unpack(O.pack(e), hp.max_seq_length, 40, 2)
    assert torch.equal(back["pos"], e["pos"]) and torch.equal(back["gf"], e["gf"]) and torch.equal(back["bef"], e["bef"])
    assert all(torch.equal(back["blocks"][i][k], e["blocks"][i][k]) for i in range(2) for k in O.BLOCK_KEYS)
    names = [n for n, _, _ in specs]
    assert O.pack(e).numel() == n and names.index(O.POS) == 3 and names[names.index(O.BEF) + 1].startswith("sequential/logit_fcn/")


def test_yaml_through_prepare_hparams():
    import clsr_amd
    from clsr_amd.deeprec_utils import prepare_hparams

    cfg = os.path.join(os.path.dirname(clsr_amd.__file__), "config")
    hp, gru = prepare_hparams(os.path.join(cfg, "sasrec.yaml")), prepare_hparams(os.path.join(cfg, "gru4rec.yaml"))
    assert hp.model_type == "SASRec" and hp.num_blocks == 2 and hp.num_heads == 1 and hp.hidden_size is None
    assert gru.num_blocks is None and gru.num_heads is None
    a, b = hp.values(), gru.values()
    assert set(a) == set(b)
    assert {k for k in a if a[k] != b[k]} == {"model_type", "num_blocks", "num_heads", "hidden_size"}
    C = hp.item_embedding_dim + hp.cate_embedding_dim
    assert query("clsr_sasrec_supported", hp.max_seq_length, hp.max_seq_length, C, hp.num_blocks, hp.num_heads) == 1
    assert query("clsr_sasrec_supported", 64, 64, 40, 2, 1) == 1


def test_refusals_are_reported_by_name(golden_hparams):
    from clsr_amd.clsr import SASRecModel
    from clsr_amd.seqnet import SeqNet
    from clsr_amd.sequential_iterator import SequentialIterator

    dims = dict(Vu=7, Vi=11, Vc=5)
    t_past = K.T_AT_40 + 1
    for kw, needle in ((dict(num_blocks=None), "num_blocks and num_heads"), (dict(num_heads=None), "num_blocks and num_heads"),
                       (dict(num_blocks=0), "num_blocks"), (dict(num_blocks=K.NB_MAX + 1), "num_blocks"),
                       (dict(num_blocks=1.5), "num_blocks"), (dict(num_heads=3), "num_heads"), (dict(num_heads=0), "num_heads"),
                       (dict(num_heads=20), "num_heads"),
                       (dict(item_embedding_dim=8, cate_embedding_dim=4), "item_embedding_dim"),
                       (dict(item_embedding_dim=K.C_MAX, cate_embedding_dim=8), "item_embedding_dim"),
                       (dict(max_seq_length=t_past), "max_seq_length %d" % t_past),
                       (dict(max_seq_length=257), "max_seq_length"),
                       (dict(user_dropout=True, dropout=[0.3, 0.3]), "dropout in SASRec's logit MLP"),
                       (dict(embedding_dropout=0.3), "embedding_dropout"), (dict(layer_sizes=[100, 64, 8]), "layer_sizes")):
        with pytest.raises(NotImplementedError, match=needle):
            SeqNet(O.hparams(golden_hparams, **kw), dims, kind="sasrec")
    hp = O.hparams(golden_hparams)
    with pytest.raises(NotImplementedError, match="precision must be 'fp32'"):
        SeqNet(hp, dims, kind="sasrec", precision="bf16")
    with pytest.raises(NotImplementedError, match="bf16 embedding tables"):
        SeqNet(hp, dims, kind="sasrec", table_dtype="bf16")
    with pytest.raises(NotImplementedError, match="precision='bf16' is not available"):
        SASRecModel(copy.deepcopy(hp), SequentialIterator, precision="bf16")
    import clsr_amd

    assert clsr_amd.SASRecModel is SASRecModel


@pytest.mark.parametrize("c", K.CASES, ids=K.case_id)
def test_kernel_cases_meet_their_conditions(c):
    """With the committed seed the reference alone meets the conditions; a float32 evaluation of the same oracle opens the
    same gates.  The kernel test's bound is four times the largest error of a float32 restatement over the summation orders
    of sasrec_oracle.fp32_bounds; torch's float32 evaluation in the given order is one of them."""
    inp, ref = K.case_data(c)
    C = c.Di + c.Dc
    assert query("clsr_sasrec_supported", c.T, c.Tmax, C, c.nb, c.nh) == 1
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


def test_case_table_reaches_what_it_says():
    assert [query("clsr_sasrec_supported", *shape) for shape, _ in K.PAST] == [0] * len(K.PAST)
    assert [query("clsr_sasrec_parts", 2, s[0], s[1], s[2], s[3]) for s, _ in K.PAST if s[4] == 1] == [0] * 8
    for C_, T_ in ((K.C_MAX, K.T_AT_MAX), (40, K.T_AT_40)):
        assert K.lds_bytes(T_, C_) <= K.BUDGET < K.lds_bytes(T_ + 1, C_)
        assert K.lds_bytes(T_, C_) == K.lds_formula(T_, C_)
    assert K.BUDGET == 160 * 1024 and K.lds_bytes(50, 40) == 4 * (9 * 50 * 41 + 50 * 21 + 2) and K.T_AT_40 >= 64
    assert K.C_MAX >= 40 and K.NB_MAX >= 4 and K.T_MAX == 256
    S, m = K.SLICE_4_8, K.MULTI
    assert query("clsr_sasrec_parts", m.Hn, m.T, m.Tmax, 8, m.nb) == K.PARTS_MAX == query("clsr_sasrec_max_parts")
    assert m.Hn == (K.PARTS_MAX + 1) * S + 3 and S == 256 // 4
    one = K.CASES[8]
    assert one.Hn == K.SLICE_9_8 + 1 and query("clsr_sasrec_parts", one.Hn, 9, 9, 8, 1) == 2 and one.Hn % K.SLICE_9_8
    mixed = K.make_inputs(K.MIXED)["lens"].tolist()
    assert 0 in mixed and K.MIXED.T in mixed and len(set(mixed)) == 5 and K.MIXED.Hn <= query("clsr_sasrec_slice", 6, 8, 1)
    assert (K.CASES[5].Di + K.CASES[5].Dc) // K.CASES[5].nh == 4 and K.CASES[5].Di + K.CASES[5].Dc == K.C_MAX
    assert K.CASES[7].nb == K.NB_MAX and K.CASES[1].T == 1 and K.POS_PAST_T.Tmax > K.POS_PAST_T.T
    assert query("clsr_sasrec_saved_floats", 3, 50, 40, 2) == 2 * 3 * 50 * 40 + 3 * 40
    # the forward's slice is the larger one: scoring needs five of the nine rows
    assert query("clsr_sasrec_lds_bytes", 50, 40, 0) == 4 * (5 * 50 * 41 + 2)
    assert math.isfinite(float(K.case_data(K.MIXED)[1]["s"].abs().max()))
