"""NextItNet without a GPU: the oracle's pieces against torch's own operators, its row order against a literal restatement
of the reference's reshape chain, the iterator against the fixtures captured from the reference's
(scripts/make_golden_nextitnet.py), the variable inventory, the refusals by key name, and the conditions that the kernel
cases' comparisons rest on (tests/nextitnet_cases.py), which pins their seeds."""
import copy
import os
import random

import numpy as np
import pytest
import torch

import nextitnet_cases as K
import nextitnet_oracle as O
from clsr_amd.ops import query
from clsr_amd.params import init_tensor, sibling_kind, sibling_specs


def _golden(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name))
    return {k[3:]: g[k] for k in g.files if k.startswith("b0_")}


@pytest.mark.parametrize("k,d,T", [(3, 1, 9), (3, 4, 9), (3, 64, 9), (1, 3, 5), (8, 1, 12), (2, 5, 1)])
def test_causal_conv_equals_conv1d(k, d, T):
    gen = torch.Generator().manual_seed(k * 100 + d)
    a = torch.randn(3, T, 6, generator=gen, dtype=torch.float64)
    W = torch.randn(k, 6, 4, generator=gen, dtype=torch.float64)
    b = torch.randn(4, generator=gen, dtype=torch.float64)
    padded = torch.nn.functional.pad(a.transpose(1, 2), ((k - 1) * d, 0))
    exp = torch.nn.functional.conv1d(padded, W.permute(2, 1, 0), b, dilation=d).transpose(1, 2)
    got = O.causal_conv(a, W, b, d)
    assert got.shape == exp.shape == (3, T, 4)
    assert float((got - exp).abs().max()) < 1e-13
    # tap j of position t reads position t - (k - 1 - j) d: the last tap is the current position
    assert O.taps(k, d, T)[-1] == (k - 1, 0)


def test_layer_norm_equals_torch():
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(4, 7, 12, generator=gen, dtype=torch.float64)
    g, b = torch.randn(12, generator=gen, dtype=torch.float64), torch.randn(12, generator=gen, dtype=torch.float64)
    y, xhat, rstd, var = O.layer_norm(x, g, b)
    assert float((y - torch.layer_norm(x, (12,), g, b, eps=1e-8)).abs().max()) < 1e-13
    assert float((var - x.var(-1, unbiased=False, keepdim=True)).abs().max()) < 1e-14
    # eps sits inside the root: a constant row gives exactly beta
    y0 = O.layer_norm(torch.full((1, 12), 0.625, dtype=torch.float64), g, b)[0]
    assert torch.equal(y0[0], b)


def test_row_order_equals_the_literal_chain():
    gen = torch.Generator().manual_seed(9)
    Hn, G, T, C = 3, 5, 4, 6
    xL = torch.randn(Hn, T, C, generator=gen, dtype=torch.float64)
    target = torch.randn(Hn * G, T, C, generator=gen, dtype=torch.float64)
    labels = torch.randn(Hn * G, T, generator=gen, dtype=torch.float64)
    mo = O.training_rows(xL, target, G)
    assert torch.equal(mo, O.literal_training_output(xL, target, G, T))
    lt = O.transpose_labels(labels, G, T)
    assert torch.equal(lt, labels.reshape(-1, G, T).transpose(2, 1).reshape(-1))
    for h, t, g in ((0, 0, 0), (1, 2, 3), (2, 3, 4)):
        r = (h * T + t) * G + g
        assert torch.equal(mo[r], torch.cat([xL[h, t], target[h * G + g, t]])) and lt[r] == labels[h * G + g, t]


def _iterator(golden_hparams):
    from clsr_amd.sequential_iterator import NextItNetIterator

    return NextItNetIterator(O.hparams(golden_hparams))


def test_iterator_equals_the_reference_fixtures(golden_dir, golden_hparams):
    it = _iterator(golden_hparams)
    d = os.path.join(golden_dir, "data")
    for name, infile, ngs in (("iterator_train_nextitnet.npz", "train_data", 4), ("iterator_eval_nextitnet.npz", "valid_data", 0)):
        exp = _golden(golden_dir, name)
        random.seed(1234)
        feed = next(f for f in it.load_data_from_file(os.path.join(d, infile), batch_num_ngs=ngs, min_seq_length=1) if f)
        assert set(exp) <= set(feed)
        for k, v in exp.items():
            got = np.asarray(feed[k])
            assert got.shape == v.shape and got.dtype == v.dtype, (name, k, got.shape, v.shape, got.dtype, v.dtype)
            assert np.array_equal(got, v), (name, k)
    tr = _golden(golden_dir, "iterator_train_nextitnet.npz")
    assert tr["items"].shape == tr["labels"].shape == (320, 10)
    # left-padded: the real steps are the last ones; row 0 of a group is the history one step on
    m = tr["mask"]
    assert np.all(np.diff(m, axis=1) >= 0) and np.all(m[:, -1] == 1) and m.min() == 0
    assert np.array_equal(tr["items"][::5, :-1], tr["item_history"][::5, 1:])
    assert np.all(tr["labels"][::5] == 1) and tr["labels"].sum() == 64 * 10
    # a negative never equals the positive of its position
    pos = np.repeat(tr["items"][::5], 4, axis=0)
    neg = tr["items"].reshape(64, 5, 10)[:, 1:].reshape(-1, 10)
    assert not np.any(pos == neg)


def test_a_batch_of_four_instances_is_dropped(golden_dir, golden_hparams):
    it = _iterator(golden_hparams)
    lines = it.parse_file(os.path.join(golden_dir, "data", "train_data"))[:5]
    assert it._convert_chunk(lines[:4], 4) is None
    assert it._convert_chunk(lines, 4)["items"].shape == (25, 10)
    assert it._convert_chunk(lines[:4], 0)["items"].shape == (4, 1)


def test_variable_inventory(golden_hparams):
    hp = O.hparams(golden_hparams, dilations=[1, 4], kernel_size=3)
    assert sibling_kind(hp.model_type) == "nextitnet"
    dims = dict(Vu=7, Vi=11, Vc=5)
    specs = sibling_specs(dims, hp, "nextitnet")
    assert [(n, tuple(s)) for n, s, _ in specs] == [(n, tuple(s)) for n, s, _ in O.param_specs(dims, hp)]
    b = "sequential/nextitnet/nextitnet_residual_block_one_decoder_layer_1_4/"
    names = [n for n, _, _ in specs if n.startswith(b)]
    assert names == [b + s for s in ("layer_norm1/beta", "layer_norm1/gamma", "conv1d_1/weight", "conv1d_1/bias",
                                     "layer_norm2/beta", "layer_norm2/gamma", "dilated_conv/weight", "dilated_conv/bias",
                                     "layer_norm3/beta", "layer_norm3/gamma", "conv1d_2/weight", "conv1d_2/bias")]
    shapes = {n[len(b):]: tuple(s) for n, s, _ in specs if n.startswith(b)}
    assert shapes["conv1d_1/weight"] == (1, 1, 40, 20) and shapes["dilated_conv/weight"] == (1, 3, 20, 20)
    assert shapes["conv1d_2/weight"] == (1, 1, 20, 40) and shapes["layer_norm2/gamma"] == (20,)
    kinds = {n[len(b):]: k for n, _, k in specs if n.startswith(b)}
    assert kinds["conv1d_2/weight"] == "tnormal_0.02" and kinds["layer_norm3/gamma"] == "one" and kinds["conv1d_1/bias"] == "zero"
    w = init_tensor("tnormal_0.02", (1, 3, 20, 20), hp, torch.Generator().manual_seed(0))
    assert float(w.abs().max()) <= 0.04 and 0.015 < float(w.std()) < 0.02
    n = sum(int(np.prod(s)) for nme, s, _ in specs if nme.startswith("sequential/nextitnet/"))
    assert n == query("clsr_nextitnet_param_floats", 40, 3, 2)
    # the flat layout of the kernels is the creation order
    blocks = O.blocks_of(O.init_params(dims, hp, seed=1, perturb=0.1), hp)
    back = O.unpack_blocks(O.pack_blocks(blocks), 40, 3, 2)
    assert all(torch.equal(back[i][k], blocks[i][k]) for i in range(2) for k in O.BLOCK_KEYS)


def test_refusals_are_reported_by_name(golden_hparams):
    from clsr_amd.clsr import NextItNetModel
    from clsr_amd.seqnet import SeqNet
    from clsr_amd.sequential_iterator import NextItNetIterator

    dims = dict(Vu=7, Vi=11, Vc=5)
    t_past = K.T_AT_40 + 1
    for kw, needle in ((dict(dilations=[]), "dilations"), (dict(dilations=[1] * 17), "dilations"),
                       (dict(dilations=[1, 0]), "dilations"), (dict(dilations=None), "dilations and kernel_size"),
                       (dict(kernel_size=9), "kernel_size"), (dict(kernel_size=0), "kernel_size"),
                       (dict(item_embedding_dim=8, cate_embedding_dim=4), "item_embedding_dim"),
                       (dict(item_embedding_dim=128, cate_embedding_dim=8), "item_embedding_dim"),
                       (dict(max_seq_length=t_past), "max_seq_length %d" % t_past),
                       (dict(max_seq_length=257), "max_seq_length"), (dict(train_num_ngs=0), "train_num_ngs"),
                       (dict(user_dropout=True, dropout=[0.3, 0.3]), "dropout in NextItNet's logit MLP"),
                       (dict(layer_sizes=[100, 64, 8]), "layer_sizes")):
        with pytest.raises(NotImplementedError, match=needle):
            SeqNet(O.hparams(golden_hparams, **kw), dims, kind="nextitnet")
    hp = O.hparams(golden_hparams)
    with pytest.raises(NotImplementedError, match="precision must be 'fp32'"):
        SeqNet(hp, dims, kind="nextitnet", precision="bf16")
    with pytest.raises(NotImplementedError, match="bf16 embedding tables"):
        SeqNet(hp, dims, kind="nextitnet", table_dtype="bf16")
    with pytest.raises(NotImplementedError, match="precision='bf16' is not available"):
        NextItNetModel(copy.deepcopy(hp), NextItNetIterator, precision="bf16")


def test_explicit_backward_equals_autograd():
    c = K.CASES[2]
    inp = K.make_inputs(c)
    blocks = [{k: v.double().requires_grad_(True) for k, v in p.items()} for p in inp["blocks"]]
    x = inp["x"].double().requires_grad_(True)
    xL, _ = O.stack_forward(x, blocks, c.dilations)
    (xL * inp["dout"].double()).sum().backward()
    ref = K.case_data(c)[1]
    assert float((x.grad - ref["dx"]).abs().max()) < 1e-12
    for key in O.BLOCK_KEYS:
        assert float((blocks[0][key].grad - ref["grads"][0][key]).abs().max()) < 1e-12, key


@pytest.mark.parametrize("c", K.CASES, ids=K.case_id)
def test_kernel_cases_meet_their_conditions(c):
    """With the committed seed the reference alone meets the conditions; a float32 evaluation of the same oracle opens the
    same gates.  The kernel test's bound is four times the largest error of a float32 restatement over nine summation
    orders (nextitnet_oracle.fp32_bounds); torch's float32 evaluation in the given order is one of them."""
    inp, ref = K.case_data(c)
    assert query("clsr_nextitnet_supported", c.T, c.Di + c.Dc, c.k, len(c.dilations), max(c.dilations)) == 1
    assert ref["min_var"] >= 1e-4, ref["min_var"]
    assert ref["min_pre"] > 2.0 ** -16, ref["min_pre"]
    r32 = K.reference(c, inp, torch.float32)
    assert all(torch.equal(a, b) for a, b in zip(ref["gates"], r32["gates"]))
    print("float32 restatement, |err| / (N eps S): " + " ".join("%.4f" % m for m in ref["fp32_measured"]))
    assert all(0 < m < 1 for m in ref["fp32_measured"])
    assert float(((r32["xL"].double() - ref["xL"]).abs() - ref["e_xL"]).max()) <= 0
    for l in range(1, len(c.dilations)):
        err = (r32["caches"][l]["x"].double() - ref["caches"][l]["x"]).abs()
        assert float((err - ref["e_inputs"][l]).max()) <= 0, l
    assert float(inp["x"][0, 0].abs().max()) > 0          # (the padded steps' row is not zero)


def test_case_table_reaches_what_it_says():
    live = K.case_data(K.LIVE_TAP)[1]
    assert float(live["grads"][0]["Wd"][:2].abs().max()) == 0.0 and float(live["grads"][0]["Wd"][2].abs().max()) > 0
    one = K.CASES[2]
    assert (one.k - 1) * one.dilations[0] == one.T - 1
    S, m = K.SLICE_4_8, K.MULTI
    assert query("clsr_nextitnet_parts", m.Hn, m.T, 8, m.k, 2) == K.PARTS_MAX and m.Hn == (K.PARTS_MAX + 1) * S + 3
    assert [query("clsr_nextitnet_supported", *shape, 1) for shape, _ in K.PAST] == [0] * len(K.PAST)
    assert K.lds_bytes(K.T_AT_128, 128) <= K.BUDGET < K.lds_bytes(K.T_AT_128 + 1, 128)
    assert K.lds_bytes(K.T_AT_40, 40) <= K.BUDGET < K.lds_bytes(K.T_AT_40 + 1, 40)
    assert K.BUDGET == 65536 and K.lds_bytes(50, 40) == 4 * (50 * (2 * 41 + 3 * 21) + 8 * 40)


def test_gate_case_is_what_it_says():
    c, inp = K.GATE, K.make_gate_inputs()
    ref = K.reference(c, inp)
    c0 = ref["caches"][0]
    assert float(c0["v1"][0, 1]) == 0.0 and torch.equal(c0["y1"][0, 1], inp["blocks"][0]["be1"].double())
    assert float(c0["y1"][0, 1, 2]) == 0.0 and not bool(c0["y1"][0, 1, 2] > 0) and float(c0["a1"][0, 1, 2]) == 0.0
    assert bool(c0["y1"][0, 1, 0] > 0) and not bool(c0["y1"][0, 1, 1] > 0)
    r32 = K.reference(c, inp, torch.float32)
    assert float(r32["caches"][0]["v1"][0, 1]) == 0.0 and all(torch.equal(a, b) for a, b in zip(ref["gates"], r32["gates"]))
    # every element that is NOT designed meets the cases' conditions: the other rows' variances, the other ReLU inputs
    designed_v = torch.zeros_like(c0["v1"], dtype=torch.bool)
    designed_v[0, 1] = True
    assert float(c0["v1"][~designed_v].min()) >= 1e-4 and float(c0["v2"].min()) >= 1e-4 and float(c0["v3"].min()) >= 1e-4
    designed_y = torch.zeros_like(c0["y1"], dtype=torch.bool)
    designed_y[0, 1, 2] = True
    assert float(c0["y1"][~designed_y].abs().min()) > 2.0 ** -16
    assert float(c0["y2"].abs().min()) > 2.0 ** -16 and float(c0["y3"].abs().min()) > 2.0 ** -16
    assert float(((r32["xL"].double() - ref["xL"]).abs() - ref["e_xL"]).max()) <= 0
    # the forward cannot see the SIZE of eps at the variance-0 row (beta for any eps), the backward does: d x there is
    # rstd = eps^-1/2 = 1e4 times a combination of O(1) terms, so an eps of 1e-6 or 1e-10 misses d hist by a factor of 10
    assert float(c0["r1"][0, 1]) == 1e4 and float(ref["dx"][0, 1].abs().max()) > 1e3
    assert float(ref["dx"][0, 1].abs().max()) > 10 * float(ref["dx"][1].abs().max())
    # an open gate at the zero would show: d beta1[2] changes by a whole term
    open_gate = copy.deepcopy(inp)
    open_gate["blocks"][0]["be1"][2] = 2.0 ** -20
    other = K.reference(c, open_gate)
    diff = float((other["grads"][0]["be1"][2] - ref["grads"][0]["be1"][2]).abs())
    assert diff > 2e-3 * float(ref["grads"][0]["be1"].abs().max()) * 10, diff
