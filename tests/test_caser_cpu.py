"""CPU tests of the Caser plumbing that needs no GPU: the variable inventory (TF names -- checkpoints are keyed by them --
shapes, initialiser kinds), the index conventions of the test oracle (tests/caser_oracle.py) against torch's own conv1d,
the fixture's distance from near-ties of the pooling and the ReLU gates, and the refusals, each reported by name."""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

import caser_cases as K
import caser_oracle as O
from clsr_amd.params import sibling_kind, sibling_specs


def _feed(golden_dir, name, b):
    g = np.load(os.path.join(golden_dir, name))
    pre = "b%d_" % b
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}


def _dims(hp):
    return dict(Vu=len(pickle.load(open(hp.user_vocab, "rb"))), Vi=len(pickle.load(open(hp.item_vocab, "rb"))),
                Vc=len(pickle.load(open(hp.cate_vocab, "rb"))))


def test_variable_inventory(golden_hparams):
    hp = O.hparams(golden_hparams)
    assert (hp.max_seq_length, hp.item_embedding_dim, hp.cate_embedding_dim) == (10, 32, 8)
    assert sibling_kind(hp.model_type) == "caser"
    dims = dict(Vu=50, Vi=70, Vc=9)
    specs = [tuple(x) for x in sibling_specs(dims, hp, "caser")]
    c = "sequential/caser/"
    expect = [("sequential/embedding/user_embedding", (50, 16), "w"),
              ("sequential/embedding/item_embedding", (70, 32), "w"),
              ("sequential/embedding/cate_embedding", (9, 8), "w"),
              (c + "item/vertical/conv_32/kernel", (32, 10, 16), "glorot_conv"),
              (c + "item/vertical/conv_32/bias", (16,), "zero"),
              (c + "item/horizonal/conv_1/kernel", (1, 32, 16), "glorot_conv"),
              (c + "item/horizonal/conv_1/bias", (16,), "zero"),
              (c + "item/horizonal/conv_2/kernel", (2, 32, 16), "glorot_conv"),
              (c + "item/horizonal/conv_2/bias", (16,), "zero"),
              (c + "item/horizonal/conv_3/kernel", (3, 32, 16), "glorot_conv"),
              (c + "item/horizonal/conv_3/bias", (16,), "zero"),
              (c + "cate/vertical/conv_8/kernel", (8, 10, 16), "glorot_conv"),
              (c + "cate/vertical/conv_8/bias", (16,), "zero"),
              (c + "cate/horizonal/conv_1/kernel", (1, 8, 16), "glorot_conv"),
              (c + "cate/horizonal/conv_1/bias", (16,), "zero"),
              (c + "cate/horizonal/conv_2/kernel", (2, 8, 16), "glorot_conv"),
              (c + "cate/horizonal/conv_2/bias", (16,), "zero"),
              (c + "cate/horizonal/conv_3/kernel", (3, 8, 16), "glorot_conv"),
              (c + "cate/horizonal/conv_3/bias", (16,), "zero")]
    lg = "sequential/logit_fcn/nn_part/"
    assert specs[:len(expect)] == expect
    assert specs[len(expect)][:2] == (lg + "w_nn_layer0", (2 * (16 + 3 * 16) + 40, hp.layer_sizes[0]))
    assert specs[-1][:2] == (lg + "b_nn_output", (1,))
    assert specs == [tuple(x) for x in O.param_specs(dims, hp)]
    # the yaml's widths: model_output is 1064 wide
    hp = O.hparams(golden_hparams, max_seq_length=50, n_v=128, n_h=128)
    assert dict((n, s) for n, s, _ in sibling_specs(dims, hp, "caser"))[lg + "w_nn_layer0"] == (1064, hp.layer_sizes[0])


def test_initialiser_is_glorot_uniform_over_conv_fans(golden_hparams):
    """tf.layers.conv1d's default: limit sqrt(6 / (width * (in + out))); biases zero."""
    from clsr_amd.params import init_tensor

    gen = torch.Generator().manual_seed(0)
    w = init_tensor("glorot_conv", (3, 32, 16), golden_hparams, gen)
    lim = (6.0 / (3 * (32 + 16))) ** 0.5
    assert w.shape == (3, 32, 16) and float(w.abs().max()) <= lim and float(w.abs().max()) > 0.95 * lim
    assert abs(float(w.mean())) < 0.05 * lim and abs(float(w.var()) - lim * lim / 3) < 0.1 * lim * lim / 3


def test_oracle_matches_conv1d():
    """Index conventions: the vertical kernel is [d, t, f] (conv1d over the transposed history, width Dx), a horizontal
    kernel [j, d, f] (conv1d over the history, width h, VALID), pooled with amax."""
    gen = torch.Generator().manual_seed(3)
    B, T, Dx, n = 5, 7, 4, 6
    X = torch.randn(B, T, Dx, generator=gen, dtype=torch.float64)
    Wv, bv = torch.randn(Dx, T, n, generator=gen, dtype=torch.float64), torch.randn(n, generator=gen, dtype=torch.float64)
    # TF conv1d on channels-last input [B, length, channels] with kernel [width, in, out] == torch conv1d on
    # [B, channels, length] with weight [out, in, width]
    Xt = X.transpose(1, 2)                                    # [B, length Dx, channels T]: the reference's embedding_T
    ref = torch.nn.functional.conv1d(Xt.transpose(1, 2), Wv.permute(2, 1, 0), bv)       # [B, n, 1]
    assert torch.allclose(O.vertical_pre(X, Wv, bv), ref[:, :, 0], rtol=1e-12, atol=1e-12)
    for h in (1, 2, 3, T):
        Wh, bh = torch.randn(h, Dx, n, generator=gen, dtype=torch.float64), torch.randn(n, generator=gen, dtype=torch.float64)
        ref = torch.nn.functional.conv1d(X.transpose(1, 2), Wh.permute(2, 1, 0), bh)    # [B, n, T - h + 1]
        c = O.horizontal_pre(X, Wh, bh)
        assert c.shape == (B, T - h + 1, n)
        assert torch.allclose(c, ref.transpose(1, 2), rtol=1e-12, atol=1e-12)
        assert torch.allclose(torch.relu(c.amax(1)), torch.relu(ref).amax(2), rtol=1e-12, atol=1e-12)
        pos = O.first_max(c)
        assert torch.equal(c.gather(1, pos.unsqueeze(1)).squeeze(1), c.amax(1))
    # ties: the first maximum
    c = torch.tensor([[[1.0], [3.0], [3.0], [2.0]]])
    assert O.first_max(c).tolist() == [[1]]


@pytest.mark.parametrize("L", [1, 3, 10])
def test_fixture_sits_clear_of_near_ties(golden_dir, golden_hparams, L):
    """The float32 and the float64 oracle select the same window in every pool of the golden training batch -- or windows
    with bit-identical inputs (all-padding windows) -- and open the same ReLU gates: with the committed seed and
    scale_dense no selection of the GPU tests hangs on the rounding of fp32."""
    hp = O.hparams(golden_hparams, L=L)
    feed = _feed(golden_dir, "iterator_train_sa.npz", 1)
    p32 = O.init_params(_dims(hp), hp, dtype=torch.float32, **O.FIXTURE)
    p64 = type(p32)((k, v.double()) for k, v in p32.items())
    sel, hist = {}, {}
    for tag, params, dt in (("f32", p32, torch.float32), ("f64", p64, torch.float64)):
        with torch.no_grad():
            out = O.forward(params, O.init_bn_state(params), O.to_torch_feed(feed, dtype=dt), hp, True, {})
        sel[tag], hist[tag] = O.selection(out, hp), out["hist"]
    pools = 0
    for key in ("item", "cate"):
        a, b = sel["f32"][key], sel["f64"][key]
        assert torch.equal(a["gate_v"], b["gate_v"]), key + ": vertical ReLU gates differ between float32 and float64"
        assert torch.equal(a["gate"], b["gate"]), key + ": pool ReLU gates differ between float32 and float64"
        X = hist["f32"][key]
        for r, h0, f in (a["pos"] != b["pos"]).nonzero().tolist():
            h, pa, pb = h0 + 1, int(a["pos"][r, h0, f]), int(b["pos"][r, h0, f])
            assert torch.equal(X[r, pa:pa + h], X[r, pb:pb + h]), \
                "%s row %d width %d filter %d: float32 picks window %d, float64 window %d" % (key, r, h, f, pa, pb)
        pools += a["pos"].numel()
        assert 0 < int(a["gate"].sum()) < a["gate"].numel() or L == 10    # both states of the gate are exercised
    assert pools == 2 * feed["items"].shape[0] * L * 16


def test_config_step_feed_sits_clear_of_near_ties(golden_hparams):
    """The generated feed of the training step at caser.yaml's widths and length (tests/test_caser_gpu.py): with the committed
    seed the float32 and the float64 oracle select alike, as for the golden batch above."""
    cs = K.CONFIG_STEP
    hp = O.hparams(golden_hparams, max_seq_length=cs["T"], n_v=128, n_h=128)
    feed = K.edge_feed(cs["T"], hp.train_num_ngs + 1, cs["dims"]["Vi"], cs["dims"]["Vc"], cs["lens"], cs["seed"])
    assert sorted({int(n) for n in feed["mask"].sum(1)}) == sorted(set(cs["lens"])) and 1 in cs["lens"] and 50 in cs["lens"]
    p32 = O.init_params(cs["dims"], hp, dtype=torch.float32, **O.FIXTURE)
    p64 = type(p32)((k, v.double()) for k, v in p32.items())
    sel, hist = {}, {}
    for tag, params, dt in (("f32", p32, torch.float32), ("f64", p64, torch.float64)):
        with torch.no_grad():
            out = O.forward(params, O.init_bn_state(params), O.to_torch_feed(feed, dtype=dt), hp, True, {})
        sel[tag], hist[tag] = O.selection(out, hp), out["hist"]
    for key in ("item", "cate"):
        a, b = sel["f32"][key], sel["f64"][key]
        assert torch.equal(a["gate_v"], b["gate_v"]), key + ": vertical ReLU gates differ between float32 and float64"
        assert torch.equal(a["gate"], b["gate"]), key + ": pool ReLU gates differ between float32 and float64"
        X = hist["f32"][key]
        for r, h0, f in (a["pos"] != b["pos"]).nonzero().tolist():
            h, pa, pb = h0 + 1, int(a["pos"][r, h0, f]), int(b["pos"][r, h0, f])
            assert torch.equal(X[r, pa:pa + h], X[r, pb:pb + h]), \
                "%s row %d width %d filter %d: float32 picks window %d, float64 window %d" % (key, r, h, f, pa, pb)
        assert 0 < int(a["gate"].sum()) < a["gate"].numel()


# ------------------------------------------------------------- the kernel-level reference (tests/test_caser_kernels_gpu.py)
def _as_params(blk, hp, key):
    p = {O.vname(hp, key) + "kernel": blk["Wv"], O.vname(hp, key) + "bias": blk["bv"]}
    for h0, (W, b) in enumerate(zip(blk["Wh"], blk["bh"])):
        p[O.hname(key, h0 + 1) + "kernel"], p[O.hname(key, h0 + 1) + "bias"] = W, b
    return p


def test_block_layout_roundtrip():
    """pack_block / unpack_block: the flat layout csrc/caser.hip states -- Wv [Dx][T][n_v] | bv | Wh_1 | bh_1 | ... ."""
    T, Dx, L, n_v, n_h = 5, 4, 3, 8, 4
    n = Dx * T * n_v + n_v + sum(h * Dx * n_h + n_h for h in range(1, L + 1))
    flat = torch.arange(n, dtype=torch.float64)
    blk = O.unpack_block(flat, T, Dx, L, n_v, n_h)
    assert blk["Wv"].shape == (Dx, T, n_v) and float(blk["Wv"][1, 2, 3]) == (1 * T + 2) * n_v + 3
    assert float(blk["bv"][0]) == Dx * T * n_v
    o2 = Dx * T * n_v + n_v + (Dx * n_h + n_h)                  # Wh_2 follows Wh_1 | bh_1
    assert blk["Wh"][1].shape == (2, Dx, n_h) and float(blk["Wh"][1][1, 2, 3]) == o2 + (1 * Dx + 2) * n_h + 3
    assert float(blk["bh"][2][n_h - 1]) == n - 1
    assert torch.equal(O.pack_block(blk), flat)


def test_explicit_backward_equals_autograd():
    """The written-out backward against autograd of ``O.cnn`` under (pooled * dpool).sum(), at a shape with ties (torch.amax
    splits evenly among tied positions) and closed gates."""
    import types

    c = K.Case(6, 40, 8, 4, 4, 8, 4, 3, "")
    inp = K.make_inputs(c)
    hp = types.SimpleNamespace(L=c.L, item_embedding_dim=c.Di, cate_embedding_dim=c.Dc)
    PW = c.n_v + c.L * c.n_h
    gen = torch.Generator().manual_seed(4)
    tied = 0
    for i, key in enumerate(("item", "cate")):
        X = inp["X"][key].clone().requires_grad_(True)
        blk = O.map_block(inp["blk"][key], lambda t: t.clone().requires_grad_(True))
        dpool = torch.randn(c.Hn, PW, generator=gen, dtype=torch.float64)
        pooled = O.cnn(X, key, _as_params(blk, hp, key), hp)
        (pooled * dpool).sum().backward()
        with torch.no_grad():
            mine, m = O.block_forward(X, blk)
            assert torch.equal(mine, pooled)
            dX, dblk = O.explicit_backward(X, blk, dpool, m)
        tied += sum(int(((n > 1) & g).sum()) for n, g in zip(m["n"], m["gate"]))
        assert any(int((~g).sum()) for g in m["gate"]) and int((~m["gate_v"]).sum())
        for name, got, exp in [("dX", dX, X.grad), ("dWv", dblk["Wv"], blk["Wv"].grad), ("dbv", dblk["bv"], blk["bv"].grad)] + \
                [("dWh%d" % (h + 1), dblk["Wh"][h], blk["Wh"][h].grad) for h in range(c.L)] + \
                [("dbh%d" % (h + 1), dblk["bh"][h], blk["bh"][h].grad) for h in range(c.L)]:
            assert float((got - exp).abs().max()) <= 1e-12, (key, name, float((got - exp).abs().max()))
    assert tied > 0


@pytest.mark.parametrize("c", K.CASES + [K.GATES], ids=K.case_id)
def test_kernel_cases_are_exact_in_float32_and_offer_every_pool_kind(c):
    """Guards the grid argument: the float32 and the float64 reference forward are bit-equal (values, first maxima, tie
    masks), so no near-tie allowance exists at kernel level; and the inputs hold an open pool with a single winner, an
    open pool whose tied positions span two mask words (T > 32) and a closed gate.  (The widest case at n_v = 8: the
    vertical path's exactness does not depend on the filter count.)"""
    n_v = 8 if c == K.WS_CAPPED else None
    inp = K.make_gate_inputs() if c == K.GATES else K.make_inputs(c, n_v=n_v)
    masks = {}
    for key in ("item", "cate"):
        X, blk = inp["X"][key], inp["blk"][key]
        assert float(X.abs().max()) <= 1 and torch.equal(X * 4, (X * 4).round())
        assert float(blk["Wv"].abs().max()) <= 0.5 and torch.equal(blk["Wv"] * 8, (blk["Wv"] * 8).round())
        p64, m64 = O.block_forward(X, blk)
        p32, m32 = O.block_forward(X.float(), O.map_block(blk, lambda t: t.float()))
        assert p32.dtype == torch.float32 and torch.equal(p32.double(), p64)
        assert torch.equal(m32["gate_v"], m64["gate_v"])
        for a, b in zip(m32["M"] + m32["first"] + m32["gate"], m64["M"] + m64["first"] + m64["gate"]):
            assert torch.equal(a, b)
        masks[key] = m64
    ok, found = K.conditions_hold(c, masks)
    assert ok, found


def _bar_fails(c, ref, dX, dblk, key):
    """Whether the comparator of the GPU test rejects (dX, dblk) as the result of table ``key``."""
    N = O.chain_lengths(c.Hn, c.T, c.L, c.n_v, c.n_h, 16)
    bad = [O.bar_excess(dX, ref["dX"][key], ref["SX"][key], N["dhist"])[0] > 0]
    r, S = ref["dblk"][key], ref["Sblk"][key]
    bad += [O.bar_excess(dblk["Wv"], r["Wv"], S["Wv"], N["Wv"])[0] > 0, O.bar_excess(dblk["bv"], r["bv"], S["bv"], N["bv"])[0] > 0]
    for h0 in range(c.L):
        bad += [O.bar_excess(dblk["Wh"][h0], r["Wh"][h0], S["Wh"][h0], N["Wh"][h0])[0] > 0]
    return bad


def test_comparator_is_sharp_at_the_config_shape():
    """One tied position's share removed, and one window shifted by one position: each misses the bar N * 2^-23 * S of the
    GPU test, in d hist and in the kernel gradient of its width; the unperturbed result, rounded to float32, passes."""
    c = K.CONFIG
    inp, ref = K.case_data(c)
    key = "item"
    X, blk, m = inp["X"][key], inp["blk"][key], ref["masks"][key]
    PW = c.n_v + c.L * c.n_h
    dp = inp["dpool"][:, :PW].double()
    dX, dblk = O.explicit_backward(X, blk, dp, m)
    assert not any(_bar_fails(c, ref, dX.float(), O.map_block(dblk, lambda t: t.float()), key))
    h0 = 1                                                               # width 2
    col = lambda f: c.n_v + h0 * c.n_h + f

    def perturbed(pick, change):
        M, n, gate = m["M"][h0], m["n"][h0], m["gate"][h0]
        cands = [(b, f) for b, f in (gate & pick(n)).nonzero().tolist() if float(dp[b, col(f)]) != 0.0]
        b, f = min(cands, key=lambda bf: int(n[bf[0], bf[1]]))           # (the smallest tie set: the largest share)
        s = int(O.first_max(M.double())[b, f])
        M2 = M.clone()
        change(M2, b, s, f)
        m2 = dict(m, M=[M2 if i == h0 else x for i, x in enumerate(m["M"])])     # (n stays: the share is LOST, not re-split)
        return O.explicit_backward(X, blk, dp, m2)

    def drop(M2, b, s, f):
        M2[b, s, f] = False

    def shift(M2, b, s, f):
        s2 = s + 1 if s + 1 < M2.shape[1] else s - 1
        M2[b, s, f], M2[b, s2, f] = False, True

    for pick, change in ((lambda n: n > 1, drop), (lambda n: n == 1, shift)):
        dX2, dblk2 = perturbed(pick, change)
        bad = _bar_fails(c, ref, dX2, dblk2, key)
        assert bad[0], "d hist: the perturbed reference passes"
        assert bad[3 + h0], "d Wh_2: the perturbed reference passes"


def test_refusals_are_reported_by_name(golden_hparams):
    from clsr_amd.clsr import CaserModel
    from clsr_amd.seqnet import SeqNet
    from clsr_amd.sequential_iterator import SequentialIterator

    dims = dict(Vu=10, Vi=20, Vc=5)
    for over, needle in ((dict(L=0), "L must lie in 1..max_seq_length"),
                         (dict(L=11), "L must lie in 1..max_seq_length"),
                         (dict(n_h=6), "n_h must be a positive multiple of 4"),
                         (dict(n_v=None), "L, n_v and n_h must be set"),
                         (dict(user_dropout=True, dropout=[0.3, 0.3]), "dropout in Caser's logit MLP"),
                         (dict(enable_BN=False), "enable_BN"),
                         (dict(activation=["sigmoid", "relu"]), "activation must be relu")):
        hp = O.hparams(golden_hparams, **over)
        with pytest.raises(NotImplementedError, match=needle):
            SeqNet(hp, dims, kind="caser")
    hp = O.hparams(golden_hparams)
    with pytest.raises(NotImplementedError, match="precision='bf16' is not available"):
        CaserModel(hp, SequentialIterator, precision="bf16")
    hp2 = copy.deepcopy(hp)
    hp2.user_dropout, hp2.dropout = True, [0.0, 0.0]        # dropout NOT in effect (keep 1 is the identity): no refusal
    bad = []
    SeqNet._check_dropout(hp2, bad, True)
    assert bad == [] and not SeqNet.dropout_in_effect(hp2)
