"""CPU tests of the NCF plumbing that needs no GPU: the variable inventory (TF names -- checkpoints are keyed by them --
shapes, initialiser kinds), ncf.yaml, the refusals by key name and the keys NCF never reads, the oracle's backward against a
written-out one, and -- for every parameter seed and shape the GPU tests use -- that no tower unit is undecidable."""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

import ncf_cases as K
import ncf_oracle as O
from clsr_amd.params import sibling_kind, sibling_specs, sibling_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _feed(golden_dir, name, b=0):
    g = np.load(os.path.join(golden_dir, name))
    pre = "b%d_" % b
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}


def _dims(hp):
    return dict(Vu=len(pickle.load(open(hp.user_vocab, "rb"))), Vi=len(pickle.load(open(hp.item_vocab, "rb"))),
                Vc=len(pickle.load(open(hp.cate_vocab, "rb"))))


def test_variable_inventory(golden_hparams):
    hp = O.hparams(golden_hparams, ncf_layer_sizes=[80, 40, 8])
    assert sibling_kind("NCF") == "ncf" and sibling_kind(hp.model_type) == "ncf"
    dims = dict(Vu=50, Vi=70, Vc=9)
    specs = [tuple(x) for x in sibling_specs(dims, hp, "ncf")]
    e, s = "sequential/embedding/", "sequential/fully_connected"
    assert specs == [(e + "user_embedding", (50, 16), "w"), (e + "item_embedding", (70, 32), "w"),
                     (e + "cate_embedding", (9, 8), "w"),
                     (e + "user_gmf_embedding", (50, 16), "w"), (e + "user_mlp_embedding", (50, 16), "w"),
                     (e + "item_gmf_embedding", (70, 16), "w"), (e + "item_mlp_embedding", (70, 16), "w"),
                     (s + "/weights", (32, 80), "glorot"), (s + "/biases", (80,), "zero"),
                     (s + "_1/weights", (80, 40), "glorot"), (s + "_1/biases", (40,), "zero"),
                     (s + "_2/weights", (40, 8), "glorot"), (s + "_2/biases", (8,), "zero"),
                     (s + "_3/weights", (16 + 8, 1), "glorot")]
    assert specs == [tuple(x) for x in O.param_specs(dims, hp)]
    assert dict(sibling_tables("ncf")) == dict(O.TABLES)
    assert [n for n, _, _ in specs[7:]] == O.dense_names(hp)


def test_yaml_holds_the_reference_values():
    from clsr_amd.deeprec_utils import prepare_hparams

    hp = prepare_hparams(os.path.join(ROOT, "clsr_amd", "config", "ncf.yaml"))
    want = dict(model_type="NCF", ncf_layer_sizes=[80, 40], user_embedding_dim=40, item_embedding_dim=32,
                cate_embedding_dim=8, optimizer="adam", learning_rate=0.001, embed_l2=1e-4, layer_l2=1e-4, batch_size=400,
                train_num_ngs=4, max_seq_length=50, loss="softmax", method="classification", init_method="tnormal",
                init_value=0.01, layer_sizes=[100, 64], att_fcn_layer_sizes=[80, 40], hidden_size=40, attention_size=40,
                enable_BN=True, user_dropout=False, dropout=[0.0, 0.0], epochs=50, EARLY_STOP=10, need_sample=True)
    for k, v in want.items():
        assert getattr(hp, k) == v, (k, getattr(hp, k))


def test_refusals_name_the_key_and_ignored_keys_pass(golden_hparams):
    from clsr_amd.clsr import NCFModel
    from clsr_amd.seqnet import SeqNet
    from clsr_amd.sequential_iterator import SequentialIterator

    dims = dict(Vu=10, Vi=20, Vc=5)
    wmax, lmax = K.WMAX, K.query("clsr_ncf_max_layers")
    for over, needle in ((dict(user_embedding_dim=6), "user_embedding_dim must be a positive multiple of 4"),
                         (dict(user_embedding_dim=wmax + 4), "user_embedding_dim must be a positive multiple of 4"),
                         (dict(ncf_layer_sizes=[80, 42]), "ncf_layer_sizes must be positive multiples of 4"),
                         (dict(ncf_layer_sizes=[wmax + 4]), "ncf_layer_sizes must be positive multiples of 4"),
                         (dict(ncf_layer_sizes=[]), "ncf_layer_sizes must hold 1 to %d layers" % lmax),
                         (dict(ncf_layer_sizes=[8] * (lmax + 1)), "ncf_layer_sizes must hold 1 to %d layers" % lmax),
                         (dict(train_num_ngs=K.query("clsr_ncf_max_group")), "train_num_ngs must be at most"),
                         (dict(user_embedding_dim=K.PAST_LDS[0], ncf_layer_sizes=list(K.PAST_LDS[1])), "words of LDS"),
                         (dict(loss="log_loss"), "loss must be softmax"),
                         (dict(method="regression"), "method classification"),
                         (dict(layer_l1=1e-4), "l1 / cross regularisers"),
                         (dict(cross_l2=1e-4), "l1 / cross regularisers"),
                         (dict(item_embedding_dim=30), "item / cate embedding dims")):
        hp = O.hparams(golden_hparams, **over)
        with pytest.raises(NotImplementedError, match=needle):
            SeqNet(hp, dims, kind="ncf")
    # what NCF's graph never reads: any value passes (the limits are the whole configuration check of the constructor)
    hp = O.hparams(golden_hparams, enable_BN=False, activation=["dice", "dice"], user_dropout=True, dropout=[0.3, 0.2],
                   embedding_dropout=0.1, layer_sizes=[7], att_fcn_layer_sizes=[5, 5, 5], hidden_size=None,
                   attention_size=3)
    assert SeqNet._ncf_limits(hp) == []
    assert SeqNet._ncf_limits(O.hparams(golden_hparams, user_embedding_dim=40, ncf_layer_sizes=[K.WMAX, K.LDS_AT])) == []
    with pytest.raises(NotImplementedError, match="precision='bf16' is not available"):
        NCFModel(O.hparams(golden_hparams), SequentialIterator, precision="bf16")


def test_oracle_backward_equals_the_written_out_chain():
    """autograd of ``O.tower`` against the chain rule written out (the form csrc/ncf.hip computes), float64."""
    c = K.CASES[3]
    inp, ref = K.make_inputs(c), K.reference(c)
    u, i = inp["users"].long(), inp["items"].long()
    sl = [t.double()[u if k < 2 else i] for k, t in enumerate(inp["tabs"])]
    Ws, bs, wout = [W.double() for W in inp["Ws"]], [b.double() for b in inp["bs"]], inp["wout"].double()
    t = O.tower(sl[0], sl[1], sl[2], sl[3], Ws, bs, wout)
    dl = ref["dlogit"]
    dmo = dl[:, None] * wout[None, :]
    Du = c.Du
    dz = dmo[:, Du:] * (t["act"][-1] > 0)
    pieces = []
    for j in range(len(Ws) - 1, -1, -1):
        a_in = t["act"][j - 1] if j else torch.cat([sl[1], sl[3]], -1)
        pieces = [a_in.T @ dz, dz.sum(0)] + pieces
        dz = dz @ Ws[j].T
        if j:
            dz = dz * (t["act"][j - 1] > 0)
    dblock = torch.cat([p.reshape(-1) for p in pieces] + [t["model_output"].T @ dl])
    assert float((dblock - ref["dblock"]).abs().max()) <= 1e-12
    for got, exp in zip((dmo[:, :Du] * sl[2], dz[:, :Du], dmo[:, :Du] * sl[0], dz[:, Du:]), ref["slices"]):
        assert float((got - exp).abs().max()) <= 1e-12


@pytest.mark.parametrize("c", K.CASES + K.SCORE, ids=K.case_id)
def test_kernel_cases_hold_no_undecidable_unit(c):
    ref = K.reference(c)
    assert ref["units"] == c.B * sum(c.widths)
    assert ref["undecidable"] == 0, "%d of %d units within their fp32 bound of zero: pick another seed" % (
        ref["undecidable"], ref["units"])
    if c.ids == "edge":
        inp = K.make_inputs(c)
        assert int(inp["users"].min()) == 0 and int(inp["users"].max()) == inp["tabs"][0].shape[0] - 1
        assert int(inp["items"].min()) == 0 and int(inp["items"].max()) == inp["tabs"][2].shape[0] - 1


def test_kernel_cases_reach_the_edges():
    """The tile arithmetic behind the case list, from the kernel's queries."""
    parts = lambda c: K.query("clsr_ncf_parts", c.B, c.G)
    assert [parts(c) for c in K.CASES[:4]] == [1, 1, 1, 2] and parts(K.CASES[4]) == 3
    assert parts(K.MULTI) == K.PARTS_MAX and K.MULTI.B // K.tile(K.MULTI.G) == K.PARTS_MAX + 2
    assert K.query("clsr_ncf_supported", 40, 2, K.WMAX, K.LDS_AT, 0, 0, 5) == 1
    assert K.query("clsr_ncf_supported", 40, 2, K.WMAX, K.LDS_PAST, 0, 0, 5) == 0
    assert K.query("clsr_ncf_supported", 40, 2, 80, 40, 0, 0, 5) == 1          # ncf.yaml
    assert {c.Du for c in K.CASES} >= {4, 8, 40, 44} and {len(c.widths) for c in K.CASES} == {1, 2, 3}
    assert {w for c in K.CASES for w in c.widths} >= {4, 36, 40, 80, K.WMAX}
    assert {c.G for c in K.CASES + K.SCORE} == {1, 2, 5}


GOLDEN_SHAPES = [("iterator_train_plain.npz", 0, {}), ("iterator_train_plain.npz", 1, {}), ("iterator_eval_plain.npz", 0, {})]


@pytest.mark.parametrize("name,b,over", GOLDEN_SHAPES)
def test_golden_batches_hold_no_undecidable_unit(golden_dir, golden_hparams, name, b, over):
    """The fixture of tests/test_ncf_gpu.py and tests/test_ncf_dp_gpu.py (O.FIXTURE) on the golden batches they feed."""
    hp = O.hparams(golden_hparams, **over)
    p32 = O.init_params(_dims(hp), hp, **O.FIXTURE)
    p64 = type(p32)((k, v.double()) for k, v in p32.items())
    out = O.predict(p64, O.to_torch_feed(_feed(golden_dir, name, b), dtype=torch.float64), hp, bound=True)
    assert sum(int(p.numel()) for p in out["pre"]) == out["logit"].shape[0] * sum(hp.ncf_layer_sizes)
    assert O.undecidable(out) == 0
    gates = torch.cat([(p > 0).reshape(-1) for p in out["pre"]])
    assert 0 < int(gates.sum()) < gates.numel()          # both states of the gate are exercised


def test_bias_and_output_weights_are_regularised(golden_dir, golden_hparams):
    """layer_l2 reaches the tower biases and the output weights; embed_l2 the involved item / cate rows only."""
    hp = O.hparams(golden_hparams, layer_l2=0.5, embed_l2=0.25)
    p = O.init_params(_dims(hp), hp, dtype=torch.float64, **O.FIXTURE)
    feed = O.to_torch_feed(_feed(golden_dir, "iterator_train_plain.npz", 0), dtype=torch.float64)
    ls = O.losses(p, O.forward(p, feed, hp), feed, hp)
    dense = sum(float((p[n] ** 2).sum()) / 2 for n in O.dense_names(hp))
    inv = {k: O.C._unique(torch.cat([feed[h].reshape(-1), feed[t].reshape(-1)]))
           for k, h, t in (("item", "item_history", "items"), ("cate", "item_cate_history", "cates"))}
    emb = sum(float((p[O.TABLES[k]][inv[k]] ** 2).sum()) / 2 for k in inv)
    assert abs(float(ls["regular_loss"]) - (0.5 * dense + 0.25 * emb)) < 1e-12
    assert float((p[O.fc(0) + "biases"] ** 2).sum()) > 0
    _, _, _, out = O.gradients(p, feed, hp)
    raw = out["raw_grads"]
    assert float(raw[O.EMB + "user_gmf_embedding"].abs().max()) > 0
    g = raw[O.TABLES["item"]]
    assert torch.allclose(g[inv["item"]], 0.25 * p[O.TABLES["item"]][inv["item"]], rtol=0, atol=1e-15)
    assert copy.copy(g).index_fill_(0, inv["item"], 0.0).abs().max() == 0
