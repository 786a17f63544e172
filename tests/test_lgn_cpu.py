"""LGN's graph builder (clsr_amd/lgn_graph.py) against the reference's own matrices (tests/golden/lgn_graph.npz, written by
scripts/make_golden_lgn.py from the reference's get_adj_mat / get_item2cate on tests/golden/data), and the pieces around it
that need no GPU: the transpose, the split plan of the kernels' long rows, the propagation oracle and its fixtures."""
import os
import types

import numpy as np
import pytest

from clsr_amd import lgn_graph

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "golden", "data")


def _hp(d=DATA):
    return types.SimpleNamespace(user_vocab=os.path.join(d, "user_vocab.pkl"), item_vocab=os.path.join(d, "item_vocab.pkl"),
                                 cate_vocab=os.path.join(d, "category_vocab.pkl"))


@pytest.fixture(scope="module")
def graph():
    return lgn_graph.build_graph(_hp())


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "lgn_graph.npz"))


def _dense(indptr, indices, values, ncols):
    A = np.zeros((len(indptr) - 1, ncols))
    A[np.repeat(np.arange(len(indptr) - 1), np.diff(indptr)), indices] = values
    return A


def test_builder_equals_the_reference_matrix(graph, golden):
    """Exactly: the index arrays, the float32 values, item2cate -- which includes the attribution of the previous line's
    history to the user of the line where the user changes."""
    assert graph.n_users + graph.n_items == len(golden["indptr"]) - 1 == 1184
    assert np.array_equal(graph.indptr, golden["indptr"])
    assert graph.indices.dtype == np.int32 and np.array_equal(graph.indices, golden["indices"])
    assert graph.values.dtype == np.float32 and np.array_equal(graph.values, golden["values"])
    assert graph.item2cate.dtype == np.int32 and np.array_equal(graph.item2cate, golden["item2cate"])
    assert len(graph.indices) == 9940
    deg = np.diff(graph.indptr)
    assert deg.min() == 1 and deg.max() == 75


def test_matrix_is_the_row_normalised_adjacency_with_its_diagonal(graph):
    N, Vu = graph.n_users + graph.n_items, graph.n_users
    A = _dense(graph.indptr, graph.indices, graph.values, N)
    assert (np.diag(A) > 0).all()                                   # every row holds its diagonal entry
    np.testing.assert_allclose(A.sum(1), 1.0, rtol=1e-6)           # D^-1 (A + I): rows sum to one
    pattern = A > 0
    assert np.array_equal(pattern, pattern.T) and not np.allclose(A, A.T)       # symmetric pattern, values not
    assert not pattern[:Vu, :Vu][~np.eye(Vu, dtype=bool)].any()    # bipartite: no user-user ...
    Vi = graph.n_items
    assert not pattern[Vu:, Vu:][~np.eye(Vi, dtype=bool)].any()    # ... and no item-item entries but the diagonal
    rows = np.repeat(np.arange(N), np.diff(graph.indptr))
    assert (np.diff(graph.indices)[np.diff(rows) == 0] > 0).all()   # ascending inside a row
    assert graph.item2cate[0] == 0


def test_user_change_attribution_is_the_reference_s(tmp_path):
    """Three lines, two users: the FIRST line's history goes to the SECOND user (the line where the user changes), the
    second line is never used, the last line's history goes to its own user."""
    import pickle
    d = tmp_path
    for name, voc in (("user_vocab.pkl", {"ua": 0, "ub": 1}), ("item_vocab.pkl", {"default_mid": 0, "i1": 1, "i2": 2, "i3": 3, "i4": 4}),
                      ("category_vocab.pkl", {"default_cat": 0, "c1": 1, "c2": 2})):
        with open(os.path.join(d, name), "wb") as f:
            pickle.dump(voc, f)
    with open(os.path.join(d, "train_data"), "w") as f:
        f.write("1\tua\ti4\tc2\t10\ti1\tc1\t1\n")
        f.write("1\tub\ti4\tc1\t11\ti2\tc2\t2\n")
        f.write("1\tub\ti1\tc2\t12\ti3,i2\tc1,c1\t3,4\n")
    g = lgn_graph.build_graph(_hp(str(d)))
    A = _dense(g.indptr, g.indices, g.values, 7) > 0
    edges = {(u, i) for u in range(2) for i in range(5) if A[u, 2 + i]}
    assert edges == {(1, 1), (1, 3), (1, 2)}          # ub: i1 (from ua's line), i3 and i2 (its own last line); ua: nothing
    # item2cate: i4 -> c2 and i1 -> c1 at the change; the last line: its target i1 -> c2 overrides, i3 -> c1, i2 -> c1
    assert g.item2cate.tolist() == [0, 2, 1, 1, 2]
    assert not any(n for n in os.listdir(d) if n not in ("user_vocab.pkl", "item_vocab.pkl", "category_vocab.pkl", "train_data"))


def test_transpose_is_the_transpose(graph):
    N = graph.n_users + graph.n_items
    A = _dense(graph.indptr, graph.indices, graph.values, N)
    At = _dense(graph.t_indptr, graph.t_indices, graph.t_values, N)
    assert np.array_equal(At, A.T)
    rows = np.repeat(np.arange(N), np.diff(graph.t_indptr))
    assert (np.diff(graph.t_indices)[np.diff(rows) == 0] > 0).all()
    assert graph.t_values.dtype == np.float32 and graph.t_indices.dtype == np.int32
    # a rectangular matrix with an empty row and an empty column
    indptr, indices, values = np.array([0, 2, 2, 3]), np.array([0, 3, 3], dtype=np.int32), np.array([1., 2., 3.], dtype=np.float32)
    t = lgn_graph.csr_transpose(indptr, indices, values, 4)
    assert np.array_equal(_dense(*t, 3), _dense(indptr, indices, values, 4).T)


def test_split_plan():
    indptr = np.cumsum([0, 3, 8, 0, 9, 4, 17])
    rows, off = lgn_graph.split_plan(indptr, 4)
    assert rows.tolist() == [1, 3, 5] and off.tolist() == [0, 2, 5, 10]
    assert rows.dtype == np.int32 and off.dtype == np.int32
    rows, off = lgn_graph.split_plan(indptr, 17)
    assert rows.tolist() == [] and off.tolist() == [0]


def test_builder_refuses_ids_the_vocabulary_lacks(tmp_path):
    import pickle
    for name, voc in (("user_vocab.pkl", {"ua": 0}), ("item_vocab.pkl", {"i1": 0}), ("category_vocab.pkl", {"c1": 0})):
        with open(os.path.join(tmp_path, name), "wb") as f:
            pickle.dump(voc, f)
    with open(os.path.join(tmp_path, "train_data"), "w") as f:
        f.write("1\tua\ti1\tc1\t10\ti9\tc1\t1\n")
    with pytest.raises(ValueError, match="i9"):
        lgn_graph.build_graph(_hp(str(tmp_path)))


# ------------------------------------------------------------------ the propagation oracle and its fixtures
@pytest.mark.parametrize("name", ["golden", "skewed"])
def test_oracle_agrees_with_a_dense_restatement_and_with_autograd(name):
    import torch

    import lgn_cases as K
    import lgn_oracle as O

    c = K.case(name)
    d = lambda t: t.double()
    E0, Ws, bs, dF = d(c["E0"]), [d(W) for W in c["Ws"]], [d(b) for b in c["bs"]], d(c["dF"])
    # the dense restatement: numpy, the adjacency rebuilt entry by entry, no shared code with the oracle
    g = c["graph"]
    A = np.zeros((c["N"], c["N"]))
    for r in range(c["N"]):
        for e in range(int(g.indptr[r]), int(g.indptr[r + 1])):
            A[r, g.indices[e]] = g.values[e]
    E = [E0.numpy()]
    for W, b in zip(Ws, bs):
        z = A @ E[-1] @ W.numpy() + b.numpy()
        E.append(np.where(z > 0, z, 0.2 * z))
    np.testing.assert_allclose(c["fwd"]["F"].numpy(), (E[0] + E[1] + E[2]) / 3.0, rtol=1e-12, atol=1e-14)
    # explicit backward against autograd
    dE0, dW, db = c["bwd"][:3]
    a_dE0, a_dW, a_db = O.autograd(c["A"], E0, Ws, bs, dF)
    for got, exp in [(dE0, a_dE0)] + list(zip(dW, a_dW)) + list(zip(db, a_db)):
        assert torch.allclose(got, exp, rtol=1e-11, atol=1e-13)
    # the transposed CSR is what the explicit backward multiplies with
    At = O.dense_adjacency(g.t_indptr, g.t_indices, g.t_values)
    assert torch.equal(At, c["A"].t())


@pytest.mark.parametrize("name", ["golden", "skewed"])
def test_no_pre_activation_is_undecidable(name):
    """CONDITION of the GPU comparison: on the committed fixture parameters no pre-activation of either layer lies within
    its fp32 bound of zero -- zero units, not a share -- and both branches of the leaky ReLU are taken."""
    import lgn_cases as K
    import lgn_oracle as O

    fwd = K.case(name)["fwd"]
    assert O.undecidable(fwd) == 0
    for z, e in zip(fwd["Z"], fwd["e_Z"]):
        assert float((z.abs() / e).min()) > 100.0          # (far from it: the biases dominate)
        assert 0.2 < float((z > 0).double().mean()) < 0.8


# ------------------------------------------------------------------ the model: inventory, refusals, the step fixtures
def _dims(hp):
    import pickle
    return dict(Vu=len(pickle.load(open(hp.user_vocab, "rb"))), Vi=len(pickle.load(open(hp.item_vocab, "rb"))),
                Vc=len(pickle.load(open(hp.cate_vocab, "rb"))))


def test_variable_inventory(golden_hparams):
    import lgn_oracle as O
    from clsr_amd.params import init_tensor, sibling_kind, sibling_specs, sibling_tables

    hp = O.hparams(golden_hparams)
    dims = _dims(hp)
    assert sibling_kind("LGN") == "lgn"
    specs = sibling_specs(dims, hp, "lgn")
    assert specs == O.param_specs(dims, hp)
    assert [n for n, _, _ in specs] == ["sequential/embedding/user_embedding", "sequential/embedding/item_embedding",
                                        "sequential/embedding/cate_embedding", "sequential/W_gc_0", "sequential/b_gc_0",
                                        "sequential/W_gc_1", "sequential/b_gc_1"]
    assert dict(sibling_tables("lgn"))["user"] == "sequential/embedding/user_embedding"      # trained here, unlike the siblings
    assert [s for _, s, _ in specs[3:]] == [(40, 40), (40,), (40, 40), (40,)]
    # random_normal(0.01), not truncated: some of 40 000 draws lie beyond two sigma
    import torch
    w = init_tensor("normal_0.01", (200, 200), hp, torch.Generator().manual_seed(0))
    assert abs(float(w.std()) - 0.01) < 2e-4 and float(w.abs().max()) > 0.03


def test_config_file_holds_the_reference_s_values():
    from clsr_amd.deeprec_utils import prepare_hparams
    root = os.path.dirname(HERE)
    hp = prepare_hparams(os.path.join(root, "clsr_amd", "config", "lgn.yaml"))
    assert hp.model_type == "LGN" and (hp.item_embedding_dim, hp.cate_embedding_dim, hp.user_embedding_dim) == (32, 8, 40)
    assert (hp.embed_l2, hp.layer_l2, hp.learning_rate, hp.optimizer, hp.train_num_ngs) == (1e-4, 1e-4, 1e-3, "adam", 4)


@pytest.mark.parametrize("over, word", [
    (dict(user_embedding_dim=16), "user_embedding_dim must equal item_embedding_dim \\+ cate_embedding_dim"),
    (dict(item_embedding_dim=30, user_embedding_dim=38), "item_embedding_dim and cate_embedding_dim must be positive multiples of 4"),
    (dict(item_embedding_dim=128, user_embedding_dim=136), "at most 128 together"),
    (dict(optimizer="sgd"), "optimizer must be adam or lazyadam"),
    (dict(embedding_dropout=0.3), "embedding_dropout must be 0"),
    (dict(embed_l1=0.1), "l1 / cross regularisers"),
])
def test_refusals_by_key_name(golden_hparams, over, word):
    """Raised while the net is built, before any device work (the limits come first in the constructor)."""
    import lgn_cases as K
    import lgn_oracle as O
    from clsr_amd.seqnet import SeqNet

    hp = O.hparams(golden_hparams, **over)
    with pytest.raises(NotImplementedError, match=word):
        SeqNet(hp, _dims(hp), kind="lgn", device="cpu", graph=K.golden_model_graph())


def test_precision_and_table_formats_are_refused(golden_hparams):
    import lgn_cases as K
    import lgn_oracle as O
    from clsr_amd.seqnet import SeqNet

    hp = O.hparams(golden_hparams)
    with pytest.raises(NotImplementedError, match="precision must be 'fp32'"):
        SeqNet(hp, _dims(hp), kind="lgn", device="cpu", graph=K.golden_model_graph(), precision="bf16")
    with pytest.raises(NotImplementedError, match="bf16 embedding tables"):
        SeqNet(hp, _dims(hp), kind="lgn", device="cpu", graph=K.golden_model_graph(), table_dtype="bf16")
    # keys LGN never reads: any value is accepted as far as the limits go
    hp = O.hparams(golden_hparams, layer_sizes=[7], activation=["sigmoid"], enable_BN=False, user_dropout=True, dropout=[0.5],
                   hidden_size=3, attention_size=5)
    assert SeqNet._lgn_limits(types.SimpleNamespace(precision="fp32"), hp) == []


def test_model_fixture_leaves_no_unit_undecidable(golden_hparams, golden_dir):
    """CONDITION of tests/test_lgn_gpu.py: with the committed fixture parameters, before and after the oracle's step, on both
    graphs, no pre-activation lies within its fp32 bound of zero -- zero units, not a share."""
    import torch

    import lgn_cases as K
    import lgn_oracle as O

    hp = O.hparams(golden_hparams)
    dims = _dims(hp)
    g = np.load(os.path.join(golden_dir, "iterator_train_plain.npz"))
    feed = O.to_torch_feed({k[3:]: g[k] for k in g.files if k.startswith("b0_")}, dtype=torch.float64)
    for graph, dims_g in ((K.golden_model_graph(), dims), (K.skewed_model_graph(**K.skewed_dims(dims)), K.skewed_dims(dims))):
        p32 = O.init_params(dims_g, hp, **O.FIXTURE)
        params = type(p32)((k, v.double()) for k, v in p32.items())
        A = O.dense_adjacency(graph.indptr, graph.indices, graph.values)
        new_p = O.train_step(params, O.init_adam(params), 1, feed, hp, A, graph.item2cate)[0]
        for p in (params, new_p):
            prop = O.model_forward(p, feed, hp, A, graph.item2cate, bound=True)["prop"]
            assert O.undecidable(prop) == 0
            assert min(float((z.abs() / e).min()) for z, e in zip(prop["Z"], prop["e_Z"])) > 100.0
