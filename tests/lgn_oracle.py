"""CPU oracle of LGN's propagation for the tests (torch, float64, autograd and an explicit backward beside it)  --  TEST
INFRASTRUCTURE ONLY.

Restatement of ``LGNModel._create_lightgcn_embed_ui`` (models/sequential/lgn.py:107-132) with node_dropout_flag False and
n_layers 2; the n_fold split is a memory measure of TensorFlow's and changes nothing:

    E_0 = the node rows;   S_k = A_hat E_k;   E_{k+1} = leaky_relu(S_k W_k + b_k)   (tf.nn.leaky_relu: slope 0.2)
    F   = (E_0 + E_1 + E_2) / 3

``backward`` is the adjoint written out, the form the kernels run (csrc/lgn.hip): with P_k = dE_{k+1} * lrelu'(E_{k+1}),
dE_k = dF / 3 + (A_hat^T P_k) W_k^T, dW_k = S_k^T P_k, db_k = column sums of P_k; lrelu' is 1 where the OUTPUT is positive and
0.2 elsewhere (an output of exactly zero included).

Bounds.  Every value is a sum of products of the inputs.  ``forward(..., bound=True)`` carries beside it the same graph
over the absolute values (|A|, |E|, |W|, |b|; the leaky ReLU replaced by the identity, which dominates it) and the number n
of additions between the inputs and the value, so that an fp32 evaluation in any order is off by at most

    SLACK * gamma_n * (the absolute-value graph),    gamma_n = n u / (1 - n u),  u = 2^-24,  SLACK = 2.

A unit whose float64 pre-activation lies within that bound of zero is UNDECIDABLE: fp32 may gate it the other way, which
changes gradients by whole terms.  tests/test_lgn_cpu.py holds that the fixtures below leave none.
"""
import numpy as np
import torch

U = 2.0 ** -24
SLACK = 2.0
SLOPE = 0.2
N_LAYERS = 2


def gamma(n):
    return n * U / (1.0 - n * U)


def dense_adjacency(indptr, indices, values, dtype=torch.float64):
    N = len(indptr) - 1
    A = torch.zeros(N, N, dtype=dtype)
    rows = np.repeat(np.arange(N), np.diff(np.asarray(indptr, dtype=np.int64)))
    A[torch.as_tensor(rows), torch.as_tensor(np.asarray(indices, dtype=np.int64))] = torch.as_tensor(np.asarray(values)).to(dtype)
    return A


def lrelu(z):
    return torch.where(z > 0, z, SLOPE * z)


def forward(A, E0, Ws, bs, bound=False):
    """-> dict(E [E_0, E_1, E_2], S [S_0, S_1], Z (pre-activations), F) and, with ``bound``, e_S, e_Z (lists) and e_F."""
    E, S, Z = [E0], [], []
    if bound:
        Aa, Ea, maxdeg, C = A.abs(), E0.abs(), int((A != 0).sum(1).max()), E0.shape[1]
        n, e_Z, e_S, n_S, Fa = 0, [], [], [], E0.abs()
    for W, b in zip(Ws, bs):
        S.append(A @ E[-1])
        Z.append(S[-1] @ W + b)
        E.append(lrelu(Z[-1]))
        if bound:
            n_S.append(n + maxdeg + 1)
            e_S.append(SLACK * gamma(n_S[-1]) * (Aa @ Ea))
            n += maxdeg + C + 3           # the row's entries, the layer's C columns, bias, slope, one to spare
            Ea = (Aa @ Ea) @ W.abs() + b.abs()
            e_Z.append(SLACK * gamma(n) * Ea)
            Fa = Fa + Ea
    out = dict(E=E, S=S, Z=Z, F=(E[0] + E[1] + E[2]) / 3.0)
    if bound:
        out.update(e_Z=e_Z, e_S=e_S, n_S=n_S, e_F=SLACK * gamma(n + 4) * Fa / 3.0, n=n)
    return out


def undecidable(out):
    return sum(int((z.abs() <= e).sum()) for z, e in zip(out["Z"], out["e_Z"]))


def backward(A, out, Ws, dF, bs=None, parts=0):
    """The explicit adjoint.  -> (dE_0, [dW_k], [db_k]); given the biases (``out`` from ``forward(bound=True)``) also the
    fp32 bounds of the three (same shapes); ``parts``: the rows of the partial-sum reduction (clsr_lgn_parts(N)), whose additions
    d W_k and d b_k also go through."""
    At, E, S, bound = A.t(), out["E"], out["S"], bs is not None
    gate = lambda y: torch.where(y > 0, torch.ones_like(y), torch.full_like(y, SLOPE))
    dE = dF / 3.0
    dW, db = [None] * N_LAYERS, [None] * N_LAYERS
    if bound:
        Ata, dEa, N, C = At.abs(), dF.abs() / 3.0, A.shape[0], dF.shape[1]
        maxdeg_t = int((At != 0).sum(1).max())
        # the absolute-value image of S_k: what forward(bound=True) carries, formed again here
        Sa, Ea = [], E[0].abs()
        for W, b in zip(Ws, bs):
            Sa.append(A.abs() @ Ea)
            Ea = Sa[-1] @ W.abs() + b.abs()
        n, e_dW, e_db = 2, [None] * N_LAYERS, [None] * N_LAYERS
    for k in range(N_LAYERS - 1, -1, -1):
        P = dE * gate(E[k + 1])
        dW[k], db[k] = S[k].t() @ P, P.sum(0)
        dE = dF / 3.0 + (At @ P) @ Ws[k].t()
        if bound:
            Pa = dEa                        # (the gate is at most 1)
            nf = out["n_S"][k]               # additions behind S_k
            e_dW[k] = SLACK * gamma(n + nf + N + parts) * (Sa[k].t() @ Pa)
            e_db[k] = SLACK * gamma(n + N + parts) * Pa.sum(0)
            n += maxdeg_t + C + 4
            dEa = dF.abs() / 3.0 + (Ata @ Pa) @ Ws[k].abs().t()
    if bound:
        return dE, dW, db, SLACK * gamma(n) * dEa, e_dW, e_db
    return dE, dW, db


def autograd(A, E0, Ws, bs, dF):
    """The same gradients from torch's autograd through ``forward``."""
    leaves = [t.detach().clone().requires_grad_(True) for t in [E0] + list(Ws) + list(bs)]
    out = forward(A, leaves[0], leaves[1:1 + N_LAYERS], leaves[1 + N_LAYERS:])
    out["F"].backward(dF)
    g = [t.grad for t in leaves]
    return g[0], g[1:1 + N_LAYERS], g[1 + N_LAYERS:]


def fixture_params(N, C, seed, e_std=0.1, w_std=0.02, b_lo=0.2, b_hi=0.4):
    """Node rows, the two layers and a cotangent as fp32 numbers.  The biases dominate the pre-activations (|S W| stays near
    e_std w_std sqrt(C)), with either sign, so that both branches of the leaky ReLU are taken and none is near zero."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    E0 = (rn(N, C) * e_std).float()
    Ws = [(rn(C, C) * w_std).float() for _ in range(N_LAYERS)]
    bs = []
    for _ in range(N_LAYERS):
        mag = b_lo + (b_hi - b_lo) * torch.rand(C, generator=g, dtype=torch.float64)
        sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0).double()
        bs.append((mag * sign).float())
    dF = rn(N, C).float()
    return E0, Ws, bs, dF


# ------------------------------------------------------------------------------------------ the model on the trunk
# Restatement of ``LGNModel`` (models/sequential/lgn.py) on the ``SequentialBaseModel`` trunk, from the unchanged blocks of
# oracle/clsr_oracle.py (``_unique``, ``_clip_factor``, ``adam_apply``, ``to_torch_feed``):
#
#   E_0 = [user_embedding ; item_embedding ++ cate_embedding[item2cate]]   (lgn.py:52-59,113; C = Di + Dc = Du)
#   F = propagate(E_0);  logit = sum_c F[users] * F[Vu + items];  pred = sigmoid(logit): LGN overrides _fcn_net (no MLP)
#   loss = group softmax + the regulariser.
# 1. The regulariser goes through the graph: when _lookup_from_embedding runs, self.item_lookup is already the propagated
#    table, so embed_l2 acts on the involved rows of F's item part (C wide, history ids included) and its gradient flows back
#    through both layers; the involved rows of the raw cate_embedding get the usual term; user_embedding rows get none;
#    W_gc_k and b_gc_k live outside the embedding scope, so layer_l2 reaches them.  History lookups reach no loss term.
# 2. Gradient types decide the clip norms: user_embedding and item_embedding enter through concat -- dense gradients, the norm
#    of the whole summed gradient, and LazyAdam is Adam for them; cate_embedding is reached through two lookups (Vi rows by
#    item2cate, the involved rows): its norm runs over those un-deduplicated slices, its touched rows under LazyAdam are
#    set(item2cate) | involved.
# 3. The graph comes from train_data by the reference's rules (clsr_amd/lgn_graph.py restates them; tests/test_lgn_cpu.py
#    holds the builder to the reference's own matrices): lines where the user changes and the last line; at a change the
#    previous line's history goes to the new line's user; item2cate[0] = 0, unseen items -> category 0.
from collections import OrderedDict  # noqa: E402
import math  # noqa: E402

from oracle import clsr_oracle as C_  # noqa: E402

EMB = C_.EMB
TABLES = OrderedDict([("user", EMB + "user_embedding"), ("item", EMB + "item_embedding"), ("cate", EMB + "cate_embedding")])
FIXTURE = dict(seed=5, scale_tables=10.0, w_std=0.02, b_lo=0.2, b_hi=0.4)
to_torch_feed = C_.to_torch_feed


def hparams(golden_hparams, **kw):
    """The golden hparams (T = 10, Di = 32, Dc = 8) as an LGN configuration: Du = 40."""
    import copy

    hp = copy.deepcopy(golden_hparams)
    for k, v in dict(dict(model_type="LGN", user_embedding_dim=40), **kw).items():
        setattr(hp, k, v)
    return hp


def dense_names():
    return ["sequential/%s_gc_%d" % (n, k) for k in range(N_LAYERS) for n in ("W", "b")]


def param_specs(dims, hp):
    Cw = hp.item_embedding_dim + hp.cate_embedding_dim
    specs = [(TABLES["user"], (dims["Vu"], hp.user_embedding_dim), "w"), (TABLES["item"], (dims["Vi"], hp.item_embedding_dim), "w"),
             (TABLES["cate"], (dims["Vc"], hp.cate_embedding_dim), "w")]
    for k in range(N_LAYERS):
        specs += [("sequential/W_gc_%d" % k, (Cw, Cw), "normal_0.01"), ("sequential/b_gc_%d" % k, (Cw,), "normal_0.01")]
    return specs


def init_params(dims, hp, seed=0, dtype=torch.float32, scale_tables=1.0, w_std=0.01, b_lo=None, b_hi=None):
    """tnormal tables (``scale_tables`` widens them), normal W_gc; b_gc normal(0.01) as the reference draws it, or -- the
    tests' fixture -- of magnitude b_lo .. b_hi with either sign, so that the biases dominate the pre-activations."""
    gen = torch.Generator().manual_seed(seed)
    params = OrderedDict()
    for name, shape, k in param_specs(dims, hp):
        if k == "w":
            params[name] = C_._tnormal(gen, shape, hp.init_value * scale_tables, dtype)
        elif len(shape) == 2 or b_lo is None:
            params[name] = (torch.randn(shape, generator=gen, dtype=torch.float64) * (w_std if len(shape) == 2 else 0.01)).to(dtype)
        else:
            mag = b_lo + (b_hi - b_lo) * torch.rand(shape, generator=gen, dtype=torch.float64)
            params[name] = (mag * torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0).double()).to(dtype)
    return params


def init_adam(params):
    return OrderedDict((k, (torch.zeros_like(v), torch.zeros_like(v))) for k, v in params.items())


def node_table(params, item2cate):
    i2c = torch.as_tensor(np.asarray(item2cate, dtype=np.int64))
    return torch.cat([params[TABLES["user"]], torch.cat([params[TABLES["item"]], params[TABLES["cate"]][i2c]], 1)], 0)


def model_forward(params, feed, hp, A, item2cate, sites=None, bound=False):
    Vu = params[TABLES["user"]].shape[0]
    i2c = torch.as_tensor(np.asarray(item2cate, dtype=np.int64))

    def site(name, idx):
        g = params[TABLES["cate"]][idx]
        if sites is not None:
            g.retain_grad()
            sites[name] = (g, idx)
        return g

    cate_rows = site("cate/lookup", i2c)
    E0 = torch.cat([params[TABLES["user"]], torch.cat([params[TABLES["item"]], cate_rows], 1)], 0)
    Ws = [params["sequential/W_gc_%d" % k] for k in range(N_LAYERS)]
    bs = [params["sequential/b_gc_%d" % k] for k in range(N_LAYERS)]
    prop = forward(A, E0, Ws, bs, bound=bound)
    F = prop["F"]
    inv_items = C_._unique(torch.cat([feed["item_history"].reshape(-1), feed["items"].reshape(-1)]))
    inv_cates = C_._unique(torch.cat([feed["item_cate_history"].reshape(-1), feed["cates"].reshape(-1)]))
    logit = (F[feed["users"]] * F[Vu + feed["items"]]).sum(-1)
    return dict(prop=prop, F=F, logit=logit, pred=torch.sigmoid(logit), inv_items=inv_items, inv_cates=inv_cates,
                involved=dict(item=F[Vu + inv_items], cate=site("cate/involved", inv_cates)))


def losses(params, out, feed, hp):
    group = hp.train_num_ngs + 1
    logits, labels = out["logit"].reshape(-1, group), feed["labels"].reshape(-1, group)
    sm = torch.softmax(logits, -1)
    data_loss = -group * torch.log(torch.where(labels == 1, sm, torch.ones_like(sm))).mean()
    l2 = lambda t: (t ** 2).sum() / 2
    reg = hp.embed_l2 * (l2(out["involved"]["item"]) + l2(out["involved"]["cate"]))
    for name, p in params.items():
        if not name.startswith(EMB):
            reg = reg + hp.layer_l2 * l2(p)
    return dict(loss=data_loss + reg, data_loss=data_loss, regular_loss=reg)


def gradients(params, feed, hp, A, item2cate):
    leaf = OrderedDict((k, v.detach().clone().requires_grad_(True)) for k, v in params.items())
    sites = {}
    out = model_forward(leaf, feed, hp, A, item2cate, sites)
    ls = losses(leaf, out, feed, hp)
    ls["loss"].backward()
    grads, norms, raw = OrderedDict(), OrderedDict(), OrderedDict()
    for name, p in leaf.items():
        gr = p.grad
        if name == TABLES["cate"]:      # the un-deduplicated slices of its two lookups
            norms[name] = math.sqrt(sum(float((g.grad.double() ** 2).sum()) for g, _ in sites.values()))
        else:                           # dense: the whole summed gradient
            norms[name] = float(gr.double().norm())
        raw[name] = gr.detach().clone()
        if hp.is_clip_norm:
            gr = gr * C_._clip_factor(norms[name] ** 2, float(hp.max_grad_norm))
        grads[name] = gr.detach()
    out["raw_grads"] = raw
    out["cate_slice_norms"] = {k: float(g.grad.double().norm()) for k, (g, _) in sites.items()}
    out["touched"] = {TABLES["user"]: torch.arange(leaf[TABLES["user"]].shape[0]), TABLES["item"]: torch.arange(leaf[TABLES["item"]].shape[0]),
                      TABLES["cate"]: C_._unique(torch.cat([sites["cate/lookup"][1], sites["cate/involved"][1]]))}
    return {k: v.detach() for k, v in ls.items()}, grads, norms, out


def train_step(params, adam, step, feed, hp, A, item2cate, lazy=False):
    ls, grads, norms, out = gradients(params, feed, hp, A, item2cate)
    new_p, new_a = C_.adam_apply(params, grads, adam, step, hp.learning_rate, lazy_rows=out["touched"] if lazy else None)
    return new_p, new_a, ls, grads, norms, out


@torch.no_grad()
def predict(params, feed, hp, A, item2cate):
    return model_forward(params, feed, hp, A, item2cate)
