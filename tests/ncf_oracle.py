"""CPU oracle of NCF for the tests (torch, float64 by default, autograd)  --  TEST INFRASTRUCTURE ONLY.

Restatement of ``NCFModel`` (models/sequential/ncf.py) on the ``SequentialBaseModel`` trunk, from the unchanged blocks of
oracle/clsr_oracle.py (``_unique``, ``_clip_factor``, ``adam_apply``, ``init_adam``, ``to_torch_feed``, initialisers):

  four tables [V, user_embedding_dim] beside the trunk's, looked up by ``users`` / ``items``, one slice per feed line
  gmf = user_gmf * item_gmf;  mlp = relu tower over user_mlp ++ item_mlp (weights + bias per layer, no batch-norm)
  model_output = gmf ++ mlp;  logit = model_output . w (no bias, no activation): NCF overrides ``_fcn_net``
  loss = group softmax + layer_l2 over EVERY non-embedding variable (biases included) + embed_l2 over the involved rows
  of item_embedding / cate_embedding (which therefore get a regulariser gradient and no data gradient)

Next to every forward value travels a PROPAGATED fp32 bound (``tower(..., bound=True)``): a value computed as a sum of K
terms in fp32, in any order, from inputs that are off by e_in, is off by at most |W|^T e_in + K 2^-23 |W|^T |a| -- K 2^-23 is
twice the any-order summation bound (K - 1) 2^-24 plus the products' roundings, so no further factor is needed.  ReLU is
1-Lipschitz (the bound passes through), the GMF product is one term.  A tower unit whose float64 pre-activation lies
within its own bound of zero is UNDECIDABLE: fp32 may gate it the other way, which changes gradients by whole terms.
"""
import math
from collections import OrderedDict

import torch

from oracle import clsr_oracle as C

EMB = C.EMB
EPS = 2.0 ** -23
TABLES = OrderedDict([("item", EMB + "item_embedding"), ("cate", EMB + "cate_embedding"),
                      ("user_gmf", EMB + "user_gmf_embedding"), ("user_mlp", EMB + "user_mlp_embedding"),
                      ("item_gmf", EMB + "item_gmf_embedding"), ("item_mlp", EMB + "item_mlp_embedding")])
NCF_KEYS = ("user_gmf", "user_mlp", "item_gmf", "item_mlp")
# parameters of the tests' fixture: tests/test_ncf_cpu.py shows that with them no tower unit of the golden batches is
# undecidable
FIXTURE = dict(seed=4, scale_dense=8.0, bias_std=0.05)


def hparams(golden_hparams, **kw):
    """The golden hparams (T = 10, Di = 32, Dc = 8) as an NCF configuration: Du = 16, tower [80, 40] unless overridden."""
    import copy

    hp = copy.deepcopy(golden_hparams)
    for k, v in dict(dict(model_type="NCF", user_embedding_dim=16, ncf_layer_sizes=[80, 40]), **kw).items():
        setattr(hp, k, v)
    return hp


def fc(i):
    """TF 1.15 numbers tf.contrib.layers.fully_connected's default scope under "sequential" (name_scope('ncf') does not
    reach variable names); unpinned like every other name until the TF 1.15 pin is run."""
    return "sequential/fully_connected" + ("" if i == 0 else "_%d" % i) + "/"


def dense_names(hp):
    n = len(hp.ncf_layer_sizes)
    return [fc(i) + s for i in range(n) for s in ("weights", "biases")] + [fc(n) + "weights"]


def param_specs(dims, hp):
    Vu, Vi, Vc = dims["Vu"], dims["Vi"], dims["Vc"]
    Di, Dc, Du = hp.item_embedding_dim, hp.cate_embedding_dim, hp.user_embedding_dim
    specs = [(EMB + "user_embedding", (Vu, Du), "w"), (TABLES["item"], (Vi, Di), "w"), (TABLES["cate"], (Vc, Dc), "w")]
    specs += [(TABLES[k], (Vu if k.startswith("user") else Vi, Du), "w") for k in NCF_KEYS]
    last = 2 * Du
    for i, n in enumerate(hp.ncf_layer_sizes):
        specs += [(fc(i) + "weights", (last, int(n)), "glorot"), (fc(i) + "biases", (int(n),), "zero")]
        last = int(n)
    specs.append((fc(len(hp.ncf_layer_sizes)) + "weights", (Du + last, 1), "glorot"))
    return specs


def init_params(dims, hp, seed=0, dtype=torch.float32, scale_dense=1.0, bias_std=0.0):
    """tnormal tables (``scale_dense`` widens them), Xavier-uniform weights; ``bias_std`` > 0 draws the biases instead of
    leaving them at zero, so that a test holds the bias path to non-trivial values."""
    gen = torch.Generator().manual_seed(seed)
    params = OrderedDict()
    for name, shape, k in param_specs(dims, hp):
        if k == "w":
            params[name] = C._tnormal(gen, shape, hp.init_value * scale_dense, dtype)
        elif k == "glorot":
            params[name] = C._glorot(gen, shape, dtype)
        elif bias_std > 0:
            params[name] = (torch.randn(shape, generator=gen, dtype=torch.float64) * bias_std).to(dtype)
        else:
            params[name] = torch.zeros(shape, dtype=dtype)
    return params


to_torch_feed = C.to_torch_feed
init_adam = C.init_adam


def tower(ug, um, ig, im, Ws, bs, wout, bound=False):
    """The graph between the four gathered slices [B, Du] and the logit [B].  -> dict(gmf, pre (list), act (list),
    model_output, logit) and, with ``bound``, e_pre (list), e_model_output, e_logit: the propagated fp32 bounds."""
    gmf = ug * ig
    a = torch.cat([um, im], -1)
    out = dict(gmf=gmf, pre=[], act=[])
    if bound:
        e = torch.zeros_like(a)                 # table values are fp32 numbers: exact inputs
        out["e_pre"] = []
    for W, b in zip(Ws, bs):
        pre = a @ W + b
        if bound:
            K = W.shape[0] + 1                  # (the bias is one more term)
            e = e @ W.abs() + K * EPS * (a.abs() @ W.abs() + b.abs())
            out["e_pre"].append(e)
        a = torch.relu(pre)
        out["pre"].append(pre)
        out["act"].append(a)
    mo = torch.cat([gmf, a], -1)
    w = wout.reshape(-1)
    out.update(model_output=mo, logit=mo @ w)
    if bound:
        e_mo = torch.cat([EPS * gmf.abs(), e], -1)
        out.update(e_model_output=e_mo, e_logit=e_mo @ w.abs() + mo.shape[1] * EPS * (mo.abs() @ w.abs()))
    return out


def undecidable(t):
    """Number of tower units of a ``tower(..., bound=True)`` result whose pre-activation lies within its bound of zero."""
    return sum(int((p.abs() <= e).sum()) for p, e in zip(t["pre"], t["e_pre"]))


def _dense(params, hp):
    n = len(hp.ncf_layer_sizes)
    return ([params[fc(i) + "weights"] for i in range(n)], [params[fc(i) + "biases"] for i in range(n)],
            params[fc(n) + "weights"])


def forward(params, feed, hp, sites=None, bound=False):
    users, items, cates = feed["users"], feed["items"], feed["cates"]
    ih, ch = feed["item_history"], feed["item_cate_history"]

    def site(name, key, idx):
        g = params[TABLES[key]][idx]
        if sites is not None:
            if g.requires_grad:
                g.retain_grad()
            sites[name] = (g, idx)
        return g

    inv_item = site("item/involved", "item", C._unique(torch.cat([ih.reshape(-1), items.reshape(-1)])))
    inv_cate = site("cate/involved", "cate", C._unique(torch.cat([ch.reshape(-1), cates.reshape(-1)])))
    sl = [site(k + "/lookup", k, users if k.startswith("user") else items) for k in NCF_KEYS]
    Ws, bs, wout = _dense(params, hp)
    out = tower(sl[0], sl[1], sl[2], sl[3], Ws, bs, wout, bound=bound)
    out.update(pred=torch.sigmoid(out["logit"]), involved=dict(item=inv_item, cate=inv_cate))
    return out


def losses(params, out, feed, hp):
    """``BaseModel._get_loss``: softmax data loss + L2 of the involved item / cate rows and of every non-embedding variable."""
    group = hp.train_num_ngs + 1
    logits = out["logit"].reshape(-1, group)
    labels = feed["labels"].reshape(-1, group)
    sm = torch.softmax(logits, -1)
    data_loss = -group * torch.log(torch.where(labels == 1, sm, torch.ones_like(sm))).mean()
    l2 = lambda t: (t ** 2).sum() / 2
    reg = out["logit"].new_zeros(())
    for k in ("item", "cate"):
        reg = reg + hp.embed_l2 * l2(out["involved"][k])
    for name, p in params.items():
        if not name.startswith(EMB):
            reg = reg + hp.layer_l2 * l2(p)
    return dict(loss=data_loss + reg, data_loss=data_loss, regular_loss=reg)


def gradients(params, feed, hp):
    """Loss, per-variable gradients clipped by the reference's per-site norms (a table's norm is that of the un-merged
    IndexedSlices: every lookup site's slices, duplicate ids not summed first), the norms, the forward outputs."""
    leaf = OrderedDict((k, v.detach().clone().requires_grad_(not k.endswith("/user_embedding")))
                       for k, v in params.items())
    sites = {}
    out = forward(leaf, feed, hp, sites)
    ls = losses(leaf, out, feed, hp)
    ls["loss"].backward()
    grads, norms, raw = OrderedDict(), OrderedDict(), OrderedDict()
    tables = set(TABLES.values())
    for name, p in leaf.items():
        if name.endswith("/user_embedding"):
            continue
        if name in tables:
            key = [k for k, v in TABLES.items() if v == name][0]
            sumsq = sum(float((g.grad.double() ** 2).sum()) for sname, (g, _) in sites.items()
                        if sname.startswith(key + "/") and g.grad is not None)
            norms[name] = math.sqrt(sumsq)
            gr = p.grad if p.grad is not None else torch.zeros_like(p)
        else:
            gr = p.grad
            norms[name] = float(gr.double().norm())
        raw[name] = gr.detach().clone()
        if hp.is_clip_norm:
            gr = gr * C._clip_factor(norms[name] ** 2, float(hp.max_grad_norm))
        grads[name] = gr.detach()
    out["raw_grads"] = raw
    out["touched"] = {TABLES[k]: C._unique(sites[k + ("/involved" if k in ("item", "cate") else "/lookup")][1])
                      for k in TABLES}
    return {k: v.detach() for k, v in ls.items()}, grads, norms, out


def train_step(params, adam, step, feed, hp, lazy=False):
    """One ``train`` call: forward, backward, per-variable clip, Adam (``lazy``: LazyAdam -- a table's untouched rows keep
    their values and moments,
    by the shared ``adam_apply(lazy_rows=...)``)."""
    ls, grads, norms, out = gradients(params, feed, hp)
    new_p, new_a = C.adam_apply(params, grads, adam, step, hp.learning_rate, lazy_rows=out["touched"] if lazy else None)
    return new_p, new_a, ls, grads, norms, out


@torch.no_grad()
def predict(params, feed, hp, bound=False):
    return forward(params, feed, hp, bound=bound)
