"""CPU oracle of Caser for the tests (torch, float64 by default, autograd)  --  TEST INFRASTRUCTURE ONLY.

Restatement of ``CaserModel._build_seq_graph`` (models/sequential/caser.py:37-106) on the ``SequentialBaseModel`` trunk
of oracle/sibling_oracle.py (embeddings, involved rows, logit MLP, losses) and the building blocks of
oracle/clsr_oracle.py (``fcn_net``, ``_unique``, ``_clip_factor``, ``adam_apply``, initialisers).  Per table X [B, T, Dx]:

  vertical    conv1d over the TRANSPOSED history [B, Dx, T] (length Dx, channels T), kernel width Dx -> one output step:
              out_v[b, f] = relu(bv[f] + sum_{d, t} X[b, t, d] Wv[d, t, f])              kernel [Dx, T, n_v]
  horizonal   for h = 1..L: c_h[b, t, f] = bh[f] + sum_{j < h, d} X[b, t + j, d] Wh[j, d, f]  (VALID), kernel [h, Dx, n_h];
              out_h = max_t relu(c_h) = relu(max_t c_h)

No mask: padded steps (table row 0) take part.  The pooling is ``torch.amax``, which like TensorFlow splits the gradient
evenly among tied positions.  ``select`` overrides single pools / gates with a given selection (the device's, at a near-tie
between fp32 and float64): the pooled value is gathered at the given position and the ReLU gate is taken as given.

At the end: the kernel-level reference of tests/test_caser_kernels_gpu.py -- one table's variables as a block
(``pack_block`` / ``unpack_block``: the flat layout of csrc/caser.hip), its forward with the tie masks, the backward written
out (``explicit_backward``, no autograd) and the comparator of the running-sum bound (``bar_excess``).
"""
import math
from collections import OrderedDict

import torch

from oracle import clsr_oracle as C
from oracle import sibling_oracle as S

EMB = C.EMB
TABLES = S.TABLES
# parameters of the tests' fixture: tests/test_caser_cpu.py shows that with them no pool and no ReLU gate of the golden
# training batch sits at a near-tie (the float32 and the float64 oracle select alike), for every L the GPU tests use
FIXTURE = dict(seed=5, scale_dense=8.0, bias_std=0.05)


def hparams(golden_hparams, **kw):
    """The golden hparams (T = 10, Di = 32, Dc = 8) as a Caser configuration: L = 3, n_v = n_h = 16 unless overridden."""
    import copy

    hp = copy.deepcopy(golden_hparams)
    for k, v in dict(dict(model_type="Caser", user_embedding_dim=16, L=3, n_v=16, n_h=16, T=1), **kw).items():
        setattr(hp, k, v)
    return hp


SCOPE = {"item": "sequential/caser/item/", "cate": "sequential/caser/cate/"}


def _dx(hp, key):
    return int(hp.item_embedding_dim if key == "item" else hp.cate_embedding_dim)


def vname(hp, key):
    return SCOPE[key] + "vertical/conv_%d/" % _dx(hp, key)


def hname(key, h):
    return SCOPE[key] + "horizonal/conv_%d/" % h


def param_specs(dims, hp):
    Vu, Vi, Vc = dims["Vu"], dims["Vi"], dims["Vc"]
    Di, Dc, Du = hp.item_embedding_dim, hp.cate_embedding_dim, hp.user_embedding_dim
    T, L, n_v, n_h = int(hp.max_seq_length), int(hp.L), int(hp.n_v), int(hp.n_h)
    specs = [(EMB + "user_embedding", (Vu, Du), "w"), (EMB + "item_embedding", (Vi, Di), "w"),
             (EMB + "cate_embedding", (Vc, Dc), "w")]
    for key in ("item", "cate"):
        Dx = _dx(hp, key)
        specs += [(vname(hp, key) + "kernel", (Dx, T, n_v), "glorot_conv"), (vname(hp, key) + "bias", (n_v,), "zero")]
        for h in range(1, L + 1):
            specs += [(hname(key, h) + "kernel", (h, Dx, n_h), "glorot_conv"), (hname(key, h) + "bias", (n_h,), "zero")]
    specs += C.mlp_names("sequential/logit_fcn/", 2 * (n_v + L * n_h) + Di + Dc, list(hp.layer_sizes))
    return specs


def init_params(dims, hp, seed=0, dtype=torch.float32, scale_dense=1.0, bias_std=0.0):
    """tnormal tables / MLP weights (``scale_dense`` widens them as in the sibling oracle), glorot_uniform conv kernels
    (fans = width * channels, tf.layers.conv1d's default).  ``bias_std`` > 0 draws the conv biases instead of leaving
    them at zero, so that a test also holds the bias path to non-trivial values."""
    gen = torch.Generator().manual_seed(seed)
    params = OrderedDict()
    for name, shape, k in param_specs(dims, hp):
        if k == "w":
            params[name] = C._tnormal(gen, shape, hp.init_value * scale_dense, dtype)
        elif k == "glorot_conv":
            lim = math.sqrt(6.0 / (shape[0] * (shape[1] + shape[2])))
            params[name] = ((torch.rand(shape, generator=gen, dtype=torch.float64) * 2 - 1) * lim).to(dtype)
        elif k == "one":
            params[name] = torch.ones(shape, dtype=dtype)
        elif bias_std > 0 and name.startswith("sequential/caser/"):
            params[name] = (torch.randn(shape, generator=gen, dtype=torch.float64) * bias_std).to(dtype)
        else:
            params[name] = torch.zeros(shape, dtype=dtype)
    return params


init_bn_state = C.init_bn_state
to_torch_feed = C.to_torch_feed
init_adam = C.init_adam


def vertical_pre(X, Wv, bv):
    """bv + the dense contraction of the flattened history: [B, n_v]."""
    return torch.einsum("btd,dtf->bf", X, Wv) + bv


def horizontal_pre(X, Wh, bh):
    """c_h [B, T - h + 1, n_h]."""
    h, T = Wh.shape[0], X.shape[1]
    c = bh.expand(X.shape[0], T - h + 1, -1)
    for j in range(h):
        c = c + X[:, j:T - h + 1 + j] @ Wh[j]
    return c


def first_max(c):
    """First position of the maximum over dim 1: [B, n_h] (long)."""
    n = c.shape[1]
    pos = torch.arange(n).view(1, n, 1).expand_as(c)
    return torch.where(c == c.amax(1, keepdim=True), pos, torch.full_like(pos, n)).amin(1)


def cnn(X, key, params, hp, select=None, info=None):
    """``_add_cnn``: [out_v | out_h(1) | ... | out_h(L)].  ``select`` (optional, this table's): dict of
    mask_v / gate_v [B, n_v] and mask / pos / gate [B, L, n_h]: where a mask is set, the given gate (and position) replace
    the oracle's own.  ``info`` receives the pre-activations: pre_v, c (list over h)."""
    L = int(hp.L)
    pre_v = vertical_pre(X, params[vname(hp, key) + "kernel"], params[vname(hp, key) + "bias"])
    out_v = torch.relu(pre_v)
    if select is not None:
        out_v = torch.where(select["mask_v"], pre_v * select["gate_v"].to(pre_v.dtype), out_v)
    outs, cs = [out_v], []
    for h in range(1, L + 1):
        c = horizontal_pre(X, params[hname(key, h) + "kernel"], params[hname(key, h) + "bias"])
        cs.append(c)
        o = torch.relu(torch.amax(c, 1))
        if select is not None:
            m, p, g = (select[k][:, h - 1] for k in ("mask", "pos", "gate"))
            picked = c.gather(1, p.clamp(0, c.shape[1] - 1).unsqueeze(1)).squeeze(1) * g.to(c.dtype)
            o = torch.where(m, picked, o)
        outs.append(o)
    if info is not None:
        info[key] = dict(pre_v=pre_v.detach(), c=[c.detach() for c in cs])
    return torch.cat(outs, 1)


def forward(params, bn_state, feed, hp, training, new_bn=None, sites=None, select=None):
    items, cates = feed["items"], feed["cates"]
    ih, ch = feed["item_history"], feed["item_cate_history"]
    item_tbl, cate_tbl = params[EMB + "item_embedding"], params[EMB + "cate_embedding"]

    def site(name, tbl, idx):
        g = tbl[idx]
        if sites is not None:
            if g.requires_grad:
                g.retain_grad()
            sites[name] = (g, idx)
        return g

    item_emb = site("item/target", item_tbl, items)
    item_hist = site("item/history", item_tbl, ih)
    cate_emb = site("cate/target", cate_tbl, cates)
    cate_hist = site("cate/history", cate_tbl, ch)
    inv_item = site("item/involved", item_tbl, C._unique(torch.cat([ih.reshape(-1), items.reshape(-1)])))
    inv_cate = site("cate/involved", cate_tbl, C._unique(torch.cat([ch.reshape(-1), cates.reshape(-1)])))
    target = torch.cat([item_emb, cate_emb], -1)
    info = {}
    sel = select or {}
    item_out = cnn(item_hist, "item", params, hp, sel.get("item"), info)
    cate_out = cnn(cate_hist, "cate", params, hp, sel.get("cate"), info)
    model_output = torch.cat([item_out, cate_out, target], 1)
    logit = C.fcn_net(model_output, list(hp.layer_sizes), "sequential/logit_fcn/", params, bn_state, hp, training, new_bn)
    return dict(logit=logit, pred=torch.sigmoid(logit), model_output=model_output, target=target,
                hist=dict(item=item_hist.detach(), cate=cate_hist.detach()), info=info,
                involved=dict(item=inv_item, cate=inv_cate))


def selection(out, hp):
    """The oracle's own selection of a forward pass: per table gate_v [B, n_v], pos / gate [B, L, n_h] (first maximum)."""
    sel = {}
    for key, inf in out["info"].items():
        sel[key] = dict(gate_v=inf["pre_v"] > 0, pos=torch.stack([first_max(c) for c in inf["c"]], 1),
                        gate=torch.stack([c.amax(1) > 0 for c in inf["c"]], 1))
    return sel


def abs_terms(X, params, hp, key):
    """Sum of |x . w| (+ |bias|) behind every pre-activation, and the number of terms K: the fp32 summation bound of a
    value is K * 2^-23 * that sum.  -> (a_v [B, n_v], K_v, [a_h [B, T - h + 1, n_h]], [K_h])"""
    A = {k: v.abs() for k, v in params.items()}
    Dx, T, L = _dx(hp, key), X.shape[1], int(hp.L)
    a_v = vertical_pre(X.abs(), A[vname(hp, key) + "kernel"], A[vname(hp, key) + "bias"])
    a_h = [horizontal_pre(X.abs(), A[hname(key, h) + "kernel"], A[hname(key, h) + "bias"]) for h in range(1, L + 1)]
    return a_v, T * Dx + 1, a_h, [h * Dx + 1 for h in range(1, L + 1)]


losses = S.losses


def gradients(params, bn_state, feed, hp, select=None, dedup_group=None):
    leaf = OrderedDict((k, v.detach().clone().requires_grad_(not k.endswith("/user_embedding")))
                       for k, v in params.items())
    new_bn, sites = OrderedDict(), {}
    out = forward(leaf, bn_state, feed, hp, True, new_bn, sites, select)
    ls = losses(leaf, out, feed, hp)
    ls["loss"].backward()
    grads, norms, raw = OrderedDict(), OrderedDict(), OrderedDict()
    tables = set(TABLES.values())
    for name, p in leaf.items():
        if name.endswith("/user_embedding"):
            continue
        if name in tables:
            key = [k for k, v in TABLES.items() if v == name][0]
            sumsq = sum(C.site_sumsq(sname, g.grad, dedup_group) for sname, (g, _) in sites.items()
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
    return {k: v.detach() for k, v in ls.items()}, grads, norms, new_bn, out


def train_step(params, bn_state, adam, step, feed, hp, select=None, lazy=False, dedup_group=None):
    """``lazy``: LazyAdam on the two tables (rows outside the feed's lookup sites keep values and moments);
    ``dedup_group``: the clip norms of the step with de-duplicated histories (clsr_oracle.site_sumsq)."""
    ls, grads, norms, new_bn, out = gradients(params, bn_state, feed, hp, select, dedup_group)
    new_params, new_adam = C.adam_apply(params, grads, adam, step, hp.learning_rate,
                                        lazy_rows=S.touched_rows(feed) if lazy else None)
    bn2 = OrderedDict(bn_state)
    bn2.update(new_bn)
    return new_params, bn2, new_adam, ls, grads, norms, out


@torch.no_grad()
def predict(params, bn_state, feed, hp):
    return forward(params, bn_state, feed, hp, False)


# ------------------------------------------------------------------------------------------ kernel-level reference
# One table's variables as a "block": dict(Wv [Dx, T, n_v], bv [n_v], Wh = [[h, Dx, n_h] for h = 1..L], bh = [[n_h]] * L);
# flat, it is the layout csrc/caser.hip states:  Wv | bv | Wh_1 | bh_1 | ... | Wh_L | bh_L,  each tensor contiguous.
EPS32 = 2.0 ** -23


def pack_block(blk):
    parts = [blk["Wv"].reshape(-1), blk["bv"].reshape(-1)]
    for W, b in zip(blk["Wh"], blk["bh"]):
        parts += [W.reshape(-1), b.reshape(-1)]
    return torch.cat(parts)


def unpack_block(flat, T, Dx, L, n_v, n_h):
    flat = flat.reshape(-1)
    o = [0]

    def take(*shape):
        n = int(math.prod(shape))
        t = flat[o[0]:o[0] + n].reshape(shape)
        o[0] += n
        return t

    blk = dict(Wv=take(Dx, T, n_v), bv=take(n_v), Wh=[], bh=[])
    for h in range(1, L + 1):
        blk["Wh"].append(take(h, Dx, n_h))
        blk["bh"].append(take(n_h))
    assert o[0] == flat.numel(), (o[0], flat.numel())
    return blk


def map_block(blk, fn):
    return dict(Wv=fn(blk["Wv"]), bv=fn(blk["bv"]), Wh=[fn(w) for w in blk["Wh"]], bh=[fn(b) for b in blk["bh"]])


def block_forward(X, blk):
    """-> (pooled [B, n_v + L n_h], masks): the pre-activations of one table in X's dtype and what the backward needs of
    them: gate_v [B, n_v] (pre_v > 0), per width M [B, T - h + 1, n_h] (c_h == max_t c_h), n [B, n_h] (tied positions),
    gate [B, n_h] (max > 0), first [B, n_h] (first maximum)."""
    pre_v = vertical_pre(X, blk["Wv"], blk["bv"])
    outs = [torch.relu(pre_v)]
    masks = dict(gate_v=pre_v > 0, M=[], n=[], gate=[], first=[])
    for W, b in zip(blk["Wh"], blk["bh"]):
        c = horizontal_pre(X, W, b)
        top = c.amax(1)
        M = c == top.unsqueeze(1)
        outs.append(torch.relu(top))
        masks["M"].append(M)
        masks["n"].append(M.sum(1))
        masks["gate"].append(top > 0)
        masks["first"].append(first_max(c))
    return torch.cat(outs, 1), masks


def explicit_backward(X, blk, dpool, masks):
    """The backward of one table written out, NOT autograd: with g = dpool where the gate is open (0 elsewhere) and
    A_h[b, s, f] = g_h[b, f] / n_h[b, f] where M_h[b, s, f] (0 elsewhere),
        d X[b, t, d]     = sum_f g_v[b, f] Wv[d, t, f] + sum_h sum_j sum_f A_h[b, t - j, f] Wh_h[j, d, f]
        d Wv[d, t, f]    = sum_b g_v[b, f] X[b, t, d]              d bv[f]   = sum_b g_v[b, f]
        d Wh_h[j, d, f]  = sum_b sum_s A_h[b, s, f] X[b, s + j, d]  d bh_h[f] = sum_b g_h[b, f]
    Every output is a sum of products that is linear in (g, W) and in (g, X) and the masks are GIVEN, so the same call on
    |X|, |W|, |dpool| returns S, the sum of the absolute addends of every output element.  -> (d X, gradient block)"""
    n_v = blk["Wv"].shape[2]
    g_v = dpool[:, :n_v] * masks["gate_v"].to(dpool.dtype)
    dX = torch.einsum("bf,dtf->btd", g_v, blk["Wv"]).contiguous()
    dblk = dict(Wv=torch.einsum("bf,btd->dtf", g_v, X), bv=g_v.sum(0), Wh=[], bh=[])
    off = n_v
    for h0, W in enumerate(blk["Wh"]):
        h, n_h = h0 + 1, W.shape[2]
        P = X.shape[1] - h + 1
        g = dpool[:, off:off + n_h] * masks["gate"][h0].to(dpool.dtype)
        off += n_h
        A = (g / masks["n"][h0].to(dpool.dtype)).unsqueeze(1) * masks["M"][h0].to(dpool.dtype)
        dblk["Wh"].append(torch.stack([torch.einsum("bsf,bsd->df", A, X[:, j:j + P]) for j in range(h)]))
        dblk["bh"].append(g.sum(0))
        for j in range(h):
            dX[:, j:j + P] += A @ W[j].t()
    return dX, dblk


def bar_excess(got, ref, S, N):
    """Worst of |got - ref| - N * 2^-23 * S over the elements (<= 0: within the running-sum bound of N addends whose
    absolute values sum to S) and where it sits."""
    ex = ((got.double() - ref.double()).abs() - N * EPS32 * S.double()).reshape(-1)
    if ex.numel() == 0:
        return 0.0, -1
    i = int(ex.argmax())
    return float(ex[i]), i


def chain_lengths(Hn, T, L, n_v, n_h, parts):
    """Addends of the longest chain behind an element: d hist (n_v vertical filters, up to h tied windows of every filter of
    every width, the prior content, the rounding of g / n), per variable of the gradient block (the histories' windows,
    the slices' partial sums, the rounding of g / n) -- the N of ``bar_excess``."""
    return dict(dhist=n_v + n_h * L * (L + 1) // 2 + 2, Wv=Hn + parts + 2, bv=Hn + parts,
                Wh=[Hn * (T - h + 1) + parts + 2 for h in range(1, L + 1)], bh=[Hn + parts] * L)
