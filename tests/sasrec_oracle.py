"""CPU oracle of SASRec for the tests (torch, float64 by default)  --  TEST INFRASTRUCTURE ONLY.

The executable form of the model's definition (csrc/sasrec.hip) on the ``SequentialBaseModel`` trunk of
oracle/sibling_oracle.py (embeddings, involved rows, logit MLP, losses) and the building blocks of oracle/clsr_oracle.py
(``fcn_net``, ``_unique``, ``_clip_factor``, ``adam_apply``).  Per history of ``len`` valid steps (left aligned), dh = C / heads:

    x_0[t] = hist[t] + pos[len - 1 - t]
    block:  u = LN1(x)   q, k, v = u Wq + bq, u Wk + bk, u Wv + bv
            a[t, s] = softmax over {s <= t, s < len} of q_h[t] . k_h[s] / sqrt(dh)     o[t] = concat_h sum_s a_h[t, s] v_h[s]
            y = x + o Wo + bo    w = LN2(y)    x' = y + relu(w W1 + b1) W2 + b2
    s = LNf(x_L[len - 1])        model_output = s ++ target
    LN(v) = gain (v - mean) / sqrt(var + 1e-8) + bias over the channel axis, biased variance

Steps t >= len are padding: their rows of every x_l are ZERO here (the kernels save zeros there), they are never keys, and
nothing that depends on them reaches s.  len = 0: s = 0.

The forward and the backward of the encoder are written out (``encoder_forward`` / ``encoder_backward``, no autograd; autograd
and torch's own attention / layer norm check them in tests/test_sasrec_cpu.py).  The kernel tests hold s and every saved
tensor to FOUR TIMES the largest error of a FLOAT32 restatement of this file against the float64 one on the same inputs
(``fp32_bounds``), measured per case and per tensor on the CPU over FP32_DRAWS + 1 summation orders: the channels as they
are and FP32_DRAWS seeded permutations of them (of the residual channels, of the feed-forward's hidden channels, and of the
heads and the channels inside a head), each evaluated one term at a time and with torch's own float32 operators.  Nothing
in a bound comes from a kernel.
"""
import copy
import math
from collections import OrderedDict

import torch

from oracle import clsr_oracle as C
from oracle import sibling_oracle as S

EMB = C.EMB
TABLES = S.TABLES
LN_EPS = 1e-8
SCOPE = "sequential/sasrec/"
#: the variables of a block in creation order = the flat layout of csrc/sasrec.hip
BLOCK_KEYS = ("g1", "be1", "Wq", "bq", "Wk", "bk", "Wv", "bv", "Wo", "bo", "g2", "be2", "W1", "b1", "W2", "b2")
BLOCK_NAMES = ("layer_norm1/gain", "layer_norm1/bias", "attention/query/kernel", "attention/query/bias",
               "attention/key/kernel", "attention/key/bias", "attention/value/kernel", "attention/value/bias",
               "attention/output/kernel", "attention/output/bias", "layer_norm2/gain", "layer_norm2/bias", "ffn_1/kernel",
               "ffn_1/bias", "ffn_2/kernel", "ffn_2/bias")
POS, GF, BEF = SCOPE + "position_embedding", SCOPE + "layer_norm_final/gain", SCOPE + "layer_norm_final/bias"
# parameters of the step tests' fixture: tables and MLP weights widened as in the sibling oracle, the encoder's zero / one
# variables perturbed so that every bias and gain path carries a non-trivial value
FIXTURE = dict(seed=11, scale_dense=8.0, perturb=0.1)


def hparams(golden_hparams, **kw):
    """The golden hparams (T = 10, Di = 32, Dc = 8) as a SASRec configuration: two blocks, one head."""
    hp = copy.deepcopy(golden_hparams)
    for k, v in dict(dict(model_type="SASRec", user_embedding_dim=16, num_blocks=2, num_heads=1), **kw).items():
        setattr(hp, k, v)
    return hp


def block_scope(l):
    return SCOPE + "block_%d/" % l


def encoder_names(nblocks):
    """Every variable of the encoder in creation order."""
    return [POS] + [block_scope(l) + n for l in range(nblocks) for n in BLOCK_NAMES] + [GF, BEF]


def param_specs(dims, hp):
    Vu, Vi, Vc = dims["Vu"], dims["Vi"], dims["Vc"]
    Di, Dc, Du = hp.item_embedding_dim, hp.cate_embedding_dim, hp.user_embedding_dim
    D = Di + Dc
    specs = [(EMB + "user_embedding", (Vu, Du), "w"), (EMB + "item_embedding", (Vi, Di), "w"),
             (EMB + "cate_embedding", (Vc, Dc), "w"), (POS, (int(hp.max_seq_length), D), "w")]
    for l in range(int(hp.num_blocks)):
        for key, name in zip(BLOCK_KEYS, BLOCK_NAMES):
            kind = "mat" if key[0] == "W" else ("one" if key[0] == "g" else "zero")
            specs.append((block_scope(l) + name, (D, D) if key[0] == "W" else (D,), kind))
    specs += [(GF, (D,), "one"), (BEF, (D,), "zero")]
    return specs + C.mlp_names("sequential/logit_fcn/", 2 * D, list(hp.layer_sizes))


def init_params(dims, hp, seed=0, dtype=torch.float32, scale_dense=1.0, perturb=0.0, mat_std=0.02):
    gen = torch.Generator().manual_seed(seed)
    params = OrderedDict()
    for name, shape, k in param_specs(dims, hp):
        if k == "w":
            params[name] = C._tnormal(gen, shape, hp.init_value * scale_dense, dtype)
        elif k == "mat":
            params[name] = C._tnormal(gen, shape, mat_std * scale_dense, dtype)
        else:
            base = torch.ones(shape, dtype=torch.float64) if k == "one" else torch.zeros(shape, dtype=torch.float64)
            if name.startswith(SCOPE) and perturb > 0:
                base = base + torch.randn(shape, generator=gen, dtype=torch.float64) * perturb
            params[name] = base.to(dtype)
    return params


init_bn_state = C.init_bn_state
to_torch_feed = C.to_torch_feed
init_adam = C.init_adam


def encoder_of(params, hp):
    """dict(pos, blocks = [dict over BLOCK_KEYS], gf, bef) of a parameter dict"""
    blocks = [{key: params[block_scope(l) + name] for key, name in zip(BLOCK_KEYS, BLOCK_NAMES)}
              for l in range(int(hp.num_blocks))]
    return dict(pos=params[POS], blocks=blocks, gf=params[GF], bef=params[BEF])


def cast(enc, dtype):
    return dict(pos=enc["pos"].to(dtype), blocks=[{k: v.to(dtype) for k, v in p.items()} for p in enc["blocks"]],
                gf=enc["gf"].to(dtype), bef=enc["bef"].to(dtype))


def pack(enc):
    """The flat parameter block of csrc/sasrec.hip."""
    return torch.cat([enc["pos"].reshape(-1)] + [p[key].reshape(-1) for p in enc["blocks"] for key in BLOCK_KEYS]
                     + [enc["gf"], enc["bef"]])


def unpack(flat, Tmax, C_, nblocks):
    o = Tmax * C_
    enc = dict(pos=flat[:o].reshape(Tmax, C_), blocks=[])
    for _ in range(nblocks):
        p = {}
        for key in BLOCK_KEYS:
            n = C_ * C_ if key[0] == "W" else C_
            p[key] = flat[o:o + n].reshape((C_, C_) if key[0] == "W" else (C_,))
            o += n
        enc["blocks"].append(p)
    enc["gf"], enc["bef"] = flat[o:o + C_], flat[o + C_:o + 2 * C_]
    assert o + 2 * C_ == flat.numel(), (o, flat.numel())
    return enc


# ------------------------------------------------------------------------------------------ the encoder, written out
def layer_norm(x, gain, bias):
    """-> (y, xhat, rstd, var)"""
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    xhat = d * rstd
    return gain * xhat + bias, xhat, rstd, var


def linear(a, W, b):
    return a @ W + b


def relu(y):
    """open for y > 0, closed at exactly 0"""
    return torch.where(y > 0, y, torch.zeros_like(y))


def masks(lens, T):
    """valid [Hn, T]: t < len; attend [Hn, T, T]: query t (valid) sees key s <= t, s < len"""
    t = torch.arange(T)
    valid = t[None, :] < lens[:, None]
    attend = valid[:, :, None] & valid[:, None, :] & (t[None, None, :] <= t[None, :, None])
    return valid, attend


def heads(x, nh):
    Hn, T, C_ = x.shape
    return x.reshape(Hn, T, nh, C_ // nh).transpose(1, 2)           # [Hn, nh, T, dh]


def attention(q, k, v, attend, nh):
    """Masked softmax attention written out.  Rows that see no key (padding queries) give zeros.  -> (o, a [Hn, nh, T, T])"""
    qh, kh, vh = heads(q, nh), heads(k, nh), heads(v, nh)
    m = attend[:, None]
    sc = (qh @ kh.transpose(-1, -2)) / math.sqrt(q.shape[-1] // nh)
    big = torch.where(m, sc, torch.full_like(sc, -float("inf"))).max(-1, keepdim=True).values
    big = torch.where(torch.isfinite(big), big, torch.zeros_like(big))
    e = torch.where(m, torch.exp(torch.where(m, sc, big) - big), torch.zeros_like(sc))
    l = e.sum(-1, keepdim=True)
    a = e / torch.where(l > 0, l, torch.ones_like(l))
    o = (a @ vh).transpose(1, 2).reshape(q.shape)
    return o, a


def block_forward(x, p, valid, attend, nh, ln=layer_norm, lin=linear):
    """-> (x', cache).  Rows of padding come out zero."""
    c = dict(x=x)
    c["u"], c["xh1"], c["r1"], c["v1"] = ln(x, p["g1"], p["be1"])
    c["q"], c["k"], c["v"] = lin(c["u"], p["Wq"], p["bq"]), lin(c["u"], p["Wk"], p["bk"]), lin(c["u"], p["Wv"], p["bv"])
    c["o"], c["a"] = attention(c["q"], c["k"], c["v"], attend, nh)
    y = x + lin(c["o"], p["Wo"], p["bo"])
    c["w"], c["xh2"], c["r2"], c["v2"] = ln(y, p["g2"], p["be2"])
    c["z"] = lin(c["w"], p["W1"], p["b1"])
    c["h1"] = relu(c["z"])
    vm = valid.unsqueeze(-1)
    return torch.where(vm, y + lin(c["h1"], p["W2"], p["b2"]), torch.zeros_like(y)), c


def encoder_forward(hist, lens, enc, nh, ln=layer_norm, lin=linear):
    """hist [Hn, T, C], lens [Hn] (int64, 0 .. T) -> (s [Hn, C], cache).  cache: x0, the blocks' caches (``x``: the input
    of the block), xlast = x_L[len - 1] (zero for len = 0) and the final layer norm's xhat / rstd / var."""
    Hn, T, C_ = hist.shape
    valid, attend = masks(lens, T)
    t = torch.arange(T)
    pidx = (lens[:, None] - 1 - t[None, :]).clamp(min=0)
    x = torch.where(valid.unsqueeze(-1), hist + enc["pos"][pidx], torch.zeros_like(hist))
    cache = dict(x0=x, valid=valid, attend=attend, pidx=pidx, blocks=[], lens=lens)
    for p in enc["blocks"]:
        x, c = block_forward(x, p, valid, attend, nh, ln, lin)
        cache["blocks"].append(c)
    some = (lens > 0).unsqueeze(-1)
    last = (lens - 1).clamp(min=0)
    xl = torch.where(some, x[torch.arange(Hn), last], torch.zeros_like(x[:, 0]))
    sf, cache["xhf"], cache["rf"], cache["vf"] = ln(xl, enc["gf"], enc["bef"])
    cache["xL"], cache["xlast"], cache["last"] = x, xl, last
    return torch.where(some, sf, torch.zeros_like(sf)), cache


def ln_backward(du, xhat, rstd, gain):
    """du: the gradient w.r.t. the norm's output.  -> (d input, d gain, d bias)"""
    dxh = du * gain
    dx = rstd * (dxh - dxh.mean(-1, keepdim=True) - xhat * (dxh * xhat).mean(-1, keepdim=True))
    red = tuple(range(du.dim() - 1))
    return dx, (du * xhat).sum(red), du.sum(red)


def block_backward(c, p, valid, nh, dout):
    """The backward of one block written out, NOT autograd.  -> (d x, gradient dict over BLOCK_KEYS)"""
    g = {}
    flat = lambda t: t.reshape(-1, t.shape[-1])
    d = dout * valid.unsqueeze(-1).to(dout.dtype)
    g["W2"], g["b2"] = flat(c["h1"]).t() @ flat(d), flat(d).sum(0)
    dh1 = (d @ p["W2"].t()) * (c["z"] > 0).to(d.dtype)
    g["W1"], g["b1"] = flat(c["w"]).t() @ flat(dh1), flat(dh1).sum(0)
    dyn, g["g2"], g["be2"] = ln_backward(dh1 @ p["W1"].t(), c["xh2"], c["r2"], p["g2"])
    dy = d + dyn
    g["Wo"], g["bo"] = flat(c["o"]).t() @ flat(dy), flat(dy).sum(0)
    doh = heads(dy @ p["Wo"].t(), nh)
    qh, kh, vh, a = heads(c["q"], nh), heads(c["k"], nh), heads(c["v"], nh), c["a"]
    da = doh @ vh.transpose(-1, -2)
    dsc = a * (da - (a * da).sum(-1, keepdim=True)) / math.sqrt(c["q"].shape[-1] // nh)
    back = lambda t: t.transpose(1, 2).reshape(c["q"].shape)
    dq, dk, dv = back(dsc @ kh), back(dsc.transpose(-1, -2) @ qh), back(a.transpose(-1, -2) @ doh)
    du = dq @ p["Wq"].t() + dk @ p["Wk"].t() + dv @ p["Wv"].t()
    for n, dd in (("q", dq), ("k", dk), ("v", dv)):
        g["W" + n], g["b" + n] = flat(c["u"]).t() @ flat(dd), flat(dd).sum(0)
    dxn, g["g1"], g["be1"] = ln_backward(du, c["xh1"], c["r1"], p["g1"])
    return dy + dxn, g


def encoder_backward(cache, enc, nh, ds):
    """ds [Hn, C] = d s.  -> (d hist [Hn, T, C], gradient dict(pos, blocks, gf, bef))"""
    lens, valid = cache["lens"], cache["valid"]
    Hn = ds.shape[0]
    some = (lens > 0).unsqueeze(-1).to(ds.dtype)
    dsm = ds * some
    dxl, dgf, dbef = ln_backward(dsm, cache["xhf"], cache["rf"], enc["gf"])
    dx = torch.zeros_like(cache["xL"])
    dx[torch.arange(Hn), cache["last"]] = dxl * some
    grads = [None] * len(enc["blocks"])
    for i in reversed(range(len(enc["blocks"]))):
        dx, grads[i] = block_backward(cache["blocks"][i], enc["blocks"][i], valid, nh, dx)
    dx = dx * valid.unsqueeze(-1).to(dx.dtype)
    dpos = torch.zeros_like(enc["pos"])
    dpos.index_add_(0, cache["pidx"][valid], dx[valid])
    return dx, dict(pos=dpos, blocks=grads, gf=dgf, bef=dbef)


def conditions(cache):
    """(smallest layer-norm variance over the VALID rows, smallest |ReLU input| there) of a forward pass"""
    valid = cache["valid"]
    some = cache["lens"] > 0
    if not bool(valid.any()):
        return float("inf"), float("inf")
    v = min([float(c[k][valid].min()) for c in cache["blocks"] for k in ("v1", "v2")] + [float(cache["vf"][some].min())])
    z = min(float(c["z"][valid].abs().min()) for c in cache["blocks"])
    return v, z


def gates(cache):
    return [(c["z"] > 0) & cache["valid"].unsqueeze(-1) for c in cache["blocks"]]


# ------------------------------------------------------------------------------------------ float32, other summation orders
def _seq_sum(v):
    acc = torch.zeros_like(v[..., 0])
    for i in range(v.shape[-1]):
        acc = acc + v[..., i]
    return acc


def seq_layer_norm(x, gain, bias):
    n = x.shape[-1]
    mean = (_seq_sum(x) / n).unsqueeze(-1)
    d = x - mean
    var = (_seq_sum(d * d) / n).unsqueeze(-1)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    xhat = d * rstd
    return gain * xhat + bias, xhat, rstd, var


def seq_linear(a, W, b):
    acc = b.expand(a.shape[:-1] + (W.shape[1],)).clone()
    for n in range(W.shape[0]):
        acc = acc + a[..., n:n + 1] * W[n]
    return acc


FP32_DRAWS = 8


def permuted(hist, enc, nh, gen):
    """The same computation with the channels in another order: one permutation of the residual channels for the whole
    stack, per block one of the feed-forward's hidden channels and one of the attention's (the heads among themselves and
    the channels inside each head: q, k, v and the rows of Wo alike, so every head keeps its members).  float64 gives the
    same s up to its own rounding, float32 ANOTHER draw of its rounding.  -> (hist', enc', the residual permutation)"""
    C_ = hist.shape[-1]
    dh = C_ // nh
    pc = torch.randperm(C_, generator=gen)
    blocks = []
    for p in enc["blocks"]:
        pf = torch.randperm(C_, generator=gen)
        ph = torch.cat([hd * dh + torch.randperm(dh, generator=gen) for hd in torch.randperm(nh, generator=gen).tolist()])
        q = dict(g1=p["g1"][pc], be1=p["be1"][pc], Wo=p["Wo"][ph][:, pc], bo=p["bo"][pc], g2=p["g2"][pc], be2=p["be2"][pc],
                 W1=p["W1"][pc][:, pf], b1=p["b1"][pf], W2=p["W2"][pf][:, pc], b2=p["b2"][pc])
        for n in "qkv":
            q["W" + n], q["b" + n] = p["W" + n][pc][:, ph], p["b" + n][ph]
        blocks.append(q)
    return hist[..., pc], dict(pos=enc["pos"][:, pc], blocks=blocks, gf=enc["gf"][pc], bef=enc["bef"][pc]), pc


def checked_tensors(s, cache):
    """What the kernels write in a training forward: s, the input of every block, x_L[len - 1]"""
    return [s] + [c["x"] for c in cache["blocks"]] + [cache["xlast"]]


def fp32_bounds(hist, lens, enc, nh):
    """Per tensor of ``checked_tensors``: 4 x the largest |float32 - float64| over all its elements and over 2 (FP32_DRAWS
    + 1) float32 evaluations of this file on the same inputs -- the channels as they are and FP32_DRAWS seeded permutations,
    each one term at a time (``seq_linear``, ``seq_layer_norm``) and with torch's own float32 operators.  -> (bounds, errors)"""
    s, cache = encoder_forward(hist, lens, enc, nh)
    refs = checked_tensors(s, cache)
    errs = [0.0] * len(refs)
    gen = torch.Generator().manual_seed(20241021)
    for draw in range(FP32_DRAWS + 1):
        if draw == 0:
            hp_, ep_, back = hist, enc, None
        else:
            hp_, ep_, pc = permuted(hist, enc, nh, gen)
            back = torch.argsort(pc)
        h32, e32 = hp_.float(), cast(ep_, torch.float32)
        for ops in (dict(ln=seq_layer_norm, lin=seq_linear), dict()):
            s32, c32 = encoder_forward(h32, lens, e32, nh, **ops)
            for i, got in enumerate(checked_tensors(s32, c32)):
                got = got.double() if back is None else got.double()[..., back]
                errs[i] = max(errs[i], float((got - refs[i]).abs().max()))
    return [4 * e for e in errs], errs


# ------------------------------------------------------------------------------------------ the model
def forward(params, bn_state, feed, hp, training, new_bn=None, sites=None):
    items, cates = feed["items"], feed["cates"]
    ih, ch, mask = feed["item_history"], feed["item_cate_history"], feed["mask"]
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
    hist = torch.cat([item_hist, cate_hist], 2)
    seq_len = mask.sum(1).long()
    s, cache = encoder_forward(hist, seq_len, encoder_of(params, hp), int(hp.num_heads))
    model_output = torch.cat([s, target], 1)
    logit = C.fcn_net(model_output, list(hp.layer_sizes), "sequential/logit_fcn/", params, bn_state, hp, training, new_bn)
    return dict(logit=logit, pred=torch.sigmoid(logit), model_output=model_output, target=target, hist_input=hist,
                seq_len=seq_len, s=s, involved=dict(item=inv_item, cate=inv_cate))


losses = S.losses


def gradients(params, bn_state, feed, hp, dedup_group=None):
    leaf = OrderedDict((k, v.detach().clone().requires_grad_(not k.endswith("/user_embedding")))
                       for k, v in params.items())
    new_bn, sites = OrderedDict(), {}
    out = forward(leaf, bn_state, feed, hp, True, new_bn, sites)
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
    out = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}
    out["raw_grads"] = raw
    return {k: v.detach() for k, v in ls.items()}, grads, norms, new_bn, out


def train_step(params, bn_state, adam, step, feed, hp, lazy=False, dedup_group=None):
    ls, grads, norms, new_bn, out = gradients(params, bn_state, feed, hp, dedup_group)
    new_params, new_adam = C.adam_apply(params, grads, adam, step, hp.learning_rate,
                                        lazy_rows=S.touched_rows(feed) if lazy else None)
    bn2 = OrderedDict(bn_state)
    bn2.update(new_bn)
    return new_params, bn2, new_adam, ls, grads, norms, out


@torch.no_grad()
def predict(params, bn_state, feed, hp):
    return forward(params, bn_state, feed, hp, False)
