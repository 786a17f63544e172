"""CPU oracle of NextItNet for the tests (torch, float64 by default)  --  TEST INFRASTRUCTURE ONLY.

Restatement of ``NextItNetModel._build_seq_graph`` (models/sequential/nextitnet.py:21-232) on the ``SequentialBaseModel``
trunk of oracle/sibling_oracle.py (embeddings, involved rows, logit MLP, losses) and the building blocks of
oracle/clsr_oracle.py (``fcn_net``, ``_unique``, ``_clip_factor``, ``adam_apply``).  One residual block per entry of
``dilations`` over x [B, T, C], half = C / 2:

    a1 = relu(LN1(x))   z1 = a1 . W1 + b1
    a2 = relu(LN2(z1))  z2[t] = bd + sum_{j < k} a2[t - (k - 1 - j) d] . Wd[j]     (positions before the history: zero)
    a3 = relu(LN3(z2))  x' = x + a3 . W2 + b2
    LN(v) = gamma (v - mean) / sqrt(var + 1e-8) + beta over the channel axis, biased variance

No mask anywhere.  Training: model_output has Hn T G rows in (h, t, g) order, row (h, t, g) = x_L[h, t] ++ the embedding of
items / cates [h G + g, t]; the labels are transposed the same way.  Evaluation: x_L[:, T - 1] ++ target.

The forward and the backward of a block are written out (``block_forward`` / ``block_backward``, no autograd; autograd
checks them in tests/test_nextitnet_cpu.py).  The kernel tests hold x_L and every saved block input to 4 m N 2^-23 S
(``fp32_bounds``): S (``abs_scale``) is the |.| evaluation of x_L = x_0 + sum_l (a3_l . W2_l + b2_l), N (``chain_length``)
the addends of the products behind an element, and m the error of a FLOAT32 restatement of this file against the float64
one on the same inputs, in units of N 2^-23 S, measured per case and per tensor on the CPU as the largest over nine
summation orders (``fp32_bounds``: the channels as they are and eight seeded permutations of them, each one term at a time
and with torch's own float32 operators).  A bound propagated term by term through three layer norms per block
diverges (an interval for the variance that reaches zero puts 1e4 on the root), so the rule for a factor that has to move
is used: measure float32 against float64 on the same inputs, allow four times that for a different summation order.
"""
import copy
import math
from collections import OrderedDict

import torch

from oracle import clsr_oracle as C
from oracle import sibling_oracle as S

EMB = C.EMB
TABLES = S.TABLES
EPS32 = 2.0 ** -23
LN_EPS = 1e-8
SCOPE = "sequential/nextitnet/"
#: the variables of a block in creation order = the flat layout of csrc/nextitnet.hip
BLOCK_KEYS = ("be1", "g1", "W1", "b1", "be2", "g2", "Wd", "bd", "be3", "g3", "W2", "b2")
BLOCK_NAMES = ("layer_norm1/beta", "layer_norm1/gamma", "conv1d_1/weight", "conv1d_1/bias", "layer_norm2/beta",
               "layer_norm2/gamma", "dilated_conv/weight", "dilated_conv/bias", "layer_norm3/beta", "layer_norm3/gamma",
               "conv1d_2/weight", "conv1d_2/bias")
# parameters of the step tests' fixture: tables and MLP weights widened as in the sibling oracle, the blocks' zero / one
# variables perturbed so that every bias, gamma and beta path carries a non-trivial value
FIXTURE = dict(seed=11, scale_dense=8.0, perturb=0.1)


def hparams(golden_hparams, **kw):
    """The golden hparams (T = 10, Di = 32, Dc = 8) as a NextItNet configuration: dilations [1, 2, 4], kernel_size 3."""
    hp = copy.deepcopy(golden_hparams)
    for k, v in dict(dict(model_type="NextItNet", user_embedding_dim=16, dilations=[1, 2, 4], kernel_size=3), **kw).items():
        setattr(hp, k, v)
    return hp


def block_scope(i, d):
    return SCOPE + "nextitnet_residual_block_one_decoder_layer_%d_%d/" % (i, d)


def block_shapes(C_, k):
    h = int(0.5 * C_)
    return OrderedDict(zip(BLOCK_KEYS, ((C_,), (C_,), (1, 1, C_, h), (h,), (h,), (h,), (1, k, h, h), (h,), (h,), (h,),
                                       (1, 1, h, C_), (C_,))))


def param_specs(dims, hp):
    Vu, Vi, Vc = dims["Vu"], dims["Vi"], dims["Vc"]
    Di, Dc, Du = hp.item_embedding_dim, hp.cate_embedding_dim, hp.user_embedding_dim
    specs = [(EMB + "user_embedding", (Vu, Du), "w"), (EMB + "item_embedding", (Vi, Di), "w"),
             (EMB + "cate_embedding", (Vc, Dc), "w")]
    for i, d in enumerate(hp.dilations):
        for key, name, shape in zip(BLOCK_KEYS, BLOCK_NAMES, block_shapes(Di + Dc, int(hp.kernel_size)).values()):
            kind = "conv" if key[0] == "W" else ("one" if key[0] == "g" else "zero")
            specs.append((block_scope(i, int(d)) + name, shape, kind))
    return specs + C.mlp_names("sequential/logit_fcn/", 2 * (Di + Dc), list(hp.layer_sizes))


def init_params(dims, hp, seed=0, dtype=torch.float32, scale_dense=1.0, perturb=0.0, conv_std=0.02):
    gen = torch.Generator().manual_seed(seed)
    params = OrderedDict()
    for name, shape, k in param_specs(dims, hp):
        nx = name.startswith(SCOPE)
        if k == "w":
            params[name] = C._tnormal(gen, shape, hp.init_value * scale_dense, dtype)
        elif k == "conv":
            params[name] = C._tnormal(gen, shape, conv_std * scale_dense, dtype)
        else:
            base = torch.ones(shape, dtype=torch.float64) if k == "one" else torch.zeros(shape, dtype=torch.float64)
            if nx and perturb > 0:
                base = base + torch.randn(shape, generator=gen, dtype=torch.float64) * perturb
            params[name] = base.to(dtype)
    return params


init_bn_state = C.init_bn_state
to_torch_feed = C.to_torch_feed
init_adam = C.init_adam


def blocks_of(params, hp):
    """Per block the dict of BLOCK_KEYS with the conv weights squeezed: W1 [C, half], Wd [k, half, half], W2 [half, C]."""
    out = []
    for i, d in enumerate(hp.dilations):
        b = block_scope(i, int(d))
        p = {key: params[b + name] for key, name in zip(BLOCK_KEYS, BLOCK_NAMES)}
        p["W1"], p["Wd"], p["W2"] = p["W1"][0, 0], p["Wd"][0], p["W2"][0, 0]
        out.append(p)
    return out


# ------------------------------------------------------------------------------------------ the block, written out
def layer_norm(x, gamma, beta):
    """-> (y, xhat, rstd, var)"""
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    xhat = d * rstd
    return gamma * xhat + beta, xhat, rstd, var


def relu(y):
    """open for y > 0, closed at exactly 0"""
    return torch.where(y > 0, y, torch.zeros_like(y))


def taps(k, d, T):
    """(tap j, offset (k - 1 - j) d) of the taps that reach a position of the history at all"""
    return [(j, (k - 1 - j) * d) for j in range(k) if (k - 1 - j) * d < T]


def causal_conv(a, Wd, bd, d):
    """z[:, t] = bd + sum_j a[:, t - (k - 1 - j) d] . Wd[j], a [B, T, hin], Wd [k, hin, hout]"""
    T = a.shape[1]
    z = bd.expand(a.shape[0], T, Wd.shape[2])
    for j, off in taps(Wd.shape[0], d, T):
        z = z + torch.nn.functional.pad(a[:, :T - off] @ Wd[j], (0, 0, off, 0))
    return z


def block_forward(x, p, d):
    """-> (x', cache).  cache: the block's input, per layer norm i = 1..3 y_i (pre-ReLU), xhat_i, rstd_i, var_i, the
    activations a_i, and A = |a3| . |W2| + |b2|: the |.| evaluation of the residual branch's last product."""
    c = dict(x=x)
    c["y1"], c["xh1"], c["r1"], c["v1"] = layer_norm(x, p["g1"], p["be1"])
    c["a1"] = relu(c["y1"])
    z1 = c["a1"] @ p["W1"] + p["b1"]
    c["y2"], c["xh2"], c["r2"], c["v2"] = layer_norm(z1, p["g2"], p["be2"])
    c["a2"] = relu(c["y2"])
    z2 = causal_conv(c["a2"], p["Wd"], p["bd"], d)
    c["y3"], c["xh3"], c["r3"], c["v3"] = layer_norm(z2, p["g3"], p["be3"])
    c["a3"] = relu(c["y3"])
    c["A"] = c["a3"].abs() @ p["W2"].abs() + p["b2"].abs()
    return x + c["a3"] @ p["W2"] + p["b2"], c


def ln_backward(dy, y, xhat, rstd, gamma):
    """-> (d input, d gamma, d beta); the ReLU gate y > 0 is applied to dy first"""
    du = dy * (y > 0).to(dy.dtype)
    dxh = du * gamma
    dx = rstd * (dxh - dxh.mean(-1, keepdim=True) - xhat * (dxh * xhat).mean(-1, keepdim=True))
    red = tuple(range(dy.dim() - 1))
    return dx, (du * xhat).sum(red), du.sum(red)


def block_backward(c, p, d, dout):
    """The backward of one block written out, NOT autograd.  -> (d x, gradient dict over BLOCK_KEYS)"""
    k, T = p["Wd"].shape[0], dout.shape[1]
    g = {}
    flat = lambda t: t.reshape(-1, t.shape[-1])
    g["W2"], g["b2"] = flat(c["a3"]).t() @ flat(dout), flat(dout).sum(0)
    dz2, g["g3"], g["be3"] = ln_backward(dout @ p["W2"].t(), c["y3"], c["xh3"], c["r3"], p["g3"])
    da2 = torch.zeros_like(c["a2"])
    g["Wd"] = torch.zeros_like(p["Wd"])
    for j, off in taps(k, d, T):
        g["Wd"][j] = flat(c["a2"][:, :T - off]).t() @ flat(dz2[:, off:])
        da2[:, :T - off] += dz2[:, off:] @ p["Wd"][j].t()
    g["bd"] = flat(dz2).sum(0)
    dz1, g["g2"], g["be2"] = ln_backward(da2, c["y2"], c["xh2"], c["r2"], p["g2"])
    g["W1"], g["b1"] = flat(c["a1"]).t() @ flat(dz1), flat(dz1).sum(0)
    dx1, g["g1"], g["be1"] = ln_backward(dz1 @ p["W1"].t(), c["y1"], c["xh1"], c["r1"], p["g1"])
    return dout + dx1, g


def stack_forward(x, blocks, dilations):
    """-> (x_L, caches)"""
    caches = []
    for p, d in zip(blocks, dilations):
        x, c = block_forward(x, p, int(d))
        caches.append(c)
    return x, caches


def abs_scale(x0, caches):
    """S of x_L = x_0 + sum_l (a3_l . W2_l + b2_l): the sum of the absolute addends, |x_0| + sum_l (|a3_l| . |W2_l| + |b2_l|)"""
    return x0.abs() + sum(c["A"] for c in caches)


def chain_length(C_, k, nblocks):
    """Addends of the products behind an element of x_L, block after block: C + 1 (first 1x1 convolution and its bias),
    k half + 1 (dilated convolution), half + 1 (second 1x1 convolution), and the residual sum."""
    h = C_ // 2
    return nblocks * ((C_ + 1) + (k * h + 1) + (h + 1) + 1)


# ------------------------------------------------------------------------------------------ float32, one term at a time
def _seq_sum(v):
    acc = torch.zeros_like(v[..., 0])
    for i in range(v.shape[-1]):
        acc = acc + v[..., i]
    return acc


def _seq_ln(x, gamma, beta):
    n = x.shape[-1]
    mean = (_seq_sum(x) / n).unsqueeze(-1)
    d = x - mean
    var = (_seq_sum(d * d) / n).unsqueeze(-1)
    return gamma * (d * (1.0 / torch.sqrt(var + LN_EPS))) + beta


def _seq_lin(a, W, b):
    acc = b.expand(a.shape[:-1] + (W.shape[1],)).clone()
    for n in range(W.shape[0]):
        acc = acc + a[..., n:n + 1] * W[n]
    return acc


def stack_forward_seq32(x, blocks, dilations):
    """The forward restated in FLOAT32 with every sum taken one term at a time in ascending order (bias first, taps
    ascending, channels ascending): the measuring stick of the kernel tests' bound.  -> (x_L, [input of every block])"""
    x = x.float()
    inputs = []
    for p, d in zip(blocks, dilations):
        p = {k: v.float() for k, v in p.items()}
        inputs.append(x)
        a1 = relu(_seq_ln(x, p["g1"], p["be1"]))
        a2 = relu(_seq_ln(_seq_lin(a1, p["W1"], p["b1"]), p["g2"], p["be2"]))
        T = x.shape[1]
        z2 = p["bd"].expand(a2.shape).clone()
        for j, off in taps(p["Wd"].shape[0], int(d), T):
            for i in range(a2.shape[-1]):
                z2[:, off:] = z2[:, off:] + a2[:, :T - off, i:i + 1] * p["Wd"][j][i]
        a3 = relu(_seq_ln(z2, p["g3"], p["be3"]))
        x = x + _seq_lin(a3, p["W2"], p["b2"])
    return x, inputs


FP32_DRAWS = 8


def _permuted(x0, blocks, gen):
    """The same computation with the channels in another order (one permutation of the C channels for the whole stack, one
    of the half channels per block): float64 gives the same x_L up to its own rounding, float32 ANOTHER draw of its
    rounding, because every sum over channels runs in another order.  -> (x0', blocks', the C permutation)"""
    C_ = x0.shape[-1]
    pc = torch.randperm(C_, generator=gen)
    out = []
    for p in blocks:
        ph = torch.randperm(C_ // 2, generator=gen)
        out.append(dict(be1=p["be1"][pc], g1=p["g1"][pc], W1=p["W1"][pc][:, ph], b1=p["b1"][ph], be2=p["be2"][ph],
                        g2=p["g2"][ph], Wd=p["Wd"][:, ph][:, :, ph], bd=p["bd"][ph], be3=p["be3"][ph], g3=p["g3"][ph],
                        W2=p["W2"][ph][:, pc], b2=p["b2"][pc]))
    return x0[..., pc], out, pc


def fp32_bounds(x0, xL, caches, blocks, dilations, C_, k):
    """The bounds the kernel tests hold x_L and every saved block input to, by the rule for a factor that has to move:
    measure a float32 restatement against float64 on the SAME inputs, allow four times that for a different summation
    order.  Per tensor: m = max |float32 - float64| / (N 2^-23 S), bound = 4 m N 2^-23 S elementwise (S: ``abs_scale``,
    N: ``chain_length`` of the blocks before the tensor).  The maximum over a tensor of a few dozen elements is ONE draw of
    the rounding, and a layer-norm row of small variance makes single elements carry most of it: two float32 evaluations
    of the 56-element second input of the 16-block case gave 0.14 and 0.43, and torch's float32 products differ from one
    CPU to the next.  So the float32 error is measured over FP32_DRAWS + 1 summation orders -- the channels as they are
    and FP32_DRAWS seeded channel permutations (``_permuted``), each evaluated one term at a time
    (``stack_forward_seq32``) and by torch's own float32 operators -- and m is the largest.  Nothing here comes from a kernel.
    -> (bound of x_L, [bound of the input of block l], [m of x_L, m of the inputs of blocks 1 ..])"""
    L = len(caches)
    refs = [xL] + [caches[l]["x"] for l in range(1, L)]
    units = [chain_length(C_, k, l) * EPS32 * abs_scale(x0, caches[:l]) for l in [L] + list(range(1, L))]
    ms = [0.0] * L
    gen = torch.Generator().manual_seed(20240917)
    for draw in range(FP32_DRAWS + 1):
        if draw == 0:
            xp, bp, back = x0, blocks, None
        else:
            xp, bp, pc = _permuted(x0, blocks, gen)
            back = torch.argsort(pc)
        s32, sin = stack_forward_seq32(xp, bp, dilations)
        v32, vc = stack_forward(xp.float(), [{key: v.float() for key, v in p.items()} for p in bp], dilations)
        for gots in ([s32] + sin[1:], [v32] + [c["x"] for c in vc[1:]]):
            for i, got in enumerate(gots):
                got = got.double() if back is None else got.double()[..., back]
                ms[i] = max(ms[i], float(((got - refs[i]).abs() / units[i]).max()))
    bounds = [4 * m * u for m, u in zip(ms, units)]
    return bounds[0], [torch.zeros_like(x0)] + bounds[1:], ms


def stack_backward(caches, blocks, dilations, dout):
    grads = [None] * len(blocks)
    for i in reversed(range(len(blocks))):
        dout, grads[i] = block_backward(caches[i], blocks[i], int(dilations[i]), dout)
    return dout, grads


def pack_blocks(blocks):
    """The flat parameter block of csrc/nextitnet.hip."""
    return torch.cat([p[key].reshape(-1) for p in blocks for key in BLOCK_KEYS])


def unpack_blocks(flat, C_, k, nblocks):
    h, o, out = C_ // 2, 0, []
    shapes = dict(be1=(C_,), g1=(C_,), W1=(C_, h), b1=(h,), be2=(h,), g2=(h,), Wd=(k, h, h), bd=(h,), be3=(h,), g3=(h,),
                  W2=(h, C_), b2=(C_,))
    for _ in range(nblocks):
        p = {}
        for key in BLOCK_KEYS:
            n = int(math.prod(shapes[key]))
            p[key] = flat[o:o + n].reshape(shapes[key])
            o += n
        out.append(p)
    assert o == flat.numel(), (o, flat.numel())
    return out


def conditions(caches):
    """(smallest layer-norm variance, smallest |ReLU input|) over every block of a forward pass"""
    v = min(float(c[k].min()) for c in caches for k in ("v1", "v2", "v3"))
    y = min(float(c[k].abs().min()) for c in caches for k in ("y1", "y2", "y3"))
    return v, y


def gates(caches):
    return [c[k] > 0 for c in caches for k in ("y1", "y2", "y3")]


# ------------------------------------------------------------------------------------------ the model
def training_rows(xL, target, G):
    """model_output of a training step by index: row (h, t, g) = xL[h, t] ++ target[h G + g, t].  xL [Hn, T, C],
    target [Hn G, T, C] -> [Hn T G, 2 C]"""
    Hn, T, C_ = xL.shape
    tg = target.reshape(Hn, G, T, C_).permute(0, 2, 1, 3)
    return torch.cat([xL.unsqueeze(2).expand(Hn, T, G, C_), tg], -1).reshape(Hn * T * G, 2 * C_)


def literal_training_output(dilate_input, target, G, T):
    """``_training_output`` call by call: repeat, concat, reshape, transpose, reshape (nextitnet.py:78-92); dilate_input
    [Hn, T, C] (the histories of every G-th feed row), target [Hn G, T, C]."""
    mo = torch.repeat_interleave(dilate_input, G, dim=0)
    mo = torch.cat([mo, target], -1)
    mo = mo.reshape(-1, G, T, mo.shape[-1])
    mo = mo.permute(0, 2, 1, 3)
    return mo.reshape(-1, mo.shape[-1])


def transpose_labels(labels, G, T):
    """labels [Hn G, T] -> [Hn T G] in model_output's row order"""
    return labels.reshape(-1, G, T).permute(0, 2, 1).reshape(-1)


def forward(params, bn_state, feed, hp, training, new_bn=None, sites=None):
    items, cates = feed["items"], feed["cates"]
    ih, ch = feed["item_history"], feed["item_cate_history"]
    item_tbl, cate_tbl = params[EMB + "item_embedding"], params[EMB + "cate_embedding"]
    G, T = hp.train_num_ngs + 1, ih.shape[1]

    def site(name, tbl, idx):
        g = tbl[idx]
        if sites is not None:
            if g.requires_grad:
                g.retain_grad()
            sites[name] = (g, idx)
        return g

    if training:        # the graph takes the histories of every G-th row (nextitnet.py:29-38)
        ih, ch = ih[::G], ch[::G]
    item_emb = site("item/target", item_tbl, items)
    item_hist = site("item/history", item_tbl, ih)
    cate_emb = site("cate/target", cate_tbl, cates)
    cate_hist = site("cate/history", cate_tbl, ch)
    inv_item = site("item/involved", item_tbl, C._unique(torch.cat([feed["item_history"].reshape(-1), items.reshape(-1)])))
    inv_cate = site("cate/involved", cate_tbl, C._unique(torch.cat([feed["item_cate_history"].reshape(-1), cates.reshape(-1)])))
    target = torch.cat([item_emb, cate_emb], -1)
    x0 = torch.cat([item_hist, cate_hist], -1)
    xL, caches = stack_forward(x0, blocks_of(params, hp), hp.dilations)
    if training:
        model_output = training_rows(xL, target, G)
        labels_t = transpose_labels(feed["labels"], G, T)
    else:
        model_output = torch.cat([xL[:, -1], target[:, -1]], -1)
        labels_t = feed["labels"].reshape(-1)
    logit = C.fcn_net(model_output, list(hp.layer_sizes), "sequential/logit_fcn/", params, bn_state, hp, training, new_bn)
    return dict(logit=logit, pred=torch.sigmoid(logit), model_output=model_output, xL=xL, caches=caches, labels_t=labels_t,
                involved=dict(item=inv_item, cate=inv_cate))


def losses(params, out, feed, hp):
    """the trunk's losses over the transposed labels: data loss = - sum log p_pos / (Hn T)"""
    return S.losses(params, out, dict(labels=out["labels_t"]), hp)


def gradients(params, bn_state, feed, hp):
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
    out = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items() if k != "caches"}
    out["raw_grads"] = raw
    return {k: v.detach() for k, v in ls.items()}, grads, norms, new_bn, out


def lazy_adam_apply(params, grads, adam, step, lr, touched, beta1=0.9, beta2=0.999, eps=1e-8):
    """LazyAdam: as ``adam_apply``, but a table's moments and rows move only where the step touched a row (``touched``:
    table name -> row ids); dense variables as Adam."""
    return C.adam_apply(params, grads, adam, step, lr, beta1, beta2, eps, lazy_rows=touched)


def train_step(params, bn_state, adam, step, feed, hp, lazy=False):
    ls, grads, norms, new_bn, out = gradients(params, bn_state, feed, hp)
    if lazy:
        touched = {TABLES[k]: C._unique(torch.cat([feed[hk].reshape(-1), feed[tk].reshape(-1)]))
                   for k, hk, tk in (("item", "item_history", "items"), ("cate", "item_cate_history", "cates"))}
        new_params, new_adam = lazy_adam_apply(params, grads, adam, step, hp.learning_rate, touched)
    else:
        new_params, new_adam = C.adam_apply(params, grads, adam, step, hp.learning_rate)
    bn2 = OrderedDict(bn_state)
    bn2.update(new_bn)
    return new_params, bn2, new_adam, ls, grads, norms, out


@torch.no_grad()
def predict(params, bn_state, feed, hp):
    return forward(params, bn_state, feed, hp, False)
