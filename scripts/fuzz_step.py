#!/usr/bin/env python
"""Shape fuzzing of the training / scoring step against the CPU oracle (test infrastructure, like tests/).

Random small shapes -- embedding width D (= Du = H), history length T, positives P, rows per positive G, encoder
kind, MLP widths, losses, sequence-length patterns incl. length-1 histories and P = 1 -- one training step and one
scoring pass each, compared with oracle/clsr_oracle.py: logits, the five loss terms, every dense gradient, and the
embedding-table side of the step: the gradient table of every embedding, the IndexedSlices clip norms, the (lazy-)Adam
update of the tables and, under lazyadam, bit equality of every row the step does not involve.

    python scripts/fuzz_step.py [n_cases] [seed] [clsr,gru4rec,din,sli_rec,a2svd,dien]
    python scripts/fuzz_step.py long [clsr,gru4rec,din,sli_rec,a2svd,dien]

``long``: the committed long-history cases (long_cases(): T = 63 .. 256, the edges of the 64-step attention chunks), pinned
draws that run the same comparisons at the same bars (run_case) as the random ones; tests/test_long_histories_{cpu,gpu}.py
run the same lists.

FUZZ_F32=1 adds, to every failing gradient, how far the float32 ORACLE is from the float64 oracle on that tensor;
FUZZ_F32=cpu needs no GPU: the float32 oracle takes the place of the HIP step and is held to the same gradient / norm /
update bars (a case it misses is ill-conditioned in float32, whatever the kernels do).  Both end with the worst distance
per check and variable (STATS).
"""
import os
import sys
import traceback
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import build_hparams  # noqa: E402
from clsr_amd.net import CLSRNet  # noqa: E402
from clsr_amd.seqnet import SeqNet  # noqa: E402
from clsr_amd.synthetic import synthetic_feed  # noqa: E402
from oracle import clsr_oracle as O  # noqa: E402
from oracle import sibling_oracle as SO  # noqa: E402

# fp32 = the reference's arithmetic (every product at fp32 accuracy); fp32x3 = two-piece split-bf16 products (FUZZ_PRECISION)
PRECISION = os.environ.get("FUZZ_PRECISION", "fp32")
SIB_TYPES = {"gru4rec": "GRU4Rec", "din": "DIN", "sli_rec": "sli_rec", "a2svd": "A2SVD", "dien": "DIEN"}


STATS = {}     # (check, variable) -> [worst err / bar, worst abs err, largest |exp|] over the cases run so far


def close(got, exp, rtol, atol, tag=None):
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    exp = torch.as_tensor(exp).detach().double().cpu().reshape(-1)
    if got.shape != exp.shape:
        return "shape %s vs %s" % (tuple(got.shape), tuple(exp.shape))
    err = (got - exp).abs()
    if tag is not None:
        st = STATS.setdefault(tag, [0.0, 0.0, 0.0])
        ratio = float((err / (atol + rtol * exp.abs()).clamp_min(1e-300)).max())
        st[:] = [max(st[0], ratio), max(st[1], float(err.max())), max(st[2], float(exp.abs().max()))]
    if not bool(torch.isfinite(got).all() and torch.isfinite(exp).all()):      # (NaN passes every `err <= bar` below)
        return "non-finite values: %d computed, %d expected" % (int((~torch.isfinite(got)).sum()), int((~torch.isfinite(exp)).sum()))
    if float((err - (atol + rtol * exp.abs())).max()) > 0:
        return "max abs err %.3e (max |exp| %.3e)" % (float(err.max()), float(exp.abs().max()))
    return None


def trace(name, got, exp, rtol, atol):
    """FUZZ_TRACE: where a tensor misses its bar -- for a table [row, column], which narrows a failure to a width."""
    gt, ex = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(exp).detach().double().cpu()
    badm = ~((gt - ex).abs() <= (rtol * ex.abs() + atol))
    idx_bad = badm.nonzero()
    print(name, tuple(ex.shape), "mismatches", int(badm.sum()), "first", idx_bad[:4].tolist(), "last", idx_bad[-2:].tolist())
    if ex.dim() == 2 and len(idx_bad):
        print("    rows %d..%d (%d distinct), columns %d..%d (%d distinct)" % (
            int(idx_bad[:, 0].min()), int(idx_bad[:, 0].max()), len(idx_bad[:, 0].unique()),
            int(idx_bad[:, 1].min()), int(idx_bad[:, 1].max()), len(idx_bad[:, 1].unique())))
    for ij in idx_bad[:4].tolist():
        print("   ", ij, "got", float(gt[tuple(ij)]), "exp", float(ex[tuple(ij)]))


def table_norms(table_sumsq):
    """Clip norm per table from the step's squared-norm slots (``captured["table_sumsq"]``): the norm of the un-summed
    IndexedSlices values of every lookup site of the table, the layout tests/test_step_gpu.py reads."""
    ss = torch.as_tensor(table_sumsq).double().cpu().numpy()
    return dict(item=(ss[0] + ss[2] + ss[4]) ** 0.5, cate=(ss[1] + ss[3] + ss[5]) ** 0.5,
                user_long=(ss[6] + ss[8]) ** 0.5, user_short=(ss[7] + ss[9]) ** 0.5)


def table_checks(pre, tmap, got_grad, got_norm, got_new, loaded, oracle, floor, hp, raw32=None):
    """The embedding-table side of one step against the float64 oracle, at the bars of tests/test_step_gpu.py.
    ``got_grad``: table key -> gradient table (pre-clip, regulariser included), or None where the step ran without captured
    gradients (fuzz_sequence's pass with launch plans: the update and the idle rows only); ``got_norm``: key -> clip norm, or
    None where the step does not keep the reference's IndexedSlices norm (de-duplicated histories); ``got_new`` / ``loaded``:
    variable name -> float32 table after / before the step; ``oracle``: (params, new_p, grads, raw_grads, norms) of the
    float64 step."""
    params, new_p, grads, raw, norms = oracle
    problems = []
    if got_grad is not None and set(got_grad) != set(tmap):
        problems.append("%sgradient tables %s, expected %s" % (pre, sorted(got_grad), sorted(tmap)))
    for key, name in tmap.items():
        if got_grad is not None and key not in got_grad:
            continue
        # ---- the gradient table (dense equivalent of the IndexedSlices)
        scale = float(raw[name].abs().max()) + 1e-12
        rtol, atol = 2e-3, 2e-4 * scale + floor
        e = close(got_grad[key], raw[name], rtol, atol, ("grad", key)) if got_grad is not None else None
        if e:
            problems.append("%sgrad %s: %s" % (pre, name, e))
            if raw32 is not None:
                problems.append("      float32 oracle vs float64 oracle: max abs err %.3e" %
                                float((raw32[name].double() - raw[name].double()).abs().max()))
            if os.environ.get("FUZZ_TRACE"):
                trace(name, got_grad[key], raw[name], rtol, atol)
        # ---- tf.clip_by_norm's norm of the IndexedSlices
        if got_norm is not None:
            e = close([got_norm[key]], [norms[name]], 1e-3, 1e-7, ("norm", key))
            if e:
                problems.append("%sclip norm %s: %s (got %.6e, oracle %.6e)" % (pre, name, e, got_norm[key], norms[name]))
        # ---- the applied update (clip + Adam / lazy Adam)
        new = torch.as_tensor(got_new[name]).detach().cpu()
        before = torch.as_tensor(loaded[name]).detach().cpu()
        g_ = grads[name].double().reshape(-1)
        sel = g_.abs() > 100 * floor      # Adam's first step is ~lr * sign(g): skip gradients at noise level
        if int(sel.sum()):
            upd_got = (new.double().reshape(-1) - params[name].reshape(-1))[sel]
            upd_exp = (new_p[name].reshape(-1) - params[name].reshape(-1))[sel]
            e = close(upd_got, upd_exp, 5e-3, 0.02 * hp.learning_rate, ("update", key))
            if e:
                problems.append("%sadam update %s: %s" % (pre, name, e))
                if os.environ.get("FUZZ_TRACE"):
                    full = torch.zeros_like(g_)
                    full[sel] = 1.0
                    trace("update of " + name, (new.double() - params[name]) * full.view_as(params[name]),
                          (new_p[name] - params[name]) * full.view_as(params[name]), 5e-3, 0.02 * hp.learning_rate)
        # ---- lazy Adam touches involved rows only: every row the oracle leaves alone keeps its bits
        if str(hp.optimizer) == "lazyadam":
            V = params[name].shape[0]
            idle = (new_p[name] == params[name]).reshape(V, -1).all(1) & (grads[name] == 0).reshape(V, -1).all(1)
            same = (new.float().view(torch.int32) == before.float().view(torch.int32)).reshape(V, -1).all(1)
            STATS.setdefault(("idle rows", key), [0.0, 0.0, 0.0])[2] += float(idle.sum())
            if not bool(same[idle].all()):
                rows = (idle & ~same).nonzero().reshape(-1)
                problems.append("%slazyadam %s: %d of %d untouched rows changed, first %s" % (
                    pre, name, len(rows), int(idle.sum()), rows[:6].tolist()))
    return problems


def f32_step(orc, extra, params32, feed, hp):
    p32 = type(params32)((k, v.float()) for k, v in params32.items())
    return orc.train_step(p32, orc.init_bn_state(p32), orc.init_adam(p32), 1, orc.to_torch_feed(feed, dtype=torch.float32),
                          hp, *extra)


KINK = 2.0 ** -20     # 16 float32 ulps at 1: batch-norm outputs are O(1) sums of up to 512 float32 products


def kink_shifted(shift):
    """Context: the oracle's ReLUs of the hidden MLP layers switch at ``shift`` instead of at 0 (values move by at most
    |shift|; the gradient masks of the elements within |shift| of the kink flip).  A float64 step under +-KINK is what ANY
    float32 computation may give for a batch-norm output that close to 0, whichever order it sums in."""
    import contextlib

    @contextlib.contextmanager
    def cm():
        plain = O._activate
        O._activate = lambda x, name: torch.where(x > shift, x, torch.zeros_like(x)) if name == "relu" else plain(x, name)
        try:
            yield
        finally:
            O._activate = plain
    return cm()


def f32_case(kind, idx, dims, hp, feed, P):
    """FUZZ_F32=cpu: the float32 ORACLE in the place of the HIP step, against the float64 oracle at the gradient, clip-norm
    and update bars of one_case (no GPU).  What misses a bar here is ill-conditioned in float32 whatever computes it."""
    from clsr_amd.params import SIB_TABLES, TABLES

    if P == 1:
        return []
    if kind == "clsr":
        orc, extra, tmap = O, (), TABLES
        params32 = O.init_params(dims, hp, seed=idx, scale_dense=8.0)
    else:
        orc, extra, tmap = SO, (kind,), SIB_TABLES
        params32 = SO.init_params(dims, hp, kind, seed=idx, scale_dense=8.0)
    params = type(params32)((k, v.double()) for k, v in params32.items())
    new_p, _, _, _, grads, norms, out = orc.train_step(params, orc.init_bn_state(params), orc.init_adam(params), 1,
                                                       orc.to_torch_feed(feed, dtype=torch.float64), hp, *extra)
    new32, _, _, _, _, norms32, out32 = f32_step(orc, extra, params32, feed, hp)
    raw, raw32 = out["raw_grads"], out32["raw_grads"]
    dense = [n for n in raw if n not in set(tmap.values())]
    floor = 4e-6 * max(float(raw[n].abs().max()) for n in dense)
    problems = []
    for name in dense:
        scale = float(raw[name].abs().max()) + 1e-12
        e = close(raw32[name], raw[name], 2e-3, 2e-4 * scale + floor, ("grad", "dense"))
        if e:
            problems.append("float32 oracle grad %s: %s" % (name, e))
        sel = grads[name].double().reshape(-1).abs() > 100 * floor
        if int(sel.sum()):
            e = close((new32[name].double().reshape(-1) - params[name].reshape(-1))[sel],
                      (new_p[name].reshape(-1) - params[name].reshape(-1))[sel], 5e-3, 0.02 * hp.learning_rate,
                      ("update", "dense"))
            if e:
                problems.append("float32 oracle adam update %s: %s" % (name, e))
    return problems + table_checks("float32 oracle ", tmap, {k: raw32[v] for k, v in tmap.items()},
                                   {k: norms32[v] for k, v in tmap.items()}, new32, params32,
                                   (params, new_p, grads, raw, norms), floor, hp)


def kink_case(kind, idx, dims, hp, feed, P):
    """Second condition of admission of a long case, on the float64 oracle alone: no hidden unit within float32 noise of its
    ReLU kink carries a gradient that matters -- the float64 step with the kinks moved by +-KINK keeps every gradient within
    the bars of one_case (a case that does not is decided by rounding, not by kernels).  Conservative: the width assumes
    O(1) terms; a column of small terms is computed more finely than that, and its draw is turned away all the same."""
    from clsr_amd.params import SIB_TABLES, TABLES

    if P == 1:
        return []
    if kind == "clsr":
        orc, extra, tmap = O, (), TABLES
        params32 = O.init_params(dims, hp, seed=idx, scale_dense=8.0)
    else:
        orc, extra, tmap = SO, (kind,), SIB_TABLES
        params32 = SO.init_params(dims, hp, kind, seed=idx, scale_dense=8.0)
    params = type(params32)((k, v.double()) for k, v in params32.items())
    step = lambda: orc.train_step(params, orc.init_bn_state(params), orc.init_adam(params), 1,
                                  orc.to_torch_feed(feed, dtype=torch.float64), hp, *extra)[6]["raw_grads"]
    raw = step()
    dense = [n for n in raw if n not in set(tmap.values())]
    floor = 4e-6 * max(float(raw[n].abs().max()) for n in dense)
    problems = []
    for shift in (KINK, -KINK):
        with kink_shifted(shift):
            rawk = step()
        for name in raw:
            scale = float(raw[name].abs().max()) + 1e-12
            e = close(rawk[name], raw[name], 2e-3, 2e-4 * scale + floor, ("kink", "dense" if name in dense else "tables"))
            if e:
                problems.append("float64 oracle, ReLU kinks at %+.1e, grad %s: %s" % (shift, name, e))
    return problems


def print_stats():
    for tag in sorted(STATS):
        print("    worst %-10s %-10s err / bar %.3f   max abs err %.3e   (largest |exp| %.3e)" % (tag + tuple(STATS[tag])))


def draw_case(rng, idx, kind="clsr", pin=None):
    """Shape, hyper-parameters and feed recipe of one random case.  ``pin``: values that replace the drawn ones -- D, Dc, T,
    P, G, lengths or any hyper-parameter -- while the random rest (and the random stream) stays what it is."""
    pin = dict(pin or {})
    D = int(rng.choice([8, 12, 16, 20, 24, 32, 40, 48, 52, 64, 96, 128]))
    Dc = int(rng.choice([4, 8])) if D > 8 else 4
    T = int(rng.choice([1, 2, 3, 5, 8, 10, 17, 50]))
    P = int(rng.choice([1, 2, 3, 7, 16, 33, 64]))
    G = int(rng.choice([2, 3, 5, 10]))
    if os.environ.get("FUZZ_LONG"):      # histories across the 64-step chunks of the attention kernels (slow oracle)
        T = int(rng.choice([63, 64, 65, 100, 129, 250]))
        P = int(rng.choice([2, 3, 5]))
    enc = str(rng.choice(["time4lstm", "gru", "lstm"]))
    over = dict(
        sequential_model=enc, train_num_ngs=G - 1,
        contrastive_loss=str(rng.choice(["triplet", "bpr"])),
        att_fcn_layer_sizes=[int(rng.choice([8, 20, 40, 80])), int(rng.choice([4, 12, 40]))],
        layer_sizes=[int(rng.choice([16, 36, 100])), int(rng.choice([8, 64]))],
        contrastive_recent_k=int(rng.choice([1, 3, 5])),
        contrastive_length_threshold=int(rng.choice([0, 2, 5])),
        is_clip_norm=int(rng.choice([0, 1])),
        optimizer=str(rng.choice(["adam", "lazyadam"])),
    )
    if os.environ.get("FUZZ_CASE"):      # "D,Dc,T,P,G,encoder": pin the shape, keep the random rest
        tok = os.environ["FUZZ_CASE"].split(",")
        D, Dc, T, P, G = (int(x) for x in tok[:5])
        over.update(sequential_model=tok[5], train_num_ngs=G - 1)
        if len(tok) > 9:                 # ",a0,a1,l0,l1": pin the MLP widths too
            over.update(att_fcn_layer_sizes=[int(tok[6]), int(tok[7])], layer_sizes=[int(tok[8]), int(tok[9])])
    if kind == "clsr":
        over.update(interest_evolve=bool(rng.random() < 0.7), predict_long_short=bool(rng.random() < 0.7),
                    manual_alpha=bool(rng.random() < 0.25), manual_alpha_value=float(rng.choice([0.0, 0.3, 1.0])),
                    embed_l2=float(rng.choice([0.0, 1e-6, 1e-3])), layer_l2=float(rng.choice([0.0, 1e-6, 1e-3])),
                    discrepancy_loss_weight=float(rng.choice([0.0, 0.01, 0.5])),
                    contrastive_loss_weight=float(rng.choice([0.0, 0.1, 1.0])),
                    contrastive_margin=float(rng.choice([0.5, 1.0, 2.0])),
                    max_grad_norm=float(rng.choice([0.01, 2.0])))
    if os.environ.get("FUZZ_OVERRIDE"):  # json dict applied on top of the drawn hyper-parameters (probing a failing case)
        import json
        over.update(json.loads(os.environ["FUZZ_OVERRIDE"]))
    if kind != "clsr":    # the siblings: free hidden / attention / user widths (reference sli_rec.yaml & co.)
        over.update(model_type=SIB_TYPES[kind], user_embedding_dim=int(rng.choice([4, 16, 40])),
                    attention_size=int(rng.choice([8, 20, 40])), hidden_size=int(rng.choice([8, 20, 40, 64])))
        if kind == "sli_rec":
            over["hidden_size"] = D      # alpha mixes the A2SVD feature (D wide) with the encoder feature (H wide)
        if kind in ("sli_rec", "a2svd"):
            over["attention_size"] = D   # the A2SVD query is contracted with the projected history (base_model.py:622)
    D, Dc, T, P, G = (int(pin.pop(k, v)) for k, v in (("D", D), ("Dc", Dc), ("T", T), ("P", P), ("G", G)))
    if kind == "sli_rec":                # the sibling overrides above follow a pinned D (an unpinned one: the same values)
        over["hidden_size"] = D
    if kind in ("sli_rec", "a2svd"):
        over["attention_size"] = D
    over["train_num_ngs"] = G - 1
    pin_lengths = pin.pop("lengths", None)
    over.update(pin)
    cfg = dict(T=T, Di=D - Dc, Dc=Dc, Du=D, H=over.get("hidden_size", D), Vu=50, Vi=200, Vc=12)
    desc = "case %d %s: D=%d Dc=%d T=%d P=%d G=%d %s" % (idx, kind, D, Dc, T, P, G, over)
    one_case.desc = desc
    hp = build_hparams(cfg, P, **over)
    dims = dict(Vu=cfg["Vu"], Vi=cfg["Vi"], Vc=cfg["Vc"])
    lengths = str(rng.choice(["full", "uniform", "lognormal"])) if T > 1 else "full"
    feed_seed, short = int(rng.integers(1 << 30)), rng.random() < 0.5
    if pin_lengths and T > 1:
        lengths = pin_lengths
    return types.SimpleNamespace(desc=desc, hp=hp, dims=dims, cfg=cfg, D=D, Dc=Dc, T=T, P=P, G=G, lengths=lengths,
                                 feed_seed=feed_seed, short=short, idx=idx, kind=kind)


def make_feed(c, P=None, seed=None):
    """The training feed of a drawn case (``P`` / ``seed``: another batch of the same shape family)."""
    P = c.P if P is None else P
    feed = synthetic_feed(P, c.T, c.dims["Vu"], c.dims["Vi"], c.dims["Vc"], G=c.G, lengths=c.lengths,
                          ids="uniform", seed=c.feed_seed if seed is None else seed)
    if c.short and c.T > 1:     # force some length-1 histories
        k = max(1, P // 3)
        rows = np.arange(k * c.G)
        for key in ("item_history", "item_cate_history", "mask", "time_diff", "time_from_first_action",
                    "time_to_now"):
            feed[key][rows, 1:] = 0
    return feed


def one_case(rng, idx, kind="clsr"):
    c = draw_case(rng, idx, kind)
    only = os.environ.get("FUZZ_ONLY")   # "6,11": run these case numbers only (the random stream stays the same)
    if only and str(idx) not in only.split(","):
        return c.desc, None
    return c.desc, run_case(c)


def run_case(c):
    """Every comparison of one drawn case (random or pinned, draw_case sets ``c.idx`` / ``c.kind``): the problems found."""
    one_case.desc = c.desc
    desc, hp, dims, P, idx, kind = c.desc, c.hp, c.dims, c.P, c.idx, c.kind
    feed = make_feed(c)
    problems = []
    if os.environ.get("FUZZ_F32") == "cpu":       # (the long cases: both conditions of their admission)
        return f32_case(kind, idx, dims, hp, feed, P) + (kink_case(kind, idx, dims, hp, feed, P) if hasattr(c, "which") else [])
    for dedup in (True, False):
        if kind == "clsr":
            orc, extra = O, ()
            params32 = O.init_params(dims, hp, seed=idx, scale_dense=8.0)
            net = CLSRNet(hp, dims, device="cuda:0", seed=0, dedup_histories=dedup, precision=PRECISION)
        else:
            orc, extra = SO, (kind,)
            params32 = SO.init_params(dims, hp, kind, seed=idx, scale_dense=8.0)
            net = SeqNet(hp, dims, kind=kind, device="cuda:0", seed=0, dedup_histories=dedup)
        sd = dict(params32)
        sd.update(orc.init_bn_state(params32))
        net.load_state_dict(sd, strict=True)
        params = type(params32)((k, v.double()) for k, v in params32.items())
        tf = orc.to_torch_feed(feed, dtype=torch.float64)
        bn = orc.init_bn_state(params)
        # scoring (moving statistics)
        ev = orc.forward(params, bn, tf, hp, *extra, False)
        got_ev = net.forward(net.upload(feed, False), False)
        torch.cuda.synchronize()
        e = close(got_ev["logit"], ev["logit"], 1e-4, 1e-4)
        if e:
            problems.append("dedup=%s eval logit: %s" % (dedup, e))
        adam = orc.init_adam(params)
        new_p, new_bn, _, ls, grads, norms, out = orc.train_step(params, bn, adam, 1, tf, hp, *extra)
        if os.environ.get("FUZZ_WARM"):  # diagnosis: allocate every workspace in a throw-away pass first (a deviation
            net.train_step(net.upload(feed, True), apply=False)   # that disappears is a first-step allocation race)
            torch.cuda.synchronize()
        net.capture_grads = True
        got = net.train_step(net.upload(feed, True))
        torch.cuda.synchronize()
        e = close(got["logit"], out["logit"], 1e-4, 1e-4)
        if e:
            problems.append("dedup=%s train logit: %s" % (dedup, e))
        if os.environ.get("FUZZ_DEBUG") and kind == "clsr":   # gradients of the INTERMEDIATE tensors against autograd
            from collections import OrderedDict
            leaf = OrderedDict((k, v.detach().clone().requires_grad_(not k.endswith("/user_embedding")))
                               for k, v in params.items())
            o2 = O.forward(leaf, bn, tf, hp, True, OrderedDict(), {})
            keys = [k for k in ("att_fea_long", "att_fea_short", "short_intention", "causal_state", "target", "rnn_out",
                                "hist_input") if k in o2 and getattr(o2[k], "requires_grad", False)]
            for k in keys:
                o2[k].retain_grad()
            O.losses(leaf, o2, tf, hp)["loss"].backward()
            B_, T_, G_, Hn_ = net.last_shape
            D_, H_, Du_ = net.D, net.H, net.Du
            zp = [v for k, v in net._bufs.items() if k[0] == "zero_pool"][-1].detach().double().cpu()
            off = [0]

            def take(*shape):
                n = int(np.prod(shape))
                t = zp[off[0]:off[0] + n].view(*shape)
                off[0] += n
                return t
            dhist, drnn, dhist_lt = take(Hn_, T_, D_), take(Hn_, T_, H_), take(Hn_, T_, D_)
            dtarget, dS = take(B_, D_), take(B_, D_)
            dL, dM, dR = take(Hn_, D_), take(Hn_, D_), take(Hn_, D_)
            dfs, dsi = take(Hn_, H_), take(Hn_, Du_)
            for k in ("alpha", "att_fea_long", "att_fea_short", "model_output", "causal_state", "short_intention",
                      "rnn_out", "logit", "w_long", "w_short"):
                if k in got and k in o2 and got[k] is not None:
                    g_, e_ = got[k].detach().double().cpu(), o2[k].detach().double()
                    if g_.numel() != e_.numel() and e_.shape[0] == B_ and g_.shape[0] == Hn_:
                        e_ = e_.reshape(Hn_, B_ // Hn_, *e_.shape[1:])[:, 0]
                    if g_.numel() == e_.numel():
                        print("    [debug dedup=%s] fwd %-16s max abs err %.3e  (max |exp| %.3e)" % (
                            dedup, k, float((g_.reshape(-1) - e_.reshape(-1)).abs().max()), float(e_.abs().max())))
            grp = lambda t: t.reshape(Hn_, B_ // Hn_, *t.shape[1:]).sum(1) if t.shape[0] == B_ and Hn_ != B_ else t
            for nm, got_t, key in (("dS", dS, "att_fea_short"), ("dL", dL, "att_fea_long"), ("dsi", dsi, "short_intention"),
                                   ("dfs", dfs, "causal_state"), ("dtarget", dtarget, "target"), ("drnn", drnn, "rnn_out")):
                if key not in keys:
                    continue
                ex = o2[key].grad.double()
                ex = ex if ex.shape == got_t.shape else grp(ex)
                err = float((got_t - ex).abs().max())
                print("    [debug dedup=%s] %-8s max abs err %.3e  (max |exp| %.3e)" % (dedup, nm, err, float(ex.abs().max())))
                if os.environ.get("FUZZ_DEBUG") == "2":
                    rows = (got_t - ex).abs().reshape(got_t.shape[0], -1).max(1)[0]
                    print("        rows with err > 10%% of max:", (rows > 0.1 * rows.max()).nonzero().reshape(-1).tolist()[:40],
                          "of", got_t.shape[0])
        gl = net.read_losses()
        for k in ("loss", "data_loss", "regular_loss") + (("contrastive_loss", "discrepancy_loss")
                                                            if kind == "clsr" else ()):
            e = close([gl[k]], [float(ls[k])], 1e-5, 1e-6)
            if e:
                problems.append("dedup=%s %s: %s" % (dedup, k, e))
        if P == 1:
            # one positive: its in-batch "negatives" are the same item, every row of the batch is identical, every
            # batch-norm output sits exactly on the ReLU kink (y = beta = 0) and the oracle's float64 masks are
            # decided by rounding noise -- gradients are not comparable there; values and losses are
            continue
        raw = out["raw_grads"]
        raw32 = None
        if os.environ.get("FUZZ_F32"):   # conditioning check: how far is a float32 run of the ORACLE from its float64 run?
            raw32 = f32_step(orc, extra, params32, feed, hp)[6]["raw_grads"]
        floor = 4e-6 * max(float(raw[n].abs().max()) for n in net.dense_names)
        for name in net.dense_names:
            scale = float(raw[name].abs().max()) + 1e-12
            e = close(net.captured["dense"][name], raw[name], 2e-3, 2e-4 * scale + floor, ("grad", "dense"))
            if e:
                problems.append("dedup=%s grad %s: %s" % (dedup, name, e))
                if raw32 is not None:
                    problems.append("      float32 oracle vs float64 oracle: max abs err %.3e" %
                                    float((raw32[name].double() - raw[name].double()).abs().max()))
                if os.environ.get("FUZZ_TRACE"):
                    trace(name, net.captured["dense"][name], raw[name], 2e-3, 2e-4 * scale + floor)
        # the embedding tables: gradient tables, IndexedSlices clip norms (replicated computation == the reference's
        # semantics; de-duplicated histories sum a group's slices before the norm), (lazy-)Adam update
        sd = net.state_dict()
        problems += table_checks("dedup=%s " % dedup, net._table_map(), net.captured["tables"],
                                 None if dedup else table_norms(net.captured["table_sumsq"]), sd, params32,
                                 (params, new_p, grads, raw, norms), floor, hp, raw32)
        for name in net._unused_tables():     # created for checkpoint compatibility, never trained: an exactly-zero update
            if not torch.equal(sd[name].view(torch.int32), params32[name].view(torch.int32)):
                problems.append("dedup=%s unused table %s changed" % (dedup, name))
        # the applied update (clip + Adam, dense variables) and the batch-norm moving statistics
        for name in net.dense_names:
            g_ = grads[name].double().reshape(-1)
            sel = g_.abs() > 100 * floor      # Adam's first step is ~lr * sign(g): skip gradients at noise level
            if int(sel.sum()):
                e = close((sd[name].double().cpu().reshape(-1) - params[name].reshape(-1))[sel],
                          (new_p[name].reshape(-1) - params[name].reshape(-1))[sel], 5e-3, 0.02 * hp.learning_rate,
                          ("update", "dense"))
                if e:
                    problems.append("dedup=%s adam update %s: %s" % (dedup, name, e))
        for k, v in new_bn.items():
            e = close(sd[k], v, 1e-4, 1e-6)
            if e:
                problems.append("dedup=%s %s: %s" % (dedup, k, e))
    return problems


LONG_KINDS = ("clsr", "gru4rec", "din", "sli_rec", "a2svd", "dien")
LONG_T = (63, 64, 65, 127, 128, 129, 191, 192, 193, 250, 255, 256)    # the edges of the 64-step attention chunks
LONG_FULL_T = (64, 128, 192, 256)                                     # every chunk full
LONG_SEED = dict(A=64, B=256)
# Draws the float32 ORACLE does not hold within half of every bar, or whose float64 gradients move by more than that when
# the ReLU kinks of the hidden layers move by +-KINK (ill-conditioned in float32 whatever computes them; f32_case, kink_case):
# case number -> the attempt of np.random.default_rng([seed, idx, attempt]) that replaces it, first admitted
# (tests/test_long_histories_cpu.py holds the committed lists to the rule; DESIGN.md has the ratios).  At most 8 of list A
# and 4 of list B; the HIP step never decides what is in the lists.
LONG_REDRAWN = dict(A={11: 1, 36: 1, 42: 1, 43: 2, 66: 1}, B={73: 1, 75: 1})
LONG_ADMIT = 0.5


def long_cases(kinds=None, redrawn=None):
    """The committed long-history cases (64-step chunk edges 63 .. 256), drawn cases for run_case.  List A: every kind x
    every T of LONG_T, 2 / 3 / 5 positives, case numbers 0 .. 71; list B: every kind x LONG_FULL_T with three positives
    and every history T long, case numbers 72 .. 95.  A draw named in LONG_REDRAWN comes from a stream of its own, so
    replacing one moves no other."""
    redrawn = LONG_REDRAWN if redrawn is None else redrawn
    cases = []
    rng_a, rng_b = np.random.default_rng(LONG_SEED["A"]), np.random.default_rng(LONG_SEED["B"])
    idx = 0
    for which, rng, Ts in (("A", rng_a, LONG_T), ("B", rng_b, LONG_FULL_T)):
        for kind in LONG_KINDS:
            for T in Ts:
                pin = (lambda r: dict(T=T, P=int(r.choice([2, 3, 5])))) if which == "A" else \
                    (lambda r: dict(T=T, P=3, lengths="full"))
                c = draw_case(rng, idx, kind, pin=pin(rng))       # always drawn: the stream of the rest stays put
                attempt = redrawn[which].get(idx, 0)
                if attempt:
                    own = np.random.default_rng([LONG_SEED[which], idx, attempt])
                    c = draw_case(own, idx, kind, pin=pin(own))
                c.which, c.attempt = which, attempt
                c.id = "%s-T%d-%s%d" % (kind, T, which, idx)
                if kinds is None or kind in kinds:
                    cases.append(c)
                idx += 1
    return cases


BOUNDARY_SEED = 4096
# Draws of boundary_cases() the float32 ORACLE does not hold within LONG_ADMIT of every bar: case number -> the attempt of
# np.random.default_rng([BOUNDARY_SEED, idx, attempt]) that replaces it (same kind, same pinned shape).  At most one case in
# twenty (tests/test_boundaries_cpu.py); the HIP step never decides what is in the list.
BOUNDARY_REDRAWN = {86: 1, 167: 1}       # clsr-golden-G9 (0.594 of the worst bar), sli_rec-H48 (0.560)
BOUNDARY_TINY = dict(T=6, P=3, G=3, lengths="uniform")
BOUNDARY_ENC = ("time4lstm", "gru", "lstm")
BOUNDARY_D_EVERY_ENC = (8, 12, 44, 48, 52, 60, 64, 68, 80, 84, 88, 124, 128)       # widths every encoder runs at
BOUNDARY_A0 = (4, 8, 44, 76, 80, 84, 88, 96, 100, 104, 128, 132, 256)
BOUNDARY_A1 = (4, 8, 12, 44, 48, 52, 56, 80)
BOUNDARY_LAYERS = ((4, 4), (100, 60), (100, 64), (100, 68), (260, 64), (1024, 128))
BOUNDARY_G = (2, 8, 9, 16)
# per-row query columns of DIN / DIEN (= D: SeqNet splits no query; DIN's keys are D wide as well)
BOUNDARY_Q = (48, 52, 64, 68, 80, 84, 88, 128, 132, 160, 164)
BOUNDARY_SIB_H = (4, 8, 44, 48, 52, 64, 68, 80, 84, 100, 124, 128)      # (sli_rec: H = D is its query width as well)
BOUNDARY_SIB_ATT = (4, 44, 48, 52, 128)
BOUNDARY_SIB_DU = (4, 44)
BOUNDARY_SIBLINGS = ("gru4rec", "dien", "din", "a2svd", "sli_rec")


def _boundary_specs():
    """(axis, id, kind, pin) of every boundary case, in the committed order: a new case is APPENDED (its number seeds its
    stream, so no other case moves).  One axis moves per case; the rest sits well inside every dispatch boundary of
    clsr_amd/net.py / seqnet.py (widths 24 / 16 / 8: multiples of 8, so that every fused kernel admits them)."""
    small = dict(att_fcn_layer_sizes=[16, 8], layer_sizes=[16, 8])
    clsr = dict(BOUNDARY_TINY, D=24, Dc=4, **small)
    sib = dict(BOUNDARY_TINY, D=24, Dc=4, hidden_size=24, attention_size=24, user_embedding_dim=16, **small)
    every = dict(interest_evolve=True, predict_long_short=True, manual_alpha=False)     # every encoder and head in the graph
    golden = dict(clsr, D=40, Dc=8, att_fcn_layer_sizes=[80, 40], layer_sizes=[100, 64], sequential_model="time4lstm", **every)
    specs = []
    # ---- D of the CLSR graph (= Du = H): every multiple of 4 in 8 .. 128
    n = 0
    for D in range(8, 129, 4):
        for e in (range(3) if D in BOUNDARY_D_EVERY_ENC else (n % 3,)):
            Dc = 4 if (n % 2 == 0 or D < 16) else 4 * (D // 8)     # item / category column offsets of the segmented sums vary
            specs.append(("D", "clsr-D%d-%s" % (D, BOUNDARY_ENC[e]), "clsr", dict(clsr, D=D, Dc=Dc, sequential_model=BOUNDARY_ENC[e])))
            n += 1
    for A0 in BOUNDARY_A0:
        specs.append(("A0", "clsr-A0_%d" % A0, "clsr", dict(clsr, att_fcn_layer_sizes=[A0, 8])))
    for A1 in BOUNDARY_A1:
        specs.append(("A1", "clsr-A1_%d" % A1, "clsr", dict(clsr, att_fcn_layer_sizes=[16, A1])))
    for L in BOUNDARY_LAYERS:
        specs.append(("L", "clsr-L%dx%d" % L, "clsr", dict(clsr, layer_sizes=list(L))))
    for G in BOUNDARY_G:      # the golden widths: the fused heads and the fused encoder tail
        specs.append(("G", "clsr-golden-G%d" % G, "clsr", dict(golden, G=G)))
    for G in BOUNDARY_G:
        specs.append(("G", "clsr-D24-G%d" % G, "clsr", dict(clsr, G=G, sequential_model="time4lstm", **every)))
    # ---- the siblings: per-row query columns, encoder input width, hidden / attention / user widths
    for kind in ("din", "dien"):
        for Q in BOUNDARY_Q:
            specs.append(("Q", "%s-Q%d" % (kind, Q), kind, dict(sib, D=Q, Dc=4 * (Q // 8))))
    for D in (128, 132, 136):
        specs.append(("Q", "gru4rec-D%d" % D, "gru4rec", dict(sib, D=D)))
    for kind in BOUNDARY_SIBLINGS:
        for H in BOUNDARY_SIB_H:
            if kind == "sli_rec" and H == 4:
                continue      # (sli_rec: H = D, and D = 4 leaves no room for an item and a category width of 4 each)
            specs.append(("H", "%s-H%d" % (kind, H), kind, dict(sib, D=H) if kind == "sli_rec" else dict(sib, hidden_size=H)))
    for kind in ("din", "dien"):
        for A in BOUNDARY_SIB_ATT:
            specs.append(("att", "%s-att%d" % (kind, A), kind, dict(sib, attention_size=A)))
    for kind in BOUNDARY_SIBLINGS:
        for Du in BOUNDARY_SIB_DU:
            specs.append(("Du", "%s-Du%d" % (kind, Du), kind, dict(sib, user_embedding_dim=Du)))
    return specs


def boundary_cases(kinds=None, axes=None, redrawn=None):
    """The committed dispatch-boundary cases: tiny shapes (T = 6, three positives, three rows each) that put one width at a
    time on the last admitted and on the first refused value of every shape-dependent branch of the step (DESIGN.md section
    6 has the table; tests/test_boundaries_cpu.py holds the list to it by the kernels' own ``clsr_*_supported`` queries).
    Case ``idx`` is draw_case on np.random.default_rng([BOUNDARY_SEED, idx]) with the shape pinned: adding or replacing one
    case moves no other.  ``c.axis``: the swept argument; ``c.x3``: also run with precision="fp32x3" (the CLSR cases at a
    boundary of a kernel with a two-piece instance: every CLSR axis but the logit MLP's widths)."""
    redrawn = BOUNDARY_REDRAWN if redrawn is None else redrawn
    cases = []
    for idx, (axis, cid, kind, pin) in enumerate(_boundary_specs()):
        if (kinds is not None and kind not in kinds) or (axes is not None and axis not in axes):
            continue
        attempt = redrawn.get(idx, 0)
        # (widths the model ties to D -- sli_rec: hidden and attention size, a2svd: attention size -- follow D: draw_case)
        pin = {k: v for k, v in pin.items() if not ((k == "hidden_size" and kind == "sli_rec")
                                                    or (k == "attention_size" and kind in ("sli_rec", "a2svd")))}
        c = draw_case(np.random.default_rng([BOUNDARY_SEED, idx] + ([attempt] if attempt else [])), idx, kind, pin=pin)
        c.axis, c.id, c.attempt, c.pin = axis, cid, attempt, dict(pin)
        c.x3 = kind == "clsr" and axis != "L"
        cases.append(c)
    return cases


def worst_ratio():
    """Largest err / bar of the comparisons recorded in STATS."""
    return max([st[0] for st in STATS.values()] or [0.0])


def main_long(kinds):
    """``python scripts/fuzz_step.py long [kinds]``: the committed long cases, then the worst distance per check."""
    only = os.environ.get("FUZZ_ONLY")
    bad = n = 0
    merged = {}
    for c in long_cases(kinds):
        if only and str(c.idx) not in only.split(","):
            continue
        n += 1
        STATS.clear()
        try:
            problems = run_case(c)
        except Exception:
            bad += 1
            print("CRASH " + c.desc)
            print("    " + traceback.format_exc().strip().splitlines()[-1][:400])
            if os.environ.get("FUZZ_TRACE"):
                traceback.print_exc()
            if os.environ.get("FUZZ_F32") != "cpu":
                torch.cuda.synchronize()      # a device fault ends the run here: nothing more is started on that GPU
            continue
        for tag, st in STATS.items():
            m = merged.setdefault(tag, [0.0, 0.0, 0.0])
            m[:] = [max(m[0], st[0]), max(m[1], st[1]), m[2] + st[2] if tag[0] == "idle rows" else max(m[2], st[2])]
        if problems:
            bad += 1
            print("FAIL " + c.desc)
            for p in problems[:8]:
                print("    " + p)
        else:
            print("ok   %-22s worst err / bar %.3f   %s" % (c.id, worst_ratio(), c.desc.split(" {")[0]))
    print("%d of %d cases with problems" % (bad, n))
    STATS.clear()
    STATS.update(merged)
    print_stats()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "long":
        return main_long(sys.argv[2].split(",") if len(sys.argv) > 2 else None)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    kinds = sys.argv[3].split(",") if len(sys.argv) > 3 else ["clsr"]
    rng = np.random.default_rng(seed)
    bad = 0
    for i in range(n):
        try:
            desc, problems = one_case(rng, i, kinds[i % len(kinds)])
        except Exception as exc:
            bad += 1
            print("CRASH " + getattr(one_case, "desc", "case %d" % i))
            print("    " + traceback.format_exc().strip().splitlines()[-1][:400])
            if os.environ.get("FUZZ_TRACE"):
                traceback.print_exc()
            continue
        if problems is None:
            continue
        if problems:
            bad += 1
            print("FAIL " + desc)
            for p in problems[:8]:
                print("    " + p)
        else:
            print("ok   " + desc.split(" {")[0])
    print("%d of %d cases with problems" % (bad, n))
    print_stats()


if __name__ == "__main__":
    main()
