#!/usr/bin/env python
"""Step time of LGN with lgn.yaml's shape (item 32 + cate 8 = user 40) at batch 4096 positives x 5 rows, next to the A2SVD
step -- the lightest sibling on the same trunk -- both in ONE process, in the protocol of scripts/ncf_step_time.py.

The graph is synthetic, at the vocabulary sizes of CONFIGS["taobao"] (36 915 users, 64 138 items), ``--degree`` edges a user
on average (entries = 2 edges + one diagonal entry a row: 3 792 553 at the default 50).  Two runs, the SAME entry count:
even degrees, and Zipf item degrees plus one hub user of ``--hub`` items (scripts/lgn_propagation_time.py builds both).

Both nets are warmed up (allocation, plan recording, replay), then they take turns: ``--repeats`` timed regions of ``--steps``
steps each per net, a device synchronise on both sides of a region, host clock.  Reported: median, minimum and maximum per
net and the ratio of the medians; then every new launch alone (device events, idle device): the propagation launches beside
their gathered bytes (entries x C x 4) and the guide's rates for indexed rows from L2 and from the Infinity Cache, then
scoring, the logit backward, the category segment sums, the row regulariser and the gradient norms.

    python scripts/lgn_step_time.py [--steps 200] [--repeats 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import build_hparams, time_kernel  # noqa: E402
from clsr_amd import lgn_graph  # noqa: E402
from clsr_amd.ops import call  # noqa: E402
from clsr_amd.seqnet import SeqNet  # noqa: E402
from clsr_amd.synthetic import CONFIGS, synthetic_feed  # noqa: E402
from lgn_propagation_time import L2_TBS, MALL_TBS, even_edges, skewed_edges  # noqa: E402


def make(cfg, feed, kind, graph=None, **over):
    hp = build_hparams(cfg, cfg["P"], model_type=kind, layer_sizes=[100, 64], **over)
    kw = dict(graph=graph) if graph is not None else {}
    net = SeqNet(hp, dict(Vu=cfg["Vu"], Vi=cfg["Vi"], Vc=cfg["Vc"]), kind=kind, device="cuda:0", seed=0, **kw)
    return net, net.upload(feed, True)


def region(net, f, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        net.train_step(f)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def graph_of(cfg, edges, seed):
    Vu, Vi = cfg["Vu"], cfg["Vi"]
    a = lgn_graph.normalised_adjacency(Vu, Vi, *edges)
    i2c = np.random.default_rng(seed).integers(1, cfg["Vc"], Vi).astype(np.int32)
    i2c[0] = 0
    return lgn_graph.Graph(Vu, Vi, *a, *lgn_graph.csr_transpose(*a, Vu + Vi), i2c)


def new_launches(net, f):
    """Every launch of csrc/lgn.hip in the last training step again, on its buffers: name -> microseconds."""
    B, T, G, Hn = net.last_shape
    p, Vu, Vi, C, Di, Dc = net.lg_prop, net.dims["Vu"], net.dims["Vi"], net.D, net.Di, net.Dc
    udiv = G if f.get("compact") else 1
    b = p._bufs
    E0, F, dF, dE0 = net._buf("lg.E0", Vu + Vi, C), b["F"], net._buf("lg.dF", Vu + Vi, C), b["dE0"]
    logit, dlogit = net._buf("logit", B), net._buf("dlogit", B)
    du, di, uid = net._buf("lg.d_user", B, C), net._buf("lg.d_item", B, C), net._buf("lg.uid", B, dtype=torch.int32)
    scratch, tmp = torch.zeros_like(dF), torch.zeros(8, dtype=torch.float64, device=dF.device)
    cs, tg = net.lg_cate, net.tab_grad
    runs = dict(
        fwd_layer=lambda: call("clsr_lgn_layer_fwd", *p.fwd.head(), C, E0, net.lg_W[0], net.lg_b[0], b["S0"], b["E1"], None, None, p.fwd.ws),
        bwd_layer=lambda: call("clsr_lgn_layer_bwd", *p.bwd.head(), C, b["P1"], net.lg_W[1], dF, b["S1"], b["E1"], b["P0"], b["part1"], p.bwd.ws),
        gate=lambda: call("clsr_lgn_gate", dF, b["E2"], dF.numel(), 1.0 / 3.0, b["P1"]),
        score=lambda: call("clsr_lgn_score", f["users"], udiv, f["items"], F, Vu, Vi, C, B, logit),
        logit_bwd=lambda: call("clsr_lgn_logit_bwd", f["users"], udiv, f["items"], F, Vu, Vi, C, B, dlogit, du, di, uid),
        cate_sums=lambda: call("clsr_lgn_rows_sum", *cs.head(), Vi, dE0[Vu:, Di:], C, Dc, tg["cate"], Dc, cs.ws),
        reg_rows=lambda: call("clsr_lgn_reg_rows", net.lg_inv, F[Vu:], scratch[Vu:], Vi, C, 1e-6, net.lg_stats, tmp[0:], None),
        grad_sumsq=lambda: call("clsr_lgn_grad_sumsq", dE0, Vu, Vu + Vi, C, Di, net.lg_stats, tmp[1:], tmp[2:], tmp[3:]))
    out = {k: round(1e6 * time_kernel(fn, iters=30), 1) for k, fn in runs.items()}
    call("clsr_zero_floats", tg["cate"], tg["cate"].numel())       # (the gradient tables are zero between steps)
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--degree", type=int, default=50)
    ap.add_argument("--hub", type=int, default=20000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a step time is a measurement on the device")
    cfg = CONFIGS["taobao"]
    Vu, Vi = cfg["Vu"], cfg["Vi"]
    feed = synthetic_feed(cfg["P"], cfg["T"], Vu, Vi, cfg["Vc"], G=5, lengths="full", seed=20220425)
    graphs = dict(even=graph_of(cfg, even_edges(Vu, Vi, a.degree), 1),
                  skewed=graph_of(cfg, skewed_edges(Vu, Vi, Vu * a.degree, a.hub, 7), 1))
    lgn_over = dict(user_embedding_dim=cfg["Di"] + cfg["Dc"])
    variants = [("a2svd", make(cfg, feed, "a2svd", user_embedding_dim=16, attention_size=cfg["Di"] + cfg["Dc"]))]
    variants += [("lgn " + n, make(cfg, feed, "lgn", graph=g, **lgn_over)) for n, g in graphs.items()]
    for _, (net, f) in variants:
        region(net, f, a.warmup)
    times = {name: [] for name, _ in variants}
    for _ in range(a.repeats):
        for name, (net, f) in variants:
            times[name].append(region(net, f, a.steps))
    out = {}
    for name, _ in variants:
        t = times[name]
        out[name] = dict(median_ms=round(statistics.median(t), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4))
        print("%-12s median %.4f ms/step  (min %.4f, max %.4f over %d regions of %d steps)"
              % (name, out[name]["median_ms"], out[name]["min_ms"], out[name]["max_ms"], a.repeats, a.steps))
    print("lgn even / a2svd = %.3f, lgn skewed / lgn even = %.3f"
          % (out["lgn even"]["median_ms"] / out["a2svd"]["median_ms"], out["lgn skewed"]["median_ms"] / out["lgn even"]["median_ms"]))
    for name, (net, f) in variants[1:]:
        entries = net.lg_prop.entries
        gathered = entries * net.D * 4.0
        us = new_launches(net, f)
        out[name]["launches_us"], out[name]["entries"] = us, entries
        print("%s: %d entries, %.0f MB gathered per propagation launch (%.0f us at the L2 rate of %.1f TB/s, %.0f us at the "
              "Infinity Cache rate of %.1f)" % (name, entries, gathered / 1e6, gathered / L2_TBS / 1e6, L2_TBS,
                                                gathered / MALL_TBS / 1e6, MALL_TBS))
        for k, v in us.items():
            extra = "  = %.2f TB/s of gathered rows" % (gathered / v / 1e6) if k in ("fwd_layer", "bwd_layer") else ""
            print("    %-10s %8.1f us%s" % (k, v, extra))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
