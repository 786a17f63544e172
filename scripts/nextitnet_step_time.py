#!/usr/bin/env python
"""Step time of NextItNet with nextitnet.yaml's shape (dilations [1, 2, 4, 1, 2, 4], kernel_size 3, C = 40) at
``--histories`` histories x 5 rows, seq_len 50, next to the A2SVD step, the sibling with the same trunk; both in ONE process.
Every position is trained: 4096 histories (the default, the batch of scripts/caser_step_time.py) are 1 024 000 logit rows
where A2SVD's logit MLP sees 20 480; ``--histories 819`` is a feed of 4 095 rows, 204 750 logit rows.

Both nets are warmed up (allocation, plan recording, replay), then they take turns: ``--repeats`` timed regions of
``--steps`` steps each per net, a device synchronise on both sides of a region, host clock.  Reported: median, minimum
and maximum of the regions per net and the ratio of the medians; then the two new launches alone (csrc/nextitnet.hip),
timed with device events on an otherwise idle device, beside what their FLOP count costs at the fp32 vector rate and
their bytes at the HBM rate.

    python scripts/nextitnet_step_time.py [--histories 4096] [--steps 20] [--repeats 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import build_hparams, time_kernel  # noqa: E402
from clsr_amd.ops import call, query  # noqa: E402
from clsr_amd.seqnet import SeqNet  # noqa: E402
from clsr_amd.synthetic import CONFIGS, synthetic_feed  # noqa: E402

FP32_TFLOPS = 157.3        # MI355X vector fp32 peak
HBM_TBS = 8.0              # MI355X HBM3E peak
DILATIONS, KERNEL = [1, 2, 4, 1, 2, 4], 3


def make(cfg, feed, kind, **over):
    hp = build_hparams(cfg, cfg["P"], model_type=kind, user_embedding_dim=16, layer_sizes=[100, 64], **over)
    net = SeqNet(hp, dict(Vu=cfg["Vu"], Vi=cfg["Vi"], Vc=cfg["Vc"]), kind=kind, device="cuda:0", seed=0)
    return net, net.upload(feed, True)


def per_position_feed(feed, G, Vi, Vc, seed):
    """The synthetic feed in NextItNetIterator's layout: full histories (no padding either way), row 0 of a group the
    history one step on with the target appended, the other rows drawn ids that differ from the positive."""
    rng = np.random.default_rng(seed)
    ih, ch = feed["item_history"][::G], feed["item_cate_history"][::G]
    P, T = ih.shape
    items, cates = np.zeros((P, G, T), dtype=np.int32), np.zeros((P, G, T), dtype=np.int32)
    items[:, 0, :-1], cates[:, 0, :-1] = ih[:, 1:], ch[:, 1:]
    items[:, 0, -1], cates[:, 0, -1] = feed["items"][::G], feed["cates"][::G]
    neg = rng.integers(1, Vi - 1, size=(P, G - 1, T))
    items[:, 1:] = neg + (neg >= items[:, :1])
    cates[:, 1:] = rng.integers(1, Vc, size=(P, G - 1, T))
    labels = np.zeros((P, G, T), dtype=np.float32)
    labels[:, 0] = 1.0
    return dict(feed, items=items.reshape(P * G, T), cates=cates.reshape(P * G, T), labels=labels.reshape(P * G, T))


def region(net, f, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        net.train_step(f)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def new_launches(net):
    """The two NextItNet launches of the last training step again, on its buffers: (forward us, backward us, FLOP, bytes)."""
    R, T, G, Hn = net.last_shape
    D, W, k, nb = net.D, net.out_dim, net.nx_k, net.nx_nb
    h = D // 2
    hist, mo = net._buf("hist", Hn, T, D), net._buf("model_output", R, W)
    saved, dxl = net._buf("nx.saved", nb, Hn, T, D), net._buf("nx.dxl", Hn, T, D)
    shape = (Hn, T, D, k, nb)
    parts, ws = query("clsr_nextitnet_parts", *shape), net._buf("nx.ws", query("clsr_nextitnet_workspace_floats", *shape))
    dhist = torch.zeros(Hn, T, D, device=hist.device)

    def fwd():
        call("clsr_nextitnet_fwd", hist, Hn, T, D, net.nx_W, k, nb, net.nx_dil, saved, mo, W, G, 0)

    def bwd():
        call("clsr_nextitnet_bwd", dxl, saved, Hn, T, D, net.nx_W, k, nb, net.nx_dil, dhist, ws)

    macs = D * h + k * h * h + h * D          # per position and block
    f_fwd = 2.0 * Hn * T * nb * macs
    f_bwd = 3 * f_fwd                         # the block again, its input gradients, its weight gradients
    b_fwd = 4.0 * (Hn * T * D * (1 + nb + G) + net.nx_P)
    b_bwd = 4.0 * (Hn * T * D * (2 + nb) + net.nx_P * (1 + parts))
    return (1e6 * time_kernel(fwd, iters=30), 1e6 * time_kernel(bwd, iters=30), (f_fwd, f_bwd), (b_fwd, b_bwd))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--histories", type=int, default=CONFIGS["taobao"]["P"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a step time is a measurement on the device")
    cfg = dict(CONFIGS["taobao"], P=a.histories)
    feed = synthetic_feed(cfg["P"], cfg["T"], cfg["Vu"], cfg["Vi"], cfg["Vc"], G=5, lengths="full", seed=20220425)
    nfeed = per_position_feed(feed, 5, cfg["Vi"], cfg["Vc"], seed=7)
    variants = [("a2svd", make(cfg, feed, "a2svd", attention_size=cfg["Di"] + cfg["Dc"])),
                ("nextitnet d=[1,2,4,1,2,4] k=3", make(cfg, nfeed, "nextitnet", dilations=DILATIONS, kernel_size=KERNEL))]
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
        print("%-30s median %.4f ms/step  (min %.4f, max %.4f over %d regions of %d steps)"
              % (name, out[name]["median_ms"], out[name]["min_ms"], out[name]["max_ms"], a.repeats, a.steps))
    print("nextitnet / a2svd = %.3f" % (out[variants[1][0]]["median_ms"] / out[variants[0][0]]["median_ms"]))
    fwd_us, bwd_us, flop, byts = new_launches(variants[1][1][0])
    for tag, us, fl, by in (("forward", fwd_us, flop[0], byts[0]), ("backward", bwd_us, flop[1], byts[1])):
        print("nextitnet %-8s launch alone: %8.1f us   (%.2f GFLOP = %.1f us at %.0f TFLOP/s fp32; %.1f MB = %.1f us at %.0f TB/s)"
              % (tag, us, fl / 1e9, fl / FP32_TFLOPS / 1e6, FP32_TFLOPS, by / 1e6, by / HBM_TBS / 1e6, HBM_TBS))
    out["histories"], out["logit_rows"] = a.histories, variants[1][1][0].last_shape[0]
    out["nextitnet_launches_us"] = dict(forward=round(fwd_us, 1), backward=round(bwd_us, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
