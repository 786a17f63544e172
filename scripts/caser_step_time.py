#!/usr/bin/env python
"""Step time of Caser with caser.yaml's widths (L 3, n_v 128, n_h 128) at batch 4096 positives x 5 rows, seq_len 50,
next to the A2SVD step -- the sibling with the same trunk and no recurrence -- both in ONE process.

Both nets are warmed up (allocation, plan recording, replay), then they take turns: ``--repeats`` timed regions of
``--steps`` steps each per net, a device synchronise on both sides of a region, host clock.  Reported: median, minimum
and maximum of the regions per net and the ratio of the medians; then the new launches alone (csrc/caser.hip: the
forward launch, the three backward launches), timed with device events on an otherwise idle device, beside what their
FLOP count costs at the fp32 vector rate and their bytes at the HBM rate.

    python scripts/caser_step_time.py [--steps 400] [--repeats 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import build_hparams, time_kernel  # noqa: E402
from clsr_amd.ops import call, query  # noqa: E402
from clsr_amd.seqnet import SeqNet  # noqa: E402
from clsr_amd.synthetic import CONFIGS, synthetic_feed  # noqa: E402

FP32_TFLOPS = 157.3        # MI355X vector fp32 peak
HBM_TBS = 8.0              # MI355X HBM3E peak


def make(cfg, feed, kind, **over):
    hp = build_hparams(cfg, cfg["P"], model_type=kind, user_embedding_dim=16, layer_sizes=[100, 64], **over)
    net = SeqNet(hp, dict(Vu=cfg["Vu"], Vi=cfg["Vi"], Vc=cfg["Vc"]), kind=kind, device="cuda:0", seed=0)
    return net, net.upload(feed, True)


def region(net, f, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        net.train_step(f)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def new_launches(net):
    """The Caser launches of the last training step again, on its buffers: (forward us, backward us, FLOP, bytes)."""
    B, T, G, Hn = net.last_shape
    Di, Dc, D, L, nv, nh = net.Di, net.Dc, net.D, net.cz_L, net.cz_nv, net.cz_nh
    PW2 = 2 * net.cz_pw
    hist, pooled, dpool = net._buf("hist", Hn, T, D), net._buf("cz.pooled", Hn, PW2), net._buf("cz.dpool", Hn, PW2)
    am = [net._buf("cz.argmax." + k, Hn, L, nh, dtype=torch.int32) for k in ("item", "cate")]
    ti = [net._buf("cz.ties." + k, Hn, L, nh, 1 + (T + 31) // 32, dtype=torch.int32) for k in ("item", "cate")]
    shape = (Hn, T, Di, Dc, L, nv, nh)
    ws = net._buf("cz.ws", query("clsr_caser_hconv_bwd_workspace_floats", *shape))
    dhist = torch.zeros(Hn, T, D, device=hist.device)
    W, dW = net.cz_W, net.cz_dW

    def fwd():
        call("clsr_caser_hconv_fwd", hist, D, Hn, T, Di, Dc, W["item"], W["cate"], L, nv, nh, pooled, PW2, am[0], am[1],
             ti[0], ti[1])

    def bwd():
        call("clsr_caser_hconv_bwd", dpool, PW2, pooled, PW2, am[0], am[1], ti[0], ti[1], hist, D, Hn, T, Di, Dc,
             W["item"], W["cate"], L, nv, nh, dhist, dW["item"], dW["cate"], ws)

    taps = L * (L + 1) // 2
    # forward: every window product + the vertical contraction; backward: the weight gradients' gathered sums (vertical:
    # a full product) + d hist of the vertical path (a full product) + the selected windows
    f_fwd = 2.0 * Hn * D * (sum((T - h + 1) * h for h in range(1, L + 1)) * nh + T * nv)
    f_bwd = 2.0 * Hn * D * (2 * T * nv + 2 * taps * nh)
    nparam = sum(query("clsr_caser_param_floats", T, Dx, L, nv, nh) for Dx in (Di, Dc))
    parts = query("clsr_caser_hconv_bwd_parts", *shape)
    b_fwd = 4.0 * (Hn * T * D + nparam + Hn * PW2 + Hn * L * nh * 2 * (2 + (T + 31) // 32))
    b_bwd = 4.0 * (3 * Hn * T * D + 2 * Hn * PW2 + nparam * (2 + 2 * parts))
    return (1e6 * time_kernel(fwd, iters=50), 1e6 * time_kernel(bwd, iters=50), (f_fwd, f_bwd), (b_fwd, b_bwd))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a step time is a measurement on the device")
    cfg = CONFIGS["taobao"]
    feed = synthetic_feed(cfg["P"], cfg["T"], cfg["Vu"], cfg["Vi"], cfg["Vc"], G=5, lengths="full", seed=20220425)
    variants = [("a2svd", make(cfg, feed, "a2svd", attention_size=cfg["Di"] + cfg["Dc"])),
                ("caser L=3 n_v=128 n_h=128", make(cfg, feed, "caser", L=3, n_v=128, n_h=128))]
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
        print("%-28s median %.4f ms/step  (min %.4f, max %.4f over %d regions of %d steps)"
              % (name, out[name]["median_ms"], out[name]["min_ms"], out[name]["max_ms"], a.repeats, a.steps))
    print("caser / a2svd = %.3f" % (out[variants[1][0]]["median_ms"] / out[variants[0][0]]["median_ms"]))
    fwd_us, bwd_us, flop, byts = new_launches(variants[1][1][0])
    for tag, us, fl, by in (("forward", fwd_us, flop[0], byts[0]), ("backward", bwd_us, flop[1], byts[1])):
        print("caser %-8s launches alone: %7.1f us   (%.2f GFLOP = %.1f us at %.0f TFLOP/s fp32; %.1f MB = %.1f us at %.0f TB/s)"
              % (tag, us, fl / 1e9, fl / FP32_TFLOPS / 1e6, FP32_TFLOPS, by / 1e6, by / HBM_TBS / 1e6, HBM_TBS))
    out["caser_launches_us"] = dict(forward=round(fwd_us, 1), backward=round(bwd_us, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
