#!/usr/bin/env python
"""Step time of NCF with ncf.yaml's shape (user_embedding_dim 40, tower [80, 40]) at batch 4096 positives x 5 rows, next
to the A2SVD step -- the lightest sibling on the same trunk -- both in ONE process.

Both nets are warmed up (allocation, plan recording, replay), then they take turns: ``--repeats`` timed regions of
``--steps`` steps each per net, a device synchronise on both sides of a region, host clock.  Reported: median, minimum
and maximum of the regions per net and the ratio of the medians; then the new launches alone (csrc/ncf.hip: the scoring
launch, the two training launches), timed with device events on an otherwise idle device, beside what their FLOP count
costs at the fp32 vector rate and their bytes at the HBM rate.

    python scripts/ncf_step_time.py [--steps 400] [--repeats 7]
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
    hp = build_hparams(cfg, cfg["P"], model_type=kind, layer_sizes=[100, 64], **over)
    net = SeqNet(hp, dict(Vu=cfg["Vu"], Vi=cfg["Vi"], Vc=cfg["Vc"]), kind=kind, device="cuda:0", seed=0)
    return net, net.upload(feed, True)


def region(net, f, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        net.train_step(f)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def new_launches(net, f):
    """The NCF launches of the last training step again, on its buffers: (score us, train us, FLOP, bytes)."""
    B, T, G, Hn = net.last_shape
    Du, W = net.nc_Du, net.out_dim
    Gl = net.hp.train_num_ngs + 1
    udiv = G if f.get("compact") else 1
    shape = (net.nc_Du, net.nc_nl) + net.nc_w4
    logit, mo, dlogit = net._buf("logit", B), net._buf("model_output", B, W), net._buf("dlogit", B)
    sl = [net._buf("nc.d_" + k, B, Du) for k in ("user_gmf", "user_mlp", "item_gmf", "item_mlp")]
    uid = net._buf("nc.uid", B, dtype=torch.int32)
    ws = net._buf("nc.ws", query("clsr_ncf_workspace_floats", B, Gl, *shape))
    loss, ss = torch.zeros(8, dtype=torch.float64, device=logit.device), torch.zeros(4, dtype=torch.float64, device=logit.device)
    tabs = net._ncf_tables()

    def score():
        call("clsr_ncf_score", f["users"], udiv, f["items"], *tabs, net.nc_W, *shape, B, logit, None)

    def train():
        call("clsr_ncf_train", f["users"], udiv, f["items"], f["labels"], *tabs, net.nc_W, *shape, B, Gl, 1.0 / (B // Gl),
             logit, mo, dlogit, sl[0], sl[1], sl[2], sl[3], uid, ws, loss, ss)

    macs = net.nc_P + Du                       # multiply-adds a line: every weight once, the GMF product
    parts = query("clsr_ncf_parts", B, Gl)
    f_score, f_train = 2.0 * B * macs, 6.0 * B * macs
    b_score = 4.0 * (B * (4 * Du + 3) + net.nc_P)
    b_train = 4.0 * (B * (8 * Du + W + 6) + net.nc_P * (1 + parts))
    return (1e6 * time_kernel(score, iters=50), 1e6 * time_kernel(train, iters=50), (f_score, f_train), (b_score, b_train))


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
    variants = [("a2svd", make(cfg, feed, "a2svd", user_embedding_dim=16, attention_size=cfg["Di"] + cfg["Dc"])),
                ("ncf Du=40 [80, 40]", make(cfg, feed, "ncf", user_embedding_dim=40, ncf_layer_sizes=[80, 40]))]
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
    print("ncf / a2svd = %.3f" % (out[variants[1][0]]["median_ms"] / out[variants[0][0]]["median_ms"]))
    net, f = variants[1][1]
    nvals = sum(t.numel() for t in net.tables.values())
    print("table values swept by the dense Adam update: %.1f M in %d tables" % (nvals / 1e6, len(net.tables)))
    s_us, t_us, flop, byts = new_launches(net, f)
    for tag, us, fl, by in (("score", s_us, flop[0], byts[0]), ("train", t_us, flop[1], byts[1])):
        print("ncf %-6s launches alone: %7.1f us   (%.2f GFLOP = %.1f us at %.0f TFLOP/s fp32; %.1f MB = %.1f us at %.0f TB/s)"
              % (tag, us, fl / 1e9, fl / FP32_TFLOPS / 1e6, FP32_TFLOPS, by / 1e6, by / HBM_TBS / 1e6, HBM_TBS))
    out["ncf_launches_us"] = dict(score=round(s_us, 1), train=round(t_us, 1))
    out["table_values_M"] = round(nvals / 1e6, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
