#!/usr/bin/env python
"""Step time of A2SVD with and without dropout in the logit MLP (batch 4096 positives x 5 rows, seq_len 50: the shape
of ``python bench.py --model a2svd``), both in ONE process.

Every variant is warmed up (allocation, plan recording, replay), then the variants take turns: ``--repeats`` timed
regions of ``--steps`` steps each per variant, a device synchronise on both sides of a region, host clock.  Reported:
median, minimum and maximum of the regions per variant, and the ratio of the medians.

    python scripts/dropout_step_time.py [--steps 400] [--repeats 7] [--atomics]

``--atomics`` adds a third variant: no dropout, the target rows' gradients scattered with float atomics behind the sorted
history sums instead of riding in the sorted lists (the launch sequence before the target rows joined them)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import build_hparams  # noqa: E402
from clsr_amd.seqnet import SeqNet  # noqa: E402
from clsr_amd.synthetic import CONFIGS, synthetic_feed  # noqa: E402


def make(cfg, feed, **over):
    hp = build_hparams(cfg, cfg["P"], model_type="a2svd", user_embedding_dim=16, attention_size=cfg["Di"] + cfg["Dc"], **over)
    net = SeqNet(hp, dict(Vu=cfg["Vu"], Vi=cfg["Vi"], Vc=cfg["Vc"]), kind="a2svd", device="cuda:0", seed=0)
    return net, net.upload(feed, True)


def region(net, f, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        net.train_step(f)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--atomics", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a step time is a measurement on the device")
    cfg = CONFIGS["taobao"]
    feed = synthetic_feed(cfg["P"], cfg["T"], cfg["Vu"], cfg["Vi"], cfg["Vc"], G=5, lengths="full", seed=20220425)
    variants = [("user_dropout=False", make(cfg, feed)),
                ("dropout [0.3, 0.3]", make(cfg, feed, user_dropout=True, dropout=[0.3, 0.3]))]
    if a.atomics:
        net, f = make(cfg, feed)
        net._det_merged = lambda f_: {}
        variants.append(("user_dropout=False, atomic target scatter", (net, f)))
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
        print("%-45s median %.4f ms/step  (min %.4f, max %.4f over %d regions of %d steps)"
              % (name, out[name]["median_ms"], out[name]["min_ms"], out[name]["max_ms"], a.repeats, a.steps))
    base = out[variants[0][0]]["median_ms"]
    for name, _ in variants[1:]:
        print("%s / %s = %.3f" % (name, variants[0][0], out[name]["median_ms"] / base))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
