#!/usr/bin/env python
"""The optimisers of the reference other than Adam (csrc/optim_tf.hip), measured two ways:

1. the row-list update of the BASELINE configs[4] item table (100M x 96 fp32) in isolation, with rotating sets of
   ~200 k touched rows (HIP events): bytes moved / kernel time, against lazy Adam's row update in the same run;
2. training steps at configs[1] (taobao) for adam, sgd, adagrad and ftrl (HIP events around K steps, after W warm-up
   steps).

    python scripts/bench_optim.py [--rows-only | --steps-only] [--steps K] [--warmup W]
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import build_hparams, time_kernel  # noqa: E402
from clsr_amd.net import TF_OPTIMIZERS  # noqa: E402
from clsr_amd.ops import call  # noqa: E402

HBM = 8e12      # MI355X HBM3E peak, bytes/s
# bytes per updated element: read g, p (+ slots); write p (+ slots), g = 0
ELEM_BYTES = {"sgd": 16, "adagrad": 24, "rmsprop": 32, "adadelta": 32, "ftrl": 32, "lazyadam": 32}


def bench_rows(V=100_000_000, C=96, nsets=3, touched=4096 * 51, reps=3):
    dev = "cuda"
    table = torch.zeros(V, C, device=dev)
    grad = torch.zeros(V, C, device=dev)
    s1 = torch.full((V, C), 0.1, device=dev)
    s2 = torch.zeros(V, C, device=dev)
    flags = torch.zeros(V, dtype=torch.uint8, device=dev)
    sumsq = torch.tensor([1.0, 0.0], dtype=torch.float64, device=dev)
    state = torch.tensor([1.0, 0.9, 0.999, 1e-3, 0.0, 0, 0, 0], dtype=torch.float64, device=dev)
    sets = []
    for j in range(nsets):
        g = torch.Generator(device=dev).manual_seed(777 + j)
        ids = torch.unique(torch.randint(1, V, (touched,), generator=g, device=dev)).int()
        sets.append((ids, torch.tensor([ids.numel(), 0], dtype=torch.int32, device=dev)))
    cap = max(s[0].numel() for s in sets)
    out = []
    for name in ["lazyadam", "sgd", "adagrad", "rmsprop", "adadelta", "ftrl"]:
        turn = [0]

        def run():
            ids, count = sets[turn[0] % nsets]
            turn[0] += 1
            if name == "lazyadam":
                call("clsr_table_adam_rows", table, grad, s1, s2, flags, ids, count, ids.numel(), C, sumsq, 1, 1, 5.0, state,
                     0.9, 0.999, 1e-8)
            else:
                code, slots = TF_OPTIMIZERS[name]
                call("clsr_table_tf_rows", code, table, grad, s1 if slots else None, s2 if len(slots) > 1 else None, flags,
                     ids, count, ids.numel(), C, sumsq, 1, 1, 5.0, state, 1e-3)
        nrows = sum(s[0].numel() for s in sets) / nsets
        nbytes = nrows * C * ELEM_BYTES[name] + nrows * 4 + nrows
        for r in range(reps):
            t = time_kernel(run, iters=21)
            rec = dict(what="row-list update, configs[4] item table %dx%d, %d touched rows" % (V, C, nrows), optimizer=name,
                       us=round(t * 1e6, 2), bytes=nbytes, gbps=round(nbytes / t / 1e9, 1), frac_hbm=round(nbytes / t / HBM, 4),
                       rep=r)
            print(json.dumps(rec), flush=True)
            out.append(rec)
    del table, grad, s1, s2
    torch.cuda.empty_cache()
    return out


def bench_steps(steps, warmup, names=("adam", "sgd", "adagrad", "ftrl"), config="taobao"):
    from clsr_amd.net import CLSRNet
    from clsr_amd.synthetic import CONFIGS, synthetic_feed

    cfg = CONFIGS[config]
    P, T = cfg["P"], cfg["T"]
    feed = synthetic_feed(P, T, cfg["Vu"], cfg["Vi"], cfg["Vc"], G=5, lengths="full", seed=20220425, ids="zipf")
    for name in names:
        hp = build_hparams(cfg, P, optimizer=name)
        net = CLSRNet(hp, dict(Vu=cfg["Vu"], Vi=cfg["Vi"], Vc=cfg["Vc"]), device="cuda:0", seed=0)
        f = net.upload(feed, True)
        for _ in range(warmup):
            net.train_step(f)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            net.train_step(f)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / steps
        net.check_abort()
        print(json.dumps(dict(what="configs[1] (%s) train step" % config, optimizer=name, ms_per_step=round(ms, 4),
                              steps=steps, warmup=warmup)), flush=True)
        del net, f
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-only", action="store_true")
    ap.add_argument("--steps-only", action="store_true")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--optimizers", default="adam,sgd,adagrad,ftrl")
    a = ap.parse_args()
    if not a.steps_only:
        bench_rows()
    if not a.rows_only:
        bench_steps(a.steps, a.warmup, names=a.optimizers.split(","))
