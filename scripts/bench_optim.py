#!/usr/bin/env python
"""The optimisers of the reference other than Adam (csrc/optim_tf.hip), measured two ways:

1. the row-list update of the BASELINE configs[4] item table (100M x 96 fp32) in isolation, with rotating sets of
   ~200 k touched rows (HIP events): bytes moved / kernel time, against lazy Adam's row update in the same run -- on the
   fp32 table, on a bf16 table (``lazyadam_h``) and on a bf16 table with its fp32 master (``lazyadam_hm``); the legs
   are interleaved (one timing of every leg per repetition);
2. training steps at configs[1] (taobao) for adam, sgd, adagrad and ftrl (HIP events around K steps, after W warm-up
   steps), per table mode of ``--tables`` (fp32 | bf16 | bf16+master).

    python scripts/bench_optim.py [--rows-only | --steps-only] [--steps K] [--warmup W] [--rows adam] [--tables MODES]
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
# (lazyadam_h: the bf16 table moves 2 + 2 bytes instead of 4 + 4; lazyadam_hm: bf16 half + 16-bit residual, 32 again)
ELEM_BYTES = {"sgd": 16, "adagrad": 24, "rmsprop": 32, "adadelta": 32, "ftrl": 32, "lazyadam": 32, "lazyadam_h": 28,
              "lazyadam_hm": 32}
ROW_LEGS = ["lazyadam", "lazyadam_h", "lazyadam_hm", "sgd", "adagrad", "rmsprop", "adadelta", "ftrl"]


def bench_rows(V=100_000_000, C=96, nsets=3, touched=4096 * 51, reps=3, names=ROW_LEGS):
    dev = "cuda"
    table = torch.zeros(V, C, device=dev)
    table_h = torch.zeros(V, C, dtype=torch.bfloat16, device=dev) if any(n.startswith("lazyadam_h") for n in names) else None
    table_lo = torch.zeros(V, C, dtype=torch.int16, device=dev) if "lazyadam_hm" in names else None
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

    def leg(name):
        turn = [0]

        def run():
            ids, count = sets[turn[0] % nsets]
            turn[0] += 1
            if name == "lazyadam":
                call("clsr_table_adam_rows", table, grad, s1, s2, flags, ids, count, ids.numel(), C, sumsq, 1, 1, 5.0, state,
                     0.9, 0.999, 1e-8)
            elif name == "lazyadam_h":
                call("clsr_table_adam_rows_h", table_h, grad, s1, s2, flags, ids, count, ids.numel(), C, sumsq, 1, 1, 5.0,
                     state, 0.9, 0.999, 1e-8)
            elif name == "lazyadam_hm":
                call("clsr_table_adam_rows_hm", table_h, table_lo, grad, s1, s2, flags, ids, count, ids.numel(), C, sumsq, 1,
                     1, 5.0, state, 0.9, 0.999, 1e-8)
            else:
                code, slots = TF_OPTIMIZERS[name]
                call("clsr_table_tf_rows", code, table, grad, s1 if slots else None, s2 if len(slots) > 1 else None, flags,
                     ids, count, ids.numel(), C, sumsq, 1, 1, 5.0, state, 1e-3)
        return run

    runs = [(name, leg(name)) for name in names]
    nrows = sum(s[0].numel() for s in sets) / nsets
    for r in range(reps):
        for name, run in runs:
            nbytes = nrows * C * ELEM_BYTES[name] + nrows * 4 + nrows
            t = time_kernel(run, iters=21)
            rec = dict(what="row-list update, configs[4] item table %dx%d, %d touched rows" % (V, C, nrows), optimizer=name,
                       us=round(t * 1e6, 2), bytes=nbytes, gbps=round(nbytes / t / 1e9, 1), frac_hbm=round(nbytes / t / HBM, 4),
                       rep=r)
            print(json.dumps(rec), flush=True)
            out.append(rec)
    del table, table_h, table_lo, grad, s1, s2, runs
    torch.cuda.empty_cache()
    return out


TABLE_MODES = {"fp32": {}, "bf16": dict(table_dtype="bf16"), "bf16+master": dict(table_dtype="bf16", table_master=True)}


def bench_steps(steps, warmup, names=("adam", "sgd", "adagrad", "ftrl"), config="taobao", tables=("fp32",), reps=1):
    from clsr_amd.net import CLSRNet
    from clsr_amd.synthetic import CONFIGS, synthetic_feed

    cfg = CONFIGS[config]
    P, T = cfg["P"], cfg["T"]
    feed = synthetic_feed(P, T, cfg["Vu"], cfg["Vi"], cfg["Vc"], G=5, lengths="full", seed=20220425, ids="zipf")
    for name, mode in [(n, m) for n in names for m in tables]:
        if mode != "fp32" and name in TF_OPTIMIZERS:
            continue                # (bf16 tables train with (lazy)Adam only)
        hp = build_hparams(cfg, P, optimizer=name)
        net = CLSRNet(hp, dict(Vu=cfg["Vu"], Vi=cfg["Vi"], Vc=cfg["Vc"]), device="cuda:0", seed=0, **TABLE_MODES[mode])
        f = net.upload(feed, True)
        for _ in range(warmup):
            net.train_step(f)
        for rep in range(reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                net.train_step(f)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / steps
            net.check_abort()
            print(json.dumps(dict(what="configs[1] (%s) train step" % config, optimizer=name, tables=mode,
                                  ms_per_step=round(ms, 4), steps=steps, warmup=warmup, rep=rep)), flush=True)
        del net, f
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-only", action="store_true")
    ap.add_argument("--steps-only", action="store_true")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--optimizers", default="adam,sgd,adagrad,ftrl")
    ap.add_argument("--rows", default="all", help="'all' or 'adam': only the three lazy-Adam legs of the row-list update")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tables", default="fp32", help="comma list of fp32, bf16, bf16+master (training steps)")
    a = ap.parse_args()
    if not a.steps_only:
        bench_rows(reps=a.reps, names=ROW_LEGS[:3] if a.rows == "adam" else ROW_LEGS)
    if not a.rows_only:
        bench_steps(a.steps, a.warmup, names=a.optimizers.split(","), tables=a.tables.split(","),
                    reps=a.reps if a.tables != "fp32" else 1)
