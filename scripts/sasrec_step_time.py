#!/usr/bin/env python
"""Step time of SASRec with sasrec.yaml's shape (num_blocks 2, num_heads 1, C = 40) at ``--histories`` histories x 5 rows,
``--seq_len`` steps (50), next to the GRU4Rec step, the sibling with the same trunk and the same tail; both in ONE process.
``--long_histories`` builds the SASRec net with that keyword: a length the resident kernels refuse (106 and more at C = 40)
runs the tiled pair.  Where BOTH pairs admit the length (``--long_histories --seq_len 105``), the launches of the tiled pair
are also timed against the resident pair's, in alternating regions.

Both nets are warmed up (allocation, plan recording, replay), then they take turns: ``--repeats`` timed regions of
``--steps`` steps each per net, a device synchronise on both sides of a region, host clock.  Reported: median, minimum
and maximum of the regions per net and the ratio of the medians; then the two new launches alone (csrc/sasrec.hip),
timed with device events on an otherwise idle device, beside what their FLOP count costs at the fp32 vector rate and
their bytes at the HBM rate.

    python scripts/sasrec_step_time.py [--histories 4096] [--steps 20] [--repeats 7]
    python scripts/sasrec_step_time.py --long_histories --seq_len 105                      # tiled against resident launches
    python scripts/sasrec_step_time.py --long_histories --seq_len 250 --histories 1024     # the Kuaishou quick start's length
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
BLOCKS, HEADS = 2, 1


def make(cfg, feed, kind, **over):
    hp = build_hparams(cfg, cfg["P"], model_type=kind, user_embedding_dim=16, layer_sizes=[100, 64],
                       **{k: v for k, v in over.items() if k != "long_histories"})
    kw = dict(long_histories=True) if over.get("long_histories") else {}
    net = SeqNet(hp, dict(Vu=cfg["Vu"], Vi=cfg["Vi"], Vc=cfg["Vc"]), kind=kind, device="cuda:0", seed=0, **kw)
    return net, net.upload(feed, True)


def region(net, f, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        net.train_step(f)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def new_launches(net, f, tile, repeats=1):
    """The two SASRec launches of the last training step again, on its buffers -- the tiled pair under ``tile``, the
    resident pair for tile 0: (forward us, backward us, FLOP, bytes), each time the median of ``repeats`` regions of 30
    launches.  A list of tiles: the pairs take turns, region by region, and a tuple comes back per tile."""
    tiles = list(tile) if isinstance(tile, (list, tuple)) else [tile]
    B, T, G, Hn = net.last_shape
    D, W, nb, nh, Tm = net.D, net.out_dim, net.sa_nb, net.sa_nh, net.sa_T
    hist, mo = net._buf("hist", Hn, T, D), net._buf("model_output", B, W)
    saved = net._buf("sa.saved", query("clsr_sasrec_saved_floats", Hn, T, D, nb))
    shape = (Hn, T, Tm, D, nb)
    ds = torch.randn(Hn, D, device=hist.device)
    dhist = torch.zeros(Hn, T, D, device=hist.device)
    ls = 1 if f.get("compact") else G
    pairs = []
    for tl in tiles:
        if tl:
            parts = query("clsr_sasrec_tiled_parts", *shape)
            ws = net._buf("sa.tws.train", query("clsr_sasrec_tiled_workspace_floats", *(shape + (tl, 1))))
            fwd = (lambda tl=tl, ws=ws: call("clsr_sasrec_tiled_fwd", hist, f["seq_len"], ls, Hn, T, Tm, D, net.sa_W, nb, nh,
                                             saved, mo, W, G, tl, ws))
            bwd = (lambda tl=tl, ws=ws: call("clsr_sasrec_tiled_bwd", ds, saved, f["seq_len"], ls, Hn, T, Tm, D, net.sa_W, nb,
                                             nh, dhist, tl, ws))
            # the backward's parked rows (q, d o, d q Wq^T, the softmax statistics) go out once per block and come back once
            # per pair of tiles i >= j; the gradient rows make two round trips per block through d hist
            nt = (T + tl - 1) // tl
            extra = 4.0 * Hn * T * nb * ((3 * D + D // 2) * (1 + (nt + 1) / 2.0) + 4 * D)
        else:
            parts = query("clsr_sasrec_parts", *shape)
            ws = net._buf("sa.ws", query("clsr_sasrec_workspace_floats", *shape))
            fwd = (lambda: call("clsr_sasrec_fwd", hist, f["seq_len"], ls, Hn, T, Tm, D, net.sa_W, nb, nh, saved, mo, W, G))
            bwd = (lambda ws=ws: call("clsr_sasrec_bwd", ds, saved, f["seq_len"], ls, Hn, T, Tm, D, net.sa_W, nb, nh, dhist,
                                      ws))
            extra = 0.0
        pairs.append((fwd, bwd, parts, extra))
    # per position and block: six C x C products; the causal attention touches (T + 1) / 2 keys per query on average, a
    # score and a weighted value of C multiply-adds each (the two-pass softmax forms every score twice: not counted)
    macs = 6 * D * D + 2 * D * (T + 1) / 2
    f_fwd = 2.0 * Hn * T * nb * macs
    f_bwd = 3 * f_fwd                         # the block again, its input gradients, its weight gradients
    b_fwd = 4.0 * (Hn * T * D * (1 + nb) + Hn * D * (1 + G) + net.sa_P)
    t_f, t_b = [[] for _ in pairs], [[] for _ in pairs]
    for _ in range(repeats):
        for i, (fwd, bwd, _, _) in enumerate(pairs):
            t_f[i].append(1e6 * time_kernel(fwd, iters=30))
            t_b[i].append(1e6 * time_kernel(bwd, iters=30))
    res = []
    for i, (_, _, parts, extra) in enumerate(pairs):
        b_bwd = 4.0 * (Hn * T * D * (1 + nb) + 2 * Hn * D + net.sa_P * (1 + parts)) + extra
        res.append((statistics.median(t_f[i]), statistics.median(t_b[i]), (f_fwd, f_bwd), (b_fwd, b_bwd)))
    return res if isinstance(tile, (list, tuple)) else res[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--histories", type=int, default=CONFIGS["taobao"]["P"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seq_len", type=int, default=CONFIGS["taobao"]["T"], help="steps of every history (all of them real)")
    ap.add_argument("--long_histories", action="store_true", help="build the SASRec net with long_histories=True")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a step time is a measurement on the device")
    cfg = dict(CONFIGS["taobao"], P=a.histories, T=a.seq_len)
    feed = synthetic_feed(cfg["P"], cfg["T"], cfg["Vu"], cfg["Vi"], cfg["Vc"], G=5, lengths="full", seed=20220425)
    variants = [("gru4rec", make(cfg, feed, "gru4rec")),
                ("sasrec blocks=%d heads=%d" % (BLOCKS, HEADS), make(cfg, feed, "sasrec", num_blocks=BLOCKS, num_heads=HEADS, long_histories=a.long_histories))]
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
    print("sasrec / gru4rec = %.3f" % (out[variants[1][0]]["median_ms"] / out[variants[0][0]]["median_ms"]))
    net, f = variants[1][1]
    tile = net._sasrec_tile(a.seq_len)
    pair = "tiled (tile %d)" % tile if tile else "resident"
    fwd_us, bwd_us, flop, byts = new_launches(net, f, tile)
    for tag, us, fl, by in (("forward", fwd_us, flop[0], byts[0]), ("backward", bwd_us, flop[1], byts[1])):
        print("sasrec %-8s launch alone, %s: %8.1f us   (%.2f GFLOP = %.1f us at %.0f TFLOP/s fp32; %.1f MB = %.1f us at "
              "%.0f TB/s)" % (tag, pair, us, fl / 1e9, fl / FP32_TFLOPS / 1e6, FP32_TFLOPS, by / 1e6, by / HBM_TBS / 1e6,
                              HBM_TBS))
    out["seq_len"], out["pair"] = a.seq_len, pair
    if a.long_histories and not tile:
        # both pairs admit the length: what tiling costs, medians of alternating regions of 30 launches
        tl = query("clsr_sasrec_tiled_default_tile", a.seq_len, net.D)
        res, til = new_launches(net, f, [0, tl], repeats=a.repeats)
        print("launches alone at seq_len %d, medians of %d alternating regions: forward resident %.1f us, tiled (tile %d) "
              "%.1f us (x %.2f); backward resident %.1f us, tiled %.1f us (x %.2f)"
              % (a.seq_len, a.repeats, res[0], tl, til[0], til[0] / res[0], res[1], til[1], til[1] / res[1]))
        out["resident_launches_us"] = dict(forward=round(res[0], 1), backward=round(res[1], 1))
        out["tiled_launches_us"] = dict(forward=round(til[0], 1), backward=round(til[1], 1), tile=tl)
    out["histories"], out["rows"] = a.histories, variants[1][1][0].last_shape[0]
    out["sasrec_launches_us"] = dict(forward=round(fwd_us, 1), backward=round(bwd_us, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
