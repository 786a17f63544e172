#!/usr/bin/env python
"""Throughput of ``recommend_k_items``' device path next to what the scoring path offered before it, CLSR and GRU4Rec.

Workload: synthetic requests (clsr_amd/synthetic.py) at CONFIGS["taobao"]'s widths, ``T = 50``; a catalogue of 64 138 items
(ids 1 .. 64 138, the item count of scripts/lgn_step_time.py); ``--requests`` 1024 requests; ``top_k = 10``; seen items
removed.  The planner's chunks (clsr_amd.recommend.plan: 8 requests x 3 773 candidates a pass, 17 passes a request batch).

Three variants do the same job in ONE process on one stream, each warmed up (allocation, plan recording, replay); then they
take turns, ``--repeats`` timed regions each -- a region is the whole job, a device synchronise on both sides, host clock:

  (a) the new path: the request batch uploaded once, per chunk fill -> forward -> merge on the device
      (clsr_amd.recommend.merge_catalogue), one synchronisation per request batch;
  (b) the same chunks as host arrays through ``net.upload`` and ``forward``, the logits collected into an [n, M] matrix on
      the device, seen ids masked with torch, ``torch.topk``, one synchronisation per request batch;
  (c) ``forward`` alone on a prebuilt device feed of the chunk shape, as many passes as the job has: the floor the existing
      scoring kernels set.

Reported per model: median, minimum and maximum per variant, requests/s and scored rows/s of (a) and (b), ``(a - c) / c`` --
what fill and merge add to the scoring they wrap -- and whether (a) is slower than (b) beyond the spread of the regions.
The ids of (a) and (b) are compared for every request whose 11 best scores in (b) are distinct (``torch.topk`` fixes no
order among equal scores).

    python scripts/recommend_throughput.py [--requests 1024] [--repeats 7]
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

from bench import build_hparams  # noqa: E402
from clsr_amd import ops  # noqa: E402
from clsr_amd.catalogue import Catalogue  # noqa: E402
from clsr_amd.net import CLSRNet  # noqa: E402
from clsr_amd.recommend import merge_catalogue, plan  # noqa: E402
from clsr_amd.seqnet import SeqNet  # noqa: E402
from clsr_amd.synthetic import CONFIGS, synthetic_feed  # noqa: E402

M_ITEMS, K = 64138, 10
HIST = ("item_history", "item_cate_history", "mask", "time_from_first_action", "time_to_now")


def make_net(kind, cfg, dims):
    if kind == "clsr":
        return CLSRNet(build_hparams(cfg, cfg["P"]), dims, device="cuda:0", seed=0)
    hp = build_hparams(cfg, cfg["P"], model_type=kind, layer_sizes=[100, 64])
    return SeqNet(hp, dims, kind=kind, device="cuda:0", seed=0)


def host_feed(req, lo, hi, g, items=None, cates=None):
    n = hi - lo
    feed = {k: req[k][lo:hi] for k in HIST}
    feed["users"] = req["users"][lo:hi]
    feed["items"] = np.zeros(n * g, dtype=np.int32) if items is None else items
    feed["cates"] = np.zeros(n * g, dtype=np.int32) if cates is None else cates
    feed["labels"] = np.zeros(n * g, dtype=np.float32)
    feed["hist_group"] = g
    return feed


class Job(object):
    def __init__(self, net, req, cat, n, g):
        self.net, self.req, self.cat, self.n, self.g = net, req, cat, n, g
        self.N, self.M = req["users"].shape[0], len(cat)
        assert self.N % n == 0
        self.dev = cat.device(net.device)
        self.fa = net.upload(host_feed(req, 0, n, g), False)
        self.fb = net.upload(host_feed(req, 0, n, g), False)
        self.fc = net.upload(host_feed(req, 0, n, g, np.tile(cat.items[:g], n), np.tile(cat.cates[:g], n)), False)
        self.best_s = torch.empty(n, K, dtype=torch.float32, device=net.device)
        self.best_i = torch.empty(n, K, dtype=torch.int32, device=net.device)
        self.logits = torch.empty(n, self.M, dtype=torch.float32, device=net.device)
        self.pad_i, self.pad_c = np.zeros(g, dtype=np.int32), np.zeros(g, dtype=np.int32)
        self.passes = (self.N // n) * -(-self.M // g)

    def new_path(self, N=None):
        out = []
        for lo in range(0, N or self.N, self.n):
            self.net.upload(host_feed(self.req, lo, lo + self.n, self.g), False, into=self.fa)
            merge_catalogue(self.net, self.fa, self.dev[0], self.dev[1], self.M, self.g, K, True, self.best_s, self.best_i)
            out.append(self.best_i.cpu())
        return torch.cat(out)

    def host_path(self, k=K, N=None):
        n, g, M, cat = self.n, self.g, self.M, self.cat
        out_i, out_s = [], []
        for lo in range(0, N or self.N, n):
            for c0 in range(0, M, g):
                nv = min(g, M - c0)
                ci, cc = cat.items[c0:c0 + g], cat.cates[c0:c0 + g]
                if nv < g:
                    ci, cc = self.pad_i.copy(), self.pad_c.copy()
                    ci[:nv], cc[:nv] = cat.items[c0:], cat.cates[c0:]
                self.net.upload(host_feed(self.req, lo, lo + n, g, np.tile(ci, n), np.tile(cc, n)), False, into=self.fb)
                logit = self.net.forward(self.fb, False)["logit"]
                self.logits[:, c0:c0 + nv] = logit.view(n, g)[:, :nv]
            seen = (self.dev[0].view(1, M, 1) == self.fb["item_history"].view(n, 1, -1)).any(-1)
            top = torch.topk(self.logits.masked_fill(seen, float("-inf")), k, dim=1)
            out_i.append(self.dev[0][top.indices].cpu())
            out_s.append(top.values.cpu())
        return torch.cat(out_i), torch.cat(out_s)

    def floor(self, passes=None):
        for _ in range(passes or self.passes):
            self.net.forward(self.fc, False)


def region(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--models", default="clsr,gru4rec")
    args = ap.parse_args()
    cfg = dict(CONFIGS["taobao"], Vi=M_ITEMS + 1)
    dims = dict(Vu=cfg["Vu"], Vi=cfg["Vi"], Vc=cfg["Vc"])
    rng = np.random.default_rng(7)
    cat = Catalogue(np.arange(1, M_ITEMS + 1, dtype=np.int32), rng.integers(1, cfg["Vc"], M_ITEMS).astype(np.int32),
                    n_items=cfg["Vi"])
    n, g = plan(args.requests, M_ITEMS, ops.query("clsr_reco_max_chunk"))
    N = max(2, args.requests // n) * n
    item2cate = np.concatenate([[0], cat.cates]).astype(np.int32)
    req = synthetic_feed(N, cfg["T"], cfg["Vu"], cfg["Vi"], cfg["Vc"], G=1, item2cate=item2cate)
    stream = torch.cuda.Stream()
    for kind in args.models.split(","):
        net = make_net(kind, cfg, dims)
        with torch.cuda.stream(stream):
            job = Job(net, req, cat, n, g)
            # warm-up on two request batches (twice: the second pass of a feed records its launch plan), and the ids
            for _ in range(2):
                ids_a = job.new_path(2 * n)
                job.floor(4)
                ids_b, val_b = job.host_path(K + 1, 2 * n)
            distinct = (val_b[:, :-1] > val_b[:, 1:]).all(1)
            same = bool((ids_a[distinct] == ids_b[distinct][:, :K]).all())
            times = {"a": [], "b": [], "c": []}
            for _ in range(args.repeats):
                times["a"].append(region(job.new_path))
                times["b"].append(region(job.host_path))
                times["c"].append(region(job.floor))
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = max(max(v) - min(v) for v in (times["a"], times["b"]))
        rows = N * M_ITEMS
        res = dict(model=kind, requests=N, catalogue=M_ITEMS, top_k=K, plan=[n, g], passes=job.passes,
                   seconds={k: dict(median=round(med[k], 4), min=round(min(v), 4), max=round(max(v), 4))
                            for k, v in times.items()},
                   requests_per_s=dict(a=round(N / med["a"], 1), b=round(N / med["b"], 1)),
                   rows_per_s=dict(a=round(rows / med["a"]), b=round(rows / med["b"]), c=round(job.passes * n * g / med["c"])),
                   added_over_scoring=round((med["a"] - med["c"]) / med["c"], 4),
                   a_not_slower_than_b=bool(med["a"] <= med["b"] + spread),
                   ids_checked=int(distinct.sum()), ids_skipped_for_ties=int((~distinct).sum()), ids_equal=same)
        print(json.dumps(res), flush=True)
        del job, net
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
