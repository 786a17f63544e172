#!/usr/bin/env python
"""Throughput of ``run_catalogue_eval``'s device path next to the scoring it wraps and to ``recommend_k_items``, CLSR and GRU4Rec.

Workload and protocol of scripts/recommend_throughput.py: synthetic requests (clsr_amd/synthetic.py) at CONFIGS["taobao"]'s
widths, ``T = 50``; a catalogue of 64 138 items (ids 1 .. 64 138); ``--requests`` 1024 requests, each with a target drawn from
the catalogue; seen items removed.  The planners' chunks: 8 requests x (1 target + 3 773 candidates) a pass for the ranks
(clsr_amd.recommend.plan_ranked), 8 x 3 773 for the recommendations (plan); 17 passes a request batch either way.

Four variants run in ONE process on one stream, each warmed up (allocation, plan recording, replay); then they take turns,
``--repeats`` timed regions each -- a region is the whole job, a device synchronise on both sides, host clock:

  (a) the new path: the request batch uploaded once, per chunk fill_ranked -> forward -> rank_count on the device
      (clsr_amd.recommend.count_catalogue), ``1 + partial.sum(1)`` and one synchronisation per request batch;
  (b) ``forward`` alone on a prebuilt device feed of (a)'s chunk shape, as many passes as the job has: the floor;
  (c) ``recommend_k_items(top_k=10)``'s loop on the same requests (clsr_amd.recommend.merge_catalogue), for context;
  (d) ``forward`` alone at (c)'s chunk shape: the floor of (c).

Reported per model: median, minimum and maximum per variant, requests/s and scored rows/s of (a), ``(a - b) / b`` -- what
fill_ranked and rank_count add to the scoring they wrap --, the same per pass in microseconds, ``(c - d) / d`` -- what fill and
merge add on the recommend path, measured in the same session -- and whether the first lies below the second.  The ranks of
the first two request batches are checked against ``recommend``'s lists: a target that is no seen item has ``rank <= 10``
exactly when it is entry ``rank - 1`` of its request's list.

    python scripts/catalogue_eval_throughput.py [--requests 1024] [--repeats 7]
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
from clsr_amd.recommend import count_catalogue, merge_catalogue, plan, plan_ranked  # noqa: E402
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
    def __init__(self, net, req, cat, n, c, gk):
        """``n`` requests a batch; ``c`` candidates a chunk of the ranks (group ``c + 1``); ``gk``: the recommend path's chunk."""
        self.net, self.req, self.cat, self.n, self.g, self.gk = net, req, cat, n, c + 1, gk
        self.N, self.M = req["users"].shape[0], len(cat)
        assert self.N % n == 0
        dev = net.device
        self.dev = cat.device(dev)
        self.t_items = torch.from_numpy(req["items"]).to(dev)
        self.t_cates = torch.from_numpy(req["cates"]).to(dev)
        tile = lambda a, g: np.tile(a[:g], n)
        self.fa = net.upload(host_feed(req, 0, n, self.g), False)
        self.fb = net.upload(host_feed(req, 0, n, self.g, tile(cat.items, self.g), tile(cat.cates, self.g)), False)
        self.fc = net.upload(host_feed(req, 0, n, gk), False)
        self.fd = net.upload(host_feed(req, 0, n, gk, tile(cat.items, gk), tile(cat.cates, gk)), False)
        self.partial = torch.empty(n, -(-c // ops.query("clsr_reco_rank_slab")), dtype=torch.int32, device=dev)
        self.t_score = torch.empty(n, dtype=torch.float32, device=dev)
        self.best_s = torch.empty(n, K, dtype=torch.float32, device=dev)
        self.best_i = torch.empty(n, K, dtype=torch.int32, device=dev)
        self.passes = (self.N // n) * -(-self.M // c)
        self.passes_k = (self.N // n) * -(-self.M // gk)

    def ranks(self, N=None):
        out = []
        for lo in range(0, N or self.N, self.n):
            self.net.upload(host_feed(self.req, lo, lo + self.n, self.g), False, into=self.fa)
            count_catalogue(self.net, self.fa, self.dev[0], self.dev[1], self.M, self.g, self.t_items[lo:lo + self.n],
                            self.t_cates[lo:lo + self.n], True, self.partial, self.t_score)
            out.append((self.partial.sum(1, dtype=torch.int32) + 1).cpu())
        return torch.cat(out)

    def lists(self, N=None):
        out = []
        for lo in range(0, N or self.N, self.n):
            self.net.upload(host_feed(self.req, lo, lo + self.n, self.gk), False, into=self.fc)
            merge_catalogue(self.net, self.fc, self.dev[0], self.dev[1], self.M, self.gk, K, True, self.best_s, self.best_i)
            out.append(self.best_i.cpu())
        return torch.cat(out)

    def floor(self, passes=None):
        for _ in range(passes or self.passes):
            self.net.forward(self.fb, False)

    def floor_k(self, passes=None):
        for _ in range(passes or self.passes_k):
            self.net.forward(self.fd, False)


def region(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def consistent(ranks, lists, req):
    """Requests checked / agreeing: the target is no seen item, and ``rank <= K`` iff it is entry ``rank - 1`` of the list."""
    checked = agree = 0
    for n in range(ranks.shape[0]):
        t = int(req["items"][n])
        if t in set(req["item_history"][n].tolist()):
            continue
        row, r = lists[n].tolist(), int(ranks[n])
        checked += 1
        agree += int((r <= K) == (t in row) and (r > K or row.index(t) == r - 1))
    return checked, agree


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
    gmax = ops.query("clsr_reco_max_chunk")
    n, c = plan_ranked(args.requests, M_ITEMS, gmax)
    nk, gk = plan(args.requests, M_ITEMS, gmax)
    assert n == nk, "both paths batch the same requests"
    N = max(2, args.requests // n) * n
    item2cate = np.concatenate([[0], cat.cates]).astype(np.int32)
    req = synthetic_feed(N, cfg["T"], cfg["Vu"], cfg["Vi"], cfg["Vc"], G=1, item2cate=item2cate)
    req["items"] = np.ascontiguousarray(np.clip(np.asarray(req["items"]).reshape(-1), 1, M_ITEMS), dtype=np.int32)
    req["cates"] = np.ascontiguousarray(item2cate[req["items"]], dtype=np.int32)
    stream = torch.cuda.Stream()
    for kind in args.models.split(","):
        net = make_net(kind, cfg, dims)
        with torch.cuda.stream(stream):
            job = Job(net, req, cat, n, c, gk)
            # warm-up on two request batches (twice: the second pass of a feed records its launch plan), and the check
            for _ in range(2):
                ranks = job.ranks(2 * n)
                job.floor(4)
                lists = job.lists(2 * n)
                job.floor_k(4)
            checked, agree = consistent(ranks.numpy(), lists.numpy(), req)
            times = {"a": [], "b": [], "c": [], "d": []}
            for _ in range(args.repeats):
                times["a"].append(region(job.ranks))
                times["b"].append(region(job.floor))
                times["c"].append(region(job.lists))
                times["d"].append(region(job.floor_k))
        med = {k: statistics.median(v) for k, v in times.items()}
        rows = N * M_ITEMS
        added, added_k = (med["a"] - med["b"]) / med["b"], (med["c"] - med["d"]) / med["d"]
        res = dict(model=kind, requests=N, catalogue=M_ITEMS, plan_ranks=[n, c], plan_lists=[nk, gk], passes=job.passes,
                   seconds={k: dict(median=round(med[k], 4), min=round(min(v), 4), max=round(max(v), 4))
                            for k, v in times.items()},
                   requests_per_s=dict(a=round(N / med["a"], 1), c=round(N / med["c"], 1)),
                   rows_per_s=dict(a=round(rows / med["a"]), b=round(job.passes * n * (c + 1) / med["b"]), c=round(rows / med["c"])),
                   added_over_scoring=dict(ranks=round(added, 4), lists=round(added_k, 4)),
                   added_us_per_pass=dict(ranks=round(1e6 * (med["a"] - med["b"]) / job.passes, 1),
                                          lists=round(1e6 * (med["c"] - med["d"]) / job.passes_k, 1)),
                   ranks_add_less_than_lists=bool(added < added_k),
                   mean_rank=round(float(ranks.double().mean()), 1), requests_checked=checked, requests_agreeing=agree)
        print(json.dumps(res), flush=True)
        del job, net
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
