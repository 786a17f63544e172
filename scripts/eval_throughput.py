#!/usr/bin/env python
"""Throughput of the scoring / evaluation path: CLSRModel.run_weighted_eval and predict on a synthetic test
file with 1 + 99 lines per positive (the reference's test protocol).   python scripts/eval_throughput.py [n_pos]
[--shard_eval] [--resident_eval] [--model NAME] [--json PATH] [--tag TEXT] [--no_predict]

--model NAME: CLSRModel (default, config/clsr.yaml, SASequentialIterator) or A2SVDModel (config/asvd.yaml,
SequentialIterator).  --resident_eval builds the model with ``resident_eval=True`` and reports, beside the passes, the
one-time cost (image upload + the flag launch, host clock around a synchronise), the bytes resident and the two new
launches alone by device events.  --json PATH appends one line with every figure printed (and ``--tag TEXT``: which tree
ran); --no_predict stops before the ``predict`` pass.

--shard_eval measures the sharded evaluation path at a world of one (``shard_eval=True`` over a one-rank host-staged
process group: the partial kernels, one reduce, the finalize launches) -- its overhead against the default path.

CLSR_EVAL_WEIGHTED=wauc adds ``wauc`` to the metrics of config/clsr.yaml (which requests no user-weighted metric);
CLSR_EVAL_WEIGHTED=all requests all four (wauc, wmrr, whit@k, wndcg@k) on a user vocabulary above 2^18 (400 000 train
lines over 10^6 users instead of 4 096 over 20 000)."""
import cProfile
import json
import os
import pstats
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import clsr_amd.clsr as models  # noqa: E402
from clsr_amd.deeprec_utils import prepare_hparams  # noqa: E402
from clsr_amd.sequential_iterator import SASequentialIterator, SequentialIterator  # noqa: E402
from clsr_amd.synthetic import make_tsv_dataset  # noqa: E402

MODELS = {"CLSRModel": ("clsr.yaml", SASequentialIterator), "A2SVDModel": ("asvd.yaml", SequentialIterator)}


def _option(args, name):
    """Remove ``name VALUE`` from ``args``; the value or None."""
    if name not in args:
        return None
    i = args.index(name)
    value = args[i + 1]
    del args[i:i + 2]
    return value


def _launches_alone(model, infile):
    """Device time of clsr_feed_same_rows over the whole file and of clsr_feed_build_eval per chunk, by events, back to
    back on an idle device: (same_rows ms, [build ms per chunk of the plan], n_chunks)."""
    import torch

    from clsr_amd import ops
    from clsr_amd.resident import eval_chunk_plan

    with model._stream_ctx():
        lines = model._resident_eval.get(infile, model.min_seq_length)
        rc = lines.rc
        plan = eval_chunk_plan(lines.flags, lines.n_keep, model.iterator.batch_size,
                               int(os.environ.get("CLSR_EVAL_ROWS", "32768")), model._dedup)
        flags = torch.empty(lines.n_keep, dtype=torch.uint8, device=model.net.device)
        ptrs = ops.feed_eval_pointers(rc.dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        for timed in (False, True):         # (the first round warms the code objects and the arenas)
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(10):
                ops.feed_same_rows(ptrs, rc.N, lines.keep_dev, lines.n_keep, rc.T, flags)
            ev[1].record()
            feeds = {}
            for k0, n, g in plan:
                feeds[(n, g)] = model.net.build_eval_feed(lines, k0, n, g, into=feeds.get((n, g)))
            torch.cuda.synchronize()
            ev[2].record()
            for _ in range(10):
                for k0, n, g in plan:
                    model.net.build_eval_feed(lines, k0, n, g, into=feeds[(n, g)])
            ev[3].record()
            torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / 10, ev[2].elapsed_time(ev[3]) / 10, len(plan)


def main():
    args = [a for a in sys.argv[1:] if a not in ("--shard_eval", "--resident_eval", "--no_predict")]
    shard, resident, no_predict = ("--" + k in sys.argv[1:] for k in ("shard_eval", "resident_eval", "no_predict"))
    name, json_path, tag = _option(args, "--model") or "CLSRModel", _option(args, "--json"), _option(args, "--tag")
    if name not in MODELS:
        raise SystemExit("--model: one of %s" % ", ".join(MODELS))
    n_pos = int(args[0]) if args else 2000
    mode = os.environ.get("CLSR_EVAL_WEIGHTED", "")
    if mode not in ("", "wauc", "all"):
        raise SystemExit("CLSR_EVAL_WEIGHTED: wauc or all")
    full = mode == "all"
    d = "/tmp/clsr_eval_tsv" + ("_full" if full else "")
    paths = make_tsv_dataset(d, n_users=10 ** 6 if full else 20000, n_items=60000, n_cates=4000,
                             n_train=400000 if full else 4096, n_valid=64, n_test=n_pos, test_ngs=99, max_hist=70)
    extra = {"": {}, "wauc": dict(weighted_metrics=["wauc"]),
             "all": dict(weighted_metrics=["wauc", "wmrr", "whit@1;2;5;10", "wndcg@1;2;5;10"])}[mode]
    hp = prepare_hparams(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "clsr_amd",
                                      "config", MODELS[name][0]),
                         user_vocab=paths["user_vocab"], item_vocab=paths["item_vocab"],
                         cate_vocab=paths["category_vocab"], max_seq_length=50, batch_size=4000, train_num_ngs=4,
                         time_unit="s", contrastive_loss="triplet", contrastive_length_threshold=5, is_clip_norm=1,
                         embed_l2=1e-6, layer_l2=1e-6, discrepancy_loss_weight=0.01, contrastive_loss_weight=0.1,
                         show_step=10 ** 9, save_model=False, MODEL_DIR=None, epochs=1, **extra)
    kw = {}
    if shard:
        import socket

        import torch.distributed as dist

        from clsr_amd.dp import HostStagedDist

        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(s.getsockname()[1]))
        s.close()
        dist.init_process_group("gloo", rank=0, world_size=1)
        kw = dict(dist=HostStagedDist(dist), shard_eval=True)
    if resident:
        kw["resident_eval"] = True
    model = getattr(models, name)(hp, MODELS[name][1], seed=0, **kw)
    print("%s, user vocabulary: %d, weighted metrics: %s" % (name, model.user_vocab_length, hp.weighted_metrics))
    rows = n_pos * 100
    out = {"tag": tag, "model": name, "resident_eval": resident, "shard_eval": shard, "weighted": mode, "rows": rows}
    t = time.perf_counter()
    if resident:
        import torch

        # parse first, so that the one-time cost of the store is timed apart from the parser
        model.iterator.eval_lines(paths["test_data"], model.min_seq_length)
        out["parse_s"] = time.perf_counter() - t
        t1 = time.perf_counter()
        with model._stream_ctx():
            model._resident_eval.get(paths["test_data"], model.min_seq_length)
            torch.cuda.synchronize()
        out["store_s"], out["store_bytes"] = time.perf_counter() - t1, model._resident_eval.nbytes
        print("resident_eval store: %.3f s once (image upload + flag launch + read-back), %d bytes resident"
              % (out["store_s"], out["store_bytes"]))
    res = model.run_weighted_eval(paths["test_data"], num_ngs=99)
    out["first_pass_s"] = time.perf_counter() - t
    print("first pass (parses the file): %.2f s  %s" % (out["first_pass_s"], res))
    dts = []
    for _ in range(3):
        t = time.perf_counter()
        res2 = model.run_weighted_eval(paths["test_data"], num_ngs=99)
        dts.append(time.perf_counter() - t)
        assert res2 == res
    dt = min(dts)
    out["passes_s"], out["rows_per_s"] = dts, [rows / x for x in dts]
    print("run_weighted_eval%s: %.3f s for %d rows = %.0f rows/s (best of %s)" % (
        " (shard_eval, one rank)" if shard else "", dt, rows, rows / dt, " ".join("%.3f" % x for x in dts)))

    def dump():
        if json_path:
            with open(json_path, "a") as f:
                f.write(json.dumps(out) + "\n")

    if shard:
        assert model.eval_rows_scored == rows
        return dump()
    t = time.perf_counter()
    n = sum(1 for f in model.iterator.load_data_from_file(paths["test_data"], batch_num_ngs=0) if f)
    out["iterator_alone_s"] = time.perf_counter() - t
    print("  iterator alone: %.3f s (%d batches)" % (out["iterator_alone_s"], n))
    if resident:
        out["same_rows_ms"], out["build_eval_ms_per_pass"], out["chunks"] = _launches_alone(model, paths["test_data"])
        print("  launches alone: clsr_feed_same_rows %.3f ms (whole file), clsr_feed_build_eval %.3f ms for the %d chunks of "
              "a pass" % (out["same_rows_ms"], out["build_eval_ms_per_pass"], out["chunks"]))
    dump()
    if no_predict:
        return
    t = time.perf_counter()
    model.predict(paths["test_data"], os.path.join(d, "pred.txt"))
    dt = time.perf_counter() - t
    print("predict: %.3f s = %.0f rows/s" % (dt, rows / dt))
    if os.environ.get("CLSR_PROFILE"):
        cProfile.runctx("model.run_weighted_eval(paths['test_data'], num_ngs=99)", globals(), locals(), "/tmp/ev.prof")
        pstats.Stats("/tmp/ev.prof").sort_stats("cumtime").print_stats(18)


if __name__ == "__main__":
    main()
