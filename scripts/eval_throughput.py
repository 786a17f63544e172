#!/usr/bin/env python
"""Throughput of the scoring / evaluation path: CLSRModel.run_weighted_eval and predict on a synthetic test
file with 1 + 99 lines per positive (the reference's test protocol).   python scripts/eval_throughput.py [n_pos]
[--shard_eval]

--shard_eval measures the sharded evaluation path at a world of one (``shard_eval=True`` over a one-rank host-staged
process group: the partial kernels, one reduce, the finalize launches) -- its overhead against the default path.

CLSR_EVAL_WEIGHTED=wauc adds ``wauc`` to the metrics of config/clsr.yaml (which requests no user-weighted metric);
CLSR_EVAL_WEIGHTED=all requests all four (wauc, wmrr, whit@k, wndcg@k) on a user vocabulary above 2^18 (400 000 train
lines over 10^6 users instead of 4 096 over 20 000)."""
import cProfile
import os
import pstats
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clsr_amd.clsr import CLSRModel  # noqa: E402
from clsr_amd.deeprec_utils import prepare_hparams  # noqa: E402
from clsr_amd.sequential_iterator import SASequentialIterator  # noqa: E402
from clsr_amd.synthetic import make_tsv_dataset  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if a != "--shard_eval"]
    shard = len(args) != len(sys.argv) - 1
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
                                      "config", "clsr.yaml"),
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
    model = CLSRModel(hp, SASequentialIterator, seed=0, **kw)
    print("user vocabulary: %d, weighted metrics: %s" % (model.user_vocab_length, hp.weighted_metrics))
    rows = n_pos * 100
    t = time.perf_counter()
    res = model.run_weighted_eval(paths["test_data"], num_ngs=99)
    print("first pass (parses the file): %.2f s  %s" % (time.perf_counter() - t, res))
    dts = []
    for _ in range(3):
        t = time.perf_counter()
        res2 = model.run_weighted_eval(paths["test_data"], num_ngs=99)
        dts.append(time.perf_counter() - t)
        assert res2 == res
    dt = min(dts)
    print("run_weighted_eval%s: %.3f s for %d rows = %.0f rows/s (best of %s)" % (
        " (shard_eval, one rank)" if shard else "", dt, rows, rows / dt, " ".join("%.3f" % x for x in dts)))
    if shard:
        assert model.eval_rows_scored == rows
        return
    t = time.perf_counter()
    n = sum(1 for f in model.iterator.load_data_from_file(paths["test_data"], batch_num_ngs=0) if f)
    print("  iterator alone: %.3f s (%d batches)" % (time.perf_counter() - t, n))
    t = time.perf_counter()
    model.predict(paths["test_data"], os.path.join(d, "pred.txt"))
    dt = time.perf_counter() - t
    print("predict: %.3f s = %.0f rows/s" % (dt, rows / dt))
    if os.environ.get("CLSR_PROFILE"):
        cProfile.runctx("model.run_weighted_eval(paths['test_data'], num_ngs=99)", globals(), locals(), "/tmp/ev.prof")
        pstats.Stats("/tmp/ev.prof").sort_stats("cumtime").print_stats(18)


if __name__ == "__main__":
    main()
