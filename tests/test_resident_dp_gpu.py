"""Data parallelism with ``resident_data=True``: two rank processes on one GPU (host-staged collectives), a whole epoch
whose batches do not divide by the ranks -- every rank builds its own shard on the device, and the replicas end where
the host-fed replicas end, bit for bit."""
import copy
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _epoch_worker(rank, world, port, hp, train, flag, out):
    import random

    import torch.distributed as dist

    from clsr_amd.clsr import CLSRModel
    from clsr_amd.dp import HostStagedDist
    from clsr_amd.sequential_iterator import SASequentialIterator

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model = CLSRModel(hp, SASequentialIterator, seed=3, dist=HostStagedDist(dist), sync_bn=True, resident_data=flag)
    random.seed(11)
    it = model.iterator.load_data_from_file(train, batch_num_ngs=hp.train_num_ngs)
    loss = model.batch_train(it, model.sess)
    torch.cuda.synchronize()
    model.net.read_losses()      # (raises if a grid barrier of the fused heads timed out)
    sd = {k: v.detach().cpu().numpy() for k, v in model.net.state_dict().items()}
    out[rank] = dict(loss=float(loss), sd=sd, dropped=model.dp_dropped_positives, skipped=model.dp_skipped_batches,
                     resident=sorted(str(k) for k in model._static if "resident" in k),
                     host=sorted(str(k) for k in model._static if "resident" not in k), state=random.getstate())
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_epoch_from_resident_columns_matches_the_host_fed_epoch(golden_dir, golden_hparams):
    """600 lines in batches of 85 positives (odd: the sharding drops one per batch) and a last batch of 5 (two per rank)."""
    import torch.multiprocessing as mp

    train = os.path.join(golden_dir, "data", "train_data")
    hp = copy.deepcopy(golden_hparams)
    hp.batch_size = 85
    res = {}
    for flag in (False, True):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        ctx = mp.get_context("spawn")
        out = ctx.Manager().dict()
        mp.spawn(_epoch_worker, args=(2, port, hp, train, flag, out), nprocs=2, join=True)
        res[flag] = {r: out[r] for r in (0, 1)}
    for rank in (0, 1):
        off, on = res[False][rank], res[True][rank]
        assert on["resident"] and not on["host"] and off["host"] and not off["resident"]
        assert (on["dropped"], on["skipped"]) == (off["dropped"], off["skipped"]) == (8, 0)
        assert on["state"] == off["state"]
        assert np.isfinite(on["loss"])
        assert set(on["sd"]) == set(off["sd"])
        for k, v in off["sd"].items():
            np.testing.assert_array_equal(on["sd"][k], v, err_msg=k)
    for k, v in res[True][0]["sd"].items():
        np.testing.assert_array_equal(res[True][1]["sd"][k], v, err_msg=k)      # replicas stay bit-identical
