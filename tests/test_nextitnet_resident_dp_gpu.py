"""NextItNet data parallelism with ``resident_data=True``: two rank processes on one GPU (host-staged collectives), a whole
epoch whose batches do not divide by the ranks -- every rank builds its own shard on the device from ``(sel, psrc)``, whose
``psrc`` points anywhere in the global batch, and the replicas end where the host-fed replicas end, bit for bit."""
import copy
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RANK_TIMEOUT_S = 240


def _epoch_worker(rank, world, port, hp, train, it_name, flag, out):
    import random

    import torch
    import torch.distributed as dist

    import clsr_amd.sequential_iterator as I
    from clsr_amd.clsr import NextItNetModel
    from clsr_amd.dp import HostStagedDist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model = NextItNetModel(hp, getattr(I, it_name), seed=3, dist=HostStagedDist(dist), sync_bn=True, resident_data=flag)
    random.seed(11)
    it = model.iterator.load_data_from_file(train, batch_num_ngs=hp.train_num_ngs)
    loss = model.batch_train(it, model.sess)
    torch.cuda.synchronize()
    model.net.read_losses()
    sd = {k: v.detach().cpu().numpy() for k, v in model.net.state_dict().items()}
    out[rank] = dict(loss=float(loss), sd=sd, dropped=model.dp_dropped_positives, skipped=model.dp_skipped_batches,
                     resident=sorted(str(k) for k in model._static if "resident" in k),
                     host=sorted(str(k) for k in model._static if "resident" not in k), state=random.getstate())
    dist.barrier()
    dist.destroy_process_group()


def _two_ranks(hp, train, it_name, flag):
    """Both ranks as processes of their own, each under its own time limit; a rank that fails or overstays ends the other
    and the test -- nothing further is started."""
    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    procs = [ctx.Process(target=_epoch_worker, args=(r, 2, port, hp, train, it_name, flag, out)) for r in (0, 1)]
    for p in procs:
        p.start()
    codes = []
    for p in procs:
        p.join(RANK_TIMEOUT_S)
        codes.append(p.exitcode)
    for p in procs:
        if p.is_alive():
            p.kill()
            p.join()
    assert codes == [0, 0], "rank exit codes %r (None: over its %d s limit) for %s, resident_data=%s" % (
        codes, RANK_TIMEOUT_S, it_name, flag)
    return {r: out[r] for r in (0, 1)}


def test_two_rank_epoch_from_resident_columns_matches_the_host_fed_epoch(golden_dir, golden_hparams):
    """600 lines in batches of 85 positives (odd: the sharding drops one per batch) and a last batch of 5 (two per rank).
    The host-fed epoch of the literal iterator runs first; the recipe-fed one is started only when it succeeded."""
    train = os.path.join(golden_dir, "data", "train_data")
    hp = copy.deepcopy(golden_hparams)
    for k, v in dict(model_type="NextItNet", user_embedding_dim=16, dilations=[1, 2, 4], kernel_size=3, batch_size=85,
                     show_step=10 ** 9).items():
        setattr(hp, k, v)
    off = _two_ranks(hp, train, "NextItNetIterator", False)
    on = _two_ranks(hp, train, "NextItNetColumnIterator", True)
    for rank in (0, 1):
        a, b = off[rank], on[rank]
        assert b["resident"] and not b["host"] and a["host"] and not a["resident"]
        assert (b["dropped"], b["skipped"]) == (a["dropped"], a["skipped"]) == (8, 0)
        assert b["state"] == a["state"]
        assert np.isfinite(b["loss"])
        assert set(b["sd"]) == set(a["sd"])
        for k, v in a["sd"].items():
            np.testing.assert_array_equal(b["sd"][k], v, err_msg=k)
    for k, v in on[0]["sd"].items():
        np.testing.assert_array_equal(on[1]["sd"][k], v, err_msg=k)      # replicas stay bit-identical
