"""Data-parallel SASRec with ``long_histories=True`` at ``max_seq_length = 120`` (the tiled kernels of csrc/sasrec.hip): two
ranks on one GPU reproduce the single-process step on the global batch -- losses, every dense gradient (the encoder's among
them), the gradients of both tables and their clip norms.  Pattern, process count and tolerances of
tests/test_sasrec_dp_gpu.py."""
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sasrec_cases as K  # noqa: E402
import sasrec_oracle as O  # noqa: E402
from clsr_amd.dp import HostStagedDist as _HostStagedDist  # noqa: E402

T = 120
DIMS = dict(Vu=8, Vi=60, Vc=9)
LENS = (1, T, 64, 65)


def _worker(rank, world, port, hp, dims, feed, sd, sparse, out):
    import torch.distributed as dist

    from clsr_amd.dp import DataParallel, shard_feed
    from clsr_amd.seqnet import SeqNet

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    net = SeqNet(hp, dims, kind="sasrec", device="cuda:0", seed=rank, long_histories=True)
    if rank == 0:
        net.load_state_dict(sd)
    dp = DataParallel(net, _HostStagedDist(dist), sync_bn=True, sparse_tables=sparse)
    net.capture_grads = True
    dp.train_step(dp.prepare(net.upload(shard_feed(feed, rank, world, hp.train_num_ngs + 1), True)))
    torch.cuda.synchronize()
    if rank == 0:
        out["grads"] = {k: v.cpu().numpy() for k, v in net.captured["dense"].items()}
        out["tgrads"] = {k: v.cpu().numpy() for k, v in net.captured["tables"].items()}
        out["sumsq"] = net.captured["table_sumsq"].cpu().numpy()
        out["losses"] = net.read_losses()
        out["tiled"] = any(k[0] == "sa.tws.train" for k in net._bufs)
    dist.barrier()
    dist.destroy_process_group()


def test_sasrec_two_ranks_match_single_process(golden_hparams):
    import torch.multiprocessing as mp

    from clsr_amd.seqnet import SeqNet

    hp = O.hparams(golden_hparams, max_seq_length=T, train_num_ngs=4)
    feed = K.edge_feed(T, 5, DIMS["Vi"], DIMS["Vc"], LENS, seed=3)
    params = O.init_params(DIMS, hp, **O.FIXTURE)
    sd = dict(params)
    sd.update(O.init_bn_state(params))
    single = SeqNet(hp, DIMS, kind="sasrec", device="cuda:0", seed=0, long_histories=True)
    assert single._sasrec_tile(T) > 0
    single.load_state_dict(sd)
    single.capture_grads = True
    single.train_step(single.upload(feed, True))
    torch.cuda.synchronize()
    ref_losses = single.read_losses()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    mp.spawn(_worker, args=(2, port, hp, DIMS, feed, sd, "all", out), nprocs=2, join=True)
    assert out["tiled"]
    for k in ("loss", "data_loss", "regular_loss"):
        assert abs(out["losses"][k] - ref_losses[k]) < 1e-5 * max(1.0, abs(ref_losses[k])), (k, out["losses"], ref_losses)
    ref_g = {k: v.cpu().numpy() for k, v in single.captured["dense"].items()}
    assert set(O.encoder_names(int(hp.num_blocks))) <= set(ref_g)
    floor = 4e-6 * max(float(np.abs(v).max()) for v in ref_g.values())
    for k, v in ref_g.items():
        d = np.abs(out["grads"][k] - v)
        assert float(d.max()) <= 2e-3 * float(np.abs(v).max()) + floor, (k, float(d.max()), float(np.abs(v).max()))
    assert set(single.captured["tables"]) == set(O.TABLES)
    for k, v in single.captured["tables"].items():
        v = v.cpu().numpy()
        assert float(np.abs(v).max()) > 0, k
        assert float(np.abs(out["tgrads"][k] - v).max()) <= 2e-3 * float(np.abs(v).max()), k
    ref_ss = single.captured["table_sumsq"].cpu().numpy()
    assert np.all(ref_ss[:4] > 0) and np.allclose(out["sumsq"][:4], ref_ss[:4], rtol=1e-4, atol=0)
