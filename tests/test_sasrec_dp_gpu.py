"""Data-parallel SASRec: two ranks on one GPU (collectives staged through gloo on the host, as in tests/test_dp_gpu.py)
reproduce the single-process step on the global batch -- losses, every dense gradient (the encoder's among them, the rows of
the positional table included), the gradients of both tables and their clip norms -- with the tables exchanged as row lists
(``sparse_tables="all"``) and in the dense all-reduce (``"none"``).  Pattern, process count and tolerances of
tests/test_ncf_dp_gpu.py."""
import os
import pickle
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sasrec_oracle as O  # noqa: E402
from clsr_amd.dp import HostStagedDist as _HostStagedDist  # noqa: E402


def _worker(rank, world, port, hp, dims, feed, sd, sparse, out):
    import torch.distributed as dist

    from clsr_amd.dp import DataParallel, shard_feed
    from clsr_amd.seqnet import SeqNet

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    net = SeqNet(hp, dims, kind="sasrec", device="cuda:0", seed=rank)      # different seeds: the broadcast must fix that
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
        out["sparse"] = list(dp.last_sparse)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("sparse", ["all", "none"])
def test_sasrec_two_ranks_match_single_process(golden_dir, golden_hparams, sparse):
    import torch.multiprocessing as mp

    from clsr_amd.seqnet import SeqNet

    hp = O.hparams(golden_hparams)
    dims = dict(Vu=len(pickle.load(open(hp.user_vocab, "rb"))), Vi=len(pickle.load(open(hp.item_vocab, "rb"))),
                Vc=len(pickle.load(open(hp.cate_vocab, "rb"))))
    g = np.load(os.path.join(golden_dir, "iterator_train_sa.npz"))
    feed = {k[3:]: g[k] for k in g.files if k.startswith("b0_")}
    params = O.init_params(dims, hp, **O.FIXTURE)
    sd = dict(params)
    sd.update(O.init_bn_state(params))
    single = SeqNet(hp, dims, kind="sasrec", device="cuda:0", seed=0)
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
    mp.spawn(_worker, args=(2, port, hp, dims, feed, sd, sparse, out), nprocs=2, join=True)
    assert sorted(out["sparse"]) == (sorted(single.tables) if sparse == "all" else [])
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
