"""Data-parallel step with the non-Adam optimisers (csrc/optim_tf.hip): two ranks on one GPU over the host-staged
transport, touched-row exchange of every table (sparse_tables="all"), against the single-process step on the global
batch."""
import copy
import os
import pickle
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from clsr_amd.dp import HostStagedDist  # noqa: E402


def _worker(rank, world, port, hp, dims, feed, sd, out):
    import torch.distributed as dist

    from clsr_amd.dp import DataParallel, shard_feed
    from clsr_amd.net import CLSRNet

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    net = CLSRNet(hp, dims, device="cuda:0", seed=rank)  # different seeds: the broadcast must fix that
    if rank == 0:
        net.load_state_dict(sd)
    dp = DataParallel(net, HostStagedDist(dist), sync_bn=True, sparse_tables="all")
    for b in range(2):
        f = dp.prepare(net.upload(shard_feed(feed[b], rank, world, hp.train_num_ngs + 1), True))
        dp.train_step(f)
    torch.cuda.synchronize()
    if rank == 0:
        out["state"] = {k: v.numpy() for k, v in net.state_dict().items()}
        out["sparse"] = list(dp.last_sparse)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("name", ["adagrad", "ftrl"])
def test_two_ranks_match_single_process(golden_dir, golden_hparams, name):
    import torch.multiprocessing as mp

    from clsr_amd.net import CLSRNet
    from oracle import clsr_oracle as O

    hp = copy.deepcopy(golden_hparams)
    hp.optimizer = name
    dims = dict(Vu=len(pickle.load(open(hp.user_vocab, "rb"))), Vi=len(pickle.load(open(hp.item_vocab, "rb"))),
                Vc=len(pickle.load(open(hp.cate_vocab, "rb"))))
    g = np.load(os.path.join(golden_dir, "iterator_train_sa.npz"))
    feeds = [{k[3:]: g[k] for k in g.files if k.startswith("b%d_" % b)} for b in range(2)]
    params = O.init_params(dims, hp, seed=5, scale_dense=8.0)
    sd = dict(params)
    sd.update(O.init_bn_state(params))
    single = CLSRNet(hp, dims, device="cuda:0", seed=0)
    with pytest.warns(UserWarning):      # (no slots in the payload: they start from their initial values)
        single.load_state_dict(sd)
    for fd in feeds:
        single.train_step(single.upload(fd, True))
    torch.cuda.synchronize()
    ref = single.state_dict()

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    mp.spawn(_worker, args=(2, port, hp, dims, feeds, sd, out), nprocs=2, join=True)
    assert len(out["sparse"]) == 4
    got = out["state"]
    assert set(got) == set(ref)
    for k, v in ref.items():
        v = v.numpy()
        scale = float(np.abs(v).max()) + 1e-12
        d = np.abs(got[k] - v)
        # gradients of the global batch agree to fp32 accumulation noise; the updates follow them
        assert float(d.max()) <= 1e-4 * scale + 1e-6, (name, k, float(d.max()), scale)
