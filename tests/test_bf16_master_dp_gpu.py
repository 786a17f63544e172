"""Data-parallel step on bf16 tables with an fp32 master (``CLSRNet(table_dtype="bf16", table_master=True)``): two ranks
on one GPU over the host-staged transport, touched-row exchange of every table (sparse_tables="all"), against the
single-process step on the global batch.  The exchange carries gradients and the update is local, so the only thing the
master adds to data parallelism is that the residual tables are broadcast with the other variables.

Every key of rank 0's checkpoint (merged fp32 masters, dense variables, moments, BN statistics) is compared with the single-
process net's at ``1e-4 * scale + 1e-6``, the bar of tests/test_optimizers_dp_gpu.py -- except the variables that Adam drives
by summation noise alone, which get a bound of their own.  Those are the ``b_nn_layer*`` biases and the ``b_nn_output`` of the
two attention MLPs and of logit_fcn: each sits in front of a batch norm or of a softmax (attention weights, the softmax data
loss over a group), so its true gradient is zero; what reaches it
is fp32 summation noise, Adam normalises that to steps of a fraction of lr with the sign of the noise, and two ranks sum in
another order than one process.  The moving mean of logit_fcn's first batch norm follows its bias.  Bound for these: either
side moves such an element by at most lr per step, so the two differ by at most 2 * lr * steps.  Measured on one MI355X after
these two steps, the same for fp32 tables, bf16 tables and bf16 tables with a master (so not an effect of the master):
logit_fcn b_nn_layer0 off by 4.3e-4 to 5.5e-4, b_nn_layer1 3.6e-5 to 8.2e-5, the other biases 1e-6 to 4.1e-5, that moving mean
1.1e-5 to 1.7e-5; every other key stays below a fifth of the bar.  (tests/test_dp_gpu.py,
test_model_train_with_two_ranks_matches_single_process, describes the same effect for the item table over more steps.)"""
import copy
import hashlib
import os
import pickle
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from clsr_amd.dp import HostStagedDist  # noqa: E402

LOGIT_BN0_MEAN = "sequential/logit_fcn/nn_part/batch_normalization/moving_mean"


def _digest(net):
    h = hashlib.sha1()
    for k in sorted(net.tab_lo):
        h.update(net.tab_lo[k].cpu().numpy().tobytes())
        h.update(net.tables[k].view(torch.int16).cpu().numpy().tobytes())
    return h.hexdigest()


def _worker(rank, world, port, hp, dims, feed, sd, out):
    import torch.distributed as dist

    from clsr_amd.dp import DataParallel, shard_feed
    from clsr_amd.net import CLSRNet

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    net = CLSRNet(hp, dims, device="cuda:0", seed=rank, table_dtype="bf16", table_master=True)  # the broadcast fixes the seeds
    if rank == 0:
        net.load_state_dict(sd)
    before = _digest(net)
    dp = DataParallel(net, HostStagedDist(dist), sync_bn=True, sparse_tables="all")
    out["lo%d" % rank] = (before, _digest(net))
    for b in range(2):
        f = dp.prepare(net.upload(shard_feed(feed[b], rank, world, hp.train_num_ngs + 1), True))
        dp.train_step(f)
    torch.cuda.synchronize()
    if rank == 0:
        out["state"] = {k: v.numpy() for k, v in net.state_dict().items()}
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_match_single_process_with_master(golden_dir, golden_hparams):
    import torch.multiprocessing as mp

    from clsr_amd.net import CLSRNet
    from clsr_amd.params import TABLES
    from oracle import clsr_oracle as O

    hp = copy.deepcopy(golden_hparams)
    hp.item_embedding_dim, hp.cate_embedding_dim = 32, 8
    dims = dict(Vu=len(pickle.load(open(hp.user_vocab, "rb"))), Vi=len(pickle.load(open(hp.item_vocab, "rb"))),
                Vc=len(pickle.load(open(hp.cate_vocab, "rb"))))
    g = np.load(os.path.join(golden_dir, "iterator_train_sa.npz"))
    feeds = [{k[3:]: g[k] for k in g.files if k.startswith("b%d_" % b)} for b in range(2)]
    params = O.init_params(dims, hp, seed=5, scale_dense=8.0)
    sd = dict(params)
    sd.update(O.init_bn_state(params))
    single = CLSRNet(hp, dims, device="cuda:0", seed=0, table_dtype="bf16", table_master=True)
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
    assert out["lo0"][0] != out["lo1"][0], "the ranks were built from different seeds"
    assert out["lo0"][1] == out["lo1"][1] == out["lo0"][0], "after construction both ranks hold rank 0's (hi, lo) tables"
    got = out["state"]
    assert set(got) == set(ref)
    noise_bound = 2.0 * float(hp.learning_rate) * len(feeds)

    def noisy(k):
        last = k.rsplit("/", 1)[-1]
        return (last.startswith("b_nn_layer") or (last == "b_nn_output" and "fcn_alpha" not in k)   # (alpha = sigmoid: real gradient)
                or k == LOGIT_BN0_MEAN)

    assert LOGIT_BN0_MEAN in ref and all(TABLES[k] in ref for k in single.tables)
    for k, v in ref.items():
        v = v.numpy()
        scale = float(np.abs(v).max()) + 1e-12
        d = np.abs(got[k] - v)
        # gradients of the global batch agree to fp32 accumulation noise; the updates follow them
        bar = noise_bound if noisy(k) else 1e-4 * scale + 1e-6
        print("%s: max diff %.3e, bar %.3e" % (k, float(d.max()), bar))
        assert float(d.max()) <= bar, (k, float(d.max()), scale)
    moved = sum(int((ref[TABLES[k]] != torch.as_tensor(np.asarray(sd[TABLES[k]]), dtype=torch.float32)).sum())
                for k in single.tables)
    assert moved > 0
