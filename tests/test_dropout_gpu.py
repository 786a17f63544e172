"""GPU tests of dropout in the logit MLP of A2SVD / GRU4Rec (clsr_amd/csrc/dropout.hip, CLSRNet._mlp_fwd_drop): the
kernels against torch on the CPU with a numpy restatement of the mask rule written here, the whole training step against
the sibling oracle with a dropout-aware ``fcn_net`` patched in, the no-op settings, the seed / draw counter in checkpoints
and replayed launch plans, the refusals, two data-parallel ranks against one process, and the model API."""
import copy
import os
import pickle
import socket
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from clsr_amd.ops import call, query  # noqa: E402
from clsr_amd.params import SIB_TABLES  # noqa: E402

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


# ------------------------------------------------------------------------------- the mask rule, restated
def philox4x32_10(ctr, key):
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k = [np.asarray(key[..., i], dtype=np.uint64) for i in range(2)]
    lo = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & lo, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & lo]
        k = [(k[0] + np.uint64(W0)) & lo, (k[1] + np.uint64(W1)) & lo]
    return np.stack(c, -1).astype(np.uint32)


def threshold(keep):
    return int(round(keep * (1 << 24)))


def inv_keep(keep):
    return float(np.float32(1.0 / keep))


def mask_np(seed, draw, layer, row0, B, C, thr):
    """counter (global row, column / 4, layer, draw), key (seed low, seed high); word k serves column 4 (c / 4) + k;
    kept <=> (word >> 8) < thr."""
    Q = (C + 3) // 4
    ctr = np.zeros((B, Q, 4), dtype=np.uint32)
    ctr[..., 0] = ((row0 + np.arange(B, dtype=np.int64)) & 0xffffffff).astype(np.uint32)[:, None]
    ctr[..., 1] = np.arange(Q, dtype=np.uint32)[None, :]
    ctr[..., 2] = layer
    ctr[..., 3] = draw
    key = np.zeros((B, Q, 2), dtype=np.uint32)
    key[..., 0], key[..., 1] = seed & 0xffffffff, (seed >> 32) & 0xffffffff
    words = philox4x32_10(ctr, key).reshape(B, 4 * Q)[:, :C]
    return (words >> np.uint32(8)) < np.uint32(thr)


def _state(seed, draw):
    return torch.from_numpy(np.array([seed & 0xffffffff, seed >> 32, draw, 0], dtype=np.uint32).view(np.int32).copy()).cuda()


# ------------------------------------------------------------------------------- 5. kernels
# the (B, C, row0) cases of the host mask test + one whose part count reaches its cap (more rows than 4 per row slot)
CASES = [(1, 4, 0), (5, 8, 0), (37, 100, 0), (3, 1024, 0), (257, 64, 1000003), (2051, 64, 5)]


@pytest.mark.parametrize("B,C,row0", CASES)
def test_dropout_kernels(B, C, row0):
    seed, draw, layer, keep = 0x9e3779b97f4a7c15, 6, 1, 0.7
    thr, inv = threshold(keep), inv_keep(keep)
    g = torch.Generator().manual_seed(B * 1000 + C)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    z, da = rnd(B, C), rnd(B, C)
    sc, sh, mu, istd = rnd(C).abs() * 0.5 + 0.5, rnd(C) * 0.3, rnd(C) * 0.1, rnd(C).abs() + 0.5
    dev = [t.cuda() for t in (z, sc, sh, mu, istd, da)]
    dz, dsc, dsh, dmu, dis, dda = dev
    st = _state(seed, draw)
    eps = 2.0 ** -24

    def expected(d):
        m = torch.from_numpy(mask_np(seed, d, layer, row0, B, C, thr))
        y = z.double() * sc.double() + sh.double()
        a = torch.where(m, torch.relu(y) * inv, torch.zeros_like(y))
        dy = torch.where(m & (y > 0), da.double() * inv, torch.zeros_like(y))
        return m, y, a, dy

    def forward():
        a = torch.full((B, C), float("nan"), device="cuda")
        call("clsr_bn_relu_dropout_fwd", dz, dsc, dsh, st, layer, row0, thr, inv, B, C, a)
        return a.cpu()

    def check_fwd(a, d):
        m, y, a_exp, _ = expected(d)
        assert bool((a[~m] == 0).all()), "dropped elements must be exactly zero"
        # one multiply-add (rounded once or twice) and the multiplication by 1 / keep
        bound = 1.01 * eps * (inv * ((z.double() * sc.double()).abs() + y.abs()) + a_exp.abs())
        err = (a.double() - a_exp).abs()
        assert bool((err <= bound).all()), float((err - bound).max())

    a = forward()
    check_fwd(a, draw)
    # backward: parts rows of sums, nothing beyond them
    parts = query("clsr_bn_relu_dropout_bwd_parts", B, C)
    assert 0 < parts <= 512

    def backward():
        dy = torch.full((B, C), float("nan"), device="cuda")
        bnp = torch.full((parts + 2, 2, C), 12345.0, dtype=torch.float64, device="cuda")
        call("clsr_bn_relu_dropout_bwd", dda, dz, dsc, dsh, dmu, dis, st, layer, row0, thr, inv, B, C, dy, bnp)
        return dy, bnp

    dy, bnp = backward()
    dy2, bnp2 = backward()
    assert torch.equal(dy, dy2) and torch.equal(bnp, bnp2), "two runs must be bit-identical"
    assert bool((bnp[parts:] == 12345.0).all())
    m, y, _, dy_exp = expected(draw)
    dyc = dy.cpu()
    assert bool((dyc[~m] == 0).all())
    err = (dyc.double() - dy_exp).abs()
    assert bool((err <= 1.01 * eps * dy_exp.abs()).all()), float(err.max())
    tot = bnp[:parts].sum(0).cpu()
    xhat = (z.double() - mu.double()) * istd.double()
    for got, exp, name in ((tot[0], dy_exp.sum(0), "sum dy"), (tot[1], (dy_exp * xhat).sum(0), "sum dy xhat")):
        d = (got - exp).abs()
        assert bool((d <= 1e-4 + 1e-4 * exp.abs()).all()), (name, float(d.max()))
    # in place (dy = da), as the step calls it
    dinp = dda.clone()
    bnp3 = torch.empty(parts, 2, C, dtype=torch.float64, device="cuda")
    call("clsr_bn_relu_dropout_bwd", dinp, dz, dsc, dsh, dmu, dis, st, layer, row0, thr, inv, B, C, dinp, bnp3)
    assert torch.equal(dinp, dy) and torch.equal(bnp3, bnp[:parts])
    # the tick moves the draw number by one: another mask, the restated one at draw + 1
    call("clsr_dropout_tick", st)
    assert st.cpu().numpy().view(np.uint32).tolist() == [seed & 0xffffffff, seed >> 32, draw + 1, 0]
    a1 = forward()
    check_fwd(a1, draw + 1)
    if B * C >= 64:
        assert not torch.equal(a1 == 0, a == 0)


# ------------------------------------------------------------------------------- helpers of tests/test_siblings_gpu.py
KINDS = {"gru4rec": dict(model_type="GRU4Rec"), "din": dict(model_type="DIN"), "sli_rec": dict(model_type="sli_rec"),
         "a2svd": dict(model_type="A2SVD"), "dien": dict(model_type="DIEN")}


def _hp(golden_hparams, kind, **kw):
    hp = copy.deepcopy(golden_hparams)
    for k, v in dict(KINDS[kind], user_embedding_dim=16, attention_size=40, **kw).items():
        setattr(hp, k, v)
    return hp


def _dims(hp):
    return dict(Vu=len(pickle.load(open(hp.user_vocab, "rb"))), Vi=len(pickle.load(open(hp.item_vocab, "rb"))),
                Vc=len(pickle.load(open(hp.cate_vocab, "rb"))))


def _feed(golden_dir, name, b=0):
    g = np.load(os.path.join(golden_dir, name))
    pre = "b%d_" % b
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}


def _close(got, exp, rtol, atol, name):
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    exp = torch.as_tensor(exp).detach().double().cpu().reshape(-1)
    assert got.shape == exp.shape, (name, got.shape, exp.shape)
    err = (got - exp).abs()
    excess = float((err - (atol + rtol * exp.abs())).max())
    assert excess <= 0, "%s: max abs err %.3e, max |exp| %.3e" % (name, float(err.max()), float(exp.abs().max()))


def _setup(hp, kind, dedup, seed=0):
    from clsr_amd.seqnet import SeqNet
    from oracle import sibling_oracle as O

    dims = _dims(hp)
    params32 = O.init_params(dims, hp, kind, seed=5, scale_dense=8.0)
    net = SeqNet(hp, dims, kind=kind, device="cuda:0", seed=seed, dedup_histories=dedup)
    sd = dict(params32)
    sd.update(O.init_bn_state(params32))
    net.load_state_dict(sd, strict=True)
    params64 = type(params32)((k, v.double()) for k, v in params32.items())
    return O, net, params64


def _dropout_fcn_net(C, seed, draw, row0=0):
    """``oracle.clsr_oracle.fcn_net`` with the reference's dropout in front of the activation (base_model.py
    _active_layer): same body, the restated mask of this draw applied to the batch-normalised values."""
    def fcn_net(x, sizes, scope, params, bn_state, hp, training, new_bn):
        h = x
        for i in range(len(sizes)):
            h = h @ params[scope + "nn_part/w_nn_layer%d" % i] + params[scope + "nn_part/b_nn_layer%d" % i]
            if hp.enable_BN is True:
                bn = scope + "nn_part/batch_normalization" + ("" if i == 0 else "_%d" % i) + "/"
                h = C.batch_norm(h, bn, params, bn_state, training, new_bn)
            if training and hp.user_dropout:
                keep = 1.0 - float(hp.dropout[i])
                m = mask_np(seed, draw, i, row0, h.shape[0], h.shape[1], threshold(keep))
                h = h * torch.from_numpy(m).to(h.dtype) * inv_keep(keep)
            h = C._activate(h, hp.activation[i])
        return h @ params[scope + "nn_part/w_nn_output"] + params[scope + "nn_part/b_nn_output"]
    return fcn_net


# ------------------------------------------------------------------------------- 6. step parity
@pytest.mark.parametrize("dropout", [[0.3, 0.3], [0.5, 0.0]])
@pytest.mark.parametrize("dedup", [True, False])
@pytest.mark.parametrize("kind", ["a2svd", "gru4rec"])
def test_train_step_with_dropout_matches_oracle(golden_dir, golden_hparams, monkeypatch, kind, dedup, dropout):
    from oracle import clsr_oracle as C

    hp = _hp(golden_hparams, kind, user_dropout=True, dropout=dropout)
    O, net, params = _setup(hp, kind, dedup, seed=0)
    monkeypatch.setattr(C, "fcn_net", _dropout_fcn_net(C, 0, 1))     # seed 0; the step's tick makes it draw 1
    feed = _feed(golden_dir, "iterator_train_sa.npz", b=1)
    tf = O.to_torch_feed(feed, dtype=torch.float64)
    bn, adam = O.init_bn_state(params), O.init_adam(params)
    new_p, new_bn, _, ls, grads, norms, out = O.train_step(params, bn, adam, 1, tf, hp, kind)
    net.capture_grads = True
    got = net.train_step(net.upload(feed, True))
    torch.cuda.synchronize()
    B, T, G, Hn = net.last_shape
    rep = (lambda t: t) if G == 1 else (lambda t: t[::G])
    _close(got["logit"], out["logit"], 1e-4, 1e-4, "logit")
    _close(got["model_output"], out["model_output"], 1e-4, 1e-5, "model_output")
    if kind == "a2svd":
        _close(got["asvd_output"], rep(out["asvd_output"]), 1e-4, 1e-5, "asvd_output")
        _close(got["w_asvd"], rep(out["w_asvd"]), 1e-4, 1e-6, "A2SVD weights")
    if kind == "gru4rec":
        _close(got["final_state"], rep(out["final_state"]), 1e-4, 1e-5, "final_state")
    gl = net.read_losses()
    for k in ("loss", "data_loss", "regular_loss"):
        _close([gl[k]], [float(ls[k])], 1e-5, 1e-7, k)
    cap, raw = net.captured, out["raw_grads"]
    floor = 4e-6 * max(float(raw[n].abs().max()) for n in net.dense_names)
    assert set(net.dense_names) | set(SIB_TABLES.values()) == set(raw)
    for i, name in enumerate(net.dense_names):
        scale = float(raw[name].abs().max()) + 1e-12
        _close(cap["dense"][name], raw[name], 2e-3, 2e-4 * scale + floor, "grad " + name)
        _close([float(cap["dense_sumsq"][i]) ** 0.5], [norms[name]], 1e-3, 20 * floor, "norm " + name)
    ss = cap["table_sumsq"].cpu().numpy()
    tab_norm = dict(item=(ss[0] + ss[2] + ss[4]) ** 0.5, cate=(ss[1] + ss[3] + ss[5]) ** 0.5)
    for key, name in SIB_TABLES.items():
        scale = float(raw[name].abs().max()) + 1e-12
        _close(cap["tables"][key], raw[name], 2e-3, 2e-4 * scale + floor, "grad " + name)
        if not dedup:
            _close([tab_norm[key]], [norms[name]], 1e-3, 1e-7, "clip norm " + name)
    sd = net.state_dict()
    lr = hp.learning_rate
    for name in list(net.dense_names) + list(SIB_TABLES.values()):
        g_ = grads[name].double().reshape(-1)
        sel = g_.abs() > 100 * floor
        upd_got = (sd[name].double().reshape(-1) - params[name].reshape(-1))[sel]
        upd_exp = (new_p[name].reshape(-1) - params[name].reshape(-1))[sel]
        if upd_exp.numel():
            _close(upd_got, upd_exp, 5e-3, 0.02 * lr, "adam update " + name)
    for k, v in new_bn.items():
        _close(sd[k], v, 1e-4, 1e-6, k)
    assert sd["__dropout__/state"].tolist() == [0, 0, 1]


# ------------------------------------------------------------------------------- 7. no-op settings
def _one_step(net, feed):
    net.capture_grads = True
    out = net.train_step(net.upload(feed, True))
    torch.cuda.synchronize()
    res = {"logit": out["logit"].clone()}
    res.update({"g/" + k: v.clone() for k, v in net.captured["dense"].items()})
    res.update({"t/" + k: v.clone() for k, v in net.captured["tables"].items()})
    res.update({"p/" + k: v for k, v in net.state_dict().items()})
    return res


@pytest.mark.parametrize("model", ["a2svd", "clsr"])
def test_settings_without_effect_change_nothing(golden_dir, golden_hparams, model):
    from clsr_amd.net import CLSRNet
    from clsr_amd.seqnet import SeqNet

    feed = _feed(golden_dir, "iterator_train_sa.npz", b=1)
    res = []
    for kw in ({}, dict(user_dropout=True, dropout=[0.0, 0.0]), dict(user_dropout=False, dropout=[0.3, 0.3])):
        if model == "clsr":
            hp = copy.deepcopy(golden_hparams)
            for k, v in kw.items():
                setattr(hp, k, v)
            net = CLSRNet(hp, _dims(hp), device="cuda:0", seed=4)
        else:
            hp = _hp(golden_hparams, model, **kw)
            net = SeqNet(hp, _dims(hp), kind=model, device="cuda:0", seed=4)
        assert not net.drop_on
        res.append(_one_step(net, feed))
    for other in res[1:]:
        assert set(other) == set(res[0]) and not any(k.startswith("p/__dropout__") for k in other)
        bad = [k for k in res[0] if not torch.equal(res[0][k], other[k])]
        assert not bad, bad


# ------------------------------------------------------------------------------- 8. seed and draw counter as state
@pytest.fixture(scope="module")
def drop_setup(golden_dir, golden_hparams):
    hp = _hp(golden_hparams, "a2svd", user_dropout=True, dropout=[0.3, 0.3])
    from oracle import sibling_oracle as O

    params32 = O.init_params(_dims(hp), hp, "a2svd", seed=5, scale_dense=8.0)
    sd = dict(params32)
    sd.update(O.init_bn_state(params32))
    return hp, sd, _feed(golden_dir, "iterator_train_sa.npz", b=1), _feed(golden_dir, "iterator_eval_sa.npz", b=0)


def _net(hp, sd, seed, **kw):
    from clsr_amd.seqnet import SeqNet

    net = SeqNet(hp, _dims(hp), kind="a2svd", device="cuda:0", seed=seed, **kw)
    if sd is not None:
        net.load_state_dict(sd)
    return net


def _same(a, b):
    assert set(a) == set(b)
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, bad


def test_checkpoint_carries_seed_and_draw(drop_setup):
    hp, sd, feed, ev = drop_setup
    a = _net(hp, sd, 3)
    f = a.upload(feed, True)
    for _ in range(3):
        a.train_step(f)
    ckpt = a.state_dict()
    assert ckpt["__dropout__/state"].tolist() == [3, 0, 3]
    for _ in range(3):
        a.train_step(f)
    b = _net(hp, ckpt, 99)
    fb = b.upload(feed, True)
    for _ in range(3):
        b.train_step(fb)
    torch.cuda.synchronize()
    sa = a.state_dict()
    assert sa["__dropout__/state"].tolist() == [3, 0, 6]
    _same(sa, b.state_dict())
    # a checkpoint without the key: the net's own seed, draw 0
    c = _net(hp, sd, 7)
    c.train_step(c.upload(feed, True))
    c.load_state_dict(sd)
    assert c.state_dict()["__dropout__/state"].tolist() == [7, 0, 0]
    # scoring never drops: twice the same scores, and those of a net without dropout restored from the same checkpoint
    fe = a.upload(ev, False)
    s1 = a.forward(fe, False)["logit"].clone()
    s2 = a.forward(fe, False)["logit"].clone()
    hp0 = copy.deepcopy(hp)
    hp0.user_dropout = False
    plain = _net(hp0, sa, 1)
    s3 = plain.forward(plain.upload(ev, False), False)["logit"].clone()
    assert torch.equal(s1, s2) and torch.equal(s1, s3)
    assert a.state_dict()["__dropout__/state"].tolist() == [3, 0, 6]      # (scoring does not tick)


def test_seed_selects_the_masks(drop_setup):
    hp, sd, feed, _ = drop_setup
    logits = []
    for seed in (1, 2, 1):
        net = _net(hp, sd, seed)
        logits.append(net.train_step(net.upload(feed, True))["logit"].clone())
    assert not torch.equal(logits[0], logits[1])
    assert torch.equal(logits[0], logits[2])


def test_replayed_plan_draws_a_new_mask_per_step(drop_setup):
    """The third identical call replays the recorded launches with their recorded scalars: the draw number must come from
    the device, or every replay would apply the mask of the recorded step."""
    hp, sd, feed, _ = drop_setup
    runs = []
    for plans in (False, True):
        net = _net(hp, sd, 5)
        net.use_plans = plans
        f = net.upload(feed, True)
        logits = [net.train_step(f)["logit"].clone() for _ in range(3)]
        torch.cuda.synchronize()
        assert sum(1 for e in net._step_plans.values() if e[1] is not None) == (1 if plans else 0)
        runs.append((logits, net.state_dict()))
    for x, y in zip(runs[0][0], runs[1][0]):
        assert torch.equal(x, y)
    _same(runs[0][1], runs[1][1])
    assert runs[1][1]["__dropout__/state"].tolist() == [5, 0, 3]


# ------------------------------------------------------------------------------- 9. refusals
def test_refusals(golden_hparams):
    from clsr_amd.net import CLSRNet
    from clsr_amd.seqnet import SeqNet

    on = dict(user_dropout=True, dropout=[0.3, 0.3])
    hp = copy.deepcopy(golden_hparams)
    for k, v in on.items():
        setattr(hp, k, v)
    with pytest.raises(NotImplementedError, match="attention MLP"):
        CLSRNet(hp, _dims(hp), device="cuda:0", seed=0)
    for kind in ("din", "dien", "sli_rec"):
        hp = _hp(golden_hparams, kind, **on)
        with pytest.raises(NotImplementedError, match="attention MLP"):
            SeqNet(hp, _dims(hp), kind=kind, device="cuda:0", seed=0)
    for kind in ("a2svd", "gru4rec"):
        hp = _hp(golden_hparams, kind, embedding_dropout=0.1)
        with pytest.raises(NotImplementedError, match="embedding_dropout"):
            SeqNet(hp, _dims(hp), kind=kind, device="cuda:0", seed=0)
        hp = _hp(golden_hparams, kind, user_dropout=True, dropout=[1.0, 0])
        with pytest.raises(ValueError):
            SeqNet(hp, _dims(hp), kind=kind, device="cuda:0", seed=0)
    hp = copy.deepcopy(golden_hparams)
    hp.embedding_dropout = 0.1
    with pytest.raises(NotImplementedError, match="embedding_dropout"):
        CLSRNet(hp, _dims(hp), device="cuda:0", seed=0)
    hp = copy.deepcopy(golden_hparams)
    hp.dropout = [1.0, 0]
    with pytest.raises(ValueError):
        CLSRNet(hp, _dims(hp), device="cuda:0", seed=0)


# ------------------------------------------------------------------------------- 10. data parallel
WAIT_S = 120.0


def _dp_worker(rank, world, port, hp, dims, feed, sd, out):
    import torch.distributed as dist

    from clsr_amd.dp import DataParallel, HostStagedDist, shard_feed
    from clsr_amd.seqnet import SeqNet

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    net = SeqNet(hp, dims, kind="a2svd", device="cuda:0", seed=10 + rank)     # different seeds: the broadcast fixes that
    if rank == 0:
        net.load_state_dict(sd)
    dp = DataParallel(net, HostStagedDist(dist), sync_bn=True, sparse_tables="auto")
    net.capture_grads = True
    dp.train_step(dp.prepare(net.upload(shard_feed(feed, rank, world, hp.train_num_ngs + 1), True)))
    torch.cuda.synchronize()
    out["drop%d" % rank] = net.drop_state.cpu().numpy().view(np.uint32).tolist()
    if rank == 0:
        out["grads"] = {k: v.cpu().numpy() for k, v in net.captured["dense"].items()}
        out["tgrads"] = {k: v.cpu().numpy() for k, v in net.captured["tables"].items()}
        out["losses"] = net.read_losses()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_draw_the_masks_of_the_global_batch(golden_dir, drop_setup):
    import torch.multiprocessing as mp

    hp, sd, _, _ = drop_setup
    feed = _feed(golden_dir, "iterator_train_sa.npz", b=0)
    dims = _dims(hp)
    single = _net(hp, sd, 10)
    single.capture_grads = True
    single.train_step(single.upload(feed, True))
    torch.cuda.synchronize()
    ref_losses = single.read_losses()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = mp.get_context("spawn").Manager().dict()
    pc = mp.spawn(_dp_worker, args=(2, port, hp, dims, feed, sd, out), nprocs=2, join=False)
    deadline = time.monotonic() + WAIT_S
    try:
        while not pc.join(timeout=max(0.1, deadline - time.monotonic())):
            if time.monotonic() >= deadline:
                pytest.fail("rank processes still running after %.0f s" % WAIT_S)
    finally:
        for p in pc.processes:
            if p.is_alive():
                p.terminate()
        for p in pc.processes:
            p.join(10)
            if p.is_alive():
                p.kill()
    assert out["drop0"] == out["drop1"] == [10, 0, 1, 0]
    for k in ("loss", "data_loss", "regular_loss"):
        assert abs(out["losses"][k] - ref_losses[k]) < 1e-5 * max(1.0, abs(ref_losses[k])), (k, out["losses"], ref_losses)
    ref_g = {k: v.cpu().numpy() for k, v in single.captured["dense"].items()}
    floor = 4e-6 * max(float(np.abs(v).max()) for v in ref_g.values())
    for k, v in ref_g.items():
        d = np.abs(out["grads"][k] - v)
        assert float(d.max()) <= 2e-3 * float(np.abs(v).max()) + floor, (k, float(d.max()), float(np.abs(v).max()))
    for k, v in single.captured["tables"].items():
        v = v.cpu().numpy()
        assert float(np.abs(out["tgrads"][k] - v).max()) <= 2e-3 * float(np.abs(v).max()) + floor, k


# ------------------------------------------------------------------------------- 11. model API
def test_a2svd_model_trains_with_the_reference_dropout(tmp_path):
    """A2SVDModel the way the reference's asvd.yaml trains it (user_dropout, dropout [0.3, 0.3]) on the synthetic task of
    tests/test_model_api_gpu.py: fit runs, the test AUC rises, the checkpoint round trip holds."""
    from clsr_amd.clsr import A2SVDModel, latest_checkpoint
    from clsr_amd.deeprec_utils import prepare_hparams
    from clsr_amd.sequential_iterator import SequentialIterator
    from clsr_amd.synthetic import make_tsv_dataset

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = make_tsv_dataset(str(tmp_path / "data"), n_users=400, n_items=1500, n_cates=12, n_train=5000, n_valid=200,
                             n_test=200, valid_ngs=4, test_ngs=9, max_hist=20, signal=True)
    hp = prepare_hparams(os.path.join(root, "clsr_amd", "config", "asvd.yaml"), user_vocab=paths["user_vocab"],
                         item_vocab=paths["item_vocab"], cate_vocab=paths["category_vocab"], max_seq_length=20,
                         batch_size=500, train_num_ngs=4, time_unit="s", is_clip_norm=1, embed_l2=1e-6, layer_l2=1e-6,
                         learning_rate=0.005, show_step=10 ** 9, save_model=True,
                         MODEL_DIR=str(tmp_path / "model") + "/", SUMMARIES_DIR=None, write_tfevents=False, epochs=4,
                         EARLY_STOP=10, user_dropout=True, dropout=[0.3, 0.3])
    model = A2SVDModel(hp, SequentialIterator, seed=7)
    assert model.net.drop_on and model.net.drop_thr == (threshold(0.7),) * 2
    before = model.run_eval(paths["test_data"], 9)
    assert model.fit(paths["train_data"], paths["valid_data"], valid_num_ngs=4, eval_metric="group_auc") is model
    after = model.run_eval(paths["test_data"], 9)
    print("A2SVD with dropout [0.3, 0.3]: test AUC before %.4f, after %.4f" % (before["auc"], after["auc"]))
    assert after["auc"] > before["auc"], (before, after)
    assert int(model.net.drop_state[2].item()) > 0
    ckpt = latest_checkpoint(hp.MODEL_DIR)
    fresh = A2SVDModel(hp, SequentialIterator, seed=123)
    fresh.load_model(ckpt)
    model.load_model(ckpt)
    assert fresh.run_eval(paths["valid_data"], 4) == model.run_eval(paths["valid_data"], 4)
    assert torch.equal(fresh.net.drop_state, model.net.drop_state)
