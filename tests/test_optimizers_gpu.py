"""GPU tests of the reference's other optimisers (base_model.py:249-279; csrc/optim_tf.hip): the three update kernels
against a float64 restatement of the TF 1.15 update rules, and the CLSR step / checkpoints / siblings / model API
trained with them."""
import copy
import math
import os
import pickle
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from clsr_amd import ops  # noqa: E402
from clsr_amd.net import TF_OPTIMIZERS, CLSRNet  # noqa: E402
from clsr_amd.ops import call  # noqa: E402

NAMES = ["sgd", "adagrad", "padagrad", "rmsprop", "adadelta", "ftrl", "pgd"]
KERNEL_OPTS = ["sgd", "adagrad", "padagrad", "rmsprop", "adadelta", "ftrl"]
EPS32 = 2.0 ** -23
ADAGRAD_FIT_LR = 0.05     # (Adagrad steps ~lr * g / sqrt(acc): far larger rates than Adam's 0.005)


# ---------------------------------------------------------------------------- float64 restatement (TF 1.15 defaults)
def restate(name, g, p, s1, s2, lr):
    """One update of already clipped gradients g (float64 arrays); returns (p, s1, s2, tol) where tol is the fp32
    rounding bound of the kernels' arithmetic per element of (p, s1, s2) beyond a relative 1e-6: a few ulps of the
    operands of the final subtraction (var - step cancels where the step is close to var), plus FTRL's own term."""
    pn, n1, n2, tol = _restate(name, g, p, s1, s2, lr)
    return pn, n1, n2, (tol[0] + 4 * EPS32 * (np.abs(p) + np.abs(pn - p)), tol[1] + 4 * EPS32 * np.abs(s1),
                        tol[2] + 4 * EPS32 * np.abs(s2))


def _restate(name, g, p, s1, s2, lr):
    z = np.zeros_like(p)
    if name in ("sgd", "gd", "pgd"):
        return p - lr * g, s1, s2, (z, z, z)
    if name in ("adagrad", "padagrad"):
        a = s1 + g * g
        return p - lr * g / np.sqrt(a), a, s2, (z, z, z)
    if name == "rmsprop":
        ms = s1 + (g * g - s1) * (1 - 0.9)
        mom = 0.0 * s2 + lr * g / np.sqrt(ms + 1e-10)
        return p - mom, ms, mom, (z, z, z)
    if name == "adadelta":
        acc = 0.95 * s1 + 0.05 * g * g
        u = np.sqrt(s2 + 1e-8) / np.sqrt(acc + 1e-8) * g
        accu = 0.95 * s2 + 0.05 * u * u
        return p - lr * u, acc, accu, (z, z, z)
    if name == "ftrl":
        n = s1 + g * g
        lin = s2 + g - (np.sqrt(n) - np.sqrt(s1)) / lr * p
        pn = np.where(np.abs(lin) > 0, -lin / (np.sqrt(n) / lr), 0.0)
        # sqrt(n) - sqrt(acc) cancels in fp32: its rounding, amplified by |var| / lr, bounds the error of lin
        tl = 8 * EPS32 * (np.sqrt(n) * np.abs(p) / lr + np.abs(g))
        return pn, n, lin, (tl * lr / np.sqrt(n), z, tl)
    raise ValueError(name)


def slot_inits(name):
    ini = [v for _, v in TF_OPTIMIZERS[name][1]]
    return (ini + [None, None])[:2]


def _close(got, exp, tol, rtol, what):
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    exp = np.asarray(exp, dtype=np.float64).reshape(-1)
    tol = np.asarray(tol, dtype=np.float64).reshape(-1)
    err = np.abs(got - exp)
    lim = rtol * np.abs(exp) + tol + 1e-30
    bad = err > lim
    assert not bad.any(), "%s: %d bad, worst err %.3e at exp %.3e" % (what, int(bad.sum()), float(err[bad].max()),
                                                                       float(exp[bad][np.argmax(err[bad])]))


def _f32(a, dev="cuda:0"):
    return torch.tensor(np.asarray(a, dtype=np.float32), device=dev)


def _clip(sumsq, clip):
    if clip <= 0:
        return 1.0
    return clip / max(math.sqrt(sumsq), clip)


def _state(abort=False):
    return torch.tensor([1.0, 0.9, 0.999, 0.0, 1.0 if abort else 0.0, 0, 0, 0], dtype=torch.float64, device="cuda:0")


def _slots_for(name, shape, rng):
    """Random positive slot values of the right kind (accumulators > 0), None where the optimiser has no slot."""
    i1, i2 = slot_inits(name)
    s1 = None if i1 is None else (rng.uniform(0.05, 0.5, shape) if name != "adadelta" else rng.uniform(0, 1e-3, shape))
    s2 = None
    if i2 is not None:
        s2 = rng.uniform(0, 1e-3, shape) if name == "adadelta" else rng.normal(0, 1e-3, shape)
    return s1, s2


def _code(name):
    return TF_OPTIMIZERS[name][0]


# ---------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("clip", [0.05, 100.0])
@pytest.mark.parametrize("name", KERNEL_OPTS)
def test_dense_kernel(name, clip):
    rng = np.random.default_rng(1)
    sizes = [12, 40, 8, 100]
    n = sum(sizes)
    seg_of = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    p, g = rng.normal(0, 0.1, n), rng.normal(0, 0.02, n)
    s1, s2 = _slots_for(name, n, rng)
    sumsq = np.array([float((g[seg_of == i].astype(np.float32).astype(np.float64) ** 2).sum()) for i in range(len(sizes))])
    skip = np.array([0, 1, 0, 0], dtype=np.uint8)
    lr = 0.01
    P, G = _f32(p), _f32(g)
    S1, S2 = (None if s is None else _f32(s) for s in (s1, s2))
    call("clsr_dense_tf", _code(name), P, G, S1, S2, torch.tensor(seg_of, device="cuda:0"),
         torch.tensor(skip, device="cuda:0"), torch.tensor(sumsq, device="cuda:0"), clip, _state(), lr, n)
    torch.cuda.synchronize()
    p32, g32 = p.astype(np.float32).astype(np.float64), g.astype(np.float32).astype(np.float64)
    f = np.array([_clip(s, clip) for s in sumsq])[seg_of]
    z = np.zeros(n)
    e1 = z if s1 is None else s1.astype(np.float32).astype(np.float64)
    e2 = z if s2 is None else s2.astype(np.float32).astype(np.float64)
    ep, n1, n2, tol = restate(name, g32 * f, p32, e1, e2, lr)
    live = skip[seg_of] == 0
    got_p = P.cpu().double().numpy()
    _close(got_p[live], ep[live], tol[0][live], 2e-6, "param")
    assert np.array_equal(P.cpu().numpy()[~live], p.astype(np.float32)[~live])      # skipped tensor: bit-identical
    if S1 is not None:
        _close(S1.cpu().numpy()[live], n1[live], tol[1][live], 2e-6, "slot1")
        assert np.array_equal(S1.cpu().numpy()[~live], s1.astype(np.float32)[~live])
    if S2 is not None:
        _close(S2.cpu().numpy()[live], n2[live], tol[2][live], 2e-6, "slot2")
        assert np.array_equal(S2.cpu().numpy()[~live], s2.astype(np.float32)[~live])
    assert float(G.abs().max()) == 0.0


def _table_case(name, V, C, rng, touched_frac=0.3):
    t, g = rng.normal(0, 0.1, (V, C)), np.zeros((V, C))
    flags = (rng.random(V) < touched_frac).astype(np.uint8)
    flags[0] = 1
    g[flags == 1] = rng.normal(0, 0.02, (int(flags.sum()), C))
    s1, s2 = _slots_for(name, (V, C), rng)
    return t, g, flags, s1, s2


def _check_table(name, T, G, S1, S2, FL, t, g, flags, s1, s2, factor, lr, what):
    t32 = t.astype(np.float32)
    e1 = np.zeros_like(t) if s1 is None else s1.astype(np.float32).astype(np.float64)
    e2 = np.zeros_like(t) if s2 is None else s2.astype(np.float32).astype(np.float64)
    ep, n1, n2, tol = restate(name, g.astype(np.float32).astype(np.float64) * factor, t32.astype(np.float64), e1, e2, lr)
    on = flags == 1
    gt = T.cpu().numpy()
    _close(gt[on], ep[on], tol[0][on], 2e-6, what + " table")
    assert np.array_equal(gt[~on], t32[~on]), what + ": untouched rows changed"
    for S, s, n_, tl in ((S1, s1, n1, tol[1]), (S2, s2, n2, tol[2])):
        if S is None:
            continue
        gs = S.cpu().numpy()
        _close(gs[on], n_[on], tl[on], 2e-6, what + " slot")
        assert np.array_equal(gs[~on], s.astype(np.float32)[~on]), what + ": untouched slot rows changed"
    assert float(G.abs().max()) == 0.0, what + ": gradient not cleared"
    assert int(FL.sum()) == 0, what + ": flags not cleared"


# C = 32: the 16-byte sweep clears the flags itself (8 chunks per row divide a wave); C = 24: 6 chunks -- separate
# clearing launch; C = 6: the scalar sweep
@pytest.mark.parametrize("clip", [0.05, 100.0])
@pytest.mark.parametrize("name", KERNEL_OPTS)
def test_tables_multi_kernel(name, clip):
    rng = np.random.default_rng(2)
    lr = 0.02
    shapes = [(300, 32), (77, 24), (50, 6)]
    for group in (shapes[:2], shapes[2:]):
        cases, descs, keep = [], [], []
        for V, C in group:
            t, g, flags, s1, s2 = _table_case(name, V, C, rng)
            T, G, FL = _f32(t), _f32(g), torch.tensor(flags, device="cuda:0")
            S1, S2 = (None if s is None else _f32(s) for s in (s1, s2))
            pieces = np.array([0.3, 0.0, 0.2, 0.0]) * float((g.astype(np.float32).astype(np.float64) ** 2).sum()) / 0.5
            SS = torch.tensor(pieces, device="cuda:0")
            keep.append((T, G, FL, S1, S2, SS))
            cases.append((t, g, flags, s1, s2, _clip(pieces[0] + pieces[2], clip)))
            descs.append((T.data_ptr(), None, G.data_ptr(), ops._ptr(S1), ops._ptr(S2), FL.data_ptr(), None, None,
                          SS.data_ptr(), V, C, 2, 2, 0.0, 0.0, 0))
        ops.multi("clsr_tables_tf_multi", ops.TableDesc, descs, _code(name), clip, _state(), lr)
        torch.cuda.synchronize()
        for (T, G, FL, S1, S2, _), (t, g, flags, s1, s2, f), (V, C) in zip(keep, cases, group):
            _check_table(name, T, G, S1, S2, FL, t, g, flags, s1, s2, f, lr, "sweep C=%d" % C)


@pytest.mark.parametrize("C", [32, 6])
@pytest.mark.parametrize("name", KERNEL_OPTS)
def test_table_rows_kernel(name, C):
    rng = np.random.default_rng(3)
    V, lr, clip = 500, 0.05, 0.05
    t, g, flags, s1, s2 = _table_case(name, V, C, rng)
    ids = np.nonzero(flags)[0].astype(np.int32)
    cap = len(ids) + 7
    IDS = torch.zeros(cap, dtype=torch.int32, device="cuda:0")
    IDS[:len(ids)] = torch.tensor(ids, device="cuda:0")
    CNT = torch.tensor([len(ids), 0], dtype=torch.int32, device="cuda:0")
    T, G, FL = _f32(t), _f32(g), torch.tensor(flags, device="cuda:0")
    S1, S2 = (None if s is None else _f32(s) for s in (s1, s2))
    sumsq = float((g.astype(np.float32).astype(np.float64) ** 2).sum())
    SS = torch.tensor([sumsq, 0.0], device="cuda:0", dtype=torch.float64)
    call("clsr_table_tf_rows", _code(name), T, G, S1, S2, FL, IDS, CNT, cap, C, SS, 1, 2, clip, _state(), lr)
    torch.cuda.synchronize()
    _check_table(name, T, G, S1, S2, FL, t, g, flags, s1, s2, _clip(sumsq, clip), lr, "rows C=%d" % C)


@pytest.mark.parametrize("name", ["sgd", "adagrad", "ftrl"])
def test_kernels_touch_nothing_in_an_aborted_step(name):
    rng = np.random.default_rng(4)
    V, C, lr = 64, 8, 0.01
    t, g, flags, s1, s2 = _table_case(name, V, C, rng)
    T, G, FL = _f32(t), _f32(g), torch.tensor(flags, device="cuda:0")
    S1, S2 = (None if s is None else _f32(s) for s in (s1, s2))
    before = [x.clone() for x in (T, G, FL) + tuple(s for s in (S1, S2) if s is not None)]
    SS = torch.tensor([1.0, 0.0], device="cuda:0", dtype=torch.float64)
    st = _state(abort=True)
    ids = torch.tensor(np.nonzero(flags)[0].astype(np.int32), device="cuda:0")
    CNT = torch.tensor([ids.numel(), 0], dtype=torch.int32, device="cuda:0")
    call("clsr_table_tf_rows", _code(name), T, G, S1, S2, FL, ids, CNT, ids.numel(), C, SS, 1, 1, 1.0, st, lr)
    ops.multi("clsr_tables_tf_multi", ops.TableDesc, [(T.data_ptr(), None, G.data_ptr(), ops._ptr(S1), ops._ptr(S2),
                                                      FL.data_ptr(), None, None, SS.data_ptr(), V, C, 1, 1, 0.0, 0.0, 0)],
              _code(name), 1.0, st, lr)
    seg = torch.zeros(V * C, dtype=torch.int32, device="cuda:0")
    call("clsr_dense_tf", _code(name), T.view(-1), G.view(-1), None if S1 is None else S1.view(-1),
         None if S2 is None else S2.view(-1), seg, None, SS, 1.0, st, lr, V * C)
    torch.cuda.synchronize()
    after = [T, G, FL] + [s for s in (S1, S2) if s is not None]
    for b, a in zip(before, after):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------- the CLSR step
def _feed(golden_dir, b=0):
    g = np.load(os.path.join(golden_dir, "iterator_train_sa.npz"))
    pre = "b%d_" % b
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}


def _dims(hp):
    return dict(Vu=len(pickle.load(open(hp.user_vocab, "rb"))), Vi=len(pickle.load(open(hp.item_vocab, "rb"))),
                Vc=len(pickle.load(open(hp.cate_vocab, "rb"))))


def _hp(hp, **kw):
    hp2 = copy.deepcopy(hp)
    for k, v in kw.items():
        setattr(hp2, k, v)
    return hp2


def _net(hp, precision="fp32", **kw):
    from oracle import clsr_oracle as O

    dims = _dims(hp)
    params = O.init_params(dims, hp, seed=3, scale_dense=8.0)
    net = CLSRNet(hp, dims, device="cuda:0", seed=0, precision=precision, **kw)
    sd = dict(params)
    sd.update(O.init_bn_state(params))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # (a checkpoint without slots: the slots stay at their initial values)
        net.load_state_dict(sd, strict=True)
    return O, net, params


def _touched(feed):
    """Involved rows per table (the reference's IndexedSlices rows: every lookup site's ids)."""
    it = np.unique(np.concatenate([feed["item_history"].ravel(), feed["items"].ravel()]))
    ct = np.unique(np.concatenate([feed["item_cate_history"].ravel(), feed["cates"].ravel()]))
    us = np.unique(feed["users"].ravel())
    return dict(item=it, cate=ct, user_long=us, user_short=us)


TABLE_NORM_SLOTS = dict(item=(0, 2, 4), cate=(1, 3, 5), user_long=(6, 8), user_short=(7, 9))


def _snapshot(net):
    tabs = {k: t.detach().double().cpu().numpy().copy() for k, t in net.tables.items()}
    s1 = {k: t.double().cpu().numpy().copy() for k, t in net.tab_m.items()}
    s2 = {k: t.double().cpu().numpy().copy() for k, t in net.tab_v.items()}
    dm = None if net.dense_m is None else net.dense_m.double().cpu().numpy().copy()
    dv = None if net.dense_v is None else net.dense_v.double().cpu().numpy().copy()
    return net.dense.double().cpu().numpy().copy(), dm, dv, tabs, s1, s2


@pytest.mark.parametrize("name", NAMES)
def test_step_applies_the_restatement_to_captured_gradients(golden_dir, golden_hparams, name):
    """Three steps; each one against the float64 restatement applied to the net's own captured gradients; rows
    outside the involved set stay bit-identical."""
    hp = _hp(golden_hparams, optimizer=name)
    _, net, _ = _net(hp)
    lr, clip = float(hp.learning_rate), float(hp.max_grad_norm)
    seg_of = net.seg_of.cpu().numpy()
    net.capture_grads = True
    for step in range(3):
        feed = _feed(golden_dir, step)
        d0, dm0, dv0, t0, s10, s20 = _snapshot(net)
        net.train_step(net.upload(feed, True))
        torch.cuda.synchronize()
        cap = net.captured
        d1, dm1, dv1, t1, s11, s21 = _snapshot(net)
        # dense
        gd = np.zeros_like(d0)
        for nme, g in cap["dense"].items():
            o = int(net.seg_off[net.dense_names.index(nme)])
            gd[o:o + g.numel()] = g.double().cpu().numpy().reshape(-1)
        dss = cap["dense_sumsq"].cpu().numpy()
        f = np.array([_clip(s, clip) for s in dss])[seg_of]
        z = np.zeros_like(d0)
        ep, e1, e2, tol = restate(name, gd * f, d0, z if dm0 is None else dm0, z if dv0 is None else dv0, lr)
        _close(d1, ep, tol[0] + 1e-9, 2e-6, "%s step %d dense" % (name, step))
        if dm1 is not None:
            _close(dm1, e1, tol[1] + 1e-12, 2e-6, "%s step %d dense slot 1" % (name, step))
        if dv1 is not None:
            _close(dv1, e2, tol[2] + 1e-12, 2e-6, "%s step %d dense slot 2" % (name, step))
        # tables: touched rows only
        ss = cap["table_sumsq"].cpu().numpy()
        rows = _touched(feed)
        for k in net.tables:
            g = cap["tables"][k].double().cpu().numpy()
            fk = _clip(sum(ss[i] for i in TABLE_NORM_SLOTS[k]), clip)
            zt = np.zeros_like(t0[k])
            ep, e1, e2, tol = restate(name, g * fk, t0[k], s10.get(k, zt), s20.get(k, zt), lr)
            r = rows[k]
            off = np.ones(t0[k].shape[0], bool)
            off[r] = False
            _close(t1[k][r], ep[r], tol[0][r] + 1e-9, 2e-6, "%s step %d table %s" % (name, step, k))
            assert np.array_equal(t1[k][off], t0[k][off]), (name, step, k)
            for got, exp, tl, before in ((s11.get(k), e1, tol[1], s10.get(k)), (s21.get(k), e2, tol[2], s20.get(k))):
                if got is not None:
                    _close(got[r], exp[r], tl[r] + 1e-12, 2e-6, "%s step %d slot %s" % (name, step, k))
                    assert np.array_equal(got[off], before[off]), (name, step, k)
            if name == "ftrl" and step == 0:     # (from lin = 0 the first step moves every touched row)
                assert (np.abs(t1[k][r] - t0[k][r]).max(axis=1) > 0).all(), "ftrl: a touched row of %s did not move" % k
        assert float(net.adam_state[0]) == step + 1


@pytest.mark.parametrize("name,precision", [(n, "fp32") for n in NAMES] + [("adagrad", "fp32x3"), ("sgd", "bf16")])
def test_three_steps_follow_the_oracle(golden_dir, golden_hparams, name, precision):
    """The oracle's clipped gradients + the restatement for three steps; parameters at the Adam-update tolerances of
    test_step_gpu.py (updates compared where the gradient is well above fp32 noise)."""
    import torch as _t

    hp = _hp(golden_hparams, optimizer=name)
    O, net, params = _net(hp, precision=precision)
    lr = float(hp.learning_rate)
    p = type(params)((k, v.double()) for k, v in params.items())
    bn = {k: v.double() for k, v in O.init_bn_state(params).items()}
    i1, i2 = slot_inits(name)
    slots = {k: [np.full(tuple(v.shape), 0.0 if i1 is None else i1), np.full(tuple(v.shape), 0.0 if i2 is None else i2)]
             for k, v in p.items() if not k.endswith("/user_embedding")}
    tnames = {"sequential/embedding/item_embedding": "item", "sequential/embedding/cate_embedding": "cate",
              "sequential/embedding/user_long_embedding": "user_long",
              "sequential/embedding/user_short_embedding": "user_short"}
    for step in range(3):
        feed = _feed(golden_dir, step)
        _, grads, _, new_bn, _ = O.gradients(p, bn, O.to_torch_feed(feed, dtype=_t.float64), hp)
        rows = _touched(feed)
        prev = p
        p = type(p)(p)
        for k, g in grads.items():
            pk, g_ = prev[k].numpy(), g.double().numpy()
            ep, s1, s2, _ = restate(name, g_, pk, slots[k][0], slots[k][1], lr)
            if k in tnames:
                r = rows[tnames[k]]
                ep2, a, b = pk.copy(), slots[k][0].copy(), slots[k][1].copy()
                ep2[r], a[r], b[r] = ep[r], s1[r], s2[r]
                ep, s1, s2 = ep2, a, b
            p[k] = _t.from_numpy(ep)
            slots[k] = [s1, s2]
        bn = dict(bn)
        bn.update(new_bn)
        net.train_step(net.upload(feed, True))
        torch.cuda.synchronize()
        sd = net.state_dict()
        for k, g in grads.items():
            gv = g.double().reshape(-1).abs()
            floor = 4e-6 * float(gv.max())
            sel = (gv > 100 * floor).numpy()
            upd_got = (sd[k].double().reshape(-1) - prev[k].reshape(-1)).numpy()[sel]
            upd_exp = (p[k].reshape(-1) - prev[k].reshape(-1)).numpy()[sel]
            if upd_exp.size == 0:
                continue
            # the parameters the oracle steps from are its own; the net's drift from them is part of the tolerance
            drift = np.abs(sd[k].double().reshape(-1).numpy() - p[k].reshape(-1).numpy())[sel]
            assert np.all(drift <= 5e-3 * np.abs(upd_exp) + 0.02 * lr), \
                "%s step %d %s: max drift %.3e" % (name, step, k, float(drift.max()))
        if name == "ftrl":
            got = sd["sequential/embedding/item_embedding"].numpy()
            assert np.abs(got[rows["item"]]).max() > 0
        # rows outside the involved set keep their initial values
        for k, key in tnames.items():
            if key not in net.tables:
                continue
            off = np.ones(p[k].shape[0], bool)
            seen = np.unique(np.concatenate([_touched(_feed(golden_dir, s))[key] for s in range(step + 1)]))
            off[seen] = False
            assert np.array_equal(sd[k].numpy()[off], params[k].numpy()[off]), (name, step, k)


@pytest.mark.parametrize("name", ["adagrad", "ftrl", "rmsprop"])
def test_paths_agree(golden_dir, golden_hparams, name, monkeypatch):
    """Row lists (rowlist_min_elems = 0) == the flag sweep; no early user-table update == the default; two runs of the
    same steps are bit-identical."""
    hp = _hp(golden_hparams, optimizer=name)
    feed = _feed(golden_dir, 2)

    def run(thresh=None, early=True):
        if not early:
            monkeypatch.setenv("CLSR_NO_EARLY_USER_UPDATE", "1")
        _, net, _ = _net(hp)
        monkeypatch.delenv("CLSR_NO_EARLY_USER_UPDATE", raising=False)
        if thresh is not None:
            net.rowlist_min_elems = thresh
        f = net.upload(feed, True)
        for _ in range(2):
            net.train_step(f)
        torch.cuda.synchronize()
        return net, net.state_dict()

    net0, sd0 = run()
    for variant in (dict(thresh=0), dict(early=False)):
        net1, sd1 = run(**variant)
        for k in sd0:
            if "embedding" in k or k.startswith("__opt__/") and "dense" not in k and k != "__opt__/state":
                _close(sd1[k].numpy(), sd0[k].numpy(), 1e-7, 1e-6, "%s %s %s" % (name, variant, k))
        for k, t in net1.tab_flags.items():
            assert int(t.sum()) == 0
            assert float(net1.tab_grad[k].abs().max()) == 0.0
    _, sd2 = run()
    for k in sd0:
        assert torch.equal(sd0[k], sd2[k]), k


def test_checkpoint_resume_equals_uninterrupted(golden_dir, golden_hparams):
    hp = _hp(golden_hparams, optimizer="ftrl")
    feeds = [_feed(golden_dir, b) for b in range(3)]
    _, a, _ = _net(hp)
    for fd in feeds:
        a.train_step(a.upload(fd, True))
    _, b, _ = _net(hp)
    for fd in feeds[:2]:
        b.train_step(b.upload(fd, True))
    ck = b.state_dict()
    assert "__opt__/ftrl/dense_accum" in ck and "__opt__/ftrl/item_linear" in ck and "__opt__/state" in ck
    assert not any(k.startswith("__adam__/") for k in ck)
    _, c, _ = _net(hp)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        c.load_state_dict(ck)
    c.train_step(c.upload(feeds[2], True))
    torch.cuda.synchronize()
    sa, sc = a.state_dict(), c.state_dict()
    for k in sa:
        _close(sc[k].numpy(), sa[k].numpy(), 1e-6, 1e-5, k)


def test_adam_checkpoint_into_ftrl_net(golden_dir, golden_hparams):
    _, adam, _ = _net(golden_hparams)
    adam.train_step(adam.upload(_feed(golden_dir, 0), True))
    ck = adam.state_dict()
    _, net, _ = _net(_hp(golden_hparams, optimizer="ftrl"))
    net.dense_m.fill_(7.0)
    with pytest.warns(UserWarning, match="another optimizer"):
        net.load_state_dict(ck)
    assert torch.equal(net.tables["item"].cpu(), ck["sequential/embedding/item_embedding"])
    assert float(net.dense_m.min()) == float(net.dense_m.max()) == pytest.approx(0.1)
    assert float(net.tab_m["item"].min()) == pytest.approx(0.1) and float(net.tab_v["item"].abs().max()) == 0.0
    assert float(net.adam_state[0]) == 0.0


@pytest.mark.parametrize("name,nslots", [("sgd", 0), ("adagrad", 1), ("ftrl", 2), ("adam", 2)])
def test_slot_memory(golden_hparams, name, nslots):
    _, net, _ = _net(_hp(golden_hparams, optimizer=name))
    assert len(net.tab_m) == (len(net.tables) if nslots >= 1 else 0)
    assert len(net.tab_v) == (len(net.tables) if nslots >= 2 else 0)
    assert (net.dense_m is not None) == (nslots >= 1) and (net.dense_v is not None) == (nslots >= 2)
    if name == "rmsprop":
        assert float(net.dense_m.min()) == 1.0


def test_unknown_optimizer_trains_with_gradient_descent(golden_dir, golden_hparams):
    with pytest.warns(UserWarning, match="momentum_sgd"):
        _, net, _ = _net(_hp(golden_hparams, optimizer="momentum_sgd"))
    assert net.optimizer == "gd" and not net.tab_m
    before = net.tables["item"].clone()
    net.train_step(net.upload(_feed(golden_dir, 0), True))
    torch.cuda.synchronize()
    assert not torch.equal(before, net.tables["item"])


def test_bf16_tables_need_adam(golden_hparams):
    with pytest.raises(NotImplementedError, match="bf16.*adagrad|adagrad.*bf16"):
        CLSRNet(_hp(golden_hparams, optimizer="adagrad"), _dims(golden_hparams), device="cuda:0", table_dtype="bf16")


# ---------------------------------------------------------------------------- siblings
@pytest.mark.parametrize("kind", ["gru4rec", "din"])
@pytest.mark.parametrize("name", ["rmsprop", "ftrl"])
def test_sibling_step(golden_dir, golden_hparams, kind, name):
    """One step of GRU4Rec / DIN against sibling_oracle.gradients + the restatement (embedding rows without a
    gradient are the untouched ones: they are covered by the CLSR tests)."""
    from clsr_amd.seqnet import SeqNet
    from oracle import sibling_oracle as S

    hp = _hp(golden_hparams, optimizer=name, model_type={"gru4rec": "GRU4Rec", "din": "DIN"}[kind],
             user_embedding_dim=16, attention_size=40)
    dims = _dims(hp)
    params = S.init_params(dims, hp, kind, seed=5, scale_dense=8.0)
    net = SeqNet(hp, dims, kind=kind, device="cuda:0", seed=0)
    sd = dict(params)
    sd.update(S.init_bn_state(params))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net.load_state_dict(sd, strict=True)
    feed = _feed(golden_dir, 1)
    p = type(params)((k, v.double()) for k, v in params.items())
    _, grads, _, _, _ = S.gradients(p, S.init_bn_state(p), S.to_torch_feed(feed, dtype=torch.float64), hp, kind)
    net.train_step(net.upload(feed, True))
    torch.cuda.synchronize()
    got = net.state_dict()
    lr = float(hp.learning_rate)
    i1, i2 = slot_inits(name)
    n = 0
    for k, g in grads.items():
        pk, g_ = p[k].numpy(), g.double().numpy()
        ep, _, _, _ = restate(name, g_, pk, np.full(pk.shape, i1), np.full(pk.shape, i2), lr)
        gv = np.abs(g_).reshape(-1)
        sel = gv > 4e-4 * float(gv.max())
        upd_got = (got[k].double().numpy() - pk).reshape(-1)[sel]
        upd_exp = (ep - pk).reshape(-1)[sel]
        if upd_exp.size:
            n += 1
            err = np.abs(upd_got - upd_exp)
            assert np.all(err <= 5e-3 * np.abs(upd_exp) + 0.02 * lr), (kind, name, k, float(err.max()))
    assert n >= 8


# ---------------------------------------------------------------------------- model API
def test_fit_with_adagrad_learns_a_learnable_task(tmp_path):
    """CLSRModel.fit with optimizer="adagrad" on the learnable synthetic task of test_model_api_gpu.py."""
    from clsr_amd.clsr import CLSRModel
    from clsr_amd.deeprec_utils import prepare_hparams
    from clsr_amd.sequential_iterator import SASequentialIterator
    from clsr_amd.synthetic import make_tsv_dataset

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = make_tsv_dataset(str(tmp_path), n_users=400, n_items=1500, n_cates=12, n_train=6000, n_valid=300,
                             n_test=300, valid_ngs=4, test_ngs=9, max_hist=20, signal=True)
    hp = prepare_hparams(os.path.join(root, "clsr_amd", "config", "clsr.yaml"), user_vocab=paths["user_vocab"],
                         item_vocab=paths["item_vocab"], cate_vocab=paths["category_vocab"], max_seq_length=20,
                         batch_size=500, train_num_ngs=4, time_unit="s", contrastive_loss="triplet",
                         contrastive_length_threshold=5, is_clip_norm=1, embed_l2=1e-6, layer_l2=1e-6,
                         discrepancy_loss_weight=0.01, contrastive_loss_weight=0.1, learning_rate=ADAGRAD_FIT_LR,
                         optimizer="adagrad", show_step=10 ** 9, save_model=False, MODEL_DIR=None, epochs=6,
                         EARLY_STOP=10)
    model = CLSRModel(hp, SASequentialIterator, seed=7)
    assert model.net.optimizer == "adagrad"
    model.fit(paths["train_data"], paths["valid_data"], valid_num_ngs=4, eval_metric="group_auc")
    after = model.run_weighted_eval(paths["test_data"], num_ngs=9)
    assert after["auc"] > 0.85, after
