"""GPU parity of the whole CLSR step (forward, losses, gradients, clip norms, Adam, BN moving
statistics, eval-mode scoring) against the float64 oracle on batches captured from the
reference iterator (tests/golden/iterator_*.npz).  Tolerance on logits: 1e-3 is the bar stated by
BASELINE.json:north_star; the fp32 kernels are held to ~1e-4 here."""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from clsr_amd.net import CLSRNet  # noqa: E402
from clsr_amd.params import TABLES  # noqa: E402


def _feed(golden_dir, name, b=0):
    g = np.load(os.path.join(golden_dir, name))
    pre = "b%d_" % b
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}


def _dims(hp):
    return dict(Vu=len(pickle.load(open(hp.user_vocab, "rb"))), Vi=len(pickle.load(open(hp.item_vocab, "rb"))),
                Vc=len(pickle.load(open(hp.cate_vocab, "rb"))))


def _variant(hp, **kw):
    hp2 = copy.deepcopy(hp)
    for k, v in kw.items():
        setattr(hp2, k, v)
    return hp2


def _close(got, exp, rtol, atol, name):
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    exp = torch.as_tensor(exp).detach().double().cpu().reshape(-1)
    assert got.shape == exp.shape, (name, got.shape, exp.shape)
    err = (got - exp).abs()
    excess = float((err - (atol + rtol * exp.abs())).max())
    assert excess <= 0, "%s: max abs err %.3e, max |exp| %.3e" % (name, float(err.max()), float(exp.abs().max()))


def _setup(hp, dedup, seed=3, precision="fp32"):
    from oracle import clsr_oracle as O

    dims = _dims(hp)
    params32 = O.init_params(dims, hp, seed=seed, scale_dense=8.0)
    split = dedup == "split"     # de-duplicated histories + the history-level query columns split off the
    net = CLSRNet(hp, dims, device="cuda:0", seed=0, dedup_histories=bool(dedup), precision=precision)   # product term at ANY width
    if split:
        net.split_query_min = 0
    sd = dict(params32)
    for k, v in O.init_bn_state(params32).items():
        sd[k] = v
    net.load_state_dict(sd, strict=True)
    params64 = type(params32)((k, v.double()) for k, v in params32.items())
    return O, net, params64


CONFIGS = [
    dict(),
    dict(sequential_model="gru", contrastive_loss="bpr"),
    dict(interest_evolve=False, predict_long_short=False),
    dict(manual_alpha=True, manual_alpha_value=0.3),
    dict(sequential_model="lstm"),
    dict(embed_l1=2e-5, layer_l1=3e-5, embed_l2=1e-4),     # L1 regularisers (base_model.py:134-147), off by default
    dict(att_fcn_layer_sizes=[8, 12]),     # attention widths below one MFMA tile (masked lanes: clamped addresses)
]


# "fp32": every product at fp32 accuracy (fp32-input MFMAs or three bf16 pieces per operand) -- the reference's arithmetic, the
# benchmark's headline; "fp32x3": fp32 storage, the recurrences / attention backward / encoder tail as TWO-piece split-bf16 sums
# (csrc/rnn.hip, attbwdx3.hip, encbwd.hip ...) -- held to the SAME tolerances
@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
@pytest.mark.parametrize("dedup", [True, False, "split"])
@pytest.mark.parametrize("cfg", range(len(CONFIGS)))
def test_train_step_matches_oracle(golden_dir, golden_hparams, cfg, dedup, precision):
    hp = _variant(golden_hparams, **CONFIGS[cfg])
    O, net, params = _setup(hp, dedup, precision=precision)
    feed = _feed(golden_dir, "iterator_train_sa.npz", b=cfg % 3)
    tf = O.to_torch_feed(feed, dtype=torch.float64)
    bn = O.init_bn_state(params)
    adam = O.init_adam(params)
    new_p, new_bn, _, ls, grads, norms, out = O.train_step(params, bn, adam, 1, tf, hp)

    net.capture_grads = True
    f = net.upload(feed, True)
    got = net.train_step(f)
    torch.cuda.synchronize()
    B, T, G, Hn = net.last_shape
    rep = (lambda t: t) if G == 1 else (lambda t: t[::G])
    # ---- forward values
    _close(got["logit"], out["logit"], 1e-4, 1e-4, "logit")
    if not hp.manual_alpha:
        _close(got["alpha"], out["alpha"], 1e-4, 1e-5, "alpha")
    _close(got["att_fea_short"], out["att_fea_short"], 1e-4, 1e-5, "att_fea_short")
    _close(got["att_fea_long"], rep(out["att_fea_long"]), 1e-4, 1e-5, "att_fea_long")
    _close(got["hist_mean"], rep(out["hist_mean"]), 1e-5, 1e-6, "hist_mean")
    _close(got["hist_recent"], rep(out["hist_recent"]), 1e-5, 1e-6, "hist_recent")
    _close(got["short_intention"], rep(out["short_intention"]), 1e-4, 1e-5, "short_term_intention")
    _close(got["rnn_out"], rep(out["rnn_out"]), 1e-4, 1e-5, "rnn_outputs")
    _close(got["w_short"], out["w_short"], 1e-4, 1e-6, "short attention weights")
    # ---- the five loss terms of CLSRModel.train
    gl = net.read_losses()
    for k in ("loss", "data_loss", "regular_loss", "contrastive_loss", "discrepancy_loss"):
        _close([gl[k]], [float(ls[k])], 1e-5, 1e-7, k)
    # ---- gradients of every dense variable (pre-clip, regularisers included) and their norms
    cap = net.captured
    raw = out["raw_grads"]
    # absolute floor: biases that feed a batch-norm (and the softmax-invariant output bias) have an
    # exactly-zero gradient which fp32 accumulation returns as noise of a few 1e-7 of the layer's scale (the sum
    # of ~20 k row gradients that cancel analytically; its value moves with the summation order upstream)
    floor = 4e-6 * max(float(raw[n].abs().max()) for n in net.dense_names)
    for i, name in enumerate(net.dense_names):
        scale = float(raw[name].abs().max()) + 1e-12
        _close(cap["dense"][name], raw[name], 2e-3, 2e-4 * scale + floor, "grad " + name)
        _close([float(cap["dense_sumsq"][i]) ** 0.5], [norms[name]], 1e-3, 20 * floor, "norm " + name)
    # ---- embedding tables: dense-equivalent gradients; IndexedSlices clip norms
    ss = cap["table_sumsq"].cpu().numpy()
    tab_norm = dict(item=(ss[0] + ss[2] + ss[4]) ** 0.5, cate=(ss[1] + ss[3] + ss[5]) ** 0.5,
                    user_long=(ss[6] + ss[8]) ** 0.5, user_short=(ss[7] + ss[9]) ** 0.5)
    for key, name in TABLES.items():
        scale = float(raw[name].abs().max()) + 1e-12
        _close(cap["tables"][key], raw[name], 2e-3, 2e-4 * scale + floor, "grad " + name)
        if not dedup:
            # replicated computation == reference IndexedSlices semantics
            _close([tab_norm[key]], [norms[name]], 1e-3, 1e-7, "clip norm " + name)
    # ---- Adam step + BN moving statistics
    sd = net.state_dict()
    lr = hp.learning_rate
    for name in list(net.dense_names) + list(TABLES.values()):
        g_ = grads[name].double().reshape(-1)
        # Adam's first step is ~lr*sign(g): only compare where the gradient is well above fp32 noise
        sel = g_.abs() > 100 * floor
        upd_got = (sd[name].double().reshape(-1) - params[name].reshape(-1))[sel]
        upd_exp = (new_p[name].reshape(-1) - params[name].reshape(-1))[sel]
        if upd_exp.numel():
            _close(upd_got, upd_exp, 5e-3, 0.02 * lr, "adam update " + name)
    for k, v in new_bn.items():
        _close(sd[k], v, 1e-4, 1e-6, k)
    assert float(net.adam_state[0]) == 1.0


@pytest.mark.parametrize("cfg", [0, 1])
def test_eval_scores_match_oracle(golden_dir, golden_hparams, cfg):
    hp = _variant(golden_hparams, **CONFIGS[cfg])
    O, net, params = _setup(hp, True)
    bn = O.init_bn_state(params)
    # make the moving statistics non-trivial: one oracle training step first, mirrored on the GPU
    feed_t = _feed(golden_dir, "iterator_train_sa.npz", b=0)
    new_p, new_bn, _, _, _, _, _ = O.train_step(params, bn, O.init_adam(params), 1,
                                               O.to_torch_feed(feed_t, dtype=torch.float64), hp)
    net.train_step(net.upload(feed_t, True))
    for b in range(2):
        feed = _feed(golden_dir, "iterator_eval_sa.npz", b=b)
        exp = O.predict(new_p, new_bn, O.to_torch_feed(feed, dtype=torch.float64), hp)
        f = net.upload(feed, False)
        got = net.forward(f, False)
        torch.cuda.synchronize()
        # parameters differ by one Adam step computed in fp32 vs fp64 -> slightly looser
        _close(torch.sigmoid(got["logit"]), exp["pred"], 1e-3, 2e-4, "pred")
        _close(got["logit"], exp["logit"], 1e-3, 1e-3, "logit")


def test_three_steps_stay_on_the_oracle_trajectory(golden_dir, golden_hparams):
    hp = golden_hparams
    O, net, params = _setup(hp, True)
    bn, adam = O.init_bn_state(params), O.init_adam(params)
    for step in range(3):
        feed = _feed(golden_dir, "iterator_train_sa.npz", b=step)
        params, bn, adam, ls, _, _, _ = O.train_step(params, bn, adam, step + 1,
                                                     O.to_torch_feed(feed, dtype=torch.float64), hp)
        net.train_step(net.upload(feed, True))
        gl = net.read_losses()
        assert abs(gl["loss"] - float(ls["loss"])) < 2e-3 * abs(float(ls["loss"])), (step, gl, ls)


def _compact(feed, G):
    """History-level form of a row-layout training feed (what sequential_iterator.LazyFeed.compact holds)."""
    c = {k: feed[k] for k in ("labels", "items", "cates")}
    for k in ("users", "item_history", "item_cate_history", "mask", "time_from_first_action", "time_to_now"):
        assert np.array_equal(np.repeat(feed[k][::G], G, axis=0), feed[k])
        c[k] = np.ascontiguousarray(feed[k][::G])
    c["hist_group"] = G
    return c


@pytest.mark.parametrize("dedup", [True, False])
def test_compact_feed_is_the_same_step(golden_dir, golden_hparams, dedup):
    """A compact (history-level) training feed gives the same step as the (1+ngs)-fold repeated row
    layout of the reference iterator: same logits, losses and updated variables (the embedding
    gradients are atomic float sums, hence a tiny tolerance instead of bit equality)."""
    hp = golden_hparams
    feed = _feed(golden_dir, "iterator_train_sa.npz", b=1)
    G = hp.train_num_ngs + 1
    res = []
    for fd in (feed, _compact(feed, G)):
        _, net, _ = _setup(hp, dedup)
        f = net.upload(fd, True)
        assert bool(f["compact"]) == (dedup and "hist_group" in fd)
        out = net.train_step(f)
        torch.cuda.synchronize()
        res.append((out["logit"].clone(), net.read_losses(), {k: v.clone() for k, v in net.state_dict().items()}))
    (l0, ls0, sd0), (l1, ls1, sd1) = res
    assert torch.equal(l0, l1)
    for k in ls0:
        assert abs(ls0[k] - ls1[k]) <= 1e-6 * max(1.0, abs(ls0[k])), k
    for k in sd0:
        _close(sd1[k], sd0[k], 1e-5, 1e-6, k)


def test_row_list_optimizer_path_equals_sweep(golden_dir, golden_hparams):
    """lazyadam through the compacted involved-row lists (the path huge catalogues take) == the flag sweep."""
    hp = _variant(golden_hparams, optimizer="lazyadam")
    feed = _feed(golden_dir, "iterator_train_sa.npz", b=2)
    res = []
    for thresh in (1 << 26, 0):
        _, net, _ = _setup(hp, True)
        net.rowlist_min_elems = thresh
        f = net.upload(feed, True)
        for _ in range(2):
            net.train_step(f)
        torch.cuda.synchronize()
        res.append((net.read_losses(), {k: v.clone() for k, v in net.state_dict().items()},
                    {k: t.clone() for k, t in net.tab_flags.items()}, {k: t.clone() for k, t in net.tab_grad.items()}))
    (ls0, sd0, fl0, tg0), (ls1, sd1, fl1, tg1) = res
    for k in ls0:
        assert abs(ls0[k] - ls1[k]) <= 1e-6 * max(1.0, abs(ls0[k])), (k, ls0[k], ls1[k])
    # (dense biases in front of a batch-norm have a zero gradient: their Adam steps follow summation noise and
    #  differ from run to run -- the optimiser paths under test only touch the embedding tables)
    tabs = [k for k in sd0 if "embedding" in k]
    assert len(tabs) >= 4
    for k in tabs:
        _close(sd1[k], sd0[k], 1e-5, 1e-7, k)
    for k in fl0:   # both paths leave the flags and gradient tables cleared for the next step
        assert int(fl1[k].sum()) == 0 and int(fl0[k].sum()) == 0
        assert float(tg1[k].abs().max()) == 0.0 and float(tg0[k].abs().max()) == 0.0


def _step_is_idle(net):
    fresh = type(net._step)()
    return all(getattr(net._step, k) == getattr(fresh, k) for k in fresh.__slots__)


def _fail_a_step(net, f, monkeypatch):
    """One training step that raises on the HOST between the forward and the backward of the heads (nothing faults on the
    device); the monkeypatch is undone before returning."""
    def boom(*a, **kw):
        raise RuntimeError("host exception inside a step")

    with monkeypatch.context() as m:
        m.setattr(net, "_heads_fused_step", boom)
        m.setattr(net, "_heads_bwd_launches", boom)
        with pytest.raises(RuntimeError, match="host exception inside a step"):
            net.train_step(f)


@pytest.mark.parametrize("overlap", [True, False])
def test_host_exception_in_a_step_leaves_no_step_state(golden_dir, golden_hparams, monkeypatch, overlap):
    """A step that raises on the host leaves neither per-step state nor stream bookkeeping for the next step to trip over."""
    _, net, _ = _setup(golden_hparams, True)
    net.overlap = overlap
    f = net.upload(_feed(golden_dir, "iterator_train_sa.npz", b=0), True)
    net.train_step(f)
    assert _step_is_idle(net)
    _fail_a_step(net, f, monkeypatch)
    torch.cuda.synchronize()
    assert _step_is_idle(net)
    assert net._joins == []
    assert not any(net._dw_pending.values()) and not any(net._rp_pending.values())
    assert net._dw_batch is None
    assert net._ws_tag == ""
    assert not net._dw_async


def test_failed_step_does_not_change_the_next_update(golden_dir, golden_hparams, monkeypatch):
    """Twin nets, one of which went through a step that raised on the host: restored from the same checkpoint, both make
    the bit-identical next update the way the data-parallel stepper drives it (``train_step(apply=False)`` +
    ``_apply_updates()``), and the Adam clock advances by one on both.  Two UNDISTURBED twins are bit-equal through this
    sequence (deterministic embedding gradients, batched weight-gradient reduction; checked on the commit before this
    test existed), so the comparison is exact.  A stale ``ticked`` left by the failed step made the update skip the clock
    and the distinct-user count."""
    from clsr_amd import ops

    feed = _feed(golden_dir, "iterator_train_sa.npz", b=0)
    (_, a, _), (_, b, _) = _setup(golden_hparams, True), _setup(golden_hparams, True)
    ck = a.state_dict()
    fa, fb = a.upload(feed, True), b.upload(feed, True)
    _fail_a_step(b, fb, monkeypatch)
    torch.cuda.synchronize()
    for net, f in ((a, fa), (b, fb)):
        net.load_state_dict(ck)
        t0 = float(net.adam_state[0])
        with ops.stream_scope():
            net.train_step(f, apply=False)
            net._apply_updates()
        torch.cuda.synchronize()
        assert float(net.adam_state[0]) == t0 + 1.0
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
