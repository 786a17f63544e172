"""GPU tests at BASELINE.json's full sizes (configs[1] Taobao-shaped: 4096 positives x 5 rows, T=50;
configs[2] Kuaishou-shaped: T=250) through size-independent properties -- the float64 oracle is far too
slow at those batch sizes -- plus oracle checks on small batches: the whole step at T=250 on 8 positives here
(about a second of oracle), and the 63 .. 256-step cases of tests/test_long_histories_gpu.py."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hp(cfg, P, **over):
    import sys

    sys.path.insert(0, ROOT)
    from bench import build_hparams

    return build_hparams(cfg, P, **over)


def _net(cfg, P, dedup=True, seed=0, precision="fp32", **over):
    from clsr_amd.net import CLSRNet

    hp = _hp(cfg, P, **over)
    return hp, CLSRNet(hp, dict(Vu=cfg["Vu"], Vi=cfg["Vi"], Vc=cfg["Vc"]), seed=seed, dedup_histories=dedup,
                       precision=precision)


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_taobao_full_size_properties(precision):
    """(precision="fp32": the benchmark's headline arithmetic -- every product at fp32 accuracy -- at the benchmark's size: 1 M
    positions; "fp32x3": the two-piece split products at the same size and tolerances)"""
    from clsr_amd.synthetic import CONFIGS, synthetic_feed

    cfg = CONFIGS["taobao"]
    P, T, G = cfg["P"], cfg["T"], 5
    feed = synthetic_feed(P, T, cfg["Vu"], cfg["Vi"], cfg["Vc"], G=G, lengths="lognormal")
    hp, net = _net(cfg, P, dedup=True, seed=1, precision=precision)
    _, ref = _net(cfg, P, dedup=False, seed=1, precision=precision)     # replicated (reference-shaped) computation
    ref.load_state_dict(net.state_dict())
    f, fr = net.upload(feed, True), ref.upload(feed, True)
    net.capture_grads = ref.capture_grads = True
    out, out_r = net.train_step(f), ref.train_step(fr)
    torch.cuda.synchronize()
    B = P * G
    lens = torch.as_tensor(feed["mask"].sum(1).astype(np.int64))
    # (1) de-duplicated == replicated: logits, losses, every gradient
    assert float((out["logit"] - out_r["logit"]).abs().max()) < 2e-4
    la, lb = net.read_losses(), ref.read_losses()
    for k in la:
        assert abs(la[k] - lb[k]) <= 1e-5 * max(1.0, abs(lb[k])), (k, la[k], lb[k])
    # floor: biases in front of a batch-norm have an analytically ZERO gradient; what is compared there is
    # fp32 summation noise (~1e-5 of the gradient scale over 1M positions)
    gs = max(float(g.abs().max()) for g in ref.captured["dense"].values())
    for name, g in ref.captured["dense"].items():
        d = float((net.captured["dense"][name] - g).abs().max())
        assert d <= 2e-3 * float(g.abs().max()) + 2e-5 * gs, (name, d)
    for k, g in ref.captured["tables"].items():
        d = float((net.captured["tables"][k] - g).abs().max())
        assert d <= 2e-3 * float(g.abs().max()) + 2e-5 * gs, (k, d)
    # (2) attention weights: a probability distribution over the valid steps, exactly 0 past the length
    w = out["w_short"].cpu()
    valid = torch.arange(T)[None, :] < lens[:, None]
    assert float((w.sum(1) - 1).abs().max()) < 1e-5
    assert float(w[~valid].abs().max()) == 0.0 and float(w.min()) >= 0.0
    wl = out["w_long"].cpu()
    assert float((wl.sum(1) - 1).abs().max()) < 1e-5 and float(wl[~valid[::G]].abs().max()) == 0.0
    # (3) gather round trip: history rows are table rows (bit exact), padded steps hold row 0
    hist = out_r["hist_input"].cpu()
    item_tbl, cate_tbl = ref.tables["item"].cpu(), ref.tables["cate"].cpu()
    # tables were updated by the step; compare against a fresh gather instead
    f2 = ref.upload(feed, False)
    hist2 = ref.forward(f2, False)["hist_input"].cpu()
    ih = torch.as_tensor(feed["item_history"].astype(np.int64))
    ch = torch.as_tensor(feed["item_cate_history"].astype(np.int64))
    sel = torch.randint(0, B, (512,))
    assert torch.equal(hist2[sel, :, :cfg["Di"]], item_tbl[ih[sel]])
    assert torch.equal(hist2[sel, :, cfg["Di"]:], cate_tbl[ch[sel]])
    # (4) dynamic_rnn semantics: encoder outputs are exactly zero past the sequence length
    ro = out["rnn_out"].cpu()
    assert float(ro[~valid[::G]].abs().max()) == 0.0
    # (5) alpha in (0,1); fused representation is the convex combination
    al = out["alpha"].cpu()
    assert float(al.min()) > 0 and float(al.max()) < 1
    mo = out["model_output"].cpu()
    L = out["att_fea_long"].cpu().repeat_interleave(G, 0)
    S = out["att_fea_short"].cpu()
    assert float((mo[:, :40] - (al[:, None] * L + (1 - al[:, None]) * S)).abs().max()) < 1e-5
    # (6) the step is deterministic up to atomic ordering and finite
    for k, v in net.state_dict().items():
        assert bool(torch.isfinite(v).all()), k


def test_kuaishou_shape_runs_and_matches_oracle_on_a_slice():
    """T = 250 (long-history stress, BASELINE configs[2]) against the oracle on 8 positives."""
    from clsr_amd.synthetic import synthetic_feed
    from oracle import clsr_oracle as O

    cfg = dict(Vu=500, Vi=3000, Vc=50, Di=32, Dc=8, Du=40, H=40, T=250, P=8)
    feed = synthetic_feed(cfg["P"], cfg["T"], cfg["Vu"], cfg["Vi"], cfg["Vc"], lengths="uniform_long", seed=3)
    hp, net = _net(cfg, cfg["P"], seed=0)
    params = O.init_params(dict(Vu=cfg["Vu"], Vi=cfg["Vi"], Vc=cfg["Vc"]), hp, seed=2, scale_dense=6.0)
    sd = dict(params)
    sd.update(O.init_bn_state(params))
    net.load_state_dict(sd)
    net.capture_grads = True
    p64 = type(params)((k, v.double()) for k, v in params.items())
    _, _, _, ls, _, _, out = O.train_step(p64, O.init_bn_state(p64), O.init_adam(p64), 1,
                                           O.to_torch_feed(feed, dtype=torch.float64), hp)
    got = net.train_step(net.upload(feed, True))
    torch.cuda.synchronize()
    assert float((got["logit"].cpu().double() - out["logit"].detach().reshape(-1)).abs().max()) < 1e-3
    gl = net.read_losses()
    assert abs(gl["loss"] - float(ls["loss"])) < 1e-4 * abs(float(ls["loss"]))
    # the five loss terms, every dense gradient and every gradient table (pre-clip, as captured), at the bars of
    # test_catalogue_dims_match_oracle_on_a_slice
    for k in ("loss", "data_loss", "contrastive_loss", "regular_loss", "discrepancy_loss"):
        assert abs(gl[k] - float(ls[k])) <= 1e-4 * max(1e-3, abs(float(ls[k]))), (k, gl[k], float(ls[k]))
    raw = out["raw_grads"]
    gs = max(float(raw[n].abs().max()) for n in net.captured["dense"])
    tables = {net._table_map()[k]: g for k, g in net.captured["tables"].items()}
    assert set(tables) == set(net._table_map().values())
    for name, g in list(net.captured["dense"].items()) + list(tables.items()):
        exp = raw[name].reshape(g.shape)
        d = float((g.cpu().double() - exp).abs().max())
        assert bool(torch.isfinite(g).all()) and d <= 2e-3 * float(exp.abs().max()) + 3e-6 * gs, (name, d)


def test_kuaishou_full_size_step_is_finite():
    from clsr_amd.synthetic import CONFIGS, synthetic_feed

    cfg = CONFIGS["kuaishou"]
    feed = synthetic_feed(cfg["P"], cfg["T"], cfg["Vu"], cfg["Vi"], cfg["Vc"], lengths="uniform_long")
    hp, net = _net(cfg, cfg["P"])
    for _ in range(2):
        net.train_step(net.upload(feed, True))
    ls = net.read_losses()
    assert all(np.isfinite(v) for v in ls.values()), ls


def test_catalogue_dims_match_oracle_on_a_slice():
    """BASELINE configs[4] layer sizes (item 96 + category 32 = 128 = user = hidden) on a small vocabulary and
    batch: the whole training step against the oracle (logits 1e-3, losses, dense gradients)."""
    from clsr_amd.synthetic import synthetic_feed
    from oracle import clsr_oracle as O

    cfg = dict(Vu=300, Vi=2000, Vc=40, Di=96, Dc=32, Du=128, H=128, T=20, P=24)
    feed = synthetic_feed(cfg["P"], cfg["T"], cfg["Vu"], cfg["Vi"], cfg["Vc"], lengths="lognormal", seed=5)
    hp, net = _net(cfg, cfg["P"], seed=0)
    dims = dict(Vu=cfg["Vu"], Vi=cfg["Vi"], Vc=cfg["Vc"])
    params = O.init_params(dims, hp, seed=2, scale_dense=4.0)
    sd = dict(params)
    sd.update(O.init_bn_state(params))
    net.load_state_dict(sd)
    net.capture_grads = True
    p64 = type(params)((k, v.double()) for k, v in params.items())
    _, _, _, ls, grads, _, out = O.train_step(p64, O.init_bn_state(p64), O.init_adam(p64), 1,
                                               O.to_torch_feed(feed, dtype=torch.float64), hp)
    got = net.train_step(net.upload(feed, True))
    torch.cuda.synchronize()
    assert float((got["logit"].cpu().double() - out["logit"].detach().reshape(-1)).abs().max()) < 1e-3
    gl = net.read_losses()
    for k in ("loss", "data_loss", "contrastive_loss", "regular_loss", "discrepancy_loss"):
        assert abs(gl[k] - float(ls[k])) <= 1e-4 * max(1e-3, abs(float(ls[k]))), (k, gl[k], float(ls[k]))
    gs = max(float(g.abs().max()) for n, g in grads.items() if n in net.captured["dense"])
    for name, g in net.captured["dense"].items():
        d = float((g.cpu().double() - grads[name].reshape(g.shape)).abs().max())
        # floor: 3e-6 of the gradient scale.  The biases in front of a batch-norm have an analytically ZERO gradient; what
        # is compared there is the fp32 rounding of a sum of O(gs) terms -- 1e-6 * gs is ONE ulp of such a term (round 3:
        # 1.49e-7 against a floor of 1.37e-7 after the reduction order inside the statistics kernels changed)
        assert d <= 2e-3 * float(grads[name].abs().max()) + 3e-6 * gs, (name, d)


def test_wide_layer_kernels_match_the_narrow_ones_at_catalogue_widths():
    """The kernels that only engage at the 128-wide layer sizes on many positions -- the in-kernel K loop of the wide-K
    products (pgemm_kloop_kernel) and the 128 x 128-tile weight gradients (csrc/dwwide.hip) -- against the chunked launches
    they replace: one whole training step each way from the same state, BASELINE configs[4] widths, 1 024 x 50 positions."""
    from clsr_amd.synthetic import synthetic_feed

    cfg = dict(Vu=3000, Vi=20000, Vc=400, Di=96, Dc=32, Du=128, H=128, T=50, P=1024)
    feed = synthetic_feed(cfg["P"], cfg["T"], cfg["Vu"], cfg["Vi"], cfg["Vc"], lengths="lognormal", seed=9)
    res = []
    sd = None
    for wide in (True, "clsr_pgemm_dw_wide", False):      # (default: three-piece products; CLSR_DW_WIDE=fp32; the narrow kernels)
        os.environ.pop("CLSR_PGEMM_NO_KLOOP", None)
        hp, net = _net(cfg, cfg["P"], seed=3)
        if sd is None:
            sd = net.state_dict()
        net.load_state_dict(sd)
        net.dw_wide = bool(wide)
        if isinstance(wide, str):
            assert net.dw_wide_entry == "clsr_pgemm_dw_wide_x6"
            net.dw_wide_entry = wide
        net.capture_grads = True
        out = net.train_step(net.upload(feed, True))
        torch.cuda.synchronize()
        res.append((out["logit"].clone(), net.read_losses(), {k: v.clone() for k, v in net.captured["dense"].items()}))
    lb, lossb, gb = res[-1]
    for la, lossa, ga in res[:-1]:
        assert float((la - lb).abs().max()) <= 1e-5
        for k in lossa:
            assert abs(lossa[k] - lossb[k]) <= 2e-6 * max(1.0, abs(lossb[k])), k
        gs = max(float(g.abs().max()) for g in gb.values())
        for name, g in gb.items():
            d = float((ga[name] - g).abs().max())
            assert d <= 5e-4 * float(g.abs().max()) + 2e-5 * gs, (name, d, float(g.abs().max()))


def test_catalogue100m_full_size_step():
    """BASELINE configs[4] on one GPU: 100M-item catalogue (38 GB table + gradient table + lazy-Adam slots),
    128-wide layers, lazy Adam through the involved-row lists.  Properties: finite losses, only rows that were
    touched move, the row lists were not truncated, gradient tables / flags are clean for the next step."""
    from clsr_amd.synthetic import CONFIGS, synthetic_feed

    free, _ = torch.cuda.mem_get_info()
    if free < 200 * (1 << 30):
        pytest.skip("needs ~170 GB of free HBM")
    cfg = CONFIGS["catalogue100m"]
    P, T = 1024, cfg["T"]
    feed = synthetic_feed(P, T, cfg["Vu"], cfg["Vi"], cfg["Vc"], G=5, lengths="lognormal", ids="uniform", seed=11)
    hp, net = _net(cfg, P, optimizer="lazyadam")
    before = net.tables["item"][:4096].clone()
    touched = np.unique(np.concatenate([feed["item_history"].reshape(-1), feed["items"].reshape(-1)]))
    probe = torch.as_tensor(touched[:2048].astype(np.int64), device="cuda")
    before_t = net.tables["item"][probe].clone()
    for _ in range(2):
        net.train_step(net.upload(feed, True))
    torch.cuda.synchronize()
    ls = net.read_losses()
    assert all(np.isfinite(v) for v in ls.values()), ls
    low = torch.as_tensor(touched[touched < 4096].astype(np.int64), device="cuda")
    after = net.tables["item"][:4096]
    moved = (after != before).any(1)
    expect = torch.zeros(4096, dtype=torch.bool, device="cuda")
    expect[low] = True
    assert torch.equal(moved, expect)                      # lazy: untouched rows keep their values bit for bit
    assert bool((net.tables["item"][probe] != before_t).any(1).all())
    assert int(net._buf("rows.count.item", 2, dtype=torch.int32)[1]) == 0
    assert int(net.tab_flags["item"].sum()) == 0
    assert float(net.tab_grad["item"][probe].abs().max()) == 0.0
    del net
    torch.cuda.empty_cache()


def test_catalogue_dims_speed_mode_runs_and_agrees_with_the_parity_mode():
    """128-wide layers (BASELINE configs[4] dims on a small vocabulary) in precision="bf16": the d(hist) product of this width
    (K = 1 536) does not fit the position-tiled bf16 kernel's LDS image -- the step must take the fp32 route for it instead of
    failing (it raised `unsupported shape` until round 5) -- and its logits stay within the speed mode's 2e-3 of the parity mode's."""
    from clsr_amd.net import CLSRNet
    from clsr_amd.synthetic import synthetic_feed

    cfg = dict(Vu=3000, Vi=20000, Vc=400, Di=96, Dc=32, Du=128, H=128, T=50, P=512)
    feed = synthetic_feed(cfg["P"], cfg["T"], cfg["Vu"], cfg["Vi"], cfg["Vc"], lengths="lognormal", seed=5)
    hp, net = _net(cfg, cfg["P"], seed=3)
    neth = CLSRNet(hp, dict(Vu=cfg["Vu"], Vi=cfg["Vi"], Vc=cfg["Vc"]), seed=3, precision="bf16")
    neth.load_state_dict(net.state_dict())
    out = net.train_step(net.upload(feed, True))
    outh = neth.train_step(neth.upload(feed, True))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outh["logit"]).all())
    assert float((out["logit"] - outh["logit"]).abs().max()) <= 2e-3
    la, lb = net.read_losses(), neth.read_losses()
    assert abs(la["loss"] - lb["loss"]) <= 1e-3 * max(1.0, abs(la["loss"]))
