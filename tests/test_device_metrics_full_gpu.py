"""GPU tests of the device metrics beyond auc / logloss / wauc (clsr_amd/csrc/metrics.hip, clsr_amd/device_metrics.py):
the user-weighted rank metrics wmrr / whit@k / wndcg@k for any user id, rmse / acc / f1, mean_alpha.  Everything is
compared with the host functions of clsr_amd/deeprec_utils.py (pinned to the reference by
tests/golden/metrics_golden.json) and with float64 restatements below.  Rank metrics are compared on tie-free float32
scores only (numpy's argsort leaves the order of ties undefined); the device's tie rule has a test of its own."""
import json
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from clsr_amd import device_metrics as DM  # noqa: E402
from clsr_amd.deeprec_utils import HParams, cal_mean_alpha_metric, cal_metric, cal_weighted_metric  # noqa: E402

DEV = "cuda:0"
ALL_W = ["wauc", "wmrr", "whit@1;2;5", "wndcg@1;2;5;100"]
W_KS = [1, 2, 5, 100]


def _hp(**kw):
    d = dict(metrics=[], pairwise_metrics=[], weighted_metrics=list(ALL_W))
    d.update(kw)
    return types.SimpleNamespace(**d)


def _same(got, exp, raw, k, edge=1e-7):
    """equal after the 4-decimal rounding -- or one unit apart when the unrounded value sits ON a rounding boundary
    (within ``edge`` units of the 4th decimal): summation order then decides the direction.  NaN equals NaN."""
    if got != got or exp != exp:
        return got != got and exp != exp
    if abs(got - exp) < 1e-9:
        return True
    frac = (raw[k] * 1e4) % 1.0
    return abs(got - exp) < 1.0000001e-4 and abs(frac - 0.5) < edge


def _device(preds, labels, users, hp, group=1, chunks=3, raw=None, n_users=None, alpha=None):
    acc = DM.DeviceScores(torch.device(DEV))
    n = len(preds)
    cut = sorted(set([0, n] + [n * i // chunks for i in range(1, chunks)]))
    for a, b in zip(cut[:-1], cut[1:]):       # appended in pieces like an evaluation loop does
        acc.append(torch.tensor(preds[a:b], dtype=torch.float32, device=DEV),
                   torch.tensor(labels[a:b], dtype=torch.float32, device=DEV),
                   torch.tensor(np.asarray(users[a:b], dtype=np.int64), dtype=torch.int32, device=DEV),
                   None if alpha is None else torch.tensor(alpha[a:b], dtype=torch.float32, device=DEV))
    return DM.compute(acc, hp, group, True, raw=raw, n_users=n_users, mean_alpha=alpha is not None)


def _host_weighted(preds, labels, users, wm):
    with np.errstate(all="ignore"):           # (0 / 0 of a user without a positive line: NaN, as in the reference)
        return cal_weighted_metric(np.asarray(users), np.asarray(preds, dtype=np.float32), np.asarray(labels), wm)


def _restatement(preds, labels, users, ks):
    """The four weighted metrics in float64 from their definitions; tie-free scores inside every user."""
    preds, labels, users = np.asarray(preds, dtype=np.float32), np.asarray(labels), np.asarray(users)
    N = len(preds)
    out = {k: 0.0 for k in ["wauc", "wmrr"] + ["whit@%d" % k for k in ks] + ["wndcg@%d" % k for k in ks]}
    for u in np.unique(users):
        idx = np.flatnonzero(users == u)
        s, pos = preds[idx], labels[idx] == 1
        assert np.unique(s).size == s.size
        w, P = len(idx) / N, int(pos.sum())
        ranks = np.array([1 + int((s > v).sum()) for v in s[pos]], dtype=np.float64)
        if 0 < P < len(idx):
            gt = sum(int((s[~pos] < v).sum()) for v in s[pos])
            out["wauc"] += w * (gt / (P * (len(idx) - P)))
        out["wmrr"] += w * (float((1.0 / ranks).sum()) / P)
        for k in ks:
            dcg = float((1.0 / np.log2(ranks[ranks <= k] + 1.0)).sum())
            ideal = float((1.0 / np.log2(np.arange(1, min(k, P, len(idx)) + 1) + 1.0)).sum())
            out["wndcg@%d" % k] += w * (dcg / ideal)
            out["whit@%d" % k] += w * (1.0 if (ranks <= k).any() else 0.0)
    return out


def _tie_free(n, rng):
    """n distinct float32 scores in (0, 1) (n < 2^24)."""
    p = ((rng.permutation(n) + 0.5) / n).astype(np.float32)
    assert np.unique(p).size == n
    return p


def _check(preds, labels, users, wm, ks, n_users=None, restate=True):
    raw = {}
    hp = _hp(weighted_metrics=wm)
    got = _device(preds, labels, users, hp, raw=raw, n_users=n_users)
    exp = _host_weighted(preds, labels, users, wm)
    assert set(got) == set(exp), (sorted(got), sorted(exp))
    for k in exp:
        print("%s: device %.17g host %s" % (k, raw[k], exp[k]))
        assert _same(got[k], exp[k], raw, k), (k, got[k], exp[k], raw[k])
    if restate:
        # the kernel's only inexact steps are float64 operations and ONE 2^-60 fixed-point rounding per user and metric
        # (a few thousand users at most here: below 1e-14); the bound is that of
        # test_wauc_with_more_positives_per_user_than_one_tile
        ref = _restatement(preds, labels, users, ks)
        for k in exp:
            assert abs(raw[k] - ref[k]) <= 1e-12, (k, raw[k], ref[k])
    return got, raw


# ------------------------------------------------------------------------------------------ 1. reference-captured values
def test_reference_captured_weighted_hits(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "metrics_golden.json")))
    labels = np.asarray(g["labels"], dtype=np.float64).reshape(-1)
    preds = np.asarray(g["preds"], dtype=np.float64).reshape(-1)
    users = np.asarray(g["users"]).astype(np.int64)
    got = _device(preds, labels, users, _hp(weighted_metrics=["wauc", "whit@1;2"]))
    assert set(got) == {"wauc", "whit@1", "whit@2"}
    # (both orders of the fixture's tied lines give these values: the ties do not decide a top-2 membership)
    assert got["whit@1"] == 0.0833 == g["expected"]["whit@1"] and got["whit@2"] == 0.1667 == g["expected"]["whit@2"]
    assert got["wauc"] == 0.4728 == g["expected"]["wauc"]


# ------------------------------------------------------------------------------------------ 2. equal to the host
def _grouped_file(n_groups, group, n_users, seed, shuffle=False):
    rng = np.random.default_rng(seed)
    N = n_groups * group
    labels = np.zeros((n_groups, group))
    labels[:, 0] = 1.0
    extra = rng.random((n_groups, group)) < 0.03          # a few groups with more than one positive
    extra[:, -1] = False                                   # (always at least one negative)
    labels = np.maximum(labels, extra).reshape(-1)
    users = np.repeat(rng.integers(0, n_users, n_groups), group)
    preds = _tie_free(N, rng)
    if shuffle:                                            # the lines of every user spread over the file
        order = rng.permutation(N)
        labels, users = labels[order], users[order]
    return preds, labels, users


@pytest.mark.parametrize("n_groups,group,n_users,shuffle", [(2000, 5, 300, False), (700, 100, 64, False),
                                                            (400, 5, 1, False), (1, 7, 1, False), (2000, 5, 300, True)])
def test_weighted_rank_metrics_equal_the_host(n_groups, group, n_users, shuffle):
    preds, labels, users = _grouped_file(n_groups, group, n_users, n_groups + group + shuffle, shuffle)
    got, raw = _check(preds, labels, users, ALL_W, W_KS, n_users=n_users)
    assert len(got) == 2 + 3 + 4
    if n_users > 1:
        assert 0.0 < raw["whit@1"] < raw["whit@5"] <= 1.0 and raw["wndcg@2"] < raw["wndcg@100"]     # (not degenerate)


# ------------------------------------------------------------------------------------------ 3. segment and tile edges
def test_segment_and_tile_edges():
    """The user kernel takes 64 positives at a time (one per lane) and streams the user's lines in tiles of 64: users
    with 1 / 63 / 64 / 65 / 128 / 129 lines, users with 63 / 64 / 65 / 129 positives, among 150 small users, shuffled.
    No wauc: single-line and all-positive users are legal."""
    rng = np.random.default_rng(64)
    ids = rng.choice(1 << 20, 160, replace=False)
    users, labels = [], []
    for u, n in zip(ids[:6], (1, 63, 64, 65, 128, 129)):
        npos = 1 if n == 1 else int(rng.integers(1, 4))
        users += [u] * n
        labels += [1.0] * npos + [0.0] * (n - npos)
    for u, npos in zip(ids[6:10], (63, 64, 65, 129)):
        nneg = int(rng.integers(0, 200)) if npos != 64 else 0          # (one of them has positives only)
        users += [u] * (npos + nneg)
        labels += [1.0] * npos + [0.0] * nneg
    for u in ids[10:]:
        npos, nneg = int(rng.integers(1, 5)), int(rng.integers(0, 9))
        users += [u] * (npos + nneg)
        labels += [1.0] * npos + [0.0] * nneg
    order = rng.permutation(len(users))
    users, labels = np.asarray(users, dtype=np.int64)[order], np.asarray(labels)[order]
    preds = _tie_free(len(users), rng)
    wm = ["wmrr", "whit@1;2;5", "wndcg@1;2;5;100"]
    _check(preds, labels, users, wm, W_KS)
    _check(preds, labels, users, wm, W_KS, n_users=1 << 20)


# ------------------------------------------------------------------------------------------ 4. tie rule
def test_ties_inside_a_user_break_towards_the_later_line_of_the_file():
    #        line:   0    1    2    3    4    5    6
    users = np.array([7, 3, 7, 3, 7, 3, 7])
    preds = np.array([0.5, 0.5, 0.5, 0.5, 0.1, 0.1, 0.05])
    labels = np.array([1.0, 0, 0, 1.0, 0, 0, 0])
    # user 7 (4 lines): its positive (line 0) is tied with its LATER negative (line 2) and ranks behind it: rank 2
    # user 3 (3 lines): its positive (line 3) is tied with its EARLIER negative (line 1) and ranks ahead of it: rank 1
    # the equal scores of the other user's lines (later ones included) count for nothing
    raw = {}
    got = _device(preds, labels, users, _hp(weighted_metrics=["wmrr", "whit@1"]), chunks=1, raw=raw)
    assert abs(raw["wmrr"] - (4.0 / 7 * 0.5 + 3.0 / 7 * 1.0)) < 1e-12 and got["wmrr"] == 0.7143
    assert abs(raw["whit@1"] - 3.0 / 7) < 1e-12 and got["whit@1"] == 0.4286


# ------------------------------------------------------------------------------------------ 5. large and colliding ids
def _users_file(ids, seed):
    rng = np.random.default_rng(seed)
    users, labels = [], []
    for u in ids:
        npos, nneg = int(rng.integers(1, 4)), int(rng.integers(1, 7))
        users += [int(u)] * (npos + nneg)
        labels += [1.0] * npos + [0.0] * nneg
    order = rng.permutation(len(users))
    users, labels = np.asarray(users, dtype=np.int64)[order], np.asarray(labels)[order]
    return _tie_free(len(users), rng), labels, users


def test_large_and_colliding_user_ids():
    """Ids that a sort on (id mod 2^18) merges: u, u + 2^18, u + 2^30, and the largest int32."""
    assert DM.supported(_hp(), 10 ** 6, 5)
    base = np.random.default_rng(18).choice(1 << 18, 40, replace=False)
    ids = sorted(set(int(u) + off for u in base for off in (0, 1 << 18, 1 << 30)) | {2 ** 31 - 1, 0})
    preds, labels, users = _users_file(ids, 5)
    for n_users in (None, 2 ** 31 - 1):
        _check(preds, labels, users, ALL_W, W_KS, n_users=n_users)
    low = np.random.default_rng(19).choice(300000 - (1 << 18), 40, replace=False)
    ids = sorted(set(int(u) + off for u in low for off in (0, 1 << 18)) | {299999})
    preds, labels, users = _users_file(ids, 6)
    _check(preds, labels, users, ALL_W, W_KS, n_users=300000)


# ------------------------------------------------------------------------------------------ 6. point metrics
def _point_case(preds, labels, metrics):
    hp = _hp(metrics=metrics, weighted_metrics=[])
    raw = {}
    got = _device(preds, labels, np.zeros(len(preds), dtype=np.int64), hp, raw=raw)
    p32 = np.asarray(preds, dtype=np.float32)
    exp = cal_metric(list(labels), list(p32), metrics)
    assert set(got) == set(exp)
    for k in exp:
        print("%s: device %.17g host %s" % (k, raw[k], exp[k]))
        if k == "rmse":       # the root of the ROUNDED mean squared error: the boundary is one of the mse
            assert _same(round(got[k] ** 2, 4), round(float(exp[k]) ** 2, 4), raw, "mse"), (got[k], exp[k], raw["mse"])
        else:
            assert _same(got[k], exp[k], raw, k), (k, got[k], exp[k], raw[k])
    # acc and f1 come from integer counts: the host's unrounded expressions, bit for bit
    pp, lab = p32 >= 0.5, labels == 1
    if "acc" in metrics:
        assert raw["acc"] == float(np.mean(pp.astype(np.float64) == labels))
    if "f1" in metrics:
        tp = float(np.sum(pp & lab))
        den = 2.0 * tp + float(np.sum(pp & ~lab)) + float(np.sum(~pp & lab))
        assert raw["f1"] == (tp * 2.0 / den if den > 0 else 0.0)
    return got, raw


def test_point_metrics_equal_the_host():
    rng = np.random.default_rng(6)
    N = 3001
    preds = rng.random(N).astype(np.float32)
    preds[:9] = [0.5, 0.5, 0.0, 0.0, 1.0, 1.0, np.nextafter(np.float32(0.5), np.float32(0)), 0.5, 1e-13]
    labels = (rng.random(N) < 0.3).astype(np.float64)
    labels[:9] = [1, 0, 1, 0, 1, 0, 1, 1, 0]
    got, raw = _point_case(preds, labels, ["auc", "logloss", "rmse", "acc", "f1"])
    mse = float(np.mean((labels - preds.astype(np.float64)) ** 2))
    assert abs(raw["mse"] - mse) < 1e-12        # one 2^-32 fixed-point rounding per block of 2048 lines, over N
    assert 0.0 < raw["f1"] < 1.0 and 0.0 < raw["acc"] < 1.0
    # nothing predicted positive, no positive label: f1 = 0 / 0 -> 0.0
    got, raw = _point_case(np.full(70, 0.25, dtype=np.float32) * rng.random(70).astype(np.float32), np.zeros(70),
                           ["logloss", "rmse", "acc", "f1"])
    assert got["f1"] == 0.0 and got["acc"] == 1.0


def test_mean_alpha_equals_the_host():
    rng = np.random.default_rng(7)
    N = 2500
    preds, labels = rng.random(N).astype(np.float32), (rng.random(N) < 0.2).astype(np.float32)
    alpha = rng.random(N).astype(np.float32)
    raw = {}
    got = _device(preds, labels, np.zeros(N, dtype=np.int64), _hp(metrics=["logloss"], weighted_metrics=[]), raw=raw,
                  alpha=alpha)
    exp = cal_mean_alpha_metric(alpha, labels)
    exact = float((alpha.astype(np.float64) * labels).sum() / labels.sum())
    assert abs(raw["mean_alpha"] - exact) < 1e-9
    # (the host sums float32 values in float32: a relative error of up to ~1e-6, 1e-2 units of the 4th decimal)
    assert set(got) == {"logloss", "mean_alpha"} and _same(got["mean_alpha"], exp["mean_alpha"], raw, "mean_alpha", 1e-2)


# ------------------------------------------------------------------------------------------ 7. NaN and error parity
def test_nan_and_error_parity():
    users = np.array([1, 1, 1, 2, 2, 2, 2])
    preds = np.array([0.9, 0.3, 0.2, 0.8, 0.7, 0.6, 0.1], dtype=np.float32)
    labels = np.array([0.0, 1.0, 0, 0, 0, 0, 0])           # user 2 has no positive line
    wm = ["wmrr", "wndcg@2", "whit@2"]
    got = _device(preds, labels, users, _hp(weighted_metrics=wm), chunks=1)
    exp = _host_weighted(preds, labels, users, wm)
    assert set(got) == set(exp) == {"wmrr", "wndcg@2", "whit@2"}
    assert np.isnan(got["wmrr"]) and np.isnan(exp["wmrr"]) and np.isnan(got["wndcg@2"]) and np.isnan(exp["wndcg@2"])
    assert got["whit@2"] == exp["whit@2"] == round(3.0 / 7, 4)
    with pytest.raises(ValueError, match="Only one class present"):
        _device(preds, labels, users, _hp(weighted_metrics=["wmrr", "wauc"]), chunks=1)
    with pytest.raises(ValueError, match="Only one class present"):
        _host_weighted(preds, labels, users, ["wmrr", "wauc"])
    # nine distinct k over whit + wndcg: host path (the other cases of supported(): test_device_metrics_supported_cpu.py),
    # and compute() itself refuses such a request by name
    nine = _hp(weighted_metrics=["whit@1;2;3;4", "wndcg@3;4;5;6;7;8;9"])
    assert not DM.supported(nine, 100, 5)
    with pytest.raises(ValueError, match="no device form"):
        _device(preds, labels, users, nine, chunks=1)


# ------------------------------------------------------------------------------------------ 8. determinism
def test_two_computations_give_identical_raw_values():
    preds, labels, users = _grouped_file(2000, 5, 300, 8, shuffle=True)
    hp = _hp(metrics=["auc", "logloss", "rmse", "acc", "f1"])
    raws = []
    acc = DM.DeviceScores(torch.device(DEV))
    acc.append(torch.tensor(preds, device=DEV), torch.tensor(labels, dtype=torch.float32, device=DEV),
               torch.tensor(users, dtype=torch.int32, device=DEV))
    for _ in range(2):
        raws.append({})
        DM.compute(acc, hp, 1, True, raw=raws[-1])
    assert raws[0] == raws[1] and len(raws[0]) == 5 + 1 + 9


# ------------------------------------------------------------------------------------------ 9. model level
def test_model_runs_every_weighted_metric_and_mean_alpha_on_the_device(golden_dir, golden_hparams, monkeypatch):
    import pickle

    from clsr_amd.clsr import CLSRModel
    from clsr_amd.sequential_iterator import SASequentialIterator
    from oracle import clsr_oracle as O

    wm = ["wauc", "wmrr", "whit@1;2", "wndcg@1;2"]
    hp = HParams(**dict(golden_hparams.values(), weighted_metrics=wm, metrics=["auc", "logloss", "rmse", "acc", "f1"]))
    model = CLSRModel(hp, SASequentialIterator, seed=2)
    # weights with some spread (see test_model_evaluation_on_the_device_equals_the_host_path)
    dims = dict(Vu=len(pickle.load(open(hp.user_vocab, "rb"))), Vi=len(pickle.load(open(hp.item_vocab, "rb"))),
                Vc=len(pickle.load(open(hp.cate_vocab, "rb"))))
    params = O.init_params(dims, hp, seed=5, scale_dense=8.0)
    sd = dict(params)
    sd.update(O.init_bn_state(params))
    model.net.load_state_dict(sd)
    valid = os.path.join(golden_dir, "data", "valid_data")
    assert model._device_eval(valid, 4, True) is not None
    dev = model.run_weighted_eval(valid, num_ngs=4)
    dev_a = model.run_weighted_eval(valid, num_ngs=4, calc_mean_alpha=True)
    vocab = model.user_vocab_length
    model.user_vocab_length = 2 ** 20
    assert model._device_eval(valid, 4, True, mean_alpha=True) == dev_a
    model.user_vocab_length = vocab

    monkeypatch.setenv("CLSR_HOST_METRICS", "1")
    assert model._device_eval(valid, 4, True) is None
    host = model.run_weighted_eval(valid, num_ngs=4)
    host_a = model.run_weighted_eval(valid, num_ngs=4, calc_mean_alpha=True)
    users, preds, labels, alphas = [], [], [], []
    for batch in model.iterator.load_data_from_file(valid, min_seq_length=model.min_seq_length, batch_num_ngs=0):
        if batch:
            u, p, l, a = model.eval_with_user_and_alpha(model.sess, batch)
            users.extend(np.reshape(u, -1)), preds.extend(np.reshape(p, -1)), labels.extend(np.reshape(l, -1))
            alphas.extend(np.reshape(a, -1))
    users, preds, labels = np.asarray(users), np.asarray(preds, dtype=np.float32), np.asarray(labels)
    tie_free = all(np.unique(preds[users == u]).size == int((users == u).sum()) for u in np.unique(users))
    keys = set(host) if tie_free else {"auc", "logloss", "rmse", "acc", "f1", "wauc"}
    print("tie-free per user:", tie_free, "device", dev_a, "host", host_a)
    assert set(dev) == set(host) and {"wmrr", "whit@2", "wndcg@1", "rmse", "f1"} <= set(dev)
    assert set(dev_a) == set(host_a) == set(host) | {"mean_alpha"}
    # referee for a weighted value that sits on a rounding boundary (sums of n_u / N over few lines do: 4 / 640 = 0.00625)
    ref = _restatement(preds, labels, users, [1, 2]) if tie_free else {}
    for k in keys:
        assert dev_a[k] == dev[k]
        if k in ref and k != "wauc":
            assert _same(dev[k], host[k], ref, k) and _same(dev_a[k], host_a[k], ref, k), (k, dev[k], host[k], ref[k])
        else:
            assert dev[k] == host[k] and dev_a[k] == host_a[k], (k, dev[k], host[k])
    exact = float((np.asarray(alphas, dtype=np.float64) * labels).sum() / labels.sum())
    assert _same(dev_a["mean_alpha"], host_a["mean_alpha"], {"mean_alpha": exact}, "mean_alpha", 1e-2)
