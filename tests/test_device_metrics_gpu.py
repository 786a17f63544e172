"""GPU tests of the device-side evaluation metrics (clsr_amd/csrc/metrics.hip, clsr_amd/device_metrics.py) against
the host implementations of clsr_amd/deeprec_utils.py -- which are themselves pinned to the reference's cal_metric /
cal_weighted_metric by tests/golden/metrics_golden.json -- and against that reference-captured fixture directly."""
import json
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from clsr_amd import device_metrics as DM  # noqa: E402
from clsr_amd.deeprec_utils import cal_metric, cal_weighted_metric  # noqa: E402

DEV = "cuda:0"


def _hp(**kw):
    d = dict(metrics=["auc", "logloss"], pairwise_metrics=["mean_mrr", "ndcg@2;4;6", "hit@2;4;6", "group_auc"],
             weighted_metrics=["wauc"])
    d.update(kw)
    return types.SimpleNamespace(**d)


def _same(got, exp, raw, k):
    """equal after the 4-decimal rounding -- or one unit apart when the exact value sits ON a rounding boundary (a mean
    of dyadic group AUCs such as 1999/4000 = 0.49975: summation order decides the last bit, hence the direction)"""
    if abs(got - exp) < 1e-9:
        return True
    frac = (raw[k] * 1e4) % 1.0
    return abs(got - exp) < 1.0000001e-4 and abs(frac - 0.5) < 1e-7


def _device(preds, labels, users, hp, group, chunks=3, raw=None):
    acc = DM.DeviceScores(torch.device(DEV))
    n = len(preds)
    cut = sorted(set([0, n] + [n * i // chunks for i in range(1, chunks)]))
    for a, b in zip(cut[:-1], cut[1:]):       # appended in pieces like an evaluation loop does
        acc.append(torch.tensor(preds[a:b], dtype=torch.float32, device=DEV),
                   torch.tensor(labels[a:b], dtype=torch.float32, device=DEV),
                   torch.tensor(users[a:b], dtype=torch.int32, device=DEV))
    return DM.compute(acc, hp, group, True, raw=raw)


def _host(preds, labels, users, hp, group):
    p32 = np.asarray(preds, dtype=np.float32)
    res = cal_metric(list(labels), list(p32), hp.metrics)
    res.update(cal_metric(np.reshape(np.asarray(labels), (-1, group)), np.reshape(p32, (-1, group)), hp.pairwise_metrics))
    res.update(cal_weighted_metric(users, p32, labels, hp.weighted_metrics))
    return res


def test_reference_captured_known_answers(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "metrics_golden.json")))
    labels = np.asarray(g["labels"], dtype=np.float64)
    preds = np.asarray(g["preds"], dtype=np.float64)
    group = labels.shape[1]
    users = np.asarray(g["users"]).astype(np.int64)
    res = _device(preds.reshape(-1), labels.reshape(-1), users, _hp(), group)
    # the three AUCs and the logloss are tie-exact: equal to what the REFERENCE computed (the fixture)
    for k in ("auc", "logloss", "group_auc", "wauc"):
        assert abs(res[k] - g["expected"][k]) < 1e-9, (k, res[k], g["expected"][k])
    # rank metrics: the fixture holds groups where the positive's score is tied with a negative's; numpy's default
    # argsort (SIMD quicksort on this generation of numpy) orders such ties platform-dependently -- neither "earlier
    # line first" nor "later line first" reproduces the captured 0.2559 -- so the reference itself is ill-defined
    # there.  On the groups WITHOUT such a tie the device equals the host functions that the CPU suite pins to the
    # fixture; the device's own rule for ties (later line first) is exercised in the next test.
    tied = np.array([any(p[j] == p[i] and j != i for i in np.flatnonzero(l == 1) for j in range(group))
                     for l, p in zip(labels, preds)])
    assert tied.any() and not tied.all()
    lab, prd = labels[~tied], preds[~tied]
    hp = _hp(metrics=[], weighted_metrics=[], pairwise_metrics=["mean_mrr", "ndcg@2;4;6", "hit@2;4;6"])
    got = _device(prd.reshape(-1), lab.reshape(-1), np.zeros(lab.size, dtype=np.int64), hp, group)
    exp = cal_metric(lab, prd.astype(np.float32), hp.pairwise_metrics)
    for k in exp:
        assert abs(got[k] - exp[k]) < 1e-9, (k, got[k], exp[k])


def test_rank_ties_break_towards_the_later_line():
    """Documented tie rule of the device metrics: equal scores rank like a stable ascending sort read backwards."""
    hp = _hp(metrics=[], weighted_metrics=[], pairwise_metrics=["mean_mrr", "hit@1;2"])
    preds = np.array([0.5, 0.5, 0.5, 0.1,      # positive first, tied with two later negatives: rank 3
                      0.2, 0.7, 0.7, 0.1])     # positive at index 2 of the group, tied with an EARLIER negative: rank 1
    labels = np.array([1.0, 0, 0, 0, 0, 0, 1.0, 0])
    got = _device(preds, labels, np.zeros(8, dtype=np.int64), hp, 4, chunks=1)
    assert abs(got["mean_mrr"] - round((1.0 / 3 + 1.0) / 2, 4)) < 1e-12
    assert got["hit@1"] == 0.5 and got["hit@2"] == 0.5


@pytest.mark.parametrize("n_groups,group,n_users,ties", [(2000, 5, 300, False), (700, 100, 64, False), (300, 100, 40, True),
                                                        (5000, 10, 5000, True), (1, 7, 1, False)])
def test_device_metrics_equal_the_host_metrics(n_groups, group, n_users, ties):
    """Random files: tie-free scores for the rank metrics; heavy ties (scores rounded to 2 decimals) for the three AUCs
    and logloss, which are tie-exact by construction (numpy's argsort orders ties platform-dependently even in small
    groups, see above: mean_mrr / ndcg / hit are compared on tie-free scores only)."""
    rng = np.random.default_rng(n_groups + group)
    N = n_groups * group
    labels = np.zeros((n_groups, group))
    labels[:, 0] = 1.0
    extra = rng.random((n_groups, group)) < 0.03          # a few groups with more than one positive
    extra[:, -1] = False                                   # (always at least one negative)
    labels = np.maximum(labels, extra)
    preds = ((rng.permutation(N) + 0.5) / N).astype(np.float32)     # distinct float32 scores (N < 2^24): tie-free
    assert np.unique(preds).size == N
    if ties:
        preds = np.round(preds, 2).astype(np.float32)
        preds[:7] = [0.0, 1.0, 1e-13, 1.0 - 1e-9, 0.5, 0.5, 0.25][: min(7, N)]  # clipping edges of the logloss
    users = np.repeat(rng.integers(0, n_users, n_groups), group)
    hp = _hp() if not ties else _hp(pairwise_metrics=["group_auc"])
    raw = {}
    got = _device(preds, labels.reshape(-1), users, hp, group, raw=raw)
    exp = _host(preds, labels.reshape(-1), users, hp, group)
    assert set(got) == set(exp)
    for k in exp:
        assert _same(got[k], exp[k], raw, k), (k, got[k], exp[k], raw[k])


def _pair_counts(pos, neg):
    """(#{p > n}, #{p == n}) over all pairs, as Python integers (float32 scores compared exactly)."""
    pos, neg = np.sort(np.asarray(pos, dtype=np.float32)), np.sort(np.asarray(neg, dtype=np.float32))
    below = np.searchsorted(neg, pos, side="left").astype(np.int64)        # negatives strictly below each positive
    upto = np.searchsorted(neg, pos, side="right").astype(np.int64)
    return int(below.sum()), int((upto - below).sum())


@pytest.fixture(scope="module")
def many_positives():
    """Lines of six users with exactly 255 / 256 / 257 / 512 / 513 / 700 positives (the user kernel takes a user's
    positives UA_PT = 256 at a time: one tile exactly, one short of it, one over, two tiles, ...) and 300-900 negatives each,
    shuffled among the lines of 300 small users; scores rounded to 2 decimals: heavy ties."""
    rng = np.random.default_rng(256)
    ids = rng.choice(1 << 18, 306, replace=False)
    users, labels = [], []
    for u, npos in zip(ids[:6], (255, 256, 257, 512, 513, 700)):
        nneg = int(rng.integers(300, 901))
        users += [u] * (npos + nneg)
        labels += [1.0] * npos + [0.0] * nneg
    for u in ids[6:]:
        npos, nneg = int(rng.integers(1, 5)), int(rng.integers(1, 9))
        users += [u] * (npos + nneg)
        labels += [1.0] * npos + [0.0] * nneg
    order = rng.permutation(len(users))
    users, labels = np.asarray(users, dtype=np.int64)[order], np.asarray(labels)[order]
    preds = np.round(rng.random(len(users)), 2).astype(np.float32)
    assert int(labels.sum()) > 2048       # (the global AUC kernel tiles the positives by AUC_PT = 2048)
    return preds, labels, users


def test_wauc_with_more_positives_per_user_than_one_tile(many_positives):
    """wauc against integer pair counting, unrounded.  The kernel counts pairs in integers as well; its only inexact step
    is the 2^-60 fixed-point rounding of ONE partial sum per wave (fx_add), at most 16 384 waves: below 2^-46 = 1.4e-14,
    and the float64 sums of ~300 terms <= 1 on either side add a few 1e-16 each -- hence 1e-12 absolute."""
    preds, labels, users = many_positives
    N = len(preds)
    exp, per_user_pos = 0.0, []
    for u in np.unique(users):
        m = users == u
        pos, neg = preds[m & (labels == 1)], preds[m & (labels != 1)]
        gt, eq = _pair_counts(pos, neg)
        exp += (int(m.sum()) / N) * (gt + 0.5 * eq) / (len(pos) * len(neg))
        per_user_pos.append(len(pos))
    assert sorted(per_user_pos)[-6:] == [255, 256, 257, 512, 513, 700]
    raw = {}
    hp = _hp(metrics=[], pairwise_metrics=[], weighted_metrics=["wauc"])
    got = _device(preds, labels, users, hp, 1, chunks=3, raw=raw)
    print("wauc: device %.17g, pair counting %.17g, diff %.3e" % (raw["wauc"], exp, raw["wauc"] - exp))
    assert abs(raw["wauc"] - exp) <= 1e-12
    assert got["wauc"] == round(raw["wauc"], 4)
    host = cal_weighted_metric(users, preds, labels, ["wauc"])
    assert _same(got["wauc"], host["wauc"], raw, "wauc")


def test_auc_with_more_positives_than_one_tile(many_positives):
    preds, labels, users = many_positives
    gt, eq = _pair_counts(preds[labels == 1], preds[labels != 1])
    exp = (gt + 0.5 * eq) / (float(int((labels == 1).sum())) * float(int((labels != 1).sum())))
    raw = {}
    _device(preds, labels, users, _hp(metrics=["auc"], pairwise_metrics=[], weighted_metrics=[]), 1, chunks=3, raw=raw)
    assert raw["auc"] == exp, (raw["auc"], exp)       # integer counts on both sides, the same float64 expression


WIDE_KS = [1, 2, 3, 5, 10, 64, 100, 5000]      # GM_MAXK = 8 distinct k, three of them above some (or every) G


def _wide_groups(G, n_groups):
    """Tie-free float32 scores; 1-5 positives per group, from the second on one sits 64 lines behind the first (the same
    lane of the wave that owns the group); every other group has its positives moved among the 8 best scores."""
    rng = np.random.default_rng(G)
    N = n_groups * G
    preds = ((rng.permutation(N) + 0.5) / N).astype(np.float32).reshape(n_groups, G)
    assert np.unique(preds).size == N
    labels = np.zeros((n_groups, G))
    for g in range(n_groups):
        npos = 1 + g % 5
        first = int(rng.integers(0, G - 64)) if G > 64 else int(rng.integers(0, G))
        at = [first] + ([first + 64] if npos > 1 and G > 64 else [])
        rest = [i for i in rng.permutation(G) if i not in at]
        at += [int(i) for i in rest[:npos - len(at)]]
        labels[g, at] = 1.0
        if g % 2 == 0:
            best = np.argsort(preds[g])[::-1][:8]
            for i, j in zip(at, rng.permutation(best)[:npos]):
                preds[g, [i, j]] = preds[g, [j, i]]
    return preds, labels


def _group_restatement(preds, labels, ks):
    """mean_mrr / ndcg@k / hit@k / group_auc in float64 from the ranks (tie-free scores), deeprec_utils.py:554-620."""
    out = {k: 0.0 for k in ["mean_mrr", "group_auc"] + ["ndcg@%d" % k for k in ks] + ["hit@%d" % k for k in ks]}
    for p, l in zip(preds, labels):
        pos = np.flatnonzero(l == 1)
        ranks = np.array([1 + int((p > p[i]).sum()) for i in pos], dtype=np.float64)
        out["mean_mrr"] += float((1.0 / ranks).sum()) / len(pos)
        gt, eq = _pair_counts(p[l == 1], p[l != 1])
        out["group_auc"] += (gt + 0.5 * eq) / (len(pos) * (len(p) - len(pos)))
        for k in ks:
            dcg = float((1.0 / np.log2(ranks[ranks <= k] + 1.0)).sum())
            ideal = float((1.0 / np.log2(np.arange(1, min(k, len(pos), len(p)) + 1) + 1.0)).sum())
            out["ndcg@%d" % k] += dcg / ideal
            out["hit@%d" % k] += 1.0 if (ranks <= k).any() else 0.0
    return {k: v / len(preds) for k, v in out.items()}


@pytest.mark.parametrize("G,n_groups", [(64, 40), (65, 40), (128, 40), (1000, 40), (2048, 40), (4096, 8)])
def test_group_metrics_on_wide_groups(G, n_groups):
    """Groups up to the kernel's bound (G = 4096: 128 KB of dynamic LDS per workgroup), k above G, the maximum of 8 distinct
    k, several positives on one lane.  Unrounded values: every wave adds ONE partial sum (here: one group) rounded to
    2^-30 fixed point, so a mean over the groups is within 2^-31 of the float64 restatement (+ float64 noise)."""
    preds, labels = _wide_groups(G, n_groups)
    hp = _hp(metrics=[], weighted_metrics=[],
             pairwise_metrics=["mean_mrr", "ndcg@1;2;5;64;100;5000", "hit@1;3;10", "group_auc"])
    assert DM.supported(hp, 1, G)
    raw = {}
    got = _device(preds.reshape(-1), labels.reshape(-1), np.zeros(preds.size, dtype=np.int64), hp, G, raw=raw)
    exp = cal_metric(labels, preds, hp.pairwise_metrics)
    assert set(got) == set(exp) and len(exp) == 2 + 6 + 3
    for k in exp:
        assert _same(got[k], exp[k], raw, k), (k, got[k], exp[k], raw[k])
    ref = _group_restatement(preds, labels, WIDE_KS)
    for k in exp:
        assert abs(raw[k] - ref[k]) <= 2.0 ** -31 + 1e-12, (k, raw[k], ref[k])
    assert 0.0 < raw["hit@1"] < raw["hit@10"] <= 1.0 and raw["ndcg@5000"] < 1.0      # (the case is not degenerate)


def test_groups_above_the_kernel_bound_keep_the_host_path(golden_dir, golden_hparams, tmp_path):
    """``supported`` looks at the group size: above MAX_GROUP lines per group the model evaluates on the host instead of
    raising out of the group kernel."""
    from clsr_amd.clsr import CLSRModel
    from clsr_amd.sequential_iterator import SASequentialIterator

    hp = _hp()
    assert DM.MAX_GROUP == 4096
    assert DM.supported(hp, 100, DM.MAX_GROUP) and not DM.supported(hp, 100, DM.MAX_GROUP + 1)
    assert DM.supported(_hp(pairwise_metrics=[]), 100, DM.MAX_GROUP + 1)      # (no group kernel without group metrics)
    # one group of 4097 lines: a positive line of the committed validation file, then 4096 negative ones of that file
    lines = open(os.path.join(golden_dir, "data", "valid_data")).read().splitlines()
    pos = [ln for ln in lines if ln.startswith("1\t")]
    neg = [ln for ln in lines if ln.startswith("0\t")]
    G = DM.MAX_GROUP + 1
    path = str(tmp_path / "wide_group")
    with open(path, "w") as f:
        user = pos[0].split("\t")[1]      # (all lines under one user: wauc needs both classes for every user)
        rows = [pos[0]] + ["\t".join([ln.split("\t")[0], user] + ln.split("\t")[2:]) for ln in (neg * (G // len(neg) + 1))[:G - 1]]
        f.write("\n".join(rows) + "\n")
    model = CLSRModel(golden_hparams, SASequentialIterator, seed=2)
    assert model._device_eval(path, G - 1, False) is None and model._device_eval(path, G - 1, True) is None
    got = model.run_eval(path, num_ngs=G - 1)
    users, preds, labels = [], [], []
    for batch in model.iterator.load_data_from_file(path, min_seq_length=model.min_seq_length, batch_num_ngs=0):
        if batch:
            u, p, l = model.eval_with_user(model.sess, batch)
            users.extend(np.reshape(u, -1)), preds.extend(np.reshape(p, -1)), labels.extend(np.reshape(l, -1))
    assert len(preds) == G
    exp = cal_metric(labels, preds, golden_hparams.metrics)
    exp.update(cal_metric(np.reshape(labels, (-1, G)), np.reshape(preds, (-1, G)), golden_hparams.pairwise_metrics))
    assert got == exp and "mean_mrr" in got
    exp.update(cal_weighted_metric(users, preds, labels, golden_hparams.weighted_metrics))
    assert model.run_weighted_eval(path, num_ngs=G - 1) == exp
    # groups the kernel takes go through the device metrics
    assert model._device_eval(os.path.join(golden_dir, "data", "valid_data"), 4, False) is not None


def test_undefined_auc_raises_like_the_host_path():
    hp = _hp(pairwise_metrics=[], weighted_metrics=[])
    with pytest.raises(ValueError):
        _device(np.array([0.2, 0.4, 0.6, 0.8]), np.zeros(4), np.zeros(4, dtype=np.int64), hp, 2)
    hp = _hp(metrics=[], pairwise_metrics=[], weighted_metrics=["wauc"])
    with pytest.raises(ValueError):    # user 1 has positives only
        _device(np.array([0.2, 0.4, 0.6, 0.8]), np.array([1.0, 0.0, 1.0, 1.0]), np.array([0, 0, 1, 1]), hp, 2)


def test_model_evaluation_on_the_device_equals_the_host_path(golden_dir, golden_hparams, monkeypatch):
    """run_eval / run_weighted_eval through the device metrics == the same calls with CLSR_HOST_METRICS=1."""
    from clsr_amd.clsr import CLSRModel
    from clsr_amd.sequential_iterator import SASequentialIterator

    import pickle

    from oracle import clsr_oracle as O

    hp = golden_hparams
    model = CLSRModel(hp, SASequentialIterator, seed=2)
    # weights with some spread: the freshly initialised model (sigma 0.01) scores every line 0.5 +- 1e-7, i.e. with
    # exact float32 ties inside groups, where the host's numpy argsort and the device's rule legitimately differ
    dims = dict(Vu=len(pickle.load(open(hp.user_vocab, "rb"))), Vi=len(pickle.load(open(hp.item_vocab, "rb"))),
                Vc=len(pickle.load(open(hp.cate_vocab, "rb"))))
    params = O.init_params(dims, hp, seed=5, scale_dense=8.0)
    sd = dict(params)
    sd.update(O.init_bn_state(params))
    model.net.load_state_dict(sd)
    valid = os.path.join(golden_dir, "data", "valid_data")
    dev_w, dev_e = model.run_weighted_eval(valid, num_ngs=4), model.run_eval(valid, num_ngs=4)
    monkeypatch.setenv("CLSR_HOST_METRICS", "1")
    host_w, host_e = model.run_weighted_eval(valid, num_ngs=4), model.run_eval(valid, num_ngs=4)
    assert dev_w == host_w and dev_e == host_e and "wauc" in dev_w and "wauc" not in dev_e
