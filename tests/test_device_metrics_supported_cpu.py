"""Which metric requests ``device_metrics.supported`` sends to the device (a host-side decision: no GPU needed)."""
import types

from clsr_amd import device_metrics as DM


def _hp(**kw):
    d = dict(metrics=["auc", "logloss"], pairwise_metrics=["mean_mrr", "ndcg@2;4;6", "hit@2;4;6", "group_auc"],
             weighted_metrics=["wauc"])
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_every_reference_metric_has_a_device_form():
    assert DM.supported(_hp(metrics=["auc", "logloss", "rmse", "acc", "f1"]), 100, 5)
    assert DM.supported(_hp(weighted_metrics=["wauc", "wmrr", "whit@1;2;5", "wndcg@1;2;5;100"]), 100, 5)
    assert DM.supported(_hp(weighted_metrics=None), 100, 5) and DM.supported(_hp(metrics=None), 100, 5)
    assert not DM.supported(_hp(metrics=["auc", "mae"]), 100, 5)
    assert not DM.supported(_hp(weighted_metrics=["wauc", "wrecall@5"]), 100, 5)


def test_any_number_of_users_is_supported():
    for n_users in (1, 1 << 18, (1 << 18) + 1, 10 ** 6, 2 ** 31 - 1):
        assert DM.supported(_hp(), n_users, 5)


def test_bounds_that_keep_the_host_path():
    assert DM.supported(_hp(weighted_metrics=["whit@1;2;3;4", "wndcg@3;4;5;6;7;8"]), 100, 5)            # 8 distinct k
    assert not DM.supported(_hp(weighted_metrics=["whit@1;2;3;4", "wndcg@3;4;5;6;7;8;9"]), 100, 5)      # 9
    assert not DM.supported(_hp(pairwise_metrics=["ndcg@1;2;3;4;5", "hit@6;7;8;9"]), 100, 5)
    assert DM.supported(_hp(), 100, DM.MAX_GROUP) and not DM.supported(_hp(), 100, DM.MAX_GROUP + 1)
