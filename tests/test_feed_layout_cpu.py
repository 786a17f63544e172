"""``clsr_amd.feeds.layout`` and the three feed specs: every piece of a device arena in the order given, on a 16-byte
boundary, ``4 * prod(shape)`` bytes long."""
import numpy as np
import pytest


def _specs(n, G, T):
    from clsr_amd import feeds

    return {"training, compact": feeds.train_spec(n, n * G, T),
            "training, expanded": feeds.train_spec(n * G, n * G, T),
            "training, expanded, a target per position": feeds.train_spec(n * G, n * G, T, True),
            "evaluation, groups (users_rows)": feeds.eval_spec(n, n * G, T, True),
            "evaluation, rows": feeds.eval_spec(n * G, n * G, T, False)}


@pytest.mark.parametrize("n,G,T", [(3, 2, 3), (3, 2, 50), (64, 5, 50), (1, 1, 1)])
def test_pieces_are_ordered_aligned_and_sized(n, G, T):
    from clsr_amd import feeds

    for what, spec in _specs(n, G, T).items():
        lay, total = feeds.layout(spec)
        assert list(lay) == [name for name, _, _ in spec], what
        end = 0
        for name, shape, _ in spec:
            off, nb = lay[name]
            assert off == end and off % 16 == 0, (what, name)
            assert nb == 4 * int(np.prod(shape)), (what, name)
            end = off + (nb + 15) // 16 * 16
        assert total == end, what


def test_spec_names_and_shapes():
    from clsr_amd import feeds, ops

    s = _specs(3, 2, 5)
    for what in ("training, compact", "training, expanded", "training, expanded, a target per position"):
        assert tuple(name for name, _, _ in s[what]) == ops.FEED_OUTPUTS, what
    assert tuple(name for name, _, _ in s["evaluation, groups (users_rows)"]) == ops.FEED_EVAL_OUTPUTS
    assert tuple(name for name, _, _ in s["evaluation, rows"]) == ops.FEED_OUTPUTS
    shapes = lambda what: {name: (tuple(shape), dt) for name, shape, dt in s[what]}
    I, F = feeds.I32, feeds.F32
    assert shapes("training, compact") == {
        "users": ((3,), I), "items": ((6,), I), "cates": ((6,), I), "item_history": ((3, 5), I),
        "item_cate_history": ((3, 5), I), "time_from_first_action": ((3, 5), F), "time_to_now": ((3, 5), F),
        "labels": ((6,), F), "seq_len": ((3,), I), "denom": ((1,), F)}
    pos = shapes("training, expanded, a target per position")
    assert pos["items"] == ((6, 5), I) and pos["cates"] == ((6, 5), I) and pos["labels"] == ((30,), F)
    assert pos["users"] == ((6,), I) and pos["item_history"] == ((6, 5), I) and pos["seq_len"] == ((6,), I)
    ev = shapes("evaluation, groups (users_rows)")
    assert ev["users"] == ((3,), I) and ev["users_rows"] == ((6,), I) and ev["labels"] == ((6,), F)
    assert ev["time_to_now"] == ((3, 5), F) and ev["items"] == ((6,), I)


def test_a_layout_worked_by_hand():
    """n = 3 lines, G = 2, T = 3, compact: users 12 bytes -> 16; items, cates, labels 24 -> 32; the four [3, 3] arrays 36
    -> 48; seq_len 12 -> 16; denom 4 -> 16."""
    from clsr_amd import feeds

    lay, total = feeds.layout(feeds.train_spec(3, 6, 3))
    assert lay == {"users": (0, 12), "items": (16, 24), "cates": (48, 24), "item_history": (80, 36),
                   "item_cate_history": (128, 36), "time_from_first_action": (176, 36), "time_to_now": (224, 36),
                   "labels": (272, 24), "seq_len": (304, 12), "denom": (320, 4)}
    assert total == 336
    lay, total = feeds.layout((("a", (5,), None), ("b", (4,), None), ("c", (1, 1), None), ("d", (2, 3, 7), None)))
    assert lay == {"a": (0, 20), "b": (32, 16), "c": (48, 4), "d": (64, 168)} and total == 240


def test_host_arrays_have_the_layout_of_their_spec():
    """``upload`` lays its host arrays out by the same function: the byte counts are those of the arrays."""
    from clsr_amd import feeds

    h = {"users": np.zeros(3, np.int32), "item_history": np.zeros((3, 7), np.int32), "labels": np.zeros(6, np.float32)}
    lay, total = feeds.layout([(k, a.shape, a.dtype) for k, a in h.items()])
    assert lay == {"users": (0, 12), "item_history": (16, 84), "labels": (112, 24)} and total == 144
    assert all(lay[k][1] == a.nbytes for k, a in h.items())
