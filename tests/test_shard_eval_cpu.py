"""CPU test of the chunk-to-rank plan of the sharded evaluation (clsr_amd/device_metrics.py: plan_chunks, chunk_owner):
every rank derives the plan on its own from the chunk sizes it sees while iterating the same file."""
import random

import pytest

from clsr_amd.device_metrics import chunk_owner, plan_chunks


def _sizes(seed, n):
    rng = random.Random(seed)
    return [rng.choice([1, 7, 12, 60, 64, 65, 72, 4000]) for _ in range(n)]


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n_chunks", [0, 1, 2, 5, 40])
def test_plan_covers_the_file_and_gives_every_chunk_one_owner(world, n_chunks):
    sizes = _sizes(world * 100 + n_chunks, n_chunks)
    plan = plan_chunks(sizes, world)
    assert len(plan) == len(sizes)
    at = 0
    for (off, n, owner), size in zip(plan, sizes):
        assert off == at and n == size              # contiguous, in file order
        assert isinstance(owner, int) and 0 <= owner < world      # exactly one owner, a rank of the world
        at += n
    assert at == sum(sizes)                          # the plan covers all N lines
    per_rank = [sum(n for _, n, o in plan if o == r) for r in range(world)]
    assert sum(per_rank) == sum(sizes)


def test_plan_depends_on_the_sizes_and_the_world_only():
    sizes = _sizes(3, 30)
    a = plan_chunks(list(sizes), 3)
    random.seed(99)                                  # (no hidden state: global RNG, earlier calls, the caller's lists)
    plan_chunks(_sizes(4, 10), 5)
    assert plan_chunks(tuple(sizes), 3) == a
    assert plan_chunks(sizes, 2) != a
    # the evaluation loop applies chunk_owner chunk by chunk: the same owners as the plan made in one go
    loads, owners = [0, 0, 0], []
    for n in sizes:
        owners.append(chunk_owner(loads))
        loads[owners[-1]] += n
    assert owners == [o for _, _, o in a]


def test_world_larger_than_the_chunk_count_leaves_ranks_without_work():
    plan = plan_chunks([64, 64, 8], 5)
    assert [o for _, _, o in plan] == [0, 1, 2]      # ranks 3 and 4 score nothing
    assert plan_chunks([10], 2) == [(0, 10, 0)]
    assert plan_chunks([], 4) == []


def test_plan_balances_lines_not_chunk_counts():
    # one long chunk, then short ones: the short ones go to the other ranks until they have caught up
    plan = plan_chunks([4000] + [64] * 20, 2)
    assert plan[0][2] == 0 and all(o == 1 for _, _, o in plan[1:])
    loads = [sum(n for _, n, o in plan_chunks([64] * 21, 3) if o == r) for r in range(3)]
    assert max(loads) - min(loads) <= 64
