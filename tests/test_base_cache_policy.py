"""The restatement of k_group's base-slot rule (tools/base_cache_sim.py: slot_policy) on hand-made request lists: what the GPU test compares the
engine's counter with must itself say what DESIGN 3.3 says.  No GPU."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import base_cache_sim as S  # noqa: E402


def test_runs_qualify_at_three_rows():
    assert S.qualifying_runs([5, 5, 5, 9, 9, 7, 7, 7, 7]) == [(5, 0, 3), (7, 5, 4)]
    assert S.qualifying_runs([5, 5, 9, 5, 5]) == [] and S.qualifying_runs([]) == []


def test_empty_slots_are_taken_lowest_first_and_the_second_leaf_leads():
    tags, out = S.slot_policy([], [10, 11])
    assert out == ["miss", "miss"] and tags == [(11, 1), (10, 0)]
    tags, out = S.slot_policy(tags, [11])  # the next round: the second run's leaf is the tree's first run
    assert out == ["hit"] and tags == [(11, 1), (10, 0)]


def test_a_hit_keeps_its_way_and_the_other_run_takes_the_other_one():
    tags, out = S.slot_policy([(10, 1), (3, 0)], [4, 10])  # the second run hits way 1: the first run must not evict it although 3's way 0 is the only choice anyway
    assert out == ["miss", "hit"] and tags == [(10, 1), (4, 0)]
    tags, out = S.slot_policy([(3, 0), (10, 1)], [4, 10])  # ... and here the least recently used way is the one the second run hits: the first run takes way 0
    assert out == ["miss", "hit"] and tags == [(10, 1), (4, 0)]
    tags, out = S.slot_policy([(3, 0), (10, 1)], [3, 10])
    assert out == ["hit", "hit"] and tags == [(10, 1), (3, 0)]


def test_two_misses_never_share_a_way():
    tags, out = S.slot_policy([(3, 1), (8, 0)], [20, 21])
    assert out == ["miss", "miss"] and tags == [(21, 1), (20, 0)]  # the first run takes the least recently used way, the second the remaining one
    tags, out = S.slot_policy([(1, 2), (2, 0), (3, 3), (4, 1)], [20, 21], ways=4)
    assert out == ["miss", "miss"] and tags == [(21, 3), (20, 1), (1, 2), (2, 0)]


def test_third_runs_and_the_old_rule():
    tags, out = S.slot_policy([], [10, 11, 12, 13])
    assert out == ["miss", "miss", "uncacheable", "uncacheable"] and tags == [(11, 1), (10, 0)]
    tags, out = S.slot_policy([], [10, 11, 12], two_runs=False)
    assert out == ["miss", "uncacheable", "uncacheable"] and tags == [(10, 0)]
    tags, out = S.slot_policy([(7, 0)], [10, 11, 10])  # two runs of one leaf with another between them: the third is a third run
    assert out == ["miss", "miss", "uncacheable"]


def test_two_runs_of_one_leaf_share_its_base():
    tags, out = S.slot_policy([(7, 0)], [10, 10])  # (a run shorter than three rows lay between them)
    assert out == ["miss", "shared"] and tags == [(10, 1), (7, 0)]


def test_the_model_counts_what_the_tool_prints():
    m = S.BaseCacheModel()
    assert m.round({0: [1] * 11 + [2] * 5, 1: [1] * 16}) == 3
    assert m.round({0: [2] * 16, 1: [1] * 14 + [5, 5]}) == 0
    assert (m.tree_rounds, m.runs, m.full, m.second_runs, m.second_followed, m.second_reused) == (4, 5, 3, 1, 1, 1)
    old = S.BaseCacheModel(two_runs=False)
    old.round({0: [1] * 11 + [2] * 5})
    assert old.round({0: [2] * 16}) == 1 and (old.second_followed, old.second_reused) == (1, 0)
