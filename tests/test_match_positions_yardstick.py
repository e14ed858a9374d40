"""The yardsticks of the matches from given positions (omok_match_reset_from) and of the random openings (omok_env_random_positions),
pinned on the oracle alone (no GPU):

1. a MatchComposition (tests/match_harness.py) whose two instances are driven from their ordinary reset to the positions by external moves
   (positions.drive_to), instance x fed rows R_x at the last advance, holds one-node trees; the root policy of tree side * G + g is
   R_owner[g] masked over position g's stones and renormalised, owner = side ^ (g >= split), whichever side is to move;
2. the random openings restated through scripted_opponent.move(RANDOM) + place_stone (tests/random_openings.py): ok = 1 exactly where the
   board is a legal position of `stones` stones, a range of games may be cut anywhere, and both ok classes occur in the test's inputs;
3. match.paired_tally on a hand-written status vector.
"""
import numpy as np
import pytest

from omok_ai_amd import api
from omok_ai_amd import match as M
from oracle import oracle as O
from match_harness import MatchComposition
import positions as P
import random_openings as RO
from test_oracle_literal import FakeNet


@pytest.mark.parametrize("stones", [3, 4])
def test_driven_composition_holds_the_fresh_agents_of_the_match(stones):
    n, games, split = 9, 6, 2
    hw = n * n
    nets = [FakeNet(n, seed=1), FakeNet(n, seed=2)]
    boards = P.quiet(n, games, stones, seed=7)
    v, s = P.verdicts(n, boards)
    assert np.all(v == P.LEGAL) and np.all(s == stones)
    x = P.input_rows(n, boards)
    rows = [net.forward(x)[0] for net in nets]
    assert not np.array_equal(rows[0], rows[1])
    empty = O.Environment(n).encode_nn_input(0)[None]
    roots = [net.forward(empty)[0][0] for net in nets]
    comp = MatchComposition(n, games, split, roots[0], roots[1], seed=3, cap_nodes=64, cap_tables=32)
    for i in range(2):
        comp.O[i].set_episode(0)
        P.drive_to(comp.O[i], boards, rows[i], roots[i])
    assert comp.ply == stones and comp.alive_count == games and comp.error == 0
    for g in range(games):
        last = P.move_order(boards[g])[-1]
        assert comp.game_status(g) == O.IN_PROGRESS and comp.O[0].game_plies(g) == stones == comp.O[1].game_plies(g)
        assert len(comp.O[0].replay(g)[0]) == 0 and len(comp.O[1].replay(g)[0]) == 0
        for side in (0, 1):
            owner = side ^ (1 if g >= split else 0)
            assert comp.owner(g, side) == owner
            want = P.masked_renormalised(boards[g], rows[owner][g])
            ints, floats = comp.tree_dump(g, side)
            assert ints.shape == (1, 8)
            parent, action, status, turn, legal, nch, visits, packed = (int(x) for x in ints[0])
            assert (parent, action, status, turn, legal, nch, visits) == (-1, last, O.IN_PROGRESS, stones & 1, hw - stones, 0, 0)
            assert packed >> 16 == 1  # has_policy
            assert comp.tree_root(g, side) == (0, 0.0, 1, 0)
            assert floats[0, 0] == 0.0
            assert np.array_equal(floats[0, 1:].view(np.uint32), want.view(np.uint32)), f"game {g} side {side}: root policy bits"
            other = P.masked_renormalised(boards[g], rows[1 - owner][g])
            assert not np.array_equal(floats[0, 1:].view(np.uint32), other.view(np.uint32))


@pytest.mark.parametrize("n,stones", [(9, 50), (15, 100)])
def test_random_openings_yardstick(n, stones):
    key, batch = O.stream_key(5, 0), 256
    boards, ok = RO.positions(n, key, 0, stones, batch)
    share = float(np.mean(ok == 0))
    print(f"board {n}, {stones} stones: {int(np.sum(ok == 0))} of {batch} games ended on the way ({100 * share:.1f} %)")
    assert 0.15 <= share <= 0.85  # (a condition on the inputs: the stop rule is exercised and so is the full count)
    for b in range(batch):
        verdict, count = P.verdict(n, boards[b])
        assert (ok[b] == 1) == ((verdict, count) == (P.LEGAL, stones)), f"position {b}: ok {ok[b]}, verdict {verdict}, {count} stones"
        if ok[b] == 0:  # the game ended at the last stone placed: an already won position of fewer than, or exactly, `stones` stones
            assert verdict == P.WON and count <= stones
    cut = 101
    lo, ok_lo = RO.positions(n, key, 0, stones, cut)
    hi, ok_hi = RO.positions(n, key, cut, stones, batch - cut)
    assert np.array_equal(np.concatenate([lo, hi]), boards) and np.array_equal(np.concatenate([ok_lo, ok_hi]), ok)
    other, _ = RO.positions(n, O.stream_key(5, 1), 0, stones, 8)
    assert not np.array_equal(other, boards[:8])


def test_random_openings_prefixes_and_empty():
    n, key = 9, O.stream_key(5, 0)
    boards0, ok0 = RO.positions(n, key, 0, 0, 4)
    assert not boards0.any() and np.all(ok0 == 1)
    few, ok_few = RO.positions(n, key, 0, 8, 16)
    more, _ = RO.positions(n, key, 0, 9, 16)
    assert np.all(ok_few == 1) and np.all(np.count_nonzero(few, axis=1) == 8)
    assert np.all((few == more) | (few == 0)) and np.all(np.count_nonzero(few != more, axis=1) == 1)  # one more stone, the rest in place


def test_paired_tally():
    D, B_, W = api.DRAW, api.BLACK_WIN, api.WHITE_WIN
    #             opening: 0   1   2   3   4   5   6
    as_black = np.array([B_, B_, W, W, D, B_, D])  # games [0, M): the first net is Black
    as_white = np.array([W, B_, W, B_, W, D, D])   # games [M, 2 M): the first net is White
    status = np.concatenate([as_black, as_white])
    # 0: won both; 1: won as Black only; 2: won as White only; 3: lost both; 4, 5, 6: a draw in the pair
    assert M.paired_tally(status, 7) == (1, 2, 1, 3)
    assert sum(M.paired_tally(status, 7)) == 7
    w, l, d = M.tally(status, 7)
    assert (w, l, d) == (6, 4, 4)
    assert M.paired_tally(np.array([B_, W]), 1) == (1, 0, 0, 0) and M.paired_tally(np.array([W, B_]), 1) == (0, 0, 1, 0)
