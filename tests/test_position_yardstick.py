"""The yardstick of the episodes that start from given positions (omok_selfplay_reset_from), on the oracle alone (no GPU):

1. an oracle SelfPlay driven from its ordinary reset to a position by external moves (set_actions -> mirror_generate -> advance, one call
   per stone), the last advance fed the raw policy rows of the final position, is left with one-node trees: root n = 0, w = 0, ply = the
   stone count, no transition recorded, and a root policy = that row masked over the position's stones and renormalised
   (ensure_action_exists, agent.rs:166-171; oracle/selfplay.c:325-348, :277-322);
2. the position verdicts of omok_env_check_positions restated through the oracle's place_stone (tests/positions.py), pinned on hand-made
   positions."""
import numpy as np
import pytest

from oracle import oracle as O
import positions as P
from test_oracle_literal import FakeNet


@pytest.mark.parametrize("stones", [1, 2, 7, 8])
@pytest.mark.parametrize("n,games", [(9, 5), (15, 3)])
def test_external_moves_leave_the_fresh_agent_of_the_position(n, games, stones):
    hw = n * n
    net = FakeNet(n, seed=1)
    boards = P.quiet(n, games, stones, seed=7)
    v, s = P.verdicts(n, boards)
    assert np.all(v == P.LEGAL) and np.all(s == stones)
    rows = net.forward(P.input_rows(n, boards))[0]
    assert rows.dtype == np.float32 and rows.shape == (games, hw)
    root_p = net.forward(O.Environment(n).encode_nn_input(0)[None])[0][0]
    osp = O.SelfPlay(n, games, cap_nodes=64, cap_tables=32, seed=3)
    P.drive_to(osp, boards, rows, root_p)
    assert osp.ply == stones and osp.alive_count == games
    for g in range(games):
        want = P.masked_renormalised(boards[g], rows[g])
        assert np.all(want[boards[g] != 0] == 0.0) and abs(float(want.sum()) - 1.0) < 1e-5
        last = P.move_order(boards[g])[-1]
        assert osp.game_plies(g) == stones and osp.game_status(g) == O.IN_PROGRESS
        assert len(osp.replay(g)[0]) == 0  # external moves record nothing
        for side in (0, 1):
            ints, floats = osp.tree_dump(g, side)
            assert ints.shape == (1, 8)
            parent, action, status, turn, legal, nch, visits, packed = (int(x) for x in ints[0])
            # the one field a fresh agent does not share: the root remembers the last move
            assert (parent, action, status, turn, legal, nch, visits) == (-1, last, O.IN_PROGRESS, stones & 1, hw - stones, 0, 0)
            assert packed >> 16 == 1  # has_policy
            assert osp.tree_root(g, side) == (0, 0.0, 1, 0)
            assert floats[0, 0] == 0.0
            assert np.array_equal(floats[0, 1:].view(np.uint32), want.view(np.uint32)), f"game {g} side {side}: root policy bits"


@pytest.mark.parametrize("n", [9, 15])
def test_verdicts_of_hand_made_positions(n):
    hand = P.hand_made(n)
    for name, (board, want) in sorted(hand.items()):
        got, stones = P.verdict(n, board)
        assert got == want, f"{name}: verdict {got}, pinned {want}"
        assert stones == int(np.count_nonzero((board == O.BLACK) | (board == O.WHITE))), name
    names = set(hand)
    for direction in P.DIRECTIONS:
        assert {f"five_{direction}_black", f"five_{direction}_white"} <= names
    assert {"six_run", "full_board", "white_ahead", "black_two_ahead", "bad_byte"} <= names


@pytest.mark.parametrize("n", [9, 15])
def test_edge_and_word_boundary_positions_are_what_they_claim(n):
    """the inputs of the GPU test: fives on the edges, in the corners and across the bitboard word boundaries are won, sixes are not"""
    for name, board in sorted({**P.edge_positions(n), **P.straddling_fives(n)}.items()):
        got, _ = P.verdict(n, board)
        won = "five" in name or name.startswith(("row_", "column_", "diagonal_", "antidiagonal_", "corner_"))
        assert got == (P.WON if won else P.LEGAL), f"{name}: verdict {got}"
    want = {64} | ({128, 192} if n == 15 else set())
    assert {int(k.split("_")[1]) for k in P.straddling_fives(n) if k.startswith("column_")} == want
