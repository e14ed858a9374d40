"""The yardstick of omok_env_replay, pinned by hand without a GPU: tests/game_replay.py (the replay restated as a loop over the oracle's
Environment.place_stone) on cases whose answers follow from the rules of environment/src/lib.rs:104-166 alone."""
import numpy as np
import pytest

from oracle import oracle as O
import game_replay as R
import helpers
import positions as P


@pytest.mark.parametrize("n", [9, 15])
def test_draw_sequence_fills_the_board_and_an_extra_move_changes_nothing(n):
    seq = helpers.draw_sequence(n)
    board, status, played = R.replay(n, None, seq, len(seq))
    assert (status, played) == (O.DRAW, n * n) and np.count_nonzero(board) == n * n
    board2, status2, played2 = R.replay(n, None, seq + [0], len(seq) + 1)
    assert (status2, played2) == (O.DRAW, n * n) and np.array_equal(board, board2)


@pytest.mark.parametrize("n", [9, 15])
def test_win_stops_the_replay_and_upto_cuts_it(n):
    win = [0, n, 1, n + 1, 2, n + 2, 3, n + 3, 4, n + 4, 40]
    board, status, played = R.replay(n, None, win, len(win))
    assert (status, played) == (O.BLACK_WIN, 9)
    assert board[n + 4] == O.EMPTY and board[40] == O.EMPTY and np.count_nonzero(board) == 9
    board, status, played = R.replay(n, None, win, len(win), upto=8)
    assert (status, played) == (O.IN_PROGRESS, 8) and board[4] == O.EMPTY
    assert R.replay(n, None, win, len(win), upto=0)[1:] == (O.IN_PROGRESS, 0)
    assert R.replay(n, None, win, len(win), upto=100)[1:] == (O.BLACK_WIN, 9)


@pytest.mark.parametrize("n", [9, 15])
def test_overline_is_no_win(n):
    over = [0, n, 1, n + 1, 2, n + 2, 3, n + 3, 5, n + 5, 4]  # Black's last stone makes six in a row
    _, status, played = R.replay(n, None, over, len(over))
    assert (status, played) == (O.IN_PROGRESS, 11)


@pytest.mark.parametrize("n", [9, 15])
def test_illegal_moves_stop_the_replay_in_front_of_them(n):
    board, status, played = R.replay(n, None, [0, 0, 1], 3)  # an occupied cell
    assert (status, played) == (O.IN_PROGRESS, 1) and np.count_nonzero(board) == 1 and board[0] == O.BLACK
    for cell in (n * n, 0xFF):  # a cell off the board
        assert R.replay(n, None, [0, cell, 1], 3)[1:] == (O.IN_PROGRESS, 1)
    assert R.replay(n, None, [0x100 | 7], 1)[1:] == (O.IN_PROGRESS, 1)  # the external flag is no part of the cell
    assert R.replay(n, None, [0x100 | 7], 1)[0][7] == O.BLACK


def test_win_in_one_from_a_start_position():
    board, cell = P.win_in_one(9)
    empties = [int(c) for c in np.flatnonzero(board == O.EMPTY)]
    assert len(empties) == 3 and cell in empties
    for c in empties:
        out, status, played = R.replay(9, board, [c], 1)
        assert played == 1 and status == (O.BLACK_WIN if c == cell else O.IN_PROGRESS)
        assert out[c] == O.BLACK and np.count_nonzero(out) == 9 * 9 - 2


@pytest.mark.parametrize("n", [9, 15])
def test_rejected_start_boards_come_back_unchanged(n):
    seen = set()
    for name, (board, v) in sorted(P.hand_made(n).items()):
        out, status, played = R.replay(n, board, [n * n - 2], 1)
        if v != 0:
            seen.add(v)
            assert (status, played) == (-1, -v), name
            assert np.array_equal(out, board), name
        else:
            assert status >= 0 and played >= 0, name
    assert seen == {P.BAD_BYTE, P.BAD_COUNTS, P.WON, P.FULL}


@pytest.mark.parametrize("n", [9, 15])
def test_random_games_stay_in_progress(n):
    rng = np.random.default_rng([7, n])
    for length in (0, 1, 63, 64, 65, n * n - 1):
        seq = R.random_game(n, length, rng)
        assert len(set(seq)) == length
        assert R.replay(n, None, seq, length)[1:] == (O.IN_PROGRESS, length)
