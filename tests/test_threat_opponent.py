"""No-GPU pins of tests/threat_opponent.py, the plain-Python restatement of the threat-aware scripted player (OMOK_OPP_THREAT,
include/omok_mi355x.h) that the GPU tests compare the device kernels with: hand-made positions whose answer follows from the rule
read by hand, at 9 x 9 and 15 x 15 and for both sides to move."""
import os
import re

import numpy as np
import pytest

import scripted_opponent as SO
import threat_opponent as TO
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scan(n, board, side):
    return TO.scan(SO.make_env(n, board, side))[:3]


@pytest.mark.parametrize("n", [9, 15])
def test_hand_made_positions(n):
    pos = TO.hand_made(n)
    rows = (4, 8) if n == 9 else (4, 8, 12)
    assert len(pos) == 2 * (4 * len(rows) + 11)
    for name, (board, side, want) in sorted(pos.items()):
        assert _scan(n, board, side) == want, name


@pytest.mark.parametrize("n", [9, 15])
def test_a_win_beats_a_block_at_a_lower_index(n):
    board, naive_cell = SO.hand_made(n)["block_before_win"]
    at = lambda x, y: y * n + x  # noqa: E731
    assert naive_cell == at(5, 1)
    for side, cell in ((0, at(5, 5)), (1, at(5, 1))):
        env = SO.make_env(n, board, side)
        assert SO.forced_cell(env) == at(5, 1)  # the naive rule: the lower index whoever moves
        assert TO.scan(env)[:3] == (cell, 1, 0)  # the threat rule: the mover's own five
        assert TO.move(env, 0, 0, 0) == (cell, 1)


@pytest.mark.parametrize("n", [9, 15])
@pytest.mark.parametrize("side", [0, 1])
def test_winning_cells_of_threes_and_fours(n, side):
    c, other = TO.stone_of(side), TO.stone_of(1 - side)
    at = lambda x, y: y * n + x  # noqa: E731

    def T(mine, theirs, a):
        board = SO._board(n, mine, theirs) if side == 0 else SO._board(n, theirs, mine)
        assert board[a] == O.EMPTY
        return TO.winning_cells(list(board), n, c, a), TO.winning_cells(list(board), n, other, a)

    three = [at(2, 4), at(3, 4), at(4, 4)]
    assert T(three, [], at(1, 4)) == (2, 0) and T(three, [], at(5, 4)) == (2, 0)  # _XXX_ -> an open four
    assert T(three, [], at(0, 4)) == (1, 0) and T(three, [], at(6, 4)) == (1, 0)  # X_XXX: the gap only
    assert T(three + [at(6, 4)], [], at(1, 4)) == (1, 0)  # XXXX_X: (5, 4) would make six, only (0, 4) wins
    assert T(three + [at(7, 4)], [], at(5, 4)) == (1, 0)  # XXXX_X the other way: (6, 4) would make six, only (1, 4) wins
    assert T(three, [at(1, 4)], at(5, 4)) == (1, 0)  # a four against an enemy stone
    edge = [at(0, 4), at(1, 4), at(2, 4)]
    assert T(edge, [], at(3, 4)) == (1, 0)  # a four against the edge
    assert T([at(2, 4), at(3, 4), at(5, 4)], [], at(4, 4)) == (2, 0)  # XX_X: the gap makes an open four
    diag = [at(2, 2), at(3, 3), at(4, 4)]
    assert T(diag, [], at(5, 5)) == (2, 0) and T(diag, [], at(1, 1)) == (2, 0) and T(diag, [], at(0, 0)) == (1, 0)
    anti = [at(6, 2), at(5, 3), at(4, 4)]
    assert T(anti, [], at(3, 5)) == (2, 0) and T(anti, [], at(7, 1)) == (2, 0)
    # a double four: a row three and a column three closed at one end each, crossing at the cell
    cross = [at(1, 4), at(2, 4), at(3, 4), at(4, 1), at(4, 2), at(4, 3)]
    assert T(cross, [at(0, 4), at(4, 0)], at(4, 4)) == (2, 0)


@pytest.mark.parametrize("n", [9, 15])
def test_open_three_and_near(n):
    at = lambda x, y: y * n + x  # noqa: E731
    board = list(SO._board(n, [at(2, 4), at(3, 4)], [at(0, 0), at(1, 0)]))
    assert TO.open_three(board, n, O.BLACK, at(1, 4)) and TO.open_three(board, n, O.BLACK, at(4, 4))
    assert not TO.open_three(board, n, O.BLACK, at(5, 4))  # X X _ a: no run of three
    assert not TO.open_three(board, n, O.WHITE, at(2, 0))  # an end (-1, 0) off the board
    board[at(0, 4)] = O.WHITE
    assert not TO.open_three(board, n, O.BLACK, at(1, 4)) and TO.open_three(board, n, O.BLACK, at(4, 4))  # (0, 4) is taken
    assert TO.near(board, n, at(1, 1)) and TO.near(board, n, at(4, 5)) and not TO.near(board, n, at(5, 4)) and not TO.near(board, n, at(8, 8))


@pytest.mark.parametrize("n", [9, 15])
def test_the_random_set_meets_its_condition_and_runs_agree_with_the_oracle(n):
    boards, turns, want = TO.random_set(n)
    by_side = TO.levels_by_side(turns, want)
    print(f"board {n}: {len(boards)} positions, levels {[int(np.count_nonzero(want[:, 1] == lv)) for lv in range(8)]}")
    assert by_side[0] >= set(range(1, 7)) and by_side[1] >= set(range(1, 7)) and 7 in (by_side[0] | by_side[1])
    checked = 0
    for board, turn in zip(boards, turns):  # the Python L == 5 against the oracle's place_stone verdict, both colours, every empty cell
        env = SO.make_env(n, board, turn)
        cells = [a for a in range(n * n) if board[a] == O.EMPTY]
        if len(cells) < 2 or turn == 1:  # (the board of turn 1 is the board of turn 0; one empty cell: Draw is not FIVE)
            continue
        bl = list(board)
        for a in cells:
            for side in (0, 1):
                assert TO.five_by_runs(bl, n, TO.stone_of(side), a) == TO.five(env, side, a)
                checked += 1
    assert checked > 1000


def test_the_draw_of_levels_6_and_7():
    n, seed, ply, game_global = 9, 17, 6, 1000
    key = O.stream_key(seed, 3)
    board = TO.hand_made(n)["lone_s0"][0]
    for side in (0, 1):
        env = SO.make_env(n, board, side)
        cell, level, count, cells = TO.scan(env)
        assert (cell, level, count) == (-1, 6, 8) and cells == [30, 31, 32, 39, 41, 48, 49, 50]
        import ctypes as C
        out = (C.c_uint32 * 4)()
        O.lib().orc_philox(key, 0, ply, 2 * game_global + side, SO.RNG_OPPONENT, out)
        assert TO.move(env, key, ply, game_global) == (cells[(int(out[0]) * 8) >> 32], 6)
    empty = SO.make_env(n, np.zeros(n * n, dtype=np.uint8), 0)
    assert TO.move(empty, key, 0, 5) == (SO.move(SO.OPP_RANDOM, empty, key, 0, 5)[0], 7)  # level 7 IS the random player's draw


def test_constants_agree():
    from omok_ai_amd import binding
    assert TO.OPP_THREAT == binding.OPP_THREAT == 3 and binding.OPPONENTS == {"random": 0, "naive": 1, "threat": 3}
    header = open(os.path.join(ROOT, "include", "omok_mi355x.h")).read()
    assert re.search(r"^#define OMOK_OPP_THREAT 3$", header, flags=re.M) and not re.search(r"^#define OMOK_OPP_\w+ 2$", header, flags=re.M)
    rust = open(os.path.join(ROOT, "bindings", "omok_mi355x.rs")).read()
    assert re.search(r"pub const OMOK_OPP_THREAT: i32 = 3;", rust) and "pub fn omok_env_threat_scan(" in rust
    assert "omok_env_threat_scan" in binding.SYMBOLS and re.search(r"\bint omok_env_threat_scan\(", header)


def test_records_tactics_with_a_stand_in_engine():
    """GameRecords.tactics is host code over two engine calls: with the replay and the scan supplied by the yardsticks (game_replay,
    threat_opponent.scan) it must give the game-by-game walk of threat_opponent.tactics -- on games of players that do overlook wins."""
    import game_replay as GR
    from omok_ai_amd import records as R

    class StandIn:
        n = 9

        def env_replay(self, start, moves, lengths, upto=-1):
            return GR.replay_batch(self.n, start, moves, lengths, upto)

        def env_threat_scan(self, boards, turns):
            w = np.array([TO.scan(SO.make_env(self.n, b, t))[:3] for b, t in zip(boards, turns)], dtype=np.int32).reshape(-1, 3)
            return w[:, 0], w[:, 1], w[:, 2]

    n, hw, key = 9, 81, O.stream_key(5, 0)
    kinds = [(SO.OPP_RANDOM, SO.OPP_RANDOM), (SO.OPP_RANDOM, SO.OPP_NAIVE), (SO.OPP_NAIVE, SO.OPP_RANDOM), (TO.OPP_THREAT, SO.OPP_RANDOM),
             (SO.OPP_RANDOM, TO.OPP_THREAT), (SO.OPP_NAIVE, SO.OPP_NAIVE)]
    games = [TO.play(n, k, key, g) for g, k in enumerate(kinds)]
    moves = np.full((len(games), hw), 0xFFFF, dtype=np.uint16)
    lengths, status = np.zeros(len(games), dtype=np.int32), np.zeros(len(games), dtype=np.uint8)
    for g, (_pos, mv, st) in enumerate(games):
        moves[g, :len(mv)], lengths[g], status[g] = mv, len(mv), st
    zero = np.zeros((len(games), hw))
    rec = R.GameRecords.from_log(n, np.zeros((len(games), hw), dtype=np.uint8), lengths, moves, zero, zero, zero, zero, status, lengths)
    t = rec.tactics(StandIn())
    for g in range(len(games)):
        levels, missed, unblocked = TO.tactics(n, rec.start_boards[g], [int(c) for c in rec.cells[g, :lengths[g]]])
        assert [int(x) for x in t["level_before"][g, :lengths[g]]] == levels and not t["level_before"][g, lengths[g]:].any()
        assert [int(x) for x in t["missed_win"][g]] == missed and [int(x) for x in t["unblocked"][g]] == unblocked
    assert t["missed_win"].sum() > 0 and t["unblocked"].sum() > 0  # the random player does overlook both
    assert t["missed_win"][3, 0] == 0 and t["missed_win"][4, 1] == 0  # the threat player never passes a win
