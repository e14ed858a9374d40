"""The threat-aware scripted player (OMOK_OPP_THREAT, include/omok_mi355x.h), restated in plain Python (a helper of
tests/test_threat_opponent.py and tests/test_gpu_threat.py; not a test, no product code).

The rule is defined by the exact-five test alone.  FIVE goes through the oracle's orc_env_place_stone, as
scripted_opponent.forced_cell does; the runs, T, OPEN3 and NEAR are restated directly on the Stone bytes; the draw of levels 6
and 7 goes through orc_philox, as scripted_opponent.fallback_cell does.

  scan(env)  -> (cell, level, count) as omok_env_threat_scan returns them, plus the cells the draw chooses among
  move(env, key, ply, game_global) -> (cell, level): the move omok_opponent_actions(OMOK_OPP_THREAT) stages
"""
import ctypes as C

import numpy as np

from oracle import oracle as O
import scripted_opponent as SO

OPP_THREAT = 3
PAIRS = ((1, 0), (0, 1), (1, 1), (1, -1))  # one ray of each line pair (horizontal, vertical, the two diagonals); the other is its negative


def stone_of(side):
    return O.BLACK if side == 0 else O.WHITE


def run(board, n, c, x, y, dx, dy, extra=-1):
    """consecutive c stones from the cell next to (x, y) outwards along (dx, dy); the cell `extra` counts as a c stone"""
    k = 0
    while True:
        x += dx
        y += dy
        if not (0 <= x < n and 0 <= y < n):
            return k
        a = y * n + x
        if board[a] != c and a != extra:
            return k
        k += 1


def line_length(board, n, c, a, pr, extra=-1):
    """L(c, a, pr) = 1 + ra + rb"""
    dx, dy = PAIRS[pr]
    x, y = a % n, a // n
    return 1 + run(board, n, c, x, y, dx, dy, extra) + run(board, n, c, x, y, -dx, -dy, extra)


def five_by_runs(board, n, c, a):
    return any(line_length(board, n, c, a, pr) == 5 for pr in range(4))


def five(env, side, a):
    """FIVE(side, a) through the oracle: place_stone of `side` at a wins (exactly five; Draw, the last empty cell, is none)"""
    e = O.Env.from_buffer_copy(env)
    e.turn = int(side)
    status = O.lib().orc_env_place_stone(C.byref(e), int(a))
    assert status >= 0
    return status in (O.BLACK_WIN, O.WHITE_WIN)


def winning_cells(board, n, c, a):
    """T(c, a): with c at a, the empty cells a +- k d (k = 1..4, four pairs) whose L along that same pair is exactly 5"""
    t = 0
    x, y = a % n, a // n
    for pr, (dx, dy) in enumerate(PAIRS):
        for k in (-4, -3, -2, -1, 1, 2, 3, 4):
            ex, ey = x + k * dx, y + k * dy
            if 0 <= ex < n and 0 <= ey < n:
                e = ey * n + ex
                if board[e] == O.EMPTY and line_length(board, n, c, e, pr, extra=a) == 5:
                    t += 1
    return t


def open_three(board, n, c, a):
    x, y = a % n, a // n
    for dx, dy in PAIRS:
        ra, rb = run(board, n, c, x, y, dx, dy), run(board, n, c, x, y, -dx, -dy)
        if 1 + ra + rb != 3:
            continue
        ends = ((x + (ra + 1) * dx, y + (ra + 1) * dy), (x - (rb + 1) * dx, y - (rb + 1) * dy))
        if all(0 <= ex < n and 0 <= ey < n and board[ey * n + ex] == O.EMPTY for ex, ey in ends):
            return True
    return False


def near(board, n, a):
    x, y = a % n, a // n
    return any(board[v * n + u] != O.EMPTY for u in range(max(0, x - 1), min(n, x + 2)) for v in range(max(0, y - 1), min(n, y + 2)) if (u, v) != (x, y))


def scan(env):
    """(cell of levels 1..5 else -1, level 1..7 or 0 on a full board, count of the draw's cells else 0, those cells)"""
    n = env.n
    board = [int(env.board[a]) for a in range(n * n)]
    empties = [a for a in range(n * n) if board[a] == O.EMPTY]
    me, opp = int(env.turn), 1 - int(env.turn)
    if not empties:
        return -1, 0, 0, []
    if len(empties) == 1:
        return empties[0], 1, 0, []  # Draw is terminal, as in the naive rule
    levels = (lambda a: five(env, me, a), lambda a: five(env, opp, a), lambda a: winning_cells(board, n, stone_of(me), a) >= 2,
              lambda a: winning_cells(board, n, stone_of(opp), a) >= 2, lambda a: open_three(board, n, stone_of(me), a))
    for level, test in enumerate(levels, start=1):
        for a in empties:  # ascending: the first hit is the lowest cell
            if test(a):
                return a, level, 0, []
    cells = [a for a in empties if near(board, n, a)]
    if cells:
        return -1, 6, len(cells), cells
    return -1, 7, len(empties), empties


def move(env, key, ply, game_global):
    """(cell, level) of the threat-aware player on `env`; key = oracle.stream_key(seed, episode)"""
    cell, level, count, cells = scan(env)
    if level <= 5:
        return cell, level
    out = (C.c_uint32 * 4)()
    O.lib().orc_philox(int(key), 0, int(ply), (2 * int(game_global) + int(env.turn)) & 0xFFFFFFFF, SO.RNG_OPPONENT, out)
    return cells[(int(out[0]) * count) >> 32], level


def play(n, kinds, key, game_global, start=None, max_plies=None):
    """One game between two scripted players, kinds = (Black's, White's) of OPP_THREAT / SO.OPP_NAIVE / SO.OPP_RANDOM, every draw as
    omok_opponent_actions makes it.  Returns (positions [(board bytes, side to move)] before every move, moves, final status)."""
    env = SO.make_env(n, np.zeros(n * n, dtype=np.uint8) if start is None else start, 0)
    stones = n * n - env.legal
    env.turn = stones & 1
    positions, moves, status = [], [], O.IN_PROGRESS
    while status == O.IN_PROGRESS and (max_plies is None or len(moves) < max_plies):
        side = int(env.turn)
        positions.append((np.array([env.board[a] for a in range(n * n)], dtype=np.uint8), side))
        ply = stones + len(moves)
        cell = move(env, key, ply, game_global)[0] if kinds[side] == OPP_THREAT else SO.move(kinds[side], env, key, ply, game_global)[0]
        status = O.lib().orc_env_place_stone(C.byref(env), int(cell))
        assert status >= 0
        moves.append(int(cell))
    return positions, moves, status


# ---- hand-made positions (coordinates fit 9 x 9 and 15 x 15) ----------------------------------------------------------------
def hand_made(n):
    """name -> (board, side to move, (cell, level, count) expected from the rule read by hand).  The lines lie on rows 4 and 8 (and 12
    at 15 x 15), which at 15 x 15 cross the 64-cell word boundaries of a bitboard (cells 63 | 64 on row 4, 127 | 128 on row 8, 191 | 192
    on row 12)."""
    assert n in (9, 15)
    at = lambda x, y: y * n + x  # noqa: E731
    out = {}
    rows = (4, 8) if n == 9 else (4, 8, 12)
    for side in (0, 1):
        own = lambda cells, side=side: (cells, []) if side == 0 else ([], cells)  # noqa: E731
        both = lambda mine, theirs, side=side: (mine, theirs) if side == 0 else (theirs, mine)  # noqa: E731
        for y in rows:
            x0 = {4: 3, 8: 6, 12: 10}[y] if n == 15 else 2  # at 15 x 15 the stones x0, x0 + 1, x0 + 2 straddle the row's word boundary
            tag = f"s{side}_r{y}"
            three = [at(x0 + i, y) for i in range(3)]
            # _XXX_ with free cells beyond: either completion leaves an open four (T = 2) -- level 3 at the lower one
            out[f"open_three_{tag}"] = (SO._board(n, *own(three)), side, (at(x0 - 1, y), 3, 0))
            # the opponent's open three: level 4 at the same cell
            out[f"their_open_three_{tag}"] = (SO._board(n, *own(three)), 1 - side, (at(x0 - 1, y), 4, 0))
            # split three XX_X with open ends: the gap makes an open four -- level 3 at the gap (the outer cells give T = 1 only)
            split = [at(x0, y), at(x0 + 1, y), at(x0 + 3, y)]
            out[f"split_three_{tag}"] = (SO._board(n, *own(split)), side, (at(x0 + 2, y), 3, 0))
            # two stones with free ends: level 5 at the lower extending cell
            two = [at(x0, y), at(x0 + 1, y)]
            out[f"two_{tag}"] = (SO._board(n, *own(two)), side, (at(x0 - 1, y), 5, 0))
        # a three against the edge (x = 0, 1, 2 on row 4): its completion (3, 4) leaves ONE winning cell, no level 3; extending it is
        # no OPEN3 either (one end is off the board), so the rule falls to level 6 -- 9 free cells around the three (rows 3 and 5: x = 0..3,
        # row 4: x = 3)
        edge = [at(x, 4) for x in range(3)]
        out[f"edge_three_s{side}"] = (SO._board(n, *own(edge)), side, (-1, 6, 9))
        # a three closed by an enemy stone at one end, x = 2, 3, 4 with the enemy at (1, 4): T = 1 at (5, 4), no level 3; OPEN3 needs
        # L == 3; the enemy's lone stone makes no level 4; level 5 has no cell either ((5, 4) gives L = 4) -- except vertical / diagonal
        # twos: none.  Level 6 over the neighbours of four stones in a row x = 1..4: rows 3 and 5 x = 0..5 (12 cells), row 4 x = 0, 5
        blocked = [at(x, 4) for x in (2, 3, 4)]
        out[f"blocked_three_s{side}"] = (SO._board(n, *both(blocked, [at(1, 4)])), side, (-1, 6, 14))
        # the open three x = 2, 3, 4 with an own stone at x = 6: (5, 4) makes exactly five, level 1; T at (1, 4) is 1, not 2 -- the
        # completion (5, 4) of the four x = 1..4 would make six (tests/test_threat_opponent.py asserts that T)
        out[f"six_near_s{side}"] = (SO._board(n, *own([at(2, 4), at(3, 4), at(4, 4), at(6, 4)])), side, (at(5, 4), 1, 0))
        # the three x = 2, 3, 4 with an own stone at x = 7 and an enemy stone at x = 0: at (5, 4) the completion (6, 4) would make six
        # (T = 1: only (1, 4)), at (1, 4) the completion (0, 4) is taken (T = 1: only (5, 4)) -- no level 3, where the same three without
        # the stone at x = 7 has T = 2 at (5, 4).  No L == 3 anywhere: level 6 over rows 3 and 5, x = 0..8, and row 4, x = 1, 5, 6, 8
        out[f"six_far_s{side}"] = (SO._board(n, *both([at(2, 4), at(3, 4), at(4, 4), at(7, 4)], [at(0, 4)])), side, (-1, 6, 22))
        # two stones whose line runs off the board at one end (x = 0, 1 on row 4): no level 5 -- level 6 over rows 3, 5 x = 0..2 and (2, 4)
        out[f"edge_two_s{side}"] = (SO._board(n, *own([at(0, 4), at(1, 4)])), side, (-1, 6, 7))
        # a lone stone: level 6 over its free neighbours
        out[f"lone_s{side}"] = (SO._board(n, *own([at(4, 4)])), side, (-1, 6, 8))
        out[f"lone_corner_s{side}"] = (SO._board(n, *own([at(0, 0)])), 1 - side, (-1, 6, 3))
        # the empty board: level 7 over every cell
        out[f"empty_s{side}"] = (SO._board(n, [], []), side, (-1, 7, n * n))
        # scripted_opponent's block_before_win: White's four on row 1 (completing cell (5, 1)), Black's on row 5 ((5, 5)): the side to
        # move takes ITS win, where the naive rule takes (5, 1) for both
        bbw = SO.hand_made(n)["block_before_win"][0]
        out[f"block_before_win_s{side}"] = (bbw, side, (at(5, 5) if side == 0 else at(5, 1), 1, 0))
        # only a block: scripted_opponent's closed four is Black's
        four = SO.hand_made(n)["four"][0]
        out[f"four_s{side}"] = (four, side, (at(5, 2), 1 if side == 0 else 2, 0))
        # one empty cell: level 1 (Draw is terminal)
        last, cell = SO.last_cell_position(n)
        out[f"last_cell_s{side}"] = (last, side, (cell, 1, 0))
    return out



# ---- the random set: positions of yardstick games, shared by the CPU and the GPU tests ---------------------------------------
RANDOM_SET_SEED = {9: 12, 15: 14}  # chosen with this file alone so that random_set meets the condition its users assert
_RANDOM_SET = {}


def random_set(n):
    """(boards uint8 [R][HW], turns uint8 [R], want int32 [R][3] = scan's (cell, level, count)): every position, with BOTH sides to move,
    of `games` games threat against threat, `games` games threat against naive (the threat player Black in the even games, White in the odd
    ones) and `games` random openings of 6 stones (tests/random_openings.py); games = 6 at 9 x 9, 4 at 15 x 15.  Computed once."""
    if n not in _RANDOM_SET:
        import random_openings as RO
        games = 6 if n == 9 else 4
        key = O.stream_key(RANDOM_SET_SEED[n], 0)
        boards = []
        for g in range(games):
            boards += [b for b, _side in play(n, (OPP_THREAT, OPP_THREAT), key, g)[0]]
            kinds = (OPP_THREAT, SO.OPP_NAIVE) if g % 2 == 0 else (SO.OPP_NAIVE, OPP_THREAT)
            boards += [b for b, _side in play(n, kinds, key, games + g)[0]]
        boards += list(RO.positions(n, key, 2 * games, 6, games)[0])
        boards = np.stack([b for b in boards for _t in (0, 1)])
        turns = np.array([t for _ in range(len(boards) // 2) for t in (0, 1)], dtype=np.uint8)
        want = np.array([scan(SO.make_env(n, b, t))[:3] for b, t in zip(boards, turns)], dtype=np.int32)
        _RANDOM_SET[n] = (boards, turns, want)
    return _RANDOM_SET[n]


def levels_by_side(turns, want):
    """{side: the set of levels the yardstick found with that side to move}"""
    return {side: set(int(x) for x in want[turns == side, 1]) for side in (0, 1)}


# ---- the lockstep episode of tests/test_gpu_threat.py at 15 x 15 ----------------------------------------------------------------
def lockstep_positions(n=15):
    """boards [4][HW] of 6 stones, Black to move; what the rule answers for Black at once, read by hand: game 0 Black's open three
    x = 3, 4, 5 on row 4 across the word boundary 63 | 64 (level 3), game 1 White's open three there (level 4), game 2 Black's two
    (level 5), game 3 six stones no two of which touch (level 6).  The other stones lie apart on the rows n - 1 / n - 2."""
    at = lambda x, y: y * n + x  # noqa: E731
    far = [at(1, n - 1), at(5, n - 1), at(9, n - 1), at(13, n - 2)]
    row = [at(3, 4), at(4, 4), at(5, 4)]
    boards = [SO._board(n, row, far[:3]), SO._board(n, far[:3], row), SO._board(n, row[:2] + far[3:], far[:3]),
              SO._board(n, [at(2, 2), at(7, 5), at(11, 9)], far[:3])]
    return np.stack(boards), [3, 4, 5, 6]


# ---- the tactics report of records.GameRecords.tactics, walked game by game --------------------------------------------------
def tactics(n, start, cells):
    """One game: (level_before of every move, missed_win [2], unblocked [2]) -- the mover's level in front of each move; a level-1
    position whose move did not end the game; a level-2 position whose move leaves the opponent a level-1 position."""
    start = np.asarray(start, dtype=np.uint8).reshape(-1)
    env = SO.make_env(n, start, int(np.count_nonzero(start)) & 1)
    levels, missed, unblocked = [], [0, 0], [0, 0]
    for cell in cells:
        side, level = int(env.turn), scan(env)[1]
        levels.append(level)
        status = O.lib().orc_env_place_stone(C.byref(env), int(cell))
        assert status >= 0
        if status != O.IN_PROGRESS:
            break
        if level == 1:
            missed[side] += 1
        if level == 2 and scan(env)[1] == 1:
            unblocked[side] += 1
    assert len(levels) == len(cells)
    return levels, missed, unblocked
