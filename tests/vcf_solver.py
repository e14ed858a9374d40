"""The forced-win solver (victory by continuous fours, omok_env_vcf_solve) and the scripted player that uses it (OMOK_OPP_VCF), restated
in plain Python from the rule in include/omok_mi355x.h (a helper of tests/test_vcf_solver.py, tests/test_gpu_vcf.py and
tests/test_records_forced_wins.py; not a test, no product code).

FIVE goes through the oracle's orc_env_place_stone (threat_opponent.five); T and W are restated on the Stone bytes with
threat_opponent.line_length.  Work that cannot change the result or the node count is skipped: a cell can only complete five, or leave a
completing cell, along a line pair on which enough stones of that colour lie within four steps of it.

  solve(n, board, me, D, NB) -> Result(verdict, cell, moves, nodes, pv [2 D - 1], fo1, fo2): fo1 / fo2 count the nodes at which the
                                |Fo| == 1 and the |Fo| >= 2 branch was taken
  move(env, key, ply, game_global) -> (cell, level, solved): the move omok_opponent_actions(OMOK_OPP_VCF) stages
"""
import collections
import ctypes as C

import numpy as np

from oracle import oracle as O
import scripted_opponent as SO
import threat_opponent as TO

OPP_VCF = 5
VCF_OPP_DEPTH, VCF_OPP_NODES = 6, 256

Result = collections.namedtuple("Result", "verdict cell moves nodes pv fo1 fo2")


class _Budget(Exception):
    pass


def _counts(board, n, c):
    """{(cell, pair): the number of c stones within four steps of the cell along the pair} (only the non-zero ones)"""
    cnt = collections.Counter()
    for s in range(n * n):
        if board[s] != c:
            continue
        x, y = s % n, s // n
        for pr, (dx, dy) in enumerate(TO.PAIRS):
            for k in (-4, -3, -2, -1, 1, 2, 3, 4):
                u, v = x + k * dx, y + k * dy
                if 0 <= u < n and 0 <= v < n:
                    cnt[(v * n + u, pr)] += 1
    return cnt


def fives(n, board, side, cnt=None):
    """the empty cells a with FIVE(side, a), ascending (a five needs four stones of that colour within four steps on one pair)"""
    cnt = _counts(board, n, TO.stone_of(side)) if cnt is None else cnt
    cells = sorted(set(a for (a, _pr), k in cnt.items() if k >= 4 and board[a] == O.EMPTY))
    if not cells:
        return []
    env = SO.make_env(n, np.array(board, dtype=np.uint8), side)
    return [a for a in cells if TO.five(env, side, a)]


def completing_cells(board, n, c, a, cnt=None):
    """W(a) for the colour c: with c at a, the empty cells a +- k d (k = 1..4, four pairs) whose L along that same pair is exactly 5; ascending"""
    w = []
    x, y = a % n, a // n
    for pr, (dx, dy) in enumerate(TO.PAIRS):
        if cnt is not None and cnt[(a, pr)] < 3:  # the five holds a, the completing cell and three more stones, all within four steps of a
            continue
        for k in (-4, -3, -2, -1, 1, 2, 3, 4):
            ex, ey = x + k * dx, y + k * dy
            if 0 <= ex < n and 0 <= ey < n:
                e = ey * n + ex
                if board[e] == O.EMPTY and TO.line_length(board, n, c, e, pr, extra=a) == 5:
                    w.append(e)
    return sorted(w)


def solve(n, board, me, D, NB):
    assert 1 <= D <= 16 and 1 <= NB <= 65536
    board = [int(s) if int(s) in (O.BLACK, O.WHITE) else O.EMPTY for s in board]  # a byte other than 1 or 2 counts as empty
    mine, theirs = TO.stone_of(me), TO.stone_of(1 - me)
    state = {"nodes": 0, "fo1": 0, "fo2": 0}

    def search(r):
        state["nodes"] += 1
        if state["nodes"] > NB:
            raise _Budget()
        cnt = _counts(board, n, mine)
        won = fives(n, board, me, cnt)
        if won:
            return [won[0]]
        if r == 1:
            return None
        fo = fives(n, board, 1 - me)
        if len(fo) >= 2:
            state["fo2"] += 1
            return None
        if len(fo) == 1:
            state["fo1"] += 1
        near = sorted(set(a for (a, _pr), k in cnt.items() if k >= 3 and board[a] == O.EMPTY))  # (the others have T = 0)
        for a in (fo if len(fo) == 1 else near):
            w = completing_cells(board, n, mine, a, cnt)
            if len(w) >= 2:
                return [a, w[0], w[1]]
            if len(w) == 1 and r >= 3:
                board[a], board[w[0]] = mine, theirs
                pv = search(r - 1)
                board[a], board[w[0]] = O.EMPTY, O.EMPTY
                if pv:
                    return [a, w[0]] + pv
        return None

    none = [-1] * (2 * D - 1)
    try:
        for d in range(1, D + 1):
            pv = search(d)
            if pv:
                assert len(pv) == 2 * d - 1
                return Result(1, pv[0], d, state["nodes"], pv + none[len(pv):], state["fo1"], state["fo2"])
    except _Budget:
        return Result(-1, -1, 0, NB, none, state["fo1"], state["fo2"])
    return Result(0, -1, 0, state["nodes"], none, state["fo1"], state["fo2"])


def solve_batch(n, boards, turns, D, NB):
    """(verdict, cell, moves, nodes int32 [B], pv int32 [B][2 D - 1], results): what Engine.env_vcf_solve returns, and the Results"""
    res = [solve(n, b, int(t), D, NB) for b, t in zip(boards, turns)]
    cols = [np.array([getattr(r, f) for r in res], dtype=np.int32) for f in ("verdict", "cell", "moves", "nodes")]
    return (*cols, np.array([r.pv for r in res], dtype=np.int32).reshape(len(res), 2 * D - 1), res)


def closure(n, board, me, pv):
    """The line of a verdict-1 answer replayed through place_stone: it ends in the attacker's win at its last cell; after each attacker
    move but the last the defender has no five, and every cell of W other than the reply is a FIVE for the attacker."""
    pv = [int(c) for c in pv if c >= 0]
    assert len(pv) % 2 == 1
    env = SO.make_env(n, np.asarray(board, dtype=np.uint8), me)
    win = O.BLACK_WIN if me == 0 else O.WHITE_WIN
    for i, cell in enumerate(pv):
        assert int(env.turn) == (me if i % 2 == 0 else 1 - me)
        before = [int(env.board[a]) for a in range(n * n)]
        status = O.lib().orc_env_place_stone(C.byref(env), cell)
        if i == len(pv) - 1:
            assert status == win
            return
        assert status == O.IN_PROGRESS
        if i % 2 == 0:
            now = [int(env.board[a]) for a in range(n * n)]
            assert not fives(n, now, 1 - me)
            w = completing_cells(before, n, TO.stone_of(me), cell)
            assert pv[i + 1] in w
            assert all(TO.five(env, me, e) for e in w)  # (the reply included: it is the one cell the defender must take)


# ---- the scripted player -------------------------------------------------------------------------------------------------------
def scripted_cell(env):
    """(cell of levels 1..5 or the solver's, else -1; the threat rule's level; did the solver's level decide)"""
    cell, level = TO.scan(env)[:2]
    if level >= 3:
        n = env.n
        r = solve(n, [int(env.board[a]) for a in range(n * n)], int(env.turn), VCF_OPP_DEPTH, VCF_OPP_NODES)
        if r.verdict == 1:
            return r.cell, level, True
    return cell, level, False


def move(env, key, ply, game_global):
    """(cell, level, solved) of the OMOK_OPP_VCF player on `env`: the threat-aware rule with the solver's level after level 2"""
    cell, level, solved = scripted_cell(env)
    if solved or level <= 5:
        return cell, level, solved
    return TO.move(env, key, ply, game_global)[0], level, False


def play(n, kinds, key, game_global, start=None, max_plies=None):
    """threat_opponent.play with OPP_VCF among the kinds"""
    env = SO.make_env(n, np.zeros(n * n, dtype=np.uint8) if start is None else start, 0)
    stones = n * n - env.legal
    env.turn = stones & 1
    positions, moves, status = [], [], O.IN_PROGRESS
    while status == O.IN_PROGRESS and (max_plies is None or len(moves) < max_plies):
        side = int(env.turn)
        positions.append((np.array([env.board[a] for a in range(n * n)], dtype=np.uint8), side))
        ply = stones + len(moves)
        if kinds[side] == OPP_VCF:
            cell = move(env, key, ply, game_global)[0]
        elif kinds[side] == TO.OPP_THREAT:
            cell = TO.move(env, key, ply, game_global)[0]
        else:
            cell = SO.move(kinds[side], env, key, ply, game_global)[0]
        status = O.lib().orc_env_place_stone(C.byref(env), int(cell))
        assert status >= 0
        moves.append(int(cell))
    return positions, moves, status


# ---- hand-made positions (coordinates fit 9 x 9 and 15 x 15) ------------------------------------------------------------------------
def _x0(n, y):
    return {4: 3, 8: 6, 12: 10}[y] if n == 15 else 2  # as threat_opponent.hand_made: at 15 x 15 the stones straddle the row's word boundary


def hand_made(n):
    """name -> (board, side to move, D, (verdict, moves, cell) read by hand from the rule).  The rows are threat_opponent.hand_made's: 4 and
    8 (and 12 at 15 x 15); at 15 x 15 the row stones x0, x0 + 1, ... cross the 64-cell word boundaries (63 | 64 on row 4, 127 | 128 on row
    8, 191 | 192 on row 12).  The positions of several lines lie around row 4."""
    assert n in (9, 15)
    at = lambda x, y: y * n + x  # noqa: E731
    out = {}
    rows = (4, 8) if n == 9 else (4, 8, 12)
    for side in (0, 1):
        both = lambda mine, theirs, side=side: (mine, theirs) if side == 0 else (theirs, mine)  # noqa: E731
        B = lambda mine, theirs=(), both=both: SO._board(n, *both(list(mine), list(theirs)))  # noqa: E731
        for y in rows:
            x0, tag = _x0(n, y), f"s{side}_r{y}"
            four = [at(x0 + i, y) for i in range(4)]
            # 1. a closed four: the one free end wins (m = 1); an open four: two completing cells, the lower wins
            out[f"closed_four_{tag}"] = (B(four, [at(x0 - 1, y)]), side, 8, (1, 1, at(x0 + 4, y)))
            out[f"open_four_{tag}"] = (B(four), side, 8, (1, 1, at(x0 - 1, y)))
            # 2. an open three _XXX_: x0 - 2 leaves one completing cell (the gap) and is passed over at r = 2, x0 - 1 leaves two: m = 2 at
            # the lower end; a split three XX_X: the outer cells leave one completing cell, the gap two: m = 2 at the gap
            out[f"open_three_{tag}"] = (B(four[:3]), side, 8, (1, 2, at(x0 - 1, y)))
            out[f"split_three_{tag}"] = (B([four[0], four[1], four[3]]), side, 8, (1, 2, at(x0 + 2, y)))
            # 9. only the opponent has threats
            out[f"their_open_three_{tag}"] = (B([], four[:3]), side, 8, (0, 0, -1))
        x0 = _x0(n, 4)
        row3 = [at(x0 + i, 4) for i in range(3)]
        # 3. two closed threes whose fours chain: the row three x0 .. x0 + 2 is closed by an enemy stone at x0 - 1; (x0 + 3, 4) makes it a
        # four (reply (x0 + 4, 4)) and the column (x0 + 3, 2..3) a three; (x0 + 3, 1) then makes an open four.  No cell leaves two completing
        # cells at once, so m = 3.  4. the same position is verdict 0 at D = 2
        chain = B(row3 + [at(x0 + 3, 3), at(x0 + 3, 2)], [at(x0 - 1, 4)])
        out[f"chain_m3_s{side}"] = (chain, side, 3, (1, 3, at(x0 + 3, 4)))
        out[f"chain_m3_at_depth_2_s{side}"] = (chain, side, 2, (0, 0, -1))
        # m = 4: the column is closed above by an enemy stone at (x0 + 3, 1), so after (x0 + 3, 4) its four (x0 + 3, 5) leaves one completing
        # cell (reply (x0 + 3, 6)); (x0 + 3, 5) also joins (x0 + 2, 4) and the stone at (x0 + 4, 6) to a diagonal three, and (x0 + 1, 3) then
        # makes the open four (x0 + 1, 3) .. (x0 + 4, 6)
        m4 = B(row3 + [at(x0 + 3, 3), at(x0 + 3, 2), at(x0 + 4, 6)], [at(x0 - 1, 4), at(x0 + 3, 1)])
        out[f"chain_m4_s{side}"] = (m4, side, 8, (1, 4, at(x0 + 3, 4)))
        out[f"chain_m4_at_depth_3_s{side}"] = (m4, side, 3, (0, 0, -1))
        # 5. the forced block (x0 + 4, 4) gives the defender the four (x0 + 4, 4..7), closed below by an own stone at (x0 + 4, 8): its one
        # completing cell (x0 + 4, 3) is also the fourth stone of the attacker's anti-diagonal (x0 + 1, 6), (x0 + 2, 5), (x0 + 3, 4): an open
        # four, m = 3
        theirs = [at(x0 - 1, 4), at(x0 + 4, 5), at(x0 + 4, 6), at(x0 + 4, 7)]
        mine = row3 + [at(x0 + 2, 5), at(x0 + 1, 6)]
        out[f"blocking_four_s{side}"] = (B(mine + [at(x0 + 4, 8)], theirs), side, 8, (1, 3, at(x0 + 3, 4)))
        # 6. without the stone at (x0 + 4, 8) the defender's four is open: two fives, that line fails; the other four, (x0 + 4, 4), is
        # answered at (x0 + 3, 4), which takes the anti-diagonal too: verdict 0
        out[f"block_leaves_two_fives_s{side}"] = (B(mine, theirs), side, 8, (0, 0, -1))
        # 7. the three x0 .. x0 + 2 with an own stone at x0 + 5 and an enemy stone at x0 - 1: (x0 + 3, 4) makes four stones in a row, but
        # (x0 + 4, 4) would make six and (x0 - 1, 4) is taken -- no completing cell, it is no four; (x0 + 4, 4) likewise: verdict 0
        out[f"six_is_no_four_s{side}"] = (B(row3 + [at(x0 + 5, 4)], [at(x0 - 1, 4)]), side, 8, (0, 0, -1))
        # 8. a three against the edge (x = 0, 1, 2): its fours leave one completing cell each and lead nowhere
        out[f"edge_three_s{side}"] = (B([at(x, 4) for x in range(3)]), side, 8, (0, 0, -1))
        # 10. one empty cell (placing there is a Draw, no five); a full board
        last, cell = SO.last_cell_position(n)
        out[f"last_cell_s{side}"] = (last, side, 8, (0, 0, -1))
        full = last.copy()
        full[cell] = O.BLACK
        out[f"full_board_s{side}"] = (full, side, 8, (0, 0, -1))
    return out


# ---- the random set: positions of yardstick games, shared by the CPU and the GPU tests -----------------------------------------------
RANDOM_SET_SEED = {9: 6, 15: 10}  # chosen with this file alone so that random_set meets the conditions its users assert
RANDOM_SET_GAMES = {9: 3, 15: 2}
_RANDOM_SET = {}
_WANT = {}


def random_set(n):
    """(boards uint8 [R][HW], turns uint8 [R]): every position, with BOTH sides to move, of `games` games threat against threat, `games`
    games threat against naive (the threat player Black in the even games, White in the odd ones) and `games` random openings of 6 stones
    (tests/random_openings.py); games = 3 at 9 x 9, 2 at 15 x 15 (threat_opponent.random_set's make, with a seed of this file's own)."""
    if n not in _RANDOM_SET:
        import random_openings as RO
        games = RANDOM_SET_GAMES[n]
        key = O.stream_key(RANDOM_SET_SEED[n], 0)
        boards = []
        for g in range(games):
            boards += [b for b, _side in TO.play(n, (TO.OPP_THREAT, TO.OPP_THREAT), key, g)[0]]
            kinds = (TO.OPP_THREAT, SO.OPP_NAIVE) if g % 2 == 0 else (SO.OPP_NAIVE, TO.OPP_THREAT)
            boards += [b for b, _side in TO.play(n, kinds, key, games + g)[0]]
        boards += list(RO.positions(n, key, 2 * games, 6, games)[0])
        boards = np.stack([b for b in boards for _t in (0, 1)])
        turns = np.array([t for _ in range(len(boards) // 2) for t in (0, 1)], dtype=np.uint8)
        _RANDOM_SET[n] = (boards, turns)
    return _RANDOM_SET[n]


def random_set_want(n, D, NB):
    """solve_batch on the random set, computed once per (n, D, NB) and left unchanged"""
    if (n, D, NB) not in _WANT:
        boards, turns = random_set(n)
        _WANT[(n, D, NB)] = solve_batch(n, boards, turns, D, NB)
    return _WANT[(n, D, NB)]


# ---- the forced-win report of records.GameRecords.forced_wins, walked game by game -----------------------------------------------------
def forced_wins(n, start, cells, status, D, NB):
    """One game: (moves_before of every move, had [2], dropped [2]).  moves_before[p]: the mover's `moves` in front of move p (0 none
    within D, -1 budget).  had: per side the moves with moves_before = m >= 2.  dropped: those of them for which the record shows the win
    let go -- the game ended at move p or p + 1 without the mover winning, or move p + 2 exists and moves_before[p + 2] is not in 1..m - 1."""
    start = np.asarray(start, dtype=np.uint8).reshape(-1)
    env = SO.make_env(n, start, int(np.count_nonzero(start)) & 1)
    before, sides = [], []
    for cell in cells:
        side = int(env.turn)
        r = solve(n, [int(env.board[a]) for a in range(n * n)], side, D, NB)
        before.append(r.moves if r.verdict == 1 else r.verdict)
        sides.append(side)
        assert O.lib().orc_env_place_stone(C.byref(env), int(cell)) == (O.IN_PROGRESS if len(before) < len(cells) else status)
    had, dropped = [0, 0], [0, 0]
    length, over = len(cells), status != O.IN_PROGRESS
    for p, (m, side) in enumerate(zip(before, sides)):
        if m < 2:
            continue
        had[side] += 1
        won = over and status == (O.BLACK_WIN if side == 0 else O.WHITE_WIN)
        if over and p >= length - 2:  # the game ended at move p or p + 1
            dropped[side] += 0 if (won and p == length - 1) else 1
        elif p + 2 < length and not 1 <= before[p + 2] <= m - 1:
            dropped[side] += 1
    return before, had, dropped
