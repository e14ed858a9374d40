"""The defending scripted player (OMOK_OPP_GUARD, omok_env_guard_scan), restated in plain Python from the rule in include/omok_mi355x.h (a
helper of tests/test_guard_opponent.py and tests/test_gpu_guard.py; not a test, no product code).

The rule is a plain composition of the other yardsticks: threat_opponent.scan for the threat rule's level and cells, vcf_solver.solve for the
two solves, vcf_defence.defend for the map (its null move is computed and not read), threat_opponent.winning_cells / open_three / near for the
restricted levels, and orc_philox for the games' draw words.

  move(env, x0, D, NB)            -> (cell, step, level, count) as omok_env_guard_scan returns them for the draw word x0
  play(n, kinds, key, game_global) -> vcf_solver.play with OPP_GUARD among the kinds, plus the guard's log
  hand_made(n), games(n), scan_set(n), want(n, D, NB, drawn) -> the shared test sets and their yardstick results, computed once per process
"""
import ctypes as C

import numpy as np

from oracle import oracle as O
import scripted_opponent as SO
import threat_opponent as TO
import vcf_defence as VD
import vcf_solver as VS

OPP_GUARD = 7
D_OPP, NB_OPP = VS.VCF_OPP_DEPTH, VS.VCF_OPP_NODES


def _pick(cells, x0):
    return cells[(int(x0) * len(cells)) >> 32]


def vcf_move(env, x0, D, NB):
    """(c0, L0, solved, n0): OMOK_OPP_VCF's move with the draw word x0 and the solver at (D, NB)"""
    n = env.n
    cell, level, count, cells = TO.scan(env)
    if level >= 3:
        r = VS.solve(n, [int(env.board[a]) for a in range(n * n)], int(env.turn), D, NB)
        if r.verdict == 1:
            return r.cell, level, True, 0
    if level <= 5:
        return cell, level, False, 0
    return _pick(cells, x0), level, False, count


def restricted(board, n, me, M, x0):
    """(cell, level, count) of the threat rule's levels 3..7 on the cells M (ascending, not empty)"""
    mine, theirs = TO.stone_of(me), TO.stone_of(1 - me)
    tests = (lambda a: TO.winning_cells(board, n, mine, a) >= 2, lambda a: TO.winning_cells(board, n, theirs, a) >= 2,
             lambda a: TO.open_three(board, n, mine, a))
    for level, test in enumerate(tests, start=3):
        for a in M:
            if test(a):
                return a, level, 0
    cells = [a for a in M if TO.near(board, n, a)]
    if cells:
        return _pick(cells, x0), 6, len(cells)
    return _pick(M, x0), 7, len(M)


def move(env, x0, D=D_OPP, NB=NB_OPP):
    n = env.n
    me = int(env.turn)
    c0, L0, solved, n0 = vcf_move(env, x0, D, NB)
    if L0 == 0:
        return -1, 0, 0, 0
    if L0 <= 2 or solved:
        return c0, 1, L0, n0
    board = [int(env.board[a]) for a in range(n * n)]
    board[c0] = TO.stone_of(me)
    r = VS.solve(n, board, 1 - me, D, NB)
    board[c0] = O.EMPTY
    if r.verdict != 1:
        return c0, 2, L0, n0
    status = VD.defend(n, board, me, D, NB).status
    assert status[c0] == VD.LOSES and VD.WINS not in status
    for step, kind in ((3, VD.SAFE), (4, VD.UNKNOWN)):
        M = [a for a in range(n * n) if status[a] == kind]
        if M:
            cell, level, count = restricted(board, n, me, M, x0)
            return cell, step, level, count
    return c0, 5, L0, n0


def draw_word(key, ply, game_global, side):
    out = (C.c_uint32 * 4)()
    O.lib().orc_philox(int(key), 0, int(ply), (2 * int(game_global) + int(side)) & 0xFFFFFFFF, SO.RNG_OPPONENT, out)
    return int(out[0])


def play(n, kinds, key, game_global, start=None, max_plies=None):
    """vcf_solver.play with OPP_GUARD among the kinds.  Returns (positions, moves, status, log): log = [(index of the move, x0, cell, step,
    level, count)] of the guard's moves."""
    env = SO.make_env(n, np.zeros(n * n, dtype=np.uint8) if start is None else start, 0)
    stones = n * n - env.legal
    env.turn = stones & 1
    positions, moves, status, log = [], [], O.IN_PROGRESS, []
    while status == O.IN_PROGRESS and (max_plies is None or len(moves) < max_plies):
        side = int(env.turn)
        positions.append((np.array([env.board[a] for a in range(n * n)], dtype=np.uint8), side))
        ply = stones + len(moves)
        if kinds[side] == OPP_GUARD:
            x0 = draw_word(key, ply, game_global, side)
            cell, step, level, count = move(env, x0)
            log.append((len(moves), x0, cell, step, level, count))
        elif kinds[side] == VS.OPP_VCF:
            cell = VS.move(env, key, ply, game_global)[0]
        elif kinds[side] == TO.OPP_THREAT:
            cell = TO.move(env, key, ply, game_global)[0]
        else:
            cell = SO.move(kinds[side], env, key, ply, game_global)[0]
        status = O.lib().orc_env_place_stone(C.byref(env), int(cell))
        assert status >= 0
        moves.append(int(cell))
    return positions, moves, status, log


# ---- hand-made positions (coordinates fit 9 x 9 and 15 x 15) ---------------------------------------------------------------------
def hand_made(n):
    """name -> (board, side to move, D, NB, (cell, step, level, count) read by hand from the rule with x0 = 0).  The stones lie around
    row 4 from x0 = vcf_solver._x0(n, 4) on, so at 15 x 15 the row stones cross the word boundary 63 | 64; `me` is the side to move."""
    assert n in (9, 15)
    at = lambda x, y: y * n + x  # noqa: E731
    x0 = VS._x0(n, 4)
    out = {}
    for side in (0, 1):
        both = lambda mine, theirs, side=side: (mine, theirs) if side == 0 else (theirs, mine)  # noqa: E731
        B = lambda mine, theirs=(), both=both: SO._board(n, *both(list(mine), list(theirs)))  # noqa: E731
        row3 = [at(x0 + i, 4) for i in range(3)]
        column = [at(x0 + 3, 3), at(x0 + 3, 2)]
        # step 1, own: me holds vcf_solver's chain_m3.  The threat rule alone is at level 5 ((x0 + 3, 1) makes the column an open three);
        # the solver's level decides at (x0 + 3, 4), so the count is 0
        out[f"own_win_s{side}"] = (B(row3 + column, [at(x0 - 1, 4)]), side, D_OPP, NB_OPP, (at(x0 + 3, 4), 1, 5, 0))
        # step 1, own: opp's four x0 .. x0 + 3, closed by me at x0 - 1: level 2, the block at its one free end
        out[f"block_five_s{side}"] = (B([at(x0 - 1, 4)], [at(x0 + i, 4) for i in range(4)]), side, D_OPP, NB_OPP, (at(x0 + 4, 4), 1, 2, 0))
        # step 2, kept: opp's open three _XXX_ and nothing else.  Level 4 blocks at (x0 - 1, 4), the lower of the two cells with
        # T(opp) >= 2; after it the three's one four, (x0 + 3, 4), leaves one completing cell and leads nowhere: verdict 0, the move stays
        out[f"kept_block_s{side}"] = (B([], row3), side, D_OPP, NB_OPP, (at(x0 - 1, 4), 2, 4, 0))
        # step 3: chain_m3 with the colours' roles swapped: opp holds the row three (closed by me at x0 - 1) and the column two (x0 + 3, 2..3).
        # Opp wins in three: (x0 + 3, 4) makes the row a four (reply (x0 + 4, 4)) and the column a three, then (x0 + 3, 1) or (x0 + 3, 5)
        # makes it an open four.  me has one stone and opp no cell with T >= 2, so L0 = 6: 20 cells have a neighbour, x0 = 0 draws the
        # lowest, (x0 + 2, 1), which loses.  The cells that hold (SAFE at D = 3): (x0 + 3, 4), where row and column meet; (x0 + 4, 4), after
        # which (x0 + 3, 4) leaves no completing cell; and (x0 + 3, 1) and (x0 + 3, 5), each of which is the one open-four cell and the
        # other's second completing cell.  ((x0 + 3, 0) and (x0 + 3, 6) lose: the open four at the other end stays.)  On these four cells:
        # no level 3 (me has one stone), no level 4 (opp at any of them leaves at most one completing cell), no level 5; all four have a
        # neighbour: level 6, count 4, x0 = 0 takes the lowest, (x0 + 3, 1)
        swapped = B([at(x0 - 1, 4)], row3 + column)
        out[f"map_safe_s{side}"] = (swapped, side, 3, NB_OPP, (at(x0 + 3, 1), 3, 6, 4))
        # step 4: the same position at D = 6 with 4 nodes.  Opp's win after a stone elsewhere takes exactly 4 nodes (one root per depth 1, 2, 3
        # and the node after (x0 + 3, 4), the first candidate, where (x0 + 3, 1) leaves two completing cells), so (x0 + 2, 1) still LOSES;
        # a verdict 0 would take one root per depth, 6 nodes: the four cells above run out of budget, UNKNOWN, and no cell is SAFE.  (me's own
        # solve runs out as well, so the solver's level does not decide.)  The restricted rule picks as above
        out[f"map_unknown_s{side}"] = (swapped, side, 6, 4, (at(x0 + 3, 1), 4, 6, 4))
        # step 5: two independent forced wins -- opp's open threes on row 4 and on row 8, me without a stone near them.  Level 4 blocks the
        # lower one at (x0 - 1, 4); whatever me plays, the other three becomes an open four: every cell LOSES, the move stays with L0 = 4
        x8 = VS._x0(n, 8)
        out[f"all_lose_s{side}"] = (B([], row3 + [at(x8 + i, 8) for i in range(3)]), side, D_OPP, NB_OPP, (at(x0 - 1, 4), 5, 4, 0))
    return out


# ---- the shared sets: the yardstick's games, computed once per process and left unchanged -----------------------------------------------
GAMES = {9: (3, 12), 15: (5, 8)}  # board size -> (seed, games): game indices 0 .. games - 1 under stream_key(seed, 0), each colour assignment
BUDGETS = ((6, 256), (8, 8), (2, 4096))
DRAW_SEED = 20261021
_GAMES, _SCAN_SET, _WANT = {}, {}, {}


def games(n):
    """{guard's colour: [play(n, kinds, key, g) for g]}: search-free games of the guard against OMOK_OPP_VCF"""
    if n not in _GAMES:
        seed, count = GAMES[n]
        key = O.stream_key(seed, 0)
        _GAMES[n] = {side: [play(n, (OPP_GUARD, VS.OPP_VCF) if side == 0 else (VS.OPP_VCF, OPP_GUARD), key, g) for g in range(count)] for side in (0, 1)}
    return _GAMES[n]


def game_steps(n):
    """[(step, level, r > 0)] of every guard move of games(n): r = mulhi(x0, count) is the index the draw picked"""
    return [(step, level, ((x0 * count) >> 32) > 0) for side in (0, 1) for _p, _m, _s, log in games(n)[side] for _i, x0, _c, step, level, count in log]


def assert_not_vacuous(steps):
    """the conditions under which a comparison with the yardstick says something: every step 1..5 occurs, step 3 with a level <= 5 and with
    level 6, and some draw picked another cell than the lowest"""
    assert {1, 2, 3, 4, 5} <= {s for s, _l, _r in steps}, sorted({s for s, _l, _r in steps})
    assert any(s == 3 and l <= 5 for s, l, _r in steps) and any(s == 3 and l == 6 for s, l, _r in steps)
    assert any(r for _s, _l, r in steps)


SUBSAMPLE = {9: (1, 5), 15: (2, 3)}  # (first, stride): chosen with this file alone so that the set holds just under 100 game positions and meets assert_not_vacuous


def scan_set(n):
    """(boards [R][HW], turns [R], draws uint32 [R]): the hand-made positions and every stride-th position (SUBSAMPLE) in front of a guard move of
    games(n), in the order Black's games, White's games; draw words from a fixed seed"""
    if n not in _SCAN_SET:
        hand = sorted(hand_made(n).items())
        boards, turns = [b for _name, (b, _s, _d, _nb, _w) in hand], [s for _name, (_b, s, _d, _nb, _w) in hand]
        picked = [positions[i] for side in (0, 1) for positions, _m, _s, log in games(n)[side] for i, _x, _c, _st, _l, _n in log][SUBSAMPLE[n][0]::SUBSAMPLE[n][1]]
        boards += [b for b, _t in picked]
        turns += [t for _b, t in picked]
        draws = np.random.default_rng(DRAW_SEED + n).integers(0, 1 << 32, size=len(boards), dtype=np.uint64).astype(np.uint32)
        _SCAN_SET[n] = (np.stack(boards), np.array(turns, dtype=np.uint8), draws)
    return _SCAN_SET[n]


def want(n, D, NB, drawn):
    """int32 [R][4] = move's (cell, step, level, count) on scan_set(n) with its draws (drawn) or with x0 = 0"""
    if (n, D, NB, drawn) not in _WANT:
        boards, turns, draws = scan_set(n)
        _WANT[(n, D, NB, drawn)] = np.array([move(SO.make_env(n, b, int(t)), int(x) if drawn else 0, D, NB) for b, t, x in zip(boards, turns, draws)],
                                            dtype=np.int32)
    return _WANT[(n, D, NB, drawn)]


