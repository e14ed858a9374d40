"""Caller-supplied positions, restated through the oracle library (a helper of tests/test_position_yardstick.py and
tests/test_gpu_positions.py; not a test, no product code).

  verdict       the position verdicts of omok_env_check_positions through the oracle's place_stone (environment/src/lib.rs:104-166):
                a stone "taken as the last one placed" = remove it, place it again, read the status.
  hand_made     name -> (board, verdict) pinned by hand.
  quiet         random positions of s <= 8 stones: at most four per colour, so no run of five exists on any way to them.
  drive_to      the yardstick construction: an oracle SelfPlay driven from its ordinary reset to the positions by external moves; after
                it both trees of every game are the one-node trees omok_selfplay_reset_from must produce (node 0's `action` aside).
"""
import ctypes as C

import numpy as np

from oracle import oracle as O
from scripted_opponent import make_env

LEGAL, BAD_BYTE, BAD_COUNTS, WON, FULL = 0, 1, 2, 3, 4


def verdict(n, board):
    """(verdict, stones) of one board [HW] of bytes: the first verdict that applies, in the order 1, 2, 3, 4"""
    board = np.asarray(board, dtype=np.uint8).reshape(-1)
    assert board.size == n * n
    black, white = int(np.count_nonzero(board == O.BLACK)), int(np.count_nonzero(board == O.WHITE))
    stones = black + white
    if np.any(board > 2):
        return BAD_BYTE, stones
    if black != white and black != white + 1:
        return BAD_COUNTS, stones
    env = make_env(n, board, O.TURN_BLACK)
    for cell in np.flatnonzero(board):  # the stone taken as the last one placed: remove it, place it again
        e = O.Env.from_buffer_copy(env)
        e.board[cell] = O.EMPTY
        e.legal += 1
        e.turn = O.TURN_BLACK if board[cell] == O.BLACK else O.TURN_WHITE
        status = O.lib().orc_env_place_stone(C.byref(e), int(cell))
        assert status >= 0
        if status in (O.BLACK_WIN, O.WHITE_WIN):
            return WON, stones
    if stones == n * n:
        return FULL, stones
    return LEGAL, stones


def verdicts(n, boards):
    out = [verdict(n, b) for b in boards]
    return np.array([v for v, _ in out], dtype=np.int32), np.array([s for _, s in out], dtype=np.int32)


def _board(n, black, white):
    b = np.zeros(n * n, dtype=np.uint8)
    for cells, colour in ((black, O.BLACK), (white, O.WHITE)):
        for c in cells:
            assert b[c] == 0
            b[c] = colour
    return b


def _line(n, x, y, dx, dy, length):
    return [(y + dy * i) * n + (x + dx * i) for i in range(length)]


def _scatter(n, avoid, count):
    """`count` cells of row n - 1 / n - 2, no two adjacent, none in `avoid`: quiet stones that form no line"""
    cells = [c for c in [(n - 1) * n + x for x in range(0, n, 2)] + [(n - 3) * n + x for x in range(1, n, 2)] if c not in avoid]
    assert len(cells) >= count
    return cells[:count]


DIRECTIONS = {"row": (1, 0), "column": (0, 1), "diagonal": (1, 1), "antidiagonal": (-1, 1)}


def hand_made(n):
    """name -> (board, verdict).  Coordinates fit 9 x 9 and 15 x 15."""
    assert n in (9, 15)
    from helpers import draw_sequence
    out = {}
    for name, (dx, dy) in DIRECTIONS.items():  # exact five in each of the four directions, for both colours
        x0 = 6 if dx < 0 else 1
        five = _line(n, x0, 1, dx, dy, 5)
        other = _scatter(n, five, 5)
        out[f"five_{name}_black"] = (_board(n, five, other[:4]), WON)   # 5 black, 4 white: Black just moved
        out[f"five_{name}_white"] = (_board(n, other, five), WON)       # 5 black, 5 white
    six = _line(n, 1, 2, 1, 0, 6)
    out["six_run"] = (_board(n, six, _scatter(n, six, 6)), LEGAL)        # an overline is no win (lib.rs:151-159)
    out["six_run_white"] = (_board(n, _scatter(n, six, 6), six), LEGAL)
    seq = draw_sequence(n)
    full = np.zeros(n * n, dtype=np.uint8)
    for i, c in enumerate(seq):
        full[c] = O.BLACK if i % 2 == 0 else O.WHITE
    out["full_board"] = (full, FULL)
    last = full.copy()
    last[seq[-1]] = O.EMPTY
    out["one_empty_cell"] = (last, LEGAL)
    out["white_ahead"] = (_board(n, [0], [2, 4]), BAD_COUNTS)
    out["black_two_ahead"] = (_board(n, [0, 2, 4], [6]), BAD_COUNTS)
    out["only_white"] = (_board(n, [], [n + 1]), BAD_COUNTS)
    bad = _board(n, [0], [2])
    bad[n * n - 1] = 3
    out["bad_byte"] = (bad, BAD_BYTE)
    bad = _board(n, _line(n, 1, 1, 1, 0, 5), [])  # a bad byte wins over counts and fives
    bad[40] = 255
    out["bad_byte_first"] = (bad, BAD_BYTE)
    out["counts_before_five"] = (_board(n, _line(n, 1, 1, 1, 0, 5), []), BAD_COUNTS)
    out["empty"] = (np.zeros(n * n, dtype=np.uint8), LEGAL)
    return out


def edge_positions(n):
    """stones in all four corners and on every edge: name -> board (verdicts come from `verdict`)"""
    e = n - 1
    corners = [0, e, e * n, e * n + e]
    out = {"corners": _board(n, corners[:2], corners[2:])}
    top, bottom = _line(n, 0, 0, 1, 0, n), _line(n, 0, e, 1, 0, n)
    left, right = _line(n, 0, 1, 0, 1, n - 2), _line(n, e, 1, 0, 1, n - 2)
    ring = top + right + bottom[::-1] + left[::-1]
    out["ring_pairs"] = _board(n, [c for i, c in enumerate(ring) if i % 4 < 2], [c for i, c in enumerate(ring) if i % 4 >= 2])  # runs of two
    out["edge_five_top"] = _board(n, _line(n, e - 4, 0, 1, 0, 5), _line(n, 0, e, 1, 0, 4))        # ends in the corner (e, 0)
    col = _line(n, e, e - 4, 0, 1, 5)
    out["edge_five_right"] = _board(n, _scatter(n, col, 5), col)                                  # White's column into the corner (e, e)
    out["corner_diagonal"] = _board(n, _line(n, 0, 0, 1, 1, 5), _line(n, e, 0, 0, 1, 4))          # from the corner (0, 0)
    out["corner_antidiagonal"] = _board(n, _line(n, e, 0, -1, 1, 5), _line(n, 0, 0, 0, 1, 4))     # from the corner (e, 0)
    out["edge_six_bottom"] = _board(n, _line(n, 0, e, 1, 0, 6), _line(n, 0, 0, 2, 0, 4) + [2 * n, 2 * n + 2])
    return out


def straddling_fives(n):
    """exact fives (and one six) whose cells lie on both sides of a bitboard word boundary: cells 63|64 and, at 15 x 15, 127|128, 191|192"""
    out = {}
    for hi in [64] + ([128, 192] if n == 15 else []):
        x, y = hi % n, hi // n
        # a row through cells hi - 1 | hi where both lie on one board row, else the column / diagonals through cell hi
        if x >= 1:
            x0 = min(max(x - 2, 0), n - 5)
            row = _line(n, x0, y, 1, 0, 5)
            assert hi - 1 in row and hi in row
            out[f"row_{hi}"] = _board(n, row, _scatter(n, row, 4))
            out[f"row_{hi}_white"] = _board(n, _scatter(n, row, 5), row)
            if x0 + 6 <= n:
                six = _line(n, x0, y, 1, 0, 6)
                out[f"six_{hi}"] = _board(n, six, _scatter(n, six, 6))
        col = _line(n, x, min(y - 2, n - 5), 0, 1, 5)  # cells below and above the boundary
        assert min(col) < hi <= max(col)
        out[f"column_{hi}"] = _board(n, col, _scatter(n, col, 4))
        if 2 <= x <= n - 3:
            d = _line(n, x - 2, y - 2, 1, 1, 5)
            out[f"diagonal_{hi}"] = _board(n, _scatter(n, d, 5), d)
            a = _line(n, x + 2, y - 2, -1, 1, 5)
            out[f"antidiagonal_{hi}"] = _board(n, a, _scatter(n, a, 4))
    return out


def decode_inputs(n, inputs):
    """Stone-byte boards of encoder.rs input rows [B][3 n n] (helpers.random_positions): channel 0 = the stones of the perspective side,
    whichever colour that is -- the colour with more stones is Black (equal counts: channel 0)."""
    hw = n * n
    x = np.asarray(inputs, dtype=np.float32).reshape(-1, 3 * hw)
    mine, theirs = x[:, 0:2 * hw:2] > 0.5, x[:, 1:2 * hw:2] > 0.5
    boards = np.zeros((len(x), hw), dtype=np.uint8)
    for i in range(len(x)):
        a, b = (mine[i], theirs[i]) if mine[i].sum() >= theirs[i].sum() else (theirs[i], mine[i])
        boards[i][a] = O.BLACK
        boards[i][b] = O.WHITE
    return boards


def quiet(n, games, stones, seed):
    """boards [games][HW]: `stones` <= 8 random stones each, Black and White alternating (at most four per colour: no run of five)"""
    assert 0 <= stones <= 8
    rng = np.random.default_rng([seed, n, games, stones])
    boards = np.zeros((games, n * n), dtype=np.uint8)
    for g in range(games):
        cells = rng.permutation(n * n)[:stones]
        boards[g][cells[0::2]] = O.BLACK
        boards[g][cells[1::2]] = O.WHITE
    return boards


def move_order(board):
    """an alternating move order that builds `board` (black = white or white + 1): Black's cells and White's in ascending order"""
    black, white = np.flatnonzero(board == O.BLACK), np.flatnonzero(board == O.WHITE)
    assert len(black) in (len(white), len(white) + 1)
    seq = []
    for i in range(len(black)):
        seq.append(int(black[i]))
        if i < len(white):
            seq.append(int(white[i]))
    return seq


def input_rows(n, boards):
    """the Player-mode input rows of the positions (encoder.rs:10-46) through the oracle's environment"""
    rows = []
    for b in boards:
        env = make_env(n, b, int(np.count_nonzero(b)) & 1)
        out = np.zeros(3 * n * n, dtype=np.float32)
        O.lib().orc_encode_nn_input(C.byref(env), O.MODE_PLAYER, out.ctypes.data_as(C.POINTER(C.c_float)))
        rows.append(out)
    return np.stack(rows)


def drive_to(osp, boards, rows, root_policy):
    """osp (oracle SelfPlay) from its ordinary reset to `boards` [G][HW] (equal stone counts >= 1) by external moves; rows [G][HW] = the
    raw policy rows of the final positions, fed to the last advance (the earlier ones get a uniform row: their nodes do not survive)."""
    games, hw = boards.shape
    orders = [move_order(b) for b in boards]
    s = len(orders[0])
    assert s >= 1 and all(len(o) == s for o in orders)
    osp.reset(root_policy)
    filler = np.full((games, hw), 1.0 / hw, dtype=np.float32)
    for i in range(s):
        osp.set_actions(np.array([o[i] for o in orders], dtype=np.int32))
        assert len(osp.mirror_generate()) == games
        osp.advance(rows if i == s - 1 else filler)
        assert osp.error == 0 and osp.alive_count == games
    assert osp.ply == s


def masked_renormalised(board, row):
    """ensure_action_exists' arithmetic in numpy float32 (agent.rs:166-171): occupied cells to 0, a sequential f32 sum in ascending
    order, and iff f32::EPSILON <= sum every element times 1.0f / sum"""
    p = np.asarray(row, dtype=np.float32).copy()
    p[np.asarray(board).reshape(-1) != 0] = np.float32(0.0)
    total = np.float32(0.0)
    for x in p:
        total = np.float32(total + x)
    if np.float32(np.finfo(np.float32).eps) <= total:
        p = (p * np.float32(np.float32(1.0) / total)).astype(np.float32)
    return p


def winning_cells(n, board):
    """the empty cells at which the side to move wins at once (place_stone -> its own win)"""
    turn = int(np.count_nonzero(board)) & 1
    env = make_env(n, board, turn)
    out = []
    for cell in np.flatnonzero(np.asarray(board) == O.EMPTY):
        e = O.Env.from_buffer_copy(env)
        if O.lib().orc_env_place_stone(C.byref(e), int(cell)) == (O.BLACK_WIN if turn == 0 else O.WHITE_WIN):
            out.append(int(cell))
    return out


def win_in_one(n=9):
    """(board, cell): a crowded 9 x 9 position with three empty cells, Black to move, and exactly one winning cell.  The five-free
    colouring of helpers.draw_sequence with row 0 rewritten to W _ B B B B W W B: Black at (1, 0) makes exactly five."""
    assert n == 9
    from helpers import draw_sequence
    seq = draw_sequence(n)
    board = np.zeros(n * n, dtype=np.uint8)
    for i, c in enumerate(seq):
        board[c] = O.BLACK if i % 2 == 0 else O.WHITE
    board[0], board[1], board[2], board[3] = O.WHITE, O.EMPTY, O.BLACK, O.BLACK
    for c in (8 * n + 8, 8 * n + 4):  # two of Black's far stones off the board: Black 39, White 39
        assert board[c] == O.BLACK
        board[c] = O.EMPTY
    assert verdict(n, board) == (LEGAL, n * n - 3) and winning_cells(n, board) == [1]
    return board, 1
