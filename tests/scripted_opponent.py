"""The scripted players of the reference's evaluation games, restated literally through the oracle library (a helper of
tests/test_scripted_opponent.py, tests/test_gpu_versus.py; not a test, no product code).

  forced_cell   the loop of play_against_naive_player (src/trainer.rs:508-534): for every empty cell in ascending order,
                `env.clone().place_stone(action).is_terminal()`, then the same on a clone whose `turn` is flipped; the first
                cell that passes either test is taken (`break`).  -1 where the reference falls through to its random pick.
  fallback_cell `legal_moves[rng.gen_range(0..legal_moves.len())]` (:534, :452-455) under the build-defined RNG contract
                (oracle/rng.c): r = mulhi(x0, len), x0 = word 0 of Philox(key, 0, ply, 2 * game_global + side to move, 4).
"""
import ctypes as C

import numpy as np

from oracle import oracle as O

OPP_RANDOM, OPP_NAIVE = 0, 1
RNG_OPPONENT = 4


def make_env(n, board, turn):
    """oracle Env structure from Stone bytes, the side to move and the empty count"""
    board = np.asarray(board, dtype=np.uint8).reshape(-1)
    assert board.size == n * n
    env = O.Env()
    O.lib().orc_env_init(C.byref(env), n)
    env.turn = int(turn)
    env.legal = int(np.count_nonzero(board == O.EMPTY))
    for i, s in enumerate(board):
        env.board[i] = int(s)
    return env


def _is_terminal(env, action, flip):
    e = O.Env.from_buffer_copy(env)  # env.clone()
    if flip:
        e.turn = 1 - e.turn  # env.turn = env.turn.opponent()
    status = O.lib().orc_env_place_stone(C.byref(e), int(action))
    assert status >= 0  # .unwrap(): the cell is empty
    return status != O.IN_PROGRESS  # GameStatus::is_terminal()


def forced_cell(env):
    hw = env.n * env.n
    for action in [a for a in range(hw) if env.board[a] == O.EMPTY]:
        if _is_terminal(env, action, False):
            return action
        if _is_terminal(env, action, True):
            return action
    return -1


def fallback_cell(env, key, ply, game_global):
    hw = env.n * env.n
    legal_moves = [a for a in range(hw) if env.board[a] == O.EMPTY]
    out = (C.c_uint32 * 4)()
    O.lib().orc_philox(int(key), 0, int(ply), (2 * int(game_global) + int(env.turn)) & 0xFFFFFFFF, RNG_OPPONENT, out)
    return legal_moves[(int(out[0]) * len(legal_moves)) >> 32]


def move(kind, env, key, ply, game_global):
    """(cell, forced?) of the scripted player `kind` on `env`; key = oracle.stream_key(seed, episode)"""
    cell = forced_cell(env) if kind == OPP_NAIVE else -1
    if cell >= 0:
        return cell, True
    return fallback_cell(env, key, ply, game_global), False


# ---- hand-made positions (coordinates fit 9 x 9 and 15 x 15): name -> (board, the forced cell or -1) -------------------
def _board(n, black, white):
    b = np.zeros(n * n, dtype=np.uint8)
    for c in black:
        assert b[c] == 0
        b[c] = O.BLACK
    for c in white:
        assert b[c] == 0
        b[c] = O.WHITE
    return b


def hand_made(n):
    """Every position has its forced cell (or none) for EITHER side to move: the rule tries a stone of both colours."""
    assert n in (9, 15)
    at = lambda x, y: y * n + x  # noqa: E731
    scattered = [at(0, 7), at(3, 7), at(6, 7), at(8, 8)]  # quiet stones of the other colour, no two adjacent
    out = {}
    # a four on row 2, x = 1..4, closed at x = 0 by the other colour: the one completing cell is (5, 2) -- a win for the side
    # that owns the four, a block for the other
    out["four"] = (_board(n, [at(x, 2) for x in range(1, 5)], [at(0, 2)] + scattered[1:]), at(5, 2))
    # the same four open at both ends: the lower completing cell
    out["open_four"] = (_board(n, [at(x, 2) for x in range(1, 5)], scattered), at(0, 2))
    # White's four on row 1 (block / win at (5, 1)) above Black's four on row 5 (win / block at (5, 5)): the lower index is
    # taken whoever moves -- for Black a block although a win exists
    out["block_before_win"] = (_board(n, [at(x, 5) for x in range(1, 5)] + [at(0, 1)], [at(x, 1) for x in range(1, 5)] + [at(0, 5)]), at(5, 1))
    # x = 0, 1, 2 and 4, 5 on row 3: a stone at (3, 3) makes six in a row -- no exact five, not terminal; nothing else is forced
    out["overline"] = (_board(n, [at(x, 3) for x in (0, 1, 2, 4, 5)], scattered + [at(3, 0)]), -1)
    # a few stones far apart
    out["quiet"] = (_board(n, [at(1, 1), at(4, 4), at(7, 2)], [at(2, 5), at(6, 6), at(8, 0)]), -1)
    return out


def last_cell_position(n):
    """(board with ONE empty cell and no exact five, that cell): place_stone there returns Draw (environment/src/lib.rs:160-161)"""
    from helpers import draw_sequence
    seq = draw_sequence(n)
    board = np.zeros(n * n, dtype=np.uint8)
    for i, c in enumerate(seq[:-1]):
        board[c] = O.BLACK if i % 2 == 0 else O.WHITE
    return board, seq[-1]
