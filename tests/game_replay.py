"""omok_env_replay restated as a loop over the oracle's Environment.place_stone (a helper of tests/test_game_replay_yardstick.py,
tests/test_records.py and the GPU tests of the game records; not a test, no product code).

  replay        one record: from a start board (None: Environment::new()) the moves moves[: min(length, upto)] (cell = word & 0xFF) by
                place_stone (environment/src/lib.rs:104-166) on an env made by scripted_opponent.make_env, side to move = stones & 1;
                stops in front of the first illegal move (cell >= HW, or occupied: place_stone returns None) and after a move that ends
                the game.  A start board whose positions.verdict v is not 0: played = -v, status = -1, the bytes unchanged.
  replay_batch  the same over a batch, in the array shapes of omok_env_replay.
  random_game   a legal game of a given length that nobody has won (random orders of a five-free colouring), for the chunk-boundary cases.
"""
import ctypes as C

import numpy as np

from oracle import oracle as O
import positions as P
from scripted_opponent import make_env


def replay(n, start, moves, length, upto=-1):
    """(board uint8 [HW], status, played)"""
    hw = n * n
    start = np.zeros(hw, dtype=np.uint8) if start is None else np.asarray(start, dtype=np.uint8).reshape(hw)
    v, stones = P.verdict(n, start)
    if v != 0:
        return start.copy(), -1, -v
    env = make_env(n, start, stones & 1)
    length = int(length) if upto < 0 else min(int(length), int(upto))
    status, played = O.IN_PROGRESS, 0
    for word in list(moves)[:length]:
        cell = int(word) & 0xFF
        if cell >= hw:
            break
        s = _place(env, cell)
        if s is None:
            break
        status, played = s, played + 1
        if s != O.IN_PROGRESS:
            break
    return np.array(env.board[:hw], dtype=np.uint8), status, played


def _place(env, cell):
    s = O.lib().orc_env_place_stone(C.byref(env), int(cell))
    return None if s < 0 else s


def replay_batch(n, starts, moves, lengths, upto=-1):
    """starts [B][HW] or None, moves [B][stride], lengths [B] -> (boards uint8 [B][HW], status int32 [B], played int32 [B])"""
    out = [replay(n, None if starts is None else starts[b], moves[b], lengths[b], upto) for b in range(len(lengths))]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int32), np.array([o[2] for o in out], dtype=np.int32))


def random_game(n, length, rng):
    """`length` <= HW - 1 distinct cells, Black first, after which the game is still in progress: the five-free colouring of
    helpers.draw_sequence (every line has runs of at most four of a colour, so no subset of it holds a five) with the cells of each colour
    in a random order"""
    from helpers import draw_sequence
    hw = n * n
    assert 0 <= length < hw
    seq = draw_sequence(n)
    black, white = rng.permutation(seq[0::2]), rng.permutation(seq[1::2])
    out = []
    for i in range(length):
        out.append(int(black[i // 2] if i % 2 == 0 else white[i // 2]))
    return out
