"""Random openings (omok_env_random_positions), restated through the oracle library (a helper of tests/test_match_positions_yardstick.py
and tests/test_gpu_match_positions.py; not a test, no product code).

Position b is the board after `stones` plies of the game with global id first_game + b in which both sides are the RANDOM scripted player:
a loop over scripted_opponent.move(OPP_RANDOM, ...) -- ply i draws with (key, ply i, game id, side to move = i & 1) -- and
orc_env_place_stone.  A placement whose status is not InProgress stops the game: ok = 0, the board holds the stones up to that one.
"""
import ctypes as C

import numpy as np

from oracle import oracle as O
import scripted_opponent as SO

_GAMES = {}  # (n, key, game id) -> [cells played so far, the game is over, its environment]


def game(n, key, game_id, stones):
    """(cells, over): the first min(stones, length) moves of the game and whether a placement among them ended it"""
    assert 0 <= stones < n * n
    rec = _GAMES.setdefault((n, int(key), int(game_id)), [[], False, SO.make_env(n, np.zeros(n * n, dtype=np.uint8), O.TURN_BLACK)])
    cells, _over, env = rec
    while len(cells) < stones and not rec[1]:
        i = len(cells)
        assert env.turn == (i & 1)
        cell, forced = SO.move(SO.OPP_RANDOM, env, key, i, game_id)
        assert not forced
        status = O.lib().orc_env_place_stone(C.byref(env), int(cell))
        assert status >= 0
        cells.append(int(cell))
        rec[1] = status != O.IN_PROGRESS
    over = rec[1] and len(cells) <= stones
    return cells[:stones], over


def positions(n, key, first_game, stones, batch):
    """(boards uint8 [batch][HW], ok uint8 [batch]) as omok_env_random_positions returns them"""
    boards = np.zeros((batch, n * n), dtype=np.uint8)
    ok = np.zeros(batch, dtype=np.uint8)
    for b in range(batch):
        cells, over = game(n, key, first_game + b, stones)
        boards[b][cells[0::2]] = O.BLACK
        boards[b][cells[1::2]] = O.WHITE
        ok[b] = 0 if over else 1
    return boards, ok
