"""No-GPU pins of tests/scripted_opponent.py, the restatement of the reference's scripted players (src/trainer.rs:452-455,
508-534) that the GPU tests of the evaluation games compare the device kernel with: hand-made positions whose answer is
known from the rules of environment/src/lib.rs:104-190."""
import ctypes as C

import numpy as np
import pytest

import scripted_opponent as SO
from oracle import oracle as O


@pytest.mark.parametrize("n", [9, 15])
@pytest.mark.parametrize("turn", [0, 1])
def test_hand_made_positions(n, turn):
    pos = SO.hand_made(n)
    at = lambda x, y: y * n + x  # noqa: E731
    want = {"four": at(5, 2), "open_four": at(0, 2), "block_before_win": at(5, 1), "overline": -1, "quiet": -1}
    assert sorted(pos) == sorted(want)
    for name, (board, cell) in pos.items():
        assert cell == want[name]
        assert SO.forced_cell(SO.make_env(n, board, turn)) == cell, name


@pytest.mark.parametrize("n", [9, 15])
def test_the_four_is_a_win_for_its_owner_and_a_block_for_the_other(n):
    board, cell = SO.hand_made(n)["four"]
    for turn, status in ((0, O.BLACK_WIN), (1, O.IN_PROGRESS)):  # the four is Black's
        env = SO.make_env(n, board, turn)
        assert O.lib().orc_env_place_stone(C.byref(env), cell) == status


@pytest.mark.parametrize("n", [9, 15])
def test_block_at_a_lower_index_beats_a_win_at_a_higher_one(n):
    board, cell = SO.hand_made(n)["block_before_win"]
    env = SO.make_env(n, board, 0)  # Black to move: (5, 5) would win, the scan stops at White's completing cell (5, 1) before
    win = 5 * n + 5
    e = O.Env.from_buffer_copy(env)
    assert O.lib().orc_env_place_stone(C.byref(e), win) == O.BLACK_WIN
    assert SO.forced_cell(env) == cell == n + 5 < win


@pytest.mark.parametrize("n", [9, 15])
def test_six_in_a_row_is_not_terminal(n):
    board, cell = SO.hand_made(n)["overline"]
    env = SO.make_env(n, board, 0)
    e = O.Env.from_buffer_copy(env)
    assert O.lib().orc_env_place_stone(C.byref(e), 3 * n + 3) == O.IN_PROGRESS  # x = 0..5 on row 3
    assert cell == -1 and SO.forced_cell(env) == -1


@pytest.mark.parametrize("n", [9, 15])
def test_the_last_empty_cell_is_taken(n):
    board, cell = SO.last_cell_position(n)
    assert np.count_nonzero(board == 0) == 1 and board[cell] == 0
    for turn in (0, 1):
        assert SO.forced_cell(SO.make_env(n, board, turn)) == cell  # Draw is terminal


def _philox_by_hand(key, c0, c1, c2, c3):
    """Philox4x32-10 as oracle/rng.c states it"""
    k0, k1 = key & 0xFFFFFFFF, key >> 32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def test_fallback_is_the_rth_empty_cell_of_the_opponent_stream():
    n, seed, episode, ply, game_global, turn = 9, 17, 3, 6, 1000, 0
    board, none = SO.hand_made(n)["quiet"]
    env = SO.make_env(n, board, turn)
    key = O.stream_key(seed, episode)
    assert key == (seed + episode * 0x9E3779B97F4A7C15) % 2 ** 64
    out = (C.c_uint32 * 4)()
    O.lib().orc_philox(key, 0, ply, 2 * game_global + turn, 4, out)
    assert tuple(out) == _philox_by_hand(key, 0, ply, 2 * game_global + turn, 4)
    empties = [a for a in range(n * n) if board[a] == 0]
    assert len(empties) == 75
    want = empties[(int(out[0]) * 75) >> 32]
    assert SO.move(SO.OPP_NAIVE, env, key, ply, game_global) == (want, False)
    assert SO.move(SO.OPP_RANDOM, env, key, ply, game_global) == (want, False)
    # RANDOM ignores a forced cell, NAIVE takes it
    fboard, fcell = SO.hand_made(n)["four"]
    fenv = SO.make_env(n, fboard, turn)
    assert SO.move(SO.OPP_NAIVE, fenv, key, ply, game_global) == (fcell, True)
    cell, forced = SO.move(SO.OPP_RANDOM, fenv, key, ply, game_global)
    assert not forced and fboard[cell] == 0
    # the draw depends on the ply, the game and the side to move
    draws = {SO.fallback_cell(SO.make_env(n, board, t), key, p, g) for t in (0, 1) for p in range(6) for g in range(6)}
    assert len(draws) > 20


def test_kinds_and_rng_purpose_match_the_product():
    import os
    import re
    from omok_ai_amd import binding
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert (SO.OPP_RANDOM, SO.OPP_NAIVE) == (binding.OPP_RANDOM, binding.OPP_NAIVE)
    header = open(os.path.join(root, "include", "omok_mi355x.h")).read()
    assert re.search(r"#define OMOK_OPP_RANDOM 0\b", header) and re.search(r"#define OMOK_OPP_NAIVE +1\b", header)
    common = open(os.path.join(root, "omok-ai_amd", "csrc", "common.h")).read()
    assert re.search(r"RNG_OPPONENT = %d\b" % SO.RNG_OPPONENT, common)
