"""GPU tests (run with -m gpu) of omok_env_replay, the batched replay kernel: boards, status and played byte for byte against
tests/game_replay.py (the replay restated as a loop over the oracle's Environment.place_stone), at 9 x 9 and 15 x 15."""
import ctypes as C
import functools

import numpy as np
import pytest

import omok_ai_amd as oa
from omok_ai_amd import binding as B
from oracle import oracle as O
import game_replay as R
import helpers
import positions as P

pytestmark = pytest.mark.gpu

RANDOM_LENGTHS = lambda n: (0, 1, 63, 64, 65, n * n - 1)  # noqa: E731  (both sides of the 64-move chunk the kernel loads at a time)


@functools.lru_cache(maxsize=None)
def _engine(n):
    """an engine WITHOUT a net, one per board size: omok_env_replay needs none"""
    return oa.Engine(board_size=n, games=1, max_nodes=16, max_tables=8, max_batch_k=1)


@functools.lru_cache(maxsize=None)
def _cases(n):
    """(names, starts [B][HW], moves [B][stride], lengths [B]) with stride = the longest game + 3, and the helper's answers for upto = -1:
    computed once per board size and left unchanged"""
    hw = n * n
    rng = np.random.default_rng([16, n])
    empty = np.zeros(hw, dtype=np.uint8)
    cases = []
    seq = helpers.draw_sequence(n)
    cases.append(("draw", empty, seq))
    cases.append(("draw_and_one_more", empty, seq + [0]))
    cases.append(("black_wins", empty, [0, n, 1, n + 1, 2, n + 2, 3, n + 3, 4, n + 4, 40]))
    cases.append(("overline", empty, [0, n, 1, n + 1, 2, n + 2, 3, n + 3, 5, n + 5, 4]))
    cases.append(("occupied", empty, [0, 0, 1]))
    cases.append(("off_the_board", empty, [0, hw, 1]))
    cases.append(("padding_word", empty, [0, 0xFFFF, 1]))
    cases.append(("external_flag", empty, [0x100 | 7, 0x100 | 8]))
    if n == 9:
        board, _cell = P.win_in_one(9)
        for c in np.flatnonzero(board == O.EMPTY):
            cases.append((f"win_in_one_{int(c)}", board, [int(c)]))
    for name, (board, _v) in sorted(P.hand_made(n).items()):  # every hand-made board as a start, the rejected ones included
        free = [int(c) for c in np.flatnonzero(board == 0)]
        cases.append((f"start_{name}", board, free[:2] if free else [0]))
    for g, board in enumerate(P.quiet(n, 3, 7, 5)):  # seven stones: White to move
        free = rng.permutation(np.flatnonzero(board == 0))[:9]
        cases.append((f"quiet_{g}", board, [int(c) for c in free]))
    for name, board in sorted(P.straddling_fives(n).items()):  # a win across bitboard words, by each stone of the side that moved last
        last = O.BLACK if np.count_nonzero(board == O.BLACK) > np.count_nonzero(board == O.WHITE) else O.WHITE
        for c in np.flatnonzero(board == last):
            start = board.copy()
            start[c] = O.EMPTY
            cases.append((f"straddling_{name}_{int(c)}", start, [int(c)]))
    for length in RANDOM_LENGTHS(n):
        cases.append((f"random_{length}", empty, R.random_game(n, length, rng)))
    for i in range(max(48, 135 - len(cases))):  # with these: a batch of 130 games and more, lengths mixed in one call
        cases.append((f"filler_{i}", empty, R.random_game(n, int(rng.integers(0, hw)), rng)))
    stride = max(len(m) for _, _, m in cases) + 3
    names = [c[0] for c in cases]
    starts = np.stack([c[1] for c in cases])
    moves = np.full((len(cases), stride), 0xFFFF, dtype=np.uint16)
    lengths = np.array([len(c[2]) for c in cases], dtype=np.int32)
    for b, (_, _, m) in enumerate(cases):
        moves[b, :len(m)] = m
    want = R.replay_batch(n, starts, moves, lengths)
    for a in (starts, moves, lengths) + want:
        a.setflags(write=False)
    return names, starts, moves, lengths, want


def _same(names, got, want, tag):
    for what, g, w in zip(("played", "status", "board"), got[::-1], want[::-1]):
        bad = [names[b] for b in range(len(names)) if not np.array_equal(g[b], w[b])]
        print(f"{tag}: {what}: {len(bad)} of {len(names)} games differ {bad[:5]}")
        assert not bad, (tag, what, bad[:5])
        assert g.dtype == w.dtype and g.shape == w.shape


@pytest.mark.parametrize("n", [9, 15])
def test_the_helper_answers_what_the_cases_are_there_for(n):
    """conditions on the inputs, from the helper alone"""
    names, starts, moves, lengths, (boards, status, played) = _cases(n)
    at = {name: b for b, name in enumerate(names)}
    assert len(names) >= 130 and moves.shape[1] > lengths.max()
    assert (status[at["draw"]], played[at["draw"]]) == (O.DRAW, n * n) == (status[at["draw_and_one_more"]], played[at["draw_and_one_more"]])
    assert (status[at["black_wins"]], played[at["black_wins"]]) == (O.BLACK_WIN, 9)
    assert (status[at["overline"]], played[at["overline"]]) == (O.IN_PROGRESS, 11)
    assert played[at["occupied"]] == played[at["off_the_board"]] == played[at["padding_word"]] == 1
    assert played[at["external_flag"]] == 2
    for name, (board, v) in P.hand_made(n).items():
        b = at["start_" + name]
        if v:
            assert (status[b], played[b]) == (-1, -v) and np.array_equal(boards[b], board), name
        else:
            assert played[b] == min(2, n * n - np.count_nonzero(board)), name
    straddling = [b for b, name in enumerate(names) if name.startswith("straddling_") and "_six_" not in name]
    assert len(straddling) >= (15 if n == 9 else 45)
    assert all(status[b] in (O.BLACK_WIN, O.WHITE_WIN) and played[b] == 1 for b in straddling)
    for length in RANDOM_LENGTHS(n):
        assert (status[at[f"random_{length}"]], played[at[f"random_{length}"]]) == (O.IN_PROGRESS, length)
    assert all(np.count_nonzero(starts[at[f"quiet_{g}"]]) == 7 and played[at[f"quiet_{g}"]] == 9 for g in range(3))
    assert len(set(int(x) for x in lengths)) > 20


@pytest.mark.parametrize("n", [9, 15])
def test_replay_of_the_whole_batch(n):
    names, starts, moves, lengths, want = _cases(n)
    _same(names, _engine(n).env_replay(starts, moves, lengths), want, f"board {n}")


@pytest.mark.parametrize("n", [9, 15])
@pytest.mark.parametrize("upto", [0, 8, 64, 100000])
def test_upto(n, upto):
    names, starts, moves, lengths, _ = _cases(n)
    want = R.replay_batch(n, starts, moves, lengths, upto)
    _same(names, _engine(n).env_replay(starts, moves, lengths, upto=upto), want, f"board {n} upto {upto}")
    if upto == 0:
        assert np.array_equal(want[0], starts) and not want[2][want[2] > 0].any()


@pytest.mark.parametrize("n", [9, 15])
def test_batch_of_one_and_other_strides(n):
    names, starts, moves, lengths, want = _cases(n)
    eng = _engine(n)
    for name in ("draw", "black_wins", "occupied", "random_64", "random_65", "start_full_board", "start_bad_byte"):
        b = names.index(name)
        got = eng.env_replay(starts[b:b + 1], moves[b:b + 1], lengths[b:b + 1])
        _same([name], got, tuple(w[b:b + 1] for w in want), f"board {n} alone")
        length = int(lengths[b])
        if length >= 1:  # stride = the length exactly
            got = eng.env_replay(starts[b:b + 1], moves[b:b + 1, :length], lengths[b:b + 1])
            _same([name], got, tuple(w[b:b + 1] for w in want), f"board {n} alone, stride {length}")


@pytest.mark.parametrize("n", [9, 15])
def test_no_start_boards_is_the_empty_board(n):
    names, starts, moves, lengths, want = _cases(n)
    keep = np.flatnonzero(~starts.any(axis=1))
    assert len(keep) >= 60
    got = _engine(n).env_replay(None, moves[keep], lengths[keep])
    _same([names[b] for b in keep], got, tuple(w[keep] for w in want), f"board {n} without start boards")


@pytest.mark.parametrize("n", [9, 15])
def test_every_output_may_be_null(n):
    names, starts, moves, lengths, want = _cases(n)
    eng, batch = _engine(n), len(names)
    u8, i32, u16 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_uint16)
    s, m, ln = np.array(starts), np.array(moves), np.array(lengths)
    for skip in range(4):  # 3: all three
        boards = np.full((batch, n * n), 9, dtype=np.uint8)
        status = np.full(batch, 9, dtype=np.int32)
        played = np.full(batch, 9, dtype=np.int32)
        outs = [boards.ctypes.data_as(u8), status.ctypes.data_as(i32), played.ctypes.data_as(i32)]
        for i in range(3):
            if skip in (i, 3):
                outs[i] = None
        rc = B.lib().omok_env_replay(eng.h, s.ctypes.data_as(u8), m.ctypes.data_as(u16), ln.ctypes.data_as(i32), batch, m.shape[1], -1, *outs)
        assert rc == 0
        for i, (g, w) in enumerate(zip((boards, status, played), want)):
            if skip in (i, 3):
                assert np.all(g == 9)  # untouched
            else:
                assert np.array_equal(g, w)


def test_argument_errors():
    eng = _engine(9)
    moves = np.zeros((2, 4), dtype=np.uint16)
    for lengths in ([5, 0], [0, -1]):  # outside [0, stride]
        with pytest.raises(B.OmokError) as ei:
            eng.env_replay(None, moves, lengths)
        assert ei.value.code == -1
    u8, i32, u16 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_uint16)
    ln = np.zeros(2, dtype=np.int32)
    for batch, stride in ((0, 4), (2, 0)):
        assert B.lib().omok_env_replay(eng.h, None, moves.ctypes.data_as(u16), ln.ctypes.data_as(i32), batch, stride, -1, None, None, None) == -1
    assert B.lib().omok_env_replay(eng.h, None, None, ln.ctypes.data_as(i32), 2, 4, -1, None, None, None) == -1
    assert B.lib().omok_env_replay(eng.h, None, moves.ctypes.data_as(u16), None, 2, 4, -1, None, None, None) == -1
