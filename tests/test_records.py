"""omok_ai_amd.records without a GPU: the .npz round trip, the text form of a hand-made record, the metadata, and verify / position_at
against a stand-in engine whose env_replay is tests/game_replay.py (the oracle's place_stone)."""
import numpy as np
import pytest

from omok_ai_amd import records as R
import game_replay as GR
import positions as P


class FakeEngine:
    """what records.py needs of an Engine: the board size and env_replay, here the oracle-side restatement"""

    def __init__(self, n):
        self.n, self.hw = n, n * n

    def env_replay(self, start_boards, moves, lengths, upto=-1):
        return GR.replay_batch(self.n, start_boards, np.asarray(moves), np.asarray(lengths), upto)


def _hand_made(n=9):
    """three games: a Black win in 9 moves from the empty board (White's moves external), an unfinished game of 3 moves from a start
    position of 2 stones, and a game without a move"""
    hw = n * n
    win = [0, n, 1, n + 1, 2, n + 2, 3, n + 3, 4]
    moves = np.full((3, hw), 0xFFFF, dtype=np.uint16)
    moves[0, :9] = [c | (0x100 if i % 2 else 0) for i, c in enumerate(win)]
    moves[1, :3] = [40, 41, 42]
    start = np.zeros((3, hw), dtype=np.uint8)
    start[1, [10, 20]] = [1, 2]
    lengths = np.array([9, 3, 0], dtype=np.int32)
    root_n, child_n = np.zeros((3, hw), dtype=np.uint32), np.zeros((3, hw), dtype=np.uint32)
    root_w, child_w = np.zeros((3, hw), dtype=np.float32), np.zeros((3, hw), dtype=np.float32)
    root_n[0, 0:9:2], child_n[0, 0:9:2] = 32, [8, 9, 10, 11, 12]
    root_w[0, 0:9:2], child_w[0, 0:9:2] = -3.5, [2.0, 2.25, 5.0, 5.5, 12.0]
    root_n[1, :3], child_n[1, :3], child_w[1, :3] = 16, 4, [-1.0, 0.5, np.float32(0.1)]
    return R.GameRecords.from_log(n, start, lengths, moves, root_n, root_w, child_n, child_w, status=[2, 0, 0], plies=[9, 5, 0],
                                  meta={"net1": "a.bin", "net2": "b.bin", "split": 1, "sims": 32, "seed": 3, "openings": None,
                                        "paired": {"both": 0, "one_each": 1, "neither": 0, "drawn_pairs": 0}})


def test_from_log_splits_the_move_word():
    rec = _hand_made()
    assert rec.cells.dtype == np.int16 and rec.external.dtype == bool
    assert list(rec.cells[0, :10]) == [0, 9, 1, 10, 2, 11, 3, 12, 4, -1]
    assert list(rec.external[0, :10]) == [False, True] * 4 + [False, False]
    assert np.all(rec.cells[2] == -1) and not rec.external[2].any()
    assert rec.moves().dtype == np.uint16 and rec.moves()[0, 1] == 0x109 and rec.moves()[0, 9] == 0xFFFF


def test_npz_round_trip(tmp_path):
    rec = _hand_made()
    path = tmp_path / "games.npz"
    rec.save(path)
    back = R.load(path)
    assert back == rec
    for name in R._ARRAYS:
        a, b = getattr(rec, name), getattr(back, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    assert back.meta == rec.meta and back.meta["paired"]["one_each"] == 1 and back.meta["openings"] is None  # paired-style metadata survives
    assert back.n == 9 and back.games == 3
    back.child_w[1, 2] = np.float32(0.2)
    assert back != rec


def test_to_text_of_a_hand_made_record():
    rec = _hand_made()
    text = rec.to_text(0).splitlines()
    assert text[0] == "game 0: 9 x 9, 0 stones at the start, 9 moves, black wins"
    assert text[1].split() == list("abcdefghi")
    assert text[2].split() == ["1", "1", "3", "5", "7", "9", ".", ".", ".", "."]   # row 1: Black's five, by move number
    assert text[3].split() == ["2", "2", "4", "6", "8", ".", ".", ".", ".", "."]
    rows = [line.split() for line in text[12:]]
    assert len(rows) == 9
    assert rows[0] == ["1", "0", "black", "a1", "32", "8", "+0.2500"]
    assert rows[1] == ["2", "1", "white", "a2", "ext", "0", "0", "-"]             # an external move: nothing was known of it
    assert rows[8] == ["9", "8", "black", "e1", "32", "12", "+1.0000"]
    text = rec.to_text(1).splitlines()
    assert text[0] == "game 1: 9 x 9, 2 stones at the start, 3 moves, in progress"
    assert text[3].split() == ["2", ".", "X", ".", ".", ".", ".", ".", ".", "."]   # cell 10 = b2: a start stone of Black
    assert text[4].split()[3] == "O"                                                # cell 20 = c3: a start stone of White
    assert text[6].split()[5:8] == ["1", "2", "3"]                                  # cells 40, 41, 42 = e5, f5, g5
    assert [line.split()[:4] for line in text[12:]] == [["1", "2", "black", "e5"], ["2", "3", "white", "f5"], ["3", "4", "black", "g5"]]
    assert text[12].split()[-1] == "-0.2500"
    assert len(rec.to_text(2).splitlines()) == 12                                    # a game without a move: the board and the header


def test_main_show(tmp_path, capsys):
    rec = _hand_made()
    path = tmp_path / "games.npz"
    rec.save(path)
    assert R.main(["show", str(path), "--game", "1"]) == 0
    out = capsys.readouterr().out
    assert out.splitlines()[0].startswith("meta: {") and '"net1": "a.bin"' in out
    assert rec.to_text(1) in out
    with pytest.raises(SystemExit):
        R.main(["show", str(path), "--game", "3"])


def test_verify_and_position_at_through_the_replay():
    rec = _hand_made()
    eng = FakeEngine(9)
    finals = rec.verify(eng)
    assert np.count_nonzero(finals[0]) == 9 and np.count_nonzero(finals[1]) == 5 and not finals[2].any()
    assert np.array_equal(rec.position_at(1, 0, eng), rec.start_boards[1])
    at2 = rec.position_at(1, 2, eng)
    assert at2[40] == 1 and at2[41] == 2 and at2[42] == 0 and at2[10] == 1 and at2[20] == 2
    assert np.array_equal(rec.position_at(0, 9, eng), finals[0])


@pytest.mark.parametrize("damage", ["status", "occupied", "length", "plies", "after_the_end"])
def test_verify_catches_a_record_that_does_not_replay(damage):
    rec = _hand_made()
    if damage == "status":
        rec.status[0] = 3
    elif damage == "occupied":
        rec.cells[1, 2] = 40
    elif damage == "length":
        rec.lengths[1] = 2
    elif damage == "plies":
        rec.plies[1] = 6
    else:  # a move recorded after the winning one
        rec.lengths[0], rec.cells[0, 9], rec.plies[0] = 10, 50, 10
    with pytest.raises(AssertionError):
        rec.verify(FakeEngine(9))


def test_verify_on_a_won_start_board():
    n = 9
    board, v = P.hand_made(n)["five_row_black"]
    assert v == P.WON
    hw = n * n
    z32, zf = np.zeros((1, hw), dtype=np.uint32), np.zeros((1, hw), dtype=np.float32)
    rec = R.GameRecords.from_log(n, board[None], [0], np.full((1, hw), 0xFFFF, dtype=np.uint16), z32, zf, z32, zf, status=[0], plies=[9])
    with pytest.raises(AssertionError):
        rec.verify(FakeEngine(n))
