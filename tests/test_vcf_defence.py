"""No-GPU tests that pin the yardstick of the defender's half of the forced-win solver (tests/vcf_defence.py: omok_env_vcf_defend's rule
in plain Python) by hand, assert the conditions tests/test_gpu_vcf_defence.py relies on, and test records.GameRecords.vcf_defence -- host
code over three engine calls -- on hand-made records through a stand-in engine backed by the yardsticks.

CPU cost measured when this file was written (one core): set_a at (8, 4096) 15 s / 16 s at 9 x 9 / 15 x 15, set_b at (8, 8) 4 s / 10 s,
set_b at (2, 4096) 1 s / 3 s; each is computed once per process (vcf_defence.want)."""
import numpy as np
import pytest

import game_replay as GR
import scripted_opponent as SO
import vcf_defence as VD
import vcf_solver as VS
from omok_ai_amd import records as R

SIZES = [9, 15]
OCCUPIED, SAFE, WINS, LOSES, UNKNOWN = VD.OCCUPIED, VD.SAFE, VD.WINS, VD.LOSES, VD.UNKNOWN


def _cells(m, status):
    return [a for a, s in enumerate(m.status) if s == status]


# ---- the rule, read by hand ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_open_three_with_the_other_side_to_move(n, side):
    at = lambda x, y: y * n + x  # noqa: E731
    x0 = VS._x0(n, 4)
    board = VS.hand_made(n)[f"open_three_s{side}_r4"][0]  # `side` holds _XXX_ at x0 .. x0 + 2 on row 4; the other side has no stone
    m = VD.defend(n, board, 1 - side, 8, 4096)
    assert m.threat == (1, 2, at(x0 - 1, 4))
    # only the two cells next to the three hold: the four that is left is closed and leads nowhere.  A stone two cells off leaves the open
    # four at the far end, every other stone leaves both
    assert _cells(m, SAFE) == [at(x0 - 1, 4), at(x0 + 3, 4)] and not _cells(m, WINS) and not _cells(m, UNKNOWN)
    assert _cells(m, OCCUPIED) == [at(x0 + i, 4) for i in range(3)]
    for a in _cells(m, LOSES):  # a win in two found at the root of depth 2: one node per depth
        assert (m.moves[a], m.nodes[a], m.reply[a]) == (2, 2, at(x0 + 3, 4) if a == at(x0 - 2, 4) else at(x0 - 1, 4)), a
    assert all(m.moves[a] == 0 and m.reply[a] == -1 and m.nodes[a] > 8 for a in _cells(m, SAFE))
    assert all(m.moves[a] == 0 and m.reply[a] == -1 and m.nodes[a] == 0 for a in _cells(m, OCCUPIED))


@pytest.mark.parametrize("n", SIZES)
def test_a_four_of_the_movers_own_postpones_or_holds_as_the_rule_gives_it(n):
    at = lambda x, y: y * n + x  # noqa: E731
    x0 = VS._x0(n, 4)
    three = [at(x0 + i, 4) for i in range(3)]
    # White holds the column (x0 + 3, 5..7), closed below (the edge at 9 x 9, a black stone at 15 x 15).  Its four at (x0 + 3, 8) leaves the
    # one completing cell (x0 + 3, 4): Black must take it, and there it makes the open four: the four only postpones -- LOSES in two, by the
    # solver's |Fo| == 1 branch.  The four at (x0 + 3, 4) itself takes the three's end and leaves two completing cells: Black has two fives
    # against it and no win
    column = [at(x0 + 3, y) for y in (5, 6, 7)]
    board = SO._board(n, three + ([at(x0 + 3, 9)] if n == 15 else []), column)
    m = VD.defend(n, board, 1, 8, 4096)
    assert m.threat == (1, 2, at(x0 - 1, 4))
    a = at(x0 + 3, 8)
    assert (m.status[a], m.moves[a], m.nodes[a], m.reply[a]) == (LOSES, 2, 2, at(x0 + 3, 4))
    assert m.status[at(x0 + 3, 4)] == SAFE and m.status[at(x0 - 1, 4)] == SAFE
    # an edge three of White's on the bottom row instead: its four (3, n - 1) forces Black to (4, n - 1), which is no four of Black's: SAFE,
    # though the open three still stands (the mover is to move again after the forced reply: the map answers for the solver's rule); the
    # split four (4, n - 1) likewise, with Black forced to (3, n - 1)
    board = SO._board(n, three, [at(x, n - 1) for x in range(3)])
    m = VD.defend(n, board, 1, 8, 4096)
    assert m.threat == (1, 2, at(x0 - 1, 4)) and m.status[at(3, n - 1)] == SAFE and m.nodes[at(3, n - 1)] == 8
    assert _cells(m, SAFE) == sorted([at(x0 - 1, 4), at(x0 + 3, 4), at(3, n - 1), at(4, n - 1)])


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_chain_m3_with_the_other_side_to_move(n, side):
    at = lambda x, y: y * n + x  # noqa: E731
    x0 = VS._x0(n, 4)
    board = VS.hand_made(n)[f"chain_m3_s{side}"][0]
    m = VD.defend(n, board, 1 - side, 3, 4096)
    assert m.threat == (1, 3, at(x0 + 3, 4))
    # the cell where the two lines meet, the forced reply's cell (the row is then closed at both ends), and the two cells next to the column's
    # three-to-be (one completing cell is left to its four); a stone one further off leaves the open four on the other side
    assert _cells(m, SAFE) == sorted([at(x0 + 3, 4), at(x0 + 4, 4), at(x0 + 3, 1), at(x0 + 3, 5)])
    assert not _cells(m, WINS) and not _cells(m, UNKNOWN)
    assert all(m.moves[a] == 3 and m.reply[a] == at(x0 + 3, 4) for a in _cells(m, LOSES))
    assert m.status[at(x0 + 3, 0)] == LOSES and m.status[at(x0 + 3, 6)] == LOSES
    m = VD.defend(n, board, 1 - side, 2, 4096)  # at depth 2 there is no threat, and no stone of the mover's makes one
    assert m.threat == (0, 0, -1) and not _cells(m, LOSES) and len(_cells(m, SAFE)) == n * n - 6
    assert all(m.nodes[a] == 2 for a in _cells(m, SAFE))


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_last_cell_and_full_board(n, side):
    last, cell = SO.last_cell_position(n)
    m = VD.defend(n, last, side, 8, 4096)  # on the full board the solver counts one node per depth
    assert _cells(m, SAFE) == [cell] and len(_cells(m, OCCUPIED)) == n * n - 1
    assert (m.moves[cell], m.nodes[cell], m.reply[cell]) == (0, 8, -1) and m.threat == (0, 0, -1)
    m = VD.defend(n, last, side, 8, 7)
    assert _cells(m, UNKNOWN) == [cell] and (m.moves[cell], m.nodes[cell], m.reply[cell]) == (0, 7, -1)
    full = VS.hand_made(n)[f"full_board_s{side}"][0]
    m = VD.defend(n, full, side, 8, 4096)
    assert m.status == [OCCUPIED] * (n * n) and m.threat == (0, 0, -1) and not any(m.nodes) and set(m.reply) == {-1}


def non_monotone_position(n):
    """(board, side to move 1, the cells WINS, LOSES, the reply): White holds the four x0 .. x0 + 3 on row 4, closed by a black stone at
    x0 - 1: its five at x0 + 4 is the one cell Black would have to take, and that is no four of Black's: Black's open three on row 8 wins
    nothing while it stands.  White's own stone at x0 + 5 turns that five into a six: the counter-threat is gone and the three wins in two."""
    at = lambda x, y: y * n + x  # noqa: E731
    x0, x8 = VS._x0(n, 4), VS._x0(n, 8)
    board = SO._board(n, [at(x0 - 1, 4)] + [at(x8 + i, 8) for i in range(3)], [at(x0 + i, 4) for i in range(4)])
    return board, at(x0 + 4, 4), at(x0 + 5, 4), at(x8 - 1, 8)


@pytest.mark.parametrize("n", SIZES)
def test_the_map_is_not_monotone(n):
    board, wins, loses, reply = non_monotone_position(n)
    m = VD.defend(n, board, 1, 8, 4096)
    assert m.threat == (0, 0, -1)  # passing is safe ...
    assert _cells(m, WINS) == [wins] and _cells(m, LOSES) == [loses]  # ... and one stone of the mover's own loses
    assert (m.moves[loses], m.nodes[loses], m.reply[loses]) == (2, 2, reply)
    assert (m.moves[wins], m.nodes[wins], m.reply[wins]) == (0, 0, -1)
    assert len(_cells(m, SAFE)) == n * n - 8 - 2


# ---- the conditions the GPU tests rely on ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_set_sizes(n):
    assert len(VD.set_a(n)[0]) == {9: 89, 15: 76}[n] and len(VD.set_b(n)[0]) == {9: 71, 15: 66}[n]
    assert len(VD.hand_set(n)[1]) == len(VS.hand_made(n))


def _both(w):
    return (w["status"] == SAFE).any(axis=1) & (w["status"] == LOSES).any(axis=1)


@pytest.mark.parametrize("n", SIZES)
def test_set_a_covers_every_status_and_the_non_monotone_case(n):
    w = VD.want("a", n, 8, 4096)
    st, threat = w["status"], w["threat"]
    print(f"board {n}: {len(st)} positions, cells by status {[int((st == v).sum()) for v in range(5)]}, nodes {int(w['nodes'].sum())}")
    assert all((st == v).any() for v in (OCCUPIED, SAFE, WINS, LOSES)) and not (st == UNKNOWN).any() and not (threat[:, 0] < 0).any()
    assert np.count_nonzero((threat[:, 0] == 1) & _both(w)) >= 8
    assert np.count_nonzero((threat[:, 0] == 0) & (st == LOSES).any(axis=1)) == {9: 2, 15: 1}[n]
    for k, v in VD.counts(st).items():
        assert np.array_equal(w[k], v)
    assert np.array_equal(w["safe"] + w["wins"] + w["loses"] + w["unknown"], np.count_nonzero(st, axis=1))


@pytest.mark.parametrize("n", SIZES)
def test_set_b_runs_out_of_budget_and_has_shallow_threats(n):
    w = VD.want("b", n, 8, 8)
    assert np.count_nonzero(w["status"] == UNKNOWN) == {9: 470, 15: 647}[n] and np.count_nonzero(w["threat"][:, 0] < 0) >= 3
    assert np.all(w["nodes"][w["status"] == UNKNOWN] == 8) and w["nodes"].max() == 8
    w = VD.want("b", n, 2, 4096)
    assert np.count_nonzero((w["threat"][:, 0] == 1) & _both(w)) >= 7 and not (w["status"] == UNKNOWN).any()


# ---- the report on hand-made records, through a stand-in engine ------------------------------------------------------------------------
N, HW = 9, 81
R_BLACK_WIN, R_WHITE_WIN = 2, 3


class StandIn:
    n = N

    def env_replay(self, start, moves, lengths, upto=-1):
        return GR.replay_batch(self.n, start, moves, lengths, upto)

    def env_vcf_solve(self, boards, turns, max_depth=8, max_nodes=4096):
        return VS.solve_batch(self.n, boards, turns, max_depth, max_nodes)[:5]

    def env_vcf_defend(self, boards, turns, max_depth=8, max_nodes=4096):
        return VD.defend_batch(self.n, boards, turns, max_depth, max_nodes)


def at(x, y):
    return y * N + x


def _records(games, status):
    moves = np.full((len(games), HW), 0xFFFF, dtype=np.uint16)
    lengths = np.zeros(len(games), dtype=np.int32)
    for g, mv in enumerate(games):
        moves[g, :len(mv)], lengths[g] = mv, len(mv)
    zero = np.zeros((len(games), HW))
    return R.GameRecords.from_log(N, np.zeros((len(games), HW), dtype=np.uint8), lengths, moves, zero, zero, zero, zero,
                                  np.array(status, dtype=np.uint8), lengths)


# Black builds the open three (2..4, 4) while White plays scattered stones on row 8.  In front of move 5 White faces a win in two and plays
# elsewhere: conceded.  Black makes the open four (a threat in one move: tactics()'s ground), White blocks one end, Black makes five.
CONCEDED = [at(2, 4), at(0, 8), at(3, 4), at(2, 8), at(4, 4), at(4, 8), at(1, 4), at(0, 4), at(5, 4)]
# White has the edge three (0..2, 8) when Black completes its open three.  In front of move 7 White answers with the four (3, 8): Black's
# forced block is no four, the solver's rule gives SAFE: held.  Black blocks (move 8: White's five is a threat in one, not counted for
# Black).  In front of move 9 the open three still stands: threatened again, White closes it at (1, 4): held.
HELD = [at(2, 4), at(0, 8), at(3, 4), at(1, 8), at(8, 0), at(2, 8), at(4, 4), at(3, 8), at(4, 8), at(1, 4)]
# Black's move 8 makes two open threes at once, (2..4, 4) and (4, 2..4); White's stones stand in the corners: no cell holds both
INDEFENSIBLE = [at(2, 4), at(0, 8), at(3, 4), at(8, 8), at(4, 2), at(0, 0), at(4, 3), at(8, 0), at(4, 4), at(1, 4), at(4, 1)]
GAMES = ((CONCEDED, R_BLACK_WIN), (HELD, 0), (INDEFENSIBLE, 0))


def _check_against_the_walk(f, depth, budget):
    for g, (cells, status) in enumerate(GAMES):
        before, want = VD.report(N, np.zeros(HW, dtype=np.uint8), cells, status, depth, budget)
        assert [int(x) for x in f["threat_before"][g, :len(cells)]] == before and not f["threat_before"][g, len(cells):].any(), g
        for name in VD.NAMES:
            assert f[name][g].tolist() == want[name], (g, name)


def test_conceded_held_and_indefensible():
    rec = _records([c for c, _s in GAMES], [s for _c, s in GAMES])
    f = rec.vcf_defence(StandIn(), max_depth=4, max_nodes=512)
    tb = f["threat_before"]
    assert [int(x) for x in tb[0, :9]] == [0, 0, 0, 0, 0, 2, 0, 1, 0]  # White faces m = 2 in front of move 5, m = 1 in front of move 7
    assert [f[k][0].tolist() for k in VD.NAMES] == [[0, 1], [0, 1], [0, 0], [0, 1], [0, 0]]
    assert [int(x) for x in tb[1, :10]] == [0, 0, 0, 0, 0, 0, 0, 2, 1, 2]  # (in front of move 8 it is Black that faces White's five)
    assert [f[k][1].tolist() for k in VD.NAMES] == [[0, 2], [0, 2], [0, 2], [0, 0], [0, 0]]
    assert [int(x) for x in tb[2, :11]] == [0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0]
    assert [f[k][2].tolist() for k in VD.NAMES] == [[0, 1], [0, 0], [0, 0], [0, 0], [0, 0]]
    assert f["threat_before"].dtype == np.int8 and all(f[k].dtype == np.int32 and f[k].shape == (3, 2) for k in VD.NAMES)
    _check_against_the_walk(f, 4, 512)


def test_cut_off_by_the_budget():
    rec = _records([c for c, _s in GAMES], [s for _c, s in GAMES])
    # two nodes: a win in two is found at the root of depth 2 (stage 1's threat, a LOSES cell), anything that needs a third node is cut off:
    # stage 1 without a threat in one or two, and every cell that holds.  So the threatened positions have no SAFE cell left: not defensible,
    # the played LOSES cell is no concession, and the cells that held are unknown
    f = rec.vcf_defence(StandIn(), max_depth=4, max_nodes=2)
    assert [int(x) for x in f["threat_before"][0, :9]] == [-1, -1, -1, -1, -1, 2, -1, 1, -1]
    assert [f[k][0].tolist() for k in VD.NAMES] == [[0, 1], [0, 0], [0, 0], [0, 0], [5, 2]]  # (stage 1 cut off in front of five black and two white moves)
    assert [f[k][1].tolist() for k in VD.NAMES] == [[0, 2], [0, 0], [0, 0], [0, 0], [4, 3 + 2]]
    _check_against_the_walk(f, 4, 2)


def test_an_empty_record_set():
    f = _records([], []).vcf_defence(StandIn())
    assert f["threat_before"].shape == (0, HW) and all(f[k].shape == (0, 2) for k in VD.NAMES)
