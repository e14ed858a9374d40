"""No-GPU pins of tests/vcf_solver.py, the plain-Python restatement of the forced-win solver (victory by continuous fours,
omok_env_vcf_solve in include/omok_mi355x.h) that the GPU tests compare the device kernel with: hand-made positions whose answer follows
from the rule read by hand, at 9 x 9 and 15 x 15 and for both sides to move; the closure of every line it reports; the conditions the
random set has to meet."""
import os
import re

import numpy as np
import pytest

import scripted_opponent as SO
import threat_opponent as TO
import vcf_solver as VS
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [9, 15])
def test_hand_made_positions(n):
    pos = VS.hand_made(n)
    rows = (4, 8) if n == 9 else (4, 8, 12)
    assert len(pos) == 2 * (5 * len(rows) + 10)
    for name, (board, side, depth, want) in sorted(pos.items()):
        r = VS.solve(n, board, side, depth, 4096)
        assert (r.verdict, r.moves, r.cell) == want, name
        assert len(r.pv) == 2 * depth - 1
        if r.verdict == 1:
            assert r.pv[0] == r.cell and sum(c >= 0 for c in r.pv) == 2 * r.moves - 1
            VS.closure(n, board, side, r.pv)
        else:
            assert all(c == -1 for c in r.pv)


@pytest.mark.parametrize("n", [9, 15])
@pytest.mark.parametrize("side", [0, 1])
def test_lines_and_node_counts_read_by_hand(n, side):
    pos = VS.hand_made(n)
    at = lambda x, y: y * n + x  # noqa: E731
    x0 = 3 if n == 15 else 2
    # the open three: one node per depth; the line is the four, then the two ends in ascending order
    board, s, _d, _w = pos[f"open_three_s{side}_r4"]
    r = VS.solve(n, board, s, 8, 4096)
    assert r.nodes == 2 and r.pv[:3] == [at(x0 - 1, 4), at(x0 - 2, 4), at(x0 + 3, 4)] and r.pv[3:] == [-1] * 12
    # the chain of two closed threes: depth 1 and 2 one node each, depth 3 the root and one child
    board, s, _d, _w = pos[f"chain_m3_s{side}"]
    r = VS.solve(n, board, s, 8, 4096)
    assert r.nodes == 4 and (r.fo1, r.fo2) == (0, 0)
    assert r.pv[:5] == [at(x0 + 3, 4), at(x0 + 4, 4), at(x0 + 3, 1), at(x0 + 3, 0), at(x0 + 3, 5)]
    assert VS.solve(n, board, s, 8, 3)[:4] == (-1, -1, 0, 3)  # the fourth node is one too many
    assert VS.solve(n, board, s, 8, 4)[:4] == (1, at(x0 + 3, 4), 3, 4)
    # m = 4: depth 3 tries both fours of the row (three nodes), depth 4 walks straight down
    board, s, _d, _w = pos[f"chain_m4_s{side}"]
    r = VS.solve(n, board, s, 8, 4096)
    assert r.nodes == 1 + 1 + 3 + 3
    assert r.pv[:7] == [at(x0 + 3, 4), at(x0 + 4, 4), at(x0 + 3, 5), at(x0 + 3, 6), at(x0 + 1, 3), at(x0, 2), at(x0 + 5, 7)]
    # the blocking four: the defender's one five is the only candidate, and it is an open four
    board, s, _d, _w = pos[f"blocking_four_s{side}"]
    r = VS.solve(n, board, s, 8, 4096)
    assert (r.fo1, r.fo2) == (1, 0) and r.pv[:5] == [at(x0 + 3, 4), at(x0 + 4, 4), at(x0 + 4, 3), at(x0 + 5, 2), at(x0, 7)]
    board, s, _d, _w = pos[f"block_leaves_two_fives_s{side}"]
    r = VS.solve(n, board, s, 8, 4096)
    assert r.fo2 == 6 and r.fo1 == 0  # at every depth from 3 on
    # nothing to try: one node per depth; a byte that is no stone counts as empty
    board, s, _d, _w = pos[f"six_is_no_four_s{side}"]
    assert VS.solve(n, board, s, 8, 4096).nodes == 8 and VS.solve(n, board, s, 16, 4096).nodes == 16
    board, s, _d, _w = pos[f"full_board_s{side}"]
    assert VS.solve(n, board, s, 5, 4096).nodes == 5
    board, s, _d, want = pos[f"open_three_s{side}_r8"]
    odd = board.copy()
    odd[board == 0] = 7
    assert VS.solve(n, odd, s, 8, 4096)[:3] == (want[0], want[2], want[1])
    # the edge three: from depth 3 on the root and its two fours
    board, s, _d, _w = pos[f"edge_three_s{side}"]
    assert VS.solve(n, board, s, 8, 4096).nodes == 2 + 6 * 3


@pytest.mark.parametrize("n", [9, 15])
def test_the_random_set_meets_its_conditions(n):
    boards, turns = VS.random_set(n)
    verdict, cell, moves, nodes, pv, res = VS.random_set_want(n, 8, 4096)
    print(f"board {n}: {len(boards)} positions, verdicts {[int(np.count_nonzero(verdict == v)) for v in (-1, 0, 1)]}, "
          f"moves {[int(np.count_nonzero(moves == m)) for m in range(9)]}, largest node count {int(nodes.max())}, "
          f"|Fo| == 1 at {sum(r.fo1 for r in res)} nodes, |Fo| >= 2 at {sum(r.fo2 for r in res)}")
    assert 150 <= len(boards) <= 1000
    for side in (0, 1):
        assert set(int(v) for v in verdict[turns == side]) == {0, 1}  # with NB = 4096 no verdict is -1
    assert {1, 2, 3} <= set(int(m) for m in moves) and moves.max() >= 4
    assert sum(r.fo1 for r in res) > 0 and sum(r.fo2 for r in res) > 0
    assert np.all(nodes[verdict == 0] >= 8) and np.all(cell[verdict == 0] == -1) and np.all(moves[verdict == 0] == 0)
    assert -1 in VS.random_set_want(n, 8, 8)[0]
    for b, t, r in zip(boards, turns, res):  # closure of every line
        if r.verdict == 1:
            VS.closure(n, b, int(t), r.pv)
    # against the threat-aware rule: m = 1 is its level 1, m = 2 its level 3 at the same cell
    for b, t, r in zip(boards, turns, res):
        c, level = TO.scan(SO.make_env(n, b, int(t)))[:2]
        if np.count_nonzero(b == 0) > 1:
            assert (r.moves == 1) == (level == 1)
        if level == 3:
            assert (r.moves, r.cell) == (2, c)


@pytest.mark.parametrize("n", [9, 15])
def test_the_scripted_player_differs_from_the_threat_player_only_at_long_wins(n):
    pos = VS.hand_made(n)
    for name, (board, side, _depth, want) in sorted(pos.items()):
        env = SO.make_env(n, board, side)
        cell, level, solved = VS.scripted_cell(env)
        r = VS.solve(n, board, side, VS.VCF_OPP_DEPTH, VS.VCF_OPP_NODES)
        assert solved == (r.verdict == 1 and level >= 3), name
        if solved and r.moves >= 3:
            assert cell == r.cell and name.startswith(("chain_m", "blocking_four")), name
        else:
            assert cell == TO.scan(env)[0], name
    key = O.stream_key(3, 0)
    env = SO.make_env(n, pos["edge_three_s0"][0], 0)
    assert VS.move(env, key, 3, 1)[:2] == TO.move(env, key, 3, 1)  # the draw of level 6 is the threat player's


def test_constants_agree():
    from omok_ai_amd import binding
    assert VS.OPP_VCF == binding.OPP_VCF == 5 and binding.OPPONENT_KINDS == {"random": 0, "naive": 1, "threat": 3, "vcf": 5}
    header = open(os.path.join(ROOT, "include", "omok_mi355x.h")).read()
    assert re.search(r"^#define OMOK_OPP_VCF 5$", header, flags=re.M) and not re.search(r"^#define OMOK_OPP_\w+ [24]$", header, flags=re.M)
    assert re.search(rf"^#define OMOK_VCF_OPP_DEPTH {VS.VCF_OPP_DEPTH}$", header, flags=re.M)
    assert re.search(rf"^#define OMOK_VCF_OPP_NODES {VS.VCF_OPP_NODES}$", header, flags=re.M)
    rust = open(os.path.join(ROOT, "bindings", "omok_mi355x.rs")).read()
    assert re.search(r"pub const OMOK_OPP_VCF: i32 = 5;", rust) and "pub fn omok_env_vcf_solve(" in rust
    assert "omok_env_vcf_solve" in binding.SYMBOLS and re.search(r"\bint omok_env_vcf_solve\(", header)
