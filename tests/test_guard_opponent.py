"""No-GPU pins of tests/guard_opponent.py, the plain-Python restatement of the defending scripted player (OMOK_OPP_GUARD, omok_env_guard_scan
in include/omok_mi355x.h) that the GPU tests compare the device kernels with: one hand-made position per step of the rule whose answer follows
from the rule read by hand, at 9 x 9 and 15 x 15 and for both sides to move; the constants; and the property the rule has by construction --
on its own games the guard concedes no position in which a safe move exists."""
import os
import re

import numpy as np
import pytest

import guard_opponent as GO
import scripted_opponent as SO
import vcf_defence as VD
import vcf_solver as VS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [9, 15])
def test_hand_made_positions_one_per_step(n):
    """the expected (cell, step, level, count) of every position are worked out in the comments of guard_opponent.hand_made"""
    hand = GO.hand_made(n)
    steps = set()
    for name, (board, side, depth, budget, expect) in sorted(hand.items()):
        got = GO.move(SO.make_env(n, board, side), 0, depth, budget)
        assert got == expect, f"{name}: {got} != {expect}"
        steps.add(got[1])
    assert steps == {1, 2, 3, 4, 5}
    full = np.full(n * n, 1, dtype=np.uint8)
    assert GO.move(SO.make_env(n, full, 0), 0) == (-1, 0, 0, 0)  # step 0: no empty cell


@pytest.mark.parametrize("n", [9, 15])
def test_the_map_of_the_swapped_chain(n):
    """step 3 and step 4 of the hand-made positions, on the map itself: the safe cells are the four read off the chain, the move OMOK_OPP_VCF
    would make loses, and at 4 nodes the same four cells are the only ones that do not lose"""
    at = lambda x, y: y * n + x  # noqa: E731
    x0 = VS._x0(n, 4)
    four = sorted([at(x0 + 3, 1), at(x0 + 3, 4), at(x0 + 4, 4), at(x0 + 3, 5)])
    for side in (0, 1):
        board, _side, depth, budget, _expect = GO.hand_made(n)[f"map_safe_s{side}"]
        env = SO.make_env(n, board, side)
        c0, level, solved, count = GO.vcf_move(env, 0, depth, budget)
        assert (c0, level, solved, count) == (at(x0 + 2, 1), 6, False, 20)
        m = VD.defend(n, board, side, depth, budget)
        assert [a for a in range(n * n) if m.status[a] == VD.SAFE] == four and m.status[c0] == VD.LOSES and VD.UNKNOWN not in m.status
        assert m.nodes[c0] == 4  # the figure the step-4 position's budget rests on
        m = VD.defend(n, board, side, 6, 4)
        assert [a for a in range(n * n) if m.status[a] == VD.UNKNOWN] == four and VD.SAFE not in m.status and m.status[c0] == VD.LOSES
    # a draw word picks among the four: r = mulhi(x0, 4)
    board, side, depth, budget, _expect = GO.hand_made(n)["map_safe_s0"]
    for r in range(4):
        assert GO.move(SO.make_env(n, board, side), (r << 30) + 5, depth, budget) == (four[r], 3, 6, 4)


def test_constants_agree():
    from omok_ai_amd import binding
    assert GO.OPP_GUARD == binding.OPP_GUARD == 7
    assert binding.SCRIPTED_PLAYERS == {"random": 0, "naive": 1, "threat": 3, "vcf": 5, "guard": 7}
    assert (GO.D_OPP, GO.NB_OPP) == (binding.VCF_OPP_DEPTH, binding.VCF_OPP_NODES)
    header = open(os.path.join(ROOT, "include", "omok_mi355x.h")).read()
    assert re.search(r"^#define OMOK_OPP_GUARD 7$", header, flags=re.M) and not re.search(r"^#define OMOK_OPP_\w+ [246]$", header, flags=re.M)
    assert re.search(r"\bint omok_env_guard_scan\(", header) and "omok_env_guard_scan" in binding.SYMBOLS
    rust = open(os.path.join(ROOT, "bindings", "omok_mi355x.rs")).read()
    assert re.search(r"pub const OMOK_OPP_GUARD: i32 = 7;", rust) and "pub fn omok_env_guard_scan(" in rust


def test_the_guard_concedes_nothing_on_its_own_games():
    """vcf_defence.report at the player's own budget: `conceded` counts the positions with a safe move in which the mover played a losing one,
    and the rule plays a LOSES cell only where no SAFE cell exists.  The games do threaten the guard, and every step of the rule occurs."""
    n = 9
    GO.assert_not_vacuous(GO.game_steps(n))
    threatened = 0
    for side in (0, 1):
        for positions, moves, status, _log in GO.games(n)[side]:
            _before, out = VD.report(n, positions[0][0], moves, status, GO.D_OPP, GO.NB_OPP)
            assert out["conceded"][side] == 0
            threatened += out["threatened"][side]
    assert threatened > 0
