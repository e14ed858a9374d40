"""GPU tests of the base cache of the sibling rounds' difference path (k_group): the first TWO qualifying runs of a tree in a
round use the game's slots, so a leaf that becomes the tree's expansion target in the middle of a round is evaluated once.

Every case plays step-wise rounds on the difference path with the oracle in lockstep (the oracle consumes the engine's p / v: its trees are
the engine's), reads the parents of every round's requests from the oracle (request_info + the parent column of tree_dump) and replays them
through the restatement of the slot rule in tools/base_cache_sim.py.  Checked per case:
  * base cache on == base cache off: p, v, logits and the value in front of tanh of every row of every round, bit for bit;
  * OMOK_STAT_WORK_DIFF_FULL_RUNS, read per round, == the restatement's count of evaluated runs;
  * the case covered what it is there for: tree-rounds with two (three) qualifying runs, second-run leaves found again by the next round.

Where a search starts decides whether a round ever holds two qualifying runs: K = 16 simulations per round, and a leaf with c empty cells
changes in the middle of a round only if c mod 16 is neither 0 nor 1 nor 2, 14, 15 (both pieces must reach SIB_MIN = 3 rows).  From the EMPTY
board the root has 81 = 5 * 16 + 1 (225 = 14 * 16 + 1) cells and its children 80 (224): the piece left over is one row, no second run
qualifies, and `tools/base_cache_sim.py 9 128 2` prints
    first two runs, 2 slots   tree-rounds 3328 runs 3328 full 951 (28.6 %)  second runs 0, first run of the next round 0, of them reused 0
So the cases from the empty board keep the identity and the counter checks and ask for no second run (the oracle has none to give);
the same shapes from positions of SIX stones (75 = 4 * 16 + 11 cells at N = 9, 219 = 13 * 16 + 11 at N = 15) are the cases that exercise the second
run: on the CPU (oracle forward, same seeds) N = 9 gave 497 of 3328 tree-rounds with two qualifying runs, 425 of their second-run leaves were the next
round's first run and all 425 were found in a slot (evaluations 1413 -> 985)."""
import functools
import os
import sys

import numpy as np
import pytest

import omok_ai_amd as oa
from omok_ai_amd import binding as B
from oracle import oracle as O
import positions as P
from helpers import draw_sequence

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import base_cache_sim as S  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 7


def _boards(n, games, start):
    """start: "empty", "six" (quiet positions of six stones, Black to move) or an int e: the no-five board of the draw tests with e empty cells"""
    if start == "empty":
        return None
    if start == "six":
        return P.quiet(n, games, 6, seed=11)
    seq = draw_sequence(n)[: n * n - int(start)]
    b = np.zeros(n * n, dtype=np.uint8)
    b[seq[0::2]], b[seq[1::2]] = O.BLACK, O.WHITE
    return np.tile(b, (games, 1))


def _play(n, games, k, rounds, plies, start, mode=B.NET_F16X3, cache=True, lockstep=False, match=False):
    """Step-wise rounds of one engine.  -> dict: out = (p, v, logits, value in front of tanh) per round, full = OMOK_STAT_WORK_DIFF_FULL_RUNS per round,
    plan_full = the same figure from omok_debug_last_plan, parents = per round {game: parents of its requests} (lockstep only), ply = ply index per round."""
    tensors = oa.weights.init_random(n, seed=0)
    eng = oa.Engine(board_size=n, games=games, max_nodes=1024, max_tables=512, max_batch_k=k, seed=SEED, net_mode=mode)
    eng.load_weights(tensors)
    if match:
        eng.load_weights2(oa.weights.init_random(n, seed=1))
    eng.set_base_cache(cache)
    sp = oa.SelfPlay(eng)
    boards = _boards(n, games, start)
    if match:
        sp.match_reset_from(games // 2, boards)
    elif boards is None:
        sp.reset()
    else:
        sp.reset_from(boards)
    osp = None
    if lockstep:
        root_p = eng.evaluate_p(O.Environment(n).encode_nn_input(0)[None]).reshape(-1)
        osp = O.SelfPlay(n, games, cap_nodes=1024, cap_tables=512, seed=SEED)
        if boards is None:
            osp.reset(root_p)
        else:
            P.drive_to(osp, boards, eng.evaluate_p(P.input_rows(n, boards)).reshape(games, -1), root_p)
    res = {"out": [], "full": [], "plan_full": [], "parents": [], "ply": []}
    for ply in range(plies):
        for rnd in range(rounds):
            nreq = sp.round_generate(rnd, k, 0.25, 0.03)
            if osp is not None:
                oin = osp.round_generate(rnd, k, 0.25, 0.03)
                assert nreq == len(oin) and np.array_equal(sp.round_inputs(), oin), f"ply {ply} round {rnd}: the oracle is out of step"
                res["parents"].append(S.oracle_parents(osp, nreq, osp.ply & 1))
            before = eng.stats()["work_diff_full_runs"]
            p, v = sp.round_eval()
            lg, vp = sp.round_logits()
            plan = eng.last_plan()
            assert plan["path"] == "difference", (ply, rnd, nreq, plan)
            res["full"].append(int(eng.stats()["work_diff_full_runs"] - before))
            res["plan_full"].append(plan["full_runs"])
            res["out"].append(tuple(np.array(a).copy() for a in (p, v, lg, vp)))
            res["ply"].append(ply)
            sp.round_scatter()
            if osp is not None:
                osp.round_scatter(p, v)
        if ply + 1 < plies:
            a = sp.sample_actions(1.0, 30)
            if osp is not None:
                assert np.array_equal(a, osp.sample(1.0, 30))
                om = osp.mirror_generate()
                assert sp.mirror_generate() == len(om)
                pm = sp.mirror_eval()
                sp.mirror_apply()
                osp.advance(pm)
            else:
                sp.advance()
    eng.close()
    return res


@functools.lru_cache(maxsize=None)
def _cached(n, games, k, rounds, plies, start, mode=B.NET_F16X3):
    """the run of a shape with the base cache on and the oracle in lockstep: computed once, shared, never modified"""
    return _play(n, games, k, rounds, plies, start, mode, cache=True, lockstep=True)


def _same_outputs(a, b, tag):
    assert len(a["out"]) == len(b["out"])
    for rnd, (x, y) in enumerate(zip(a["out"], b["out"])):
        for name, u, w in zip(("p", "v", "logits", "value in front of tanh"), x, y):
            assert u.shape == w.shape and np.array_equal(u.view(np.uint32), w.view(np.uint32)), f"{tag}: {name} of round {rnd} differ"


def _model(res):
    """the restatement over the run's request lists -> (evaluated runs per round, the model with its totals, histogram of qualifying runs per tree-round)"""
    m, want, hist, last_ply = S.BaseCacheModel(ways=2, two_runs=True), [], {}, None
    for ply, per_game in zip(res["ply"], res["parents"]):
        if ply != last_ply:
            m.clear()  # (advance: the trees changed, the engine clears its tags)
            last_ply = ply
        for parents in per_game.values():
            q = len(S.qualifying_runs(parents))
            hist[q] = hist.get(q, 0) + 1
        want.append(m.round(per_game))
    return want, m, hist


def _check_counter(res, tag, min_two, min_reused_share):
    want, m, hist = _model(res)
    two = sum(c for q, c in hist.items() if q >= 2)
    print(f"{tag}: qualifying runs per tree-round {dict(sorted(hist.items()))}; {m.line('first two runs, 2 slots')}")
    print(f"{tag}: evaluated runs per round, engine {res['full']}")
    assert res["full"] == res["plan_full"], f"{tag}: the counter and the plan of the same forwards disagree"
    assert res["full"] == want, f"{tag}: OMOK_STAT_WORK_DIFF_FULL_RUNS per round against the restatement {want}"
    assert two >= min_two and m.second_runs >= min_two, (tag, hist)
    assert 2 * m.second_reused >= m.second_runs * 2 * min_reused_share, (tag, m.second_runs, m.second_reused)
    return m, hist


# (start, tree-rounds with two qualifying runs at least, share of their second-run leaves found in a slot by the next round at least):
# the issue's bounds (20, one half) where the oracle has second runs at all, see the module's docstring
N9 = [("empty", 0, 0.0), ("six", 20, 0.5)]


@pytest.mark.parametrize("start,min_two,min_share", N9)
def test_second_runs_keep_their_base_at_9x9(start, min_two, min_share):
    """N = 9, 128 games, K = 16 (2048 rows >= the 1024-row threshold), 200 simulations (13 rounds) x two plies."""
    on = _cached(9, 128, 16, 13, 2, start)
    off = _play(9, 128, 16, 13, 2, start, cache=False)
    _same_outputs(on, off, f"9x9 from {start}: base cache on / off")
    _check_counter(on, f"9x9 from {start}", min_two, min_share)
    assert sum(off["full"]) > sum(on["full"])  # (the switch did switch the cache off)


# N = 15, 192 games, K = 16: 3072 rows, the difference path in every operand format.  Empty board: rounds 0-17 of the first ply (the root fills in round 14 with ONE
# row to spare: no second run); six stones: rounds 0-15 (the root's last 11 cells and 5 children of the next leaf share round 13, round 14 finds that leaf's base)
N15 = [("empty", 18, 0, 0.0), ("six", 16, 20, 0.5)]


@pytest.mark.parametrize("start,rounds,min_two,min_share", N15)
def test_second_runs_keep_their_base_at_15x15(start, rounds, min_two, min_share):
    on = _cached(15, 192, 16, rounds, 1, start)
    off = _play(15, 192, 16, rounds, 1, start, cache=False)
    _same_outputs(on, off, f"15x15 from {start}: base cache on / off")
    _check_counter(on, f"15x15 from {start}", min_two, min_share)


@pytest.mark.parametrize("mode", [B.NET_F16X3_FP6, B.NET_F16X3_F16])
@pytest.mark.parametrize("start,rounds", [(s, r) for s, r, _, _ in N15])
def test_cache_on_equals_cache_off_in_the_forced_formats(start, rounds, mode):
    on = _play(15, 192, 16, rounds, 1, start, mode)
    off = _play(15, 192, 16, rounds, 1, start, mode, cache=False)
    _same_outputs(on, off, f"15x15 from {start}, mode {mode}: base cache on / off")
    assert sum(off["full"]) > sum(on["full"])


@pytest.mark.parametrize("empties,rounds", [(7, 2), (9, 3)])
def test_third_runs_stay_uncacheable(empties, rounds):
    """Trees with three and more qualifying runs in one round: every game starts from the draw tests' no-five board with 7 (9) cells left, so a leaf is used up
    after 7, 6, ... (9, 8, ...) simulations and the 16 requests of a round are children of three or four leaves.  128 games keep the rounds at 1920-2048 rows: the
    difference path (the round after these falls to 128 rows and the copy path, and is not played).  The runs from the third on take slots behind the games', are
    evaluated every time and leave no tag: the counter equals the restatement, the outputs equal the cache-off outputs."""
    on = _cached(9, 128, 16, rounds, 1, empties)
    off = _play(9, 128, 16, rounds, 1, empties, cache=False)
    _same_outputs(on, off, f"{empties} empty cells: base cache on / off")
    _, hist = _check_counter(on, f"{empties} empty cells", 128, 0.0)
    assert sum(c for q, c in hist.items() if q >= 3) >= 128, hist


def test_a_match_round_with_second_runs():
    """Match rounds (k_group<true>, one net per colour: 128 games = 2048 rows per net) from the six-stone positions, rounds 0-5: the leaf change of
    round 4 and the round that finds its base.  Cache on == cache off for the rows of both nets, bit for bit."""
    on = _play(9, 256, 16, 6, 1, "six", match=True)
    off = _play(9, 256, 16, 6, 1, "six", match=True, cache=False)
    _same_outputs(on, off, "match rounds: base cache on / off")
    assert sum(off["full"]) > sum(on["full"])


def test_two_fresh_engines_agree():
    """Slots and evaluation-list entries are handed out by atomics: outputs and counters must not depend on their order."""
    a = _cached(9, 128, 16, 13, 2, "six")
    b = _play(9, 128, 16, 13, 2, "six")
    _same_outputs(a, b, "two fresh engines")
    assert a["full"] == b["full"] and a["plan_full"] == b["plan_full"]
