"""GPU tests of the run loop's sibling rounds without single-workgroup kernels on their chain: such a round launches no k_scan -- k_round
leaves every game's request count and zeroes the grouping counters, k_group derives the request offsets, the round's total and the evaluation counter -- and
the difference path's slot layout (bin starts, window tiles, K splits) is derived by workgroup 0 of the base pass's launch instead of a kernel of its own.
The step-wise rounds (round_generate / round_eval / round_scatter) keep k_scan and k_fill: they are the reference for "same bits".

  1. omok_execute == the step-wise rounds, tree dumps bit for bit after each of 2 plies, at the smallest shapes that reach each path
  2. the same with holes in the live games (a dead first game, a whole dead k_group workgroup, a dead last game, every third game between), plus the device-side
     plan of the last round and the evaluation counter
  3. omok_selfplay_run twice -> identical packed replay bytes
Reference: alpha-zero/src/parallel_mcts_executor.rs:194-265 (the order-preserving request concat and the scatter of a round)."""
import numpy as np
import pytest

import omok_ai_amd as oa
from omok_ai_amd import binding as B
from oracle import oracle as O
import positions as P
from test_gpu_headline_path import _dumps, _packed_run, _same_dumps

pytestmark = pytest.mark.gpu

PLAN_DEVICE = ("runs", "singles", "run_rows", "full_runs", "tiles", "t_split", "ways", "fways")  # what k_group / the prefix role left in d_gcnt


def _ply(sp, variant, count, k):
    if variant == "execute":
        sp.execute(count, k)
    else:
        for rnd in range(count // k):
            sp.round_generate(rnd, k)
            sp.round_eval()
            sp.round_scatter()


def _advance(sp, variant):
    sp.sample_actions(1.0, 30)
    if variant == "execute":
        sp.advance()
    else:
        sp.mirror_generate()
        sp.mirror_eval()
        sp.mirror_apply()


@pytest.mark.parametrize("n,games,k,count,path", [
    (15, 200, 16, 48, "difference"),  # 3200 rows >= 3072; 200 games = 12.5 k_group workgroups, no multiple of the old scan's chunking
    (15, 40, 16, 48, "copy"),         # 640 rows: no prefix role, k_group's offsets only
    (9, 136, 8, 24, "difference"),    # 1088 rows >= 1024: the N = 9 base pass (two samples per workgroup) with the role
])
def test_execute_equals_stepwise_rounds(n, games, k, count, path):
    """1. The run loop's rounds (no k_scan, no k_fill; the prefix role inside the base pass) leave the trees the step-wise rounds leave."""
    tensors = oa.weights.init_random(n, seed=0)
    out = []
    for variant in ("execute", "stepwise"):
        eng = oa.Engine(board_size=n, games=games, max_nodes=4 * count + 256, max_tables=count + 64, max_batch_k=k, seed=5)
        eng.load_weights(tensors)
        sp = oa.SelfPlay(eng)
        sp.reset()
        per_ply = []
        for _ in range(2):
            _ply(sp, variant, count, k)
            plan = eng.last_plan()
            assert plan["path"] == path, plan
            per_ply.append(_dumps(sp, games))
            _advance(sp, variant)
        per_ply.append(_dumps(sp, games))
        out.append(per_ply)
        eng.close()
    for ply, (a, b) in enumerate(zip(out[0], out[1])):
        _same_dumps(a, b, f"n={n} games={games} after ply {ply}")


def _dead_pattern(games):
    """game 0, games 16-31 (a whole k_group workgroup), the last game, every third game between"""
    dead = {0, games - 1} | set(range(16, 32)) | set(range(32, games - 1, 3))
    return np.array([g in dead for g in range(games)])


def _hole_boards(n, games, dead):
    """[games][HW] boards of 8 stones, Black to move, and the moves that end exactly the games of `dead`: those have four Black stones in a row with both ends
    open and the move completes five; the others are quiet random positions and the move is a cell at which Black does not win."""
    boards = P.quiet(n, games, 8, seed=7)
    actions = np.zeros(games, dtype=np.int32)
    for g in range(games):
        if dead[g]:
            x, y = 1 + g % 8, 1 + g % 11  # (the four at x .. x + 3, open cells x - 1 and x + 4 <= 12)
            four = P._line(n, x, y, 1, 0, 4)
            boards[g] = P._board(n, four, P._scatter(n, set(four), 4))
            actions[g] = y * n + x + 4
            assert actions[g] in P.winning_cells(n, boards[g])
        else:
            wins = set(P.winning_cells(n, boards[g]))
            actions[g] = next(int(c) for c in np.flatnonzero(boards[g] == O.EMPTY) if int(c) not in wins)
    verdicts, stones = P.verdicts(n, boards)
    assert np.all(verdicts == P.LEGAL) and np.all(stones == 8)
    return boards, actions


@pytest.mark.parametrize("mode", [B.NET_F16X3_FP6, B.NET_F16X3])
@pytest.mark.parametrize("games", [232, 320])
def test_execute_equals_stepwise_rounds_with_holes_in_the_live_games(games, mode):
    """2. N = 15, K = 16, 32 simulations, one ply after play_actions has ended game 0, games 16-31, the last game and every third game between (32, 35, ...).
    Of 232 games 147 stay live (2352 rows), of 320 games 206 (3296 rows).  In the fp6 format rounds below 3072 rows take the copy path, so the two sizes run the
    copy and the difference path; the mixed format switches at 2048 rows and runs the difference path at both."""
    n, k, count = 15, 16, 32
    dead = _dead_pattern(games)
    live = int((~dead).sum())
    assert live == {232: 147, 320: 206}[games]
    boards, actions = _hole_boards(n, games, dead)
    tensors = oa.weights.init_random(n, seed=0)
    out = []
    for variant in ("execute", "stepwise"):
        eng = oa.Engine(board_size=n, games=games, max_nodes=4 * count + 256, max_tables=count + 64, max_batch_k=k, seed=9, net_mode=mode)
        eng.load_weights(tensors)
        sp = oa.SelfPlay(eng)
        sp.reset_from(boards)
        sp.play_actions(actions)
        alive = sp.game_info()[0]
        assert np.array_equal(alive != 0, ~dead), "play_actions did not end exactly the chosen games"
        eng.reset_stats()
        _ply(sp, variant, count, k)
        plan = eng.last_plan()
        fmt = B.FC0_FORMATS[int(eng.stats()["fc0_format"])]
        assert plan["path"] == ("copy" if live * k < (2048 if fmt == "mixed" else 3072) else "difference"), (fmt, plan)
        if mode == B.NET_F16X3_FP6:
            assert fmt == "fp6" and plan["path"] == ("copy" if games == 232 else "difference")
        out.append((_dumps(sp, games), {key: plan[key] for key in ("path", "rows") + PLAN_DEVICE}, eng.stats()["evals"]))
        eng.close()
    _same_dumps(out[0][0], out[1][0], f"{games} games with holes")
    assert out[0][1] == out[1][1], ("device-side plan of the last round", out[0][1], out[1][1])
    assert out[0][1]["runs"] > 0 and out[0][2] > 0
    assert out[0][2] == out[1][2], ("evaluations", out[0][2], out[1][2])


def test_selfplay_run_twice_gives_the_same_replay_bytes():
    """3. N = 15, 200 games, 48 simulations, 3 plies of omok_selfplay_run on the difference path: the packed replay records of two runs are equal."""
    n, games, count, k, plies = 15, 200, 48, 16, 3
    tensors = oa.weights.init_random(n, seed=0)
    a = _packed_run(n, games, count, k, plies, 3, tensors)
    b = _packed_run(n, games, count, k, plies, 3, tensors)
    assert a[0] == games * plies
    assert a[0] == b[0] and np.array_equal(a[1], b[1]), "two identical runs differ"
    _same_dumps(a[2], b[2], "run vs run")
