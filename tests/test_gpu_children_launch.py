"""GPU tests of the children launch of a difference-path round: the full rows' fc0 runs in front of k_sib_children2, and every workgroup of
k_sib_children2 reduces its share of that launch's split-K partials into the fp32 fc0 rows (facc) the window tiles add to -- k_facc_reduce is no launch of the
chain any more.  The kernel also leaves block 0's first-layer fragments out of its LDS prologue.

  1. stale rows: a reduce that is missing, partial, or read before it was written leaves another position's fc0 row in a slot -- every row of every round
     against an OMOK_NET_F32 engine on the same inputs, base cache off (every run's row is rewritten each round) and on (a few misses among hits)
  2. determinism: the same rounds twice on one engine and once on a fresh one, equal in every bit
  3. the K split of the full rows (fways, chosen on the device) in both of its classes: >= 9 and <= 8
  4. one ply through omok_selfplay_run (k_round hands its counts to k_group, lazy policy) equals the step-wise rounds, tree dumps bit for bit

Shapes: the smallest that reach the difference path -- N = 15: 128 games x K = 16 = 2048 rows (sib_delta_min_rows of the mixed format), N = 9: 64 games x
K = 16 = 1024 rows; trees of 256 nodes.  fways = CUs / tiles of full rows, at most 64, lowered until no split is empty (bin_prefix_role): one or two tiles of
full rows (these shapes) give the class >= 9, and <= 8 needs at least CUs / 8 tiles, 29 on a 256-CU part: more than 3584 rows evaluated in full in one round.
A round-0 of G games with the cache off evaluates G bases, so that class is reached by 4096 games (N = 9, one round)."""
import functools

import numpy as np
import pytest

import omok_ai_amd as oa
from omok_ai_amd import binding as B
from test_gpu_conv_tables import _stage_boards
from test_gpu_headline_path import _dumps, _same_dumps

pytestmark = pytest.mark.gpu

TOL = 1e-3  # the project's contract against the fp32 kernels (test_gpu_conv_tables.py)
MODE = B.NET_F16X3_MIXED  # the flagship's format, set: no probe at commit
K = 16
ROUNDS = 4
# n: (games, rows, stones of the mid-game position).  The position leaves 40 empty cells: the 64 descents of four rounds expand every child of the root within
# three, so the later rounds ask for positions below the root -- new bases and single rows beside the runs whose base is cached
SHAPES = {15: (128, 2048, 185), 9: (64, 1024, 41)}


def _engine(n, games, cache, mode=MODE, seed=13):
    eng = oa.Engine(board_size=n, games=games, max_nodes=256, max_tables=128, max_batch_k=K, seed=seed, net_mode=mode)
    eng.load_weights(oa.weights.init_random(n, seed=4))
    eng.set_base_cache(cache)
    return eng


def _rounds(eng, n, games, start, rounds=ROUNDS):
    """per round: (inputs, p, v, logits, vpre, plan) of step-wise rounds from the empty board or the mid-game position"""
    sp = oa.SelfPlay(eng)
    sp.set_episode(0)  # (every reset moves on to the next RNG stream: a fresh engine's first reset uses stream 0)
    if start == "empty":
        sp.reset()
    else:
        sp.reset_from(_stage_boards(n, games, SHAPES[n][2]))
    out = []
    for rnd in range(rounds):
        nreq = sp.round_generate(rnd, K, 0.25, 0.03)
        x = sp.round_inputs().copy()
        p, v = sp.round_eval()
        lg, vp = sp.round_logits()
        plan = eng.last_plan()
        sp.round_scatter()
        out.append((x, np.array(p).reshape(nreq, -1).copy(), np.array(v).reshape(-1).copy(), lg.copy(), vp.copy(), plan))
    return out


@functools.lru_cache(maxsize=None)
def _played(n, cache, start):
    """the rounds of a fresh engine at the shape of board size n (computed once, shared by the tests, never changed)"""
    games = SHAPES[n][0]
    eng = _engine(n, games, cache)
    out = _rounds(eng, n, games, start)
    eng.close()
    return out


def _same_rounds(a, b, tag):
    assert len(a) == len(b)
    for rnd, (ra, rb) in enumerate(zip(a, b)):
        for what, ta, tb in zip(("inputs", "p", "v", "logits", "vpre"), ra, rb):
            assert ta.shape == tb.shape and np.array_equal(ta.view(np.uint32), tb.view(np.uint32)), f"{tag}: {what} of round {rnd} differ"


@pytest.mark.parametrize("start", ["empty", "mid"])
@pytest.mark.parametrize("cache", [False, True], ids=["cache off", "cache on"])
@pytest.mark.parametrize("n", [15, 9])
def test_no_stale_full_row(n, cache, start):
    """1. of the module text.  Bound: 1e-3 on p, v, logits and the pre-tanh value of every row against the fp32 kernels."""
    games, rows, _ = SHAPES[n]
    f32 = oa.Engine(board_size=n, games=games, max_nodes=64, max_tables=32, max_batch_k=K, seed=13, net_mode=B.NET_F32)
    f32.load_weights(oa.weights.init_random(n, seed=4))
    worst, plans = np.zeros(4), []
    for x, p, v, lg, vp, plan in _played(n, cache, start):
        assert plan["path"] == "difference" and len(x) == rows == plan["rows"], plan
        plans.append((plan["runs"], plan["full_runs"], plan["singles"], plan["fways"]))
        pf, vf = f32.evaluate_pv(x)
        lf, vpf = f32.evaluate_logits(x)
        d = [float(np.abs(a.reshape(len(x), -1) - b.reshape(len(x), -1)).max()) for a, b in ((p, pf), (v, vf), (lg, lf), (vp, vpf))]
        worst = np.maximum(worst, d)
    f32.close()
    print(f"n={n} cache {cache} from {start}: (runs, runs evaluated in full, singles, fways) per round {plans}; |dp| {worst[0]:.2e} |dv| {worst[1]:.2e} "
          f"|dlogit| {worst[2]:.2e} |dvpre| {worst[3]:.2e}")
    if not cache:
        assert all(full == runs for runs, full, _, _ in plans)
    elif start == "mid":  # (from the empty board four rounds stay among the root's children: every round behind the first is all hits)
        assert any(full + singles > 0 and full < runs for runs, full, singles, _ in plans[1:]), "no round with full rows among cached bases"
    assert worst.max() < TOL, worst


@pytest.mark.parametrize("cache", [False, True], ids=["cache off", "cache on"])
@pytest.mark.parametrize("n", [15, 9])
def test_same_bits_again_and_on_a_fresh_engine(n, cache):
    """2. of the module text: nothing in a round's outputs depends on which workgroup reduced which row, on what the slab or facc held before, or on timing."""
    games = SHAPES[n][0]
    eng = _engine(n, games, cache)
    first = _rounds(eng, n, games, "mid")
    again = _rounds(eng, n, games, "mid")
    eng.close()
    assert all(r[5]["path"] == "difference" for r in first + again)
    _same_rounds(first, again, "twice on one engine")
    _same_rounds(first, _played(n, cache, "mid"), "against a fresh engine")


def test_both_classes_of_the_full_row_split():
    """3. of the module text.  The rounds of the small shapes (cache on and off), round 0 of 256 games (4096 rows, N = 15) and round 0 of 4096 games with the
    cache off (N = 9: 4096 bases evaluated in full = 32 tiles); the large round's first rows against the fp32 kernels, bound as above."""
    seen = [r[5]["fways"] for n in SHAPES for cache in (False, True) for r in _played(n, cache, "empty")]
    eng = _engine(15, 256, False)
    r256 = _rounds(eng, 15, 256, "empty", rounds=1)[0]
    eng.close()
    assert r256[5]["path"] == "difference" and r256[5]["rows"] == 4096, r256[5]
    seen.append(r256[5]["fways"])
    eng = _engine(9, 4096, False)
    x, p, v, lg, vp, plan = _rounds(eng, 9, 4096, "empty", rounds=1)[0]
    eng.close()
    assert plan["path"] == "difference" and plan["rows"] == 65536, plan
    seen.append(plan["fways"])
    print(f"fways seen: {sorted(set(seen))}; the 4096-game round: {plan}")
    assert max(seen) >= 9 and min(seen) >= 1, seen
    assert 2 <= plan["fways"] <= 8, plan  # (a round without full rows shows fways = 1: not the class meant here)
    # the large round: rows of the first and the last games (their bases lie in the first and the last tile of full rows)
    f32 = oa.Engine(board_size=9, games=64, max_nodes=64, max_tables=32, max_batch_k=K, seed=13, net_mode=B.NET_F32)
    f32.load_weights(oa.weights.init_random(9, seed=4))
    for rows in (slice(0, 1024), slice(65536 - 1024, 65536)):
        pf, vf = f32.evaluate_pv(x[rows])
        lf, vpf = f32.evaluate_logits(x[rows])
        d = [float(np.abs(a[rows].reshape(1024, -1) - b.reshape(1024, -1)).max()) for a, b in ((p, pf), (v, vf), (lg, lf), (vp, vpf))]
        assert max(d) < TOL, d
    f32.close()


def test_one_ply_of_selfplay_run_equals_the_stepwise_rounds():
    """4. of the module text, at N = 15, 128 games, 64 simulations: the run loop's rounds (no k_scan: k_round's counts go to k_group; raw policy rows) against
    round_generate / round_eval / round_scatter + sample + mirror, trees after the ply bit for bit."""
    n, count = 15, 64
    games = SHAPES[n][0]
    dumps = []
    for variant in ("run", "stepwise"):
        eng = _engine(n, games, True, seed=5)
        sp = oa.SelfPlay(eng)
        sp.reset()
        if variant == "run":
            sp.run(count, K, max_plies=1)
        else:
            for rnd in range(count // K):
                sp.round_generate(rnd, K)
                sp.round_eval()
                assert eng.last_plan()["path"] == "difference"
                sp.round_scatter()
            sp.sample_actions(1.0, 30)
            sp.mirror_generate()
            sp.mirror_eval()
            sp.mirror_apply()
        assert sp.ply == 1
        assert eng.stats()["children2_launches"] == count // K  # (every round of the ply ran k_sib_children2: the difference path)
        dumps.append(_dumps(sp, games))
        eng.close()
    _same_dumps(dumps[0], dumps[1], "omok_selfplay_run against step-wise rounds")
