"""Lazy policy rows: the run loop's rounds launch no softmax / scatter kernel.  The net's heads write a request's logits into its node's policy row,
the backups mark the node raw (has_policy = 2), and the wave that first reads the row -- the root's noise, a descent through the node once it is fully expanded --
turns it into the probabilities with the eager kernel's arithmetic.

Every GPU case runs two fresh engines with the same seed, one with omok_debug_set_lazy_policy on (the default) and one with it off, and requires EQUALITY IN EVERY
BIT of omok_tree_dump (ints and floats, has_policy included: the dump materialises what is still raw) for a sample of games and both sides, of the game status, and
of the replay tuples (boards, turns, pi, z: the boards hold every sampled action).  No tolerance is involved.

The tail class of a run-loop round is a function of the host's bound on its rows (live games x K) only, so it is read with omok_debug_last_plan from one step-wise
round of the same bound at the end of a run.  At N = 15, K = 16 the three bounds give: 64 games -> the 8-way split-K tail (k_splitk_logits), 512 games -> the 4-way
split-K tail, 1040 games (16640 rows > 16384) -> the whole-K launch (k_tail_fused).  With OMOK_GEMM_W unset k_gemm_t's EPI_LOGITS instantiation writes no logits row
at all; the cases with it set take it (N = 9) and k_gemm_w's (N = 15)."""
import os

import numpy as np
import pytest

import omok_ai_amd as oa
from omok_ai_amd import binding as B
from oracle import oracle as O
import positions as P
from helpers import draw_sequence

MODE = B.NET_F16X3_MIXED  # (a set operand format: no probe at commit)
DENSE_K, DENSE_EMPTY = 8, (6, 5, 3)  # K - 2 or fewer empty cells: a node fills up within one round


def _dense_positions(n, games, empty, seed=11):
    """boards [games][HW] with `empty` empty cells: random subsets of the five-free colouring of helpers.draw_sequence (a subset of runs <= 4 holds no five), Black
    to move or White by the parity of the stones"""
    seq = draw_sequence(n)
    black, white = np.array(seq[0::2]), np.array(seq[1::2])
    stones = n * n - empty
    rng = np.random.default_rng([seed, n, games, empty])
    boards = np.zeros((games, n * n), dtype=np.uint8)
    for g in range(games):
        boards[g][rng.choice(black, (stones + 1) // 2, replace=False)] = O.BLACK
        boards[g][rng.choice(white, stones // 2, replace=False)] = O.WHITE
    return boards


@pytest.mark.parametrize("empty", DENSE_EMPTY)
def test_dense_positions_are_legal(empty):
    """No GPU: the positions of the descent-site case are legal positions of games in progress (no five, not full) with the empty-cell count the case relies on."""
    n, games = 9, 8
    boards = _dense_positions(n, games, empty)
    assert empty <= DENSE_K - 2
    for b in boards:
        assert int(np.count_nonzero(b == 0)) == empty
        assert P.verdict(n, b) == (P.LEGAL, n * n - empty)
    assert len({b.tobytes() for b in boards}) > 1


def _engine(n, games, k, lazy, max_nodes=512, max_tables=128, seed=21):
    eng = oa.Engine(board_size=n, games=games, max_nodes=max_nodes, max_tables=max_tables, max_batch_k=k, seed=seed, net_mode=MODE)
    eng.load_weights(oa.weights.init_random(n, seed=4))
    eng.set_lazy_policy(lazy)
    return eng


def _state(sp, sample):
    """everything the cases compare, as a dict of arrays"""
    out = {}
    for g in sample:
        for side in (0, 1):
            ints, floats = sp.tree_dump(g, side)
            out[f"ints g{g} s{side}"] = ints
            out[f"floats g{g} s{side}"] = floats.view(np.uint32)
        for name, a in zip(("boards", "turns", "pi", "z"), sp.replay(g)):
            out[f"replay {name} g{g}"] = a.view(np.uint32) if a.dtype == np.float32 else a.copy()
    alive, status, plies = sp.game_info()
    out["alive"], out["status"], out["plies"] = alive, status, plies
    return out


def _same(a, b, tag):
    assert a.keys() == b.keys()
    for key in a:
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), f"{tag}: {key} differs"


def _sample(games):
    return sorted({0, 1, games // 2, games - 1})


def _pair(n, games, k, script, **kw):
    """script(sp, eng) -> state, on a lazy engine and an eager one; returns (lazy state, the lazy engine's counters, the eager engine's)"""
    res = []
    for lazy in (True, False):
        eng = _engine(n, games, k, lazy, **kw)
        sp = oa.SelfPlay(eng)
        st = script(sp, eng)
        res.append((st, eng.lazy_policy_stats()))
        eng.close()
    _same(res[0][0], res[1][0], f"n={n} games={games} k={k}")
    assert res[1][1] == {"noise": 0, "descent": 0}, res[1][1]  # (the eager engine never leaves a raw row)
    return res[0][0], res[0][1]


def _has_policy(state):
    return np.concatenate([v[:, 7] >> 16 for key, v in state.items() if key.startswith("ints")])


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,sims", [(9, 8, 16), (15, 16, 32)])
def test_noise_site(n, k, sims):
    """The root never fills up in so few simulations.  A tree is re-rooted twice between two of its searches: to the child its own search chose, then to that child's
    child for the opponent's move, which a search this shallow never created -- ensure_action_exists makes it from the mirror evaluation, and in a run loop's lazy
    ply that evaluation stays logits too.  So from its second search on every tree's root is raw when it meets the noise."""
    games = 8

    def script(sp, eng):
        sp.reset()
        sp.run(sims, k, max_plies=6)
        return _state(sp, range(games))

    st, cnt = _pair(n, games, k, script)
    print(f"noise site n={n}: {cnt}")
    assert set(np.unique(_has_policy(st)).tolist()) <= {0, 1}  # (the dump shows no raw mark)
    assert cnt["noise"] > 0


@pytest.mark.gpu
def test_noise_site_on_deep_trees():
    """Six empty cells, 64 simulations: the search expands whole subtrees, the opponent's reply exists below the chosen child, and the root the next search of the
    tree starts from is a node that was evaluated in a lazy round and never filled up: the noise site materialises it."""
    n, games = 9, 8

    def script(sp, eng):
        sp.reset_from(_dense_positions(n, games, 6))
        sp.run(64, DENSE_K, max_plies=4)
        return _state(sp, range(games))

    _, cnt = _pair(n, games, DENSE_K, script)
    print(f"noise site on deep trees: {cnt}")
    assert cnt["noise"] > 0 and cnt["descent"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("empty", DENSE_EMPTY)
def test_descent_site(empty):
    """Positions with at most K - 2 empty cells: a node fills up within one round and the next round's descents pass through its raw row."""
    n, games = 9, 8

    def script(sp, eng):
        sp.reset_from(_dense_positions(n, games, empty))
        sp.run(64, DENSE_K, max_plies=2)
        return _state(sp, range(games))

    st, cnt = _pair(n, games, DENSE_K, script)
    print(f"descent site, {empty} empty cells: {cnt}")
    assert cnt["descent"] > 0


def _plan_of_bound(sp, eng, k):
    """the plan of one step-wise round with the run loop's row bound (live games x K)"""
    sp.round_generate(0, k, 0.25, 0.03)
    sp.round_eval()
    return eng.last_plan()


@pytest.mark.gpu
@pytest.mark.parametrize("games,tsplit,path", [(64, 8, "copy"), (512, 4, "difference"), (1040, 1, "difference")])
def test_the_producers(games, tsplit, path):
    """N = 15, K = 16, 32 simulations, 2 plies on the three tail classes (module text) and on both paths of the sibling rounds."""
    n, k = 15, 16
    plans = []

    def script(sp, eng):
        sp.reset()
        sp.run(32, k, max_plies=2)
        st = _state(sp, _sample(games))
        plans.append(_plan_of_bound(sp, eng, k))
        return st

    _, cnt = _pair(n, games, k, script, max_nodes=160, max_tables=48)
    print(f"producers, {games} games: {plans[0]} {cnt}")
    for plan in plans:
        assert plan["rows"] == games * k and plan["tsplit"] == tsplit and plan["path"] == path, plan


@pytest.mark.gpu
@pytest.mark.parametrize("n,games,k", [(15, 520, 32), (9, 520, 32)])  # (16640 rows: above the 16384 up to which the tail splits K)
def test_the_producers_of_the_wave_private_gemm(n, games, k):
    """OMOK_GEMM_W=1 (read at every forward) sends whole-K rounds through k_gemm_w<8, EPI_LOGITS> (N = 15) and k_gemm_t<4, EPI_LOGITS> (N = 9) instead of k_tail_fused."""
    plans = []

    def script(sp, eng):
        sp.reset()
        sp.run(2 * k, k, max_plies=2)
        st = _state(sp, _sample(games))
        plans.append(_plan_of_bound(sp, eng, k))
        return st

    old = os.environ.get("OMOK_GEMM_W")
    os.environ["OMOK_GEMM_W"] = "1"
    try:
        _, cnt = _pair(n, games, k, script, max_nodes=160, max_tables=48)
    finally:
        if old is None:
            del os.environ["OMOK_GEMM_W"]
        else:
            os.environ["OMOK_GEMM_W"] = old
    for plan in plans:
        assert plan["tsplit"] == 1, plan  # (whole K: the launches the variable selects)


@pytest.mark.gpu
def test_dumps_change_nothing():
    """A dump in mid-episode materialises raw rows early: dumping then 2 more plies equals 2 more plies without the dump, and two dumps in a row are equal."""
    n, games, k = 9, 8, 8

    def with_dump(sp, eng):
        sp.reset()
        sp.run(16, k, max_plies=3)
        first = _state(sp, range(games))
        _same(first, _state(sp, range(games)), "two dumps in a row")
        sp.run(16, k, max_plies=2)
        return _state(sp, range(games))

    def without(sp, eng):
        sp.reset()
        sp.run(16, k, max_plies=3)
        sp.run(16, k, max_plies=2)
        return _state(sp, range(games))

    a, _ = _pair(n, games, k, with_dump)
    b, _ = _pair(n, games, k, without)
    _same(a, b, "dump in mid-episode")


@pytest.mark.gpu
def test_rerooting_carries_raw_rows():
    """3 plies of 16 simulations (k_advance moves raw rows with the surviving nodes), then 2 plies of 128 simulations that descend through them."""
    n, games, k = 9, 8, 8

    def script(sp, eng):
        sp.reset()
        sp.run(16, k, max_plies=3)
        sp.run(128, k, max_plies=2)
        return _state(sp, range(games))

    _, cnt = _pair(n, games, k, script)
    print(f"re-rooting: {cnt}")


@pytest.mark.gpu
def test_eager_modes_stay_eager():
    """With the switch on, a match episode and a step-wise ply never take the lazy path: the parent's bits (the engine with the switch off), both counters 0."""
    n, games, k = 9, 8, 8

    def match(sp, eng):
        eng.load_weights2(oa.weights.init_random(n, seed=5))
        sp.match_reset(games // 2)
        sp.run(16, k, threshold=0, max_plies=3)
        return _state(sp, range(games))

    def stepwise(sp, eng):
        sp.reset()
        sp.execute(16, k)
        actions = sp.sample_actions()
        sp.advance()
        for rnd in range(2):
            if sp.round_generate(rnd, k, 0.25, 0.03):
                sp.round_eval()
            sp.round_scatter()
        st = _state(sp, range(games))
        st["actions"] = actions
        return st

    for script in (match, stepwise):
        _, cnt = _pair(n, games, k, script)
        assert cnt == {"noise": 0, "descent": 0}, (script.__name__, cnt)
