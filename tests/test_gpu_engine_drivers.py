"""GPU tests (run with -m gpu) that pin the behaviour of the engine's host drivers: the whole-episode calls (omok_selfplay_run, a match
episode's run, omok_versus_run) against the step-wise calls and against themselves cut in two, host counters included; the argument checks the
two shared-tree entry points have in common; and the move log on the match and versus paths.  Everything is on the 9 x 9 board with 4-6 games,
K = 8 and 32 simulations: rounds still hold several requests per game and the games end at different plies."""
import ctypes as C

import numpy as np
import pytest

import omok_ai_amd as oa
from omok_ai_amd import binding as B

pytestmark = pytest.mark.gpu

N, K, COUNT = 9, 8, 32
STATE, INVALID = -3, -1
MAX_TREE_WAVES = 16  # common.h
# peak_nodes / peak_tables are left out: every status read samples them, and the step-wise calls read the status more often than a run
COUNTERS = ("sims", "evals", "ply_games", "finished", "round_launches", "tree_bytes")


def _engine(games, seed, log=False, **kw):
    eng = oa.Engine(board_size=N, games=games, max_nodes=1024, max_tables=512, max_batch_k=K, seed=seed, **kw)
    eng.load_random_weights(0)
    sp = oa.SelfPlay(eng)
    if log:
        sp.game_log(True)
    return eng, sp


def _twins(games, seed, net2=False, **kw):
    pair = [_engine(games, seed, **kw), _engine(games, seed, **kw)]
    if net2:
        w2 = oa.weights.init_random(N, seed=1)  # (net 1: random-init seed 0)
        for eng, _ in pair:
            eng.load_weights2(w2)
    return pair


def _same(eng_a, a, eng_b, b, games, tag, counters=COUNTERS):
    for g in range(games):
        for side in (0, 1):
            (ai, af), (bi, bf) = a.tree_dump(g, side), b.tree_dump(g, side)
            assert ai.shape == bi.shape and np.array_equal(ai, bi), f"{tag}: node records (game {g} side {side})"
            assert np.array_equal(af.view(np.uint32), bf.view(np.uint32)), f"{tag}: w / policy bits (game {g} side {side})"
        for x, y in zip(a.replay(g), b.replay(g)):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{tag}: replay of game {g}"
    for x, y in zip(a.game_info(), b.game_info()):
        assert np.array_equal(x, y), f"{tag}: game_info"
    assert a.ply == b.ply, tag
    sa, sb = eng_a.stats(), eng_b.stats()
    print(tag, {c: (sa[c], sb[c]) for c in counters})
    assert {c: sa[c] for c in counters} == {c: sb[c] for c in counters}, tag
    return sa


def _stepwise_selfplay(sp, threshold, plies):
    for _ in range(plies):
        if sp.alive_count == 0:
            break
        sp.execute(COUNT, K)
        sp.sample_actions(1.0, threshold)
        sp.advance()


# ---- 1. the run loop equals the step-wise calls, counters included ------------------------------------------------------------
def test_selfplay_run_equals_the_stepwise_calls_with_counters():
    games = 6
    (eng_a, a), (eng_b, b) = _twins(games, 3)
    for eng in (eng_a, eng_b):
        eng.set_profiling(True)  # (round_launches counts the search rounds' brackets only while the launches are timed)
    a.reset()
    b.reset()
    a.run(COUNT, K, threshold=4, max_plies=5)
    _stepwise_selfplay(b, 4, 5)
    s = _same(eng_a, a, eng_b, b, games, "5 plies")
    assert a.ply == 5 and s["ply_games"] == 5 * games and s["sims"] == 5 * COUNT * games and s["round_launches"] == 5 * COUNT // K
    a.run(COUNT, K, threshold=4)
    _stepwise_selfplay(b, 4, N * N)
    s = _same(eng_a, a, eng_b, b, games, "end")
    alive, _, plies = a.game_info()
    assert not alive.any() and s["finished"] == games and s["ply_games"] == plies.sum()
    assert len(set(int(x) for x in plies)) > 1  # the games ended at different plies
    eng_a.close()
    eng_b.close()


# ---- 2. a run cut in two equals one run ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("match", [False, True])
def test_a_run_cut_in_two_equals_one_run(match):
    games = 6
    (eng_a, a), (eng_b, b) = _twins(games, 5, net2=match)
    for sp in (a, b):
        if match:
            sp.match_reset(games // 2)
        else:
            sp.reset()
    a.run(COUNT, K, threshold=4, max_plies=3)
    assert a.ply == 3
    a.run(COUNT, K, threshold=4)
    b.run(COUNT, K, threshold=4)
    s = _same(eng_a, a, eng_b, b, games, "match" if match else "self-play")
    assert not a.game_info()[0].any() and s["finished"] == games
    if match:  # the per-net rows too
        assert eng_a.net2_info()["evals"] == eng_b.net2_info()["evals"]
    eng_a.close()
    eng_b.close()


# ---- 3. the versus call and the step-wise calls agree on the counters -----------------------------------------------------------------
def _stepwise_versus(sp, kind, opponent_side, plies):
    for _ in range(plies):
        if sp.alive_count == 0:
            break
        if (sp.ply & 1) == opponent_side:
            sp.opponent_actions(kind)
        else:
            sp.execute(COUNT, K)
            sp.sample_actions(1.0, 0)
        sp.advance()


def test_versus_run_equals_the_stepwise_calls_with_counters():
    games = 6
    (eng_a, a), (eng_b, b) = _twins(games, 3)
    a.reset()
    b.reset()
    res, stats = a.versus_run(B.OPP_NAIVE, 0, COUNT, K, max_plies=7)
    assert a.ply == 7 and stats["ply_games"] == 7 * games
    _stepwise_versus(b, B.OPP_NAIVE, 0, 7)
    s = _same(eng_a, a, eng_b, b, games, "7 plies")
    assert s["sims"] == 3 * COUNT * games  # the net's plies only: 1, 3, 5
    for eng, sp in ((eng_a, a), (eng_b, b)):  # the same episode again, to the end
        sp.set_episode(0)
        sp.reset()
        eng.reset_stats()
    res, stats = a.versus_run(B.OPP_NAIVE, 0, COUNT, K)
    _stepwise_versus(b, B.OPP_NAIVE, 0, N * N)
    s = _same(eng_a, a, eng_b, b, games, "end")
    alive, status, plies = a.game_info()
    assert not alive.any() and a.alive_count == 0
    assert res == (int(np.sum(status == oa.api.BLACK_WIN)), int(np.sum(status == oa.api.WHITE_WIN)), int(np.sum(status == oa.api.DRAW)))
    assert sum(res) == games == int(stats["finished"]) == int(s["finished"]) and s["ply_games"] == plies.sum()
    eng_a.close()
    eng_b.close()


# ---- 4. both shared-tree entry points reject the same arguments ---------------------------------------------------------------------
def _shared(eng, recorded, count, k, waves):
    """the raw call (the wrapper of the recorded one sizes its buffers by `waves`); returns (code, error text)"""
    lib = B.lib()
    if not recorded:
        rc = lib.omok_execute_shared(eng.h, count, k, 0.25, 0.03, waves)
    else:
        per, cap = (MAX_TREE_WAVES + 1) * k, count + k
        so, bo = np.zeros((cap, per), dtype=np.uint8), np.zeros((cap, per), dtype=np.uint8)
        gc = np.zeros((cap, 3), dtype=np.int32)
        p, v = np.zeros((cap, eng.hw), dtype=np.float32), np.zeros(cap, dtype=np.float32)
        ng, nr = C.c_int32(), C.c_int32()
        rc = lib.omok_execute_shared_recorded(eng.h, count, k, 0.25, 0.03, waves, B.u8ptr(so), B.u8ptr(bo), B.iptr(gc), B.fptr(p), B.fptr(v), cap,
                                              C.byref(ng), C.byref(nr))
    return rc, lib.omok_last_error(eng.h).decode()


def _both_reject(eng, code, waves, named):
    """both entry points return `code`; named: the text names the function that was called, otherwise the texts are equal"""
    (rc_p, text_p), (rc_r, text_r) = _shared(eng, False, COUNT, K, waves), _shared(eng, True, COUNT, K, waves)
    print(rc_p, text_p, "|", rc_r, text_r)
    assert rc_p == rc_r == code
    if named:
        assert "omok_execute_shared" in text_p and "omok_execute_shared_recorded" not in text_p
        assert "omok_execute_shared_recorded" in text_r
        assert text_p.replace("omok_execute_shared", "omok_execute_shared_recorded") == text_r
    else:
        assert text_p == text_r and text_p


def test_shared_tree_entry_points_reject_the_same_arguments():
    eng, sp = _engine(1, 2, max_tree_waves=2)  # net batch = 2 * K rows
    _both_reject(eng, STATE, 2, named=False)                      # before any reset
    sp.reset()
    before = eng.stats()
    _both_reject(eng, INVALID, 0, named=False)                    # waves = 0
    _both_reject(eng, INVALID, MAX_TREE_WAVES + 1, named=False)   # waves = MAX_TREE_WAVES + 1
    _both_reject(eng, INVALID, 3, named=False)                    # waves * batch_size = 24 > 16 = the net batch
    after = eng.stats()
    assert {c: before[c] for c in COUNTERS} == {c: after[c] for c in COUNTERS} and after["sims"] == 0  # argument checks: nothing was searched
    eng.load_weights2(oa.weights.init_random(N, seed=1))
    sp.match_reset(1)
    _both_reject(eng, STATE, 2, named=True)                       # a match episode
    sp.reset()
    assert eng.stats()["sims"] == 0 and sp.ply == 0
    sp.execute_shared(COUNT, K, waves=2)                          # (and the accepted call still works after the rejected ones)
    assert len(sp.execute_shared_recorded(COUNT, K, waves=2)) == 2
    assert eng.stats()["sims"] == 2 * COUNT
    eng.close()
    eng, sp = _engine(4, 2)
    sp.reset()
    _both_reject(eng, INVALID, 2, named=True)                     # games != 1
    eng.close()


# ---- 5. the move log through the shared paths -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("versus", [False, True])
def test_the_log_changes_nothing_on_the_match_and_versus_paths(versus):
    games = 4
    (eng_a, a), (eng_b, b) = _engine(games, 3, log=True), _engine(games, 3, log=False)
    for eng, sp in ((eng_a, a), (eng_b, b)):
        if versus:
            sp.reset()
            sp.versus_run(B.OPP_NAIVE, 0, COUNT, K, max_plies=4)
        else:
            eng.load_weights2(oa.weights.init_random(N, seed=1))
            sp.match_reset(games // 2)
            sp.run(COUNT, K, threshold=0, max_plies=4)
    s = _same(eng_a, a, eng_b, b, games, "versus" if versus else "match", COUNTERS + ("peak_nodes", "peak_tables"))
    rec = a.game_records()
    assert rec.lengths.sum() == s["ply_games"] == 4 * games
    assert np.array_equal(rec.external, np.broadcast_to((np.arange(rec.hw) < 4) & (np.arange(rec.hw) % 2 == 0) & versus, rec.external.shape))
    rec.verify(eng_a)
    eng_a.close()
    eng_b.close()
