"""GPU tests (run with -m gpu) of the forced-win solver (omok_env_vcf_solve) and the scripted player that uses it (OMOK_OPP_VCF), through
the C ABI, against tests/vcf_solver.py (the rule restated in plain Python, pinned by tests/test_vcf_solver.py) and, for the trees, against
the oracle's self-play object; the forced-win report of records.GameRecords."""
import ctypes as C

import numpy as np
import pytest

import omok_ai_amd as oa
from omok_ai_amd import binding as B
from oracle import oracle as O
import positions as P
import scripted_opponent as SO
import threat_opponent as TO
import vcf_solver as VS

pytestmark = pytest.mark.gpu

SETTINGS = [(8, 4096), (8, 8), (2, 4096), (16, 4096)]


def _solver_engine(n):
    return oa.Engine(board_size=n, games=1, max_nodes=16, max_tables=8, max_batch_k=1)  # (the solver needs no net)


def _inputs(n):
    hand = sorted(VS.hand_made(n).items())
    boards, turns = VS.random_set(n)
    boards = np.concatenate([np.stack([b for _name, (b, _s, _d, _w) in hand]), boards])
    turns = np.concatenate([np.array([s for _name, (_b, s, _d, _w) in hand], dtype=np.uint8), turns])
    return len(hand), boards, turns


_HAND_WANT = {}


def _want(n, depth, budget):
    """the yardstick on the hand-made positions and the random set, computed once per setting"""
    if (n, depth, budget) not in _HAND_WANT:
        hand, boards, turns = _inputs(n)
        _HAND_WANT[(n, depth, budget)] = VS.solve_batch(n, boards[:hand], turns[:hand], depth, budget)[:5]
    return [np.concatenate([h, r]) for h, r in zip(_HAND_WANT[(n, depth, budget)], VS.random_set_want(n, depth, budget)[:5])]


# ---- 1. the solver on caller-held positions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,budget", SETTINGS)
@pytest.mark.parametrize("n", [9, 15])
def test_solver_equals_the_yardstick(n, depth, budget):
    hand, boards, turns = _inputs(n)
    want = _want(n, depth, budget)
    eng = _solver_engine(n)
    got = eng.env_vcf_solve(boards, turns, depth, budget)
    print(f"board {n} D {depth} NB {budget}: {len(boards)} positions, verdicts {[int(np.count_nonzero(want[0] == v)) for v in (-1, 0, 1)]}, "
          f"nodes {int(want[3].sum())}")
    for name, g, w in zip(("verdict", "cell", "moves", "nodes", "pv"), got, want):
        bad = np.flatnonzero(np.any((g != w).reshape(len(boards), -1), axis=1))
        assert len(bad) == 0, f"{name}: {len(bad)} differ, first at position {int(bad[0])} ({g[bad[0]]} != {w[bad[0]]})"
    if (depth, budget) == (8, 4096):
        # the closure of the lines through the engine's own replay: positions an alternating game can be in, with its mover to move
        verdict, cell, moves, nodes, pv = got
        legal = np.flatnonzero((verdict == 1) & (eng.env_check_positions(boards)[0] == 0) & ((np.count_nonzero(boards, axis=1) & 1) == turns))
        assert len(legal) > 10
        length = 2 * moves[legal] - 1
        final, status, played = eng.env_replay(boards[legal], np.where(pv[legal] < 0, 0xFFFF, pv[legal]).astype(np.uint16), length)
        assert np.array_equal(played, length) and np.array_equal(status, np.where(turns[legal] == 0, oa.api.BLACK_WIN, oa.api.WHITE_WIN))
        _f, status, played = eng.env_replay(boards[legal], np.where(pv[legal] < 0, 0xFFFF, pv[legal]).astype(np.uint16), length - 1)
        assert np.array_equal(played, length - 1) and not status.any()  # nothing before the last cell ends the game
        # each output may be NULL; batch 1; a batch that is no multiple of anything
        for keep in range(5):
            outs = [np.full(w.shape, -77, dtype=np.int32) for w in want]
            args = [B.iptr(o) if i == keep else None for i, o in enumerate(outs)]
            assert B.lib().omok_env_vcf_solve(eng.h, B.u8ptr(boards), B.u8ptr(turns), len(boards), depth, budget, *args) == 0
            assert np.array_equal(outs[keep], want[keep]) and all(np.all(o == -77) for i, o in enumerate(outs) if i != keep)
        for first, count in ((hand - 1, 1), (3, 67)):
            part = eng.env_vcf_solve(boards[first:first + count], turns[first:first + count], depth, budget)
            assert all(np.array_equal(g, w[first:first + count]) for g, w in zip(part, want))
    eng.close()


def test_rejected_calls_write_nothing():
    n = 9
    eng = _solver_engine(n)
    boards = np.stack([VS.hand_made(n)["open_three_s0_r4"][0]] * 3)
    turns = np.zeros(3, dtype=np.uint8)
    L = B.lib()

    def call(h, b, t, batch, depth, budget):
        outs = [np.full(3, -77, dtype=np.int32) for _ in range(4)] + [np.full((3, 31), -77, dtype=np.int32)]
        rc = L.omok_env_vcf_solve(h, b, t, batch, depth, budget, *[B.iptr(o) for o in outs])
        assert all(np.all(o == -77) for o in outs)
        return rc

    bp, tp = B.u8ptr(boards), B.u8ptr(turns)
    bad_turns = np.array([0, 1, 2], dtype=np.uint8)
    assert call(eng.h, bp, B.u8ptr(bad_turns), 3, 8, 4096) == -1 and "turns[2]" in L.omok_last_error(eng.h).decode()
    for args in ((None, bp, tp, 3, 8, 4096), (eng.h, None, tp, 3, 8, 4096), (eng.h, bp, None, 3, 8, 4096), (eng.h, bp, tp, 0, 8, 4096),
                 (eng.h, bp, tp, -1, 8, 4096), (eng.h, bp, tp, 3, 0, 4096), (eng.h, bp, tp, 3, 17, 4096), (eng.h, bp, tp, 3, 8, 0),
                 (eng.h, bp, tp, 3, 8, 65537)):
        assert call(*args) == -1, args[3:]
    with pytest.raises(B.OmokError) as ei:
        eng.env_vcf_solve(boards, turns, 17, 4096)
    assert ei.value.code == -1 and "max_depth" in str(ei.value)
    at = lambda x, y: y * n + x  # noqa: E731
    verdict, cell, moves, nodes, pv = eng.env_vcf_solve(boards[:1], turns[:1], 16, 65536)  # the limits themselves are accepted
    assert (int(verdict[0]), int(cell[0]), int(moves[0]), int(nodes[0])) == (1, at(1, 4), 2, 2) and pv.shape == (1, 31)
    assert [int(x[0]) for x in eng.env_vcf_solve(boards[:1], turns[:1], 1, 1)[:4]] == [0, -1, 0, 1]
    eng.close()


# ---- 2. the scripted player on caller-held positions -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [9, 15])
def test_scripted_actions_equal_the_yardstick(n):
    hand, boards, turns = _inputs(n)
    want, solved = [], 0
    for b, t in zip(boards, turns):
        cell, _level, by_solver = VS.scripted_cell(SO.make_env(n, b, int(t)))
        want.append(cell)
        solved += by_solver and cell != TO.scan(SO.make_env(n, b, int(t)))[0]
    assert solved > 0  # the solver's level decides somewhere, and differently from the threat-aware rule
    eng = _solver_engine(n)
    assert np.array_equal(eng.env_scripted_actions(B.OPP_VCF, boards, turns), np.array(want, dtype=np.int32))
    out = np.full(len(boards), -77, dtype=np.int32)
    bad_turns = turns.copy()
    bad_turns[-1] = 2
    assert B.lib().omok_env_scripted_actions(eng.h, B.OPP_VCF, B.u8ptr(boards), B.u8ptr(bad_turns), len(boards), B.iptr(out)) == -1
    assert np.all(out == -77)
    eng.close()


# ---- 3. lockstep with the oracle ------------------------------------------------------------------------------------------------
def _dumps_equal(sp, osp, games, tag):
    for g in range(games):
        for side in (0, 1):
            gi, gf = sp.tree_dump(g, side)
            oi, of = osp.tree_dump(g, side)
            assert gi.shape == oi.shape and np.array_equal(gi, oi), f"{tag}: node records (game {g} side {side})"
            assert np.array_equal(gf.view(np.uint32), of.view(np.uint32)), f"{tag}: w / policy bits (game {g} side {side})"


def _engine(n, games, k, seed, max_nodes=1024, max_tables=512):
    eng = oa.Engine(board_size=n, games=games, max_nodes=max_nodes, max_tables=max_tables, max_batch_k=k, seed=seed)
    eng.load_random_weights(0)
    return eng, oa.SelfPlay(eng)


def _lockstep(n, games, k, count, opponent_side, seed, max_plies, boards=None):
    """tests/test_gpu_threat.py's lockstep with OMOK_OPP_VCF: the scripted moves come from the device and must equal the yardstick's on the
    oracle's environments; the oracle is fed them as external moves and its trees must stay bit-identical.  Returns the (level, solved) of
    the scripted moves and the plies played."""
    eng, sp = _engine(n, games, k, seed)
    root_p = eng.evaluate_p(O.Environment(n).encode_nn_input(0)[None]).reshape(-1)
    osp = O.SelfPlay(n, games, cap_nodes=1024, cap_tables=512, seed=seed)
    if boards is None:
        sp.reset()
        osp.reset(root_p)
        boards = np.zeros((games, n * n), dtype=np.uint8)
    else:
        sp.reset_from(boards)
        turns = (np.count_nonzero(boards, axis=1) & 1).astype(np.uint8)
        rows = eng.evaluate_p(eng.encode_nn_input(boards, turns, B.MODE_PLAYER).reshape(games, -1)).reshape(games, -1)
        P.drive_to(osp, boards, rows, root_p)
    key = O.stream_key(seed, 0)
    envs = [SO.make_env(n, boards[g], int(np.count_nonzero(boards[g])) & 1) for g in range(games)]
    decided, plies = [], 0
    while osp.alive_count > 0 and plies < max_plies:
        alive = [g for g in range(games) if osp.game_alive(g)]
        assert sp.ply == osp.ply
        if (osp.ply & 1) == opponent_side:
            want = np.full(games, -1, dtype=np.int32)
            for g in alive:
                assert envs[g].turn == opponent_side
                want[g], level, solved = VS.move(envs[g], key, osp.game_plies(g), g)
                decided.append((level, solved, int(want[g]) != TO.move(envs[g], key, osp.game_plies(g), g)[0]))
            acts = sp.opponent_actions(B.OPP_VCF)
            assert np.array_equal(acts, want), f"ply {osp.ply}: scripted moves {acts} != {want}"
            osp.set_actions(want)
        else:
            for rnd in range((count + k - 1) // k):
                nreq = sp.round_generate(rnd, k, 0.25, 0.03)
                oin = osp.round_generate(rnd, k, 0.25, 0.03)
                assert nreq == len(oin) and np.array_equal(sp.round_inputs(), oin), f"ply {osp.ply} round {rnd}: requests"
                p, v = sp.round_eval()
                sp.round_scatter()
                osp.round_scatter(p, v)
            acts = sp.sample_actions(1.0, 0)
            assert np.array_equal(acts, osp.sample(1.0, 0)), f"ply {osp.ply}: sample_action(Best)"
        for g in alive:
            assert O.lib().orc_env_place_stone(C.byref(envs[g]), int(acts[g])) >= 0
        nm = sp.mirror_generate()
        assert nm == len(osp.mirror_generate()) == len(alive)
        pm = sp.mirror_eval()
        sp.mirror_apply()
        osp.advance(pm)
        assert osp.error == 0
        plies += 1
        _dumps_equal(sp, osp, games, f"after {plies} plies")
    alive, status, game_plies = sp.game_info()
    assert [int(a) for a in alive] == [osp.game_alive(g) for g in range(games)]
    assert [int(s) for s in status] == [osp.game_status(g) for g in range(games)]
    eng.close()
    return decided, plies


@pytest.mark.parametrize("opponent_side", [0, 1])
def test_vcf_opponent_whole_games_stepwise(opponent_side):
    decided, plies = _lockstep(9, 6, 8, 32, opponent_side, seed=3, max_plies=81)
    print(f"opponent_side {opponent_side}: {plies} plies, {len(decided)} scripted moves, {sum(s for _l, s, _d in decided)} by the solver, "
          f"{sum(d for _l, _s, d in decided)} unlike the threat-aware player's")
    assert any(level >= 6 for level, _s, _d in decided) and any(level <= 2 for level, _s, _d in decided)


def lockstep_positions_15():
    """boards [2][HW] at 15 x 15, Black to move with a forced win in three (vcf_solver.hand_made's chain_m3 and blocking_four, with White
    stones far off on the rows 13 / 14 to even the counts)"""
    n = 15
    at = lambda x, y: y * n + x  # noqa: E731
    boards = []
    for name in ("chain_m3_s0", "blocking_four_s0"):
        b = VS.hand_made(n)[name][0].copy()
        if np.count_nonzero(b == 1) < 6:  # (both games hold 12 stones: all games of an episode share the side to move)
            b[at(7, 12)] = 1
        spare = [at(1, 14), at(5, 14), at(9, 14), at(13, 13), at(11, 11)]
        while np.count_nonzero(b == 1) > np.count_nonzero(b == 2):
            b[spare.pop(0)] = 2
        boards.append(b)
    return np.stack(boards)


def test_vcf_opponent_from_positions_with_a_win_in_three_15():
    boards = lockstep_positions_15()
    for b in boards:  # on the yardstick: the inserted level decides the first move, and not as the threat-aware rule would
        r = VS.solve(15, b, 0, VS.VCF_OPP_DEPTH, VS.VCF_OPP_NODES)
        assert (r.verdict, r.moves) == (1, 3) and r.cell != TO.scan(SO.make_env(15, b, 0))[0]
    decided, plies = _lockstep(15, 2, 16, 64, 0, seed=5, max_plies=6, boards=boards)
    assert decided[0][1:] == (True, True) and decided[1][1:] == (True, True)


# ---- 4. the whole-episode call against the step-wise calls; the forced-win report -------------------------------------------------
def test_versus_run_equals_the_stepwise_calls_and_the_forced_win_report():
    n, games, k, count, seed, opponent_side = 9, 6, 8, 32, 3, 0
    eng_a, a = _engine(n, games, k, seed)
    eng_b, b = _engine(n, games, k, seed)
    a.game_log(True)
    a.reset()
    b.reset()
    res, stats = a.versus_run(B.OPP_VCF, opponent_side, count, k)
    for _ in range(n * n):
        if b.alive_count == 0:
            break
        if (b.ply & 1) == opponent_side:
            b.opponent_actions(B.OPP_VCF)
        else:
            b.execute(count, k)
            b.sample_actions(1.0, 0)
        b.advance()
    for x, y in zip(a.game_info(), b.game_info()):
        assert np.array_equal(x, y)
    _dumps_equal(a, b, games, "end")
    assert sum(res) == games == int(stats["finished"])
    rec = a.game_records()
    rec.verify(eng_a)
    f = rec.forced_wins(eng_a, max_depth=6, max_nodes=4096)
    had = np.zeros(2, dtype=np.int64)
    for g in range(games):
        length = int(rec.lengths[g])
        before, h, d = VS.forced_wins(n, rec.start_boards[g], [int(c) for c in rec.cells[g, :length]], int(rec.status[g]), 6, 4096)
        assert [int(x) for x in f["moves_before"][g, :length]] == before and not f["moves_before"][g, length:].any(), f"game {g}"
        assert [int(x) for x in f["had"][g]] == h and [int(x) for x in f["dropped"][g]] == d, f"game {g}"
        had += h
    print(f"results {res}, had {f['had'].sum(axis=0)}, dropped {f['dropped'].sum(axis=0)}")
    assert had.sum() > 0
    eng_a.close()
    eng_b.close()


def test_kinds_that_are_no_players_stay_rejected():
    n = 9
    eng, sp = _engine(n, 3, 8, seed=1)
    sp.reset()
    boards = np.stack([VS.hand_made(n)["open_three_s0_r4"][0]] * 3)
    turns = np.zeros(3, dtype=np.uint8)
    for bad_kind in (-1, 2, 4, 6):
        with pytest.raises(B.OmokError) as ei:
            sp.opponent_actions(bad_kind)
        assert ei.value.code == -1
        with pytest.raises(B.OmokError) as ei:
            sp.versus_run(bad_kind, 0, 16, 8)
        assert ei.value.code == -1
        with pytest.raises(B.OmokError) as ei:
            eng.env_scripted_actions(bad_kind, boards, turns)
        assert ei.value.code == -1
    assert sp.ply == 0
    eng.close()
