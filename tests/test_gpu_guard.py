"""GPU tests (run with -m gpu) of the defending scripted player (OMOK_OPP_GUARD) and omok_env_guard_scan, through the C ABI, against
tests/guard_opponent.py (the rule restated in plain Python, pinned by tests/test_guard_opponent.py) and, for the trees, against the oracle's
self-play object.  The yardstick's games and scan results are computed once per process (guard_opponent.games / want) and shared."""
import ctypes as C

import numpy as np
import pytest

import omok_ai_amd as oa
from omok_ai_amd import binding as B
from oracle import oracle as O
import guard_opponent as GO
import scripted_opponent as SO
import vcf_defence as VD
import vcf_solver as VS

pytestmark = pytest.mark.gpu

NAMES = ("cell", "step", "level", "count")


def _scan_engine(n):
    return oa.Engine(board_size=n, games=1, max_nodes=16, max_tables=8, max_batch_k=1)  # (the scan needs no net)


def _engine(n, games, k, seed, max_nodes=1024, max_tables=512):
    eng = oa.Engine(board_size=n, games=games, max_nodes=max_nodes, max_tables=max_tables, max_batch_k=k, seed=seed)
    eng.load_random_weights(0)
    return eng, oa.SelfPlay(eng)


def _steps_of(want, draws):
    return [(int(r[1]), int(r[2]), ((int(x) * int(r[3])) >> 32) > 0) for r, x in zip(want, draws)]


# ---- 1. the scan on caller-held positions -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,budget", GO.BUDGETS)
@pytest.mark.parametrize("n", [9, 15])
def test_scan_equals_the_yardstick(n, depth, budget):
    boards, turns, draws = GO.scan_set(n)
    eng = _scan_engine(n)
    for drawn in (False, True):
        want = GO.want(n, depth, budget, drawn)
        got = eng.env_guard_scan(boards, turns, draws if drawn else None, depth, budget)
        print(f"board {n} D {depth} NB {budget} drawn {drawn}: {len(boards)} positions, steps {np.bincount(want[:, 1], minlength=6).tolist()}")
        for i, name in enumerate(NAMES):
            bad = np.flatnonzero(got[name] != want[:, i])
            assert len(bad) == 0, f"{name}: {len(bad)} differ, first at position {int(bad[0])} ({got[name][bad[0]]} != {want[bad[0], i]})"
    if (depth, budget) == GO.BUDGETS[0]:
        # the hand-made positions at their own budgets; each output may be NULL; batch 1 and a batch that is no multiple of anything
        for name, (board, side, d, nb, expect) in sorted(GO.hand_made(n).items()):
            got = eng.env_guard_scan(board[None], np.array([side], dtype=np.uint8), None, d, nb)
            assert tuple(int(got[k][0]) for k in NAMES) == expect, name
        want = GO.want(n, depth, budget, True)
        u32 = draws.ctypes.data_as(C.POINTER(C.c_uint32))
        for keep in range(4):
            outs = [np.full(len(boards), -77, dtype=np.int32) for _ in range(4)]
            args = [B.iptr(o) if i == keep else None for i, o in enumerate(outs)]
            assert B.lib().omok_env_guard_scan(eng.h, B.u8ptr(boards), B.u8ptr(turns), u32, len(boards), depth, budget, *args) == 0
            assert np.array_equal(outs[keep], want[:, keep]) and all(np.all(o == -77) for i, o in enumerate(outs) if i != keep)
        for first, count in ((3, 1), (5, 67)):
            part = eng.env_guard_scan(boards[first:first + count], turns[first:first + count], draws[first:first + count], depth, budget)
            assert all(np.array_equal(part[name], want[first:first + count, i]) for i, name in enumerate(NAMES))
        full = np.full((2, n * n), 2, dtype=np.uint8)  # step 0: no empty cell
        got = eng.env_guard_scan(full, np.array([0, 1], dtype=np.uint8))
        assert all(got[name].tolist() == [v, v] for name, v in zip(NAMES, (-1, 0, 0, 0)))
    eng.close()


@pytest.mark.parametrize("n", [9, 15])
def test_the_scan_inputs_are_not_vacuous(n):
    """on the yardstick alone: over the budgets of test 1 every step occurs, step 3 with a level <= 5 and with level 6, and a draw with r > 0"""
    _boards, _turns, draws = GO.scan_set(n)
    steps = []
    for depth, budget in GO.BUDGETS:
        steps += _steps_of(GO.want(n, depth, budget, True), draws) + _steps_of(GO.want(n, depth, budget, False), np.zeros_like(draws))
    GO.assert_not_vacuous(steps)


# ---- 2. omok_env_scripted_actions(OMOK_OPP_GUARD); rejected calls -------------------------------------------------------------------
@pytest.mark.parametrize("n", [9, 15])
def test_scripted_actions_equal_the_scan_without_draws(n):
    boards, turns, _draws = GO.scan_set(n)
    want = GO.want(n, GO.D_OPP, GO.NB_OPP, False)
    eng = _scan_engine(n)
    forced = eng.env_scripted_actions(B.OPP_GUARD, boards, turns)
    assert np.array_equal(forced, np.where(want[:, 3] == 0, want[:, 0], -1))
    assert np.count_nonzero(forced >= 0) > 10 and np.count_nonzero(forced < 0) > 10
    eng.close()


def test_rejected_calls_write_nothing():
    n = 9
    eng = _scan_engine(n)
    boards = np.stack([GO.hand_made(n)["map_safe_s0"][0]] * 3)
    turns = np.zeros(3, dtype=np.uint8)
    bad_turns = np.array([0, 1, 2], dtype=np.uint8)
    L = B.lib()

    def scan(h, b, t, batch, depth, budget):
        outs = [np.full(3, -77, dtype=np.int32) for _ in range(4)]
        rc = L.omok_env_guard_scan(h, b, t, None, batch, depth, budget, *[B.iptr(o) for o in outs])
        assert all(np.all(o == -77) for o in outs)
        return rc

    def forced(h, b, t, batch):
        out = np.full(3, -77, dtype=np.int32)
        rc = L.omok_env_scripted_actions(h, B.OPP_GUARD, b, t, batch, B.iptr(out))
        assert np.all(out == -77)
        return rc

    bp, tp = B.u8ptr(boards), B.u8ptr(turns)
    assert scan(eng.h, bp, B.u8ptr(bad_turns), 3, 6, 256) == -1 and "turns[2]" in L.omok_last_error(eng.h).decode()
    assert forced(eng.h, bp, B.u8ptr(bad_turns), 3) == -1 and "turns[2]" in L.omok_last_error(eng.h).decode()
    for args in ((eng.h, bp, tp, 0, 6, 256), (eng.h, bp, tp, -1, 6, 256), (eng.h, None, tp, 3, 6, 256), (eng.h, bp, None, 3, 6, 256),
                 (eng.h, bp, tp, 3, 0, 256), (eng.h, bp, tp, 3, 17, 256), (eng.h, bp, tp, 3, 6, 0), (eng.h, bp, tp, 3, 6, 4097)):
        assert scan(*args) == -1, args[3:]
    for args in ((eng.h, bp, tp, 0), (eng.h, None, tp, 3), (eng.h, bp, None, 3)):
        assert forced(*args) == -1, args[3:]
    with pytest.raises(B.OmokError) as ei:
        eng.env_guard_scan(boards, turns, None, 6, 4097)
    assert ei.value.code == -1 and "max_nodes" in str(ei.value)
    got = eng.env_guard_scan(boards[:1], turns[:1], None, 16, 4096)  # the limits themselves are accepted
    assert int(got["step"][0]) == 3 and int(got["count"][0]) >= 1
    eng.close()


# ---- 3. the episode form: the three passes on device-resident roots with the device's own Philox words ------------------------------------
def _episode(n, guard_side, log=False):
    """a search-free episode of the guard (guard_side) against OMOK_OPP_VCF, every move chosen on the device and compared with the yardstick's
    game; returns (engine, self-play object) after the last ply"""
    seed, games = GO.GAMES[n]
    want = GO.games(n)[guard_side]
    eng, sp = _engine(n, games, 8, seed, max_nodes=64, max_tables=32)
    kinds = (B.OPP_GUARD, B.OPP_VCF) if guard_side == 0 else (B.OPP_VCF, B.OPP_GUARD)
    if log:
        sp.game_log(True)
    sp.reset()
    for ply in range(n * n):
        if sp.alive_count == 0:
            break
        acts = sp.opponent_actions(kinds[ply & 1])
        expect = [moves[ply] if ply < len(moves) else -1 for _p, moves, _s, _l in want]
        assert acts.tolist() == expect, f"ply {ply}: {acts.tolist()} != {expect}"
        sp.advance()
    alive, status, plies = sp.game_info()
    assert not alive.any() and status.tolist() == [s for _p, _m, s, _l in want] and plies.tolist() == [len(m) for _p, m, _s, _l in want]
    return eng, sp


@pytest.mark.parametrize("guard_side", [0, 1])
@pytest.mark.parametrize("n", [9, 15])
def test_search_free_episodes_equal_the_yardsticks_games(n, guard_side):
    if n == 9:
        GO.assert_not_vacuous(GO.game_steps(n))  # steps 1..5, step 3 with levels 4 and 6, a draw with r > 0
    else:  # at 15 x 15 no position of these games runs out of budget: steps 1, 2, 3 and 5, step 3 with levels 4, 5 and 6
        steps = GO.game_steps(n)
        assert {1, 2, 3, 5} <= {s for s, _l, _r in steps} and {4, 5, 6} <= {l for s, l, _r in steps if s == 3} and any(r for _s, _l, r in steps)
    eng, _sp = _episode(n, guard_side)
    eng.close()


# ---- 4. lockstep with the oracle ----------------------------------------------------------------------------------------------------
def _dumps_equal(sp, osp, games, tag):
    for g in range(games):
        for side in (0, 1):
            gi, gf = sp.tree_dump(g, side)
            oi, of = osp.tree_dump(g, side)
            assert gi.shape == oi.shape and np.array_equal(gi, oi), f"{tag}: node records (game {g} side {side})"
            assert np.array_equal(gf.view(np.uint32), of.view(np.uint32)), f"{tag}: w / policy bits (game {g} side {side})"


def test_guard_opponent_in_lockstep_with_the_oracle():
    """the guard (Black) against the net's search: its moves come from the device and must equal the yardstick's on the oracle's environments;
    the oracle is fed them as external moves and its trees must stay bit-identical after every ply"""
    n, games, k, count, opponent_side, seed = 9, 6, 8, 32, 0, 3
    eng, sp = _engine(n, games, k, seed)
    root_p = eng.evaluate_p(O.Environment(n).encode_nn_input(0)[None]).reshape(-1)
    osp = O.SelfPlay(n, games, cap_nodes=1024, cap_tables=512, seed=seed)
    sp.reset()
    osp.reset(root_p)
    key = O.stream_key(seed, 0)
    envs = [SO.make_env(n, np.zeros(n * n, dtype=np.uint8), 0) for _g in range(games)]
    steps, plies = [], 0
    while osp.alive_count > 0 and plies < n * n:
        alive = [g for g in range(games) if osp.game_alive(g)]
        assert sp.ply == osp.ply
        if (osp.ply & 1) == opponent_side:
            want = np.full(games, -1, dtype=np.int32)
            for g in alive:
                assert envs[g].turn == opponent_side
                want[g], step, _level, _count = GO.move(envs[g], GO.draw_word(key, osp.game_plies(g), g, opponent_side))
                steps.append(step)
            acts = sp.opponent_actions(B.OPP_GUARD)
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
    alive, status, _game_plies = sp.game_info()
    assert [int(a) for a in alive] == [osp.game_alive(g) for g in range(games)]
    assert [int(s) for s in status] == [osp.game_status(g) for g in range(games)]
    print(f"{plies} plies, guard moves per step {np.bincount(steps, minlength=6).tolist()}")
    assert 1 in steps and 2 in steps
    eng.close()


# ---- 5. the whole-episode call against the step-wise calls; the defence report of the guard's games --------------------------------------
def test_versus_run_equals_the_stepwise_calls():
    n, games, k, count, seed, opponent_side = 9, 6, 8, 32, 3, 0
    eng_a, a = _engine(n, games, k, seed)
    eng_b, b = _engine(n, games, k, seed)
    a.reset()
    b.reset()
    res, stats = a.versus_run(B.OPP_GUARD, opponent_side, count, k)
    for _ in range(n * n):
        if b.alive_count == 0:
            break
        if (b.ply & 1) == opponent_side:
            b.opponent_actions(B.OPP_GUARD)
        else:
            b.execute(count, k)
            b.sample_actions(1.0, 0)
        b.advance()
    for x, y in zip(a.game_info(), b.game_info()):
        assert np.array_equal(x, y)
    _dumps_equal(a, b, games, "end")
    assert sum(res) == games == int(stats["finished"])
    eng_a.close()
    eng_b.close()


def test_the_defence_report_of_the_guards_games():
    """the guard-against-VCF episode of test 3 with the move log on: the records replay, the report equals the walk of the yardstick game by
    game, and the guard's side concedes nothing although it is threatened"""
    n, guard_side = 9, 0
    eng, sp = _episode(n, guard_side, log=True)
    rec = sp.game_records()
    rec.verify(eng)
    f = rec.vcf_defence(eng, max_depth=GO.D_OPP, max_nodes=GO.NB_OPP)
    sums = {name: np.zeros(2, dtype=np.int64) for name in VD.NAMES}
    for g in range(rec.games):
        length = int(rec.lengths[g])
        before, want = VD.report(n, rec.start_boards[g], [int(c) for c in rec.cells[g, :length]], int(rec.status[g]), GO.D_OPP, GO.NB_OPP)
        assert [int(x) for x in f["threat_before"][g, :length]] == before, f"game {g}"
        for name in VD.NAMES:
            assert f[name][g].tolist() == want[name], (g, name)
            sums[name] += want[name]
    print(", ".join(f"{name} {v.tolist()}" for name, v in sums.items()))
    assert sums["conceded"][guard_side] == 0 and sums["threatened"][guard_side] > 0
    eng.close()


# ---- 6. kinds that are no players; the match episode; the trainer's parameter ------------------------------------------------------------
def test_kinds_that_are_no_players_stay_rejected(tmp_path):
    from omok_ai_amd import trainer as TR
    n = 9
    eng, sp = _engine(n, 3, 8, seed=1)
    sp.reset()
    boards = np.stack([VS.hand_made(n)["open_three_s0_r4"][0]] * 3)
    turns = np.zeros(3, dtype=np.uint8)
    for bad_kind in (-1, 6, 8):
        with pytest.raises(B.OmokError) as ei:
            sp.opponent_actions(bad_kind)
        assert ei.value.code == -1 and "OMOK_OPP_GUARD" in str(ei.value)
        with pytest.raises(B.OmokError) as ei:
            sp.versus_run(bad_kind, 0, 16, 8)
        assert ei.value.code == -1
        with pytest.raises(B.OmokError) as ei:
            eng.env_scripted_actions(bad_kind, boards, turns)
        assert ei.value.code == -1
    assert sp.ply == 0
    eng.load_weights2(oa.weights.init_random(n, seed=1))
    sp.match_reset(2)
    with pytest.raises(B.OmokError) as ei:  # a match episode has no scripted player
        sp.opponent_actions(B.OPP_GUARD)
    assert ei.value.code == -3
    with pytest.raises(B.OmokError) as ei:
        sp.versus_run(B.OPP_GUARD, 0, 16, 8)
    assert ei.value.code == -3
    eng.close()
    small = dict(model_name="tiny", episode_count=2, evaluate_count=16, evaluate_batch_size=8, test_evaluate_count=16, evaluate_games=2)
    tr = TR.Trainer(TR.Parameters(evaluate_opponent="guard", **small), board_size=n, seed=3, save_dir=str(tmp_path / "saves"), precision_rows=0)
    tr.close()
    with pytest.raises(ValueError) as ei:
        TR.Trainer(TR.Parameters(evaluate_opponent="Guard", **small), board_size=n, save_dir=str(tmp_path / "saves"))
    assert "evaluate_opponent" in str(ei.value)
