"""GPU tests (run with -m gpu) of the threat-aware scripted player (OMOK_OPP_THREAT): omok_env_threat_scan, omok_env_scripted_actions,
omok_opponent_actions and omok_versus_run with that kind, through the C ABI, against tests/threat_opponent.py (the rule restated in plain
Python, pinned by tests/test_threat_opponent.py) and, for the trees, against the oracle's self-play object; the tactics report of
records.GameRecords and the trainer's evaluate_opponent."""
import ctypes as C
import os

import numpy as np
import pytest

import omok_ai_amd as oa
from omok_ai_amd import binding as B
from oracle import oracle as O
import positions as P
import scripted_opponent as SO
import threat_opponent as TO

pytestmark = pytest.mark.gpu


def _scan_engine(n):
    return oa.Engine(board_size=n, games=1, max_nodes=16, max_tables=8, max_batch_k=1)  # (the scan needs no net)


# ---- 1. the rule on caller-held positions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [9, 15])
def test_scan_and_scripted_actions_on_positions(n):
    hand = sorted(TO.hand_made(n).items())
    boards, turns, want = TO.random_set(n)
    by_side = TO.levels_by_side(turns, want)  # a condition on the inputs, from the yardstick's verdicts alone
    assert by_side[0] >= set(range(1, 7)) and by_side[1] >= set(range(1, 7)) and 7 in (by_side[0] | by_side[1])
    boards = np.concatenate([np.stack([b for _name, (b, _s, _w) in hand]), boards])
    turns = np.concatenate([np.array([s for _name, (_b, s, _w) in hand], dtype=np.uint8), turns])
    want = np.concatenate([np.array([w for _name, (_b, _s, w) in hand], dtype=np.int32), want])
    eng = _scan_engine(n)
    cell, level, count = eng.env_threat_scan(boards, turns)
    got = np.stack([cell, level, count], axis=1)
    bad = np.flatnonzero(np.any(got != want, axis=1))
    print(f"board {n}: {len(boards)} positions, {len(bad)} answers differ; levels {[int(np.count_nonzero(want[:, 1] == lv)) for lv in range(8)]}")
    assert len(bad) == 0, f"first difference at position {int(bad[0])}: (cell, level, count) {got[bad[0]]} != {want[bad[0]]}"
    assert np.array_equal(eng.env_scripted_actions(B.OPP_THREAT, boards, turns), want[:, 0])
    full = np.full((1, n * n), 1, dtype=np.uint8)  # no empty cell: level 0, cell -1 (the stones need not be a game's)
    assert [int(x[0]) for x in eng.env_threat_scan(full, [0])] == [-1, 0, 0]
    # each output may be NULL
    ip = lambda a: B.iptr(a)  # noqa: E731
    for keep in range(3):
        outs = [np.full(len(boards), -77, dtype=np.int32) for _ in range(3)]
        args = [ip(o) if i == keep else None for i, o in enumerate(outs)]
        assert B.lib().omok_env_threat_scan(eng.h, B.u8ptr(boards), B.u8ptr(turns), len(boards), *args) == 0
        assert np.array_equal(outs[keep], want[:, keep]) and all(np.all(o == -77) for i, o in enumerate(outs) if i != keep)
    eng.close()


# ---- 2. lockstep with the oracle ------------------------------------------------------------------------------------------------
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
    """The episode step by step on the engine and on the oracle's self-play object: the scripted moves come from the device
    (omok_opponent_actions(OMOK_OPP_THREAT)) and must equal the yardstick's on the oracle's environments; the oracle is fed them as
    external moves and its trees must stay bit-identical.  Returns (the levels of the scripted moves, plies played)."""
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
    levels, plies = [], 0
    while osp.alive_count > 0 and plies < max_plies:
        alive = [g for g in range(games) if osp.game_alive(g)]
        assert sp.ply == osp.ply
        if (osp.ply & 1) == opponent_side:
            want = np.full(games, -1, dtype=np.int32)
            for g in alive:
                assert envs[g].turn == opponent_side
                want[g], level = TO.move(envs[g], key, osp.game_plies(g), g)
                levels.append(level)
            acts = sp.opponent_actions(B.OPP_THREAT)
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
    assert [int(x) for x in game_plies] == [osp.game_plies(g) for g in range(games)]
    for g in range(games):  # transitions: the net's plies only
        gb, gt, gp, gz = sp.replay(g)
        ob, ot, op, oz = osp.replay(g)
        assert len(gb) == len(ob) and np.all(gt == 1 - opponent_side)
        assert np.array_equal(gb, ob) and np.array_equal(gz, oz) and np.array_equal(gp.view(np.uint32), op.view(np.uint32))
    eng.close()
    return levels, plies


@pytest.mark.parametrize("opponent_side", [0, 1])
def test_threat_opponent_whole_games_stepwise(opponent_side):
    levels, plies = _lockstep(9, 6, 8, 32, opponent_side, seed=3, max_plies=81)
    print(f"opponent_side {opponent_side}: {plies} plies, scripted moves by level {[levels.count(lv) for lv in range(8)]}")
    assert min(levels) <= 5 and 6 in levels


def test_threat_opponent_from_positions_with_threes_15():
    boards, first = TO.lockstep_positions(15)
    levels, plies = _lockstep(15, 4, 16, 64, 0, seed=5, max_plies=8, boards=boards)
    print(f"{plies} plies, scripted moves by level {[levels.count(lv) for lv in range(8)]}")
    assert plies == 8 and levels[:4] == first
    assert min(levels) <= 5 and 6 in levels


# ---- 3. the whole-episode call against the step-wise calls; the move log; the tactics report -----------------------------------
def _stepwise_plies(sp, opponent_side, count, k, plies):
    for _ in range(plies):
        if sp.alive_count == 0:
            break
        if (sp.ply & 1) == opponent_side:
            sp.opponent_actions(B.OPP_THREAT)
        else:
            sp.execute(count, k)
            sp.sample_actions(1.0, 0)
        sp.advance()


@pytest.mark.parametrize("opponent_side", [0, 1])
def test_versus_run_equals_the_stepwise_calls(opponent_side):
    n, games, k, count, seed = 9, 6, 8, 32, 3
    eng_a, a = _engine(n, games, k, seed)
    eng_b, b = _engine(n, games, k, seed)
    a.game_log(True)
    a.reset()
    b.reset()
    res, stats = a.versus_run(B.OPP_THREAT, opponent_side, count, k, max_plies=7)
    assert a.ply == 7 and stats["ply_games"] == 7 * games
    _stepwise_plies(b, opponent_side, count, k, 7)
    _dumps_equal(a, b, games, "7 plies")
    a.set_episode(0)  # the same episode again, to the end in one call
    a.reset()
    res, stats = a.versus_run(B.OPP_THREAT, opponent_side, count, k)
    _stepwise_plies(b, opponent_side, count, k, n * n)
    ia, ib = a.game_info(), b.game_info()
    for x, y in zip(ia, ib):
        assert np.array_equal(x, y)
    alive, status, plies = ia
    assert not alive.any() and a.alive_count == 0
    assert res == (int(np.sum(status == oa.api.BLACK_WIN)), int(np.sum(status == oa.api.WHITE_WIN)), int(np.sum(status == oa.api.DRAW)))
    assert sum(res) == games == int(stats["finished"])
    _dumps_equal(a, b, games, "end")
    for g in range(games):
        for x, y in zip(a.replay(g), b.replay(g)):
            assert x.shape == y.shape and x.tobytes() == y.tobytes()
    # the move log marks the scripted player's moves, and only those, external
    rec = a.game_records()
    rec.verify(eng_a)
    assert np.array_equal(rec.lengths, plies)
    for g in range(games):
        length = int(rec.lengths[g])
        assert [bool(x) for x in rec.external[g, :length]] == [(i & 1) == opponent_side for i in range(length)]
    # the tactics report against the same walk done with the yardstick
    t = rec.tactics(eng_a)
    seen = set()
    for g in range(games):
        length = int(rec.lengths[g])
        levels, missed, unblocked = TO.tactics(n, rec.start_boards[g], [int(c) for c in rec.cells[g, :length]])
        assert [int(x) for x in t["level_before"][g, :length]] == levels and not t["level_before"][g, length:].any(), f"game {g}"
        assert [int(x) for x in t["missed_win"][g]] == missed and [int(x) for x in t["unblocked"][g]] == unblocked, f"game {g}"
        assert missed[opponent_side] == 0  # the scripted player takes its win (a block it cannot miss either, but two fives need two blocks)
        seen |= set(levels)
    print(f"opponent_side {opponent_side}: results {res}, missed wins {t['missed_win'].sum(axis=0)}, unblocked {t['unblocked'].sum(axis=0)}, levels seen {sorted(seen)}")
    eng_a.close()
    eng_b.close()


def test_tactics_command_prints_the_totals(tmp_path, capsys):
    n, games, k = 9, 4, 8
    eng, sp = _engine(n, games, k, seed=2)
    sp.game_log(True)
    sp.reset()
    sp.versus_run(B.OPP_THREAT, 0, 16, k)
    rec = sp.game_records(meta={"kind": "evaluate", "opponent": "threat"})
    t = rec.tactics(eng)
    eng.close()
    path = str(tmp_path / "games.npz")
    rec.save(path)
    from omok_ai_amd import records as R
    assert R.main(["tactics", path]) == 0
    out = capsys.readouterr().out
    import json
    line = [ln for ln in out.splitlines() if ln.startswith("tactics: ")]
    assert len(line) == 1 and '"opponent": "threat"' in out
    tot = json.loads(line[0][len("tactics: "):])
    assert tot["games"] == games and tot["moves"] == int(rec.lengths.sum())
    for s, name in ((0, "black"), (1, "white")):
        assert tot[name]["missed_win"] == int(t["missed_win"][:, s].sum()) and tot[name]["unblocked"] == int(t["unblocked"][:, s].sum())
    assert tot["black"]["missed_win"] == 0  # Black was the scripted player


# ---- 4. rejections ---------------------------------------------------------------------------------------------------------------
def test_rejections():
    n = 9
    eng, sp = _engine(n, 3, 8, seed=1)
    sp.reset()
    boards = np.stack([TO.hand_made(n)["lone_s0"][0]] * 3)
    turns = np.zeros(3, dtype=np.uint8)
    for bad_kind in (-1, 2, 4):  # still no players
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
    # a turns byte of 2, or a NULL pointer: OMOK_ERR_INVALID with nothing written
    L = B.lib()
    outs = [np.full(3, -77, dtype=np.int32) for _ in range(3)]
    bad_turns = np.array([0, 1, 2], dtype=np.uint8)
    assert L.omok_env_threat_scan(eng.h, B.u8ptr(boards), B.u8ptr(bad_turns), 3, *[B.iptr(o) for o in outs]) == -1
    assert "turns[2]" in L.omok_last_error(eng.h).decode()
    assert L.omok_env_scripted_actions(eng.h, B.OPP_THREAT, B.u8ptr(boards), B.u8ptr(bad_turns), 3, B.iptr(outs[0])) == -1
    assert L.omok_env_threat_scan(eng.h, None, B.u8ptr(turns), 3, *[B.iptr(o) for o in outs]) == -1
    assert L.omok_env_threat_scan(eng.h, B.u8ptr(boards), None, 3, *[B.iptr(o) for o in outs]) == -1
    assert L.omok_env_threat_scan(eng.h, B.u8ptr(boards), B.u8ptr(turns), 0, *[B.iptr(o) for o in outs]) == -1
    assert L.omok_env_threat_scan(None, B.u8ptr(boards), B.u8ptr(turns), 3, *[B.iptr(o) for o in outs]) == -1
    assert all(np.all(o == -77) for o in outs)
    # kinds 0 and 1 keep ignoring turns
    assert np.array_equal(eng.env_scripted_actions(B.OPP_NAIVE, boards, bad_turns), [-1, -1, -1])
    assert np.array_equal(eng.env_scripted_actions(B.OPP_RANDOM, boards, bad_turns), [-1, -1, -1])
    assert [int(x[0]) for x in eng.env_threat_scan(boards[:1], turns[:1])] == [-1, 6, 8]  # (the engine still answers)
    # a match episode: OMOK_ERR_STATE for the scripted calls; the scan needs no episode
    eng.load_weights2(oa.weights.init_random(n, seed=1))
    sp.match_reset(2)
    with pytest.raises(B.OmokError) as ei:
        sp.opponent_actions(B.OPP_THREAT)
    assert ei.value.code == -3
    with pytest.raises(B.OmokError) as ei:
        sp.versus_run(B.OPP_THREAT, 0, 16, 8)
    assert ei.value.code == -3
    assert [int(x[0]) for x in eng.env_threat_scan(boards[:1], turns[:1])] == [-1, 6, 8]
    eng.close()


# ---- 5. the trainer's evaluation games ------------------------------------------------------------------------------------------
def test_trainer_evaluates_against_the_threat_player(tmp_path):
    from omok_ai_amd import records as R
    from omok_ai_amd import trainer as TR
    n, games = 9, 4
    save_dir = str(tmp_path / "saves")
    p = TR.Parameters(model_name="tiny", episode_count=2, evaluate_count=16, evaluate_batch_size=8, evaluate_opponent="threat", evaluate_games=games,
                      test_evaluate_count=16)
    tr = TR.Trainer(p, board_size=n, seed=3, save_dir=save_dir, precision_rows=0)
    os.makedirs(save_dir, exist_ok=True)
    tr.engine.save(os.path.join(save_dir, p.model_name))  # evaluate() plays with the weights file of the iteration
    tr.iteration = 1
    path = str(tmp_path / "eval.npz")
    counts = tr.evaluate(save_games=path)
    assert sum(counts) == games
    assert tr.last_evaluation["opponent"] == "threat" and tr.last_evaluation["games"] == games
    rec = R.load(path)
    assert rec.meta["opponent"] == "threat" and rec.games == games
    twin_eng, twin = _engine(n, games, 8, seed=4)  # the same games through the C ABI: kind 3, the trainer's streams (seed + 1)
    twin_eng.load(os.path.join(save_dir, p.model_name))
    twin.reset()
    res, _ = twin.versus_run(B.OPP_THREAT, 0, 16, 8)
    assert res == counts
    twin_eng.close()
    tr.close()


def test_trainer_rejects_an_unknown_evaluate_opponent(tmp_path):
    from omok_ai_amd import trainer as TR
    for name in ("Naive", "", "search"):
        with pytest.raises(ValueError) as ei:
            TR.Trainer(TR.Parameters(evaluate_opponent=name), board_size=9, save_dir=str(tmp_path / "saves"))
        assert "evaluate_opponent" in str(ei.value)
    assert TR.Parameters().evaluate_opponent == "naive"
