"""GPU tests (run with -m gpu) of the episodes that start from given positions: omok_env_check_positions, omok_selfplay_reset_from and
omok_root_stats through the C ABI, against tests/positions.py (the verdicts restated through the oracle's place_stone; the oracle's
self-play object driven to the positions by external moves -- the construction tests/test_position_yardstick.py pins on the CPU)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import omok_ai_amd as oa
from omok_ai_amd import binding as B
from oracle import oracle as O
import positions as P
import scripted_opponent as SO
from helpers import random_positions
from test_gpu_versus import _dumps_equal, _engine

pytestmark = pytest.mark.gpu

CONFIGS = [(9, 5, 8, 32, 3), (15, 3, 16, 48, 2)]  # board, games, K, count, plies of the search-parity run
STONES = [1, 2, 7, 8]                              # both sides to move
SEED = 6


@pytest.fixture(scope="module")
def pool():
    """engines shared by the tests of this module, one per (board, games, K): every test starts its own episode on them"""
    made = {}

    def get(n, games, k, **kw):
        key = (n, games, k, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = _engine(n, games, k, SEED, max_nodes=256, max_tables=128, **kw)
        return made[key]

    yield get
    for eng, _sp in made.values():
        eng.close()


@functools.lru_cache(maxsize=None)
def _cpu_net(n):
    return O.Net(n, oa.weights.init_random(n, seed=0))  # the weights of Engine.load_random_weights(0)


def _raw_rows(eng, boards):
    """the engine's raw Player-mode policy rows of the positions: omok_encode_nn_input + ONE omok_evaluate_pv call of G rows"""
    turns = (np.count_nonzero(boards, axis=1) & 1).astype(np.uint8)
    x = eng.encode_nn_input(boards, turns, B.MODE_PLAYER).reshape(len(boards), -1)
    assert np.array_equal(x, P.input_rows(eng.n, boards))
    return x, eng.evaluate_p(x).reshape(len(boards), -1)


def _start(get, n, games, k, stones, episode=0):
    """the engine reset to `games` quiet positions of `stones` stones, and the oracle driven to them with the engine's rows"""
    eng, sp = get(n, games, k)
    boards = P.quiet(n, games, stones, seed=11)
    sp.set_episode(episode)
    sp.reset_from(boards)
    x, rows = _raw_rows(eng, boards)
    root_p = eng.evaluate_p(O.Environment(n).encode_nn_input(0)[None]).reshape(-1)
    osp = O.SelfPlay(n, games, cap_nodes=256, cap_tables=128, seed=SEED)
    osp.set_episode(episode)
    P.drive_to(osp, boards, rows, root_p)
    return eng, sp, osp, boards, x, rows


def _dumps_equal_from_position(sp, osp, games, tag):
    """bit-identical trees, with the one integer masked in which a fresh agent differs from the oracle's root: node 0's `action` (the
    oracle's root remembers the last external move) -- valid until the first re-rooting"""
    for g in range(games):
        for side in (0, 1):
            gi, gf = sp.tree_dump(g, side)
            oi, of = osp.tree_dump(g, side)
            assert gi.shape == oi.shape, f"{tag}: node count (game {g} side {side})"
            assert gi[0, 1] == -1, f"{tag}: a fresh agent's root has no action (game {g} side {side})"
            oi = oi.copy()
            oi[0, 1] = -1
            assert np.array_equal(gi, oi), f"{tag}: node records (game {g} side {side})"
            assert np.array_equal(gf.view(np.uint32), of.view(np.uint32)), f"{tag}: w / policy bits (game {g} side {side})"


# ---- 1. k_position_check against the restatement ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _check_set(n):
    boards = [b for _name, (b, _v) in sorted(P.hand_made(n).items())]
    boards += [b for _name, b in sorted(P.edge_positions(n).items())]
    boards += [b for _name, b in sorted(P.straddling_fives(n).items())]
    boards += list(P.decode_inputs(n, random_positions(n, 300, seed=21)))
    rng = np.random.default_rng([22, n])
    for stones in rng.integers(0, 30, 120):  # sparse boards: mostly legal, both sides to move
        b = np.zeros(n * n, dtype=np.uint8)
        cells = rng.permutation(n * n)[:stones]
        b[cells[0::2]] = O.BLACK
        b[cells[1::2]] = O.WHITE
        boards.append(b)
    boards = np.stack(boards)
    return boards, P.verdicts(n, boards)


@pytest.mark.parametrize("n", [9, 15])
def test_position_check(pool, n):
    boards, (want_v, want_s) = _check_set(n)
    hist = np.bincount(want_v, minlength=5)
    print(f"board {n}: {len(boards)} positions, verdicts 0..4: {hist.tolist()}")
    assert np.all(hist >= 1)  # (a condition on the inputs: every verdict occurs)
    eng, _sp = pool(n, 1, 8)
    got_v, got_s = oa.Environment.check_positions(eng, boards)
    bad = np.flatnonzero((got_v != want_v) | (got_s != want_s))
    print(f"board {n}: {len(bad)} of {len(boards)} answers differ" + (f", first at {int(bad[0])}: {got_v[bad[0]]} / {want_v[bad[0]]}" if len(bad) else ""))
    assert np.array_equal(got_v, want_v) and np.array_equal(got_s, want_s)
    one_v, one_s = eng.env_check_positions(boards[:1])  # batch of one, stones_out NULL
    assert one_v[0] == want_v[0]
    v = np.zeros(1, dtype=np.int32)
    assert B.lib().omok_env_check_positions(eng.h, B.u8ptr(boards[:1].copy()), 1, B.iptr(v), None) == 0 and v[0] == want_v[0]
    assert B.lib().omok_env_check_positions(eng.h, B.u8ptr(boards[:1].copy()), 0, B.iptr(v), None) == -1


# ---- 2. the state a position reset leaves --------------------------------------------------------------------------------------
@pytest.mark.parametrize("stones", STONES)
@pytest.mark.parametrize("n,games,k,count,plies", CONFIGS)
def test_reset_state(pool, n, games, k, count, plies, stones):
    eng, sp, osp, boards, x, rows = _start(pool, n, games, k, stones)
    _dumps_equal_from_position(sp, osp, games, f"{stones} stones")
    for g in range(games):  # (the oracle was fed ONE omok_evaluate_pv call over the G rows: equal trees = those rows, masked and renormalised)
        want = P.masked_renormalised(boards[g], rows[g])
        for side in (0, 1):
            ints, floats = sp.tree_dump(g, side)
            assert ints.shape == (1, 8) and np.array_equal(floats[0, 1:].view(np.uint32), want.view(np.uint32))
            assert (int(ints[0, 3]), int(ints[0, 4])) == (stones & 1, n * n - stones)
            assert sp.tree_root(g, side) == (0, 0.0, 1, 0)
    alive, status, game_plies = sp.game_info()
    assert np.all(alive == 1) and np.all(status == oa.api.IN_PROGRESS) and np.all(game_plies == stones)
    assert sp.ply == stones == osp.ply and sp.alive_count == games
    assert all(len(sp.replay(g)[0]) == 0 for g in range(games))
    p_cpu, _ = _cpu_net(n).forward(x, threads=4)
    err = float(np.abs(rows - p_cpu).max())
    print(f"board {n}, {stones} stones: max |p - oracle/net.c| = {err:.2e}")
    assert err < 1e-3  # the project's contract on evaluate_p


# ---- 3. search parity from a position ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stones", STONES)
@pytest.mark.parametrize("n,games,k,count,plies", CONFIGS)
def test_search_parity_from_a_position(pool, n, games, k, count, plies, stones):
    eng, sp, osp, boards, _x, _rows = _start(pool, n, games, k, stones)
    equal = _dumps_equal_from_position
    sampled = []
    for ply in range(plies):
        for rnd in range((count + k - 1) // k):
            nreq = sp.round_generate(rnd, k, 0.25, 0.03)
            oin = osp.round_generate(rnd, k, 0.25, 0.03)
            assert nreq == len(oin) and np.array_equal(sp.round_inputs(), oin), f"ply {ply} round {rnd}: request boards"
            equal(sp, osp, games, f"ply {ply} round {rnd} generate")
            p, v = sp.round_eval()
            sp.round_scatter()
            osp.round_scatter(p, v)
            equal(sp, osp, games, f"ply {ply} round {rnd} scatter")
        pi, has = sp.compute_policy()
        for g in range(games):
            want = osp.compute_policy(g)
            assert bool(has[g]) == (want is not None)
            if want is not None:
                assert np.array_equal(pi[g].view(np.uint32), want.view(np.uint32)), f"ply {ply}: compute_policy (game {g})"
        acts = sp.sample_actions(1.0, 30)
        assert np.array_equal(acts, osp.sample(1.0, 30)), f"ply {ply}: sampled actions"
        sampled.append(acts)
        nm, om = sp.mirror_generate(), osp.mirror_generate()
        assert nm == len(om) and np.array_equal(sp.mirror_inputs(), om)
        pm = sp.mirror_eval()
        sp.mirror_apply()
        osp.advance(pm)
        assert osp.error == 0
        equal = _dumps_equal  # re-rooted: the roots' actions are the moves just played, on both sides
        equal(sp, osp, games, f"ply {ply} advance")
    assert sp.ply == stones + plies == osp.ply
    for g in range(games):  # replay tuples: only the moves sampled after the reset
        gb, gt, gp, gz = sp.replay(g)
        ob, ot, op, oz = osp.replay(g)
        assert len(gb) == len(ob) <= plies and (len(gb) == plies or not osp.game_alive(g))
        assert np.array_equal(gb, ob) and np.array_equal(gt, ot) and np.array_equal(gz, oz)
        assert np.array_equal(gp.view(np.uint32), op.view(np.uint32))
        if len(gb):
            assert np.array_equal(gb[0], boards[g]) and gt[0] == (stones & 1)


# ---- 4. empty positions are the ordinary reset -----------------------------------------------------------------------------------
def _two_plies(sp, games, count, k):
    out = [[sp.tree_dump(g, s) for g in range(games) for s in (0, 1)]]
    for _ in range(2):
        sp.execute(count, k)
        out.append(sp.sample_actions(1.0, 30))
        sp.advance()
        out.append([sp.tree_dump(g, s) for g in range(games) for s in (0, 1)])
    return out


def _same(a, b):
    if not isinstance(a, (np.ndarray, list, tuple)):
        return a == b
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("n,games,k,count,plies", CONFIGS)
def test_empty_positions_take_the_ordinary_reset(pool, n, games, k, count, plies):
    eng, sp = pool(n, games, k)
    sp.set_episode(2)
    sp.reset()
    want = _two_plies(sp, games, count, k)
    sp.set_episode(2)
    sp.reset_from(np.zeros((games, n * n), dtype=np.uint8))
    assert sp.ply == 0
    got = _two_plies(sp, games, count, k)
    assert _same(got, want)


# ---- 5. rejections leave the engine as it was ------------------------------------------------------------------------------------
def _snapshot(sp, games):
    return ([sp.tree_dump(g, s) for g in range(games) for s in (0, 1)], list(sp.game_info()), sp.ply, [list(sp.replay(g)) for g in range(games)])


def test_rejections_leave_the_engine_untouched(pool):
    n, games, k, count = 9, 5, 8, 16
    eng, sp = pool(n, games, k)
    hand = P.hand_made(n)
    sp.set_episode(0)
    sp.reset()  # episode 0; the next reset takes stream 1
    sp.execute(count, k)
    sp.sample_actions(1.0, 30)
    sp.advance()
    before = _snapshot(sp, games)
    cases = [("bad_byte", 1), ("white_ahead", 2), ("five_diagonal_white", 3), ("full_board", 4)]
    for name, v in cases:
        board, pinned = hand[name]
        assert pinned == v
        boards = P.quiet(n, games, 2, seed=3)
        boards[2] = board
        with pytest.raises(B.OmokError) as ei:
            sp.reset_from(boards)
        print(ei.value)
        assert ei.value.code == -5 and "game 2" in str(ei.value) and f"verdict {v}" in str(ei.value)
    boards = P.quiet(n, games, 2, seed=3)
    boards[3] = P.quiet(n, 1, 4, seed=4)[0]
    with pytest.raises(B.OmokError) as ei:  # unequal stone counts
        sp.reset_from(boards)
    print(ei.value)
    assert ei.value.code == -1 and "game 3" in str(ei.value)
    boards[0] = hand["bad_byte"][0]  # a verdict comes before the counts
    with pytest.raises(B.OmokError) as ei:
        sp.reset_from(boards)
    assert ei.value.code == -5 and "game 0" in str(ei.value)
    assert _same(_snapshot(sp, games), before)
    # the episode counter: the next reset is episode 1, as on an engine that never saw the rejected calls

    def first_ply():
        sp.execute(count, k)
        return [sp.sample_actions(1.0, 30), [sp.tree_dump(g, s) for g in range(games) for s in (0, 1)]]

    sp.reset()
    got = first_ply()
    sp.set_episode(1)
    sp.reset()
    want = first_ply()
    sp.set_episode(7)  # (where the counter would stand had each of the six rejected calls taken a stream)
    sp.reset()
    other = first_ply()
    assert _same(got, want) and not _same(got, other)


# ---- 6. what follows a position reset ---------------------------------------------------------------------------------------------
def test_execute_shared_from_a_position(pool):
    n, k, count = 9, 8, 32
    eng, sp = pool(n, 1, k, max_tree_waves=1)
    board = P.quiet(n, 1, 7, seed=5)
    sp.set_episode(0)
    sp.reset_from(board)
    sp.execute(count, k)
    want = [sp.tree_dump(0, s) for s in (0, 1)]
    sp.set_episode(0)
    sp.reset_from(board)
    sp.execute_shared(count, k, waves=1)
    assert sp.tree_root(0, 1)[0] == count  # (7 stones: White's tree was searched)
    assert _same([sp.tree_dump(0, s) for s in (0, 1)], want)


@pytest.mark.parametrize("n,games,k,count,plies", CONFIGS)
def test_play_actions_and_root_stats_from_a_position(pool, n, games, k, count, plies):
    eng, sp, osp, boards, _x, _rows = _start(pool, n, games, k, 7)
    sp.execute(count, k)
    rn, rw = sp.root_stats()
    side = sp.ply & 1
    for g in range(games):
        n_g, w_g, _nn, _nt = sp.tree_root(g, side)
        assert int(rn[g]) == n_g == count and np.float32(rw[g]).view(np.uint32) == np.float32(w_g).view(np.uint32)
    eng, sp, osp, boards, _x, _rows = _start(pool, n, games, k, 7)
    for step in range(2):
        acts = np.array([int(np.flatnonzero(boards[g] == 0)[3 * g + step]) for g in range(games)], dtype=np.int32)
        osp.set_actions(acts)
        pm = eng.evaluate_p(osp.mirror_generate())  # the same rows omok_play_actions evaluates inside the engine
        sp.play_actions(acts)
        osp.advance(pm.reshape(len(pm), -1))
        assert osp.error == 0
        _dumps_equal(sp, osp, games, f"external move {step}")
    assert sp.ply == 9 and all(len(sp.replay(g)[0]) == 0 for g in range(games))
    rn, rw = sp.root_stats()
    assert np.all(rn == 0) and np.all(rw == 0.0)


def test_run_slots_refuses_a_position_reset(pool):
    import torch
    n, games, k = 9, 5, 8
    eng, sp = pool(n, games, k)
    sp.reset_from(P.quiet(n, games, 2, seed=3))
    rec = sp.replay_record_bytes()
    buf = torch.empty(64 * rec, dtype=torch.uint8, device="cuda")
    with pytest.raises(B.OmokError) as ei:
        sp.run_slots(games + 2, 16, k, buf.data_ptr(), 64)
    assert ei.value.code == -3


def test_versus_run_from_a_position():
    """omok_versus_run in one call from 2-stone positions (Black = the naive player moves first) against the step-wise calls beside the
    oracle, the scripted moves checked against tests/scripted_opponent.py as tests/test_gpu_versus.py does"""
    n, games, k, count, seed, kind, opponent_side, max_plies = 9, 6, 8, 16, 3, B.OPP_NAIVE, 0, 6
    boards = P.quiet(n, games, 2, seed=8)
    eng_a, a = _engine(n, games, k, seed)
    a.reset_from(boards)
    res, stats = a.versus_run(kind, opponent_side, count, k, max_plies=max_plies)
    eng_b, b = _engine(n, games, k, seed)
    b.reset_from(boards)
    _x, rows = _raw_rows(eng_b, boards)
    root_p = eng_b.evaluate_p(O.Environment(n).encode_nn_input(0)[None]).reshape(-1)
    osp = O.SelfPlay(n, games, cap_nodes=1024, cap_tables=512, seed=seed)
    P.drive_to(osp, boards, rows, root_p)
    key = O.stream_key(seed, 0)
    envs = [SO.make_env(n, boards[g], 0) for g in range(games)]
    plies = 0
    while osp.alive_count > 0 and plies < max_plies:
        alive = [g for g in range(games) if osp.game_alive(g)]
        if (osp.ply & 1) == opponent_side:
            want = np.full(games, -1, dtype=np.int32)
            for g in alive:
                assert envs[g].turn == opponent_side
                want[g], _forced = SO.move(kind, envs[g], key, osp.game_plies(g), g)
            acts = b.opponent_actions(kind)
            assert np.array_equal(acts, want), f"ply {osp.ply}: scripted moves {acts} != {want}"
            osp.set_actions(want)
        else:
            for rnd in range((count + k - 1) // k):
                nreq = b.round_generate(rnd, k, 0.25, 0.03)
                oin = osp.round_generate(rnd, k, 0.25, 0.03)
                assert nreq == len(oin) and np.array_equal(b.round_inputs(), oin)
                p, v = b.round_eval()
                b.round_scatter()
                osp.round_scatter(p, v)
            acts = b.sample_actions(1.0, 0)
            assert np.array_equal(acts, osp.sample(1.0, 0))
        for g in alive:
            assert O.lib().orc_env_place_stone(C.byref(envs[g]), int(acts[g])) >= 0
        assert b.mirror_generate() == len(osp.mirror_generate())
        pm = b.mirror_eval()
        b.mirror_apply()
        osp.advance(pm)
        assert osp.error == 0
        _dumps_equal(b, osp, games, f"ply {osp.ply}")
        plies += 1
    assert a.ply == osp.ply == 2 + plies and stats["ply_games"] > 0
    _dumps_equal(a, osp, games, "versus_run")
    alive, status, game_plies = a.game_info()
    assert [int(x) for x in alive] == [osp.game_alive(g) for g in range(games)]
    assert [int(x) for x in status] == [osp.game_status(g) for g in range(games)]
    assert [int(x) for x in game_plies] == [osp.game_plies(g) for g in range(games)]
    done = status[alive == 0]
    assert res == (int(np.sum(done == oa.api.BLACK_WIN)), int(np.sum(done == oa.api.WHITE_WIN)), int(np.sum(done == oa.api.DRAW)))
    for g in range(games):  # transitions: the net's plies only (White)
        for x, y in zip(a.replay(g), osp.replay(g)):
            assert x.shape == y.shape and np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
        assert np.all(a.replay(g)[1] == 1 - opponent_side)
    with pytest.raises(B.OmokError) as ei:  # moves were played since the reset
        a.versus_run(kind, opponent_side, count, k)
    assert ei.value.code == -3
    a.reset_from(boards)  # Black to move and opponent_side = 1: the episode starts with a search
    a.versus_run(B.OPP_RANDOM, 1, count, k, max_plies=1)
    assert a.ply == 3 and all(len(a.replay(g)[0]) == 1 and a.replay(g)[1][0] == 0 for g in range(games))
    eng_a.close()
    eng_b.close()


# ---- 7. analysis ----------------------------------------------------------------------------------------------------------------
def test_analyze_finds_the_win_in_one():
    n, count, k = 9, 64, 8
    board, win = P.win_in_one(n)
    eng, _sp = _engine(n, 1, k, seed=2)
    pi, root_n, root_w = oa.api.analyze(eng, board[None], count, k)
    order = np.argsort(pi[0])[::-1]
    print(f"win at {win}: pi = {pi[0][win]:.3f}, runner-up cell {int(order[1])}: {pi[0][order[1]]:.3f}, root n = {int(root_n[0])}, w = {float(root_w[0]):.3f}")
    assert int(order[0]) == win and pi[0][win] > pi[0][order[1]]
    assert int(root_n[0]) == count
    assert np.all(pi[0][board != 0] == 0.0) and abs(float(pi[0].sum()) - 1.0) < 1e-5
    eng.close()


# ---- 8. the trainer's evaluation games from openings ---------------------------------------------------------------------------
def test_trainer_evaluation_games_from_openings(tmp_path):
    from omok_ai_amd import trainer as TR
    n, games = 9, 6
    save_dir = str(tmp_path / "saves")
    p = TR.Parameters(model_name="tiny", episode_count=2, evaluate_count=16, evaluate_batch_size=8, evaluate_games=games, test_evaluate_count=16)
    tr = TR.Trainer(p, board_size=n, seed=3, save_dir=save_dir, precision_rows=0)
    os.makedirs(save_dir, exist_ok=True)
    tr.engine.save(os.path.join(save_dir, p.model_name))  # evaluate() plays with the weights file of the iteration
    tr.iteration = 1
    openings = P.quiet(n, games, 2, seed=9)
    counts = tr.evaluate(openings=openings)
    assert sum(counts) == games and tr.last_evaluation["games"] == games
    assert tr.evaluate(openings=openings) == counts  # the same streams, the same games
    openings[4] = P.hand_made(n)["five_row_black"][0]
    with pytest.raises(B.OmokError) as ei:
        tr.evaluate(openings=openings)
    assert ei.value.code == -5 and "game 4" in str(ei.value)
    tr.close()
