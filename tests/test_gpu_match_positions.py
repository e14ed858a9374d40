"""GPU tests (run with -m gpu) of the matches from given positions and of the random openings: omok_match_reset_from and
omok_env_random_positions through the C ABI, and match.run_match(openings=...).

Yardsticks (pinned on the CPU by tests/test_match_positions_yardstick.py): tests/match_harness.py's MatchComposition with both instances
driven to the positions by positions.drive_to, instance x fed net x's raw rows of the positions; tests/random_openings.py."""
import functools

import numpy as np
import pytest

import omok_ai_amd as oa
from omok_ai_amd import binding as B
from omok_ai_amd import match as M
from oracle import oracle as O
from match_harness import MatchComposition
import positions as P
import random_openings as RO
from test_gpu_match import _episode, _match_engine, _same_episode
from test_gpu_positions import _same

pytestmark = pytest.mark.gpu

SEED, OFFSET = 7, 5
SHAPE_A = (9, 8, 3, 8)    # board, games, split, K
SHAPE_B = (15, 4, 2, 16)
KEYS = (O.stream_key(5, 0), 0xC0FFEE0123456789)


@functools.lru_cache(maxsize=None)
def _weights(n, seed):
    return oa.weights.init_random(n, seed=seed)


# ---- 1. random openings -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bare():
    """engines WITHOUT a net, one per board size: omok_env_random_positions needs none"""
    made = {n: oa.Engine(board_size=n, games=1, max_nodes=8, max_tables=4, max_batch_k=8) for n in (9, 15)}
    yield made
    for eng in made.values():
        eng.close()


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("n,stones", [(9, 0), (9, 1), (9, 8), (9, 50), (9, 80), (15, 1), (15, 100)])
def test_random_positions_equal_the_yardstick(bare, n, stones, key):
    eng, batch = bare[n], 256
    want_b, want_ok = RO.positions(n, key, 0, stones, batch)
    got_b, got_ok = oa.Environment.random_positions(eng, key, 0, stones, batch)
    ended = int(np.sum(want_ok == 0))
    bad = np.flatnonzero(np.any(got_b != want_b, axis=1) | (got_ok != want_ok))
    print(f"board {n}, {stones} stones, key {key:#x}: {ended} of {batch} games ended on the way; {len(bad)} positions differ"
          + (f", first {int(bad[0])}" if len(bad) else ""))
    assert got_b.dtype == np.uint8 and got_ok.dtype == np.uint8
    assert np.array_equal(got_b, want_b) and np.array_equal(got_ok, want_ok)
    if (n, stones) in ((9, 50), (15, 100)):
        assert 0.15 * batch <= ended <= 0.85 * batch  # (both classes occur: the stop rule is exercised)
    elif stones < 9:
        assert ended == 0  # (five in a line needs Black's fifth stone, the ninth of the game)
    else:  # 80 of 81 cells: a game that has ended by stone 50 has ended by stone 80, so no fewer end; nearly all do
        assert 0.15 * batch <= ended
    tail_b, tail_ok = oa.Environment.random_positions(eng, key, 5, stones, batch - 5)  # a range may be cut anywhere
    assert np.array_equal(tail_b, got_b[5:]) and np.array_equal(tail_ok, got_ok[5:])
    verdict, count = oa.Environment.check_positions(eng, got_b)
    keep = got_ok == 1
    assert np.all(verdict[keep] == 0) and np.all(count[keep] == stones)
    assert np.all(verdict[~keep] == 3) and np.all(count[~keep] <= stones)


def test_random_positions_errors_and_state(bare):
    eng = bare[9]
    hw = 81
    boards, ok = np.zeros((4, hw), dtype=np.uint8), np.zeros(4, dtype=np.uint8)
    call = lambda stones, batch: B.lib().omok_env_random_positions(eng.h, 1, 0, stones, batch, B.u8ptr(boards), B.u8ptr(ok))  # noqa: E731
    assert call(hw, 4) == -1 and call(-1, 4) == -1 and call(3, 0) == -1
    assert not boards.any() and not ok.any()
    assert call(hw - 1, 4) == 0 and call(3, 1) == 0
    with pytest.raises(B.OmokError) as ei:  # (no net: the engine still refuses what needs one)
        oa.SelfPlay(eng).reset()
    assert ei.value.code == -3
    a, _ = eng.env_random_positions(KEYS[0], 1 << 40, 6, 3)  # ids beyond 2^31: the low 32 bits of 2 id + side key the draws
    assert np.array_equal(a, RO.positions(9, KEYS[0], 1 << 40, 6, 3)[0])


# ---- 2. the state a match position reset leaves ---------------------------------------------------------------------------------
def _slot1_rows(n, games, k, mode, tensors, x):
    """evaluate_p of the rows x, and of the empty board, by an engine that holds `tensors` in slot 1"""
    e = oa.Engine(board_size=n, games=games, max_nodes=256, max_tables=128, max_batch_k=k, net_mode=mode)
    e.load_weights(tensors)
    rows = e.evaluate_p(x).reshape(len(x), -1)
    root = e.evaluate_p(O.Environment(n).encode_nn_input(0)[None]).reshape(-1)
    e.close()
    return rows, root


def _start(n, games, split, k, stones, mode=B.NET_F16X3, episode=0):
    """(engine, SelfPlay after omok_match_reset_from, the driven composition, boards, [R_1, R_2])"""
    w = [_weights(n, 1), _weights(n, 2)]
    eng = _match_engine(n, games, k, mode, w[0], w[1], seed=SEED, game_offset=OFFSET, max_nodes=256, max_tables=128)
    sp = oa.SelfPlay(eng)
    boards = P.quiet(n, games, stones, seed=11)
    x = P.input_rows(n, boards)
    rows, roots = [None, None], [None, None]
    rows[0] = eng.evaluate_p(x).reshape(games, -1)  # ONE omok_evaluate_pv call of the G rows on this engine
    roots[0] = eng.evaluate_p(O.Environment(n).encode_nn_input(0)[None]).reshape(-1)
    rows[1], roots[1] = _slot1_rows(n, games, k, mode, w[1], x)
    assert not np.array_equal(rows[0], rows[1])
    comp = MatchComposition(n, games, split, roots[0], roots[1], seed=SEED, game_offset=OFFSET, cap_nodes=256, cap_tables=128)
    for i in range(2):
        comp.O[i].set_episode(episode)
        P.drive_to(comp.O[i], boards, rows[i], roots[i])
    eng.reset_stats()
    sp.set_episode(episode)
    sp.match_reset_from(split, boards)
    return eng, sp, comp, boards, rows


def _compare(sp, comp, games, tag, fresh_roots):
    """bit-identical trees; fresh_roots: node 0's `action` is masked (the driven oracle's root remembers the last external move, a fresh
    agent's has none) -- until the first re-rooting"""
    for g in range(games):
        for side in (0, 1):
            gi, gf = sp.tree_dump(g, side)
            oi, of = comp.tree_dump(g, side)
            assert gi.shape == oi.shape, f"{tag}: node count (game {g} side {side})"
            if fresh_roots:
                assert gi[0, 1] == -1, f"{tag}: a fresh agent's root has no action (game {g} side {side})"
                oi = oi.copy()
                oi[0, 1] = -1
            assert np.array_equal(gi, oi), f"{tag}: node records (game {g} side {side})"
            assert np.array_equal(gf.view(np.uint32), of.view(np.uint32)), f"{tag}: w / policy bits (game {g} side {side})"
            assert sp.tree_root(g, side)[:2] == comp.tree_root(g, side)[:2], f"{tag}: root n / w (game {g} side {side})"


@pytest.mark.parametrize("shape,stones", [(SHAPE_A, 3), (SHAPE_A, 4), (SHAPE_B, 5)])
def test_reset_state(shape, stones):
    n, games, split, k = shape
    eng, sp, comp, boards, rows = _start(n, games, split, k, stones)
    _compare(sp, comp, games, f"{stones} stones", True)
    for g in range(games):
        for side in (0, 1):
            owner = side ^ (1 if g >= split else 0)
            want = P.masked_renormalised(boards[g], rows[owner][g])
            ints, floats = sp.tree_dump(g, side)
            assert ints.shape == (1, 8) and np.array_equal(floats[0, 1:].view(np.uint32), want.view(np.uint32)), f"game {g} side {side}: the owner's row"
            assert (int(ints[0, 0]), int(ints[0, 3]), int(ints[0, 4]), int(ints[0, 5]), int(ints[0, 6])) == (-1, stones & 1, n * n - stones, 0, 0)
            assert sp.tree_root(g, side) == (0, 0.0, 1, 0)
    alive, status, game_plies = sp.game_info()
    assert np.all(alive == 1) and np.all(status == oa.api.IN_PROGRESS) and np.all(game_plies == stones)
    assert sp.ply == stones == comp.ply and sp.alive_count == games
    rn, rw = sp.root_stats()
    assert np.all(rn == 0) and np.all(rw == 0.0)
    assert all(len(sp.replay(g)[0]) == 0 for g in range(games))
    assert tuple(eng.net2_info()["evals"]) == (games, games)  # each net evaluated all G positions
    eng.close()


# ---- 3. search from the reset state ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stones", [3, 4])
def test_search_from_the_reset_state(stones):
    n, games, split, k = SHAPE_A
    count, plies = 32, 2
    eng, sp, comp, boards, _rows = _start(n, games, split, k, stones)
    fresh = True
    for ply in range(plies):
        for rnd in range(count // k):
            nreq = sp.round_generate(rnd, k, 0.25, 0.03)
            cx, _cg = comp.round_generate(rnd, k, 0.25, 0.03)
            assert nreq == len(cx) and np.array_equal(sp.round_inputs(), cx), f"ply {ply} round {rnd}: request rows in the harness's order"
            _compare(sp, comp, games, f"ply {ply} round {rnd} generate", fresh)
            p, v = sp.round_eval()  # (omok_round_eval + omok_round_outputs: the engine's p, v go to the harness)
            sp.round_scatter()
            comp.round_scatter(p, v)
            _compare(sp, comp, games, f"ply {ply} round {rnd} scatter", fresh)
        assert comp.error == 0
        a = sp.sample_actions(1.0, 0)
        assert np.array_equal(a, comp.sample(1.0, 0)), f"ply {ply}: actions"
        nm = sp.mirror_generate()
        om = comp.mirror_generate(a)
        assert nm == len(om) and np.array_equal(sp.mirror_inputs(), om), f"ply {ply}: mirror rows"
        pm = sp.mirror_eval()
        sp.mirror_apply()
        comp.advance(pm)
        fresh = False  # re-rooted: the roots' actions are the moves just played, on both sides
        _compare(sp, comp, games, f"ply {ply} advance", fresh)
    assert sp.ply == stones + plies == comp.ply
    for g in range(games):  # the first record is the opening, moved on by the side the position gives the move to
        gb, gt, _gp, _gz = sp.replay(g)
        assert len(gb) == plies and np.array_equal(gb[0], boards[g]) and gt[0] == (stones & 1)
    eng.close()


# ---- 4. the same weights in both slots: self-play from the positions ----------------------------------------------------------------
def test_same_weights_in_both_slots_is_selfplay_from_the_positions():
    n, games, k, count, stones, plies = 9, 8, 8, 32, 4, 3
    w = _weights(n, 3)
    boards = P.quiet(n, games, stones, seed=12)
    ref = oa.Engine(board_size=n, games=games, max_nodes=1024, max_tables=512, max_batch_k=k, seed=11)
    ref.load_weights(w)
    rsp = oa.SelfPlay(ref)
    rsp.reset_from(boards)
    rsp.run(count, k, threshold=0, max_plies=plies)
    want = _episode(rsp, games), [rsp.tree_dump(g, s) for g in range(games) for s in (0, 1)]
    ref.close()
    eng = _match_engine(n, games, k, B.NET_F16X3, w, w, seed=11, game_offset=0, max_nodes=1024, max_tables=512)
    sp = oa.SelfPlay(eng)
    for split in (3, 0, games):
        sp.set_episode(0)
        sp.match_reset_from(split, boards)
        sp.run(count, k, threshold=0, max_plies=plies)
        _same_episode(_episode(sp, games), want[0])
        assert _same([sp.tree_dump(g, s) for g in range(games) for s in (0, 1)], want[1]), f"split {split}: tree dumps"
    eng.close()


# ---- 5. no stones: omok_match_reset ------------------------------------------------------------------------------------------------
def _searched_ply(sp, games, count, k):
    out = [[sp.tree_dump(g, s) for g in range(games) for s in (0, 1)]]
    sp.execute(count, k)
    out.append(sp.sample_actions(1.0, 0))
    sp.advance()
    out.append([sp.tree_dump(g, s) for g in range(games) for s in (0, 1)])
    out.append([list(sp.replay(g)) for g in range(games)])
    return out


def test_no_stones_is_the_ordinary_match_reset():
    n, games, split, k = SHAPE_A
    engines = [_match_engine(n, games, k, B.NET_F16X3, _weights(n, 1), _weights(n, 2), seed=SEED, game_offset=OFFSET, max_nodes=256, max_tables=128)
               for _ in range(2)]
    a, b = (oa.SelfPlay(e) for e in engines)
    a.match_reset(split)
    b.match_reset_from(split, np.zeros((games, n * n), dtype=np.uint8))
    assert b.ply == 0
    assert _same(_searched_ply(b, games, 16, k), _searched_ply(a, games, 16, k))
    with pytest.raises(B.OmokError) as ei:
        b.play_actions(np.zeros(games, dtype=np.int32))
    assert ei.value.code == -3 and "match" in str(ei.value)
    for e in engines:
        e.close()


# ---- 6. rejections leave the engine as it was ----------------------------------------------------------------------------------------
def _snapshot(sp, games):
    return ([sp.tree_dump(g, s) for g in range(games) for s in (0, 1)], list(sp.game_info()), sp.ply, [list(sp.replay(g)) for g in range(games)])


def _rejected_calls(sp, n, games, with_net2_cases=True):
    """every rejection of omok_match_reset_from but the missing net 2, in the documented order of the checks"""
    good = P.quiet(n, games, 2, seed=3)
    for bad in (-1, games + 1):
        with pytest.raises(B.OmokError) as ei:
            sp.match_reset_from(bad, good)
        assert ei.value.code == -1 and "split" in str(ei.value)
    boards = good.copy()
    boards[2] = P.hand_made(n)["five_diagonal_white"][0]
    with pytest.raises(B.OmokError) as ei:
        sp.match_reset_from(3, boards)
    print(ei.value)
    assert ei.value.code == -5 and "game 2" in str(ei.value) and "verdict 3" in str(ei.value)
    with pytest.raises(B.OmokError) as ei:  # split is checked before the positions
        sp.match_reset_from(-1, boards)
    assert ei.value.code == -1
    boards = good.copy()
    boards[3] = P.quiet(n, 1, 4, seed=4)[0]
    with pytest.raises(B.OmokError) as ei:  # unequal stone counts
        sp.match_reset_from(3, boards)
    print(ei.value)
    assert ei.value.code == -1 and "game 3" in str(ei.value)


@pytest.mark.parametrize("episode_kind", ["selfplay", "match"])
def test_rejections_leave_the_engine_untouched(episode_kind):
    """engine A sees the rejected calls, its twin B never does: equal state afterwards, the same kind of episode, the same next RNG stream"""
    n, games, split, k = SHAPE_A
    count = 16
    pair = []
    for _ in range(2):
        eng = oa.Engine(board_size=n, games=games, max_nodes=256, max_tables=128, max_batch_k=k, seed=SEED, game_offset=OFFSET)
        eng.load_weights(_weights(n, 1))
        if episode_kind == "match":
            eng.load_weights2(_weights(n, 2))
        pair.append((eng, oa.SelfPlay(eng)))
    (eng_a, a), (eng_b, b) = pair
    for sp in (a, b):
        sp.match_reset(split) if episode_kind == "match" else sp.reset()
        sp.execute(count, k)
        first = sp.sample_actions(1.0, 0)
        sp.advance()
    acts = ((first + 1 + np.arange(games)) % (n * n)).astype(np.int32)  # empty cells: one stone lies on every board, at first[g]
    if episode_kind == "selfplay":
        with pytest.raises(B.OmokError) as ei:  # no net 2: the first thing checked after net 1, whatever the other arguments are
            a.match_reset_from(-1, P.quiet(n, games, 2, seed=3))
        assert ei.value.code == -3 and "net 2" in str(ei.value)
        assert _same(_snapshot(a, games), _snapshot(b, games))
        eng_a.load_weights2(_weights(n, 2))
    _rejected_calls(a, n, games)
    assert _same(_snapshot(a, games), _snapshot(b, games))
    if episode_kind == "match":  # still a match episode, with its split: a self-play-only call is refused, the match goes on like the twin's
        with pytest.raises(B.OmokError) as ei:
            a.play_actions(acts)
        assert ei.value.code == -3 and "match" in str(ei.value)
        for sp in (a, b):
            sp.execute(count, k)
            sp.sample_actions(1.0, 0)
            sp.advance()
    else:  # still a self-play episode: the self-play-only call works
        for sp in (a, b):
            sp.play_actions(acts)
    assert _same(_snapshot(a, games), _snapshot(b, games))
    for sp in (a, b):  # the episode counter: the next reset takes the stream the twin's takes
        sp.match_reset(split) if episode_kind == "match" else sp.reset()
    got, want = _searched_ply(a, games, count, k), _searched_ply(b, games, count, k)
    assert _same(got, want)
    b.set_episode(5)  # (and a different stream would show)
    b.match_reset(split) if episode_kind == "match" else b.reset()
    assert not _same(_searched_ply(b, games, count, k), want)
    eng_a.close()
    eng_b.close()


# ---- 7. what follows ---------------------------------------------------------------------------------------------------------------------
def test_follow_up_calls():
    n, games, split, k = SHAPE_A
    eng, sp, _comp, boards, _rows = _start(n, games, split, k, 4)
    sp.execute(16, k)
    before = _snapshot(sp, games)
    acts = np.array([int(np.flatnonzero(boards[g] == 0)[g]) for g in range(games)], dtype=np.int32)
    calls = {"omok_play_actions": lambda: sp.play_actions(acts),
             "omok_versus_run": lambda: sp.versus_run(B.OPP_RANDOM, 0, 16, k),
             "omok_opponent_actions": lambda: sp.opponent_actions(B.OPP_RANDOM),
             "omok_selfplay_run_slots": lambda: sp.run_slots(2 * games, 16, k, 1, 1024),
             "omok_execute_shared": lambda: sp.execute_shared(16, k, waves=1)}
    for name, call in calls.items():
        with pytest.raises(B.OmokError) as ei:
            call()
        assert ei.value.code == -3 and "match" in str(ei.value), name
    assert _same(_snapshot(sp, games), before)
    sp.sample_actions(1.0, 0)
    sp.advance()  # the match goes on
    assert sp.ply == 5
    sp.reset()    # and plain self-play takes over again
    assert sp.ply == 0
    sp.play_actions(acts)
    sp.execute(16, k)
    sp.reset_from(boards)
    sp.opponent_actions(B.OPP_RANDOM)
    eng.close()


# ---- 8. the front end ------------------------------------------------------------------------------------------------------------------
def test_run_match_from_openings():
    n, games, k, sims, stones = 9, 8, 8, 16, 4
    m = games // 2
    eng = _match_engine(n, games, k, B.NET_F16X3, _weights(n, 1), _weights(n, 2), seed=3, game_offset=0, max_nodes=1024, max_tables=512)
    openings = M.random_openings(eng, KEYS[0], stones, m)
    want, ok = RO.positions(n, KEYS[0], 0, stones, m)
    assert np.all(ok == 1) and np.array_equal(openings, want)  # (4 stones end no game: the book is the first M games)
    w, l, d, status, _stats = M.run_match(eng, games, sims, k, openings=openings)
    assert w + l + d == games and not oa.SelfPlay(eng).game_info()[0].any()
    sp = oa.SelfPlay(eng)
    for i in range(m):
        for g in (i, i + m):
            gb, gt, _gp, _gz = sp.replay(g)
            assert len(gb) >= 1 and np.array_equal(gb[0], openings[i]) and gt[0] == (stones & 1), f"game {g} starts from opening {i}"
    paired = M.paired_tally(status, m)
    print(f"W/L/D {w}/{l}/{d}, paired (both, one each, neither, with a draw) {paired}")
    assert sum(paired) == m
    with pytest.raises(ValueError):
        M.run_match(eng, games, sims, k, openings=openings[:3])
    eng.close()
