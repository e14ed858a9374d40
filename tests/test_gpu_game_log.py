"""GPU tests (run with -m gpu) of the move log (omok_game_log_enable / omok_game_log_read) and of the records built from it: every entry
against the oracle's self-play object driven in lockstep (the move from its sample, root n / w from its tree_root, the child's n / w from
its tree dump BEFORE the advance), the whole-episode calls against the step-wise ones, episodes from given positions, the replay closure
(records.verify through omok_env_replay), and that nothing else moves when the log is on."""
import ctypes as C

import numpy as np
import pytest

import omok_ai_amd as oa
from omok_ai_amd import binding as B
from omok_ai_amd import records as R
from oracle import oracle as O
import positions as P
import scripted_opponent as SO

pytestmark = pytest.mark.gpu

STATE, INVALID, ILLEGAL = -3, -1, -5


def _engine(n, games, k, seed, max_nodes=1024, max_tables=512, log=True, **kw):
    eng = oa.Engine(board_size=n, games=games, max_nodes=max_nodes, max_tables=max_tables, max_batch_k=k, seed=seed, **kw)
    eng.load_random_weights(0)
    sp = oa.SelfPlay(eng)
    if log:
        sp.game_log(True)
    return eng, sp


class Expected:
    """the log as the oracle dictates it, entry by entry"""

    def __init__(self, n, games):
        hw = n * n
        self.moves = np.full((games, hw), 0xFFFF, dtype=np.uint16)
        self.root_n, self.child_n = np.zeros((games, hw), dtype=np.uint32), np.zeros((games, hw), dtype=np.uint32)
        self.root_w, self.child_w = np.zeros((games, hw), dtype=np.float32), np.zeros((games, hw), dtype=np.float32)
        self.lengths = np.zeros(games, dtype=np.int32)

    def add(self, osp, g, side, cell, external):
        """before the oracle's advance: its tree of the side to move still stands at the position the move was chosen in"""
        i = int(self.lengths[g])
        rn, rw = osp.tree_root(g, side)[:2]
        ints, floats = osp.tree_dump(g, side)
        kids = [j for j in range(1, len(ints)) if ints[j, 0] == 0 and ints[j, 1] == cell]
        assert len(kids) <= 1
        self.moves[g, i] = cell | (0x100 if external else 0)
        self.root_n[g, i], self.root_w[g, i] = rn, rw
        if kids:
            self.child_n[g, i], self.child_w[g, i] = ints[kids[0], 6], floats[kids[0], 0]
        self.lengths[g] = i + 1
        return int(rn), (int(ints[kids[0], 6]) if kids else 0)

    def check(self, rec, tag):
        assert np.array_equal(rec.lengths, self.lengths), f"{tag}: lengths {rec.lengths} != {self.lengths}"
        assert np.array_equal(rec.moves(), self.moves), f"{tag}: moves"
        for name in ("root_n", "child_n"):
            assert np.array_equal(getattr(rec, name), getattr(self, name)), f"{tag}: {name}"
        for name in ("root_w", "child_w"):  # bit for bit
            assert np.array_equal(getattr(rec, name).view(np.uint32), getattr(self, name).view(np.uint32)), f"{tag}: {name}"
        beyond = np.arange(rec.hw)[None, :] >= rec.lengths[:, None]
        assert np.all(rec.moves()[beyond] == 0xFFFF) and np.all(rec.cells[beyond] == -1) and not rec.external[beyond].any()
        for name in ("root_n", "root_w", "child_n", "child_w"):
            assert not getattr(rec, name)[beyond].any(), f"{tag}: {name} beyond the length"


def _lockstep(n, games, k, count, seed, threshold, max_plies, kind=None, opponent_side=-1):
    """engine and oracle step by step (as tests/test_gpu_versus.py drives them); returns (records, expectation, oracle statuses, oracle
    plies, facts about the scripted plies)"""
    eng, sp = _engine(n, games, k, seed)
    sp.reset()
    root_p = eng.evaluate_p(O.Environment(n).encode_nn_input(0)[None]).reshape(-1)
    osp = O.SelfPlay(n, games, cap_nodes=1024, cap_tables=512, seed=seed)
    osp.reset(root_p)
    key = O.stream_key(seed, 0)
    envs = [O.Environment(n) for _ in range(games)]
    exp = Expected(n, games)
    scripted, searched_roots = [], []
    ply = 0
    while osp.alive_count > 0 and ply < max_plies:
        alive = [g for g in range(games) if osp.game_alive(g)]
        external = (ply & 1) == opponent_side
        if external:
            want = np.full(games, -1, dtype=np.int32)
            for g in alive:
                want[g], _forced = SO.move(kind, envs[g].e, key, osp.game_plies(g), g)
            acts = sp.opponent_actions(kind)
            assert np.array_equal(acts, want), f"ply {ply}: scripted moves"
            osp.set_actions(want)
        else:
            for rnd in range((count + k - 1) // k):
                nreq = sp.round_generate(rnd, k, 0.25, 0.03)
                oin = osp.round_generate(rnd, k, 0.25, 0.03)
                assert nreq == len(oin) and np.array_equal(sp.round_inputs(), oin), f"ply {ply} round {rnd}: requests"
                p, v = sp.round_eval()
                sp.round_scatter()
                osp.round_scatter(p, v)
            acts = sp.sample_actions(1.0, threshold)
            assert np.array_equal(acts, osp.sample(1.0, threshold)), f"ply {ply}: sampled moves"
        for g in alive:
            rn, cn = exp.add(osp, g, ply & 1, int(acts[g]), external)
            (scripted if external else searched_roots).append((rn, cn))
            assert envs[g].place_stone(int(acts[g])) is not None
        assert sp.mirror_generate() == len(osp.mirror_generate())
        pm = sp.mirror_eval()
        sp.mirror_apply()
        osp.advance(pm)
        assert osp.error == 0
        ply += 1
    rec = sp.game_records()
    assert [int(x) for x in rec.plies] == [osp.game_plies(g) for g in range(games)]
    assert [int(x) for x in rec.status] == [osp.game_status(g) for g in range(games)]
    assert not rec.start_boards.any()
    rec.verify(eng)  # closure: every record replays to its recorded end through omok_env_replay
    eng.close()
    return rec, exp, [osp.game_status(g) for g in range(games)], [osp.game_plies(g) for g in range(games)], (scripted, searched_roots)


# ---- 1. self-play, step by step against the oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold,statuses,plies", [
    (0, [3, 3, 2, 2, 3, 2], [40, 34, 45, 17, 42, 39]),
    (4, [2, 2, 3, 2, 2, 3], [43, 45, 48, 37, 51, 48]),
])
def test_selfplay_log_against_the_oracle(threshold, statuses, plies):
    rec, exp, o_status, o_plies, (_, searched) = _lockstep(9, 6, 8, 32, 3, threshold, 81)
    print(f"threshold {threshold}: oracle statuses {o_status} plies {o_plies}")
    assert o_status == statuses and o_plies == plies  # the oracle alone: every game ended in a win ...
    assert all(s in (O.BLACK_WIN, O.WHITE_WIN) for s in o_status)
    if threshold == 0:
        assert len(set(o_plies)) == len(o_plies)  # ... and no two lengths are equal
    exp.check(rec, f"threshold {threshold}")
    assert np.array_equal(rec.lengths, o_plies) and not rec.external.any()
    assert all(rn >= 32 and cn >= 1 for rn, cn in searched)  # (every logged root was searched, every chosen child visited)


def test_selfplay_log_on_the_large_board():
    rec, exp, o_status, o_plies, (_, searched) = _lockstep(15, 4, 16, 64, 5, 30, 8)
    assert o_status == [0, 0, 0, 0] and o_plies == [8, 8, 8, 8]  # four-word boards, max_plies: all in progress
    assert all(rn >= 64 for rn, _ in searched)
    exp.check(rec, "15 x 15")
    assert np.all(rec.lengths == 8) and np.all(rec.status == 0)


# ---- 2. versus: the scripted player's plies are external ---------------------------------------------------------------------------
def test_versus_log_against_the_oracle():
    rec, exp, o_status, o_plies, (scripted, searched) = _lockstep(9, 6, 8, 32, 3, 0, 81, kind=B.OPP_NAIVE, opponent_side=0)
    exp.check(rec, "versus")
    assert len(scripted) >= 6 and len(searched) >= 6
    assert all(rn == 0 and cn == 0 for rn, cn in scripted)  # the never-searched tree of the scripted side
    played = np.arange(rec.hw)[None, :] < rec.lengths[:, None]
    black_ply = (np.arange(rec.hw)[None, :] % 2 == 0) & played
    assert np.array_equal(rec.external, black_ply)
    assert not rec.root_n[rec.external].any() and not rec.child_n[rec.external].any() and not rec.child_w[rec.external].any()
    assert np.all(rec.root_n[played & ~rec.external] >= 32)


# ---- 3. whole-episode calls equal the step-wise log ------------------------------------------------------------------------------
def _twins(n, games, k, seed, **kw):
    return _engine(n, games, k, seed, **kw), _engine(n, games, k, seed, **kw)


def _finished_and_verified(eng, sp):
    rec = sp.game_records()
    alive, status, plies = sp.game_info()
    assert not alive.any() and np.array_equal(rec.status, status) and np.array_equal(rec.plies, plies)
    assert np.array_equal(rec.lengths, plies - np.count_nonzero(rec.start_boards, axis=1))
    rec.verify(eng)
    return rec


def test_selfplay_run_equals_the_stepwise_calls():
    n, games, k, count, seed = 9, 6, 8, 32, 3
    (eng_a, a), (eng_b, b) = _twins(n, games, k, seed)
    a.reset()
    b.reset()
    a.run(count, k, threshold=4)
    while b.alive_count > 0:
        b.execute(count, k)
        b.sample_actions(1.0, 4)
        b.advance()
    ra, rb = _finished_and_verified(eng_a, a), _finished_and_verified(eng_b, b)
    assert ra == rb and ra.lengths.min() >= 9 and not ra.external.any()
    eng_a.close()
    eng_b.close()


def _stepwise_plies(sp, kind, opponent_side, count, k, plies):
    for _ in range(plies):
        if sp.alive_count == 0:
            break
        if (sp.ply & 1) == opponent_side:
            sp.opponent_actions(kind)
        else:
            sp.execute(count, k)
            sp.sample_actions(1.0, 0)
        sp.advance()


def test_versus_run_equals_the_stepwise_calls():
    n, games, k, count, seed = 9, 6, 8, 32, 3
    (eng_a, a), (eng_b, b) = _twins(n, games, k, seed)
    a.reset()
    b.reset()
    a.versus_run(B.OPP_NAIVE, 0, count, k)
    _stepwise_plies(b, B.OPP_NAIVE, 0, count, k, n * n)
    ra, rb = _finished_and_verified(eng_a, a), _finished_and_verified(eng_b, b)
    assert ra == rb and ra.external[:, 0].all() and not ra.external[:, 1].any()
    eng_a.close()
    eng_b.close()


def test_match_run_equals_the_stepwise_calls():
    n, games, k, count, seed = 9, 6, 8, 32, 3
    (eng_a, a), (eng_b, b) = _twins(n, games, k, seed)
    w2 = oa.weights.init_random(n, seed=1)  # (net 1: random-init seed 0)
    for eng, sp in ((eng_a, a), (eng_b, b)):
        eng.load_weights2(w2)
        sp.match_reset(3)
    a.run(count, k, threshold=0)
    while b.alive_count > 0:
        b.execute(count, k)
        b.sample_actions(1.0, 0)
        b.advance()
    ra, rb = _finished_and_verified(eng_a, a), _finished_and_verified(eng_b, b)
    assert ra == rb and not ra.external.any()
    played = np.arange(ra.hw)[None, :] < ra.lengths[:, None]
    assert np.all(ra.root_n[played] >= count) and np.all(ra.child_n[played] >= 1)
    eng_a.close()
    eng_b.close()


def test_one_game_search_and_supplied_moves_interleaved():
    """the GUI's flow (gui/src/agent.rs): the engine searches and moves, then is told the other side's move"""
    n, k, count, seed = 9, 8, 32, 9
    eng, sp = _engine(n, 1, k, seed, max_tree_waves=1)
    sp.reset()
    rng = np.random.default_rng(seed)
    want = {name: [] for name in ("move", "root_n", "root_w", "child_n", "child_w")}

    def note(side, cell, external):  # what omok_tree_root / omok_root_children say in front of the advance
        rn, rw = sp.tree_root(0, side)[:2]
        acts, cn, cw, _ = sp.root_children(0, side)
        hit = np.flatnonzero(acts == cell)
        want["move"].append(cell | (0x100 if external else 0))
        want["root_n"].append(rn)
        want["root_w"].append(np.float32(rw))
        want["child_n"].append(int(cn[hit[0]]) if len(hit) else 0)
        want["child_w"].append(np.float32(cw[hit[0]]) if len(hit) else np.float32(0.0))

    board = np.zeros(n * n, dtype=np.uint8)
    for ply in range(8):
        if ply % 2 == 0:
            sp.execute_shared(count, k, waves=1)
            cell = int(sp.sample_actions(1.0, 0)[0])
            note(0, cell, False)
            sp.advance()
        else:
            cell = int(rng.choice(np.flatnonzero(board == 0)))
            note(1, cell, True)
            sp.play_actions([cell])
        board[cell] = 1 + ply % 2
        if sp.alive_count == 0:
            break
    rec = sp.game_records()
    m = int(rec.lengths[0])
    assert m == len(want["move"]) >= 5
    assert [int(x) for x in rec.moves()[0, :m]] == want["move"]
    assert list(rec.external[0, :m]) == [bool(i % 2) for i in range(m)]
    assert [int(x) for x in rec.root_n[0, :m]] == want["root_n"] and [int(x) for x in rec.child_n[0, :m]] == want["child_n"]
    assert np.array_equal(rec.root_w[0, :m].view(np.uint32), np.array(want["root_w"], dtype=np.float32).view(np.uint32))
    assert np.array_equal(rec.child_w[0, :m].view(np.uint32), np.array(want["child_w"], dtype=np.float32).view(np.uint32))
    assert all(rec.root_n[0, i] >= count for i in range(0, m, 2))
    assert np.array_equal(rec.verify(eng)[0], board)
    with pytest.raises(B.OmokError) as ei:  # a rejected move logs nothing
        sp.play_actions([cell])
    assert ei.value.code == ILLEGAL
    assert sp.game_records() == rec
    eng.close()


# ---- 4. from positions -----------------------------------------------------------------------------------------------------------
def test_log_from_given_positions():
    n, games, k, count, seed = 9, 6, 8, 32, 4
    boards = P.quiet(n, games, 7, seed)
    eng, sp = _engine(n, games, k, seed)
    sp.reset_from(boards)
    for _ in range(6):
        sp.execute(count, k)
        sp.sample_actions(1.0, 30)
        sp.advance()
    rec = sp.game_records()
    _, status, plies = sp.game_info()
    assert np.array_equal(rec.start_boards, boards)
    assert np.array_equal(rec.lengths, plies - 7) and rec.lengths.max() == 6  # lengths count from the position
    rec.verify(eng)
    for g in range(games):
        tb, tt, _, _ = sp.replay(g)  # the transitions' boards: the position in front of every sampled move
        assert len(tb) == rec.lengths[g]
        for kk in range(len(tb)):
            assert np.array_equal(rec.position_at(g, kk, eng), tb[kk]), f"game {g} move {kk}"
            assert tt[kk] == (7 + kk) & 1
        final = rec.position_at(g, int(rec.lengths[g]), eng)
        assert np.count_nonzero(final) == plies[g]
    eng.close()


# ---- 6. nothing else moves ---------------------------------------------------------------------------------------------------------
COUNTERS = ("sims", "evals", "ply_games", "finished", "tree_bytes", "peak_nodes", "peak_tables", "round_launches")


def _same_engines(a, b, games, tag):
    for g in range(games):
        for side in (0, 1):
            (ai, af), (bi, bf) = a.tree_dump(g, side), b.tree_dump(g, side)
            assert np.array_equal(ai, bi) and np.array_equal(af.view(np.uint32), bf.view(np.uint32)), f"{tag}: tree (game {g} side {side})"
        for x, y in zip(a.replay(g), b.replay(g)):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{tag}: replay of game {g}"
    for x, y in zip(a.game_info(), b.game_info()):
        assert np.array_equal(x, y), tag


def test_the_log_changes_nothing_else():
    n, games, k, count, seed = 9, 6, 8, 32, 3
    (eng_a, a), (eng_b, b) = _engine(n, games, k, seed, log=True), _engine(n, games, k, seed, log=False)
    a.reset()
    b.reset()
    sa, sb = a.run(count, k, threshold=4, max_plies=7), b.run(count, k, threshold=4, max_plies=7)
    _same_engines(a, b, games, "7 plies")
    assert {c: sa[c] for c in COUNTERS} == {c: sb[c] for c in COUNTERS}
    sa, sb = a.run(count, k, threshold=4), b.run(count, k, threshold=4)
    _same_engines(a, b, games, "end")
    assert {c: sa[c] for c in COUNTERS} == {c: sb[c] for c in COUNTERS}
    assert a.game_records().lengths.sum() == sa["ply_games"]
    eng_a.close()
    eng_b.close()


# ---- 7. state ------------------------------------------------------------------------------------------------------------------------
def _code(call):
    with pytest.raises(B.OmokError) as ei:
        call()
    return ei.value.code


def test_log_state_and_errors():
    n, games, k, count = 9, 4, 8, 16
    eng, sp = _engine(n, games, k, 2, log=False)
    sp.reset()
    assert _code(sp.game_records) == STATE                    # the log is off
    sp.game_log(True)
    assert _code(sp.game_records) == STATE                    # on, but no reset since
    sp.run(count, k, max_plies=2)                             # (moves made before the log's first reset are not logged)
    assert _code(sp.game_records) == STATE
    sp.reset()
    assert np.all(sp.game_records().lengths == 0)
    sp.run(count, k, max_plies=3)
    rec = sp.game_records()
    assert np.all(rec.lengths == 3)
    won, v = P.hand_made(n)["five_row_black"]
    assert v == P.WON
    assert _code(lambda: sp.reset_from(np.stack([won] * games))) == ILLEGAL
    assert sp.game_records() == rec                           # a rejected reset leaves the log readable and unchanged
    for first, count_ in ((-1, 1), (0, games + 1), (games, 1), (2, games - 1), (0, -1)):
        assert _code(lambda: sp.game_records(first, count_)) == INVALID
    part = sp.game_records(1, 2)                              # a range
    assert part.games == 2 and np.array_equal(part.moves(), rec.moves()[1:3]) and np.array_equal(part.plies, rec.plies[1:3])
    assert np.array_equal(part.child_w.view(np.uint32), rec.child_w[1:3].view(np.uint32))
    lengths = np.zeros(games, dtype=np.int32)                 # every output may be NULL
    assert B.lib().omok_game_log_read(eng.h, 0, games, None, B.iptr(lengths), None, None, None, None, None) == 0
    assert np.all(lengths == 3)
    assert B.lib().omok_game_log_read(eng.h, 0, games, None, None, None, None, None, None, None) == 0
    sp.reset()                                                # a reset clears the lengths
    fresh = sp.game_records()
    assert np.all(fresh.lengths == 0) and np.all(fresh.moves() == 0xFFFF) and not fresh.root_n.any() and not fresh.child_w.any()
    # slots mode: its games leave their slots
    import torch
    rb = sp.replay_record_bytes()
    cap = 2 * games * n * n
    buf = torch.empty(cap * rb, dtype=torch.uint8, device="cuda")
    assert _code(lambda: sp.run_slots(2 * games, count, k, buf.data_ptr(), cap)) == STATE
    assert "log" in B.lib().omok_last_error(eng.h).decode()
    sp.game_log(False)
    assert _code(sp.game_records) == STATE
    _, n_records, _, slot_lengths, slot_status = sp.run_slots(2 * games, count, k, buf.data_ptr(), cap)  # as before
    assert n_records == slot_lengths.sum() > 0 and np.all(slot_status >= 1)
    sp.game_log(True)                                         # enable / disable / enable allocates again and works
    assert _code(sp.game_records) == STATE
    sp.reset()
    sp.run(count, k, max_plies=2)
    again = sp.game_records()
    assert np.all(again.lengths == 2)
    again.verify(eng)
    eng.close()


# ---- 8. the front ends: match.py --save-games, Trainer.evaluate(save_games=...), records show ------------------------------------
def test_match_save_games_and_show(tmp_path, capsys):
    from omok_ai_amd import match as M
    n, games = 9, 8
    paths = []
    for s in (1, 2):
        p = str(tmp_path / f"net{s}.bin")
        oa.model_file.save(p, oa.weights.tensor_names(), oa.weights.init_random(n, seed=s))
        paths.append(p)
    out = str(tmp_path / "games.npz")
    argv = paths + ["--games", str(games), "--sims", "32", "--batch", "8", "--board", "9", "--seed", "5", "--random-openings", "4"]
    plain = M.main(argv)
    saved = M.main(argv + ["--save-games", out])
    assert saved == plain  # keeping the log changes no result
    rec = R.load(out)
    assert rec.games == games and [int(s) for s in rec.status] == plain["status"]
    assert rec.meta["net1"] == paths[0] and rec.meta["net2"] == paths[1] and rec.meta["split"] == games // 2
    assert (rec.meta["sims"], rec.meta["seed"], rec.meta["openings"], rec.meta["kind"]) == (32, 5, "random:4", "match")
    assert np.all(np.count_nonzero(rec.start_boards, axis=1) == 4) and np.array_equal(rec.start_boards[:4], rec.start_boards[4:])
    eng = oa.Engine(board_size=n, games=1, max_nodes=16, max_tables=8, max_batch_k=1)
    rec.verify(eng)
    eng.close()
    capsys.readouterr()
    assert R.main(["show", out, "--game", "5"]) == 0
    text = capsys.readouterr().out
    print(text)
    assert rec.to_text(5) in text and f"{int(rec.lengths[5])} moves" in text and text.count("\n") >= 12 + int(rec.lengths[5])


def test_trainer_evaluate_saves_its_games(tmp_path):
    import os
    from omok_ai_amd import trainer as TR
    n, games = 9, 6
    save_dir = str(tmp_path / "saves")
    p = TR.Parameters(model_name="tiny", episode_count=2, evaluate_count=16, evaluate_batch_size=8, evaluate_games=games, test_evaluate_count=16)
    tr = TR.Trainer(p, board_size=n, seed=3, save_dir=save_dir, precision_rows=0)
    os.makedirs(save_dir, exist_ok=True)
    tr.engine.save(os.path.join(save_dir, p.model_name))
    tr.iteration = 1
    counts = tr.evaluate()
    out = str(tmp_path / "eval.npz")
    assert tr.evaluate(save_games=out) == counts
    rec = R.load(out)
    assert rec.games == games and rec.meta["kind"] == "evaluate" and rec.meta["opponent"] == "naive" and rec.meta["iteration"] == 1
    assert (int(np.sum(rec.status == 2)), int(np.sum(rec.status == 3)), int(np.sum(rec.status == 1))) == counts
    assert rec.external[:, 0].all() and not rec.external[:, 1].any()  # the naive player is Black and moves first
    rec.verify(tr.engine)
    tr.close()
