"""GPU tests (run with -m gpu) of the move log in slots mode (omok_selfplay_run_slots_logged: finished games' moves packed out beside their
records, 20 B per move).  The yardstick is an episode of all the games with the move log on (omok_selfplay_run + omok_game_log_read, tied to
the oracle by tests/test_gpu_game_log.py): slots mode reproduces an episode game by game where the net is row independent (board 9;
OMOK_NET_F16X3_ROWS at board 15; tests/test_gpu_slots.py), so every entry must equal the episode's, bit for bit.
The shapes are those of tests/test_gpu_slots.py.  Its seed 21 gives no 9 x 9 game of more than 64 moves (the longest has 53) and no ply of the
15 x 15 case that harvests two slots, so this file plays seed 31 at board 9 and seed 30 at board 15, found on the yardstick episode alone: a game
of 68 / 104 moves (a log row that crosses the 64-lane sweep) and two slots harvested on one ply at either size; test 1 asserts both."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import omok_ai_amd as oa
from omok_ai_amd import binding as B
from omok_ai_amd import records as R
from omok_ai_amd import trainer as TR

pytestmark = pytest.mark.gpu

STATE, INVALID, OVERFLOW = -3, -1, -4
SEEDS, THRESHOLD, MAX_NODES = {9: 31, 15: 30}, 6, 1024
CASES = [(9, 6, 20, 32, 8, B.NET_F16X3), (9, 5, 5, 24, 8, B.NET_F16X3), (15, 4, 10, 32, 16, B.NET_F16X3_ROWS)]
CANARY = 4096


def _engine(n, games, k, mode, log):
    eng = oa.Engine(board_size=n, games=games, max_nodes=MAX_NODES, max_tables=MAX_NODES // 2, max_batch_k=k, seed=SEEDS[n], net_mode=mode)
    eng.load_random_weights(0)
    sp = oa.SelfPlay(eng)
    if log:
        sp.game_log(True)
    sp.reset()
    return eng, sp


@functools.lru_cache(maxsize=None)
def _episode(case):
    """the yardstick, computed once per case and never written to: (GameRecords of the episode's log, stats)"""
    n, _, total, sims, k, mode = case
    eng, sp = _engine(n, total, k, mode, log=True)
    stats = sp.run(sims, k, 0.25, 0.03, 1.0, THRESHOLD)
    rec = sp.game_records()
    eng.close()
    for name in R._ARRAYS:
        getattr(rec, name).setflags(write=False)
    return rec, stats


def _buffers(sp, cap):
    """records and log buffers of `cap` entries, each followed by a canary region; filled with 0xA5"""
    rb = sp.replay_record_bytes()
    rec = torch.full((cap * rb + CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
    log = torch.full((cap * R.ENTRY_BYTES + CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
    return rb, rec, log


@functools.lru_cache(maxsize=None)
def _slots_logged(case):
    """one logged slots run per case: (stats, n_records, offsets, lengths, status, records bytes, log entries [n_records][20], canaries intact)"""
    n, slots, total, sims, k, mode = case
    eng, sp = _engine(n, slots, k, mode, log=True)
    cap = total * n * n
    rb, rec, log = _buffers(sp, cap)
    stats, nrec, off, ln, status = sp.run_slots_logged(total, sims, k, rec.data_ptr(), cap, log.data_ptr(), 0.25, 0.03, 1.0, THRESHOLD)
    assert sp.alive_count == 0
    with pytest.raises(B.OmokError) as ei:  # the per-slot log describes no game any more
        sp.game_records()
    assert ei.value.code == STATE
    packed = sp.slots_game_records(log, nrec, off, ln, status)
    from_ptr = sp.slots_game_records(log.data_ptr(), nrec, off, ln, status)
    eng.close()
    rec_h, log_h = rec.cpu().numpy(), log.cpu().numpy()
    intact = bool((rec_h[cap * rb:] == 0xA5).all() and (log_h[cap * R.ENTRY_BYTES:] == 0xA5).all())
    untouched_tail = bool((log_h[nrec * R.ENTRY_BYTES:cap * R.ENTRY_BYTES] == 0xA5).all())
    return stats, nrec, off, ln, status, rec_h[:nrec * rb].copy(), log_h[:nrec * R.ENTRY_BYTES].reshape(nrec, R.ENTRY_BYTES).copy(), intact and untouched_tail, packed, from_ptr


def _harvests_at_once(lengths, slots):
    """the largest number of slots whose games end on one engine ply, from the yardstick's game lengths: games 0 .. slots-1 start at ply 0,
    a freed slot takes the next index at the next even ply, in slot order"""
    total, game, start, nxt, ply, worst = len(lengths), list(range(slots)), [0] * slots, slots, 0, 0
    while any(g >= 0 for g in game):
        ply += 1
        done = [s for s in range(slots) if game[s] >= 0 and start[s] + lengths[game[s]] == ply]
        worst = max(worst, len(done))
        for s in done:
            game[s] = -1
        if ply % 2 == 0 or not any(g >= 0 for g in game):
            ply += ply % 2  # (every slot idle on an odd ply: the engine lets the ply pass)
            for s in range(slots):
                if game[s] < 0 and nxt < total:
                    game[s], start[s], nxt = nxt, ply, nxt + 1
    return worst


# ---- 1. the slots log equals the episode's log, game by game -------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"n{c[0]}-slots{c[1]}-total{c[2]}")
def test_slots_log_equals_the_episode_log_game_by_game(case):
    n, slots, total, sims, k, mode = case
    hw = n * n
    want, estats = _episode(case)
    if total > slots:  # conditions on the inputs, one case per board size, from the yardstick alone
        assert int(want.lengths.max()) > 64, f"no game crosses the 64-lane sweep: lengths {want.lengths.tolist()}"
        assert _harvests_at_once([int(x) for x in want.lengths], slots) >= 2, f"no ply harvests two slots: lengths {want.lengths.tolist()}"
    stats, nrec, off, ln, status, rec_bytes, entries, intact, _, _ = _slots_logged(case)
    assert intact, "bytes behind the buffers, or entries beyond n_records, were written"
    assert nrec == int(want.lengths.sum())
    words, halves = entries[:, :16].copy().view("<u4"), entries[:, 16:].copy().view("<u2")
    covered = np.zeros(nrec, dtype=bool)
    want_moves = want.moves()
    for g in range(total):
        o, m = int(off[g]), int(ln[g])
        assert m == int(want.lengths[g]), f"game {g}: {m} vs {int(want.lengths[g])} moves"
        assert int(status[g]) == int(want.status[g]), f"game {g}: status"
        assert 0 <= o and o + m <= nrec and not covered[o:o + m].any(), f"game {g}: range [{o}, {o + m}) overlaps or leaves [0, {nrec})"
        covered[o:o + m] = True
        assert np.array_equal(words[o:o + m, 0], want.root_n[g, :m]), f"game {g}: root_n"
        assert np.array_equal(words[o:o + m, 1], want.root_w.view(np.uint32)[g, :m]), f"game {g}: root_w"
        assert np.array_equal(words[o:o + m, 2], want.child_n[g, :m]), f"game {g}: child_n"
        assert np.array_equal(words[o:o + m, 3], want.child_w.view(np.uint32)[g, :m]), f"game {g}: child_w"
        assert np.array_equal(halves[o:o + m, 0], want_moves[g, :m]), f"game {g}: move"
        assert not halves[o:o + m, 1].any(), f"game {g}: pad"
        assert m <= hw
    assert covered.all()
    assert stats["sims"] == estats["sims"]
    # the log changes no result: a twin with the log off writes the same records through omok_selfplay_run_slots
    eng, sp = _engine(n, slots, k, mode, log=False)
    cap = total * hw
    rb = sp.replay_record_bytes()
    buf = torch.zeros(cap * rb, dtype=torch.uint8, device="cuda")
    pstats, pn, poff, pln, pstatus = sp.run_slots(total, sims, k, buf.data_ptr(), cap, 0.25, 0.03, 1.0, THRESHOLD)
    eng.close()
    assert pn == nrec and np.array_equal(poff, off) and np.array_equal(pln, ln) and np.array_equal(pstatus, status)
    assert buf.cpu().numpy()[:nrec * rb].tobytes() == rec_bytes.tobytes()
    assert pstats["sims"] == stats["sims"]


# ---- 2. replay closure ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"n{c[0]}-slots{c[1]}-total{c[2]}")
def test_slots_records_replay_to_their_status(case):
    n, _, total, _, k, mode = case
    want, _ = _episode(case)
    _, _, _, ln, status, _, _, _, packed, from_ptr = _slots_logged(case)
    assert packed == from_ptr  # a tensor or its device pointer: the same copy
    assert packed == R.GameRecords.from_log(n, want.start_boards, want.lengths, want.moves(), want.root_n, want.root_w, want.child_n, want.child_w,
                                            want.status, want.plies)
    eng = oa.Engine(board_size=n, games=1, max_nodes=64, max_tables=32, max_batch_k=k, seed=SEEDS[n], net_mode=mode)
    packed.verify(eng)
    _, replayed, played = eng.env_replay(None, packed.moves(), packed.lengths)
    eng.close()
    assert np.array_equal(replayed, status) and np.array_equal(played, ln)


# ---- 3. state machine ----------------------------------------------------------------------------------------------------------------
def _code(call):
    with pytest.raises(B.OmokError) as ei:
        call()
    return ei.value.code


def _same_state(sp, twin):
    for a, b in zip(sp.game_info(), twin.game_info()):
        assert np.array_equal(a, b)
    assert sp.alive_count == twin.alive_count and sp.ply == twin.ply


def test_logged_run_state_and_rejections():
    n, games, k, count = 9, 4, 8, 16
    mode = B.NET_F16X3
    eng, sp = _engine(n, games, k, mode, log=False)
    twin_eng, twin = _engine(n, games, k, mode, log=False)
    cap = 2 * games * n * n
    _, rec, log = _buffers(sp, cap)
    run = lambda total=2 * games, r=rec.data_ptr(), l=log.data_ptr(): sp.run_slots_logged(total, count, k, r, cap, l)  # noqa: E731
    assert _code(run) == STATE                                   # the log is off
    assert "omok_game_log_enable" in B.lib().omok_last_error(eng.h).decode()
    _same_state(sp, twin)
    sp.game_log(True)
    assert _code(run) == STATE                                   # on, but no reset since: nothing would be logged
    sp.reset()
    twin.reset()
    assert _code(lambda: run(l=0)) == INVALID                    # no log buffer
    assert _code(lambda: run(total=games - 1)) == INVALID        # fewer games than slots
    assert _code(lambda: run(r=0)) == INVALID                    # no records buffer
    _same_state(sp, twin)
    assert np.all(sp.game_records().lengths == 0)                # the rejected calls left the ordinary log as the reset made it
    assert bool((rec == 0xA5).all()) and bool((log == 0xA5).all())  # ... and wrote nothing
    sp.run(count, k, max_plies=1)
    twin.run(count, k, max_plies=1)
    assert _code(run) == STATE                                   # not a fresh reset
    _same_state(sp, twin)
    assert np.all(sp.game_records().lengths == 1)
    sp.reset()
    _, nrec, off, ln, status = run()
    assert nrec == int(ln.sum()) > 0 and np.all(status >= 1)
    assert _code(sp.game_records) == STATE                       # the per-slot log describes no game
    sp.slots_game_records(log, nrec, off, ln, status).verify(eng)
    twin_eng.close()
    fresh_eng, fresh = _engine(n, games, k, mode, log=True)      # the next reset starts an ordinary log again: that of a fresh engine
    for s in (sp, fresh):
        s.set_episode(5)                                         # (every reset moves on to the next episode's RNG stream: name the same one)
        s.reset()
        s.run(count, k, max_plies=3)
    assert sp.game_records() == fresh.game_records()
    assert np.all(sp.game_records().lengths == 3)
    eng.close()
    fresh_eng.close()


# ---- 4. cap --------------------------------------------------------------------------------------------------------------------------
def test_a_short_cap_overflows_and_writes_neither_buffer_beyond_it():
    case = CASES[0]
    n, slots, total, sims, k, mode = case
    _, need, _, _, _, rec_bytes, entries, _, _, _ = _slots_logged(case)
    cap = need - 3
    eng, sp = _engine(n, slots, k, mode, log=True)
    rb, rec, log = _buffers(sp, cap)
    n_records = C.c_int64(-1)
    off = np.zeros(total, dtype=np.int64)
    rc = B.lib().omok_selfplay_run_slots_logged(eng.h, total, sims, k, 0.25, 0.03, 1.0, THRESHOLD, C.c_void_p(rec.data_ptr()), cap, C.c_void_p(log.data_ptr()),
                                                off.ctypes.data_as(C.POINTER(C.c_int64)), None, None, C.byref(n_records), None)
    assert rc == OVERFLOW
    assert n_records.value == need
    eng.close()
    rec_h, log_h = rec.cpu().numpy(), log.cpu().numpy()
    assert (rec_h[cap * rb:] == 0xA5).all() and rec_h[cap * rb:].size == CANARY
    assert (log_h[cap * R.ENTRY_BYTES:] == 0xA5).all() and log_h[cap * R.ENTRY_BYTES:].size == CANARY
    assert rec_h[:cap * rb].tobytes() == rec_bytes[:cap * rb].tobytes()  # what fits is what the full run wrote there
    assert log_h[:cap * R.ENTRY_BYTES].tobytes() == entries[:cap].tobytes()


# ---- 5. Trainer(save_selfplay_games=...) ---------------------------------------------------------------------------------------------
def _train(tmp_path, name, slots, save):
    p = TR.Parameters(train_backend="hip", episode_count=12, selfplay_slots=slots, evaluate_count=16, evaluate_batch_size=8,
                      parameter_update_count=3, parameter_update_batch_size=16, evaluate_every=0)
    tr = TR.Trainer(p, board_size=9, seed=3, save_dir=str(tmp_path / name), precision_rows=0,
                    save_selfplay_games=str(tmp_path / (name + "_games")) if save else None)
    logs = []
    tr.train(2, log=logs.append)
    weights = [np.asarray(t).view(np.uint32).copy() for t in tr.engine.read_weights()]
    tr.close()
    assert not any("WARNING" in line for line in logs), logs
    return weights


def test_trainer_saves_the_same_games_on_both_paths_and_trains_the_same_weights(tmp_path, capsys):
    slots_w = _train(tmp_path, "slots", 5, True)
    episode_w = _train(tmp_path, "episode", 0, True)
    plain_w = _train(tmp_path, "plain", 5, False)
    assert not (tmp_path / "plain_games").exists()
    assert len(slots_w) == len(episode_w) == len(plain_w) == 31
    for i in range(31):
        assert np.array_equal(slots_w[i], plain_w[i]) and np.array_equal(episode_w[i], plain_w[i]), f"tensor {i} differs"
    for it in (1, 2):
        name = f"selfplay_iter{it:06d}.rank0.npz"
        a, b = R.load(str(tmp_path / "slots_games" / name)), R.load(str(tmp_path / "episode_games" / name))
        assert a.games == b.games == 12 and int(a.lengths.sum()) > 0
        for field in R._ARRAYS:
            x, y = getattr(a, field), getattr(b, field)
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (it, field)
        assert a.meta["kind"] == b.meta["kind"] == "selfplay" and a.meta["iteration"] == b.meta["iteration"] == it
        assert (a.meta["slots"], b.meta["slots"]) == (5, 0)
        for key in ("seed", "sims", "batch", "game_offset"):
            assert a.meta[key] == b.meta[key], key
    assert R.main(["show", str(tmp_path / "slots_games" / "selfplay_iter000002.rank0.npz"), "--game", "11"]) == 0
    assert "game 11: 9 x 9, 0 stones at the start" in capsys.readouterr().out
