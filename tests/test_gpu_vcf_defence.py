"""GPU tests (run with -m gpu) of the defender's half of the forced-win solver (omok_env_vcf_defend) through the C ABI, against
tests/vcf_defence.py (the rule restated in plain Python, pinned by tests/test_vcf_defence.py) and against the merged solver kernel
(omok_env_vcf_solve) with no Python in between; the launch shape's edges, the rejected calls, and the report of
records.GameRecords.vcf_defence with its command line.  Every batch is bounded by 4096 nodes per wave; the rejected calls launch nothing."""
import json

import numpy as np
import pytest

import omok_ai_amd as oa
from omok_ai_amd import binding as B
from omok_ai_amd import records as R
import vcf_defence as VD
import vcf_solver as VS

pytestmark = pytest.mark.gpu

SETTINGS = [("a", 8, 4096), ("b", 8, 8), ("b", 2, 4096), ("hand", 16, 4096)]
INPUTS = {"a": VD.set_a, "b": VD.set_b, "hand": lambda n: VD.hand_set(n)[1:]}
PAD = 64  # canary elements behind every output buffer


def _solver_engine(n):
    return oa.Engine(board_size=n, games=1, max_nodes=16, max_tables=8, max_batch_k=1)  # (the call needs no net)


def _assert_equal(got, want, keys=VD.KEYS):
    for name in keys:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, name
        bad = np.flatnonzero(np.any((g != w).reshape(len(g), -1), axis=1))
        assert len(bad) == 0, f"{name}: {len(bad)} positions differ, first {int(bad[0])}: {g[bad[0]]} != {w[bad[0]]}"


# ---- 1. against the yardstick --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,depth,budget", SETTINGS)
@pytest.mark.parametrize("n", [9, 15])
def test_defend_equals_the_yardstick(n, tag, depth, budget):
    boards, turns = INPUTS[tag](n)
    want = VD.want(tag, n, depth, budget)
    eng = _solver_engine(n)
    got = eng.env_vcf_defend(boards, turns, depth, budget)
    eng.close()
    print(f"board {n} set {tag} D {depth} NB {budget}: {len(boards)} positions, cells by status "
          f"{[int((want['status'] == v).sum()) for v in range(5)]}, nodes {int(want['nodes'].sum())}")
    _assert_equal(got, want)


# ---- 2. against the merged solver kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [9, 15])
def test_rows_equal_the_solver_kernel_on_the_same_boards(n):
    depth, budget = 8, 4096
    boards, turns = VD.set_a(n)
    eng = _solver_engine(n)
    got = eng.env_vcf_defend(boards, turns, depth, budget)
    verdict, cell, moves, _nodes, _pv = eng.env_vcf_solve(boards, 1 - turns, depth, budget)  # the null move: the other side to move
    assert np.array_equal(got["threat"], np.stack([verdict, moves, cell], axis=1))
    st = got["status"]
    both = (st == VD.SAFE).any(axis=1) & (st == VD.LOSES).any(axis=1)
    odd = list(np.flatnonzero((got["threat"][:, 0] == 0) & (st == VD.LOSES).any(axis=1))[:2])  # the non-monotone ones: 2 at 9 x 9, 1 at 15 x 15
    chosen = odd + list(np.flatnonzero((got["threat"][:, 0] == 1) & both)[:8 - len(odd)])
    assert len(odd) >= 1 and len(chosen) == 8
    for b in chosen:  # every cell the rule solves: the board with the mover's stone there, the other side to move
        cells = np.flatnonzero((st[b] != VD.OCCUPIED) & (st[b] != VD.WINS))
        with_stone = np.repeat(boards[b][None], len(cells), axis=0)
        with_stone[np.arange(len(cells)), cells] = 1 + int(turns[b])
        verdict, cell, moves, nodes, _pv = eng.env_vcf_solve(with_stone, np.full(len(cells), 1 - int(turns[b]), dtype=np.uint8), depth, budget)
        status = np.where(verdict == 0, VD.SAFE, np.where(verdict == 1, VD.LOSES, VD.UNKNOWN))
        assert np.array_equal(st[b][cells], status) and np.array_equal(got["moves"][b][cells], moves), b
        assert np.array_equal(got["nodes"][b][cells], nodes) and np.array_equal(got["reply"][b][cells], cell), b
    eng.close()


# ---- 3. the launch shape's edges ---------------------------------------------------------------------------------------------------
def _raw(eng, boards, turns, depth, budget, keep=range(5), batch=None, handle=True):
    """the C call with canary-padded outputs; outputs outside `keep` are passed as NULL.  Returns (rc, the five arrays or None, canaries intact)"""
    b, hw = len(boards), boards.shape[1]
    sizes = (b * hw, b * hw, b * hw, b * hw, b * 3)
    bufs = [np.full(s + PAD, 0xA5 if i < 2 else -77, dtype=np.uint8 if i < 2 else np.int32) for i, s in enumerate(sizes)]
    args = [(B.u8ptr(a) if i < 2 else B.iptr(a)) if i in keep else None for i, a in enumerate(bufs)]
    rc = B.lib().omok_env_vcf_defend(eng.h if handle else None, B.u8ptr(boards) if boards is not None else None,
                                     B.u8ptr(turns) if turns is not None else None, b if batch is None else batch, depth, budget, *args)
    intact = all(np.all(a[s:] == (0xA5 if i < 2 else -77)) for i, (a, s) in enumerate(zip(bufs, sizes)))
    outs = [a[:s].reshape(b, -1) for a, s in zip(bufs, sizes)]
    return rc, outs, intact


@pytest.mark.parametrize("n", [9, 15])
def test_launch_shape_edges(n):
    depth, budget = 8, 4096
    boards, turns = VD.set_a(n)
    want = VD.want("a", n, depth, budget)
    names = ("status", "moves", "nodes", "reply", "threat")
    eng = _solver_engine(n)
    # batch 1, and batches whose B (HW + 1) waves are odd or no multiple of 4 or 8 (3 * 82 = 246, 7 * 226 = 1582, 5 * 82 = 410)
    for first, count in ((len(boards) - 1, 1), (2, 3), (11, 5), (20, 7)):
        rc, outs, intact = _raw(eng, boards[first:first + count], turns[first:first + count], depth, budget)
        assert rc == 0 and intact
        for name, o in zip(names, outs):
            assert np.array_equal(o, want[name][first:first + count]), (name, first, count)
    # the same position at two places of one batch gives equal rows
    twice = np.concatenate([boards[5:6], boards[:9], boards[5:6]])
    got = eng.env_vcf_defend(twice, np.concatenate([turns[5:6], turns[:9], turns[5:6]]), depth, budget)
    for name in names:
        assert np.array_equal(got[name][0], got[name][-1]) and np.array_equal(got[name][0], want[name][5]), name
    # each output alone, all but each one, and none
    part_b, part_t = boards[:13], turns[:13]
    for keep in [(i,) for i in range(5)] + [tuple(j for j in range(5) if j != i) for i in range(5)] + [()]:
        rc, outs, intact = _raw(eng, part_b, part_t, depth, budget, keep=keep)
        assert rc == 0 and intact, keep
        for i, (name, o) in enumerate(zip(names, outs)):
            if i in keep:
                assert np.array_equal(o, want[name][:13]), (keep, name)
            else:
                assert np.all(o == (0xA5 if i < 2 else -77)), (keep, name)
    # bytes that are no stone read as empty
    garbage = boards[:13].copy()
    empty = garbage == 0
    garbage[empty & (np.arange(garbage.size).reshape(garbage.shape) % 3 == 0)] = 3
    garbage[empty & (np.arange(garbage.size).reshape(garbage.shape) % 3 == 1)] = 255
    assert (garbage == 3).any() and (garbage == 255).any()
    got = eng.env_vcf_defend(garbage, part_t, depth, budget)
    _assert_equal(got, {k: v[:13] for k, v in want.items()})
    eng.close()


# ---- 4. rejected calls ----------------------------------------------------------------------------------------------------------------
def test_rejected_calls_write_nothing():
    n = 9
    eng = _solver_engine(n)
    boards = np.stack([VS.hand_made(n)["open_three_s0_r4"][0]] * 3)
    turns = np.ones(3, dtype=np.uint8)
    L = B.lib()

    def call(boards_, turns_, depth, budget, batch=None, handle=True):
        b = boards if boards_ is None else boards_  # (the shapes of the canary buffers)
        bufs = [np.full(3 * 81 + PAD, 0xA5, dtype=np.uint8) for _ in range(2)] + [np.full(3 * 81 + PAD, -77, dtype=np.int32) for _ in range(3)]
        rc = L.omok_env_vcf_defend(eng.h if handle else None, B.u8ptr(boards_) if boards_ is not None else None,
                                   B.u8ptr(turns_) if turns_ is not None else None, len(b) if batch is None else batch, depth, budget,
                                   B.u8ptr(bufs[0]), B.u8ptr(bufs[1]), B.iptr(bufs[2]), B.iptr(bufs[3]), B.iptr(bufs[4]))
        assert all(np.all(a == (0xA5 if i < 2 else -77)) for i, a in enumerate(bufs))
        return rc

    assert call(boards, np.array([0, 1, 2], dtype=np.uint8), 8, 4096) == -1 and "turns[2]" in L.omok_last_error(eng.h).decode()
    assert call(boards, turns, 8, 4096, handle=False) == -1
    assert call(None, turns, 8, 4096) == -1 and call(boards, None, 8, 4096) == -1
    assert call(boards, turns, 8, 4096, batch=0) == -1 and call(boards, turns, 8, 4096, batch=-1) == -1
    for depth, budget in ((0, 4096), (17, 4096), (-1, 4096), (8, 0), (8, 65537), (8, -1)):
        assert call(boards, turns, depth, budget) == -1, (depth, budget)
    with pytest.raises(B.OmokError) as ei:
        eng.env_vcf_defend(boards, turns, 8, 65537)
    assert ei.value.code == -1 and "max_nodes" in str(ei.value)
    at = lambda x, y: y * n + x  # noqa: E731
    got = eng.env_vcf_defend(boards[:1], turns[:1], 16, 65536)  # the limits themselves are accepted
    assert got["threat"].tolist() == [[1, 2, at(1, 4)]] and np.flatnonzero(got["status"][0] == VD.SAFE).tolist() == [at(1, 4), at(5, 4)]
    assert (int(got["safe"][0]), int(got["wins"][0]), int(got["loses"][0]), int(got["unknown"][0])) == (2, 0, 76, 0)
    got = eng.env_vcf_defend(boards[:1], turns[:1], 1, 1)  # one node: depth 1 finds no five anywhere
    assert got["threat"].tolist() == [[0, 0, -1]] and int(got["safe"][0]) == 78 and np.all(got["nodes"][0][got["status"][0] == VD.SAFE] == 1)
    eng.close()


# ---- 5. no engine state is written -----------------------------------------------------------------------------------------------------
def _engine(n, games, k, seed):
    eng = oa.Engine(board_size=n, games=games, max_nodes=1024, max_tables=512, max_batch_k=k, seed=seed)
    eng.load_random_weights(0)
    return eng, oa.SelfPlay(eng)


def _step(sp, plies, count, k):
    for _ in range(plies):
        sp.execute(count, k)
        sp.sample_actions(1.0, 0)
        sp.advance()


def test_the_call_touches_no_engine_state():
    n, games, k, count, seed = 9, 4, 8, 16, 3
    eng_a, a = _engine(n, games, k, seed)
    eng_b, b = _engine(n, games, k, seed)
    a.reset()
    b.reset()
    _step(a, 3, count, k)
    _step(b, 3, count, k)
    before = (a.game_info(), a.root_stats(), eng_a.stats())
    boards, turns = VD.set_b(n)
    eng_a.env_vcf_defend(boards[:16], turns[:16], 8, 4096)
    after = (a.game_info(), a.root_stats(), eng_a.stats())
    for x, y in zip(before[0] + before[1], after[0] + after[1]):
        assert np.array_equal(x, y)
    assert before[2] == after[2]  # every counter and every accumulated time: nothing of the engine's ran
    _step(a, 2, count, k)  # ... and the episode goes on as the twin's that never made the call
    _step(b, 2, count, k)
    for x, y in zip(a.game_info() + a.root_stats(), b.game_info() + b.root_stats()):
        assert np.array_equal(x, y)
    for g in range(games):
        for side in (0, 1):
            (ai, af), (bi, bf) = a.tree_dump(g, side), b.tree_dump(g, side)
            assert np.array_equal(ai, bi) and np.array_equal(af.view(np.uint32), bf.view(np.uint32))
    eng_a.close()
    eng_b.close()


# ---- 6. the report on the records of an episode, and its command line -------------------------------------------------------------------
def test_the_report_of_an_episode_equals_the_walk_and_the_cli_prints_its_sums(tmp_path, capsys):
    n, games, k, seed, depth, budget = 9, 6, 8, 3, 6, 4096
    eng, sp = _engine(n, games, k, seed)
    sp.game_log(True)
    sp.reset()
    for _ in range(n * n):  # OMOK_OPP_VCF (Black) against OMOK_OPP_THREAT (White), both moves chosen on the device
        if sp.alive_count == 0:
            break
        sp.opponent_actions(B.OPP_VCF if (sp.ply & 1) == 0 else B.OPP_THREAT)
        sp.advance()
    assert sp.alive_count == 0
    rec = sp.game_records()
    rec.verify(eng)
    f = rec.vcf_defence(eng, max_depth=depth, max_nodes=budget)
    sums = {name: np.zeros(2, dtype=np.int64) for name in VD.NAMES}
    for g in range(games):
        length = int(rec.lengths[g])
        before, want = VD.report(n, rec.start_boards[g], [int(c) for c in rec.cells[g, :length]], int(rec.status[g]), depth, budget)
        assert [int(x) for x in f["threat_before"][g, :length]] == before and not f["threat_before"][g, length:].any(), f"game {g}"
        for name in VD.NAMES:
            assert f[name][g].tolist() == want[name], (g, name)
            sums[name] += want[name]
    print(f"status {rec.status.tolist()}, lengths {rec.lengths.tolist()}, " + ", ".join(f"{k_} {v.tolist()}" for k_, v in sums.items()))
    assert sums["threatened"].sum() > 0
    eng.close()
    path = str(tmp_path / "games.npz")
    rec.save(path)
    capsys.readouterr()
    assert R.main(["defence", path, "--max-depth", str(depth), "--max-nodes", str(budget)]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("defence: ")]
    assert len(lines) == 1
    out = json.loads(lines[0][len("defence: "):])
    assert (out["games"], out["moves"], out["max_depth"], out["max_nodes"]) == (games, int(rec.lengths.sum()), depth, budget)
    assert out["budget_exhausted"] == int((f["threat_before"] < 0).sum())
    for s, name in ((0, "black"), (1, "white")):
        assert out[name] == {key: int(sums[key][s]) for key in VD.NAMES}
