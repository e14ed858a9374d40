"""The engine on nets whose outputs are known in closed form (tests/head_bias_nets.py): first the outputs themselves on
the device, then the run loop (SelfPlay.run, the path bench.py times) against an oracle episode that was played on the analytic rows
alone and never saw a GPU value.  Every comparison is on bits."""
import functools

import numpy as np
import pytest

import omok_ai_amd as oa
from omok_ai_amd import binding as B
import adversarial_outputs as AO
import head_bias_nets as H
from helpers import compare_trees, drive_selfplay_vs_oracle, random_positions
from test_gpu_shared_tree import _engine as shared_engine, replay_recorded_on_literal

pytestmark = pytest.mark.gpu
MODES = {"default": B.NET_F16X3, "rows": B.NET_F16X3_ROWS, "fp6": B.NET_F16X3_FP6, "f16": B.NET_F16X3_F16, "mixed": B.NET_F16X3_MIXED, "f32": B.NET_F32}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", [9, 15])
def test_outputs_are_the_closed_forms(n, mode):
    """64 random positions: evaluate_pv is the expected (p, v) bit for bit; the logits and the value in front of tanh of a step-wise
    round are the biases"""
    x = random_positions(n, 64, 11)
    eng = oa.Engine(board_size=n, games=8, max_nodes=64, max_tables=32, max_batch_k=8, seed=3, net_mode=MODES[mode])
    for kind in H.KINDS:
        eng.load_weights(H.make(n, kind))
        p, v = eng.evaluate_pv(x)
        ep, ev = H.expected_rows(n, kind, len(x))
        bad = np.flatnonzero(_bits(p) != _bits(ep))
        assert bad.size == 0, f"{kind} {mode}: p differs at {bad[:4]}: {np.asarray(p).reshape(-1)[bad[:4]]!r} vs {ep.reshape(-1)[bad[:4]]!r}"
        assert np.array_equal(_bits(v), _bits(ev)), f"{kind} {mode}: v {np.asarray(v).reshape(-1)[:4]!r} vs {ev[0]!r}"
        sp = oa.SelfPlay(eng)
        sp.reset()
        nreq = sp.round_generate(0, 8, 0.25, 0.03)
        rp, rv = sp.round_eval()
        lg, vp = sp.round_logits()
        sp.round_scatter()
        L, b = H.head_biases(n, kind)
        assert nreq == 64 and np.array_equal(_bits(lg), _bits(np.tile(L, (nreq, 1)))) and np.array_equal(_bits(vp), _bits(np.full(nreq, b)))
        assert np.array_equal(_bits(rp), _bits(ep)) and np.array_equal(_bits(rv), _bits(ev))
    eng.close()


@functools.lru_cache(maxsize=None)
def _oracle(index):
    """(the oracle after its episode, coverage of its dumps): played once per case on the analytic rows, shared and left unchanged"""
    kind, n, games, count, k, plies, _, seed = H.RUN_CASES[index]
    total = {}

    def collect(dumps):
        total.update(AO.add_counts(total, AO.coverage(dumps)))
    osp = H.oracle_episode(n, kind, games, count, k, plies, seed, H.GAME_OFFSET, threshold=H.THRESHOLD, collect=collect)
    return osp, total


def _run_and_compare(index, lazy=True):
    """The coverage asserted here is counted on the ORACLE's dumps during its episode (run() has no point at which the device's trees could be
    read): it repeats the floors of tests/test_head_bias_nets.py and says what the episode contained; the device is compared on the final trees,
    status, plies and replay tuples."""
    kind, n, games, count, k, plies, mode, seed = H.RUN_CASES[index]
    osp, counts = _oracle(index)
    eng = oa.Engine(board_size=n, games=games, max_nodes=2048, max_tables=1024, max_batch_k=k, seed=seed, game_offset=H.GAME_OFFSET,
                    net_mode=MODES[mode])
    eng.load_weights(H.make(n, kind))
    if not lazy:
        eng.set_lazy_policy(False)
    sp = oa.SelfPlay(eng)
    sp.reset()
    sp.run(count, k, 0.25, 0.03, 1.0, H.THRESHOLD, max_plies=plies)
    tag = f"{kind} n={n} {mode} lazy={lazy}"
    compare_trees(sp, osp, games, tag)
    alive, status, nply = sp.game_info()
    assert [int(a) for a in alive] == [osp.game_alive(g) for g in range(games)], tag
    assert [int(s) for s in status] == [osp.game_status(g) for g in range(games)], tag
    assert [int(q) for q in nply] == [osp.game_plies(g) for g in range(games)], tag
    for g in range(games):
        for a, b in zip(sp.replay(g), osp.replay(g)):
            assert a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), f"{tag}: replay of game {g}"
    stats = eng.lazy_policy_stats()
    eng.close()
    print(f"{tag}: plies {[int(q) for q in nply]}, lazy rows {stats}, coverage {counts}")
    for key in H.floor_keys(kind, n, count, plies):
        assert counts[key] >= AO.FLOOR, f"{tag}: {key} = {counts[key]}"
    return stats


@pytest.mark.parametrize("index", range(len(H.RUN_CASES)), ids=[f"{c[0]}_n{c[1]}_{c[6]}" for c in H.RUN_CASES])
def test_run_loop_equals_the_oracle_on_analytic_rows(index):
    """the three nets at board 9 (8 games, 32 / 8, whole games, mixed format) and flat / sparse at board 15 in the DEFAULT mode (8 games,
    64 / 16, 12 plies): lazy rows, base cache and sibling differences of the headline path, bit for bit against the oracle"""
    stats = _run_and_compare(index)
    if H.RUN_CASES[index][:2] == ("sparse", 9):
        assert stats["noise"] > 0 and stats["descent"] > 0, stats


def test_run_loop_with_eager_rows_equals_the_oracle():
    """sparse at board 9 with set_lazy_policy(False): k_softmax_scatter_policy stores every row of the run loop's rounds"""
    stats = _run_and_compare(1, lazy=False)
    assert stats == {"noise": 0, "descent": 0}, stats


def test_stepwise_path_on_the_sparse_net():
    """drive_selfplay_vs_oracle given the sparse net's tensors: k_scatter_policy sees what k_softmax_scatter_policy saw"""
    kind, n, games, count, k, plies, mode, seed = H.RUN_CASES[1]
    drive_selfplay_vs_oracle(n, games, count, k, plies, MODES[mode], threshold=H.THRESHOLD, seed=seed, game_offset=H.GAME_OFFSET,
                             tensors=H.make(n, kind))


def test_slots_mode_equals_the_oracle_episode_game_by_game():
    """run_slots with the sparse net at board 9: 4 slots play 10 games (finished slots restart with the next game index) and every game's
    packed records and status must be those of the same game index in the ORACLE's episode of all 10 games on the analytic rows: the slot
    scheduler on zero rows, p = 0 and v = 1.  Record layout as tests/test_gpu_boundary.py reads it: board [HW], turn, pad to 4 bytes,
    pi [HW] float32, z float32."""
    import torch
    kind, n, _, count, k, _, mode, seed = H.RUN_CASES[1]
    slots, total, hw = 4, 10, n * n
    osp = H.oracle_episode(n, kind, total, count, k, 0, seed, H.GAME_OFFSET, threshold=H.THRESHOLD)
    eng = oa.Engine(board_size=n, games=slots, max_nodes=2048, max_tables=1024, max_batch_k=k, seed=seed, game_offset=H.GAME_OFFSET,
                    net_mode=MODES[mode])
    eng.load_weights(H.make(n, kind))
    sp = oa.SelfPlay(eng)
    sp.reset()
    rec = sp.replay_record_bytes()
    brd = (hw + 1 + 3) // 4 * 4
    assert rec == brd + 4 * hw + 4
    cap = total * hw
    buf = torch.zeros(cap * rec, dtype=torch.uint8, device="cuda")
    _, nrec, off, ln, status = sp.run_slots(total, count, k, buf.data_ptr(), cap, 0.25, 0.03, 1.0, H.THRESHOLD)
    out = buf.cpu().numpy().reshape(-1, rec)
    assert sp.alive_count == 0 and nrec == sum(osp.game_plies(g) for g in range(total))
    covered = np.zeros(nrec, dtype=bool)
    for g in range(total):
        b, t, pi, z = osp.replay(g)
        assert ln[g] == len(t), f"game {g}: {ln[g]} vs {len(t)} transitions"
        assert status[g] == osp.game_status(g), f"game {g}: status"
        got = out[off[g]:off[g] + ln[g]]
        assert np.array_equal(got[:, :hw], b) and np.array_equal(got[:, hw], t) and np.all(got[:, hw + 1:brd] == 0), f"game {g}: boards"
        assert np.array_equal(np.ascontiguousarray(got[:, brd:brd + 4 * hw]).view(np.uint32), pi.view(np.uint32)), f"game {g}: pi bits"
        assert np.array_equal(np.ascontiguousarray(got[:, brd + 4 * hw:]).view(np.uint32).reshape(-1), z.view(np.uint32)), f"game {g}: z bits"
        assert not covered[off[g]:off[g] + ln[g]].any()
        covered[off[g]:off[g] + ln[g]] = True
    assert covered.all()
    eng.close()


def test_shared_tree_with_one_wave_is_the_sequential_executor_on_the_flat_net():
    """execute_shared(waves = 1) equals execute for 6 plies, without noise (epsilon = 0: under noise the root's priors are all distinct and
    nothing ties at the maximum).  The flat root row is then exactly uniform; 100 simulations on at most 81 cells expand every child once
    (n = 1, w = +0.0) and the rest descend: at the end of every ply the maximal score is shared by the children still at n = 1, so every
    ply's root is a tie node and each of those descents was decided by rank alone."""
    n, count, k, plies = 9, 100, 8, 6
    tensors = H.make(n, "flat")
    a_eng, a = shared_engine(n, k, 5, 0, net_mode=B.NET_F16X3_MIXED, tensors=tensors)
    b_eng, b = shared_engine(n, k, 5, 1, net_mode=B.NET_F16X3_MIXED, tensors=tensors)
    ties = 0
    for ply in range(plies):
        a.execute(count, k, 0.0, 0.03)
        b.execute_shared(count, k, 0.0, 0.03, waves=1)
        for side in (0, 1):
            ai, af = a.tree_dump(0, side)
            bi, bf = b.tree_dump(0, side)
            assert np.array_equal(ai, bi) and np.array_equal(af.view(np.uint32), bf.view(np.uint32)), f"ply {ply} side {side}"
            assert a.tree_root(0, side) == b.tree_root(0, side)
        ints, floats = a.tree_dump(0, ply & 1)
        assert ints[0, 5] == ints[0, 4], f"ply {ply}: the root is not fully expanded"
        ties += int(AO.is_tie_node(ints, floats, 0))
        assert np.array_equal(a.sample_actions(1.0, 4), b.sample_actions(1.0, 4))
        a.advance()
        b.advance()
    a_eng.close()
    b_eng.close()
    print(f"flat net, shared tree with one wave, no noise: {ties} of {plies} roots are tie nodes")
    assert ties == plies


def test_recorded_shared_tree_replays_on_the_literal_oracle_on_the_flat_net():
    """one execute_shared_recorded replay (W = 8) against lit_shared_*, as tests/test_gpu_shared_tree.py does with the random-init net"""
    replay_recorded_on_literal(9, 256, 8, 8, 6, tensors=H.make(9, "flat"))
