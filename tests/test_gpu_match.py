"""Match episodes (omok_match_reset: net 1 against net 2, benchmark/src/main.rs) on the GPU.

The yardstick is tests/match_harness.py: two oracle.SelfPlay instances, each reset with one net's root policy and compared on the trees
that net owns (tree side * G + g belongs to net side ^ (g >= split)).  The oracle consumes the GPU nets' p / v, so the comparisons
isolate the routing and the tree arithmetic; test_sibling_round_rows_use_their_own_net checks the p / v themselves against each net's
fp32 CPU forward.
"""
import numpy as np
import pytest

import omok_ai_amd as oa
from omok_ai_amd import binding as B
from omok_ai_amd import match as M
from oracle import oracle as O
from match_harness import MatchComposition

pytestmark = pytest.mark.gpu


def _compare_trees(sp, comp, games, tag):
    for g in range(games):
        for side in (0, 1):
            gi, gf = sp.tree_dump(g, side)
            oi, of = comp.tree_dump(g, side)
            assert gi.shape == oi.shape, f"{tag}: game {g} side {side}: {gi.shape[0]} vs {oi.shape[0]} nodes"
            assert np.array_equal(gi, oi), f"{tag}: node records differ (game {g} side {side})"
            assert np.array_equal(gf.view(np.uint32), of.view(np.uint32)), f"{tag}: w/policy bits differ (game {g} side {side})"
            assert sp.tree_root(g, side)[:2] == comp.tree_root(g, side)[:2], f"{tag}: root n / w (game {g} side {side})"


def _match_engine(n, games, k, mode, w1, w2, seed=7, game_offset=5, max_nodes=2048, max_tables=1024):
    eng = oa.Engine(board_size=n, games=games, max_nodes=max_nodes, max_tables=max_tables, max_batch_k=k, seed=seed, game_offset=game_offset,
                    net_mode=mode)
    eng.load_weights(w1)
    eng.load_weights2(w2)
    return eng


def _root_policy(n, k, mode, tensors):
    """evaluate_p of the empty board by a net of its own (net 1 of a separate engine: the same forward as the match engine's slot)"""
    e = oa.Engine(board_size=n, games=1, max_nodes=8, max_tables=4, max_batch_k=k, net_mode=mode)
    e.load_weights(tensors)
    p = e.evaluate_p(O.Environment(n).encode_nn_input(0)[None]).reshape(-1)
    e.close()
    return p


def _check_own_net(cpu, x, p, v, row_games, tree_side, split, rng, tag, per_class=2):
    """A few rows of each colour class (games < split, games >= split): p (and v) within 1e-3 of the fp32 CPU forward of the net that owns
    the row's tree (tree_side * G + g: net tree_side ^ (g >= split)) and outside 1e-3 of the other net's"""
    row_games = np.asarray(row_games)
    for cls in (0, 1):
        cand = np.nonzero((row_games >= split) == bool(cls))[0]
        if len(cand) == 0:
            continue
        rows = rng.choice(cand, min(per_class, len(cand)), replace=False)
        own = tree_side ^ cls
        for net, far in ((own, False), (1 - own, True)):
            pc, vc = cpu[net].forward(x[rows], threads=8)
            d = np.abs(p[rows] - pc).max(axis=1)
            if v is not None:
                d = np.maximum(d, np.abs(v[rows] - vc))
            if far:
                assert np.all(d > 1e-3), f"{tag}: rows of class {cls} also match the other net ({d.min():.2e})"
            else:
                assert np.all(d < 1e-3), f"{tag}: rows of class {cls} vs their own net: {d.max():.2e}"


def _drive_match(n, games, split, count, k, max_plies, mode, threshold=0, seed=7, game_offset=5, max_nodes=2048, max_tables=1024):
    w1, w2 = oa.weights.init_random(n, seed=1), oa.weights.init_random(n, seed=2)
    cpu = [O.Net(n, w1), O.Net(n, w2)]
    rng = np.random.default_rng(split)
    eng = _match_engine(n, games, k, mode, w1, w2, seed, game_offset, max_nodes, max_tables)
    sp = oa.SelfPlay(eng)
    sp.match_reset(split)
    comp = MatchComposition(n, games, split, _root_policy(n, k, mode, w1), _root_policy(n, k, mode, w2), seed=seed, game_offset=game_offset,
                            cap_nodes=max_nodes, cap_tables=max_tables)
    _compare_trees(sp, comp, games, "reset")
    rounds = (count + k - 1) // k
    pis = {g: [] for g in range(games)}
    ply = 0
    while comp.alive_count > 0 and (max_plies == 0 or ply < max_plies):
        for rnd in range(rounds):
            nreq = sp.round_generate(rnd, k, 0.25, 0.03)
            cx, cg = comp.round_generate(rnd, k, 0.25, 0.03)
            assert nreq == len(cx), f"ply {ply} round {rnd}: request count"
            assert np.array_equal(sp.round_inputs(), cx), f"ply {ply} round {rnd}: request boards"
            _compare_trees(sp, comp, games, f"ply {ply} after generate of round {rnd}")
            p, v = sp.round_eval()
            if rnd == rounds - 1 and nreq:
                _check_own_net(cpu, cx, p, v, cg, ply & 1, split, rng, f"ply {ply} round {rnd}")
            sp.round_scatter()
            comp.round_scatter(p, v)
        _compare_trees(sp, comp, games, f"ply {ply} after execute")
        assert comp.error == 0
        pi, has = sp.compute_policy()
        for g in range(games):
            c = comp.compute_policy(g)
            assert bool(has[g]) == (c is not None), f"ply {ply} game {g}: has_policy"
            if c is not None:
                assert np.array_equal(pi[g].view(np.uint32), c.view(np.uint32)), f"ply {ply} game {g}: pi"
                pis[g].append(c)
        a = sp.sample_actions(1.0, threshold)
        assert np.array_equal(a, comp.sample(1.0, threshold)), f"ply {ply}: actions"
        live = [g for g in range(games) if comp.game_alive(g)]
        nm = sp.mirror_generate()
        om = comp.mirror_generate(a)
        assert nm == len(om) and np.array_equal(sp.mirror_inputs(), om), f"ply {ply}: mirror inputs"
        pm = sp.mirror_eval()
        _check_own_net(cpu, om, pm, None, live, 1 - (ply & 1), split, rng, f"ply {ply}: mirror rows")  # the opponent tree's net
        sp.mirror_apply()
        comp.advance(pm)
        _compare_trees(sp, comp, games, f"ply {ply} after advance")
        alive, status, _ = sp.game_info()
        assert [int(x) for x in alive] == [comp.game_alive(g) for g in range(games)]
        assert [int(x) for x in status] == [comp.game_status(g) for g in range(games)]
        ply += 1
    for g in range(games):  # the replay's pi = the mover's own tree's compute_policy
        _, _, gp, _ = sp.replay(g)
        assert len(gp) == len(pis[g])
        for r, c in zip(gp, pis[g]):
            assert np.array_equal(r.view(np.uint32), c.view(np.uint32))
    eng.close()
    return ply


@pytest.mark.parametrize("n,games,split,count,k,max_plies,mode", [
    (9, 8, 4, 32, 8, 0, B.NET_F16X3),          # whole games, both colour classes
    (15, 4, 2, 64, 16, 6, B.NET_F16X3_ROWS),   # the benchmark board
    (9, 4, 0, 16, 8, 10, B.NET_F16X3),         # net 2 is Black everywhere
    (9, 4, 4, 16, 8, 10, B.NET_F16X3),         # net 1 is Black everywhere
])
def test_match_stepwise_bit_exact_vs_composition(n, games, split, count, k, max_plies, mode):
    plies = _drive_match(n, games, split, count, k, max_plies, mode)
    assert plies >= min(max_plies or 9, 6)


def _episode(sp, games):
    out = []
    alive, status, plies = sp.game_info()
    for g in range(games):
        b, t, pi, z = sp.replay(g)
        out.append((b.copy(), t.copy(), pi.view(np.uint32).copy(), z.view(np.uint32).copy(), int(status[g]), int(plies[g])))
    return out


def _same_episode(a, b):
    assert len(a) == len(b)
    for g, (x, y) in enumerate(zip(a, b)):
        for i in range(4):
            assert np.array_equal(x[i], y[i]), f"game {g}: replay field {i}"
        assert x[4:] == y[4:], f"game {g}: status / plies"


@pytest.mark.parametrize("n,games,count,k,max_plies,mode", [
    (9, 8, 32, 8, 0, B.NET_F16X3),
    (15, 4, 48, 16, 8, B.NET_F16X3_ROWS),
])
def test_same_net_in_both_slots_is_selfplay(n, games, count, k, max_plies, mode):
    w = oa.weights.init_random(n, seed=3)
    ref = oa.Engine(board_size=n, games=games, max_nodes=2048, max_tables=1024, max_batch_k=k, seed=11, net_mode=mode)
    ref.load_weights(w)
    rsp = oa.SelfPlay(ref)
    rsp.reset()
    rsp.run(count, k, threshold=0, max_plies=max_plies)
    want = _episode(rsp, games)
    ref.close()
    eng = _match_engine(n, games, k, mode, w, w, seed=11, game_offset=0)
    sp = oa.SelfPlay(eng)
    for split in (games // 2, 0, games):
        sp.set_episode(0)
        sp.match_reset(split)
        sp.run(count, k, threshold=0, max_plies=max_plies)
        _same_episode(_episode(sp, games), want)
    eng.close()


def test_sibling_round_rows_use_their_own_net():
    """N = 15, default net mode, 256 games x K = 16: each net's block of a round is >= 2048 rows of a 4096-row round, which takes the
    difference path of the sibling evaluation (k_sib_children2).  Every row's logits must be its OWN net's (fp32 CPU forward, 1e-3) and
    clearly not the other net's; the trees must still follow the composition fed with the GPU's p / v."""
    n, games, split, k, count = 15, 256, 128, 16, 48
    w = [oa.weights.init_random(n, seed=1), oa.weights.init_random(n, seed=2)]
    eng = _match_engine(n, games, k, B.NET_F16X3, w[0], w[1], seed=3, game_offset=0, max_nodes=512, max_tables=128)
    cpu = [O.Net(n, w[0]), O.Net(n, w[1])]
    sp = oa.SelfPlay(eng)
    sp.match_reset(split)
    comp = MatchComposition(n, games, split, _root_policy(n, k, B.NET_F16X3, w[0]), _root_policy(n, k, B.NET_F16X3, w[1]), seed=3,
                            cap_nodes=512, cap_tables=128)
    rng = np.random.default_rng(0)
    launches = eng.stats()["children2_launches"]
    checked = {0: 0, 1: 0}
    for ply in range(2):
        side = ply & 1
        for rnd in range(count // k):
            nreq = sp.round_generate(rnd, k, 0.25, 0.03)
            cx, cg = comp.round_generate(rnd, k, 0.25, 0.03)
            x = sp.round_inputs()
            assert np.array_equal(x, cx)
            p, v = sp.round_eval()
            lg, vp = sp.round_logits()
            sp.round_scatter()
            comp.round_scatter(p, v)
            if rnd == 0:
                continue  # (one request per tree: no siblings)
            assert nreq == games * k
            for cls in (0, 1):  # rows of games < split and of games >= split
                rows = rng.choice(np.nonzero((cg >= split) == bool(cls))[0], 6, replace=False)
                own = side ^ cls
                for net, far in ((own, False), (1 - own, True)):
                    _, _, l32, v32 = cpu[net].forward_logits(x[rows], threads=8)
                    d = np.maximum(np.abs(lg[rows] - l32.reshape(len(rows), -1)).max(axis=1), np.abs(vp[rows] - v32.reshape(-1)))
                    if far:
                        assert np.all(d > 1e-3), f"ply {ply} round {rnd}: rows of class {cls} also match the other net ({d.min():.2e})"
                    else:
                        assert np.all(d < 1e-3), f"ply {ply} round {rnd}: rows of class {cls} vs their own net: {d.max():.2e}"
                checked[own] += len(rows)
        _compare_trees(sp, comp, games, f"ply {ply} after execute")
        a = sp.sample_actions(1.0, 0)
        assert np.array_equal(a, comp.sample(1.0, 0))
        live = [g for g in range(games) if comp.game_alive(g)]
        sp.mirror_generate()
        om = comp.mirror_generate(a)
        assert np.array_equal(sp.mirror_inputs(), om)
        pm = sp.mirror_eval()
        _check_own_net(cpu, om, pm, None, live, 1 - side, split, rng, f"ply {ply}: mirror rows", per_class=6)  # the opponent tree's net
        sp.mirror_apply()
        comp.advance(pm)
        _compare_trees(sp, comp, games, f"ply {ply} after advance")
    assert eng.stats()["children2_launches"] > launches
    assert checked[0] > 0 and checked[1] > 0
    ev = eng.net2_info()["evals"]
    assert ev[0] > 0 and ev[1] > 0
    eng.close()


def test_match_front_end(tmp_path):
    n = 15
    paths = []
    for s in (1, 2):
        p = str(tmp_path / f"net{s}.bin")
        oa.model_file.save(p, oa.weights.tensor_names(), oa.weights.init_random(n, seed=s))
        paths.append(p)
    argv = paths + ["--games", "512", "--sims", "32", "--batch", "16", "--board", "15", "--seed", "5"]
    r1 = M.main(argv)
    r2 = M.main(argv)
    assert r1["wins"] + r1["losses"] + r1["draws"] == 512
    assert (r1["wins"], r1["losses"], r1["draws"]) == M.tally(r1["status"], 256)
    assert all(s in (oa.api.DRAW, oa.api.BLACK_WIN, oa.api.WHITE_WIN) for s in r1["status"])
    assert r1 == r2
    assert r1["evals"][0] > 0 and r1["evals"][1] > 0


def test_selfplay_after_a_match_is_fresh_selfplay():
    """No routing state or cached base evaluation outlives a match: omok_selfplay_reset + self-play after a match (sibling path: 256 games
    x K = 16 at N = 15) is bit-identical to the same episode on a fresh engine."""
    n, games, k, count, plies = 15, 256, 16, 48, 3
    w1, w2 = oa.weights.init_random(n, seed=1), oa.weights.init_random(n, seed=2)
    ref = oa.Engine(board_size=n, games=games, max_nodes=512, max_tables=128, max_batch_k=k, seed=9)
    ref.load_weights(w1)
    rsp = oa.SelfPlay(ref)
    rsp.reset()
    rsp.run(count, k, max_plies=plies)
    want = _episode(rsp, games)
    ref.close()
    eng = _match_engine(n, games, k, B.NET_F16X3, w1, w2, seed=9, game_offset=0, max_nodes=512, max_tables=128)
    sp = oa.SelfPlay(eng)
    sp.match_reset(games // 2)
    sp.run(count, k, threshold=0, max_plies=plies)
    sp.set_episode(0)
    sp.reset()
    sp.run(count, k, max_plies=plies)
    _same_episode(_episode(sp, games), want)
    eng.close()


def test_match_errors():
    n, games, k = 9, 4, 8
    eng = oa.Engine(board_size=n, games=games, max_nodes=256, max_tables=128, max_batch_k=k)
    eng.load_random_weights(1)
    sp = oa.SelfPlay(eng)
    with pytest.raises(B.OmokError) as ei:
        sp.match_reset(2)
    assert ei.value.code == -3  # OMOK_ERR_STATE: no net 2
    with pytest.raises(B.OmokError) as ei:
        eng.net2_info()
    assert ei.value.code == -3
    eng.load_weights2(oa.weights.init_random(n, seed=2))
    assert eng.net2_info()["fc0_format"] in ("fp6", "f16", "mixed", "f32")
    for bad in (-1, games + 1):
        with pytest.raises(B.OmokError) as ei:
            sp.match_reset(bad)
        assert ei.value.code == -1  # OMOK_ERR_INVALID
    sp.match_reset(2)
    sp.execute(16, k)
    before = [sp.tree_dump(g, s) for g in range(games) for s in (0, 1)], sp.game_info()
    acts = sp.sample_actions(1.0, 0)
    calls = [lambda: sp.play_actions(acts), lambda: sp.execute_shared(16, k, waves=1),
             lambda: sp.run_slots(2 * games, 16, k, 1, 1024)]
    for call in calls:
        with pytest.raises(B.OmokError) as ei:
            call()
        assert ei.value.code == -3 and "match" in str(ei.value)
    after = [sp.tree_dump(g, s) for g in range(games) for s in (0, 1)], sp.game_info()
    for (a, b), (c, d) in zip(before[0], after[0]):
        assert np.array_equal(a, c) and np.array_equal(b.view(np.uint32), d.view(np.uint32))
    for x, y in zip(before[1], after[1]):
        assert np.array_equal(x, y)
    sp.advance()  # the match goes on
    sp.reset()    # and self-play takes over again
    sp.execute(16, k)
    eng.close()
