"""The match yardstick itself (no GPU): with the same CPU net in both roles, the two-instance composition of tests/match_harness.py
reproduces a single oracle.SelfPlay episode (threshold = 0: Best every move) bit for bit -- trees, request boards, actions, statuses."""
import numpy as np
import pytest

from match_harness import MatchComposition
from oracle import oracle as O
import omok_ai_amd as oa


def _compare(single, comp, games, tag):
    for g in range(games):
        for side in (0, 1):
            si, sf = single.tree_dump(g, side)
            ci, cf = comp.tree_dump(g, side)
            assert np.array_equal(si, ci), f"{tag}: game {g} side {side}: node records"
            assert np.array_equal(sf.view(np.uint32), cf.view(np.uint32)), f"{tag}: game {g} side {side}: w / policy bits"
            assert single.tree_root(g, side)[:2] == comp.tree_root(g, side)[:2]


@pytest.mark.parametrize("split", [2, 0, 5])
def test_composition_with_one_net_is_selfplay(split):
    n, games, k, rounds, seed, off = 9, 5, 4, 2, 3, 7
    net = O.Net(n, oa.weights.init_random(n, seed=1))
    root = O.Environment(n).encode_nn_input(0)[None]
    root_p = net.forward(root)[0].reshape(-1)
    single = O.SelfPlay(n, games, cap_nodes=512, cap_tables=256, seed=seed, game_offset=off)
    single.reset(root_p)
    comp = MatchComposition(n, games, split, root_p, root_p, seed=seed, game_offset=off, cap_nodes=512, cap_tables=256)
    _compare(single, comp, games, "reset")
    ply = 0
    while single.alive_count > 0 and ply < 24:
        for rnd in range(rounds):
            x = single.round_generate(rnd, k, 0.25, 0.03)
            cx, cg = comp.round_generate(rnd, k, 0.25, 0.03)
            assert np.array_equal(x, cx), f"ply {ply} round {rnd}: request boards"
            assert list(cg) == [single.request_info(r)[0] for r in range(len(x))]
            p, v = net.forward(x, threads=4) if len(x) else (np.zeros((0, n * n), np.float32), np.zeros(0, np.float32))
            single.round_scatter(p, v)
            comp.round_scatter(p, v)
        _compare(single, comp, games, f"ply {ply} after execute")
        for g in range(games):
            a, b = single.compute_policy(g), comp.compute_policy(g)
            assert (a is None) == (b is None) and (a is None or np.array_equal(a.view(np.uint32), b.view(np.uint32)))
        acts = single.sample(1.0, 0)
        assert np.array_equal(acts, comp.sample(1.0, 0)), f"ply {ply}: actions"
        m = single.mirror_generate()
        assert np.array_equal(m, comp.mirror_generate(acts))
        pm = net.forward(m, threads=4)[0] if len(m) else np.zeros((0, n * n), np.float32)
        single.advance(pm)
        comp.advance(pm)
        _compare(single, comp, games, f"ply {ply} after advance")
        assert [single.game_status(g) for g in range(games)] == [comp.game_status(g) for g in range(games)]
        assert single.error == 0 and comp.error == 0
        ply += 1
    assert ply >= 9  # (games of at least nine plies: the trees went through several re-rootings)
