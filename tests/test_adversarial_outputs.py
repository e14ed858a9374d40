"""The yardstick of tests/test_gpu_injected_outputs.py, checked without a GPU: on the adversarial rows of
tests/adversarial_outputs.py (finite rows only: see that module's docstring for why NaN and +-inf have no yardstick) the arena
oracle and the literal oracle agree in every bit, the rows reach the branches they aim at often enough (coverage floors), the
stream matters (a search without the EPS rule, or one that flushes denormals, plays differently), and ties between visited
children go to the LAST maximum."""
import functools

import numpy as np
import pytest

import adversarial_outputs as AO
from omok_ai_amd import weights
from oracle import oracle as O
from helpers import draw_sequence
from test_oracle_literal import _compare, _perm

ARENA = {9: (2048, 1024), 15: (2048, 1024)}


@functools.lru_cache(maxsize=None)
def _root_row(n):
    """the reset's root row: the random-init net's, from the oracle's own forward (the GPU test takes the engine's)"""
    return O.Net(n, weights.init_random(n, seed=0)).forward(O.Environment(n).encode_nn_input(0)[None])[0][0]


def predicted_path(ints, floats):
    """the nodes the next simulation descends through (last maximum at every fully expanded node), with the ties met on the way:
    [(node, first-maximum child, last-maximum child)]"""
    node, ties = 0, []
    while ints[node, 5] == ints[node, 4] and ints[node, 5] > 0:
        kids, _, keys = AO.puct_scores(ints, floats, node)
        first, last = AO.first_and_last_max(keys)
        if AO.is_tie_node(ints, floats, node):
            ties.append((node, int(kids[first]), int(kids[last])))
        node = int(kids[last])
    return ties


def drive(case, transform=None, literal=True, tie_rule=False):
    """One configuration on the arena oracle (and the literal one) with the generator's rows.  transform(p, v, inputs) -> (p, v)
    rewrites every batch (v is None for a mirror batch).  Returns (coverage counts, trace, tie statistics): the trace is every move
    and every after-execute dump, as bytes."""
    name, n, games, count, k, max_plies, st = case
    eps, alpha = st.get("epsilon", 0.25), 0.03
    temperature, threshold, seed = st.get("temperature", 1.0), st.get("threshold", 6), st["kind_seed"]
    no_noise, opening = eps == 0.0, st.get("opening", 0)
    cap_nodes, cap_tables = ARENA[n]
    A = O.SelfPlay(n, games, cap_nodes=cap_nodes, cap_tables=cap_tables, seed=st.get("seed", 7), game_offset=5)
    L = O.Literal(n, games, seed=st.get("seed", 7), game_offset=5, cap_nodes=cap_nodes) if literal else None
    A.reset(_root_row(n))
    if L:
        L.reset(_root_row(n))
    counts, trace, ply = {}, [], 0
    ties = {"on_path": 0, "strict": 0}
    rounds = (count + k - 1) // k
    for cell in draw_sequence(n)[:opening]:  # the opening: external moves, no search
        acts = np.full(games, cell, dtype=np.int32)
        A.set_actions(acts)
        m = A.mirror_generate()
        pm = AO.mirror_rows(seed, ply, m, no_noise)
        if transform:
            pm, _ = transform(pm, None, m)
        if L:
            L.set_actions(acts)
            ml, mg = L.mirror_generate()
            perm = _perm(list(range(games)), mg)
            assert np.array_equal(ml, m[perm])
            L.advance(pm[perm], external=True)
        A.advance(pm)
        assert A.error == 0 and A.alive_count == games
        ply += 1
    if L and opening:
        _compare(A, L, games, f"{name}: after the opening")
    while A.alive_count > 0 and (max_plies == 0 or ply - opening < max_plies):
        side = ply & 1
        watch = []
        for rnd in range(rounds):
            x = A.round_generate(rnd, k, eps, alpha)
            if L:
                xl, gl = L.round_generate(rnd, k, eps, alpha)
                assert len(xl) == len(x), f"{name}: ply {ply} round {rnd}: request count"
                perm = _perm([A.request_info(r)[0] for r in range(len(x))], gl)
                assert np.array_equal(xl, x[perm]), f"{name}: ply {ply} round {rnd}: request boards"
            p, v = AO.rows(seed, ply, rnd, x, AO.root_candidates(A, side, len(x)) if no_noise else False)
            if transform:
                p, v = transform(p, v, x)
            A.round_scatter(p, v)
            if L:
                L.round_scatter(p[perm], v[perm])
            if tie_rule:
                for g, first, last, n_first, n_last in watch:  # the descent that followed the dump took the last maximum
                    ints, _ = A.tree_dump(g, side)
                    assert ints[last, 6] > n_last, f"{name}: ply {ply} round {rnd} game {g}: the tie went elsewhere"
                    ties["on_path"] += 1
                    ties["strict"] += int(ints[first, 6] == n_first)
                watch = []
                if rnd + 1 < rounds:  # (round 0 lays noise over the root row first: its descents do not read this dump)
                    for g in range(games):
                        if A.game_alive(g):
                            ints, floats = A.tree_dump(g, side)
                            for node, first, last in predicted_path(ints, floats):
                                assert first != last
                                watch.append((g, first, last, int(ints[first, 6]), int(ints[last, 6])))
        assert A.error == 0
        if L:
            _compare(A, L, games, f"{name}: ply {ply} after execute")
        dumps = [A.tree_dump(g, side) for g in range(games) if A.game_alive(g)]
        assert all(np.isfinite(f).all() for _, f in dumps), f"{name}: ply {ply}: a non-finite w or policy entry"
        counts = AO.add_counts(counts, AO.coverage(dumps + [A.tree_dump(g, 1 - side) for g in range(games) if A.game_alive(g)]))
        trace += [d.tobytes() for pair in dumps for d in pair]
        acts = A.sample(temperature, threshold)
        trace.append(acts.tobytes())
        if L:
            assert np.array_equal(acts, L.sample(temperature, threshold)), f"{name}: ply {ply}: actions"
        m = A.mirror_generate()
        pm = AO.mirror_rows(seed, ply, m, no_noise)
        if transform:
            pm, _ = transform(pm, None, m)
        alive = [g for g in range(games) if A.game_alive(g)]
        if L:
            ml, mg = L.mirror_generate()
            perm = _perm(alive, mg)
            assert np.array_equal(ml, m[perm]), f"{name}: ply {ply}: mirror inputs"
            L.advance(pm[perm])
            assert L.error == 0
        A.advance(pm)
        assert A.error == 0
        counts = AO.add_counts(counts, AO.coverage([A.tree_dump(g, sd) for g in alive if A.game_alive(g) for sd in (0, 1)]))
        if L:
            _compare(A, L, games, f"{name}: ply {ply} after advance")
            for g in range(games):
                assert A.game_status(g) == L.game_status(g) and A.game_plies(g) == L.game_plies(g)
        ply += 1
    for g in range(games):
        rep = A.replay(g)
        trace += [r.tobytes() for r in rep]
        if L:
            for a, b in zip(rep, L.replay(g)):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{name}: replay of game {g}"
    return counts, trace, ties


@functools.lru_cache(maxsize=None)
def baseline(index):
    return drive(AO.CASES[index], tie_rule=True)


IDS = [c[0] for c in AO.CASES]


@pytest.mark.parametrize("index", range(len(AO.CASES)), ids=IDS)
def test_oracles_agree_and_floors_are_met(index):
    """identical trees, moves and replays on both oracles (asserted inside drive), and every reachable coverage count >= 10"""
    name, n, games, count, k, plies, st = AO.CASES[index]
    counts, _, _ = baseline(index)
    print(f"{name}: coverage {counts}")
    keys = AO.floor_keys(n, count, plies, st.get("epsilon", 0.25), st.get("opening", 0))
    assert "tie_nodes" in keys and "saturated_w" in keys  # (every configuration reaches PUCT)
    for key in keys:
        assert counts[key] >= AO.FLOOR, f"{name}: {key} = {counts[key]}"


def _no_eps(p, v, x):
    return AO.without_eps_rule(p, x), v


def _ftz(p, v, x):
    return AO.flush_denormals(p), None if v is None else AO.flush_denormals(v)


@pytest.mark.parametrize("transform", [_no_eps, _ftz], ids=["without_eps_rule", "flush_to_zero"])
@pytest.mark.parametrize("index", range(len(AO.CASES)), ids=IDS)
def test_stream_is_sensitive(index, transform):
    """a search that renormalises below EPS, or reads denormals as zero, leaves another tree or plays another move"""
    _, trace, _ = baseline(index)
    _, other, _ = drive(AO.CASES[index], transform=transform, literal=False)
    assert other != trace


def test_ties_go_to_the_last_maximum():
    """Over the tie nodes the next descent met (a dump is taken after every scatter; the nodes on the path of the simulation that
    follows are the ones whose choice shows): first and last maximum name different children and the visit went to the last (asserted
    in drive); in `strict` of them the first maximum's count did not move at all during the round.  A tie node off that path shows no
    choice until a descent reaches it, and then it is on the path of that round.  At K = 1 a round is one simulation, so the check is per
    simulation there and every instance must be strict: the one descent went to the last maximum and nowhere else."""
    total = {"on_path": 0, "strict": 0}
    for index, case in enumerate(AO.CASES):
        ties = baseline(index)[2]
        print(f"tie rule, {case[0]}: {ties}")
        if case[4] == 1:
            assert ties["on_path"] >= AO.FLOOR and ties["strict"] == ties["on_path"], (case[0], ties)
        total = AO.add_counts(total, ties)
    assert total["on_path"] >= AO.FLOOR and total["strict"] >= AO.FLOOR


def test_generator_is_deterministic_and_finite():
    x = np.zeros((5, 3 * 81), dtype=np.float32)
    x[:, 2 * 40] = 1.0
    a, b = AO.rows(3, 1, 2, x), AO.rows(3, 1, 2, x)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert not np.array_equal(AO.rows(3, 1, 3, x)[0], a[0])
    assert AO.occupied_cells(x)[:, 40].all() and AO.occupied_cells(x).sum() == 5
