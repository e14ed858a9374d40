"""The scripted finishes that tests/test_gpu_launch_shapes.py plays to SET the number of live games (helpers.scripted_finish), checked
against the oracle's rules without a GPU: for every ladder point the script is legal, no surviving game finishes, every doomed game finishes
on the last ply with the intended status, and the live set is the intended one.  This is what keeps the GPU test from quietly checking fewer
rows than it claims.  Reference: environment/src/lib.rs:104-166 (place_stone)."""
import numpy as np
import pytest

from oracle import oracle as O
from helpers import LAUNCH_SHAPE_LADDER, scripted_finish


def _points():
    return sorted({(p["board"], p["games"], p["live"], p["winner"], p["pattern"]) for p in LAUNCH_SHAPE_LADDER})


def _play(n, actions):
    """final status per game (0 = in progress) and the ply it ended on, through the oracle's Environment"""
    plies, games = actions.shape
    status, ended = np.zeros(games, dtype=np.int32), np.full(games, -1, dtype=np.int32)
    for g in range(games):
        env = O.Environment(n)
        for ply in range(plies):
            s = env.place_stone(int(actions[ply, g]))
            assert s is not None, f"game {g} ply {ply}: occupied cell {actions[ply, g]}"
            assert ended[g] < 0, f"game {g} moves after it ended on ply {ended[g]}"
            if s != O.IN_PROGRESS:
                status[g], ended[g] = s, ply
    return status, ended


@pytest.mark.parametrize("n,games,live,winner,pattern", _points())
def test_scripted_finish_leaves_exactly_the_intended_games_alive(n, games, live, winner, pattern):
    actions, doomed, want = scripted_finish(n, games, live, 1, winner, pattern)
    plies = actions.shape[0]
    assert plies == (9 if winner == "black" else 10) and want == (O.BLACK_WIN if winner == "black" else O.WHITE_WIN)
    assert actions.shape == (plies, games) and int((~doomed).sum()) == live
    status, ended = _play(n, actions)
    assert np.all(status[~doomed] == O.IN_PROGRESS), "a surviving game finished"
    assert np.all(status[doomed] == want) and np.all(ended[doomed] == plies - 1), "a doomed game did not end on the last ply as intended"
    if games - live >= 2 and pattern == "permuted":
        assert doomed[0] and doomed[-1]
    if pattern == "alternate":
        assert not doomed[::2].any() or not doomed[1::2].any()
        assert np.all(doomed[1::2] != doomed[:-1:2][: len(doomed[1::2])])
    # survivors differ from game to game
    if live >= 2:
        alive = actions[:, ~doomed].T
        assert len({tuple(r) for r in alive}) == live


def test_the_ladder_has_dead_runs_of_varying_length_and_both_sides_to_move():
    winners = {p["winner"] for p in LAUNCH_SHAPE_LADDER}
    assert winners == {"black", "white"}
    assert any(p["pattern"] == "alternate" for p in LAUNCH_SHAPE_LADDER)
    _, doomed, _ = scripted_finish(15, 4096, 2700, 1)
    edges = np.flatnonzero(np.diff(np.concatenate(([0], doomed.astype(np.int8), [0]))))
    runs = edges[1::2] - edges[0::2]
    assert len(set(runs.tolist())) >= 4, "dead games come in runs of varying length"
