"""GPU test (run with -m gpu) of Parameters.selfplay_slots: the trainer mirror plays its iteration's games in slots mode
(omok_selfplay_run_slots on min(slots, episode_count) slots) and post-processes the raw records with omok_replay_augment_records_dev.  At board
size 9 slots mode reproduces the episode game by game (tests/test_gpu_slots.py), the new call reproduces the game-order layout
(tests/test_gpu_replay_records.py) and the native step is deterministic, so the two trainers must end with the same bits."""
import re

import numpy as np
import pytest

from omok_ai_amd import api
from omok_ai_amd import trainer as TR

pytestmark = pytest.mark.gpu


def _record_engines(monkeypatch):
    engines = []
    init = api.Engine.__init__

    def recording_init(self, *a, **kw):
        init(self, *a, **kw)
        engines.append((self, kw.get("games")))

    monkeypatch.setattr(api.Engine, "__init__", recording_init)
    return engines


def _train(tmp_path, name, slots, iterations=2):
    p = TR.Parameters(train_backend="hip", episode_count=12, selfplay_slots=slots, evaluate_count=16, evaluate_batch_size=8,
                      parameter_update_count=3, parameter_update_batch_size=16, evaluate_every=0)
    tr = TR.Trainer(p, board_size=9, seed=3, save_dir=str(tmp_path / name), precision_rows=0)
    logs = []
    tr.train(iterations, log=logs.append)
    return tr, logs


def test_slots_and_episode_trainers_end_with_the_same_weights(tmp_path, monkeypatch):
    engines = _record_engines(monkeypatch)
    slots_tr, slots_logs = _train(tmp_path, "slots", 5)
    assert engines == [(slots_tr.engine, 5)]  # the slots trainer's engine holds 5 games' trees, not 12
    episode_tr, episode_logs = _train(tmp_path, "episode", 0)
    assert engines[1:] == [(episode_tr.engine, 12)]
    assert len(slots_logs) == len(episode_logs) == 2
    for a, b in zip(slots_logs, episode_logs):
        ma, mb = (re.search(r"games=(\d+) transitions=(\d+)", line) for line in (a, b))
        assert ma and mb, (a, b)
        assert ma.groups() == mb.groups() and int(ma.group(1)) == 12 and int(ma.group(2)) > 0, (a, b)
    got, want = slots_tr.engine.read_weights(), episode_tr.engine.read_weights()
    assert len(got) == len(want) == 31
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(np.asarray(g).view(np.uint32), np.asarray(w).view(np.uint32)), f"tensor {i} differs"
    slots_tr.close()
    episode_tr.close()


def test_more_slots_than_games_are_clamped_and_a_negative_count_is_rejected(tmp_path, monkeypatch):
    engines = _record_engines(monkeypatch)
    with pytest.raises(ValueError):
        TR.Trainer(TR.Parameters(selfplay_slots=-1), board_size=9, save_dir=str(tmp_path / "bad"))
    assert engines == []  # rejected before any engine was created
    p = TR.Parameters(train_backend="hip", episode_count=4, selfplay_slots=50, evaluate_count=16, evaluate_batch_size=8,
                      parameter_update_count=2, parameter_update_batch_size=8, evaluate_every=0)
    tr = TR.Trainer(p, board_size=9, seed=3, save_dir=str(tmp_path / "clamped"), precision_rows=0)
    assert engines == [(tr.engine, 4)]
    logs = []
    losses = tr.train(1, log=logs.append)
    assert len(logs) == 1 and re.search(r"games=4 transitions=\d+", logs[0]), logs
    assert all(np.isfinite(v) for v in losses)
    tr.close()
