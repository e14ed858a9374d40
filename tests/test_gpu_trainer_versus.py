"""GPU test (run with -m gpu) of the trainer mirror's periodic games against the naive player (src/trainer.rs:380-394, 487-603)."""
import re

import pytest

from omok_ai_amd import api
from omok_ai_amd import trainer as TR

pytestmark = pytest.mark.gpu


def test_trainer_plays_the_naive_player_every_evaluate_every_iterations(tmp_path, monkeypatch):
    engines = []
    init = api.Engine.__init__

    def recording_init(self, *a, **kw):
        init(self, *a, **kw)
        engines.append((self, kw.get("games")))

    monkeypatch.setattr(api.Engine, "__init__", recording_init)
    p = TR.Parameters(model_name="tiny", episode_count=4, evaluate_count=16, evaluate_batch_size=8, parameter_update_count=2,
                      parameter_update_batch_size=8, replay_memory_size=500, evaluate_every=1, evaluate_games=6, test_evaluate_count=16)
    tr = TR.Trainer(p, board_size=9, seed=3, save_dir=str(tmp_path / "saves"), precision_rows=0)
    logs = []
    tr.train(1, log=logs.append)
    assert len(logs) == 1 and "net = White" in logs[0] and "naive = Black" in logs[0], logs
    m = re.search(r"black_win=(\d+) white_win=(\d+) draw=(\d+)", logs[0])
    assert m, logs[0]
    counts = [int(x) for x in m.groups()]
    assert sum(counts) == 6
    ev = tr.last_evaluation
    assert [ev["black_win"], ev["white_win"], ev["draw"]] == counts and ev["games"] == 6 and ev["iteration"] == 1
    own = [e for e, games in engines if games == 6]
    assert len(own) == 1 and own[0] is not tr.engine and own[0].h is None  # the evaluation ran on an engine of its own, closed again
    assert tr.engine.h is not None
    # `iteration % evaluate_every == 0` with the reference's 0-based index (:380): iteration index 1 of 10 plays no games
    tr.p.evaluate_every = 10
    n_engines = len(engines)
    tr.train(1, log=logs.append)
    assert len(logs) == 2 and "naive" not in logs[1] and "black_win" not in logs[1]
    assert len(engines) == n_engines and tr.last_evaluation["iteration"] == 1
    tr.close()
