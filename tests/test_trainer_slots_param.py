"""No-GPU checks of Parameters.selfplay_slots: off by default, and a negative count is refused before any engine is asked for."""
import pytest

from omok_ai_amd import api
from omok_ai_amd import trainer as TR


def test_selfplay_slots_defaults_to_the_episode_path():
    assert TR.Parameters().selfplay_slots == 0


def test_a_negative_slot_count_is_refused_before_an_engine_is_created(tmp_path, monkeypatch):
    def no_engine(self, *a, **kw):
        raise AssertionError("an engine was created")

    monkeypatch.setattr(api.Engine, "__init__", no_engine)
    with pytest.raises(ValueError, match="selfplay_slots"):
        TR.Trainer(TR.Parameters(selfplay_slots=-1), board_size=9, save_dir=str(tmp_path))
