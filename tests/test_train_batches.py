"""No-GPU pins of tests/train_batches.py, the restatement of the training step's batch draw (src/trainer.rs:329-350 choose_multiple
under the RNG contract of DESIGN 5, purpose TRAIN_BATCH) that tests/test_gpu_train_native.py compares omok_train_batch_indices with."""
import pytest

import train_batches as TB

KEY = 0x0123456789ABCDEF


def _philox_word0(key, c0, c1, c2, c3):
    """Philox4x32-10 by hand (Salmon et al. 2011): word 0 of the output block"""
    m = 0xFFFFFFFF
    k0, k1 = key & m, key >> 32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & m, p1 & m, ((p0 >> 32) ^ c3 ^ k1) & m, p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & m, (k1 + 0xBB67AE85) & m
    return c0


@pytest.mark.parametrize("batch", [128, 5])
@pytest.mark.parametrize("which", ["one", "batch", "batch+1", "large"])
def test_draw_is_a_sample_without_replacement(batch, which):
    n_records = {"one": 1, "batch": batch, "batch+1": batch + 1, "large": 1_000_003}[which]
    for step in (0, 1, 599):
        got = TB.draw(n_records, batch, KEY, step)
        assert len(got) == min(batch, n_records)
        assert len(set(got)) == len(got)
        assert all(0 <= v < n_records for v in got)
    if n_records == batch:  # every record, each once
        assert sorted(TB.draw(n_records, batch, KEY, 3)) == list(range(n_records))
    if n_records > 1:
        assert TB.draw(n_records, batch, KEY, 0) != TB.draw(n_records, batch, KEY, 1)       # the step keys the draw
        assert TB.draw(n_records, batch, KEY, 0) != TB.draw(n_records, batch, KEY + 1, 0)   # ... and so does the key


def test_first_draws_of_a_fixed_key_and_step():
    # ranks among the records not yet drawn, from the hand-written Philox: r_i = mulhi(x0_i, R - i)
    r = [(_philox_word0(KEY, i, 7, 0, TB.RNG_TRAIN_BATCH) * (1_000_003 - i)) >> 32 for i in range(8)]
    assert r == [568771, 303141, 522500, 238724, 718590, 298668, 602347, 218755]
    # ... and the records they name: 522500 -> 522501 (303141 was drawn below it), 718590 -> 718594 (four below it), ...
    assert TB.draw(1_000_003, 8, KEY, 7) == [568771, 303141, 522501, 238724, 718594, 298669, 602352, 218755]
    assert TB.draw(1_000_003, 128, KEY, 7)[:8] == TB.draw(1_000_003, 8, KEY, 7)             # a prefix does not depend on the batch size
    assert TB.draw(10, 10, KEY, 7) == [5, 2, 6, 1, 8, 3, 7, 0, 4, 9]
    assert TB.draw(6, 5, 42, 0) == [1, 5, 0, 2, 3]


def test_draw_agrees_with_the_definition_by_enumeration():
    """the r-th record not yet drawn, found by listing the records that are left (small R only)"""
    for n_records, batch, step in ((17, 17, 0), (40, 13, 5), (129, 128, 2)):
        left = list(range(n_records))
        want = []
        for i in range(min(batch, n_records)):
            r = (_philox_word0(KEY, i, step, 0, TB.RNG_TRAIN_BATCH) * (n_records - i)) >> 32
            want.append(left.pop(r))
        assert TB.draw(n_records, batch, KEY, step) == want
