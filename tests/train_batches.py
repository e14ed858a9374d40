"""The batch draw of the native training step, restated through the oracle library's Philox (a helper of
tests/test_train_batches.py and tests/test_gpu_train_native.py; not a test, no product code).

  choose_multiple (src/trainer.rs:329-350): uniform, without replacement; the reference is unseeded.  Under the build-defined RNG
  contract (purpose TRAIN_BATCH = 5) step `step` of a run with key `key` draws k = min(batch, R) indices: index i is the
  mulhi(x0, R - i)-th record, 0-based and ascending, that is not among the first i drawn, x0 = word 0 of
  Philox4x32-10(key; c0 = i, c1 = step, c2 = 0, c3 = 5).
"""
import bisect
import ctypes as C

from oracle import oracle as O

RNG_TRAIN_BATCH = 5


def draw(n_records, batch, key, step):
    """the k record indices in draw order (python ints)"""
    k = min(int(batch), int(n_records))
    out = (C.c_uint32 * 4)()
    chosen, order = [], []  # chosen: ascending
    for i in range(k):
        O.lib().orc_philox(int(key) & 0xFFFFFFFFFFFFFFFF, i, int(step), 0, RNG_TRAIN_BATCH, out)
        r = (int(out[0]) * (int(n_records) - i)) >> 32
        v = r  # the r-th record not yet chosen: walk the chosen ones in ascending order, every one at or below the candidate moves it up
        for c in chosen:
            if c <= v:
                v += 1
            else:
                break
        bisect.insort(chosen, v)
        order.append(v)
    return order
