"""tests/head_bias_nets.py without a GPU: the closed-form outputs in float64 and float32 numpy, the oracle's own net on such tensors,
and the oracle-only episodes the GPU run loop is compared with (tests/test_gpu_head_bias_nets.py): the two oracles agree on them and
they reach the branches they are there for (coverage floors)."""
import functools

import numpy as np
import pytest

import adversarial_outputs as AO
import head_bias_nets as H
from helpers import random_positions
from oracle import oracle as O


@pytest.mark.parametrize("n", [9, 15])
def test_expected_rows(n):
    hw = n * n
    for dtype in (np.float64, np.float32):
        p, v = H.expected(n, "flat", dtype)
        assert p.dtype == np.float32 and np.all(p == np.float32(1.0) / np.float32(hw)) and v.tobytes() == np.float32(0.0).tobytes()
        for kind, want in (("sparse", 1.0), ("sparse_neg", -1.0)):
            p, v = H.expected(n, kind, dtype)
            cells = H.sparse_cells(n)
            assert np.all(p[cells] == np.float32(1.0) / np.float32(6.0)) and p.sum() == p[cells].sum() and (p == 0).sum() == hw - 6
            assert v == np.float32(want)
    a, b = H.expected(n, "sparse", np.float64), H.expected(n, "sparse", np.float32)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert float(np.exp(np.float32(-200.0))) == 0.0 and np.float32(np.exp(-200.0)) == 0.0 and np.tanh(20.0) == 1.0


@pytest.mark.parametrize("kind", H.KINDS)
def test_oracle_net_emits_the_expected_rows(kind):
    """the fp32 restatement of the net (oracle/net.c) on these tensors: 0 * h + b is exact, so its logits are the biases bit for bit and
    p, v the closed forms"""
    n = 9
    x = random_positions(n, 16, 3)
    p, v, lg, vp = O.Net(n, H.make(n, kind)).forward_logits(x, threads=2)
    L, b = H.head_biases(n, kind)
    assert np.array_equal(lg.view(np.uint32), np.tile(L, (16, 1)).view(np.uint32)) and np.all(vp == b)
    ep, ev = H.expected_rows(n, kind, 16)
    assert np.array_equal(p.view(np.uint32), ep.view(np.uint32)) and np.array_equal(v.view(np.uint32), ev.view(np.uint32))


@functools.lru_cache(maxsize=None)
def episode_counts(index, literal):
    kind, n, games, count, k, plies, _, seed = H.RUN_CASES[index]
    total = {}

    def collect(dumps):
        total.update(AO.add_counts(total, AO.coverage(dumps)))
    H.oracle_episode(n, kind, games, count, k, plies, seed, H.GAME_OFFSET, threshold=H.THRESHOLD, literal=literal, collect=collect)
    return total


@pytest.mark.parametrize("index", range(len(H.RUN_CASES)), ids=[f"{c[0]}_n{c[1]}" for c in H.RUN_CASES])
def test_oracle_episodes_agree_and_meet_the_floors(index):
    kind, n, _, count, _, plies, _, _ = H.RUN_CASES[index]
    counts = episode_counts(index, True)
    print(f"{kind} n={n}: coverage {counts}")
    for key in H.floor_keys(kind, n, count, plies):
        assert counts[key] >= AO.FLOOR, f"{kind} n={n}: {key} = {counts[key]}"
