"""CPU tests of the data-parallel native training step's host side: the numpy restatement of the rank-ordered average
(tests/train_reduce.py, the yardstick of tests/test_gpu_train_dp.py) on values where the order and the inexact scale show, and
dist.gather_gradients on two gloo ranks (rows in rank order) and at world size 1 (no collective)."""
import itertools
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import train_reduce as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT = 1031  # floats per slab in the gather test (odd: no multiple of anything)


def test_average_adds_in_rank_order():
    slabs = {p: TR.average([np.array([v], np.float32) for v in p]) for p in itertools.permutations([1e8, 1.0, -1e8])}
    third = np.float32(1) / np.float32(3)
    # fp32 has 24 bits: 1e8 + 1 == 1e8, so the 1 survives only where the two large values meet first
    assert slabs[(1e8, -1e8, 1.0)][0] == slabs[(-1e8, 1e8, 1.0)][0] == np.float32(1) * third
    for p in ((1e8, 1.0, -1e8), (-1e8, 1.0, 1e8), (1.0, 1e8, -1e8), (1.0, -1e8, 1e8)):
        assert slabs[p][0] == 0.0, p
    assert slabs[(1e8, 1.0, -1e8)].dtype == np.float32


def test_average_scales_by_the_fp32_reciprocal():
    third = np.float32(1) / np.float32(3)
    assert third.dtype == np.float32 and float(third) != 1.0 / 3.0
    a, b, c = (np.array([v], np.float32) for v in (0.1, 0.7, 0.25))
    got = TR.average([a, b, c])
    assert got.dtype == np.float32 and got[0] == (a[0] + b[0] + c[0]) * third
    # ... which is not the division: 5 / 3 rounds to another float than 5 * fl(1 / 3)
    five = TR.average([np.array([v], np.float32) for v in (1.0, 2.0, 2.0)])[0]
    assert five == np.float32(5) * third and five != np.float32(5) / np.float32(3)
    # one rank: the slab itself, bit for bit (x * 1.0f), subnormals and signed zeros included
    x = np.array([1e-45, -1e-40, -0.0, 3.0e38, 1.1754944e-38], np.float32)
    assert np.array_equal(TR.average([x]).view(np.uint32), x.view(np.uint32))
    # two ranks: halving a subnormal sum rounds to even in fp32
    ulp = np.array([1, 2], np.uint32).view(np.float32)  # 1 and 2 units of 2^-149
    assert TR.average([ulp[:1], ulp[1:]]).view(np.uint32)[0] == 2  # (1 + 2) / 2 = 1.5 units -> 2


def _slab(rank):
    return (np.arange(COUNT, dtype=np.float32) + np.float32(1000 * (rank + 1))) * np.float32(0.5 - rank)


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import omok_ai_amd as oa
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    mine = torch.from_numpy(_slab(rank))
    got = oa.dist.gather_gradients(mine)
    assert got.shape == (world, COUNT) and got.dtype == torch.float32 and got.device == mine.device
    np.save(f"{out}.rank{rank}.npy", got.numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_gather_gradients_returns_rows_in_rank_order(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "slabs")
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    want = np.stack([_slab(0), _slab(1)])
    for r in range(2):  # every rank holds both slabs, rank 0's first
        assert np.array_equal(np.load(f"{out}.rank{r}.npy").view(np.uint32), want.view(np.uint32)), r


def test_gather_gradients_at_world_one_runs_no_collective(monkeypatch):
    sys.path.insert(0, ROOT)
    import omok_ai_amd as oa

    def refuse(*a, **k):
        raise AssertionError("a collective at world size 1")

    monkeypatch.setattr(dist, "all_gather_into_tensor", refuse)
    monkeypatch.setattr(dist, "all_gather", refuse)
    mine = torch.from_numpy(_slab(0))
    got = oa.dist.gather_gradients(mine)
    assert got.shape == (1, COUNT) and got.data_ptr() == mine.data_ptr()  # mine[None]: a view, nothing moved
