"""GPU tests (run with -m gpu) of the data-parallel native training step: omok_train_gradient_count / omok_train_backward /
omok_train_apply through the C ABI, dist.gather_gradients and Trainer(train_backend="hip_dp").

Three yardsticks.  (1) omok_train_step itself: the two halves with the engine's own gradient must leave its bits.  (2) tests/train_reduce.py,
the numpy fp32 restatement of the rank-ordered average, bit for bit.  (3) float64 autograd and the float64 TrainPhase chain of the FULL
batch (the mean over equal shares of the shares' mean-loss gradients is the gradient of the mean loss over the union), under the rule of
tests/test_gpu_train_native.py: err <= 4 * err_t32 + 2^-20 per tensor, err_t32 = torch's own fp32 autograd of the full batch on the GPU,
measured in the same test.  Inputs, packing and the rule's code are that file's.  The figures are printed before the assertion (run with
-s; recorded in profiles/r14_train_dp_precision.txt)."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import omok_ai_amd as oa
from omok_ai_amd import binding as B
from omok_ai_amd import train as T
import test_gpu_train_native as TN
import train_reduce as TR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = TN.DEV


def _slab_buffer(eng, ranks=None):
    shape = (eng.train_gradient_count(),) if ranks is None else (ranks, eng.train_gradient_count())
    t = torch.zeros(shape, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()  # (the engine writes and reads it on a stream of its own)
    return t


def _gradients(eng):
    return [eng.train_gradient(i) for i in range(31)]


# ---- 1. the two halves are the step ---------------------------------------------------------------------------------------------
def test_backward_and_apply_leave_what_the_step_leaves():
    n, b = 9, 37
    _, _, _, records = TN._data(n, b, 1)
    tensors = TN._weights(n, "kink")
    dev = TN._upload(records)
    eng, twin = TN._engine(n, tensors, b), TN._engine(n, tensors, b)
    sizes = [int(B.lib().omok_net_tensor_size(eng.h, i)) for i in range(31)]
    assert eng.train_gradient_count() == sum(sizes) == sum(int(np.prod(s)) for s in oa.weights.tensor_shapes(n))
    slab = _slab_buffer(eng)
    idx = np.arange(b)
    # the first half alone writes no weight and leaves the losses where they were
    before = eng.train_losses(dev.data_ptr(), b, idx)
    eng.train_backward(dev.data_ptr(), b, idx, slab.data_ptr())
    assert TN._same_bits(eng.read_weights(), tensors)
    assert eng.train_losses(dev.data_ptr(), b, idx) == before
    assert slab.cpu().numpy().any()
    for _ in range(3):
        eng.train_backward(dev.data_ptr(), b, idx, slab.data_ptr())
        g_half = _gradients(eng)
        assert np.array_equal(slab.cpu().numpy().view(np.uint32), np.concatenate(g_half).view(np.uint32))  # the exchange layout: 31 tensors back to back
        got = eng.train_apply(None, 1)
        want = twin.train_step(dev.data_ptr(), b, idx)
        assert got == want
        assert TN._same_bits(eng.read_weights(), twin.read_weights())  # (and, from the second round on, the accumulators behind them)
        assert TN._same_bits(_gradients(eng), _gradients(twin)) and TN._same_bits(g_half, _gradients(twin))
    assert not TN._same_bits(eng.read_weights(), tensors)
    eng.close()
    twin.close()


# ---- 2. the rank-ordered sum ----------------------------------------------------------------------------------------------------
def test_apply_averages_the_slabs_in_rank_order():
    n, b, ranks = 9, 5, 8
    _, _, _, records = TN._data(n, b * ranks, 3)
    tensors = TN._weights(n, "kink")
    dev = TN._upload(records)
    src, one, two = (TN._engine(n, tensors, b) for _ in range(3))
    slabs = _slab_buffer(src, ranks)
    count = src.train_gradient_count()
    for r in range(ranks):  # real gradients of eight different batches
        src.train_backward(dev.data_ptr(), b * ranks, np.arange(b * r, b * r + b), slabs[r].data_ptr())
    host = slabs.cpu().numpy()
    assert all(host[r].any() for r in range(ranks)) and not np.array_equal(host[0], host[7])
    for R in (1, 2, 3, 8):
        # the engines' own pending gradients differ (batch 0 / batch 7, and their weights move from round to round): only the slabs count
        one.train_backward(dev.data_ptr(), b * ranks, np.arange(0, b))
        two.train_backward(dev.data_ptr(), b * ranks, np.arange(b * 7, b * 7 + b))
        l1 = one.train_apply(slabs.data_ptr(), R)
        l2 = two.train_apply(slabs.data_ptr(), R)
        want = TR.average(host[:R])
        for eng in (one, two):
            got = np.concatenate(_gradients(eng))
            diff = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
            assert diff.size == 0, (R, diff[:8], got[diff[:8]], want[diff[:8]])
        assert TN._same_bits(one.read_weights(), two.read_weights()), R
        assert np.isfinite(l1).all() and np.isfinite(l2).all()
    # hand-made slabs where the order, the inexact scale and the subnormal range show (three ranks)
    synth = host[:3].copy()
    synth[:, :6] = np.array([[1e8, 1e8, 1.0, 1e-45, 3e-39, -0.0],
                             [1.0, -1e8, 1e8, 1e-45, -1e-39, -0.0],
                             [-1e8, 1.0, -1e8, 2e-45, 1e-41, -0.0]], np.float32)
    synth[:, count - 1] = np.array([0.1, 0.7, 0.25], np.float32)  # the last element of the last tensor
    slabs[:3].copy_(torch.from_numpy(synth))
    torch.cuda.synchronize()
    one.train_backward(dev.data_ptr(), b * ranks, np.arange(0, b))
    one.train_apply(slabs.data_ptr(), 3)
    got, want = np.concatenate(_gradients(one)), TR.average(synth)
    assert want[0] == 0.0 and want[1] != 0.0  # (the order shows in the yardstick itself)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got[:6], want[:6], got[-1], want[-1])
    for e in (src, one, two):
        e.close()


# ---- 3. against the float64 yardstick -------------------------------------------------------------------------------------------
def _two_rank_step(a, b_eng, dev, n_records, halves, exchange):
    """one data-parallel step of two engines in this process: each takes the gradient of its half into its row of `exchange`"""
    a.train_backward(dev.data_ptr(), n_records, halves[0], exchange[0].data_ptr())
    b_eng.train_backward(dev.data_ptr(), n_records, halves[1], exchange[1].data_ptr())
    return a.train_apply(exchange.data_ptr(), 2), b_eng.train_apply(exchange.data_ptr(), 2)


@pytest.mark.parametrize("kind", ["scaled", "kink"])
@pytest.mark.parametrize("n,half", [(9, 18), (15, 2)])
def test_averaged_gradient_against_float64_autograd_of_the_full_batch(n, half, kind):
    b = 2 * half
    x, pi, z, records = TN._data(n, b, 1)
    tensors = TN._weights(n, kind)
    ref = TN._grads64(n, b, kind)
    t32 = T.Network(n, tensors, DEV)
    t32.losses(*(torch.as_tensor(a, device=DEV) for a in (x, pi, z)))[2].backward()
    g32 = [p.grad.cpu().numpy() for p in t32.vars]
    ea, eb = TN._engine(n, tensors, half), TN._engine(n, tensors, half)
    dev = TN._upload(records)
    exchange = _slab_buffer(ea, 2)
    _two_rank_step(ea, eb, dev, b, (np.arange(half), np.arange(half, b)), exchange)
    ga, gb = _gradients(ea), _gradients(eb)
    assert TN._same_bits(ga, gb)
    ea.close()
    eb.close()
    TN._hold(f"dp gradient N={n} halves=2x{half} weights={kind}", oa.weights.tensor_names(), ga, g32, ref)


def _figures(label, names, hip, t32, ref):
    """both figures of every tensor, printed only (the record of a case the rule is not run on)"""
    for i, name in enumerate(names):
        e_hip, e_t32 = TN._err(hip[i], ref[i]), TN._err(t32[i], ref[i])
        print(f"FIGURES {label} tensor {i:2d} {name:34s} err_hip {e_hip:.3e} err_t32 {e_t32:.3e}")


@pytest.mark.parametrize("kind", ["scaled", "kink"])
def test_data_parallel_steps_against_the_float64_chain(kind):
    """After 1 and 3 two-rank steps: the replicas are bit-equal (both kinds), and the updates are held to the 4x rule against the float64
    TrainPhase chain of the full batch with "scaled" weights, the scheme of tests/test_gpu_train_native.py's test_steps_against_the_float64_chain.
    With "kink" weights the updates' figures are printed for profiles/r14_train_dp_precision.txt and the rule is not run: the biases start at
    zero, Adadelta's first step maps every |g| >> 4.5e-4 to the same +-4.47e-06 and passes smaller |g| through linearly, so the rounding error
    of one small gradient element is magnified up to 2800-fold on the update scale, for the engine and for torch's fp32 autograd alike, and
    torch's figure (the bar) changes from run to run with the order of its sums.  What "kink" is there to catch -- a wrong slope at exactly
    0 -- is held by the gradient test above, which runs the rule on both kinds."""
    n, half = 9, 18
    b = 2 * half
    x, pi, z, records = TN._data(n, b, 1)
    tensors = TN._weights(n, kind)
    var0 = [np.asarray(t, np.float64).ravel() for t in tensors]
    cpu = T.TrainPhase(n, tensors, "cpu", dtype=torch.float64, allow_cpu=True)
    gpu = T.TrainPhase(n, tensors, DEV)
    ea, eb = TN._engine(n, tensors, half), TN._engine(n, tensors, half)
    dev = TN._upload(records)
    exchange = _slab_buffer(ea, 2)
    halves = (np.arange(half), np.arange(half, b))
    x64, x32 = [torch.as_tensor(a, dtype=torch.float64) for a in (x, pi, z)], [torch.as_tensor(a, device=DEV) for a in (x, pi, z)]
    for step in (1, 2, 3):
        cpu.step(*x64)
        gpu.step(*x32)
        la, lb = _two_rank_step(ea, eb, dev, b, halves, exchange)
        assert np.isfinite(la).all() and np.isfinite(lb).all()  # (each engine's losses are those of its own half)
        if step == 2:
            continue
        wa, wb = ea.read_weights(), eb.read_weights()
        assert TN._same_bits(wa, wb), step  # the replicas stay bit-equal
        assert not TN._same_bits(wa, tensors)
        assert TN._same_bits(_gradients(ea), _gradients(eb))
        u64 = [p.detach().numpy().ravel() - v0 for p, v0 in zip(cpu.net.vars, var0)]
        u32 = [p.detach().cpu().numpy().ravel().astype(np.float64) - v0 for p, v0 in zip(gpu.net.vars, var0)]
        uhip = [t.astype(np.float64) - v0 for t, v0 in zip(wa, var0)]
        label = f"dp update after {step} step(s) N={n} halves=2x{half} weights={kind}"
        if kind == "scaled":
            TN._hold(label, oa.weights.tensor_names(), uhip, u32, u64)
        else:
            _figures(label, oa.weights.tensor_names(), uhip, u32, u64)
    ea.close()
    eb.close()


# ---- 4. rejections --------------------------------------------------------------------------------------------------------------
def test_rejected_calls_change_nothing():
    n, b = 9, 5
    _, _, _, records = TN._data(n, b, 1)
    tensors = TN._weights(n, "scaled")
    dev = TN._upload(records)
    eng, twin = TN._engine(n, tensors), TN._engine(n, tensors, b)
    L = B.lib()
    losses = np.zeros(3, np.float32)
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731
    ptr = C.c_void_p(dev.data_ptr())
    good = np.arange(b, dtype=np.int64)
    slabs = _slab_buffer(eng, 2)
    sp = C.c_void_p(slabs.data_ptr())
    # before omok_train_begin
    assert L.omok_train_apply(eng.h, None, 1, B.fptr(losses)) == -3
    assert L.omok_train_backward(eng.h, ptr, b, i64(good), b, None) == -3
    assert eng.train_gradient_count() == slabs.shape[1]  # (needs no training state)
    eng.train_begin(b)
    assert L.omok_train_apply(eng.h, None, 1, B.fptr(losses)) == -3        # no backward yet
    eng.train_step(dev.data_ptr(), b, good)
    twin.train_step(dev.data_ptr(), b, good)
    assert L.omok_train_apply(eng.h, None, 1, B.fptr(losses)) == -3        # a whole step is no pending backward
    for between in (eng.train_step, eng.train_losses):                     # ... and either of them in between takes the mark away
        eng.train_backward(dev.data_ptr(), b, good)
        between(dev.data_ptr(), b, good)
        if between == eng.train_step:
            twin.train_step(dev.data_ptr(), b, good)
        assert L.omok_train_apply(eng.h, None, 1, B.fptr(losses)) == -3
        assert L.omok_train_apply(eng.h, sp, 2, B.fptr(losses)) == -3
    eng.commit()
    before = eng.read_weights()
    eng.train_backward(dev.data_ptr(), b, good, slabs[0].data_ptr())
    slabs[1].copy_(slabs[0])
    torch.cuda.synchronize()
    assert L.omok_train_apply(eng.h, sp, 0, B.fptr(losses)) == -1
    assert L.omok_train_apply(eng.h, sp, 65, B.fptr(losses)) == -1
    assert L.omok_train_apply(eng.h, None, 2, B.fptr(losses)) == -1
    assert L.omok_train_backward(eng.h, ptr, b, i64(good), 0, None) == -1      # batch < 1
    assert L.omok_train_backward(eng.h, ptr, b, i64(np.zeros(b + 1, np.int64)), b + 1, None) == -1  # batch > max_batch
    for bad in (-1, b):                                                        # an index outside [0, n_records)
        idx = good.copy()
        idx[b - 1] = bad
        assert L.omok_train_backward(eng.h, ptr, b, i64(idx), b, None) == -1
    assert TN._same_bits(before, eng.read_weights())
    eng.evaluate_pv(TN._data(n, b, 1)[0].reshape(b, -1))  # still committed
    # none of them took the pending mark or touched the optimizer: the step completes as the twin's whole step does
    got = eng.train_apply(slabs.data_ptr(), 2)  # (two equal slabs: (g + g) * 0.5 = g)
    want = twin.train_step(dev.data_ptr(), b, good)
    assert got == want and TN._same_bits(eng.read_weights(), twin.read_weights())
    assert eng.train_step(dev.data_ptr(), b, good) == twin.train_step(dev.data_ptr(), b, good)
    assert TN._same_bits(eng.read_weights(), twin.read_weights())
    eng.close()
    twin.close()


# ---- 5. the trainer on one rank -------------------------------------------------------------------------------------------------
def test_trainer_data_parallel_backend_equals_the_native_backend_at_world_one(tmp_path):
    from omok_ai_amd import trainer as TRN
    out = {}
    for backend in ("hip", "hip_dp"):
        p = TRN.Parameters(model_name="tiny", train_backend=backend, episode_count=8, evaluate_count=16, evaluate_batch_size=8,
                           parameter_update_count=5, parameter_update_batch_size=32, evaluate_every=0)
        tr = TRN.Trainer(p, board_size=9, seed=3, save_dir=str(tmp_path / backend), precision_rows=0)
        w0 = tr.engine.read_weights()
        logs = []
        losses = tr.train(2, log=logs.append)
        assert len(logs) == 2
        out[backend] = (losses, tr.engine.read_weights(), tr.phase.net.tensors())
        assert not TN._same_bits(w0, out[backend][1])
        tr.engine.evaluate_pv(np.zeros((1, 3 * 81), np.float32))  # committed after the loop
        tr.close()
    assert out["hip"][0] == out["hip_dp"][0] and np.isfinite(out["hip_dp"][0]).all()
    assert TN._same_bits(out["hip"][1], out["hip_dp"][1])
    assert TN._same_bits(out["hip_dp"][1], out["hip_dp"][2])  # the torch mirror holds the engine's bits


# ---- 6. two ranks on the one GPU ------------------------------------------------------------------------------------------------
def test_two_ranks_train_to_the_same_bits(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # (as tests/test_gpu_rehearsal.py)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "train_dp_worker.py"), str(tmp_path)]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    from oracle import model_io as M
    got = [np.load(str(tmp_path / f"rank{r}.npz")) for r in range(2)]
    w = [[g[f"w{i}"] for i in range(31)] for g in got]
    assert [int(g["world"]) for g in got] == [2, 2] and [int(g["rank"]) for g in got] == [0, 1]
    assert TN._same_bits(w[0], w[1])
    assert not TN._same_bits(w[0], [got[0][f"i{i}"] for i in range(31)])  # the variables moved
    assert got[0]["records"] > 0 and got[1]["records"] > 0
    _, saved = M.model_load(str(tmp_path / "saves" / "tiny"))
    assert len(saved) == 31 and TN._same_bits(w[0], saved)
    for g in got:
        assert np.isfinite(g["losses"]).all() and g["losses"].shape == (3,)
