"""GPU tests (run with -m gpu) of the native training step: omok_train_* / omok_net_read / omok_debug_train_gradient through the C ABI.

The yardstick is the torch graph of omok_ai_amd.train in float64 on the CPU, which tests/test_train.py ties to oracle/train.py (forward,
losses, central-difference gradients, adadelta_apply).  Inputs are built as tests/test_train.py builds them, packed into replay records on
the host and uploaded through a torch uint8 tensor.

Precision rule (gradients and updates, per tensor): err = max|g - g64| / max|g64|; the native step's err_hip is held against torch's own fp32
autograd on the GPU, err_t32, measured in the same test: err_hip <= 4 * err_t32 + 2^-20.  Both are fp32 sums in different orders over up to
batch * HW terms; the factor 4 covers what a change of summation order moves (a missing term, a wrong slope or a transposed tap shows as
>= 1e-2), the floor 2^-20 is 16 roundings of the largest element and covers tensors where torch happens to be exact.  The figures are
printed before the assertion (run with -s; recorded in profiles/r13_train_native_precision.txt)."""
import functools
import os

import numpy as np
import pytest
import torch

import omok_ai_amd as oa
from omok_ai_amd import binding as B
from omok_ai_amd import train as T
from oracle import oracle as O
import train_batches as TB

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -20
DEV = "cuda:0"


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _batch(n, b, seed):  # tests/test_train.py: _batch
    rng = np.random.default_rng(seed)
    hw = n * n
    x = np.zeros((b, 3 * hw), np.float32)
    for i in range(b):
        env = O.Environment(n)
        for c in rng.permutation(hw)[: int(rng.integers(0, hw - 1))]:
            env.place_stone(int(c))
        x[i] = env.encode_nn_input(0)
    pi = rng.random((b, hw))
    pi = (pi / pi.sum(axis=1, keepdims=True)).astype(np.float32)
    z = rng.choice([-1.0, 0.0, 1.0], size=(b, 1)).astype(np.float32)
    return x.reshape(b, n, n, 3), pi, z


def _pack(n, x, pi, z):
    """replay records (board u8[HW], turn u8, pad to 4, pi f32[HW], z f32) whose decoding is (x, pi, z)"""
    hw = n * n
    brd = (hw + 1 + 3) // 4 * 4
    rec = brd + 4 * hw + 4
    b = x.shape[0]
    flat = x.reshape(b, 3 * hw)
    r = np.zeros((b, rec), np.uint8)
    for i in range(b):
        turn = 0 if flat[i, 2 * hw] == 1.0 else 1  # third plane: 1 where Black is to move
        mine, theirs = flat[i, 0:2 * hw:2], flat[i, 1:2 * hw:2]
        r[i, :hw] = (mine * (turn + 1) + theirs * (2 - turn)).astype(np.uint8)  # Stone::Black = 1, Stone::White = 2
        r[i, hw] = turn
        r[i, brd:brd + 4 * hw] = pi[i].view(np.uint8)
        r[i, brd + 4 * hw:] = z[i].view(np.uint8)
    dx, dpi, dz = T.decode_records(torch.from_numpy(r), n)  # the packing is this file's own code: checked against the product's decoder
    assert np.array_equal(dx.numpy(), x) and np.array_equal(dpi.numpy(), pi) and np.array_equal(dz.numpy(), z)
    return r


@functools.lru_cache(maxsize=None)
def _data(n, b, seed):
    x, pi, z = _batch(n, b, seed)
    return x, pi, z, _pack(n, x, pi, z)


@functools.lru_cache(maxsize=None)
def _weights(n, kind):
    """"scaled": init_random x 0.25 with random biases, off the LeakyReLU kink as in tests/test_train.py; "kink": plain init_random, whose
    zero biases put empty cells exactly on it.  float32: every consumer starts from the same bits."""
    tensors = oa.weights.init_random(n, seed=1)
    if kind == "scaled":
        brng = np.random.default_rng(9)
        tensors = [(np.asarray(t, np.float64) * 0.25 + (0.1 * brng.standard_normal(t.shape) if t.ndim == 1 else 0.0)).astype(np.float32) for t in tensors]
    else:
        assert kind == "kink" and all(not t.any() for t in tensors if t.ndim == 1)
    return tuple(tensors)


def _upload(records):
    dev = torch.from_numpy(records).to(DEV)
    torch.cuda.synchronize()
    return dev


def _engine(n, tensors, max_batch=None):
    eng = oa.Engine(board_size=n, games=2, max_nodes=64, max_tables=32, max_batch_k=8, seed=1)
    eng.load_weights(list(tensors))
    if max_batch:
        eng.train_begin(max_batch)
    return eng


def _bits(tensors):
    return [np.asarray(t, np.float32).ravel().view(np.uint32) for t in tensors]


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


def _err(got, want):
    want = np.asarray(want, np.float64).ravel()
    return float(np.abs(np.asarray(got, np.float64).ravel() - want).max() / max(np.abs(want).max(), 1e-300))


def _hold(label, names, hip, t32, ref):
    """the 4x rule on every tensor; prints both figures first"""
    bad = []
    for i, name in enumerate(names):
        e_hip, e_t32 = _err(hip[i], ref[i]), _err(t32[i], ref[i])
        print(f"PRECISION {label} tensor {i:2d} {name:34s} err_hip {e_hip:.3e} err_t32 {e_t32:.3e} bar {4 * e_t32 + FLOOR:.3e}")
        if not e_hip <= 4 * e_t32 + FLOOR:
            bad.append((i, name, e_hip, e_t32))
    assert not bad, (label, bad)


@functools.lru_cache(maxsize=None)
def _grads64(n, b, kind):
    x, pi, z, _ = _data(n, b, 1)
    net = T.Network(n, _weights(n, kind), "cpu", dtype=torch.float64, allow_cpu=True)
    net.losses(*(torch.as_tensor(a, dtype=torch.float64) for a in (x, pi, z)))[2].backward()
    return [p.grad.numpy().copy() for p in net.vars]


# ---- 1. the draw --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [128, 5])
def test_batch_indices_equal_the_restatement(batch):
    eng = _engine(9, _weights(9, "kink"), 128)
    key = 0x0123456789ABCDEF
    for n_records in (1, batch, batch + 1, 1_000_003):
        for step in (0, 7):
            got = eng.train_batch_indices(n_records, batch, key, step)
            assert got.dtype == np.int64 and got.tolist() == TB.draw(n_records, batch, key, step), (n_records, step)
    eng.close()


# ---- 2. gradients -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scaled", "kink"])
@pytest.mark.parametrize("n,b", [(9, 5), (9, 37), (15, 3)])
def test_gradients_against_float64_autograd(n, b, kind):
    x, pi, z, records = _data(n, b, 1)
    tensors = _weights(n, kind)
    ref = _grads64(n, b, kind)
    t32 = T.Network(n, tensors, DEV)
    t32.losses(*(torch.as_tensor(a, device=DEV) for a in (x, pi, z)))[2].backward()
    g32 = [p.grad.cpu().numpy() for p in t32.vars]
    eng = _engine(n, tensors, b)
    dev = _upload(records)
    eng.train_step(dev.data_ptr(), b, np.arange(b))
    ghip = [eng.train_gradient(i) for i in range(31)]
    eng.close()
    _hold(f"gradient N={n} batch={b} weights={kind}", oa.weights.tensor_names(), ghip, g32, ref)


# ---- 3. the step --------------------------------------------------------------------------------------------------------------
def test_steps_against_the_float64_chain():
    n, b = 9, 37
    x, pi, z, records = _data(n, b, 1)
    tensors = _weights(n, "scaled")
    var0 = [np.asarray(t, np.float64).ravel() for t in tensors]
    cpu = T.TrainPhase(n, tensors, "cpu", dtype=torch.float64, allow_cpu=True)
    gpu = T.TrainPhase(n, tensors, DEV)
    eng = _engine(n, tensors, b)
    dev = _upload(records)
    x64, x32 = [torch.as_tensor(a, dtype=torch.float64) for a in (x, pi, z)], [torch.as_tensor(a, device=DEV) for a in (x, pi, z)]
    for step in (1, 2, 3):
        pl, vl, ls = cpu.step(*x64)  # TrainPhase.step returns (p_loss, v_loss, loss)
        gpu.step(*x32)
        hv, hp, hl = eng.train_step(dev.data_ptr(), b, np.arange(b))  # (v_loss, p_loss, loss)
        if step == 2:
            continue
        print(f"STEP {step}: native v {hv:.6f} p {hp:.6f} loss {hl:.6f}   float64 v {vl:.6f} p {pl:.6f} loss {ls:.6f}")
        assert max(abs(hv - vl), abs(hp - pl), abs(hl - ls)) < 2e-3 * max(1.0, abs(ls))
        u64 = [p.detach().numpy().ravel() - v0 for p, v0 in zip(cpu.net.vars, var0)]
        u32 = [p.detach().cpu().numpy().ravel().astype(np.float64) - v0 for p, v0 in zip(gpu.net.vars, var0)]
        uhip = [t.astype(np.float64) - v0 for t, v0 in zip(eng.read_weights(), var0)]
        _hold(f"update after {step} step(s) N={n} batch={b}", oa.weights.tensor_names(), uhip, u32, u64)
    eng.close()


# ---- 4. losses only -----------------------------------------------------------------------------------------------------------
def test_train_losses_change_nothing_and_match_float64():
    n, b = 9, 37
    x, pi, z, records = _data(n, b, 1)
    tensors = _weights(n, "scaled")
    net = T.Network(n, tensors, "cpu", dtype=torch.float64, allow_cpu=True)
    with torch.no_grad():
        pl, vl, ls = (float(a) for a in net.losses(*(torch.as_tensor(a, dtype=torch.float64) for a in (x, pi, z))))
    eng, twin = _engine(n, tensors, b), _engine(n, tensors, b)
    dev = _upload(records)
    idx = np.arange(b)
    eng.train_step(dev.data_ptr(), b, idx)   # (accumulators that are no longer zero)
    twin.train_step(dev.data_ptr(), b, idx)
    before = eng.read_weights()
    again = eng.train_losses(dev.data_ptr(), b, idx)
    assert _same_bits(before, eng.read_weights())
    assert again == eng.train_losses(dev.data_ptr(), b, idx)
    eng.train_step(dev.data_ptr(), b, idx)   # the accumulators are not readable: an unchanged optimizer takes the same next step
    twin.train_step(dev.data_ptr(), b, idx)
    assert _same_bits(eng.read_weights(), twin.read_weights())
    fresh = _engine(n, tensors, b)
    hv, hp, hl = fresh.train_losses(dev.data_ptr(), b, idx)
    assert _same_bits(tensors, fresh.read_weights())
    assert max(abs(hv - vl), abs(hp - pl), abs(hl - ls)) < 2e-3 * max(1.0, abs(ls))
    for e in (eng, twin, fresh):
        e.close()


# ---- 5. same bits -------------------------------------------------------------------------------------------------------------
def test_two_engines_leave_the_same_bits():
    n, b = 9, 37
    _, _, _, records = _data(n, b, 1)
    dev = _upload(records)
    out = []
    for _ in range(2):
        eng = _engine(n, _weights(n, "kink"), b)
        losses = [eng.train_step(dev.data_ptr(), b, np.arange(b)) for _ in range(3)]
        out.append((losses, eng.read_weights(), [eng.train_gradient(i) for i in range(31)]))
        eng.close()
    assert out[0][0] == out[1][0] and _same_bits(out[0][1], out[1][1]) and _same_bits(out[0][2], out[1][2])
    assert not _same_bits(out[0][1], _weights(n, "kink"))


# ---- 6. the run ---------------------------------------------------------------------------------------------------------------
def test_run_equals_the_loop_of_draws_and_steps():
    n, r, count, batch, key = 9, 200, 12, 16, 0xC0FFEE
    x, _, _, records = _data(n, r, 2)
    tensors = _weights(n, "kink")
    dev = _upload(records)
    eng, twin = _engine(n, tensors, batch), _engine(n, tensors, batch)
    means = eng.train_run(dev.data_ptr(), r, count, batch, key)
    sums = np.zeros(3, np.float32)
    for s in range(count):
        idx = twin.train_batch_indices(r, batch, key, s)
        sums += np.asarray(twin.train_step(dev.data_ptr(), r, idx), np.float32)  # fp32, in step order, like the device
    assert _same_bits(eng.read_weights(), twin.read_weights())
    assert means == tuple(float(v) for v in sums / np.float32(count))
    # the run committed the net: the engine evaluates like the torch graph of the read-back weights (the project's 1e-3 contract)
    xe = x[:16].reshape(16, -1)
    pe, ve = eng.evaluate_pv(xe)
    net = T.Network(n, [t.reshape(s) for t, s in zip(eng.read_weights(), oa.weights.tensor_shapes(n))], DEV)
    with torch.no_grad():
        pt, vt = net(torch.as_tensor(x[:16], device=DEV))
    assert np.abs(pe.reshape(16, -1) - pt.cpu().numpy()).max() < 1e-3 and np.abs(ve.ravel() - vt.cpu().numpy().ravel()).max() < 1e-3
    with pytest.raises(B.OmokError):  # ... and the twin, stepped by hand, is not committed
        twin.evaluate_pv(xe)
    # a 30-step run lowers the loss on its own memory
    first = eng.train_losses(dev.data_ptr(), r, np.arange(16))[2]
    eng.train_run(dev.data_ptr(), r, 30, batch, key + 1)
    assert eng.train_losses(dev.data_ptr(), r, np.arange(16))[2] < first
    eng.close()
    twin.close()


# ---- 7. rejections ------------------------------------------------------------------------------------------------------------
def test_rejected_calls_change_nothing():
    import ctypes as C
    n, b = 9, 5
    _, _, _, records = _data(n, b, 1)
    tensors = _weights(n, "scaled")
    dev = _upload(records)
    eng, twin = _engine(n, tensors), _engine(n, tensors, b)
    L = B.lib()
    losses = np.zeros(3, np.float32)
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731
    ptr = C.c_void_p(dev.data_ptr())
    good = np.arange(b, dtype=np.int64)
    out = np.zeros(b, np.int64)
    # before omok_train_begin
    assert L.omok_train_step(eng.h, ptr, b, i64(good), b, B.fptr(losses)) == -3
    assert L.omok_train_losses(eng.h, ptr, b, i64(good), b, B.fptr(losses)) == -3
    assert L.omok_train_batch_indices(eng.h, b, b, 1, 0, i64(out)) == -3
    assert L.omok_train_run(eng.h, ptr, b, 1, b, 1, B.fptr(losses)) == -3
    assert L.omok_debug_train_gradient(eng.h, 0, B.fptr(np.zeros(384, np.float32)), 384) == -3
    eng.train_begin(b)
    eng.train_step(dev.data_ptr(), b, good)
    twin.train_step(dev.data_ptr(), b, good)
    eng.commit()
    before = eng.read_weights()
    for fn in (L.omok_train_step, L.omok_train_losses):
        assert fn(eng.h, ptr, b, i64(good), 0, B.fptr(losses)) == -1          # batch < 1
        assert fn(eng.h, ptr, b, i64(np.zeros(b + 1, np.int64)), b + 1, B.fptr(losses)) == -1  # batch > max_batch
        for bad in (-1, b):                                                    # an index outside [0, n_records)
            idx = good.copy()
            idx[b - 1] = bad
            assert fn(eng.h, ptr, b, i64(idx), b, B.fptr(losses)) == -1
    assert L.omok_train_run(eng.h, ptr, b, 3, 0, 1, B.fptr(losses)) == -1
    assert L.omok_train_run(eng.h, ptr, b, 3, b + 1, 1, B.fptr(losses)) == -1
    assert L.omok_train_batch_indices(eng.h, b, 0, 1, 0, i64(out)) == -1
    assert L.omok_train_batch_indices(eng.h, b, b + 1, 1, 0, i64(out)) == -1
    assert _same_bits(before, eng.read_weights())
    x = _data(n, b, 1)[0].reshape(b, -1)
    eng.evaluate_pv(x)  # still committed
    eng.train_step(dev.data_ptr(), b, good)
    twin.train_step(dev.data_ptr(), b, good)
    assert _same_bits(eng.read_weights(), twin.read_weights())
    eng.close()
    twin.close()


# ---- 8. the trainer -----------------------------------------------------------------------------------------------------------
def test_trainer_with_the_native_backend_saves_and_resumes(tmp_path):
    from omok_ai_amd import trainer as TR
    from oracle import model_io as M
    p = TR.Parameters(model_name="tiny", train_backend="hip", episode_count=8, evaluate_count=16, evaluate_batch_size=8,
                      parameter_update_count=5, parameter_update_batch_size=32, evaluate_every=0)
    save_dir = str(tmp_path / "saves")
    tr = TR.Trainer(p, board_size=9, seed=3, save_dir=save_dir)
    w0 = tr.phase.net.tensors()
    logs = []
    v_loss, p_loss, loss = tr.train(2, log=logs.append)
    assert len(logs) == 2 and np.isfinite(loss) and abs(loss - (v_loss + p_loss)) < 1e-4 * max(1.0, abs(loss))
    w2 = tr.phase.net.tensors()
    assert any(not np.array_equal(a, b) for a, b in zip(w0, w2))          # the variables moved
    assert _same_bits(w2, tr.engine.read_weights())                       # ... and the torch mirror holds the engine's bits
    _, params = M.model_load(os.path.join(save_dir, "tiny"))
    assert len(params) == 31 and _same_bits(w2, params)
    tr.close()
    tr2 = TR.Trainer(p, board_size=9, seed=99, save_dir=save_dir)           # Trainer::new -> load(model_name)
    assert _same_bits(tr2.phase.net.tensors(), w2)
    tr2.close()


def test_native_backend_refuses_more_than_one_rank(monkeypatch):
    from omok_ai_amd import dist
    from omok_ai_amd import trainer as TR
    monkeypatch.setattr(dist, "shard_info", lambda: (0, 0, 2))
    with pytest.raises(RuntimeError, match="one rank"):
        TR.Trainer(TR.Parameters(train_backend="hip"), board_size=9)
