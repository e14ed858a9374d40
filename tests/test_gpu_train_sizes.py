"""GPU tests (run with -m gpu) of the native training step at the batch sizes the trainer uses (parameter_update_batch_size = 128 on
15 x 15), where train_kernels.hip first reaches: launch_colsum and k_depthwise_taps / k_colsum_final over more than one 64-row chunk of
samples, split-K of the head and fc weight gradients in three or more splits and with a one-row last split (batch 65 -> 3 splits, 128 -> 4,
193 -> 7), fc0's unsplit weight gradient over K = batch > 37, k_draw's sorted list over up to 64 chunks, omok_train_run's log window.

Yardstick and rule are those of tests/test_gpu_train_native.py: float64 autograd of omok_ai_amd.train on the CPU, err = max|g - g64| /
max|g64| per tensor, err_hip <= 4 err_t32 + 2^-20 with err_t32 from torch's own fp32 autograd on the GPU in the same test.  The weights
are the sign-definite nets of tests/kinkfree_nets.py and the records carry targets as self-play writes them (pi zero on occupied cells,
z in {-1, -0.0, 0, 1}).  There is NO "kink" and no "scaled" parametrisation at these sizes: measured with torch on the CPU, fp32 against
float64, on the weights and batches of tests/test_gpu_train_native.py (kinkfree_nets.random_net_flips; profiles/r32_train_sizes.md):

  weights  (n, batch)  worst fp32 err     pre-activations with 0 < |pre| < 1e-6 layer max
  kink     (9, 37)     5.5e-6
  kink     (9, 128)    3.0e-4 (tensor 14) 28 in block 2's up-projection alone
  kink     (9, 193)    2.4e-4
  kink     (15, 128)   5.8e-6             90 over the trunk
  scaled   (15, 128)   4.0e-6             50 over the trunk

At these sizes a random net has dozens of units within fp32 rounding of the LeakyReLU kink; which side each falls on differs between two
correct fp32 implementations, one flipped slope moves a gradient tensor by up to 3e-4, and the rule becomes a lottery between two sets
of flips.  tests/test_kinkfree_nets.py shows (without a GPU) that the family used here has no such unit, that torch's fp32 stays within
1e-4 (measured: 7e-6) of float64 on it, and that a lost chunk, split or sample moves the reference by >= 1e-3.  Figures are printed
before each assertion (run with -s; recorded in profiles/r32_train_sizes.md)."""
import numpy as np
import pytest
import torch

import omok_ai_amd as oa
import kinkfree_nets as K
import test_gpu_train_native as TN
import train_batches as TB

pytestmark = pytest.mark.gpu

DEV = TN.DEV
NAMES = oa.weights.tensor_names()


def _grads32_gpu(n, b, lo=0, hi=None):
    x, pi, z = (a[lo:hi] for a in K.targets(n, b, 1))
    return K.gradients(n, K.make(n), x, pi, z, dtype=torch.float32, device=DEV)


def _gradients(eng):
    return [eng.train_gradient(i) for i in range(31)]


def _cpu_figures(label, g32, ref):
    """torch fp32 on the CPU beside the GPU's figures: for the record only"""
    for i, name in enumerate(NAMES):
        print(f"FIGURES {label} tensor {i:2d} {name:34s} err_cpu32 {TN._err(g32[i], ref[i]):.3e}")


# ---- a. gradients ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,b", [(9, 65), (9, 128), (9, 193), (15, 65), (15, 128)])
def test_gradients_against_float64_autograd(n, b):
    ref, g32 = K.grads64(n, b), _grads32_gpu(n, b)
    eng = TN._engine(n, K.make(n), b)
    dev = TN._upload(K.records(n, b, 1))
    eng.train_step(dev.data_ptr(), b, np.arange(b))
    ghip = _gradients(eng)
    eng.close()
    label = f"gradient N={n} batch={b} weights=kinkfree"
    _cpu_figures(label, K.grads32_cpu(n, b), ref)
    TN._hold(label, NAMES, ghip, g32, ref)


# ---- b. Adadelta, elementwise -----------------------------------------------------------------------------------------------------
def test_adadelta_elementwise_on_the_engines_own_gradient():
    """w1 - w0 against the float64 ApplyAdadelta formula (oracle/train.py: adadelta_apply) on the gradient the engine itself read back, so
    that only k_adadelta is under test: all 31 tensor sizes, the partly filled last 1024-element workgroup of each included.  The constants
    are the op's fp32 attributes (rho = float32(0.95); 1 - rho formed in fp32, which is exact; epsilon = float32(1e-8); lr = float32(0.01)),
    the arithmetic on them is float64; for step 2 the formula runs on both gradients with its float64 accumulators carried.
    Tolerance, derived and not measured: |error| <= 8 x 2^-24 |update| + ulp(w).  Each fp32 rounding of the formula is at most 2^-24
    relative; the three under the denominator's square root (g g, its scaling, the sum) weigh half, the two square roots, the quotient, the
    product with g and the product with lr weigh fully: 6.5 x 2^-24 |update|, under 8; the store w - update rounds once more, within one
    ulp of w.  The worst |error| / tolerance over all elements is printed."""
    n, b = 9, 128
    tensors = K.make(n)
    eng = TN._engine(n, tensors, b)
    dev = TN._upload(K.records(n, b, 1))
    rho, eps, lr = (float(np.float32(v)) for v in (0.95, 1e-8, 0.01))
    one_rho = float(np.float32(1.0) - np.float32(0.95))
    w = [np.asarray(t, np.float32).ravel() for t in tensors]
    acc = [np.zeros(t.size) for t in w]
    accu = [np.zeros(t.size) for t in w]
    for step in (1, 2):
        eng.train_step(dev.data_ptr(), b, np.arange(b))
        w1, g = eng.read_weights(), _gradients(eng)
        worst = 0.0
        for i in range(31):
            g64 = g[i].astype(np.float64)
            acc[i] = rho * acc[i] + one_rho * g64 * g64
            upd = np.sqrt(accu[i] + eps) / np.sqrt(acc[i] + eps) * g64
            accu[i] = rho * accu[i] + one_rho * upd * upd
            want = -lr * upd
            got = w1[i].astype(np.float64) - w[i].astype(np.float64)
            tol = 8 * 2.0 ** -24 * np.abs(want) + np.spacing(np.maximum(np.abs(w[i]), np.abs(w1[i])))
            over = np.abs(got - want) / tol
            worst = max(worst, float(over.max()))
            assert g[i].any() and np.abs(got).max() > 0
            assert (over <= 1.0).all(), (step, i, NAMES[i], int(over.argmax()), float(over.max()))
        print(f"ADADELTA step {step}: worst |error| / tolerance over all elements {worst:.3f}")
        w = w1
    eng.close()


# ---- c. the draw ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [300, 4096])
def test_large_batch_indices_equal_the_restatement(batch):
    """k_draw's sorted list at 5 and at all 64 of its 64-entry chunks (TRAIN_MAX_BATCH = 4096)"""
    eng = TN._engine(9, K.make(9), 4096)
    key = 0x0123456789ABCDEF
    for n_records in (batch, batch + 1, 5000, 1_000_003):
        for step in (0, 7):
            got = eng.train_batch_indices(n_records, batch, key, step)
            assert got.dtype == np.int64 and got.size == batch, (n_records, step)
            assert got.min() >= 0 and got.max() < n_records and np.unique(got).size == batch, (n_records, step)
            assert got.tolist() == TB.draw(n_records, batch, key, step), (n_records, step)
    eng.close()


# ---- d. the run's window and edges -------------------------------------------------------------------------------------------------
def _loop(twin, dev, r, count, batch, key, window):
    """draws and steps by hand; the fp32 in-step-order sums of the last `window` steps"""
    sums = np.zeros(3, np.float32)
    for s in range(count):
        idx = twin.train_batch_indices(r, batch, key, s)
        losses = np.asarray(twin.train_step(dev.data_ptr(), r, idx), np.float32)
        if s >= count - window:
            sums += losses
    return sums


def test_run_longer_than_its_log_window():
    n, r, count, batch, key = 9, 50, 130, 8, 0xC0FFEE
    tensors = K.make(n)
    dev = TN._upload(K.records(n, r, 2))
    eng, twin = TN._engine(n, tensors, batch), TN._engine(n, tensors, batch)
    means = eng.train_run(dev.data_ptr(), r, count, batch, key)
    sums = _loop(twin, dev, r, count, batch, key, 100)
    assert TN._same_bits(eng.read_weights(), twin.read_weights())
    assert means == tuple(float(v) for v in sums / np.float32(100))
    whole = TN._engine(n, tensors, batch)   # the window shows: the mean over all 130 steps is another figure
    assert means != tuple(float(v) for v in _loop(whole, dev, r, count, batch, key, count) / np.float32(count))
    for e in (eng, twin, whole):
        e.close()


def test_run_of_no_steps_returns_zeros_and_changes_nothing():
    n, r, batch = 9, 50, 8
    tensors = K.make(n)
    x = K.targets(n, r, 2)[0][:4].reshape(4, -1)
    dev = TN._upload(K.records(n, r, 2))
    eng = TN._engine(n, tensors, batch)
    before = eng.evaluate_pv(x)
    assert eng.train_run(dev.data_ptr(), r, 0, batch, 1) == (0.0, 0.0, 0.0)
    assert TN._same_bits(eng.read_weights(), tensors)
    after = eng.evaluate_pv(x)   # still committed, on the same net (the run commits again: within the project's 1e-3 evaluation contract)
    assert np.abs(before[0] - after[0]).max() < 1e-3 and np.abs(before[1] - after[1]).max() < 1e-3
    eng.close()


def test_run_on_fewer_records_than_a_batch():
    n, r, count, batch, key = 9, 5, 6, 16, 0xBEEF
    tensors = K.make(n)
    dev = TN._upload(K.records(n, r, 2))
    eng, twin = TN._engine(n, tensors, batch), TN._engine(n, tensors, batch)
    means = eng.train_run(dev.data_ptr(), r, count, batch, key)
    sums = np.zeros(3, np.float32)
    for s in range(count):
        idx = twin.train_batch_indices(r, batch, key, s)
        assert idx.size == r and sorted(idx.tolist()) == list(range(r))   # k = 5: every record, in the step's own order
        sums += np.asarray(twin.train_step(dev.data_ptr(), r, idx), np.float32)
    assert TN._same_bits(eng.read_weights(), twin.read_weights()) and not TN._same_bits(eng.read_weights(), tensors)
    assert means == tuple(float(v) for v in sums / np.float32(count))
    eng.close()
    twin.close()


# ---- e. the same gradient through the two halves -----------------------------------------------------------------------------------
def _halves(n, b, cut):
    """the averaged gradient two engines hold after omok_train_backward on records [0, cut) / [cut, b) and omok_train_apply(ranks = 2)"""
    tensors = K.make(n)
    ea, eb = TN._engine(n, tensors, max(cut, b - cut)), TN._engine(n, tensors, max(cut, b - cut))
    dev = TN._upload(K.records(n, b, 1))
    exchange = torch.zeros((2, ea.train_gradient_count()), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()  # (the engines write and read it on streams of their own)
    ea.train_backward(dev.data_ptr(), b, np.arange(cut), exchange[0].data_ptr())   # the exchange, emulated as in tests/test_gpu_train_dp.py
    eb.train_backward(dev.data_ptr(), b, np.arange(cut, b), exchange[1].data_ptr())
    ea.train_apply(exchange.data_ptr(), 2)
    eb.train_apply(exchange.data_ptr(), 2)
    ga, gb = _gradients(ea), _gradients(eb)
    ea.close()
    eb.close()
    assert TN._same_bits(ga, gb)
    return ga


def test_equal_halves_against_float64_autograd_of_the_full_batch():
    n, b = 15, 128
    TN._hold(f"dp gradient N={n} halves=2x64 weights=kinkfree", NAMES, _halves(n, b, 64), _grads32_gpu(n, b), K.grads64(n, b))


def test_unequal_halves_against_the_float64_mean_of_their_gradients():
    """97 + 96 records: rank averaging defines the mean of the two halves' mean-loss gradients (not the gradient of the union's mean
    loss); torch's fp32 figure is formed the same way, in float64 from its two fp32 gradients"""
    n, b, cut = 9, 193, 97
    mean = lambda p, q: [(np.asarray(a, np.float64) + np.asarray(c, np.float64)) * 0.5 for a, c in zip(p, q)]  # noqa: E731
    ref = mean(K.grads64(n, b, 0, cut), K.grads64(n, b, cut, b))
    g32 = mean(_grads32_gpu(n, b, 0, cut), _grads32_gpu(n, b, cut, b))
    TN._hold(f"dp gradient N={n} halves={cut}+{b - cut} weights=kinkfree", NAMES, _halves(n, b, cut), g32, ref)
