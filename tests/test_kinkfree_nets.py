"""The inputs of tests/test_gpu_train_sizes.py, checked without a GPU: the sign-definite nets of tests/kinkfree_nets.py have no unit near
the LeakyReLU kink, every gradient tensor is alive, torch's own fp32 stays within 1e-4 of float64 (so there are no flipped slopes to hide
behind), and the mistakes the trainer's batch sizes can hold -- a lost 64-row chunk, a lost last K split, a lost last sample, a wrong
slope -- each move the float64 reference by >= 1e-3 on the tensor named: three orders above the bar the GPU tests hold (4 err_t32 + 2^-20,
err_t32 ~ 1e-6).  The bounds are conditions on the inputs (if a seed misses one, pick another seed in kinkfree_nets.SEED; do not move the
bound): 0.02 is half the smallest margin the family showed when it was designed and more than three orders above any fp32 forward error;
1e-4 is ten times the family's worst fp32 figure and below a third of what one flipped unit moves (3e-4).  Figures are printed (run with
-s; recorded in profiles/r32_train_sizes.md)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import omok_ai_amd as oa
import kinkfree_nets as K
import test_gpu_train_native as TN

SIZES = [(9, 65), (9, 128), (9, 193), (15, 65), (15, 128)]   # tests/test_gpu_train_sizes.py: the gradient cases
NAMES = oa.weights.tensor_names()
MUTATION_FLOOR = 1e-3


def test_layers_are_off_the_kink_at_every_size():
    for n, b in SIZES:
        rows = K.margins(n, K.make(n), K.targets(n, b, 1)[0])
        for name, ratio, neg, top in rows:
            print(f"MARGINS N={n} batch={b} {name:18s} min|pre|/max|pre| {ratio:.4f} negative share {neg:.3f} max|pre| {top:.4f}")
        for name, ratio, neg, top in rows[:len(K.LAYERS)]:
            assert ratio >= 0.02 and 0.3 <= neg <= 0.7, (n, b, name, ratio, neg)
        assert rows[-2][0] == "logits" and rows[-2][3] < 2.5 and rows[-1][3] < 1.25  # no saturated softmax, no saturated tanh


def test_targets_are_what_self_play_writes():
    for n, b in SIZES:
        x, pi, z = K.targets(n, b, 1)
        flat, hw = x.reshape(b, -1), n * n
        occupied = (flat[:, 0:2 * hw:2] + flat[:, 1:2 * hw:2]) > 0
        assert pi.dtype == np.float32 and z.dtype == np.float32 and pi.shape == (b, hw) and z.shape == (b, 1)
        assert occupied.any() and not pi[occupied].any() and (pi[~occupied] > 0).all()
        assert np.abs(pi.sum(axis=1, dtype=np.float64) - 1.0).max() <= 2.0 ** -23   # each element rounds within 2^-24 of itself, and they sum to 1
        assert set(z.ravel().tolist()) == {-1.0, 0.0, 1.0} and np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
        assert K.records(n, b, 1).shape[0] == b   # (test_gpu_train_native._pack checks the round trip through the product's decoder, -0.0 included)


@pytest.mark.parametrize("n,b", SIZES)
def test_gradients_are_alive_and_fp32_has_no_flips(n, b):
    g64, g32 = K.grads64(n, b), K.grads32_cpu(n, b)
    bad = []
    for i, name in enumerate(NAMES):
        top, e = float(np.abs(g64[i]).max()), TN._err(g32[i], g64[i])
        print(f"FAMILY N={n} batch={b} tensor {i:2d} {name:34s} max|g64| {top:.3e} err_cpu32 {e:.3e}")
        if not (top >= 1e-3 and e <= 1e-4):
            bad.append((i, name, top, e))
    assert not bad, bad


def test_halves_of_the_data_parallel_cases_have_no_flips_either():
    n, b, cut = 9, 193, 97                          # tests/test_gpu_train_sizes.py: the unequal pair
    for lo, hi in ((0, cut), (cut, b)):
        g64, g32 = K.grads64(n, b, lo, hi), K.grads32_cpu(n, b, lo, hi)
        worst = max(TN._err(a, r) for a, r in zip(g32, g64))
        print(f"FAMILY N={n} records [{lo}, {hi}) of {b}: worst err_cpu32 {worst:.3e} min max|g64| {min(np.abs(g).max() for g in g64):.3e}")
        assert worst <= 1e-4 and min(np.abs(g).max() for g in g64) >= 1e-3


# ---- mutations of the reference: what a mistake at these sizes moves ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tapped_grads(n, b):
    x, pi, z = K.targets(n, b, 1)
    g, pres, dws, logits = K.gradients(n, K.make(n), x, pi, z, taps=True)
    for a, r in zip(g, K.grads64(n, b)):
        assert np.array_equal(a, r)
    return g, pres, dws, logits


def _moved(label, n, b, tensor, delta, g):
    """err of the mutated gradient g - delta against g (the figure of test_gpu_train_native._err)"""
    e = float(np.abs(np.asarray(delta)).max() / np.abs(g).max())
    print(f"MUTATION N={n} batch={b} {label:58s} tensor {tensor:2d} {NAMES[tensor]:34s} err {e:.3e}")
    return e


@pytest.mark.parametrize("n,b", SIZES)
def test_a_lost_chunk_split_or_sample_shows(n, b):
    g, pres, dws, logits = _tapped_grads(n, b)
    low = []

    def check(label, tensor, delta):
        if not _moved(label, n, b, tensor, delta, g[tensor]) >= MUTATION_FLOOR:
            low.append((label, tensor))

    # a bias gradient = the column sums of d loss / d pre in 64-row chunks (launch_colsum): the second chunk lost
    for tensor, rows in ((26, pres[11].grad), (30, logits.grad), (22, K._rows(pres[9].grad))):
        rows = rows.numpy()
        assert np.abs(rows.sum(axis=0) - g[tensor].ravel()).max() <= 1e-12 * np.abs(g[tensor]).max()
        check("bias gradient without rows [64, 128)", tensor, rows[64:128].sum(axis=0))
    # the heads' weight gradients = h1^T . d logits (d vpre) over K = batch in splits of kchunk rows (launch_gemm): the last split lost
    h1 = F.leaky_relu(pres[11].detach(), 0.2).numpy()
    for tensor, nn, d in ((29, n * n, logits.grad.numpy()), (27, 1, None)):
        splits, kchunk = K.gemm_splits(K.NF, nn, b)
        last = b - kchunk * (splits - 1)
        assert splits >= 3 and 1 <= last <= kchunk and (last == 1) == (b in (65, 193))
        if d is None:  # d loss / d vpre per sample = 2 (v - z) (1 - v^2) / batch; the two assertions below tie it to autograd's g[27], g[28]
            w = K.make(n)
            v = np.tanh(h1 @ np.asarray(w[27], np.float64) + np.asarray(w[28], np.float64))
            d = 2.0 * (v - K.targets(n, b, 1)[2]) * (1.0 - v * v) / b
            assert abs(d.sum() - g[28].ravel()[0]) <= 1e-9 * abs(d).max()
        assert np.abs(h1.T @ d - g[tensor].reshape(K.NF, nn)).max() <= 1e-9 * np.abs(g[tensor]).max()
        check(f"head weight gradient without its last K split ({last} of {b} rows)", tensor, h1[b - last:].T @ d[b - last:])
    # fc0's weight gradient: one workgroup per tile loops over K = batch: the last sample lost
    x3 = F.leaky_relu(pres[9].detach(), 0.2).permute(0, 2, 3, 1).reshape(b, -1).numpy()
    d0 = pres[10].grad.numpy()
    probe = np.abs(g[23]).argmax()
    assert abs(x3[:, probe // K.NF] @ d0[:, probe % K.NF] - g[23].ravel()[probe]) <= 1e-12 * np.abs(g[23]).max()
    check("fc0 weight gradient without sample batch - 1", 23, np.abs(x3[b - 1]).max() * np.abs(d0[b - 1]).max())
    # depthwise taps: one partial per sample, the samples added in order (k_depthwise_taps, k_colsum_final): sample 64 lost
    for i, (h, d) in enumerate(dws):
        tensor = 4 + 7 * i
        whole = torch.nn.grad.conv2d_weight(h.detach(), (K.M, 1, 3, 3), d.grad, padding=1, groups=K.M)
        assert np.abs(whole.permute(2, 3, 0, 1).numpy() - g[tensor]).max() <= 1e-12 * np.abs(g[tensor]).max()
        check("depthwise tap gradient without sample 64", tensor,
              torch.nn.grad.conv2d_weight(h.detach()[64:65], (K.M, 1, 3, 3), d.grad[64:65], padding=1, groups=K.M).numpy())
    assert not low, low


@pytest.mark.parametrize("n,b", [(9, 128), (15, 65)])
def test_a_wrong_slope_on_one_negative_channel_shows(n, b):
    g = K.grads64(n, b)
    layer, tensor = 4, 10                               # block 1's down-projection and its bias
    assert K.LAYERS[layer][2] == tensor
    bias = K.make(n)[tensor]
    c = int(np.argmax(np.where(bias < 0, np.abs(g[tensor]), 0.0)))   # the negative channel whose bias gradient is largest
    assert bias[c] < 0

    def leaky(i, pre, slope):
        out = F.leaky_relu(pre, slope)
        if i != layer:
            return out
        assert bool((pre[:, c] < 0).all())              # sign-definite: the whole channel is on the 0.2 slope
        mask = torch.zeros(pre.shape[1], dtype=torch.bool)
        mask[c] = True
        return torch.where(mask[None, :, None, None], pre, out)

    x, pi, z = K.targets(n, b, 1)
    mutant = K.gradients(n, K.make(n), x, pi, z, leaky=leaky)
    e = TN._err(mutant[tensor], g[tensor])
    print(f"MUTATION N={n} batch={b} {'slope 1 instead of 0.2 on channel %d of block1.down' % c:58s} tensor {tensor:2d} {NAMES[tensor]:34s} err {e:.3e}")
    assert e >= MUTATION_FLOOR
