"""Sign-definite ("kink-free") nets, self-play-shaped targets and the float64 yardstick of the native training step at the trainer's batch
sizes (a helper of tests/test_kinkfree_nets.py and tests/test_gpu_train_sizes.py; not a test, no product code, no GPU).

Why: at batch >= ~40 a random net has dozens of pre-activations within fp32 rounding of the LeakyReLU kink; two correct fp32 implementations
put them on different sides, one flipped slope moves a gradient tensor by up to 3e-4, and the rule err_hip <= 4 err_t32 + 2^-20 stops
being a statement about summation order (random_net_flips() below re-measures this).  In the nets made here every term of every
pre-activation has its unit's sign:

  trunk channel c has one sign s_x[c] through conv_in and all three blocks (so the residual add is sign-consistent); per block the
  down-projection channels have signs s_h, the pointwise channels s_g; fc0 has s0, fc1 has s1.  A weight from input j to output c is
  s_in[j] s_out[c] |init_random|; the net's input is 0/1 (s_in = +1), fc0's input sign is s_x tiled over the NHWC flatten; depthwise taps
  are positive; the bias of an activated unit is s_out[c] U(0.05, 0.15).  The two head matrices keep init_random's free signs and get
  small random biases.

So |pre| >= |bias| > 0 everywhere, about half the units sit on the 0.2 slope, and no unit is near the kink.  Rescaling, front to back, on a
fixed 16-record probe batch: each activated layer's weight matrix is divided so that the layer's max |pre| is its target: 1 for every
layer off the trunk, and 0.25, 0.5, 0.75, 1 for conv_in and the three block outputs (the skip connection carries the trunk's magnitude
forward whatever the up-projection is divided by, so the trunk cannot be held at one figure; a rising target can, because every term has
one sign: |pre| = |W a| / alpha + |b| + |x| and alpha = max over units of |W a| / (target - |b| - |x|)).  Then the policy head (matrix and
bias) is scaled to max |logit| = 2 and the value head to max |vpre| = 1 on the probe."""
import contextlib
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

import omok_ai_amd as oa
from omok_ai_amd import train as T
import test_gpu_train_native as TN

C, M, NF = oa.weights.C, oa.weights.M, oa.weights.F
SEED = 3                 # the family's seed in both test files (pick another if a condition of tests/test_kinkfree_nets.py is missed)
PROBE = (16, 7)          # records and seed of the probe batch
TRUNK_TARGETS = (0.25, 0.5, 0.75, 1.0)
# the activated layers in the order Network.logits_v reaches them: (name, weight tensor, bias tensor)
LAYERS = [("conv_in", 0, 1)]
for _i in range(3):
    LAYERS += [(f"block{_i}.down", 2 + 7 * _i, 3 + 7 * _i), (f"block{_i}.pointwise", 5 + 7 * _i, 6 + 7 * _i), (f"block{_i}.up", 7 + 7 * _i, 8 + 7 * _i)]
LAYERS += [("fc0", 23, 24), ("fc1", 25, 26)]


# ---- the float64 forward of train.Network with its pre-activations in hand ------------------------------------------------------
@contextlib.contextmanager
def _tapped(leaky=None):
    """Network's own code runs unchanged; the leaky_relu, the depthwise conv2d and the log_softmax it calls go through recorders
    (pre-activations, (input, output) of each depthwise layer, logits).  leaky(i, pre): replaces
    the i-th activation (the mutations of tests/test_kinkfree_nets.py)."""
    pres, dws, lgs = [], [], []

    def leaky_relu(a, slope):
        pres.append(a)
        return F.leaky_relu(a, slope) if leaky is None else leaky(len(pres) - 1, a, slope)

    def conv2d(a, w, b, **kw):
        out = F.conv2d(a, w, b, **kw)
        if kw.get("groups", 1) > 1:
            dws.append((a, out))
        return out

    def log_softmax(a, **kw):
        lgs.append(a)
        return F.log_softmax(a, **kw)

    saved = T.F
    T.F = types.SimpleNamespace(leaky_relu=leaky_relu, conv2d=conv2d, log_softmax=log_softmax)
    try:
        yield pres, dws, lgs
    finally:
        T.F = saved


def _net64(n, tensors):
    return T.Network(n, tensors, "cpu", dtype=torch.float64, allow_cpu=True)


def _rows(pre):
    """[B, C, H, W] or [B, F] -> [rows, channels]"""
    return pre.permute(0, 2, 3, 1).reshape(-1, pre.shape[1]) if pre.ndim == 4 else pre


def margins(n, tensors, x):
    """per activated layer (the order of LAYERS): (name, min|pre| / max|pre|, negative share, max|pre|), from the float64 forward of
    train.Network; then ("logits", ...) and ("vpre", ...) with their max |.| (the share is that of negative entries)"""
    net = _net64(n, tensors)
    with torch.no_grad(), _tapped() as (pres, _, _):
        logits, v = net.logits_v(torch.as_tensor(x, dtype=torch.float64))
    assert len(pres) == len(LAYERS)
    out = []
    for (name, _, _), pre in list(zip(LAYERS, pres)) + [(("logits", 0, 0), logits), (("vpre", 0, 0), torch.atanh(v))]:
        a = pre.abs()
        out.append((name, float(a.min() / a.max()), float((pre < 0).double().mean()), float(a.max())))
    return out


# ---- the family ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make(n, seed=SEED):
    """the 31 fp32 tensors of a sign-definite net (module text)"""
    hw = n * n
    rng = np.random.default_rng([seed, n])
    t = [np.abs(np.asarray(a, np.float64)) for a in oa.weights.init_random(n, seed)]
    free = oa.weights.init_random(n, seed)
    sign = lambda k: rng.choice([-1.0, 1.0], size=k)  # noqa: E731
    bias = lambda s: s * rng.uniform(0.05, 0.15, size=s.shape)  # noqa: E731
    s_x, s0, s1 = sign(C), sign(NF), sign(NF)
    t[0] = t[0] * s_x                      # [1, 1, 3, C]: the input planes are 0 / 1
    t[1] = bias(s_x)
    for i in range(3):
        s_h, s_g = sign(M), sign(M)
        o = 2 + 7 * i
        t[o] = t[o] * (s_x[:, None] * s_h[None, :])
        t[o + 1] = bias(s_h)
        # t[o + 2]: the depthwise taps stay positive: d keeps s_h
        t[o + 3] = t[o + 3] * (s_h[:, None] * s_g[None, :])
        t[o + 4] = bias(s_g)
        t[o + 5] = t[o + 5] * (s_g[:, None] * s_x[None, :])
        t[o + 6] = bias(s_x)
    t[23] = t[23] * (np.tile(s_x, hw)[:, None] * s0[None, :])   # NHWC flatten: index = pixel * C + channel
    t[24] = bias(s0)
    t[25] = t[25] * (s0[:, None] * s1[None, :])
    t[26] = bias(s1)
    for w, b in ((27, 28), (29, 30)):
        t[w] = np.asarray(free[w], np.float64)
        t[b] = rng.uniform(-0.05, 0.05, size=t[b].shape)
    # rescale front to back on the probe batch
    x = torch.as_tensor(TN._batch(n, *PROBE)[0], dtype=torch.float64)
    targets = iter(TRUNK_TARGETS)
    for li, (name, wi, bi) in enumerate(LAYERS):
        target = next(targets) if name == "conv_in" or name.endswith(".up") else 1.0
        with torch.no_grad(), _tapped() as (pres, _, _):
            _net64(n, t).logits_v(x)
        pre = _rows(pres[li]).numpy()
        b = t[bi][None, :]
        assert (np.sign(pre) == np.sign(b)).all(), name          # sign-definite: every unit has its bias's sign
        if name.endswith(".up"):                                # |pre| = |W g| + |b| + |x|: the skip's share stays
            skip = np.abs(_rows(F.leaky_relu(pres[li - 3], 0.2)).numpy())
        else:
            skip = 0.0
        wa = np.abs(pre) - np.abs(b) - skip
        room = target - np.abs(b) - skip
        assert wa.max() > 0 and (room > 0).all(), name           # (wa is 0 where every input is: an empty cell with White to move)
        t[wi] = t[wi] / (wa / room).max()
    with torch.no_grad():
        logits, v = _net64(n, t).logits_v(x)
    s = 2.0 / float(logits.abs().max())
    t[29], t[30] = t[29] * s, t[30] * s
    s = 1.0 / float(torch.atanh(v).abs().max())
    t[27], t[28] = t[27] * s, t[28] * s
    return tuple(a.astype(np.float32).reshape(sh) for a, sh in zip(t, oa.weights.tensor_shapes(n)))


@functools.lru_cache(maxsize=None)
def targets(n, b, seed):
    """(x, pi, z) like test_gpu_train_native._batch, with the targets as self-play writes them: pi is zero on occupied cells and sums to 1 in fp32
    rounding over the empty ones; z is drawn from {-1, -0.0, 0, 1}"""
    x, _, _ = TN._batch(n, b, seed)
    rng = np.random.default_rng([seed, n, b])
    flat = x.reshape(b, -1)
    hw = n * n
    empty = (flat[:, 0:2 * hw:2] + flat[:, 1:2 * hw:2]) == 0
    assert empty.sum(axis=1).min() >= 2
    pi = rng.random((b, hw)) * empty
    pi = (pi / pi.sum(axis=1, keepdims=True)).astype(np.float32)
    z = rng.choice(np.array([-1.0, -0.0, 0.0, 1.0], np.float32), size=(b, 1))
    z[:4, 0] = np.array([-1.0, -0.0, 0.0, 1.0], np.float32)  # all four are there at any batch
    return x, pi, z


@functools.lru_cache(maxsize=None)
def records(n, b, seed):
    return TN._pack(n, *targets(n, b, seed))


# ---- the yardstick -------------------------------------------------------------------------------------------------------------
def gradients(n, tensors, x, pi, z, dtype=torch.float64, device="cpu", leaky=None, taps=False):
    """the 31 gradients of train.Network's loss by autograd (numpy); taps: also (pres, dws, logits) with their .grad kept"""
    net = T.Network(n, tensors, device, dtype=dtype, allow_cpu=True)
    with _tapped(leaky) as (pres, dws, lgs):
        loss = net.losses(*(torch.as_tensor(a, dtype=dtype, device=device) for a in (x, pi, z)))[2]
    logits, = lgs
    if taps:  # (non-leaf .grad is filled by backward() for tensors marked before it)
        for a in pres + [d for _, d in dws] + [logits]:
            a.retain_grad()
    loss.backward()
    g = [p.grad.cpu().numpy().copy() for p in net.vars]
    return (g, pres, dws, logits) if taps else g


@functools.lru_cache(maxsize=None)
def grads64(n, b, lo=0, hi=None, seed=SEED):
    """float64 gradients of the family's net on records [lo, hi) of targets(n, b, 1): the reference of every case, computed once"""
    x, pi, z = (a[lo:hi] for a in targets(n, b, 1))
    return tuple(gradients(n, make(n, seed), x, pi, z))


@functools.lru_cache(maxsize=None)
def grads32_cpu(n, b, lo=0, hi=None, seed=SEED):
    x, pi, z = (a[lo:hi] for a in targets(n, b, 1))
    return tuple(gradients(n, make(n, seed), x, pi, z, dtype=torch.float32))


def gemm_splits(m, nn, k):
    """launch_gemm's plan (train_kernels.hip), restated: (splits, kchunk) of a [m][nn] product over K = k"""
    tiles = ((m + 63) // 64) * ((nn + 63) // 64)
    if tiles >= 512:
        return 1, (k + 15) // 16 * 16
    want = max(1, min(1024 // tiles, (k + 31) // 32))
    kchunk = ((k + want - 1) // want + 15) // 16 * 16
    return (k + kchunk - 1) // kchunk, kchunk


# ---- the random nets the family replaces, re-measured ----------------------------------------------------------------------------
def random_net_flips(n, b, kind):
    """(worst fp32-vs-float64 err over the 31 tensors, its tensor, count of pre-activations with 0 < |pre| < 1e-6 layer max) of torch on
    the CPU with the weights and batch of tests/test_gpu_train_native.py"""
    tensors = oa.weights.init_random(n, seed=1)
    if kind == "scaled":
        brng = np.random.default_rng(9)
        tensors = [(np.asarray(t, np.float64) * 0.25 + (0.1 * brng.standard_normal(t.shape) if t.ndim == 1 else 0.0)).astype(np.float32) for t in tensors]
    x, pi, z = TN._batch(n, b, 1)
    g64, pres, _, _ = gradients(n, tensors, x, pi, z, taps=True)
    g32 = gradients(n, tensors, x, pi, z, dtype=torch.float32)
    errs = [TN._err(a, r) for a, r in zip(g32, g64)]
    near = sum(int(((p.abs() > 0) & (p.abs() < 1e-6 * p.abs().max())).sum()) for p in pres)
    return max(errs), int(np.argmax(errs)), near
