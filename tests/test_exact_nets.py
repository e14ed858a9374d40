"""CPU tests of tests/exact_nets.py: the proof holds for every net the GPU tests load and fails past a limit, the float64 reference equals two independent
implementations (the float64 torch graph, the oracle's fp32 forward) exactly, and the exact nets are SENSITIVE: a one-unit change of an element of any of the 31
tensors, and each of the layout mistakes named in DESIGN 6, changes a logit on the test rows."""
import numpy as np
import pytest

import exact_nets as E
from helpers import random_positions


@pytest.fixture(scope="module")
def narrow():
    return {n: E.make(n, 0) for n in (9, 15)}


@pytest.mark.parametrize("n,seed,family,wide", E.GPU_NETS)
def test_prove_passes_for_every_net_the_gpu_tests_use(n, seed, family, wide):
    r = E.prove(n, E.make(n, seed, family, wide))
    assert r["modes"] == E.expected_modes(family, wide), (r["modes"], r["why_not"])
    print(f"bounds n={n} seed={seed} {family} {wide}: trunk {r['trunk_units']:.0f} units, h0 {r['h0_units']:.0f} units (|h0| <= {r['h0_magnitude']:.1f}), "
          f"h1 {r['h1_units']:.0f} units (|h1| <= {r['h1_magnitude']:.1f}), |logit| <= {r['logit_bound']:.1f}, |vpre| <= {r['vpre_bound']:.2f}, modes {sorted(r['modes'])}")
    if family == "narrow":
        assert r["trunk_units"] <= 2047 and r["h0_units"] < 2 ** 22 and r["h1_units"] < 2 ** 22 and r["h1_magnitude"] < 65504
    for mode in set(E.MODES) - r["modes"]:
        with pytest.raises(E.NotExact):
            E.prove(n, E.make(n, seed, family, wide), mode=mode)


def test_seeds_cover_every_depthwise_tap_and_every_region(narrow):
    for n in (9, 15):
        nets = [E.make(n, s) for s in (0, 1, 2)]
        for i in range(31):
            if i in E.BIASES:
                continue
            nz = sum((np.asarray(t[i]) != 0).astype(np.int64) for t in nets)
            if i in (4, 11, 18):  # every tap of the depthwise kernels is used by some channel of some seed
                assert np.all(nz.reshape(9, E.M).sum(axis=1) > 0)
            rows = nz.reshape(-1, nz.shape[-1])
            for part in np.array_split(np.arange(rows.shape[0]), min(4, rows.shape[0])):  # quarters of the rows x quarters of the columns
                for cols in np.array_split(np.arange(rows.shape[1]), min(4, rows.shape[1])):
                    assert rows[np.ix_(part, cols)].sum() > 0, (n, i)


def test_prove_fails_past_each_limit(narrow):
    n = 9
    base = narrow[n]

    def bumped(i, index, value):
        t = [a.copy() for a in base]
        t[i].reshape(-1)[index] = value
        return t
    u1 = E.unit_of(base[25])
    with pytest.raises(E.NotExact, match="fc1"):  # one fc1 weight of 2^13 units: h1 no longer splits into hi | lo
        E.prove(n, bumped(25, 0, u1 * 2 ** 13))
    with pytest.raises(E.NotExact, match="negative"):
        E.prove(n, bumped(2, 5, -0.25))
    with pytest.raises(E.NotExact, match="hi \\+ lo"):  # 23 significant bits
        E.prove(n, bumped(9, 3, (2 ** 22 + 1) * 2.0 ** -22))
    with pytest.raises(E.NotExact, match="hi \\+ lo"):  # beyond f16's range
        E.prove(n, bumped(29, 3, 131072.0))
    big = next(t for t in (bumped(7, 0, 2.0 ** k) for k in range(3, 10)) if E.prove(n, t)["trunk_units"] > 2047)  # an up-projection weight that takes the trunk output past 2047 units
    assert E.prove(n, big)["modes"] == {"f32", "f16"}
    with pytest.raises(E.NotExact, match="fp6"):
        E.prove(n, big, mode="fp6")
    with pytest.raises(E.NotExact, match="24 = "):  # one fc0 weight with 13 significant bits: fc0's sums counted in ITS unit pass 2^24
        E.prove(n, bumped(23, 77, 4097 * 2.0 ** -18))
    with pytest.raises(E.NotExact, match="fp6"):  # long fc0 weights on a net thin enough for them: not with fp6 correction terms
        E.prove(n, E.make(n, 0, "wide_weight", 23), mode="mixed")
    with pytest.raises(E.NotExact, match="24"):  # a policy-head column whose sum passes 2^24 units
        t = [a.copy() for a in base]
        t[29][:, 0] = 8 * E.unit_of(base[29])
        E.prove(n, t)


@pytest.mark.parametrize("n", [9, 15])
def test_forward64_equals_the_float64_torch_graph(n, narrow):
    import torch
    from omok_ai_amd.train import Network
    x = random_positions(n, 64, 17)
    _, _, _, lg, vp = E.forward64(n, narrow[n], x)
    net = Network(n, narrow[n], "cpu", dtype=torch.float64, allow_cpu=True)
    with torch.no_grad():
        tl, tv = net.logits_v(torch.as_tensor(x, dtype=torch.float64).reshape(-1, n, n, 3))
    assert np.array_equal(tl.numpy(), lg)  # 0 ulp
    assert torch.equal(tv.reshape(-1), torch.tanh(torch.as_tensor(vp)))
    # the value in front of tanh: Network returns tanh only, so the value head goes through the same graph as column 0 of a policy head
    as_policy = [a.copy() for a in narrow[n]]
    as_policy[29], as_policy[30] = np.zeros_like(as_policy[29]), np.zeros_like(as_policy[30])
    as_policy[29][:, 0], as_policy[30][0] = narrow[n][27][:, 0], narrow[n][28][0]
    with torch.no_grad():
        tvp = Network(n, as_policy, "cpu", dtype=torch.float64, allow_cpu=True).logits_v(torch.as_tensor(x, dtype=torch.float64).reshape(-1, n, n, 3))[0][:, 0]
    assert np.array_equal(tvp.numpy(), vp)  # 0 ulp


@pytest.mark.parametrize("n,family,wide", [(9, "narrow", None), (15, "narrow", None), (9, "wide_act", None), (9, "wide_weight", 29)])
def test_forward64_equals_the_oracle_fp32_forward_bit_for_bit(n, family, wide, narrow):
    from oracle import oracle as O
    t = narrow[n] if family == "narrow" else E.make(n, 0, family, wide)
    assert "f32" in E.prove(n, t)["modes"]
    x = E.plain_rows(n, 64)
    _, _, _, lg, vp = E.forward64(n, t, x)
    p, v, olg, ovp = O.Net(n, t).forward_logits(x, threads=4)
    assert np.array_equal(olg.view(np.uint32), lg.astype(np.float32).view(np.uint32))
    assert np.array_equal(ovp.view(np.uint32), vp.astype(np.float32).view(np.uint32))
    p64, v64 = E.softmax_tanh64(lg, vp)
    assert np.abs(p - p64).max() < 2e-6 and np.abs(v - v64).max() < 2e-6


def _bump_indices(shape, rng, count=8):
    """flat indices: first / last along every axis (all corners), then random picks up to `count` (all elements of a smaller tensor)"""
    size = int(np.prod(shape))
    corners = np.array(np.meshgrid(*[[0, s - 1] for s in shape], indexing="ij")).reshape(len(shape), -1).T
    idx = list(dict.fromkeys(int(np.ravel_multi_index(tuple(c), shape)) for c in corners))
    while len(idx) < min(count, size):
        k = int(rng.integers(0, size))
        if k not in idx:
            idx.append(k)
    return idx


@pytest.mark.parametrize("n", [9, 15])
def test_one_unit_bumps_change_a_logit(n, narrow):
    """Sensitivity, on the reference alone: >= 8 elements per tensor (all of a smaller one) moved by one unit of their tensor, kept only where the net stays provable in
    every mode.  At least 3/4 of them, and one per tensor, change a logit or vpre on 32 of the GPU tests' plain rows (the special boards and 16 random ones: what changes
    there changes on the whole set)."""
    tensors = [a.copy() for a in narrow[n]]
    x = E.plain_rows(n, 300)[:32]
    ref = E.Ref(n, tensors)
    f0 = ref.trunk(x)
    _, _, lg0, vp0 = ref.tail(f0)
    fc0 = E.fc0_summary(n, tensors[23])
    rng = np.random.default_rng(n)
    kept = changed = 0
    per_tensor = []
    for i in range(31):
        unit = E.unit_of(tensors[i])
        hit = tried = 0
        for k in _bump_indices(tensors[i].shape, rng):
            flat32, flat64 = tensors[i].reshape(-1), ref.t[i].reshape(-1)
            old = flat32[k]
            flat32[k] = old + np.float32(unit)
            try:
                r = E.prove(n, tensors, fc0=E.fc0_summary(n, tensors[23]) if i == 23 else fc0)
                provable = r["modes"] == set(E.MODES)
            except E.NotExact:
                provable = False
            if provable:
                flat64[k] = float(flat32[k])
                if i == 23:
                    ref.refresh_fc0()
                _, _, lg, vp = ref.tail(ref.trunk(x) if i < 23 else f0)
                tried += 1
                hit += not (np.array_equal(lg, lg0) and np.array_equal(vp, vp0))
                flat64[k] = float(old)
                if i == 23:
                    ref.refresh_fc0()
            flat32[k] = old
        per_tensor.append((i, hit, tried))
        kept += tried
        changed += hit
    print(f"n={n}: {changed} of {kept} provable one-unit bumps change an output ({changed / kept:.3f}); per tensor (index, changed, kept): {per_tensor}")
    assert all(hit >= 1 for _, hit, _ in per_tensor), per_tensor
    assert kept >= 200 and changed >= 0.75 * kept


@pytest.mark.parametrize("n", [9, 15])
def test_layout_mistakes_change_the_logits(n, narrow):
    """The mistakes the 1e-3 tests let through, made in the reference: two fc0 elements swapped (a non-zero one with a zero one), a pair of depthwise taps
    swapped, a pair of up-projection columns swapped.  Each changes logits on the test rows -- so a kernel that makes it cannot equal the reference."""
    x = E.plain_rows(n, 300)[:32]
    ref = E.Ref(n, narrow[n])
    _, _, _, lg0, _ = ref.forward(x)
    w = ref.t[23]
    r, c = (int(a[0]) for a in np.nonzero(w))
    r2 = next(k for k in range(r + 1, w.shape[0]) if w[k, c] == 0)  # the next zero below it in the same column: a neighbouring (pixel, channel) row
    w[r, c], w[r2, c] = w[r2, c], w[r, c]
    ref.refresh_fc0()
    lg = ref.forward(x)[3]
    rows_fc0 = int((lg != lg0).any(axis=1).sum())
    w[r, c], w[r2, c] = w[r2, c], w[r, c]
    ref.refresh_fc0()
    assert np.array_equal(ref.forward(x)[3], lg0)
    dw = ref.t[4]  # block 0's depthwise [3][3][32][1]: swap channel 0's first non-zero tap with its first zero tap
    taps = dw[:, :, 0, 0].reshape(-1)
    a, b = int(np.flatnonzero(taps != 0)[0]), int(np.flatnonzero(taps == 0)[0])
    taps[a], taps[b] = taps[b], taps[a]
    dw[:, :, 0, 0] = taps.reshape(3, 3)
    lg = ref.forward(x)[3]
    rows_dw = int((lg != lg0).any(axis=1).sum())
    taps[a], taps[b] = taps[b], taps[a]
    dw[:, :, 0, 0] = taps.reshape(3, 3)
    up = ref.t[21].reshape(E.M, E.C)  # block 2's up-projection: swap two output columns fed by different rows
    c0 = 0
    c1 = next(k for k in range(1, E.C) if not np.array_equal(up[:, k], up[:, c0]))
    up[:, [c0, c1]] = up[:, [c1, c0]]
    lg = ref.forward(x)[3]
    rows_up = int((lg != lg0).any(axis=1).sum())
    print(f"n={n}: rows of {len(x)} whose logits change: fc0 element swap {rows_fc0}, depthwise tap swap {rows_dw}, up-projection column swap {rows_up}")
    assert rows_fc0 > 0 and rows_dw > 0 and rows_up > 0


@pytest.mark.parametrize("n", [9, 15])
def test_dense_positions_are_legal_and_touch_every_corner(n):
    import positions as P
    hw = n * n
    boards = E.dense_positions(n, 16, 135 if n == 15 else 48, 2)
    assert all(P.verdict(n, b) == (0, 135 if n == 15 else 48) for b in boards)
    assert np.all(boards[:, [0, n - 1, hw - n, hw - 1]] != 0) and len({b.tobytes() for b in boards}) == 16
