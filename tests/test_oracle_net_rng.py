"""Oracle net vs the independent torch fixtures; RNG contract known answers."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import omok_ai_amd  # noqa: F401
from omok_ai_amd import weights
from oracle import oracle as O
from helpers import BoltzmannCheck, check_root_noise

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("n", [9, 15])
def test_net_matches_torch_fixture(n):
    g = np.load(os.path.join(GOLD, f"net_n{n}.npz"))
    tensors = weights.init_random(n, seed=int(g["seed"]))
    assert weights.checksum(tensors) == pytest.approx(float(g["weight_checksum"]), rel=1e-12)
    net = O.Net(n, tensors)
    p, v = net.forward(g["inputs"], threads=4)
    assert np.abs(p - g["p"]).max() < 1e-4  # fp32 restatement vs float64 torch (fp32 rounding only)
    assert np.abs(v - g["v"]).max() < 1e-4
    assert np.allclose(p.sum(axis=1), 1.0, atol=1e-5)


@pytest.mark.parametrize("n", [9, 15])
def test_forward_logits_is_the_same_forward(n):
    """orc_net_forward_logits (the checker of north_star's tolerance on the LOGITS, network.rs:227-247): p and v are those of orc_net_forward bit for bit, and they
    are softmax / tanh of the logits it hands out."""
    g = np.load(os.path.join(GOLD, f"net_n{n}.npz"))
    net = O.Net(n, weights.init_random(n, seed=int(g["seed"])))
    x = g["inputs"][:6]
    p, v = net.forward(x, threads=2)
    p2, v2, lg, vp = net.forward_logits(x, threads=2)
    assert np.array_equal(p.view(np.uint32), p2.view(np.uint32)) and np.array_equal(v.view(np.uint32), v2.view(np.uint32))
    e = np.exp(lg.astype(np.float64) - lg.max(axis=1, keepdims=True))
    assert np.abs(e / e.sum(axis=1, keepdims=True) - p).max() < 1e-6
    assert np.abs(np.tanh(vp.astype(np.float64)) - v).max() < 1e-6


def test_weight_tensor_sizes():
    for n, total in ((9, 5643250), (15, 15154306)):
        shapes = weights.tensor_shapes(n)
        assert len(shapes) == 31 == O.lib().orc_net_num_tensors()
        assert sum(int(np.prod(s)) for s in shapes) == total
        net = O.Net(n)
        for i, s in enumerate(shapes):
            assert O.lib().orc_net_tensor_size(net.h, i) == int(np.prod(s))


def test_philox_known_answers():
    """Philox4x32-10 KATs from the Random123 distribution (kat_vectors)."""
    out = (C.c_uint32 * 4)()
    O.lib().orc_philox(0, 0, 0, 0, 0, out)
    assert list(out) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    O.lib().orc_philox(0xffffffffffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, out)
    assert list(out) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    O.lib().orc_philox((0x299f31d0 << 32) | 0xa4093822, 0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, out)
    assert list(out) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_det_log_exp_accuracy():
    L = O.lib()
    for x in [1e-300, 1e-10, 0.03, 0.5, 0.9999, 1.0, 1.5, 2.0, 10.0, 12345.678, 1e300]:
        assert L.orc_det_log(x) == pytest.approx(math.log(x), rel=1e-14, abs=1e-15)
    for x in [-700.0, -50.0, -1.0, -1e-9, 0.0, 1e-9, 0.5, 1.0, 3.3, 50.0, 700.0]:
        assert L.orc_det_exp(x) == pytest.approx(math.exp(x), rel=1e-14)
    assert L.orc_det_exp(-800.0) == 0.0
    for x in np.linspace(0.0, 1.0, 33, dtype=np.float32):
        assert abs(L.orc_det_expf(float(x)) - np.exp(np.float32(x))) <= 2e-7 * np.exp(x)
    # the arguments of Boltzmann sampling, pi / T in [0, 80] (include/omok_mi355x.h): float64 exp rounded to fp32, within 1 ulp
    xs = np.concatenate([np.linspace(0.0, 80.0, 321), 80.0 * np.random.default_rng(0).random(2000)]).astype(np.float32)
    for x in xs:
        want = np.float32(np.exp(np.float64(x)))
        got = np.float32(L.orc_det_expf(float(x)))
        assert abs(np.float64(got) - np.float64(want)) <= np.float64(np.spacing(want)), float(x)


def test_gamma_distribution():
    """Dirichlet noise source: Gamma(alpha) draws have mean alpha (and variance alpha)."""
    L = O.lib()
    for alpha in (0.03, 0.5, 1.0, 2.5):
        xs = np.array([L.orc_gamma(alpha, 123, c % 200, c // 200, 7) for c in range(20000)], dtype=np.float64)
        assert np.all(xs >= 0)
        assert xs.mean() == pytest.approx(alpha, rel=0.08)
        assert xs.var() == pytest.approx(alpha, rel=0.2)
    assert L.orc_gamma(0.03, 1, 2, 3, 4) == L.orc_gamma(0.03, 1, 2, 3, 4)


def test_gamma_above_33_is_not_gamma():
    """Why the engine rejects alpha > 33: k is clamped to 32 and the rest f = alpha - 32 goes to Ahrens-Dieter GS, which samples Gamma(f)
    only for f <= 1.  Up to 33 the mean is alpha; "Gamma(40)" has a mean near 33.9."""
    L = O.lib()
    means = {}
    for alpha in (32.5, 33.0, 40.0):
        xs = np.array([L.orc_gamma(alpha, 123, c % 200, c // 200, 7) for c in range(20000)], dtype=np.float64)
        means[alpha] = xs.mean()
    print(means)
    for alpha in (32.5, 33.0):
        assert means[alpha] == pytest.approx(alpha, abs=5 * math.sqrt(alpha / 20000))
    assert means[40.0] < 35.0


def _equally_visited(n, games, children):
    """an oracle whose side-0 roots have `children` children of one visit each: one round of `children` simulations expands that many
    distinct cells"""
    sp = O.SelfPlay(n, games, cap_nodes=64, cap_tables=8, seed=7, game_offset=5)
    hw = n * n
    sp.reset(np.full(hw, 1.0 / hw, dtype=np.float32))
    x = sp.round_generate(0, children, 0.25, 0.03)
    assert len(x) == games * children
    sp.round_scatter(np.full((len(x), hw), 1.0 / hw, dtype=np.float32), np.zeros(len(x), dtype=np.float32))
    return sp


def test_overflowing_temperature_plays_cell_zero():
    """Why the engine rejects 1 / temperature > 80: pi = 1/32 on 32 equally visited children and 1 / T = 32 * 86 give exp(86) = 2.2e37 per child,
    the fp32 sum of 32 of them is inf, every normalised weight is 0, the scan finds no positive weight and falls through to cell 0 -- for every
    game and every u (the reference panics here, agent.rs:130).  At pi / T = 80 the same position still samples among its children."""
    n, games = 9, 6
    sp = _equally_visited(n, games, 32)
    pol = [sp.compute_policy(g) for g in range(games)]
    assert all(p is not None and (p > 0).sum() == 32 and np.all(p[p > 0] == np.float32(1 / 32)) for p in pol)
    acts = sp.sample(1.0 / 32.0 / 86.0, 99)
    assert np.all(acts == 0)
    sp = _equally_visited(n, games, 32)
    acts = sp.sample(1.0 / 32.0 / 80.0, 99)
    assert all(pol[g][acts[g]] > 0 for g in range(games)) and len(set(acts.tolist())) > 1


@pytest.mark.parametrize("n,games", [(9, 256), (15, 128)])
def test_oracle_root_noise_is_dirichlet(n, games):
    """(the yardstick of tests/test_gpu_search_settings.py proven first: the same check runs on the engine there)"""
    hw = n * n
    for alpha in (0.03, 0.3, 1.0, 2.5):
        sp = O.SelfPlay(n, games, cap_nodes=16, cap_tables=4, seed=7, game_offset=5)
        sp.reset(np.full(hw, 1.0 / hw, dtype=np.float32))
        sp.round_generate(0, 8, 1.0, alpha)
        dev = check_root_noise(sp, games, hw, alpha, f"oracle N={n}")
        assert abs(dev) < 3.0  # (the device is held to 5: the yardstick itself must stand well inside)


@pytest.mark.parametrize("count", [32, 128])
@pytest.mark.parametrize("temperature", [0.25, 4.0, 0.05, 0.0125, math.inf])
def test_oracle_boltzmann_sampling_matches_float64(temperature, count):
    """orc_sp_sample against the float64 restatement of agent.rs:106-133 (helpers.boltzmann_expected), 8 games x 10 plies at N = 9.  32
    simulations leave a root with untried actions, so every child has one visit and the policy is uniform; 128 are more than the 81 cells, the
    root is fully expanded, PUCT concentrates the visits and pi / T leaves [0, 1]."""
    from test_oracle_literal import FakeNet
    n, games, k, seed, offset = 9, 8, 8, 7, 5
    net = FakeNet(n)
    sp = O.SelfPlay(n, games, cap_nodes=2048, cap_tables=1024, seed=seed, game_offset=offset)
    sp.reset(net.forward(O.Environment(n).encode_nn_input(0)[None])[0][0])
    chk = BoltzmannCheck(seed, offset, temperature)
    for ply in range(10):
        for rnd in range(count // k):
            x = sp.round_generate(rnd, k, 0.25, 0.03)
            sp.round_scatter(*net.forward(x))
        pol = [sp.compute_policy(g) for g in range(games)]
        has = np.array([p is not None for p in pol])
        pi = np.stack([p if p is not None else np.zeros(n * n, np.float32) for p in pol])
        chk(ply, pi, has, sp.sample(temperature, 99))
        sp.advance(net.forward(sp.mirror_generate())[0])
    assert sp.error == 0
    chk.finish(f"oracle, {count} simulations", 8 * 10 - 8, min_nonuniform=40 if count == 128 else 0)
