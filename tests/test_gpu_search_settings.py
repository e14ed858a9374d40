"""The search settings off their defaults: epsilon, alpha (Dirichlet noise) and temperature (Boltzmann sampling) are public arguments of
omok_execute, omok_round_generate, omok_sample_actions, the run loops and omok_execute_shared; every other GPU test passes 0.25 / 0.03 / 1.0.
  a. bit-exact against the oracle, one setting off default at a time (gamma_draw's unit-exponential loop, its f == 0 case, its rejection
     loop at f where both branches are common, the clamp at alpha = 33; apply_noise at epsilon 0 and 1; det_expf outside [0, 1])
  b. the run loops and the shared-tree executor hand the settings through
  c. the root noise against the analytic Dirichlet and numpy's sampler (independent of the oracle, which shares the kernel's design)
  d. the sampled moves against a float64 restatement of agent.rs:106-133 (independent of orc_sp_sample)
  e. the bounds of include/omok_mi355x.h: alpha in (0, 33], 1 / temperature <= 80, rejected by every entry point before anything changes
The same checks run on the oracle alone, without a GPU, in tests/test_oracle_literal.py and tests/test_oracle_net_rng.py."""
import math

import numpy as np
import pytest
import torch

import omok_ai_amd as oa
from omok_ai_amd import binding as B
from helpers import BoltzmannCheck, check_root_noise, drive_selfplay_vs_oracle, episode_records
from test_gpu_shared_tree import replay_recorded_on_literal  # (the issue: the settings go through that file's own driver)

pytestmark = pytest.mark.gpu

ALL_OFF = {"epsilon": 0.5, "alpha": 2.5, "temperature": 0.25}
SEED, OFFSET = 7, 5  # (the defaults of drive_selfplay_vs_oracle)


def _ids(s):
    return ",".join(f"{k}={v:.6g}" for k, v in s.items())


# ---- a. bit-exact against the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("settings", [
    {"alpha": 0.3},                            # rejection loop with b * u1 > 1 in ~10 % of the attempts (1 % at 0.03)
    {"alpha": 1.0},                            # f == 0: one unit exponential, no rejection loop
    {"alpha": 2.5},                            # two unit exponentials (counters cell * 256 + 255 - i) + f = 0.5
    {"alpha": float(np.float32(10.0 / 3.0))},  # a fraction that is no short binary number: f = fp32(10/3) - 3 in double
    {"alpha": 33.0},                           # k clamped to 32, f = 1: the largest alpha the engine takes
    {"epsilon": 0.0},                          # the row is renormalised all the same: the bits change
    {"epsilon": 1.0},                          # (1 - epsilon) * p vanishes: pure noise
    {"temperature": 0.25},
    {"temperature": 4.0},
    {"temperature": 0.05},
    ALL_OFF,
], ids=_ids)
def test_one_setting_off_default_bit_exact_vs_oracle(settings):
    """N = 9, 3 games, 32 simulations in rounds of 8, 6 plies, every ply Boltzmann (threshold 99).  The temperature cases also hold every
    sampled move against the float64 restatement (d)."""
    chk = BoltzmannCheck(SEED, OFFSET, settings["temperature"]) if "temperature" in settings else None
    drive_selfplay_vs_oracle(9, 3, 32, 8, 6, B.NET_F16X3, threshold=99, on_sample=chk, **settings)
    if chk is not None:
        chk.finish("engine N=9", 3 * 6)


def test_all_settings_off_default_bit_exact_vs_oracle_n15():
    """IT = 4 at N = 15: the last of the four 64-lane passes over the 225 cells has pad lanes (noise draws, heated weights)"""
    chk = BoltzmannCheck(SEED, OFFSET, ALL_OFF["temperature"])
    drive_selfplay_vs_oracle(15, 2, 32, 16, 3, B.NET_F16X3, threshold=99, on_sample=chk, **ALL_OFF)
    chk.finish("engine N=15", 2 * 3)


@pytest.mark.parametrize("temperature", [0.0125, math.inf], ids=["T=0.0125", "T=inf"])
def test_the_ends_of_the_temperature_range_bit_exact_vs_oracle(temperature):
    """Both ends of what omok_sample_actions accepts: 1 / T = 80 (fp32: 0.0125f is a little above 1/80), the largest exp arguments, and
    T = +inf, 1 / T = 0: every visited cell weighs exp(0) = 1, uniform over the visited cells as agent.rs:110-128 computes it."""
    chk = BoltzmannCheck(SEED, OFFSET, temperature)
    drive_selfplay_vs_oracle(9, 3, 32, 8, 3, B.NET_F16X3, threshold=99, on_sample=chk, temperature=temperature)
    chk.finish("engine N=9", 3 * 3)


# ---- a / d with a fully expanded root ----------------------------------------------------------------------------------------------
# While a root has untried actions every simulation expands one of them (node.rs:43-58): with 32 simulations the noise sits in the root's row
# (and is compared there, bit for bit) but steers nothing, and the visit policy is uniform, so every temperature picks the same move.  128
# simulations are more than the 81 cells of N = 9: PUCT reads the noisy row, pi has unequal entries and pi / T really leaves [0, 1].
@pytest.mark.parametrize("settings", [
    ALL_OFF,
    {"epsilon": 1.0, "alpha": 0.3},
    {"temperature": 0.05},
    {"temperature": 0.0125},
    {"temperature": math.inf},
], ids=_ids)
def test_settings_off_default_with_a_fully_expanded_root(settings):
    chk = BoltzmannCheck(SEED, OFFSET, settings.get("temperature", 1.0))
    shape = drive_selfplay_vs_oracle(9, 2, 128, 8, 4, B.NET_F16X3, threshold=99, on_sample=chk, **settings)
    assert shape[0] >= 1  # (a fully expanded node: the root)
    chk.finish("engine N=9, 128 simulations", 2 * 4, min_nonuniform=2 * 4)


# ---- d. in a driver of its own: more games, more plies --------------------------------------------------------------------------
@pytest.mark.parametrize("count", [32, 128])
@pytest.mark.parametrize("temperature", [0.25, 4.0, 0.05])
def test_boltzmann_moves_match_the_float64_restatement(temperature, count):
    chk = BoltzmannCheck(SEED, OFFSET, temperature)
    drive_selfplay_vs_oracle(9, 8, count, 8, 10, B.NET_F16X3, threshold=99, on_sample=chk, temperature=temperature)
    chk.finish(f"engine N=9, 8 games x 10 plies, {count} simulations", 8 * 10 - 8, min_nonuniform=40 if count == 128 else 0)


# ---- b. the run loops carry the settings ----------------------------------------------------------------------------------------
def _engine(n, games, k, seed=3, **kw):
    eng = oa.Engine(board_size=n, games=games, max_nodes=2048, max_tables=1024, max_batch_k=k, seed=seed, **kw)
    eng.load_weights(oa.weights.init_random(n, seed=0))
    sp = oa.SelfPlay(eng)
    sp.reset()
    return eng, sp


def _state(sp, games):
    return [sp.tree_dump(g, s) for g in range(games) for s in (0, 1)], [sp.replay(g) for g in range(games)]


def _same_state(a, b):
    for (ai, af), (bi, bf) in zip(a[0], b[0]):
        assert np.array_equal(ai, bi) and np.array_equal(af.view(np.uint32), bf.view(np.uint32))
    for ra, rb in zip(a[1], b[1]):
        assert len(ra[1]) == len(rb[1]) > 0
        for x, y in zip(ra, rb):
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)


@pytest.mark.parametrize("count", [32, 128])
def test_selfplay_run_matches_stepwise_with_all_settings_off_default(count):
    """count = 32 cannot see a dropped setting (every root keeps untried actions: the same trees at every setting); count = 128 can, and
    asserts that the default settings leave other trees."""
    n, games, k = 9, 5, 8
    eps, alpha, temp = ALL_OFF["epsilon"], ALL_OFF["alpha"], ALL_OFF["temperature"]
    states = []
    for variant in ("run", "stepwise"):
        eng, sp = _engine(n, games, k)
        if variant == "run":
            sp.run(count, k, eps, alpha, temp, 99, 3)
        else:
            for _ in range(3):
                for rnd in range(count // k):
                    sp.round_generate(rnd, k, eps, alpha)
                    sp.round_eval()
                    sp.round_scatter()
                sp.sample_actions(temp, 99)
                sp.mirror_generate()
                sp.mirror_eval()
                sp.mirror_apply()
        assert sp.ply == 3
        states.append(_state(sp, games))
        eng.close()
    _same_state(states[0], states[1])
    if count == 32:
        return  # (untried actions left at every root: the trees are the same at every setting, see above)
    # ... and the settings reached the kernels: the default settings leave other trees
    eng, sp = _engine(n, games, k)
    sp.run(count, k, 0.25, 0.03, 1.0, 99, 3)
    default = _state(sp, games)
    eng.close()
    assert any(ai.shape != bi.shape or not np.array_equal(af.view(np.uint32), bf.view(np.uint32)) for (ai, af), (bi, bf) in zip(states[0][0], default[0]))


@pytest.mark.parametrize("count", [32, 128])
def test_run_slots_matches_run_with_all_settings_off_default(count):
    """count = 32 cannot see a dropped setting (uniform visit policies, and the records hold no root prior); count = 128 can, and asserts
    that the default settings play other games."""
    n, slots, total, k, seed, max_nodes = 9, 5, 7, 8, 21, 2048
    eps, alpha, temp = ALL_OFF["epsilon"], ALL_OFF["alpha"], ALL_OFF["temperature"]
    want, want_status, _ = episode_records(n, total, count, k, 99, B.NET_F16X3, seed, max_nodes, eps, alpha, temp)
    eng = oa.Engine(board_size=n, games=slots, max_nodes=max_nodes, max_tables=max_nodes // 2, max_batch_k=k, seed=seed)
    eng.load_random_weights(0)
    sp = oa.SelfPlay(eng)
    sp.reset()
    rec = sp.replay_record_bytes()
    cap = total * n * n
    buf = torch.zeros(cap * rec, dtype=torch.uint8, device="cuda")
    _, nrec, off, ln, status = sp.run_slots(total, count, k, buf.data_ptr(), cap, eps, alpha, temp, 99)
    out = buf.cpu().numpy().reshape(-1, rec)
    assert nrec == sum(len(w) for w in want)
    for g in range(total):
        assert ln[g] == len(want[g]) and status[g] == want_status[g], f"game {g}"
        assert np.array_equal(out[off[g]:off[g] + ln[g]], want[g]), f"game {g}: records differ"
    eng.close()
    if count == 128:  # the settings reached the kernels of both runs: the default settings play other games
        default, _, _ = episode_records(n, total, count, k, 99, B.NET_F16X3, seed, max_nodes)
        assert any(len(d) != len(w) or not np.array_equal(d, w) for d, w in zip(default, want))


def test_execute_shared_carries_the_noise_settings():
    """waves = 1 under the recorded schedule against O.Literal.shared_run, and the free-running omok_execute_shared(waves = 1) against the
    recorded one with the same settings"""
    replay_recorded_on_literal(9, 96, 8, 1, 4, epsilon=0.5, alpha=2.5, temperature=0.25, threshold=99)
    n, count, k = 9, 96, 8
    engines = [_engine(n, 1, k, seed=13, max_tree_waves=1) for _ in range(2)]
    (a_eng, a), (b_eng, b) = engines
    a.execute_shared(count, k, 0.5, 2.5, waves=1)
    b.execute_shared_recorded(count, k, 0.5, 2.5, waves=1)
    _same_state((_state(a, 1)[0], []), (_state(b, 1)[0], []))
    a_eng.close()
    b_eng.close()


# ---- c. the root noise is Dirichlet(alpha) --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,games", [(9, 256), (15, 128)])
def test_root_noise_is_dirichlet(n, games):
    eng = oa.Engine(board_size=n, games=games, max_nodes=64, max_tables=32, max_batch_k=8, seed=SEED, game_offset=OFFSET)
    eng.load_random_weights(0)
    sp = oa.SelfPlay(eng)
    for alpha in (0.03, 0.3, 1.0, 2.5):
        sp.set_episode(0)  # (every alpha on the stream of episode 0, like a fresh engine)
        sp.reset()
        sp.round_generate(0, 8, 1.0, alpha)
        check_root_noise(sp, games, n * n, alpha, f"engine N={n}")
        sp.round_eval()
        sp.round_scatter()
    eng.close()


# ---- e. the bounds ----------------------------------------------------------------------------------------------------------------
def test_out_of_range_settings_are_rejected_and_change_nothing():
    """(the shared-tree entry points need an engine with games = 1: the test below)"""
    n, games, count, k = 9, 4, 16, 8
    (eng, sp), (twin_eng, twin) = _engine(n, games, k), _engine(n, games, k)
    for s in (sp, twin):  # one ply played: trees with children, replay records, ply 1
        s.execute(count, k)
        s.sample_actions(1.0, 99)
        s.advance()
        s.execute(count, k)
    before = _state(sp, games)
    rec = sp.replay_record_bytes()
    cap = 16 * n * n
    buf = torch.zeros(cap * rec, dtype=torch.uint8, device="cuda")
    log = torch.zeros(cap * 20, dtype=torch.uint8, device="cuda")

    def rejected(call, word):
        with pytest.raises(B.OmokError) as ei:
            call()
        assert ei.value.code == -1 and word in str(ei.value), ei.value  # (OMOK_ERR_INVALID, and for this argument)
        assert sp.ply == 1

    for alpha in (33.5, math.inf, -math.inf, math.nan):
        rejected(lambda: sp.execute(count, k, 0.25, alpha), "alpha")
        rejected(lambda: sp.round_generate(0, k, 0.25, alpha), "alpha")
        rejected(lambda: sp.run(count, k, 0.25, alpha, 1.0, 99, 1), "alpha")
        rejected(lambda: sp.run_slots(16, count, k, buf.data_ptr(), cap, 0.25, alpha, 1.0, 99), "alpha")
        rejected(lambda: sp.run_slots_logged(16, count, k, buf.data_ptr(), cap, log.data_ptr(), 0.25, alpha, 1.0, 99), "alpha")
        rejected(lambda: sp.versus_run(B.OPP_NAIVE, 0, count, k, 0.25, alpha, 1), "alpha")
    for temperature in (0.012, math.nan, 0.0, -1.0):
        rejected(lambda: sp.sample_actions(temperature, 99), "temperature")
        rejected(lambda: sp.run(count, k, 0.25, 0.03, temperature, 99, 1), "temperature")
        rejected(lambda: sp.run_slots(16, count, k, buf.data_ptr(), cap, 0.25, 0.03, temperature, 99), "temperature")
        rejected(lambda: sp.run_slots_logged(16, count, k, buf.data_ptr(), cap, log.data_ptr(), 0.25, 0.03, temperature, 99), "temperature")
    _same_state(before, _state(sp, games))
    for s in (sp, twin):  # a valid call afterwards, at the accepted ends of both ranges, behaves as on the twin
        acts = s.sample_actions(0.0125, 99)
        assert np.all(acts >= 0)
        s.advance()
        s.execute(count, k, 1.0, 33.0)
    assert sp.ply == twin.ply == 2
    _same_state(_state(sp, games), _state(twin, games))
    eng.close()
    twin_eng.close()


def test_out_of_range_alpha_is_rejected_by_the_shared_tree_executors():
    """omok_execute_shared and omok_execute_shared_recorded on an engine they accept (games = 1, waves = 1): only alpha is wrong"""
    n, count, k = 9, 32, 8
    (eng, sp), (twin_eng, twin) = (_engine(n, 1, k, seed=13, max_tree_waves=1) for _ in range(2))
    for s in (sp, twin):
        s.execute_shared(count, k, waves=1)
        s.sample_actions(1.0, 99)
        s.advance()
        s.execute_shared(count, k, waves=1)
    before = _state(sp, 1)
    for alpha in (33.5, math.inf, -math.inf, math.nan):
        for call in (lambda: sp.execute_shared(count, k, 0.25, alpha, waves=1), lambda: sp.execute_shared_recorded(count, k, 0.25, alpha, waves=1)):
            with pytest.raises(B.OmokError) as ei:
                call()
            assert ei.value.code == -1 and "alpha" in str(ei.value), ei.value
            assert sp.ply == 1
    _same_state(before, _state(sp, 1))
    for s in (sp, twin):  # a valid call afterwards, at the accepted end of the range
        s.sample_actions(1.0, 99)
        s.advance()
        s.execute_shared(count, k, 1.0, 33.0, waves=1)
    groups = sp.execute_shared_recorded(count, k, 1.0, 33.0, waves=1)
    assert len(groups) == count // k and len(twin.execute_shared_recorded(count, k, 1.0, 33.0, waves=1)) == len(groups)
    assert sp.ply == twin.ply == 2
    _same_state(_state(sp, 1), _state(twin, 1))
    eng.close()
    twin_eng.close()
