"""GPU tests on exact-arithmetic nets (tests/exact_nets.py): every forward path of every operand format against the float64 reference with NO tolerance.
`prove` shows for every board that each product the kernels form is exact, each partial sum an integer below 2^24 of one unit and no pre-activation negative, so
whatever the summation order, K split, tile order, window rectangle or cache state, logits and the value in front of tanh must be the float64 numbers: a misplaced
weight, a dropped tap, a wrong row or a stale cache entry is a different integer.  Logits / vpre: equality of the bits.  p / v: the bar of tests/test_gpu_parity.py for
k_softmax / tanhf (2e-6) against float64 softmax / tanh of the exact logits."""
import functools

import numpy as np
import pytest

import omok_ai_amd as oa
from omok_ai_amd import binding as B
import exact_nets as E

pytestmark = pytest.mark.gpu
PV_TOL = 2e-6  # tests/test_gpu_parity.py: fp32 softmax / tanhf against the oracle's
MODE_ID = {"f32": B.NET_F32, "fp6": B.NET_F16X3_FP6, "f16": B.NET_F16X3_F16, "mixed": B.NET_F16X3_MIXED, "default": B.NET_F16X3}
ROWS = 300


@functools.lru_cache(maxsize=None)
def _net(n, seed, family, wide):
    tensors = E.make(n, seed, family, wide)
    return tensors, E.Ref(n, tensors), E.prove(n, tensors)["modes"]


@functools.lru_cache(maxsize=None)
def _rows(n):
    return E.plain_rows(n, ROWS)


@functools.lru_cache(maxsize=None)
def _plain_reference(n, seed, family, wide):
    """(logits, vpre as float32 -- exact conversions, forward64 asserts it --, p, v in float64) of the plain rows: computed once per net"""
    _, ref, _ = _net(n, seed, family, wide)
    _, _, _, lg, vp = E.forward64(n, ref, _rows(n))
    return (lg.astype(np.float32), vp.astype(np.float32)) + E.softmax_tanh64(lg, vp)


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def _describe(lg, vp, rlg, rvp):
    """where a result differs: rows, columns and the differences in units of the smallest one (the integers make a misplaced element easy to find)"""
    bad = np.argwhere(lg != rlg)
    d = (lg.astype(np.float64) - rlg)[lg != rlg]
    vbad = np.flatnonzero(vp != rvp)
    return (f"{len(bad)} logits differ in {len(set(bad[:, 0]))} rows (first (row, cell): {bad[:4].tolist()}, differences {d[:4].tolist()}, "
            f"largest {np.abs(d).max() if d.size else 0.0}); {len(vbad)} vpre differ (rows {vbad[:4].tolist()})")


def _check(tag, got, want, index=None):
    """got = (logits, vpre, p, v) of the engine, want = the reference tuple (rows `index` of it)"""
    lg, vp, p, v = got
    rlg, rvp, p64, v64 = (a if index is None else a[index] for a in want)
    lg, p = lg.reshape(rlg.shape), p.reshape(rlg.shape)
    assert _bits_equal(lg, rlg) and _bits_equal(vp.reshape(-1), rvp), f"{tag}: {_describe(lg, vp.reshape(-1), rlg, rvp)}"
    dp, dv = float(np.abs(p - p64).max()), float(np.abs(v.reshape(-1) - v64).max())
    assert dp < PV_TOL and dv < PV_TOL, f"{tag}: |dp| {dp:.2e} |dv| {dv:.2e} against float64 softmax / tanh of exact logits"


# ---- a (and d): plain rows -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", E.MODES)
@pytest.mark.parametrize("n", [9, 15])
def test_plain_rows_are_exact(n, mode):
    """omok_evaluate_logits / omok_evaluate_pv on 300 positions (empty, one-stone and full-minus-one boards with both sides to move, random ones) in batches of 1, 5, 127,
    128, 129 and 300 rows on a 512-row engine, of 300 and 4300 rows on a 4608-row engine (the 4300 are the 300 repeated: 34 tiles make both planners pick other K splits),
    for every net of E.GPU_NETS that `prove` admits in this mode: the narrow seeds 0..2 in all five modes, wide_act and the long fc0 weights where fc0's correction terms
    are f16 or the kernels fp32 -- and there also one trunk 1x1 per block with long weights --, long fc1 / policy-head weights everywhere."""
    x = _rows(n)
    small = oa.Engine(board_size=n, games=32, max_nodes=16, max_tables=8, max_batch_k=16, net_mode=MODE_ID[mode])
    large = oa.Engine(board_size=n, games=288, max_nodes=16, max_tables=8, max_batch_k=16, net_mode=MODE_ID[mode])
    plans, nets = [], 0
    for nn, seed, family, wide in E.GPU_NETS:
        tensors, _, modes = _net(nn, seed, family, wide)
        if nn != n or mode not in modes:
            continue
        assert modes == E.expected_modes(family, wide)
        want = _plain_reference(n, seed, family, wide)
        nets += 1
        for eng, batches in ((small, (1, 5, 127, 128, 129, ROWS) if family == "narrow" else (5, 129, ROWS)), (large, (ROWS, 4300) if family == "narrow" else (4300,))):
            eng.load_weights(tensors)
            if mode != "f32":
                fmt = B.FC0_FORMATS[int(eng.stats()["fc0_format"])]
                assert fmt == mode or mode == "default", (fmt, mode)
            for b in batches:
                index = np.arange(b) % ROWS if b > ROWS else np.arange(ROWS - b, ROWS) if b in (127, 129) else np.arange(b)  # (127 / 129: the last rows, so every row is in a short batch too)
                lg, vp = eng.evaluate_logits(x[index])
                plan = eng.last_plan()
                p, v = eng.evaluate_pv(x[index])
                assert plan["path"] == ("f32" if mode == "f32" else "plain") and (mode == "f32" or (eng.last_plan() == plan and plan["rows"] == b)), plan  # (the fp32 kernels work in chunks)
                plans.append((plan["nsplit"], plan["tsplit"]))
                _check(f"n={n} {mode} {family} {wide} seed {seed} batch {b} nsplit {plan['nsplit']} tsplit {plan['tsplit']}", (lg, vp, p, v), want, index)
    small.close()
    large.close()
    assert nets == sum(1 for nn, _, family, wide in E.GPU_NETS if nn == n and mode in E.expected_modes(family, wide)) >= 5
    print(f"n={n} {mode}: {nets} nets, (nsplit, tsplit) seen {sorted(set(plans))}")
    if mode != "f32":  # (the fp32 kernels have no K split)
        assert len({a for a, _ in plans}) >= 2 and len({b for _, b in plans}) >= 2, sorted(set(plans))


# ---- b: the commit probe ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,games,k", [(15, 32, 16), (15, 256, 16), (9, 32, 8), (9, 160, 8)])
def test_commit_probe_measures_zero_on_an_exact_net(n, games, k):
    """Default mode: the probe compares the split formats with the fp32 kernels on 2048 synthetic rows and, on an engine whose rounds reach the difference path, on a
    synthetic sibling round.  On an exact net all of them compute the same numbers, so every published figure is 0.0 (a NaN or a non-zero figure out of the fp6 block
    scales of all-zero residual blocks, which no random net produces, would show here), the format kept is the fastest and the verdict is `inside`."""
    eng = oa.Engine(board_size=n, games=games, max_nodes=64, max_tables=32, max_batch_k=k)
    eng.load_weights(_net(n, 0, "narrow", None)[0])
    st = eng.stats()
    eng.close()
    rounds = games * k >= (3072 if n == 15 else 1024)
    assert st["probe_rows"] >= 512 and (st["probe_round_rows"] >= 256) == rounds, st
    figures = [f"probe_{q}_{f}" for q in ("dp", "dv", "dlogit") for f in ("fp6", "f16")]
    if rounds:
        figures += [f"probe_round_{q}_{f}" for q in ("dp", "dv", "dlogit") for f in ("fp6", "mixed", "f16")]
    print(f"n={n} games={games}: " + " ".join(f"{name}={st[name]!r}" for name in figures))
    assert all(st[name] == 0.0 for name in figures), {name: st[name] for name in figures if not st[name] == 0.0}
    assert B.FC0_FORMATS[int(st["fc0_format"])] == "fp6" and int(st["probe_outside"]) == 0
    assert st["probe_logit_max"] > 1.0  # (the probe did evaluate the net)


def _sibling_runs(x, hw, games, k):
    """(start, end) of the sibling runs among the request rows, read off the rows themselves: the children of one position differ from each other in exactly two of the
    2 HW stone floats and share the turn plane, so a run ends where the next row is further away; and, while every tree issues its k requests (the list is compacted
    otherwise), at every multiple of k, since a run belongs to one tree (at ply 0 all trees expand the same root position)."""
    d = (x[1:, :2 * hw] != x[:-1, :2 * hw]).sum(axis=1)
    same = (d == 2) & (x[1:, 2 * hw] == x[:-1, 2 * hw])
    if len(x) == games * k:
        same[np.arange(k, len(x), k) - 1] = False
    cuts = np.flatnonzero(~same) + 1
    return list(zip(np.concatenate([[0], cuts]).tolist(), np.concatenate([cuts, [len(x)]]).tolist()))


# ---- c (and d): search rounds on their own paths ---------------------------------------------------------------------------------------------------------------
def _play_rounds(n, games, k, mode, net_key, path, cache=True, rects=True, start=None, plies=2, rounds=4, switch=None):
    """`plies` plies x `rounds` step-wise rounds; per round every row of 8 whole sibling runs (_sibling_runs, read off the request rows themselves) plus 128 random rows
    against forward64 (at most 512 rows).  Returns (rows checked, paths of the rounds, children2 launches)."""
    tensors, ref, modes = _net(*net_key)
    assert mode in modes
    eng = oa.Engine(board_size=n, games=games, max_nodes=512, max_tables=128, max_batch_k=k, seed=31, net_mode=MODE_ID[mode])
    eng.load_weights(tensors)
    if not cache:
        eng.set_base_cache(False)
    if not rects:
        eng.set_window_rects(False)
    sp = oa.SelfPlay(eng)
    if start is None:
        sp.reset()
    else:
        sp.reset_from(start)
    rng = np.random.default_rng(games + k)
    checked, paths = 0, []
    for ply in range(plies):
        for rnd in range(rounds):
            nreq = sp.round_generate(rnd, k, 0.25, 0.03)
            x = sp.round_inputs().copy()
            p, v = sp.round_eval()
            lg, vp = sp.round_logits()
            plan = eng.last_plan()
            sp.round_scatter()
            paths.append(plan["path"])
            runs = [r for r in _sibling_runs(x, n * n, games, k) if 2 <= r[1] - r[0] <= k]
            assert len(runs) >= 8, f"round {rnd} of ply {ply}: {len(runs)} sibling runs among {nreq} rows"
            whole = np.concatenate([np.arange(*runs[i]) for i in rng.choice(len(runs), size=8, replace=False)])
            pick = np.concatenate([whole, np.setdiff1d(rng.choice(nreq, size=min(128, nreq), replace=False), whole)])[:512]
            assert len(whole) <= 512
            _, _, _, rlg, rvp = E.forward64(n, ref, x[pick])
            want = (rlg.astype(np.float32), rvp.astype(np.float32)) + E.softmax_tanh64(rlg, rvp)
            _check(f"n={n} {games}x{k} {mode} {net_key[2]} ply {ply} round {rnd} ({plan['path']}, {nreq} rows, cache {cache}, rects {rects})",
                   (lg[pick], vp[pick], np.array(p).reshape(nreq, -1)[pick], np.array(v).reshape(-1)[pick]), want)
            checked += len(pick)
        sp.sample_actions(1.0, 30)
        sp.advance()
    launches = int(eng.stats()["children2_launches"])
    eng.close()
    print(f"n={n} {games}x{k} {mode} {net_key[2]}: {checked} rows exact, paths {paths}, children2 launches {launches}")
    assert all(set(paths[ply * rounds + 1:(ply + 1) * rounds]) == {path} for ply in range(plies)), paths  # (a ply's first round may hold roots only)
    assert launches >= plies * (rounds - 1) if path == "difference" else launches == 0
    return checked


@pytest.mark.parametrize("mode", ["fp6", "f16", "mixed"])
@pytest.mark.parametrize("n,games,k,path", [(15, 256, 16, "difference"), (15, 64, 16, "copy"), (9, 160, 8, "difference")])
def test_search_rounds_are_exact(n, games, k, path, mode):
    """Step-wise rounds with the base cache on (later rounds reuse cached bases): 4096-row rounds on the difference path and 1024-row rounds on the copy path at N = 15,
    1280-row rounds on the difference path at N = 9, in the three split formats."""
    assert _play_rounds(n, games, k, mode, (n, 1, "narrow", None), path) >= 8 * 128


@pytest.mark.parametrize("what", ["no base cache", "no window rectangles", "dense start"])
def test_search_rounds_are_exact_without_cache_without_rectangles_and_from_dense_positions(what):
    """One N = 15 difference-path configuration each with omok_debug_set_base_cache(0), with omok_debug_set_window_rects(0), and started by reset_from on boards of 135
    stones with a stone in every corner: the children's windows lie on edges and corners, and bases are crowded boards."""
    n, games, k = 15, 256, 16
    start = E.dense_positions(n, games, 135, 2) if what == "dense start" else None
    _play_rounds(n, games, k, "mixed" if what == "dense start" else "fp6", (n, 2, "narrow", None), "difference", cache=what != "no base cache",
                 rects=what != "no window rectangles", start=start)


def test_long_trunk_weights_are_exact_on_the_difference_path():
    """wide_weight with block 1's pointwise carrying 12-bit weights: lo fragments of the packed trunk weights, and ~22-bit activations (non-zero lo) in every later layer of
    k_trunk and k_sib_children2, in the base entries, the operand rows and the difference rows; f16 format, 256 x 16."""
    _play_rounds(15, 256, 16, "f16", (15, 0, "wide_weight", 12), "difference", plies=1)


@pytest.mark.parametrize("mode", ["f16", "f32"])
def test_wide_activations_are_exact_on_search_rounds(mode):
    """wide_act (trunk output with ~13 bits: non-zero residual parts in the operand rows, the base entries and the difference rows) through the rounds of a 256 x 16
    engine: the difference path in the f16 format; the fp32 kernels' own path in OMOK_NET_F32 on 64 x 16 (they keep the logits of 1024 rows)."""
    _play_rounds(15, 256 if mode == "f16" else 64, 16, mode, (15, 0, "wide_act", None), "difference" if mode == "f16" else "f32", plies=1)


# ---- e: commits ---------------------------------------------------------------------------------------------------------------------------------------------
def test_commits_leave_nothing_behind():
    """One engine: exact net seed 0, the random initialiser, exact net seed 0 again; after each commit plain rows and one ply of three difference-path rounds.  The first
    and third results are exact: no stale packed fragment, conv table or cached base survives a commit."""
    n, games, k = 15, 256, 16
    tensors, ref, _ = _net(n, 0, "narrow", None)
    want = _plain_reference(n, 0, "narrow", None)
    x = _rows(n)
    eng = oa.Engine(board_size=n, games=games, max_nodes=512, max_tables=128, max_batch_k=k, seed=5)
    sp = oa.SelfPlay(eng)
    for step, t in enumerate((tensors, oa.weights.init_random(n, seed=0), tensors)):
        eng.load_weights(t)
        lg, vp = eng.evaluate_logits(x)
        p, v = eng.evaluate_pv(x)
        if step != 1:
            _check(f"commit {step}: plain rows", (lg, vp, p, v), want)
        else:
            assert not _bits_equal(lg, want[0])
        sp.reset()
        for rnd in range(3):
            nreq = sp.round_generate(rnd, k, 0.25, 0.03)
            xr = sp.round_inputs().copy()
            p, v = sp.round_eval()
            lg, vp = sp.round_logits()
            sp.round_scatter()
            if step != 1:
                pick = np.arange(0, nreq, max(1, nreq // 256))[:256]
                _, _, _, rlg, rvp = E.forward64(n, ref, xr[pick])
                _check(f"commit {step}: round {rnd}", (lg[pick], vp[pick], np.array(p).reshape(nreq, -1)[pick], np.array(v).reshape(-1)[pick]),
                       (rlg.astype(np.float32), rvp.astype(np.float32)) + E.softmax_tanh64(rlg, rvp))
    assert int(eng.stats()["children2_launches"]) >= 6
    eng.close()
