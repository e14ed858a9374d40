"""The net forward at the launch shapes an episode passes through on its way from full rounds to a few rows.

Every change of shape is a planner's decision: forward_f16x3 (host) picks the path of a sibling round (copy / difference by the row
bound), the dense fc0's K split `nsplit` (1..64, uneven last split) and the tail GEMMs' `tsplit` (8 / 4 / 2 / 1); k_bin_prefix (device)
picks the window tiles' K-split set (`t_split`, moved down to a bin start), its `ways` (1..14) and the full-row fc0's `fways` (1..64).
Here the live count is SET (helpers.scripted_finish through omok_play_actions: dead and live trees interleaved), the plan taken is READ
(omok_debug_last_plan), and every row of every checked round is compared with an OMOK_NET_F32 engine's evaluation of the same inputs, a
seeded sample of 48 rows per round with the oracle's forward -- 1e-3 on p, v, the logits and the value in front of tanh (north_star).
The last test of each half asserts the planner classes the recorded plans cover; when a change moves the planners and it fails, re-pick the
points with tools/scan_launch_shapes.py.  Reference: alpha-zero/src/agent_model.rs:116-134, parallel_mcts_executor.rs:194-265."""
import time

import numpy as np
import pytest

import omok_ai_amd as oa
from omok_ai_amd import binding as B
from oracle import oracle as O
from helpers import LAUNCH_SHAPE_LADDER, plan_text, random_positions, scripted_finish

pytestmark = pytest.mark.gpu
TOL = 1e-3
MODES = {"fp6": B.NET_F16X3_FP6, "f16": B.NET_F16X3_F16, "mixed": B.NET_F16X3_MIXED, "default": B.NET_F16X3}
WEIGHT_SEED = 1
ROUNDS = 4        # round 0 (a partial round) and three sibling rounds of live x K rows
ORACLE_ROWS = 48  # per round

_RECORDED = []    # (engine key, point, round, to-move, plan) of every checked round of the ladder
_PLAIN = []       # (board, mode, engine rows, B, plan) of the plain-row test
_T0 = time.time()


class _Refs:
    """fp32 kernels (every row) and the oracle's forward (sampled rows) of one board size"""
    _cache = {}

    def __init__(self, n):
        self.tensors = oa.weights.init_random(n, seed=WEIGHT_SEED)
        self.f32 = oa.Engine(board_size=n, games=256, max_nodes=16, max_tables=8, max_batch_k=16, net_mode=B.NET_F32)
        self.f32.load_weights(self.tensors)
        self.oracle = O.Net(n, self.tensors)

    @classmethod
    def of(cls, n):
        if n not in cls._cache:
            cls._cache[n] = cls(n)
        return cls._cache[n]

    def f32_rows(self, x):
        p, v = self.f32.evaluate_pv(x)
        lg, vp = self.f32.evaluate_logits(x)
        return p.reshape(len(x), -1), v.reshape(-1), lg, vp

    def oracle_rows(self, x):
        return self.oracle.forward_logits(x, threads=8)


def _worst(got, ref):
    """max |difference| of (p, v, logits, vpre); a NaN anywhere makes the figure NaN (and the assertion below fail)"""
    return [float(np.max(np.abs(np.asarray(g, dtype=np.float64).reshape(np.shape(r)) - r))) if np.size(r) else 0.0 for g, r in zip(got, ref)]


def _group(points):
    out = {}
    for p in points:
        for mode in p["modes"]:
            out.setdefault((p["board"], p["k"], p["games"], mode), []).append(p)
    return out


_ENGINES = _group(LAUNCH_SHAPE_LADDER)


def _rows_extend_their_live_games(occ, occ_live, live_games, k):
    """The request list is dense and in game order, at most K rows per live game: every row's stones contain the position of the live game it
    belongs to -- no row comes from a dead game's tree."""
    nreq = len(occ)
    if nreq == len(live_games) * k:
        owner = live_games[np.arange(nreq) // k]
        assert np.all(occ[occ_live[owner]]), "a request row does not extend the position of its live game"
        return
    j, cnt = 0, 0
    for r in range(nreq):
        while cnt == k or np.any(occ_live[live_games[j]] & ~occ[r]):
            j, cnt = j + 1, 0
            assert j < len(live_games), f"request row {r} extends no live game's position"
        cnt += 1


@pytest.mark.parametrize("board,k,games,mode", sorted(_ENGINES))
def test_rounds_at_set_live_counts_against_the_fp32_kernels_and_the_oracle(board, k, games, mode):
    refs = _Refs.of(board)
    hw = board * board
    eng = oa.Engine(board_size=board, games=games, max_nodes=128, max_tables=64, max_batch_k=k, seed=3, net_mode=MODES[mode])
    eng.load_weights(refs.tensors)
    fmt = B.FC0_FORMATS[int(eng.stats()["fc0_format"])]
    sp = oa.SelfPlay(eng)
    rng = np.random.default_rng(7)
    failures = []
    for pt in _ENGINES[(board, k, games, mode)]:
        live, cache = pt["live"], pt["cache"]
        t0 = time.time()
        actions, doomed, want = scripted_finish(board, games, live, 1, pt["winner"], pt["pattern"])
        eng.set_base_cache(cache)
        sp.reset()
        for row in actions:
            sp.play_actions(row)
        alive, status, plies = sp.game_info()
        assert np.array_equal(alive != 0, ~doomed) and np.all(status[doomed] == want) and sp.alive_count == live, "the script did not set the live count"
        side = sp.ply & 1
        assert side == (1 if pt["winner"] == "black" else 0)
        live_games = np.flatnonzero(~doomed)
        occ_live = np.zeros((games, hw), dtype=bool)
        for row in actions:
            occ_live[np.arange(games), row] = True
        dead3 = [int(g) for g in np.flatnonzero(doomed)[[0, len(np.flatnonzero(doomed)) // 2, -1]]] if doomed.any() else []
        worst_f32, worst_orc, plans = [0.0] * 4, [0.0] * 4, []
        for rnd in range(ROUNDS):
            roots = [sp.tree_root(g, s)[0] for g in dead3 for s in (0, 1)]
            before = eng.stats()
            nreq = sp.round_generate(rnd, k)
            x = sp.round_inputs().copy()
            p, v = sp.round_eval()
            p, v = np.array(p).reshape(nreq, -1), np.array(v).reshape(-1)
            lg, vp = sp.round_logits()
            plan = eng.last_plan()
            sp.round_scatter()
            after = eng.stats()
            assert [sp.tree_root(g, s)[0] for g in dead3 for s in (0, 1)] == roots, "the tree of a dead game changed"
            assert 0 < nreq <= live * k and plan["rows"] == live * k and plan["path"] in ("copy", "difference")
            occ = x[:, : 2 * hw].reshape(nreq, hw, 2).sum(axis=2) > 0
            # a simulation that ends on a terminal node asks for no evaluation (a child that completes a five): the round then has that many rows fewer
            terminal = int(round((after["sims"] - before["sims"]) - (after["evals"] - before["evals"])))
            assert after["sims"] - before["sims"] == live * k and nreq == live * k - terminal, (nreq, live * k, terminal)
            if rnd > 0:
                assert terminal <= max(2, live * k // 50), "a sibling round of live x K rows (less the few terminal hits)"
                _rows_extend_their_live_games(occ, occ_live, live_games, k)
                assert np.all(occ.sum(axis=1) > len(actions))
                assert plan["runs"] * 3 <= plan["run_rows"] and plan["singles"] + plan["run_rows"] == nreq
            f = _worst((p, v, lg, vp), refs.f32_rows(x))
            pick = rng.choice(nreq, size=min(ORACLE_ROWS, nreq), replace=False)
            o = _worst((p[pick], v[pick], lg[pick], vp[pick]), refs.oracle_rows(x[pick]))
            worst_f32 = [max(a, b) if b == b else b for a, b in zip(worst_f32, f)]
            worst_orc = [max(a, b) if b == b else b for a, b in zip(worst_orc, o)]
            plans.append(plan)
            _RECORDED.append(((board, k, games, mode, fmt), pt, rnd, side, plan))
            line = (f"launch-shape board {board} K {k} G {games} {mode}({fmt}) L {live} cache {int(cache)} {'white' if side else 'black'}-to-move "
                    f"round {rnd} rows {nreq}: {plan_text(plan)} | vs fp32 dp {f[0]:.1e} dv {f[1]:.1e} dlogit {f[2]:.1e} dvpre {f[3]:.1e} | "
                    f"vs oracle ({len(pick)} rows) {o[0]:.1e} {o[1]:.1e} {o[2]:.1e} {o[3]:.1e}")
            print(line, flush=True)
            if not all(d < TOL for d in f + o):
                failures.append(line)
        print(f"launch-shape point board {board} G {games} {mode} L {live}: worst vs fp32 {max(worst_f32):.2e}, vs oracle {max(worst_orc):.2e}, "
              f"{time.time() - t0:.1f} s (file so far {time.time() - _T0:.0f} s)", flush=True)
    eng.close()
    assert not failures, "rounds outside 1e-3:\n" + "\n".join(failures)


def _classes(plans):
    """the planner classes a set of plans covers"""
    c = set()
    for pl in plans:
        c.add(("path", pl["path"]))
        c.add(("tsplit", pl["tsplit"]))
        if pl["path"] in ("plain", "copy"):
            ns = pl["nsplit"]
            c.add(("nsplit", "1" if ns == 1 else "2-8" if ns <= 8 else "9-49" if ns <= 49 else ">=50"))
            if pl["nsup"] % ns:
                c.add(("nsplit", "uneven"))
        if pl["path"] == "difference":
            tiles, ts, ways, fw = pl["tiles"], pl["t_split"], pl["ways"], pl["fways"]
            if ts == 0 and ways >= 2:
                c.add(("window", "all-split"))
            elif ways == 1:
                assert ts == tiles
                c.add(("window", "whole-K"))
            elif 0 < ts < tiles:
                c.add(("window", "partial 2-4" if ways <= 4 else "partial 5-9" if ways <= 9 else "partial >=10"))
                if ts % pl["n_cu"]:
                    c.add(("window", "t_split moved down"))
            c.add(("fways", "1" if fw == 1 else "2-8" if fw <= 8 else "9-63" if fw <= 63 else "64"))
    return c


def test_the_recorded_plans_cover_the_planner_classes():
    """Runs after the ladder (same session): what the checked rounds covered.  A class leaves this list only where no live count reaches it
    (reason beside it), never because it fails."""
    keys = {key for key, *_ in _RECORDED}
    assert len(keys) == len(_ENGINES), "run the whole file: the ladder tests record the plans"
    for fmt in ("fp6", "f16", "mixed"):
        got = _classes([pl for key, _, _, _, pl in _RECORDED if key[4] == fmt])
        assert {("path", "copy"), ("path", "difference")} <= got, (fmt, sorted(got))
    assert any(key[3] == "default" and pl["path"] == "copy" for key, _, _, _, pl in _RECORDED)
    assert any(key[3] == "default" and pl["path"] == "difference" for key, _, _, _, pl in _RECORDED)
    got = _classes([pl for *_, pl in _RECORDED])
    want = {("tsplit", 1), ("tsplit", 2), ("tsplit", 4), ("tsplit", 8),
            # dense fc0 of sibling rounds = the copy path = at most 3071 rows (24 tiles; board 9: 1023 rows): nsplit >= 10 there.  nsplit 1 and 2-8 are
            # asserted on plain rows below, which take the same planner.
            ("nsplit", "9-49"), ("nsplit", ">=50"), ("nsplit", "uneven"),
            ("window", "all-split"), ("window", "whole-K"), ("window", "partial 2-4"), ("window", "partial 5-9"), ("window", "partial >=10"),
            ("window", "t_split moved down"),
            # fways 64 cannot be reached: the no-empty-split rule takes 64 ways down to 57 (450 super-steps: 63 x 8 >= 450) and to 54 at board 9
            # (162 super-steps) -- the scan shows 57 / 54 wherever one tile of full rows meets a large slab (profiles/r09_launch_shapes.log)
            ("fways", "1"), ("fways", "2-8"), ("fways", "9-63")}
    assert max(pl["fways"] for *_, pl in _RECORDED if pl["path"] == "difference") >= 54  # (the cap the rule leaves)
    assert want <= got, sorted(want - got)
    assert {side for _, _, _, side, _ in _RECORDED} == {0, 1}, "checked rounds with black and with white to move"
    for board in (9, 15):
        assert {pl["path"] for key, _, _, _, pl in _RECORDED if key[0] == board} == {"copy", "difference"}, board
    print(f"launch-shape ladder: {len(_RECORDED)} checked rounds, classes {sorted(got, key=str)}; file so far {time.time() - _T0:.0f} s")


# ---- plain rows (omok_evaluate_pv, mirror and root evaluations) under the same planners ----------------------------------------------
PLAIN_TILES = list(range(1, 41)) + [48, 64, 65, 96, 128, 129, 137, 200, 255, 256, 257]
# Tile counts that also run on an engine of their own capacity (128 x tiles rows: the partial slab is max(8 x capacity, 32768) rows instead of the
# 4096-game engine's 524288, which caps nsplit at 8 from 33 tiles on and tsplit by the same rule).  Creating an engine costs ~1 s (the fc0 weights
# are packed on the host), so the tile counts whose plan under the small slab repeats a neighbour's class are left to the large engine alone.
OWN_TILES = (1, 2, 3, 5, 6, 8, 13, 16, 24, 32, 33, 40, 48, 65, 129, 257)


def _plain_counts(t):
    return (128 * t, 128 * t - 1 if t % 2 else 128 * t - 127)  # a full last tile; one row short of it / one row in it


@pytest.mark.parametrize("mode", ["fp6", "f16"])
@pytest.mark.parametrize("board", [15, 9])
def test_plain_rows_at_every_tile_count_are_position_independent_and_right(board, mode):
    """400 base positions tiled to B rows, B covering every tile count 1..40 and {48 .. 257} tiles (full last tile, and B - 1 or B - 127 rows), on a
    4096-game engine and (OWN_TILES) on an engine whose capacity is that many tiles: every copy of a base row inside one launch is bit-identical to the first copy, the first 400
    rows are within 1e-3 of the fp32 kernels and the oracle on p, v and the logits."""
    refs = _Refs.of(board)
    hw, k, nb = board * board, 16, 400
    base = random_positions(board, nb, 11)
    ref_f32 = refs.f32_rows(base)
    ref_orc = refs.oracle_rows(base)
    big = oa.Engine(board_size=board, games=4096, max_nodes=16, max_tables=8, max_batch_k=k, net_mode=MODES[mode])
    big.load_weights(refs.tensors)
    failures, t0 = [], time.time()
    for tiles in PLAIN_TILES:
        engines = [(big, 4096 * k)]
        if tiles in OWN_TILES:
            own = oa.Engine(board_size=board, games=128 * tiles // k, max_nodes=16, max_tables=8, max_batch_k=k, net_mode=MODES[mode])
            own.load_weights(refs.tensors)
            engines.append((own, 128 * tiles))
        for rows in _plain_counts(tiles):
            first = np.arange(rows) % nb
            x, m = base[first], min(rows, nb)
            for eng, cap in engines:
                p, v = eng.evaluate_pv(x)
                plan_pv = eng.last_plan()
                lg, vp = eng.evaluate_logits(x)
                plan = eng.last_plan()
                assert plan == plan_pv and plan["path"] == "plain" and plan["rows"] == rows
                p, v = p.reshape(rows, -1), v.reshape(-1)
                _PLAIN.append((board, mode, cap, rows, plan))
                same = all(np.array_equal(a.view(np.uint32), a[first].view(np.uint32)) for a in (p, v, lg, vp))
                f = _worst((p[:m], v[:m], lg[:m], vp[:m]), [r[:m] for r in ref_f32])
                o = _worst((p[:m], v[:m], lg[:m], vp[:m]), [r[:m] for r in ref_orc])
                line = (f"plain rows board {board} {mode} engine rows {cap} B {rows}: {plan_text(plan)} | copies identical {same} | vs fp32 "
                        f"{f[0]:.1e} {f[1]:.1e} {f[2]:.1e} {f[3]:.1e} | vs oracle {o[0]:.1e} {o[1]:.1e} {o[2]:.1e} {o[3]:.1e}")
                print(line, flush=True)
                if not same or not all(d < TOL for d in f + o):
                    failures.append(line)
        for eng, _ in engines[1:]:
            eng.close()
    big.close()
    print(f"plain rows board {board} {mode}: {time.time() - t0:.1f} s (file so far {time.time() - _T0:.0f} s)")
    assert not failures, "plain-row launches outside the contract:\n" + "\n".join(failures)
    got = _classes([pl for b, m_, _, _, pl in _PLAIN if b == board and m_ == mode])
    want = {("tsplit", 1), ("tsplit", 2), ("tsplit", 4), ("tsplit", 8), ("nsplit", "1"), ("nsplit", "2-8"), ("nsplit", "9-49"), ("nsplit", ">=50"),
            ("nsplit", "uneven")}
    assert want <= got, sorted(want - got)
