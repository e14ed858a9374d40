"""The defending scripted player OMOK_OPP_GUARD beside OMOK_OPP_VCF at 4096 games of 15 x 15 (`python tools/guard_timing.py [OUT.txt]`): search-free
episodes in which both sides move through omok_opponent_actions + omok_advance, as tools/versus_bench.py --scripted-vs plays them -- guard against
vcf and against threat with either colour, and vcf against threat beside them.  Per episode: the wall-clock time of the whole loop, the plies,
milliseconds per ply, and the results by colour.  For the first episode (guard Black, vcf White) the move log is on: every position in front of a
guard move is replayed on the host and given to omok_env_guard_scan with the game's own draw word (the oracle's Philox), which must return the
recorded move; its step_out gives the share of guard moves per step of the rule, and the flagged share per ply says how many waves of the map
pass had work.  A measurement, no gate."""
import ctypes as C
import os
import sys
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import omok_ai_amd as oa
from omok_ai_amd import binding as B
from oracle import oracle as O

n, games, seed = 15, 4096, 1
eng = oa.Engine(board_size=n, games=games, max_nodes=256, max_tables=64, max_batch_k=16, seed=seed)
eng.load_random_weights(0)  # (advance evaluates the new roots)
sp = oa.SelfPlay(eng)
out = []


def say(line):
    print(line, flush=True)
    out.append(line)


def episode(black, white, log=False):
    kinds = (B.SCRIPTED_PLAYERS[black], B.SCRIPTED_PLAYERS[white])
    sp.game_log(log)
    sp.reset()
    t = time.perf_counter()
    while sp.alive_count > 0:
        sp.opponent_actions(kinds[sp.ply & 1])
        sp.advance()
    ms = (time.perf_counter() - t) * 1e3
    _alive, status, plies = sp.game_info()
    res = [int((status == s).sum()) for s in (oa.api.BLACK_WIN, oa.api.WHITE_WIN, oa.api.DRAW)]
    say(f"{black} (Black) against {white} (White): {ms:.1f} ms for {sp.ply} plies, {ms / sp.ply:.2f} ms per ply; black wins {res[0]}, white wins {res[1]}, "
        f"draws {res[2]}; mean plies per game {float(plies.mean()):.2f}")
    return sp.game_records() if log else None


say(f"{games} games of {n} x {n}, seed {seed}, no search: both sides through omok_opponent_actions + omok_advance; one untimed episode first")
sp.reset()
while sp.alive_count > 0:  # warm-up: code objects and clocks
    sp.opponent_actions(B.OPP_VCF if (sp.ply & 1) == 0 else B.OPP_GUARD)
    sp.advance()
rec = episode("guard", "vcf", log=True)  # the engine's episode 1: its draw words are keyed by stream_key(seed, 1)
for black, white in (("vcf", "guard"), ("guard", "threat"), ("threat", "guard"), ("vcf", "threat"), ("guard", "vcf"), ("vcf", "threat")):
    episode(black, white)

# the guard's moves of the logged episode, step by step
word = (C.c_uint32 * 4)()
O.lib().orc_philox(int(O.stream_key(seed, 1)), 0, 0, 0, 4, word)  # (game 0's first move, on the empty board: the draw over all cells)
assert (int(word[0]) * n * n) >> 32 == int(rec.cells[0, 0]), "the logged episode is not the engine's episode 1"
key = O.stream_key(seed, 1)
boards = np.ascontiguousarray(rec.start_boards).copy()
steps = np.zeros(6, dtype=np.int64)
levels = np.zeros((6, 8), dtype=np.int64)
flagged = []
for ply in range(int(rec.lengths.max())):
    live = np.flatnonzero(rec.lengths > ply)
    if (ply & 1) == 0:  # a guard move
        draws = np.zeros(len(live), dtype=np.uint32)
        for i, g in enumerate(live):
            O.lib().orc_philox(int(key), 0, ply, (2 * int(g)) & 0xFFFFFFFF, 4, word)
            draws[i] = word[0]
        got = eng.env_guard_scan(boards[live], np.zeros(len(live), dtype=np.uint8), draws)
        assert np.array_equal(got["cell"], rec.cells[live, ply].astype(np.int32)), f"ply {ply}: the scan does not return the recorded moves"
        steps += np.bincount(got["step"], minlength=6)
        np.add.at(levels, (got["step"], got["level"]), 1)
        flagged.append((ply, len(live), int((got["step"] >= 3).sum())))
    boards[live, rec.cells[live, ply].astype(np.int64)] = 1 + (ply & 1)
total = int(steps.sum())
say(f"guard (Black) against vcf (White), the logged episode: {total} guard moves, every one returned by omok_env_guard_scan with the game's draw word; "
    f"moves per step 0..5: {steps.tolist()} = {[round(100.0 * int(s) / total, 2) for s in steps]} %")
say(f"levels of the restricted rule in steps 3 / 4 (3..7): {levels[3, 3:].tolist()} / {levels[4, 3:].tolist()}; L0 in step 5 (3..7): {levels[5, 3:].tolist()}")
busy = [p for p in flagged if p[2] > 0]
say(f"the map pass had flagged games on {len(busy)} of the guard's {len(flagged)} plies; per such ply on average {np.mean([f for _p, _l, f in busy]):.1f} of "
    f"{np.mean([l for _p, l, _f in busy]):.0f} live games flagged (at most {max(f for _p, _l, f in busy)}): "
    f"{100.0 * sum(f for _p, _l, f in flagged) / sum(l for _p, l, _f in flagged):.2f} % of the map pass's position slots over the episode did a map, the rest "
    f"left after reading the flag ({n * n} waves each)")
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(out) + "\n")
eng.close()
