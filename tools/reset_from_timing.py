"""omok_selfplay_reset_from beside omok_selfplay_reset at G = 4096, N = 15: HIP-event kernel time (the engine's own per-category events) and
the wall-clock time of the blocking call (`python tools/reset_from_timing.py [--match] [OUT.txt]`).  --match: the same for
omok_match_reset_from beside omok_match_reset (two random-init nets), and k_random_positions at 4096 positions of 8 and of 100 stones."""
import os
import sys
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # (positions.quiet: the boards)
import omok_ai_amd as oa
import positions as P

args = [a for a in sys.argv[1:] if a != "--match"]
match = "--match" in sys.argv[1:]
n, games, k = 15, 4096, 16
eng = oa.Engine(board_size=n, games=games, max_nodes=64, max_tables=16, max_batch_k=k, seed=1)
eng.load_random_weights(0)
if match:
    eng.load_weights2(oa.weights.init_random(n, seed=1))
sp = oa.SelfPlay(eng)
boards = P.quiet(n, games, 8, seed=1)
eng.set_profiling(1)
KEYS = ("ms_trunk", "ms_fc0", "ms_tail", "ms_ply")
out = []


def timed(name, call, ply_label):
    for _ in range(3):
        call()
    wall, ev = [], []
    for _ in range(9):
        eng.reset_stats()
        t = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t) * 1e3)
        st = eng.stats()
        ev.append({kk: st[kk] for kk in KEYS})
    med = {kk: float(np.median([e[kk] for e in ev])) for kk in KEYS}
    line = (f"{name}: wall-clock of the blocking call median {np.median(wall):.3f} ms (min {min(wall):.3f}, max {max(wall):.3f}); HIP events, median: "
            f"net forward {med['ms_trunk'] + med['ms_fc0'] + med['ms_tail']:.3f} ms (trunk {med['ms_trunk']:.3f}, fc0 {med['ms_fc0']:.3f}, tail {med['ms_tail']:.3f}), "
            f"{ply_label} {med['ms_ply']:.3f} ms")
    print(line)
    out.append(line)


if match:
    split = games // 2
    timed("omok_match_reset", lambda: sp.match_reset(split), "encode + k_reset_from")
    timed("omok_match_reset_from", lambda: sp.match_reset_from(split, boards), "encode + k_reset_from")
    for stones in (8, 100):
        timed(f"omok_env_random_positions, {games} positions of {stones} stones", lambda: eng.env_random_positions(1, 0, stones, games), "k_random_positions")
else:
    timed("omok_selfplay_reset", sp.reset, "encode + k_reset_from")
    timed("omok_selfplay_reset_from", lambda: sp.reset_from(boards), "encode + k_reset_from")
if args:
    open(args[0], "w").write("\n".join(out) + "\n")
eng.close()
