"""omok_env_vcf_defend beside omok_env_vcf_solve at 4096 positions of 15 x 15 (`python tools/vcf_defend_timing.py [OUT.txt]`): the positions of
4096 games OMOK_OPP_THREAT against OMOK_OPP_THREAT after PLY plies, played on the device (open threes stand on many of them); per setting
(max_depth, max_nodes) the wall-clock time of the blocking call and the kernel under the engine's HIP events (omok_set_profiling), medians of 9
calls after 3 warm-up calls, the sum of nodes_out and from it a kernel time per node (and, for the solver, per node of its longest wave), and the ratio of the two calls.  A measurement, no gate."""
import os
import sys
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import omok_ai_amd as oa
from omok_ai_amd import binding as B

n, games, PLY = 15, 4096, 24
eng = oa.Engine(board_size=n, games=games, max_nodes=256, max_tables=64, max_batch_k=16, seed=1)
eng.load_random_weights(0)  # (advance evaluates the new roots)
sp = oa.SelfPlay(eng)
sp.game_log(True)
sp.reset()
while sp.alive_count > 0 and sp.ply < PLY:
    sp.opponent_actions(B.OPP_THREAT)
    sp.advance()
rec = sp.game_records()
boards, status, _played = eng.env_replay(rec.start_boards, rec.moves(), rec.lengths, upto=PLY)
turns = (np.count_nonzero(boards, axis=1) & 1).astype(np.uint8)
level = eng.env_threat_scan(boards, turns)[1]
out = [f"{games} positions of {n} x {n}: OMOK_OPP_THREAT against OMOK_OPP_THREAT (seed 1) after {PLY} plies; {int((status == 0).sum())} in progress, "
       f"levels of the threat-aware rule for the side to move: {np.bincount(level, minlength=8).tolist()}"]
print(out[0])
eng.set_profiling(1)


def timed(call):
    for _ in range(3):
        call()
    wall, ev = [], []
    for _ in range(9):
        eng.reset_stats()
        t = time.perf_counter()
        res = call()
        wall.append((time.perf_counter() - t) * 1e3)
        ev.append(eng.stats()["ms_ply"])
    return res, float(np.median(wall)), min(wall), max(wall), float(np.median(ev))


for depth, budget in ((6, 256), (8, 4096)):
    res, w_s, lo, hi, k_s = timed(lambda: eng.env_vcf_solve(boards, turns, depth, budget))
    nodes_s = int(res[3].astype(np.int64).sum())
    line = (f"D {depth} NB {budget}  omok_env_vcf_solve: wall-clock of the blocking call median {w_s:.3f} ms (min {lo:.3f}, max {hi:.3f}); k_env_vcf, HIP events, "
            f"median {k_s:.3f} ms; verdicts -1 / 0 / 1: {[int((res[0] == v).sum()) for v in (-1, 0, 1)]}; nodes {nodes_s}, {k_s * 1e6 / max(nodes_s, 1):.1f} ns of kernel time per node "
            f"({games} waves, all resident at once); the longest wave counted {int(res[3].max())} nodes: at most {k_s * 1e3 / max(int(res[3].max()), 1):.1f} us per node of one wave")
    print(line)
    out.append(line)
    res, w_d, lo, hi, k_d = timed(lambda: eng.env_vcf_defend(boards, turns, depth, budget))
    nodes_d = int(res["nodes"].astype(np.int64).sum())
    line = (f"D {depth} NB {budget}  omok_env_vcf_defend: wall-clock of the blocking call median {w_d:.3f} ms (min {lo:.3f}, max {hi:.3f}); k_env_vcf_defend, HIP events, "
            f"median {k_d:.3f} ms; cells safe / wins / loses / unknown: {[int(res[k].sum()) for k in ('safe', 'wins', 'loses', 'unknown')]}, threats -1 / 0 / 1: "
            f"{[int((res['threat'][:, 0] == v).sum()) for v in (-1, 0, 1)]}; nodes {nodes_d} (the null moves' not among them), {k_d * 1e6 / max(nodes_d, 1):.1f} ns of kernel time per node "
            f"({games * (n * n + 1)} waves)")
    print(line)
    out.append(line)
    line = f"D {depth} NB {budget}  defend / solve: wall-clock {w_d / w_s:.1f} x, kernel {k_d / k_s:.1f} x, nodes {nodes_d / max(nodes_s, 1):.1f} x"
    print(line)
    out.append(line)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(out) + "\n")
eng.close()
