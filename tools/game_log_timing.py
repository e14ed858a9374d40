"""What the move log costs (`python tools/game_log_timing.py [OUT.txt] [--games G] [--sims S]`): configs[1]-sized self-play episodes (4096 games,
15 x 15, 800 simulations, K = 16) with the log off and on, alternating in one process on one engine -- 2 warm-up episodes, then 3 pairs -- as
games/s and as OMOK_STAT_MS_PLY (the ply-level kernels under HIP events: a second pass of 4 plies per setting with omok_set_profiling, so the
events do not sit in the timed episodes); then the read-back of all games (omok_game_log_read through SelfPlay.game_records) and
omok_env_replay of those records, wall clock of the blocking call and k_replay under the engine's HIP events."""
import os
import sys
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import omok_ai_amd as oa


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


games, sims = opt("--games", 4096), opt("--sims", 800)
args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and not sys.argv[i - 1].startswith("--")]
n, k = 15, 16
max_nodes = min(16384, 4 * sims + 1024)
eng = oa.Engine(board_size=n, games=games, max_nodes=max_nodes, max_tables=max(256, max_nodes // 4), max_batch_k=k, seed=1)
eng.load_random_weights(0)
sp = oa.SelfPlay(eng)
out = []


def say(line):
    print(line, flush=True)
    out.append(line)


def episode(log, max_plies=0):
    """one episode from a reset; (seconds, stats of this episode)"""
    sp.game_log(log)
    sp.reset()
    eng.reset_stats()
    t = time.perf_counter()
    st = sp.run(sims, k, max_plies=max_plies)
    return time.perf_counter() - t, st


say(f"{games} games, {n} x {n}, {sims} simulations, K = {k}; log off / on alternating on one engine, 2 warm-up episodes, then 3 pairs")
for log in (False, True):
    episode(log)
rate = {False: [], True: []}
for pair in range(3):
    for log in (False, True):
        dt, st = episode(log)
        rate[log].append(st["finished"] / dt)
        say(f"pair {pair} log {'on ' if log else 'off'}: {st['finished']:.0f} games in {dt:.3f} s = {st['finished'] / dt:.2f} games/s, {st['ply_games']:.0f} game-plies")
for log in (False, True):
    say(f"log {'on ' if log else 'off'}: median {np.median(rate[log]):.2f} games/s (min {min(rate[log]):.2f}, max {max(rate[log]):.2f})")
say(f"on / off, medians: {np.median(rate[True]) / np.median(rate[False]):.4f}")

eng.set_profiling(1)
for log in (False, True):
    ms = []
    for _ in range(3):
        _, st = episode(log, max_plies=4)
        ms.append(st["ms_ply"] / 4)
    say(f"log {'on ' if log else 'off'}: OMOK_STAT_MS_PLY per ply over the first 4 plies (HIP events, all games alive): median {np.median(ms) * 1e3:.1f} us "
        f"(min {min(ms) * 1e3:.1f}, max {max(ms) * 1e3:.1f})")
eng.set_profiling(0)

episode(True)  # whole games to read back
wall = []
for _ in range(5):
    t = time.perf_counter()
    rec = sp.game_records()
    wall.append((time.perf_counter() - t) * 1e3)
say(f"omok_game_log_read + omok_game_info, all {games} games ({rec.lengths.sum()} moves, {19 * games * n * n / 1e6:.1f} MB of log): wall clock median "
    f"{np.median(wall):.2f} ms (min {min(wall):.2f}, max {max(wall):.2f})")
moves = rec.moves()
eng.set_profiling(1)
wall, ev = [], []
for i in range(8):
    eng.reset_stats()
    t = time.perf_counter()
    boards, status, played = eng.env_replay(rec.start_boards, moves, rec.lengths)
    wall.append((time.perf_counter() - t) * 1e3)
    ev.append(eng.stats()["ms_ply"])
wall, ev = wall[3:], ev[3:]
assert np.array_equal(played, rec.lengths) and np.array_equal(status, rec.status)
say(f"omok_env_replay of those {games} records (mean length {rec.lengths.mean():.1f}): k_replay under HIP events median "
    f"{np.median(ev) * 1e3:.1f} us (min {min(ev) * 1e3:.1f}, max {max(ev) * 1e3:.1f}); wall clock of the blocking call median {np.median(wall):.2f} ms")
if args:
    open(args[0], "w").write("\n".join(out) + "\n")
eng.close()
