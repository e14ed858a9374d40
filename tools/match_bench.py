#!/usr/bin/env python3
"""Throughput of a match episode (omok_match_reset: net 1 against net 2, benchmark/src/main.rs) at the configs[1] size.

Default: 4096 concurrent 15x15 games, 800 simulations per move, K = 16, two random-init nets (seeds 0 and 1), threshold = 0 (Best
every move), half of the games with each net as Black.  One untimed match warms clocks and code objects, then `--matches` timed
matches run on fresh RNG streams.  Prints one JSON line: games/s, rows evaluated by each net, each net's fc0 operand format, W/L/D.

    python tools/match_bench.py [--games 4096] [--sims 800] [--batch 16] [--matches 2]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import omok_ai_amd as oa  # noqa: E402
from omok_ai_amd import binding as B  # noqa: E402
from omok_ai_amd import match as M  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--board", type=int, default=15)
    ap.add_argument("--matches", type=int, default=2, help="timed matches")
    ap.add_argument("--warmup-plies", type=int, default=4, help="plies of the untimed warm-up match")
    a = ap.parse_args(argv)
    max_nodes = min(16384, 4 * a.sims + 1024)
    t0 = time.perf_counter()
    eng = oa.Engine(board_size=a.board, games=a.games, max_nodes=max_nodes, max_tables=max(256, max_nodes // 4), max_batch_k=a.batch, seed=1)
    eng.load_random_weights(0)
    eng.load_weights2(oa.weights.init_random(a.board, seed=1))
    t_setup = time.perf_counter() - t0
    sp = oa.SelfPlay(eng)
    sp.match_reset(a.games // 2)
    sp.run(a.sims, a.batch, epsilon=M.EPSILON, alpha=M.ALPHA, threshold=0, max_plies=a.warmup_plies)
    eng.reset_stats()
    secs, wld = [], [0, 0, 0]
    for _ in range(a.matches):
        t = time.perf_counter()
        w, l, d, status, stats = M.run_match(eng, a.games, a.sims, a.batch)
        secs.append(time.perf_counter() - t)
        wld = [wld[0] + w, wld[1] + l, wld[2] + d]
    plies = stats["ply_games"]  # (the stats are cumulative since reset_stats: the last match's figure covers all timed matches)
    st = eng.stats()
    info = eng.net2_info()
    eng.close()
    games = a.games * a.matches
    out = {"metric": "match games/sec (net 1 vs net 2)", "value": round(games / sum(secs), 2), "unit": "games/s",
           "config": {"games": a.games, "board": a.board, "sims_per_move": a.sims, "batch_k": a.batch, "threshold": 0, "matches": a.matches},
           "s_per_match": [round(s, 3) for s in secs], "mean_plies_per_game": round(plies / games, 3), "game_plies_per_s": round(plies / sum(secs), 1),
           "evals_net1": info["evals"][0], "evals_net2": info["evals"][1], "evals_total": st["evals"],
           "fc0_format_net1": B.FC0_FORMATS[int(st["fc0_format"])], "fc0_format_net2": info["fc0_format"],
           "probe_outside": [int(st["probe_outside"]), info["probe_outside"]],
           "net1_wins": wld[0], "net1_losses": wld[1], "draws": wld[2], "setup_s": round(t_setup, 2)}
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
