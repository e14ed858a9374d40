#!/usr/bin/env python3
"""Throughput of an evaluation episode against a scripted player (omok_versus_run: play_against_naive_player, src/trainer.rs:487-603) beside
a self-play episode on the same engine, at the configs[1] size.

Default: 4096 concurrent 15x15 games, 800 simulations per move of the net, K = 16, the naive player as Black (opponent_side = 0), a random-init
net.  A few untimed self-play plies warm clocks and code objects, then one timed versus episode and one timed self-play episode run on fresh RNG
streams.  Prints one JSON line: games/s and game-plies/s of both, the result counts by colour.  `--plies P` stops both episodes after P plies
(the workload of a rocprofv3 --kernel-trace --stats pass: k_opponent_move<N, KIND>, one instantiation per scripted player, beside k_sample / k_mirror_scan /
k_advance).  `--scripted-vs KIND2` adds one episode without any search: `--kind` as Black against KIND2 as White, both moving through
omok_opponent_actions (the strength of one scripted player against another; its counts by colour land under "scripted").

    python tools/versus_bench.py [--games 4096] [--sims 800] [--batch 16] [--kind naive|random|threat|vcf|guard] [--opponent-side 0] [--plies 0] [--no-selfplay]
                                 [--scripted-vs naive|random|threat|vcf|guard]
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--board", type=int, default=15)
    ap.add_argument("--kind", choices=sorted(B.SCRIPTED_PLAYERS), default="naive")
    ap.add_argument("--scripted-vs", choices=sorted(B.SCRIPTED_PLAYERS), default=None, help="one more episode: --kind (Black) against this player (White), no search")
    ap.add_argument("--opponent-side", type=int, default=0)
    ap.add_argument("--plies", type=int, default=0, help="stop the timed episodes after this many plies (0: whole episodes)")
    ap.add_argument("--warmup-plies", type=int, default=2)
    ap.add_argument("--no-selfplay", action="store_true")
    a = ap.parse_args(argv)
    kind = B.SCRIPTED_PLAYERS[a.kind]
    max_nodes = min(16384, 4 * a.sims + 1024)
    eng = oa.Engine(board_size=a.board, games=a.games, max_nodes=max_nodes, max_tables=max(256, max_nodes // 4), max_batch_k=a.batch, seed=1)
    eng.load_random_weights(0)
    sp = oa.SelfPlay(eng)
    sp.reset()
    sp.run(a.sims, a.batch, max_plies=a.warmup_plies)

    def episode(versus):
        eng.reset_stats()
        sp.reset()
        t = time.perf_counter()
        if versus:
            res, st = sp.versus_run(kind, a.opponent_side, a.sims, a.batch, max_plies=a.plies)
        else:
            res, st = None, sp.run(a.sims, a.batch, max_plies=a.plies)
        dt = time.perf_counter() - t
        out = {"seconds": round(dt, 3), "games_per_s": round(st["finished"] / dt, 2), "game_plies_per_s": round(st["ply_games"] / dt, 1),
               "finished": int(st["finished"]), "game_plies": int(st["ply_games"]), "simulations": st["sims"], "evals": st["evals"]}
        if st["finished"]:
            out["mean_plies_per_game"] = round(st["ply_games"] / st["finished"], 3) if a.plies == 0 else None
        if res is not None:
            out.update({"black_win": res[0], "white_win": res[1], "draw": res[2]})
        return out

    out = {"metric": "evaluation games/sec against a scripted player", "unit": "games/s",
           "config": {"games": a.games, "board": a.board, "sims_per_move": a.sims, "batch_k": a.batch, "kind": a.kind, "opponent_side": a.opponent_side,
                      "plies": a.plies},
           "fc0_format": B.FC0_FORMATS[int(eng.stats()["fc0_format"])]}
    out["versus"] = episode(True)
    out["value"] = out["versus"]["games_per_s"]
    if not a.no_selfplay:
        out["selfplay"] = episode(False)
    if a.scripted_vs is not None:
        kinds = (kind, B.SCRIPTED_PLAYERS[a.scripted_vs])
        sp.reset()
        t = time.perf_counter()
        while sp.alive_count > 0 and (a.plies == 0 or sp.ply < a.plies):
            sp.opponent_actions(kinds[sp.ply & 1])
            sp.advance()
        dt = time.perf_counter() - t
        _alive, status, plies = sp.game_info()
        out["scripted"] = {"black": a.kind, "white": a.scripted_vs, "seconds": round(dt, 3), "plies": int(sp.ply),
                           "black_win": int((status == oa.api.BLACK_WIN).sum()), "white_win": int((status == oa.api.WHITE_WIN).sum()),
                           "draw": int((status == oa.api.DRAW).sum()), "mean_plies_per_game": round(float(plies.mean()), 3)}
    eng.close()
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
