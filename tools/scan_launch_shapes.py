"""Which launch shape does the net forward take at a given number of live games?  Plays the scripted finishes of tests/helpers.py
(scripted_finish) on one engine for a list of live counts, runs one ply of step-wise rounds and prints the plan of every round
(omok_debug_last_plan): path, row bound, the host's K splits, the window planner's tile count / split set / ways.  No reference is
computed: a few seconds on the GPU.  tests/test_gpu_launch_shapes.py picks its ladder from this output and asserts the classes it
covers; when a change moves the planners and that assertion fails, re-pick the points with this script.
    python tools/scan_launch_shapes.py --games 4096 --mode fp6 --lives 1700:2500:50,4096 [--no-cache] [--winner white]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import omok_ai_amd as oa  # noqa: E402
from omok_ai_amd import binding as B  # noqa: E402
from helpers import plan_text, scripted_finish  # noqa: E402

MODES = {"default": B.NET_F16X3, "fp6": B.NET_F16X3_FP6, "f16": B.NET_F16X3_F16, "mixed": B.NET_F16X3_MIXED}


def lives(text):
    out = []
    for part in text.split(","):
        if ":" in part:
            a, b, c = (int(x) for x in part.split(":"))
            out += list(range(a, b, c))
        else:
            out.append(int(part))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=15)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--mode", default="fp6", choices=sorted(MODES))
    ap.add_argument("--lives", default="4096")
    ap.add_argument("--winner", default="black")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--no-cache", action="store_true", help="omok_debug_set_base_cache(0): every run evaluated in full")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    eng = oa.Engine(board_size=a.board, games=a.games, max_nodes=128, max_tables=64, max_batch_k=a.k, seed=3, net_mode=MODES[a.mode])
    eng.load_random_weights(0)
    eng.set_base_cache(not a.no_cache)
    sp = oa.SelfPlay(eng)
    for live in lives(a.lives):
        if live > a.games:
            continue
        actions, _, _ = scripted_finish(a.board, a.games, live, a.seed, a.winner)
        sp.reset()
        for row in actions:
            sp.play_actions(row)
        assert sp.alive_count == live
        mirror = eng.last_plan()
        print(f"board {a.board} K {a.k} G {a.games} {a.mode} L {live}: last mirror evaluation: {plan_text(mirror)}", flush=True)
        for rnd in range(a.rounds):
            nreq = sp.round_generate(rnd, a.k)
            sp.round_eval()
            plan = eng.last_plan()
            sp.round_scatter()
            print(f"    round {rnd} nreq {nreq}: {plan_text(plan)}", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
