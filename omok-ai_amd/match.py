"""Net-against-net match: what benchmark/src/main.rs:14-108 does with two checkpoints, played as one batched match episode.

    python -c "from omok_ai_amd import match; match.main(['left.bin', 'right.bin', '--games', '4096'])"

Half of the games (games [0, G/2)) have the first net as Black, the other half the second net (main.rs:24-56).  Each agent searches its
own tree with its own net, mirrors the opponent's move with its own net (ensure_action_exists, main.rs:79-82,99-102) and plays the
most visited move (sample_action(Best) with EPSILON = 0, ALPHA = 1: benchmark/src/agent.rs:14-15,34-49).  Prints wins, losses and
draws from the first net's side and returns them with the per-game results.
"""
import argparse
import json

import numpy as np

from . import api
from . import binding as B

EPSILON, ALPHA = 0.0, 1.0  # benchmark/src/agent.rs:14-15


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="net 1 against net 2 (benchmark/src/main.rs)")
    ap.add_argument("net1", help="weights file of the first net (ModelIO format)")
    ap.add_argument("net2", help="weights file of the second net")
    ap.add_argument("--games", type=int, default=100, help="games in all (main.rs GAME_COUNT); the first net is Black in the first half")
    ap.add_argument("--sims", type=int, default=800, help="simulations per move (main.rs MCTS_COUNT)")
    ap.add_argument("--batch", type=int, default=8, help="simulations per tree and round (main.rs MCTS_BATCH_SIZE)")
    ap.add_argument("--board", type=int, default=15, choices=(9, 15))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--threshold", type=int, default=0, help="plies played with temperature sampling before Best (0: Best throughout, as main.rs)")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--max-nodes", type=int, default=0, help="tree arena (0: sized from --sims)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--net-mode", default="NET_F16X3", help="binding constant of the net mode (NET_F16X3, NET_F16X3_ROWS, NET_F32, ...)")
    ap.add_argument("--json", action="store_true", help="print the result as one JSON line as well")
    return ap.parse_args(argv)


def tally(status, split):
    """W/L/D from the first net's side: it is Black in games [0, split), White in [split, G)."""
    status = np.asarray(status)
    first_black = np.arange(status.size) < split
    wins = int(np.sum(first_black & (status == api.BLACK_WIN)) + np.sum(~first_black & (status == api.WHITE_WIN)))
    losses = int(np.sum(first_black & (status == api.WHITE_WIN)) + np.sum(~first_black & (status == api.BLACK_WIN)))
    draws = int(np.sum(status == api.DRAW))
    return wins, losses, draws


def run_match(eng, games, sims, batch, threshold=0, temperature=1.0):
    """One match episode on an engine whose two net slots are loaded; returns (wins, losses, draws, status [G], stats)."""
    sp = api.SelfPlay(eng)
    split = games // 2
    sp.match_reset(split)
    stats = sp.run(sims, batch, epsilon=EPSILON, alpha=ALPHA, temperature=temperature, threshold=threshold)
    alive, status, _ = sp.game_info()
    if alive.any():
        raise RuntimeError(f"{int(alive.sum())} game(s) still in progress after the match")
    w, l, d = tally(status, split)
    return w, l, d, status, stats


def main(argv=None):
    a = parse_args(argv)
    max_nodes = a.max_nodes or min(16384, 4 * a.sims + 1024)
    eng = api.Engine(board_size=a.board, games=a.games, max_nodes=max_nodes, max_tables=max(256, max_nodes // 4), max_batch_k=a.batch,
                     device=a.device, net_mode=getattr(B, a.net_mode), seed=a.seed)
    try:
        eng.load(a.net1)
        eng.load2(a.net2)
        w, l, d, status, stats = run_match(eng, a.games, a.sims, a.batch, a.threshold, a.temperature)
        info = eng.net2_info()
    finally:
        eng.close()
    print(f"Playing {a.games} games ({a.games // 2} with the first net as Black)...")
    print(f"{'':12s}{'wins':>8s}{'losses':>8s}{'draws':>8s}")
    print(f"{'first net':12s}{w:8d}{l:8d}{d:8d}")
    print(f"{'second net':12s}{l:8d}{w:8d}{d:8d}")
    result = {"games": a.games, "wins": w, "losses": l, "draws": d, "status": [int(s) for s in status],
              "fc0_format": [B.FC0_FORMATS[int(stats["fc0_format"])], info["fc0_format"]], "evals": list(info["evals"])}
    if a.json:
        print(json.dumps({k: v for k, v in result.items() if k != "status"}))
    return result


if __name__ == "__main__":
    main()
