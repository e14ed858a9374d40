"""Net-against-net match: what benchmark/src/main.rs:14-108 does with two checkpoints, played as one batched match episode.

    python -c "from omok_ai_amd import match; match.main(['left.bin', 'right.bin', '--games', '4096'])"

Half of the games (games [0, G/2)) have the first net as Black, the other half the second net (main.rs:24-56).  Each agent searches its
own tree with its own net, mirrors the opponent's move with its own net (ensure_action_exists, main.rs:79-82,99-102) and plays the
most visited move (sample_action(Best) with EPSILON = 0, ALPHA = 1: benchmark/src/agent.rs:14-15,34-49).  Prints wins, losses and
draws from the first net's side and returns them with the per-game results.

From the empty board with Best moves the G games of a colour assignment are one game but for the expansion draws.  With an opening book
(--openings FILE.npy, [M][HW] Stone bytes, or --random-openings S: M = games / 2 positions of S random stones made on the device from
--seed) games i and i + M both start from opening i, once with each net as Black (omok_match_reset_from, split = M), and the result is
also counted per opening (paired_tally).
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
    ap.add_argument("--temperature", type=float, default=1.0, help="Boltzmann temperature of those plies; the engine takes 1 / temperature <= 80 (>= 0.0125)")
    ap.add_argument("--max-nodes", type=int, default=0, help="tree arena (0: sized from --sims)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--net-mode", default="NET_F16X3", help="binding constant of the net mode (NET_F16X3, NET_F16X3_ROWS, NET_F32, ...)")
    ap.add_argument("--json", action="store_true", help="print the result as one JSON line as well")
    ap.add_argument("--openings", metavar="FILE.npy", help="opening book [M][HW] Stone bytes (equal stone counts), M = games / 2: each opening is played "
                    "twice, once with each net as Black")
    ap.add_argument("--random-openings", type=int, metavar="S", help="the same with games / 2 random positions of S stones made on the device from --seed")
    ap.add_argument("--save-games", metavar="FILE.npz", help="keep the move log and write every game's record there (python -m omok_ai_amd.records show FILE.npz --game i)")
    return ap.parse_args(argv)


def tally(status, split):
    """W/L/D from the first net's side: it is Black in games [0, split), White in [split, G)."""
    status = np.asarray(status)
    first_black = np.arange(status.size) < split
    wins = int(np.sum(first_black & (status == api.BLACK_WIN)) + np.sum(~first_black & (status == api.WHITE_WIN)))
    losses = int(np.sum(first_black & (status == api.WHITE_WIN)) + np.sum(~first_black & (status == api.BLACK_WIN)))
    draws = int(np.sum(status == api.DRAW))
    return wins, losses, draws


def paired_tally(status, m):
    """(both, one_each, neither, drawn_pairs) over the M openings, from the first net's side: opening i was played as game i (first net Black)
    and as game i + M (first net White).  both / neither: the first net won / lost both games; one_each: one win and one loss (the colour
    decided); drawn_pairs: either game was a draw.  The four sum to M."""
    status = np.asarray(status).reshape(-1)
    assert status.size == 2 * m
    as_black, as_white = status[:m], status[m:]
    drawn = (as_black == api.DRAW) | (as_white == api.DRAW)
    won = (as_black == api.BLACK_WIN).astype(np.int64) + (as_white == api.WHITE_WIN).astype(np.int64)
    return tuple(int(np.sum(~drawn & (won == w))) for w in (2, 1, 0)) + (int(np.sum(drawn)),)


def random_openings(eng, key, stones, count, chunk=None):
    """`count` random openings of `stones` stones (Environment.random_positions under RNG key `key`): consecutive ranges of game ids from 0,
    the positions of games still in progress kept in id order -- the book depends on (key, stones, count) only"""
    chunk = chunk or max(64, 2 * count)
    kept, first = [], 0
    while sum(len(k) for k in kept) < count:
        boards, ok = api.Environment.random_positions(eng, key, first, stones, chunk)
        kept.append(boards[ok == 1])
        first += chunk
    return np.concatenate(kept)[:count]


def run_match(eng, games, sims, batch, threshold=0, temperature=1.0, openings=None, save_games=None, meta=None):
    """One match episode on an engine whose two net slots are loaded; returns (wins, losses, draws, status [G], stats).  openings [M][HW]
    (the engine has games = 2 M): games i and i + M start from opening i, the first net Black in the first half (split = M).  save_games: a
    path = the move log is kept for this episode and the games' records (records.GameRecords, with `meta` and the split) written there."""
    sp = api.SelfPlay(eng)
    split = games // 2
    if save_games is not None:
        sp.game_log(True)
    if openings is None:
        sp.match_reset(split)
    else:
        openings = np.ascontiguousarray(openings, dtype=np.uint8).reshape(-1, eng.hw)
        if games != 2 * len(openings) or eng.games != games:
            raise ValueError(f"{len(openings)} openings need an engine of {2 * len(openings)} games, not {games}")
        sp.match_reset_from(split, np.concatenate([openings, openings]))
    stats = sp.run(sims, batch, epsilon=EPSILON, alpha=ALPHA, temperature=temperature, threshold=threshold)
    alive, status, _ = sp.game_info()
    if alive.any():
        raise RuntimeError(f"{int(alive.sum())} game(s) still in progress after the match")
    w, l, d = tally(status, split)
    if save_games is not None:
        sp.game_records(meta=dict(meta or {}, kind="match", split=split, sims=sims, batch=batch, threshold=threshold)).save(save_games)
        sp.game_log(False)
    return w, l, d, status, stats


def main(argv=None):
    a = parse_args(argv)
    book = a.openings is not None or a.random_openings is not None
    if a.openings is not None and a.random_openings is not None:
        raise SystemExit("--openings and --random-openings exclude each other")
    if book and a.games % 2:
        raise SystemExit("--games must be even with openings: each opening is played once with each net as Black")
    max_nodes = a.max_nodes or min(16384, 4 * a.sims + 1024)
    eng = api.Engine(board_size=a.board, games=a.games, max_nodes=max_nodes, max_tables=max(256, max_nodes // 4), max_batch_k=a.batch,
                     device=a.device, net_mode=getattr(B, a.net_mode), seed=a.seed)
    try:
        eng.load(a.net1)
        eng.load2(a.net2)
        openings = None
        if a.openings is not None:
            openings = np.load(a.openings)
        elif a.random_openings is not None:
            openings = random_openings(eng, a.seed, a.random_openings, a.games // 2)
        meta = {"net1": a.net1, "net2": a.net2, "seed": a.seed, "board": a.board,
                "openings": a.openings if a.openings is not None else (f"random:{a.random_openings}" if a.random_openings is not None else None)}
        w, l, d, status, stats = run_match(eng, a.games, a.sims, a.batch, a.threshold, a.temperature, openings=openings, save_games=a.save_games, meta=meta)
        info = eng.net2_info()
    finally:
        eng.close()
    print(f"Playing {a.games} games ({a.games // 2} with the first net as Black)...")
    print(f"{'':12s}{'wins':>8s}{'losses':>8s}{'draws':>8s}")
    print(f"{'first net':12s}{w:8d}{l:8d}{d:8d}")
    print(f"{'second net':12s}{l:8d}{w:8d}{d:8d}")
    paired = paired_tally(status, a.games // 2) if book else None
    if paired is not None:
        print(f"{a.games // 2} openings, each played with both colours: the first net won both games of {paired[0]}, one of {paired[1]}, "
              f"neither of {paired[2]}; {paired[3]} with a draw")
    result = {"games": a.games, "wins": w, "losses": l, "draws": d, "status": [int(s) for s in status],
              "fc0_format": [B.FC0_FORMATS[int(stats["fc0_format"])], info["fc0_format"]], "evals": list(info["evals"])}
    if paired is not None:
        result["paired"] = dict(zip(("both", "one_each", "neither", "drawn_pairs"), paired))
    if a.json:
        print(json.dumps({k: v for k, v in result.items() if k != "status"}))
    return result


if __name__ == "__main__":
    main()
