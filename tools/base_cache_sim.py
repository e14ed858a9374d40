#!/usr/bin/env python3
"""tools/base_cache_sim.py N G PLIES [SIMS] [K] [SEED]: the base cache of the sibling rounds without a GPU.

Plays PLIES plies of G games on the oracle with the oracle's own forward (random-init net, weight seed 0), reads every round's runs
of sibling requests (request_info + the parent column of tree_dump; a run qualifies at SIB_MIN = 3 rows) and replays them through the
slot policy of k_group (net_kernels.hip), restated below in `slot_policy`.  Prints, per policy -- the first run only (the rule before
the second run got a slot) and the first two runs, with 2 and 4 slots per game -- the runs, the runs evaluated in full, the second
runs and how many second-run leaves were found in a slot by the tree's first run of the following round.

`qualifying_runs`, `slot_policy` and `BaseCacheModel` are what tests/test_gpu_base_cache.py compares the engine's counter with."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIB_MIN = 3


def qualifying_runs(parents):
    """parents: the parent node of every request of ONE tree in one round, in request order.  -> [(parent, first index, length)] of the
    runs (maximal stretches of adjacent requests with one parent) that are at least SIB_MIN long."""
    runs, i = [], 0
    while i < len(parents):
        j = i
        while j < len(parents) and parents[j] == parents[i]:
            j += 1
        if j - i >= SIB_MIN:
            runs.append((int(parents[i]), i, j - i))
        i = j
    return runs


def slot_policy(tags, leaves, ways=2, two_runs=True):
    """k_group's base-slot rule for one tree and one round.
    tags: [(leaf, way)] of the game's slots, most recently used first (at most `ways` entries); leaves: the parents of the tree's
    qualifying runs in request order.  -> (new tags, outcome per run): "hit" (the leaf's base is in a slot), "miss" (evaluated into a
    slot), "shared" (the second run has the first run's leaf: one base serves both), "uncacheable" (evaluated, no slot of the game)."""
    if not leaves:
        return list(tags), []
    cached = 2 if two_runs and len(leaves) > 1 else 1
    out = ["uncacheable"] * len(leaves)
    first, second = leaves[0], leaves[1] if cached == 2 else None
    if second == first:
        out[1], second = "shared", None
    way_of = dict(tags)
    w = {leaf: way_of.get(leaf) for leaf in (first, second) if leaf is not None}  # both lookups come before any victim is chosen
    for leaf in (first, second):
        if leaf is None:
            continue
        if w[leaf] is not None:
            out[leaves.index(leaf)] = "hit"
            continue
        taken = {x for x in w.values() if x is not None}
        never_used = [x for x in range(ways) if x not in way_of.values() and x not in taken]
        lru = [way for _, way in tags if way not in taken]
        w[leaf] = never_used[0] if never_used else lru[-1]
        out[leaves.index(leaf)] = "miss"
    front = [(leaf, w[leaf]) for leaf in (second, first) if leaf is not None]  # the leaf the tree expands now comes first
    rest = [(leaf, way) for leaf, way in tags if way not in w.values()]
    return (front + rest)[:ways], out


class BaseCacheModel:
    """The tags of every game under one policy, and the totals the tool prints."""

    def __init__(self, ways=2, two_runs=True):
        self.ways, self.two_runs = ways, two_runs
        self.tags = {}
        self.pending = {}  # game -> the leaf of the last round's second run
        self.runs = self.full = self.second_runs = self.second_followed = self.second_reused = self.tree_rounds = 0

    def clear(self):
        """the trees changed (reset, advance): no cached base is valid"""
        self.tags.clear()
        self.pending.clear()

    def round(self, per_game):
        """per_game: {game: parents of its side-to-move tree's requests in request order}.  -> runs evaluated in full this round"""
        full = 0
        for g, parents in per_game.items():
            leaves = [r[0] for r in qualifying_runs(parents)]
            if not leaves:
                continue
            self.tree_rounds += 1
            self.tags[g], out = slot_policy(self.tags.get(g, []), leaves, self.ways, self.two_runs)
            if g in self.pending:  # the second run of the round before: is its leaf this round's first run, and was its base kept?
                leaf = self.pending.pop(g)
                if leaf == leaves[0]:
                    self.second_followed += 1
                    self.second_reused += out[0] == "hit"
            if len(leaves) > 1:
                self.second_runs += 1
                self.pending[g] = leaves[1]
            self.runs += len(leaves)
            full += sum(o in ("miss", "uncacheable") for o in out)
        self.full += full
        return full

    def line(self, name):
        return (f"{name:34s} tree-rounds {self.tree_rounds:7d} runs {self.runs:7d} full {self.full:6d} ({100.0 * self.full / max(self.runs, 1):5.1f} %)  "
                f"second runs {self.second_runs:5d}, first run of the next round {self.second_followed:5d}, of them reused {self.second_reused:5d}")


POLICIES = (("first run only, 2 slots", 2, False), ("first run only, 4 slots", 4, False), ("first two runs, 2 slots", 2, True), ("first two runs, 4 slots", 4, True))


def oracle_parents(osp, nreq, side):
    """{game: parents of its requests in request order} of the round the oracle has just generated"""
    info = [osp.request_info(r) for r in range(nreq)]
    per_game, parent_col = {}, {}
    for g, node in info:
        if g not in parent_col:
            parent_col[g] = osp.tree_dump(g, side)[0][:, 0]
        per_game.setdefault(g, []).append(int(parent_col[g][node]))
    return per_game


def main(argv):
    from oracle import oracle as O
    import omok_ai_amd.weights as W
    n, games, plies = int(argv[1]), int(argv[2]), int(argv[3])
    sims = int(argv[4]) if len(argv) > 4 else (800 if n == 15 else 200)
    k = int(argv[5]) if len(argv) > 5 else 16
    seed = int(argv[6]) if len(argv) > 6 else 0
    threads = min(16, os.cpu_count() or 1)
    cap = 4 * sims + 1024
    tensors = W.init_random(n, seed=0)
    net = O.Net(n, tensors)
    osp = O.SelfPlay(n, games, cap_nodes=cap, cap_tables=cap // 2, seed=seed)
    osp.reset(net.forward(O.Environment(n).encode_nn_input(0)[None])[0][0])
    models = [(name, BaseCacheModel(ways, two)) for name, ways, two in POLICIES]
    for ply in range(plies):
        for _, m in models:
            m.clear()
        for rnd in range((sims + k - 1) // k):
            x = osp.round_generate(rnd, k, 0.25, 0.03)
            per_game = oracle_parents(osp, len(x), ply & 1)
            for _, m in models:
                m.round(per_game)
            p, v = net.forward(x, threads=threads)
            osp.round_scatter(p, v)
        osp.sample(1.0, 30)
        osp.advance(net.forward(osp.mirror_generate(), threads=threads)[0])
        print(f"ply {ply}: " + "; ".join(f"{name}: {m.full}/{m.runs}" for name, m in models), flush=True)
    print(f"N = {n}, {games} games x {plies} plies, {sims} simulations per move, K = {k}, tags cleared every ply")
    for name, m in models:
        print(m.line(name))


if __name__ == "__main__":
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    main(sys.argv)
