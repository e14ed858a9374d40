"""The yardstick of match episodes (omok_match_reset) built from two unmodified oracle.SelfPlay instances (no GPU, no product code).

oracle.SelfPlay.reset takes ONE root policy for all trees, so one instance cannot hold two nets.  MatchComposition keeps O[0] (reset with
net 1's root policy) and O[1] (net 2's) over the same games, seed and game_offset.  Tree side * G + g belongs to net side ^ (g >= split);
only the trees net X owns are meaningful in O[X].  Its other trees are searched with placeholder p / v (uniform, 0); the RNG streams are
keyed per tree, so they cannot perturb the owned ones.  Moves reach both instances as external moves (set_actions): the mover's tree
plays it after ensure_action_exists (a no-op, the searched move is a child), the other tree after ensure + its mirror row.

Row order of the step-wise interface: requests in game order (the owned trees of the side to move), mirror rows one per live game.
"""
import numpy as np

from oracle import oracle as O


class MatchComposition:
    def __init__(self, n, games, split, root_p1, root_p2, seed=0, game_offset=0, cap_nodes=4096, cap_tables=2048):
        self.n, self.hw, self.games, self.split = n, n * n, games, split
        self.O = [O.SelfPlay(n, games, cap_nodes=cap_nodes, cap_tables=cap_tables, seed=seed, game_offset=game_offset) for _ in range(2)]
        self.O[0].reset(root_p1)
        self.O[1].reset(root_p2)
        self._filler = np.full(self.hw, 1.0 / self.hw, dtype=np.float32)

    def owner(self, g, side):
        """net index (0 = net 1, 1 = net 2) of tree side * G + g"""
        return side ^ (1 if g >= self.split else 0)

    ply = property(lambda s: s.O[0].ply)
    alive_count = property(lambda s: s.O[0].alive_count)
    error = property(lambda s: s.O[0].error | s.O[1].error)

    def game_alive(self, g):
        return self.O[0].game_alive(g)

    def game_status(self, g):
        return self.O[0].game_status(g)

    def tree_dump(self, g, side):
        return self.O[self.owner(g, side)].tree_dump(g, side)

    def tree_root(self, g, side):
        return self.O[self.owner(g, side)].tree_root(g, side)

    # ---- search rounds --------------------------------------------------------------------------
    def round_generate(self, rnd, k, epsilon, alpha):
        """Both instances generate; returns (inputs, games): the owned requests in game order = the engine's request rows."""
        side = self.ply & 1
        self._req = []
        inputs, rows, games = [], [], []
        for x in range(2):
            inp = self.O[x].round_generate(rnd, k, epsilon, alpha)
            gs = np.array([self.O[x].request_info(r)[0] for r in range(len(inp))], dtype=np.int64)
            self._req.append(gs)
            inputs.append(inp)
        for g in range(self.games):
            x = self.owner(g, side)
            sel = np.nonzero(self._req[x] == g)[0]  # (indices into O[x]'s requests)
            rows.append(sel)
            games += [g] * len(sel)
        self._own_rows = rows
        out = [inputs[self.owner(g, side)][rows[g]] for g in range(self.games)]
        return np.concatenate(out), np.array(games, dtype=np.int64)

    def round_scatter(self, p, v):
        """p [rows][HW], v [rows]: the engine's outputs of the round, in its row order"""
        side = self.ply & 1
        p = np.asarray(p, dtype=np.float32).reshape(-1, self.hw)
        v = np.asarray(v, dtype=np.float32).reshape(-1)
        start = np.concatenate([[0], np.cumsum([len(r) for r in self._own_rows])])
        for x in range(2):
            gs = self._req[x]
            px = np.tile(self._filler, (len(gs), 1))
            vx = np.zeros(len(gs), dtype=np.float32)
            for g in range(self.games):
                if self.owner(g, side) != x:
                    continue
                sel = self._own_rows[g]
                px[sel] = p[start[g]:start[g + 1]]
                vx[sel] = v[start[g]:start[g + 1]]
            self.O[x].round_scatter(px, vx)

    # ---- moves ----------------------------------------------------------------------------------
    def compute_policy(self, g):
        side = self.ply & 1
        return self.O[self.owner(g, side)].compute_policy(g)

    def sample(self, temperature, threshold):
        """each game's move from the instance that owns its side-to-move tree"""
        side = self.ply & 1
        acts = [self.O[x].sample(temperature, threshold) for x in range(2)]
        return np.array([acts[self.owner(g, side)][g] for g in range(self.games)], dtype=np.int32)

    def mirror_generate(self, actions):
        """stages the true moves in both instances; returns the mirror boards (one per live game, game order)"""
        m = []
        for x in range(2):
            self.O[x].set_actions(actions)
            m.append(self.O[x].mirror_generate())
        assert np.array_equal(m[0], m[1])
        self._mgames = [g for g in range(self.games) if self.O[0].game_alive(g)]
        return m[0]

    def advance(self, pm):
        """pm [live games][HW]: the engine's mirror rows (game g's row evaluated by the net of g's opponent tree)"""
        side = self.ply & 1
        pm = np.asarray(pm, dtype=np.float32).reshape(-1, self.hw)
        for x in range(2):
            px = np.tile(self._filler, (len(self._mgames), 1))
            for i, g in enumerate(self._mgames):
                if self.owner(g, 1 - side) == x:
                    px[i] = pm[i]
            self.O[x].advance(px)
