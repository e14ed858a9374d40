"""Game records: every move of an episode with what the mover's search knew of it, replayable.

The reference keeps a Transition for the moves its trainer sampled (src/trainer.rs:169-173) and only counts the results of its evaluation
games and matches (trainer.rs:400-603, benchmark/src/main.rs:60-105).  A GameRecords holds what the engine's move log kept of a batch of games
(SelfPlay.game_log / game_records; include/omok_mi355x.h "game records"): the start position, every move with its `external` flag, and the
root and chosen-child statistics of the mover's tree at the moment of the move.  Replaying goes through the engine's rules kernel
(Engine.env_replay), never through a restatement of the rules here.

    python -m omok_ai_amd.records show FILE.npz --game 3
    python -m omok_ai_amd.records tactics FILE.npz
    python -m omok_ai_amd.records forced FILE.npz
    python -m omok_ai_amd.records defence FILE.npz --max-depth 8 --max-nodes 4096
"""
import argparse
import json

import numpy as np

CELL_MASK, EXTERNAL = 0xFF, 0x100  # OMOK_MOVE_CELL, OMOK_MOVE_EXTERNAL
STATUS_NAMES = {0: "in progress", 1: "draw", 2: "black wins", 3: "white wins"}
ENTRY_BYTES = 20  # omok_game_log_entry_bytes: root_n u32, root_w f32, child_n u32, child_w f32, move u16, zero u16 (little-endian)
_ARRAYS = ("start_boards", "lengths", "cells", "external", "root_n", "root_w", "child_n", "child_w", "status", "plies")


class GameRecords:
    """board size n; per game g: start_boards [G][HW] Stone bytes, lengths [G] moves since the start, cells int16 [G][HW] (-1 beyond the
    length), external bool [G][HW], root_n uint32 / root_w float32 / child_n uint32 / child_w float32 [G][HW] (0 beyond the length), status
    uint8 [G] and plies int32 [G] (omok_game_info: GameStatus, stones on the board); meta: a free dict (JSON-serialisable)."""

    def __init__(self, n, start_boards, lengths, cells, external, root_n, root_w, child_n, child_w, status, plies, meta=None):
        self.n, self.hw = int(n), int(n) * int(n)
        g = len(lengths)
        self.start_boards = np.ascontiguousarray(start_boards, dtype=np.uint8).reshape(g, self.hw)
        self.lengths = np.ascontiguousarray(lengths, dtype=np.int32).reshape(g)
        self.cells = np.ascontiguousarray(cells, dtype=np.int16).reshape(g, self.hw)
        self.external = np.ascontiguousarray(external, dtype=bool).reshape(g, self.hw)
        self.root_n = np.ascontiguousarray(root_n, dtype=np.uint32).reshape(g, self.hw)
        self.root_w = np.ascontiguousarray(root_w, dtype=np.float32).reshape(g, self.hw)
        self.child_n = np.ascontiguousarray(child_n, dtype=np.uint32).reshape(g, self.hw)
        self.child_w = np.ascontiguousarray(child_w, dtype=np.float32).reshape(g, self.hw)
        self.status = np.ascontiguousarray(status, dtype=np.uint8).reshape(g)
        self.plies = np.ascontiguousarray(plies, dtype=np.int32).reshape(g)
        self.meta = dict(meta or {})

    @classmethod
    def from_log(cls, n, start_boards, lengths, moves, root_n, root_w, child_n, child_w, status, plies, meta=None):
        """from the arrays of omok_game_log_read: moves uint16 [G][HW], cell | 0x100 if external, 0xFFFF beyond the length"""
        moves = np.asarray(moves, dtype=np.uint16)
        lengths = np.asarray(lengths, dtype=np.int32).reshape(-1)
        played = np.arange(moves.shape[1])[None, :] < lengths[:, None]
        cells = np.where(played, (moves & CELL_MASK).astype(np.int16), np.int16(-1))
        external = played & ((moves & EXTERNAL) != 0)
        return cls(n, start_boards, lengths, cells, external, root_n, root_w, child_n, child_w, status, plies, meta)

    @classmethod
    def from_packed(cls, n, entries, offsets, lengths, status, meta=None):
        """from the packed move log of a slots-mode run (omok_selfplay_run_slots_logged): entries uint8 [n_records][20], entry offsets[i] + p =
        move p of game index i (lengths[i] of them; the games may lie in any order, with gaps), status [games].  Games in game-index order,
        start boards empty, plies = lengths; beyond a game's length the rows read as omok_game_log_read leaves them (0xFFFF / 0).  No engine.
        ValueError for a length outside [0, HW], a game that reaches beyond the buffer, or a non-zero pad."""
        hw = int(n) * int(n)
        entries = np.ascontiguousarray(entries, dtype=np.uint8)
        if entries.ndim != 2 or entries.shape[1] != ENTRY_BYTES:
            raise ValueError(f"entries of shape {entries.shape}: expected [n_records, {ENTRY_BYTES}]")
        offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
        lengths = np.asarray(lengths, dtype=np.int32).reshape(-1)
        status = np.asarray(status).reshape(-1)
        g = len(lengths)
        if len(offsets) != g or len(status) != g:
            raise ValueError(f"{len(offsets)} offsets, {g} lengths, {len(status)} status values")
        if g and (lengths.min() < 0 or lengths.max() > hw):
            bad = int(np.flatnonzero((lengths < 0) | (lengths > hw))[0])
            raise ValueError(f"game {bad}: length {int(lengths[bad])} outside [0, {hw}]")
        played = np.arange(hw)[None, :] < lengths[:, None]
        beyond = (lengths > 0) & ((offsets < 0) | (offsets + lengths > entries.shape[0]))
        if beyond.any():
            bad = int(np.flatnonzero(beyond)[0])
            raise ValueError(f"game {bad}: entries [{int(offsets[bad])}, {int(offsets[bad])} + {int(lengths[bad])}) outside the buffer's {entries.shape[0]}")
        rows = (offsets[:, None] + np.arange(hw)[None, :])[played]  # entry index of every played move, game-major
        picked = entries[rows]
        words = picked[:, :16].copy().view("<u4").reshape(-1, 4)
        halves = picked[:, 16:].copy().view("<u2").reshape(-1, 2)
        if halves[:, 1].any():
            bad = int(rows[np.flatnonzero(halves[:, 1])[0]])
            raise ValueError(f"entry {bad}: bytes 18-19 are not zero")
        moves = np.full((g, hw), 0xFFFF, dtype=np.uint16)
        moves[played] = halves[:, 0]
        fields = []
        for k in range(4):  # root_n, root_w, child_n, child_w: the floats are placed as their words
            a = np.zeros((g, hw), dtype=np.uint32)
            a[played] = words[:, k]
            fields.append(a)
        return cls.from_log(n, np.zeros((g, hw), dtype=np.uint8), lengths, moves, fields[0], fields[1].view(np.float32), fields[2],
                            fields[3].view(np.float32), status.astype(np.uint8), lengths.copy(), meta)

    games = property(lambda s: len(s.lengths))

    def moves(self):
        """the uint16 words of omok_game_log_read / omok_env_replay: cell | 0x100 if external, 0xFFFF beyond the length"""
        words = (self.cells.astype(np.int32) & CELL_MASK) | np.where(self.external, EXTERNAL, 0)
        return np.where(self.cells >= 0, words, 0xFFFF).astype(np.uint16)

    def __eq__(self, other):
        """every array bit for bit (the floats compared as their words) and the metadata"""
        if not isinstance(other, GameRecords) or self.n != other.n or self.meta != other.meta:
            return False
        for name in _ARRAYS:
            a, b = getattr(self, name), getattr(other, name)
            if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
                return False
        return True

    # ---- file ------------------------------------------------------------------------------------
    def save(self, path):
        """one .npz: the arrays, the board size and the metadata as JSON text"""
        with open(path, "wb") as f:
            np.savez_compressed(f, n=np.int32(self.n), meta=np.array(json.dumps(self.meta, sort_keys=True)),
                                **{name: getattr(self, name) for name in _ARRAYS})

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(int(z["n"]), *[z[name] for name in _ARRAYS], meta=json.loads(str(z["meta"])))

    # ---- replay (the engine's rules kernel) -------------------------------------------------------
    def position_at(self, game, ply, engine):
        """Stone bytes [HW] of game `game` after its first `ply` moves (0: the start position), through Engine.env_replay"""
        assert 0 <= ply <= int(self.lengths[game])
        boards, _, played = engine.env_replay(self.start_boards[game][None], self.moves()[game][None], self.lengths[game:game + 1], upto=int(ply))
        assert int(played[0]) == ply, f"game {game}: the record stops being legal at move {int(played[0])}"
        return boards[0]

    def verify(self, engine):
        """Replays every game and raises AssertionError unless, for each: every recorded move was placed (played == length), the replay's
        GameStatus is the recorded one (in progress for an unfinished game) and the stones on the final board are the start's plus the
        length -- which is also what omok_game_info counted (plies).  Returns the final boards [G][HW]."""
        assert engine.n == self.n, f"records of board size {self.n}, engine of {engine.n}"
        boards, status, played = engine.env_replay(self.start_boards, self.moves(), self.lengths)
        stones = np.count_nonzero(boards, axis=1)
        start = np.count_nonzero(self.start_boards, axis=1)
        for g in range(self.games):
            assert int(played[g]) == int(self.lengths[g]), f"game {g}: {int(played[g])} of {int(self.lengths[g])} moves replay"
            assert int(status[g]) == int(self.status[g]), f"game {g}: replay ends with status {int(status[g])}, recorded {int(self.status[g])}"
            assert int(stones[g]) == int(start[g]) + int(self.lengths[g]), f"game {g}: {int(stones[g])} stones after {int(start[g])} + {int(self.lengths[g])}"
            assert int(self.plies[g]) == int(stones[g]), f"game {g}: plies {int(self.plies[g])}, stones {int(stones[g])}"
        return boards

    # ---- tactics (the engine's replay and the threat-aware rule's scan) -----------------------------
    def tactics(self, engine):
        """How often a mover overlooked a one-move win or loss.  Walks the plies: the positions of all games after p moves come from
        Engine.env_replay (upto = p) and are scanned with the side to move by Engine.env_threat_scan (the levels of B.OPP_THREAT,
        include/omok_mi355x.h: 1 = the mover can make five, 2 = only the opponent can).  Returns a dict:
          level_before  int8 [G][HW]: the level of the position in front of move p of game g (0 beyond the game's length)
          missed_win    int32 [G][2]: per side (0 Black, 1 White) the moves with level_before == 1 that did not end the game
          unblocked     int32 [G][2]: per side the moves with level_before == 2 after which the opponent's position has level 1
        A record that does not replay (verify) raises AssertionError."""
        assert engine.n == self.n, f"records of board size {self.n}, engine of {engine.n}"
        g = self.games
        level_before = np.zeros((g, self.hw), dtype=np.int8)
        missed_win, unblocked = np.zeros((g, 2), dtype=np.int32), np.zeros((g, 2), dtype=np.int32)
        if g == 0:
            return {"level_before": level_before, "missed_win": missed_win, "unblocked": unblocked}
        moves, start = self.moves(), np.count_nonzero(self.start_boards, axis=1)
        rows = np.arange(g)
        prev = None  # the levels one ply earlier and which games made a move there
        for p in range(int(self.lengths.max()) + 1):
            boards, status, played = engine.env_replay(self.start_boards, moves, self.lengths, upto=p)
            reached = self.lengths >= p
            assert np.all(played[reached] == p), f"the records stop being legal before move {p}"
            side = ((start + p) & 1).astype(np.uint8)
            open_ = reached & (status == 0)  # the game is still in progress after p moves: there is a position to scan
            level = np.zeros(g, dtype=np.int32)
            if open_.any():
                level[open_] = engine.env_threat_scan(boards[open_], side[open_])[1]
            if prev is not None:
                plevel, moved = prev
                mover = 1 - side  # of move p - 1
                np.add.at(missed_win, (rows[moved & (plevel == 1) & open_], mover[moved & (plevel == 1) & open_]), 1)
                np.add.at(unblocked, (rows[moved & (plevel == 2) & (level == 1)], mover[moved & (plevel == 2) & (level == 1)]), 1)
            moved = self.lengths > p
            if p < self.hw:
                level_before[moved, p] = level[moved]
            prev = (level, moved)
        return {"level_before": level_before, "missed_win": missed_win, "unblocked": unblocked}

    # ---- forced wins (the engine's replay and its forced-win solver) ---------------------------------
    def forced_wins(self, engine, max_depth=8, max_nodes=4096):
        """How often a mover had a forced win by continuous fours and let it go.  Walks the plies as tactics does: the positions of all games
        after p moves come from Engine.env_replay (upto = p) and go to Engine.env_vcf_solve with the mover to move (include/omok_mi355x.h).
        Returns a dict:
          moves_before  int8 [G][HW]: the mover's `moves` in front of move p of game g -- the attacker moves of its shortest forced win
                        within max_depth; 0 none (and beyond the game's length), -1 the node budget ran out
          had           int32 [G][2]: per side (0 Black, 1 White) the moves with moves_before = m >= 2
          dropped       int32 [G][2]: per side those of them for which the record shows the win let go: the game ended at move p or p + 1
                        without the mover winning, or move p + 2 exists and moves_before[p + 2] is not in 1..m - 1.  A record that stops
                        before it can tell counts as neither.
        A record that does not replay (verify) raises AssertionError."""
        assert engine.n == self.n, f"records of board size {self.n}, engine of {engine.n}"
        g = self.games
        moves_before = np.zeros((g, self.hw), dtype=np.int8)
        had, dropped = np.zeros((g, 2), dtype=np.int32), np.zeros((g, 2), dtype=np.int32)
        if g == 0:
            return {"moves_before": moves_before, "had": had, "dropped": dropped}
        moves, start = self.moves(), np.count_nonzero(self.start_boards, axis=1)
        final = np.zeros(g, dtype=np.int32)  # the status after the last recorded move
        for p in range(int(self.lengths.max()) + 1):
            boards, status, played = engine.env_replay(self.start_boards, moves, self.lengths, upto=p)
            reached = self.lengths >= p
            assert np.all(played[reached] == p), f"the records stop being legal before move {p}"
            final[self.lengths == p] = status[self.lengths == p]
            moved = self.lengths > p
            if p < self.hw and moved.any():
                assert not status[moved].any(), f"a game goes on after move {p} ended it"
                side = ((start[moved] + p) & 1).astype(np.uint8)
                verdict, _cell, m, _nodes, _pv = engine.env_vcf_solve(boards[moved], side, max_depth, max_nodes)
                moves_before[moved, p] = np.where(verdict == 1, m, verdict)
        for i in range(g):
            length, over = int(self.lengths[i]), final[i] != 0
            for p in range(length):
                m, side = int(moves_before[i, p]), int(start[i] + p) & 1
                if m < 2:
                    continue
                had[i, side] += 1
                if over and p >= length - 2:  # the game ended at move p or p + 1
                    dropped[i, side] += 0 if (p == length - 1 and final[i] == (2 if side == 0 else 3)) else 1
                elif p + 2 < length and not 1 <= int(moves_before[i, p + 2]) <= m - 1:
                    dropped[i, side] += 1
        return {"moves_before": moves_before, "had": had, "dropped": dropped}

    # ---- forced losses (the engine's replay, its forced-win solver and its defence map) ------------------
    def vcf_defence(self, engine, max_depth=8, max_nodes=4096):
        """How often a mover faced the opponent's forced win by continuous fours, and whether the move in the record held it off.  Walks the
        plies as forced_wins does: the positions of all games after p moves come from Engine.env_replay (upto = p).  Stage 1: Engine.env_vcf_solve
        with the side that is NOT to move (the threat if the mover passed).  Stage 2: Engine.env_vcf_defend with the mover to move, on the
        positions whose threat has verdict 1 and moves >= 2, and only on those (a threat in one move is tactics()'s `unblocked` ground and is
        not counted twice; this is the report's definition, not a shortcut: a stone of the mover's can create a threat where there was none).
        Returns a dict, per game and side (0 Black, 1 White) int32 [G][2]:
          threatened    the positions of stage 2
          defensible    those of them with at least one WINS or SAFE cell
          held          defensible, and the played cell is WINS or SAFE
          conceded      defensible, and the played cell is LOSES: a forced loss walked into with a way out on the board
          unknown       the played cell of a stage-2 position is UNKNOWN, or stage 1 ran out of its node budget
        and threat_before int8 [G][HW]: stage 1's `moves` in front of move p; 0 none (and beyond the game's length), -1 the node budget ran out.
        A record that does not replay (verify) raises AssertionError."""
        assert engine.n == self.n, f"records of board size {self.n}, engine of {engine.n}"
        g = self.games
        out = {name: np.zeros((g, 2), dtype=np.int32) for name in ("threatened", "defensible", "held", "conceded", "unknown")}
        out["threat_before"] = np.zeros((g, self.hw), dtype=np.int8)
        if g == 0:
            return out
        moves, start = self.moves(), np.count_nonzero(self.start_boards, axis=1)
        for p in range(min(int(self.lengths.max()), self.hw)):
            boards, status, played = engine.env_replay(self.start_boards, moves, self.lengths, upto=p)
            moved = np.flatnonzero(self.lengths > p)
            assert np.all(played[moved] == p), f"the records stop being legal before move {p}"
            assert not status[moved].any(), f"a game goes on after move {p} ended it"
            side = ((start[moved] + p) & 1).astype(np.uint8)
            verdict, _cell, m, _nodes, _pv = engine.env_vcf_solve(boards[moved], 1 - side, max_depth, max_nodes)
            out["threat_before"][moved, p] = np.where(verdict == 1, m, verdict)
            np.add.at(out["unknown"], (moved[verdict < 0], side[verdict < 0]), 1)
            pick = (verdict == 1) & (m >= 2)
            if not pick.any():
                continue
            rows, sides = moved[pick], side[pick]
            st = engine.env_vcf_defend(boards[rows], sides, max_depth, max_nodes)["status"]
            at = st[np.arange(len(rows)), self.cells[rows, p].astype(np.int64)]
            way_out = ((st == 1) | (st == 2)).any(axis=1)  # OMOK_VCFD_SAFE, OMOK_VCFD_WINS
            for name, which in (("threatened", np.ones(len(rows), dtype=bool)), ("defensible", way_out),
                                ("held", way_out & ((at == 1) | (at == 2))), ("conceded", way_out & (at == 3)), ("unknown", at == 4)):
                np.add.at(out[name], (rows[which], sides[which]), 1)
        return out

    # ---- text --------------------------------------------------------------------------------------
    def coordinate(self, cell):
        """column letter (a = x 0) and row number (1 = y 0) of cell = y * n + x"""
        return f"{chr(ord('a') + cell % self.n)}{cell // self.n + 1}"

    def to_text(self, game):
        """The final board of game `game` with move numbers (X / O: stones of the start position, Black / White), then one line per move:
        ply (stones on the board before it), colour, coordinate, `ext` for an external move (scripted or supplied, not sampled from the mover's
        search), root_n, child_n and q = child_w / child_n where child_n > 0.

        Whose perspective w has (read from backup() in csrc/tree_kernels.hip, Node::propagate, mcts/src/node.rs:83-99): a simulation's value
        is added to the slot of the node it reached and its sign flips at every step up the path; a terminal child that its mover won receives
        +1 in its own slot, an evaluated leaf minus the net's value for the side to move in it.  So child_w / child_n is the mean value of
        the move FOR THE SIDE THAT MADE IT (+1: the mover wins), and root_w, one step further up, has the other sign: root_w / root_n is the
        mean value of the position for the mover's OPPONENT.  The board is the moves as recorded: no rule is applied here (verify does that)."""
        n, length = self.n, int(self.lengths[game])
        start = self.start_boards[game]
        first = int(np.count_nonzero(start))
        label = {c: {1: "X", 2: "O"}.get(int(s), "?") for c, s in enumerate(start) if s}
        for i in range(length):
            label.setdefault(int(self.cells[game, i]), str(i + 1))
        width = max(3, len(str(length)) + 1)
        out = [f"game {game}: {n} x {n}, {first} stones at the start, {length} moves, {STATUS_NAMES.get(int(self.status[game]), '?')}"]
        out.append(" " * 3 + "".join(f"{chr(ord('a') + x):>{width}}" for x in range(n)))
        for y in range(n):
            out.append(f"{y + 1:>3}" + "".join(f"{label.get(y * n + x, '.'):>{width}}" for x in range(n)))
        out.append("move  ply colour cell ext   root_n  child_n        q")
        for i in range(length):
            cell, cn = int(self.cells[game, i]), int(self.child_n[game, i])
            q = f"{float(self.child_w[game, i]) / cn:+.4f}" if cn > 0 else "-"
            out.append(f"{i + 1:>4} {first + i:>4} {'black' if (first + i) % 2 == 0 else 'white':>6} {self.coordinate(cell):>4} "
                       f"{'ext' if self.external[game, i] else '':>3} {int(self.root_n[game, i]):>8} {cn:>8} {q:>8}")
        return "\n".join(out)


save = GameRecords.save
load = GameRecords.load


def main(argv=None):
    ap = argparse.ArgumentParser(prog="omok_ai_amd.records", description="game records written by match.py --save-games / Trainer.evaluate(save_games=...) / Trainer(save_selfplay_games=...)")
    sub = ap.add_subparsers(dest="cmd", required=True)
    show = sub.add_parser("show", help="print one game: the final board with move numbers and one line per move")
    show.add_argument("file")
    show.add_argument("--game", type=int, default=0)
    tac = sub.add_parser("tactics", help="count the overlooked one-move wins and losses by side (needs the GPU: replay and scan run in the engine)")
    tac.add_argument("file")
    forced = sub.add_parser("forced", help="count the forced wins by continuous fours a side had and let go (needs the GPU: replay and solver run in the engine)")
    forced.add_argument("file")
    forced.add_argument("--max-depth", type=int, default=8)
    forced.add_argument("--max-nodes", type=int, default=4096)
    defence = sub.add_parser("defence", help="count the opponent's forced wins by continuous fours a side faced, held off and walked into (needs the GPU: replay, solver and defence map run in the engine)")
    defence.add_argument("file")
    defence.add_argument("--max-depth", type=int, default=8)
    defence.add_argument("--max-nodes", type=int, default=4096)
    args = ap.parse_args(argv)
    rec = load(args.file)
    if args.cmd == "defence":
        from . import api
        eng = api.Engine(board_size=rec.n, games=1, max_nodes=16, max_tables=8, max_batch_k=1)
        try:
            f = rec.vcf_defence(eng, args.max_depth, args.max_nodes)
        finally:
            eng.close()
        out = {"games": rec.games, "moves": int((rec.cells >= 0).sum()), "max_depth": args.max_depth, "max_nodes": args.max_nodes,
               "budget_exhausted": int((f["threat_before"] < 0).sum())}
        for s, name in ((0, "black"), (1, "white")):
            out[name] = {k: int(f[k][:, s].sum()) for k in ("threatened", "defensible", "held", "conceded", "unknown")}
        if rec.meta:
            print("meta: " + json.dumps(rec.meta, sort_keys=True))
        print("defence: " + json.dumps(out, sort_keys=True))
        return 0
    if args.cmd == "forced":
        from . import api
        eng = api.Engine(board_size=rec.n, games=1, max_nodes=16, max_tables=8, max_batch_k=1)
        try:
            f = rec.forced_wins(eng, args.max_depth, args.max_nodes)
        finally:
            eng.close()
        out = {"games": rec.games, "moves": int((rec.cells >= 0).sum()), "max_depth": args.max_depth, "max_nodes": args.max_nodes,
               "budget_exhausted": int((f["moves_before"] < 0).sum())}
        for s, name in ((0, "black"), (1, "white")):
            out[name] = {"had": int(f["had"][:, s].sum()), "dropped": int(f["dropped"][:, s].sum())}
        if rec.meta:
            print("meta: " + json.dumps(rec.meta, sort_keys=True))
        print("forced: " + json.dumps(out, sort_keys=True))
        return 0
    if args.cmd == "tactics":
        from . import api
        eng = api.Engine(board_size=rec.n, games=1, max_nodes=16, max_tables=8, max_batch_k=1)
        try:
            t = rec.tactics(eng)
        finally:
            eng.close()
        sides = (rec.start_boards != 0).sum(axis=1)[:, None] + np.arange(rec.hw)[None, :] & 1
        played = rec.cells >= 0
        out = {"games": rec.games, "moves": int(played.sum())}
        for s, name in ((0, "black"), (1, "white")):
            mine = played & (sides == s)
            out[name] = {"moves": int(mine.sum()), "could_win": int((mine & (t["level_before"] == 1)).sum()), "missed_win": int(t["missed_win"][:, s].sum()),
                         "had_to_block": int((mine & (t["level_before"] == 2)).sum()), "unblocked": int(t["unblocked"][:, s].sum())}
        if rec.meta:
            print("meta: " + json.dumps(rec.meta, sort_keys=True))
        print("tactics: " + json.dumps(out, sort_keys=True))
        return 0
    if not 0 <= args.game < rec.games:
        ap.error(f"--game {args.game} outside [0, {rec.games})")
    if rec.meta:
        print("meta: " + json.dumps(rec.meta, sort_keys=True))
    print(rec.to_text(args.game))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
