"""Host-side mirror of the reference's crate API for the self-play path, over the C ABI.

Names follow the reference so parity tests read like its own code:
  Environment                      environment/src/lib.rs:62-166
  encode_nn_input                  alpha-zero/src/encoder.rs:10-46
  AgentModel.evaluate_p/_pv        alpha-zero/src/agent_model.rs:105-134
  SelfPlay.execute                 ParallelMCTSExecutor::execute, alpha-zero/src/parallel_mcts_executor.rs:26-35
  SelfPlay.sample_actions/advance  Agent::{sample_action, play_action, ensure_action_exists}, agent.rs:83-232
  SelfPlay.run                     Trainer::train self-play phase, src/trainer.rs:95-205
  Engine.load_weights2 / load2     the second agent's AgentModel of benchmark/src/main.rs:14-108
  SelfPlay.match_reset             benchmark/src/main.rs: net 1 against net 2, half of the games per colour
  SelfPlay.versus_run              Trainer::play_against_naive_player / _play_against_random_player, src/trainer.rs:400-603
  Engine.env_threat_scan           which level of the threat-aware scripted player's rule (B.OPP_THREAT, include/omok_mi355x.h) decides a position
  Engine.env_vcf_solve             does the side to move have a forced win by continuous fours?  (B.OPP_VCF is the scripted player that asks)
  Engine.env_vcf_defend            the defender's half: which moves of the side to move do not lose to the other side's forced win?
  Environment.check_positions      the rules of Environment::place_stone read backwards: is a given board a position of a game in progress?
  SelfPlay.reset_from / analyze    Agent::new (agent.rs:16-35) on given positions instead of Environment::new()
  SelfPlay.match_reset_from        the match of benchmark/src/main.rs from given positions (an opening book), each agent with its own net
  Environment.random_positions     an opening book without a file: positions after s plies of _play_against_random_player's moves on both sides
  SelfPlay.game_log / game_records every move of an episode with the mover's search statistics (the reference keeps sampled Transitions only, trainer.rs:169-173)
  Engine.env_replay                Environment::place_stone move by move over a batch of records: a record back into a position
All compute happens in the HIP library; nothing here has a CPU path.
"""
import ctypes as C

import os

import numpy as np

from . import binding as B
from . import weights as W

EMPTY, BLACK, WHITE = 0, 1, 2
TURN_BLACK, TURN_WHITE = 0, 1
IN_PROGRESS, DRAW, BLACK_WIN, WHITE_WIN = 0, 1, 2, 3


def vcf_defend_counts(status):
    """{safe, wins, loses, unknown: int32 [B]}: the cells of each status in the rows of an omok_env_vcf_defend status array [B][HW]"""
    status = np.asarray(status)
    names = (("safe", B.VCFD_SAFE), ("wins", B.VCFD_WINS), ("loses", B.VCFD_LOSES), ("unknown", B.VCFD_UNKNOWN))
    return {name: np.count_nonzero(status == value, axis=1).astype(np.int32) for name, value in names}


class Engine:
    """Opaque engine handle (omok_create / omok_destroy)."""

    def __init__(self, board_size=15, games=1, max_nodes=2048, max_tables=1024, max_batch_k=16, device=0,
                 net_mode=B.NET_F16X3, seed=0, game_offset=0, max_tree_waves=0):
        self.n, self.hw, self.games = board_size, board_size * board_size, games
        self.max_nodes = max_nodes
        self.max_batch_k = max_batch_k
        cfg = B.Config(board_size, games, max_nodes, max_tables, max_batch_k, device, net_mode, max_tree_waves, seed, game_offset)
        h = C.c_void_p()
        rc = B.lib().omok_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise B.OmokError(rc, B.lib().omok_last_error(None).decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            B.lib().omok_destroy(self.h)
            self.h = None

    def __del__(self):
        try:  # (at interpreter shutdown the module globals may already be gone: the process is ending, the driver frees the device memory)
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc < 0:
            raise B.OmokError(rc, B.lib().omok_last_error(self.h).decode())
        return rc

    # ---- net --------------------------------------------------------------------------------
    def load_weights(self, tensors):
        """31 tensors in the reference's variable order (network.rs / model_io.rs positional order)."""
        assert len(tensors) == B.lib().omok_net_num_tensors()
        for i, t in enumerate(tensors):
            t = np.ascontiguousarray(t, dtype=np.float32).ravel()
            self._chk(B.lib().omok_net_load(self.h, i, B.fptr(t), t.size))
        self._chk(B.lib().omok_net_commit(self.h))

    def load(self, path):
        """ModelIO::load (alpha-zero/src/model_io.rs:92-120): the reference's bincode weights file, positional."""
        self._chk(B.lib().omok_net_load_file(self.h, os.fsencode(path)))

    def save(self, path):
        """ModelIO::save (alpha-zero/src/model_io.rs:59-90)."""
        self._chk(B.lib().omok_net_save_file(self.h, os.fsencode(path)))

    def load_random_weights(self, seed=0):
        self.load_weights(W.init_random(self.n, seed))

    # ---- second net slot (match episodes) ---------------------------------------------------
    def load_weights2(self, tensors):
        """net 2 from 31 tensors (same order as load_weights), committed with its own fc0 format probe"""
        assert len(tensors) == B.lib().omok_net_num_tensors()
        for i, t in enumerate(tensors):
            t = np.ascontiguousarray(t, dtype=np.float32).ravel()
            self._chk(B.lib().omok_net2_load(self.h, i, B.fptr(t), t.size))
        self._chk(B.lib().omok_net2_commit(self.h))

    def load2(self, path):
        """net 2 from a ModelIO weights file (omok_net2_load_file)"""
        self._chk(B.lib().omok_net2_load_file(self.h, os.fsencode(path)))

    def net2_info(self):
        """net 2's commit outcome and the rows each net evaluated in match episodes since reset_stats:
        {"fc0_format": "fp6" | "f16" | "mixed" | "f32", "probe_outside": int, "evals": (net 1, net 2)}"""
        fmt, outside = C.c_int32(), C.c_int32()
        ev = (C.c_double * 2)()
        self._chk(B.lib().omok_net2_info(self.h, C.byref(fmt), C.byref(outside), ev))
        return {"fc0_format": B.FC0_FORMATS[fmt.value], "probe_outside": outside.value, "evals": (ev[0], ev[1])}

    # ---- native training step (AgentModel::train, agent_model.rs:136-168; Trainer::train's update loop, src/trainer.rs:329-357) ----
    def read_weights(self):
        """the 31 raw fp32 tensors of net 1 as loaded or trained (omok_net_read), flat, in the reference's variable order"""
        out = []
        for i in range(B.lib().omok_net_num_tensors()):
            t = np.empty(int(B.lib().omok_net_tensor_size(self.h, i)), dtype=np.float32)
            self._chk(B.lib().omok_net_read(self.h, i, B.fptr(t), t.size))
            out.append(t)
        return out

    def train_begin(self, max_batch):
        """a fresh AdadeltaOptimizer (zeroed accumulators) and the step's buffers for batches of up to max_batch records"""
        self._chk(B.lib().omok_train_begin(self.h, int(max_batch)))

    def train_end(self):
        self._chk(B.lib().omok_train_end(self.h))

    def _train_once(self, fn, records_ptr, n_records, indices):
        idx = np.ascontiguousarray(indices, dtype=np.int64).ravel()
        losses = np.zeros(3, dtype=np.float32)
        self._chk(fn(self.h, C.c_void_p(int(records_ptr)), int(n_records), idx.ctypes.data_as(C.POINTER(C.c_int64)), idx.size, B.fptr(losses)))
        return float(losses[0]), float(losses[1]), float(losses[2])

    def train_step(self, records_ptr, n_records, indices):
        """one AgentModel::train on the packed replay records (device pointer) `indices` names: minimize, then (v_loss, p_loss, loss) after
        the update.  Leaves the net uncommitted (commit() before searching)."""
        return self._train_once(B.lib().omok_train_step, records_ptr, n_records, indices)

    def train_losses(self, records_ptr, n_records, indices):
        """(v_loss, p_loss, loss) of the current weights on those records; changes nothing"""
        return self._train_once(B.lib().omok_train_losses, records_ptr, n_records, indices)

    def train_batch_indices(self, n_records, batch, key, step):
        """the record indices step `step` of train_run(key) draws: min(batch, n_records) distinct indices in draw order, int64"""
        out = np.zeros(int(batch), dtype=np.int64)
        k = self._chk(B.lib().omok_train_batch_indices(self.h, int(n_records), int(batch), int(key) & 0xFFFFFFFFFFFFFFFF, int(step),
                                                       out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out[:k]

    def train_run(self, records_ptr, n_records, update_count, batch_size, key):
        """trainer.rs:329-357 in one blocking call: update_count steps on device-drawn batches, then the net is committed; returns the mean
        (v_loss, p_loss, loss) of the last <= 100 steps"""
        losses = np.zeros(3, dtype=np.float32)
        self._chk(B.lib().omok_train_run(self.h, C.c_void_p(int(records_ptr)), int(n_records), int(update_count), int(batch_size),
                                         int(key) & 0xFFFFFFFFFFFFFFFF, B.fptr(losses)))
        return float(losses[0]), float(losses[1]), float(losses[2])

    def train_gradient_count(self):
        """floats of a gradient slab (omok_train_gradient_count): the 31 tensors back to back, a function of the board size only"""
        return int(self._chk(B.lib().omok_train_gradient_count(self.h)))

    def train_backward(self, records_ptr, n_records, indices, grad_dst_ptr=None):
        """first half of train_step: the gradients of the batch `indices` names, no update.  They stay readable by train_gradient and, with
        grad_dst_ptr (device memory of train_gradient_count() floats, e.g. a torch tensor's data_ptr()), are copied there before the call returns."""
        idx = np.ascontiguousarray(indices, dtype=np.int64).ravel()
        dst = C.c_void_p(int(grad_dst_ptr)) if grad_dst_ptr else None
        self._chk(B.lib().omok_train_backward(self.h, C.c_void_p(int(records_ptr)), int(n_records), idx.ctypes.data_as(C.POINTER(C.c_int64)), idx.size, dst))

    def train_apply(self, grads_ptr=None, ranks=1):
        """second half: Adadelta with the engine's own gradient (grads_ptr None, ranks 1) or with the rank-order average of the [ranks, count] fp32
        slabs at device pointer grads_ptr; then (v_loss, p_loss, loss) of the pending batch after the update.  Leaves the net uncommitted."""
        losses = np.zeros(3, dtype=np.float32)
        src = C.c_void_p(int(grads_ptr)) if grads_ptr else None
        self._chk(B.lib().omok_train_apply(self.h, src, int(ranks), B.fptr(losses)))
        return float(losses[0]), float(losses[1]), float(losses[2])

    def train_gradient(self, index):
        """gradient of tensor `index` the last step applied (omok_debug_train_gradient), flat"""
        g = np.empty(int(B.lib().omok_net_tensor_size(self.h, index)), dtype=np.float32)
        self._chk(B.lib().omok_debug_train_gradient(self.h, int(index), B.fptr(g), g.size))
        return g

    def commit(self):
        """omok_net_commit: pack the raw tensors for the search (after train_step)"""
        self._chk(B.lib().omok_net_commit(self.h))

    def evaluate_pv(self, inputs):
        x = np.ascontiguousarray(inputs, dtype=np.float32).reshape(-1, 3 * self.hw)
        b = x.shape[0]
        p = np.zeros((b, self.hw), dtype=np.float32)
        v = np.zeros(b, dtype=np.float32)
        self._chk(B.lib().omok_evaluate_pv(self.h, B.fptr(x), b, B.fptr(p), B.fptr(v)))
        return p.reshape(b, self.n, self.n), v.reshape(b, 1)

    def evaluate_logits(self, inputs):
        """pre-softmax policy logits [B][HW] and pre-tanh value [B] of the same forward (precision evidence)"""
        x = np.ascontiguousarray(inputs, dtype=np.float32).reshape(-1, 3 * self.hw)
        b = x.shape[0]
        lg = np.zeros((b, self.hw), dtype=np.float32)
        vp = np.zeros(b, dtype=np.float32)
        self._chk(B.lib().omok_evaluate_logits(self.h, B.fptr(x), b, B.fptr(lg), B.fptr(vp)))
        return lg, vp

    def evaluate_p(self, inputs):
        return self.evaluate_pv(inputs)[0]

    # ---- environment ------------------------------------------------------------------------
    def env_play(self, moves):
        """moves [B][L] int32 -> (status [B][L], boards [B][HW], turns [B], legal [B])."""
        moves = np.ascontiguousarray(moves, dtype=np.int32)
        if moves.ndim == 1:
            moves = moves[None]
        b, l = moves.shape
        status = np.zeros((b, max(l, 1)), dtype=np.int32)
        boards = np.zeros((b, self.hw), dtype=np.uint8)
        turns = np.zeros(b, dtype=np.uint8)
        legal = np.zeros(b, dtype=np.uint16)
        self._chk(B.lib().omok_env_play(self.h, B.iptr(moves), b, l, B.iptr(status), B.u8ptr(boards), B.u8ptr(turns),
                                        legal.ctypes.data_as(C.POINTER(C.c_uint16))))
        return status[:, :l], boards, turns, legal

    def env_place_stone(self, boards, turns, legal, actions):
        """Environment::place_stone on caller-held environments (updated in place); returns status [B] (-1 = None)."""
        b = len(actions)
        assert boards.dtype == np.uint8 and boards.shape == (b, self.hw) and boards.flags.c_contiguous
        assert turns.dtype == np.uint8 and legal.dtype == np.uint16
        actions = np.ascontiguousarray(actions, dtype=np.int32)
        status = np.zeros(b, dtype=np.int32)
        self._chk(B.lib().omok_env_place_stone(self.h, B.u8ptr(boards), B.u8ptr(turns), legal.ctypes.data_as(C.POINTER(C.c_uint16)),
                                               B.iptr(actions), b, B.iptr(status)))
        return status

    def env_scripted_actions(self, kind, boards, turns):
        """the forced part of the scripted player's rule (src/trainer.rs:514-531) on caller-held positions: the lowest empty cell at
        which a stone of either side ends the game, -1 where there is none (always -1 for B.OPP_RANDOM); int32 [B].  For B.OPP_THREAT: the
        cell of levels 1..5 of the threat-aware rule for the side to move turns[b] (0 / 1, anything else raises), -1 for levels 6 and 7; for
        B.OPP_GUARD: the defending player's cell where no draw decided, else -1"""
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, self.hw)
        turns = np.ascontiguousarray(turns, dtype=np.uint8).reshape(-1)
        assert len(turns) == len(boards)
        forced = np.zeros(len(boards), dtype=np.int32)
        self._chk(B.lib().omok_env_scripted_actions(self.h, int(kind), B.u8ptr(boards), B.u8ptr(turns), len(boards), B.iptr(forced)))
        return forced

    def env_threat_scan(self, boards, turns):
        """omok_env_threat_scan on caller-held positions, turns[b] = the side to move (0 Black / 1 White): which level of the B.OPP_THREAT rule
        (include/omok_mi355x.h) decides.  Returns int32 [B] arrays (cell, level, count): level 1..7, 0 on a full board; cell = the move of
        levels 1..5, else -1; count = the number of cells the draw of level 6 / 7 chooses among, else 0.  Needs no net."""
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, self.hw)
        turns = np.ascontiguousarray(turns, dtype=np.uint8).reshape(-1)
        assert len(turns) == len(boards)
        cell, level, count = (np.zeros(len(boards), dtype=np.int32) for _ in range(3))
        self._chk(B.lib().omok_env_threat_scan(self.h, B.u8ptr(boards), B.u8ptr(turns), len(boards), B.iptr(cell), B.iptr(level), B.iptr(count)))
        return cell, level, count

    def env_vcf_solve(self, boards, turns, max_depth=8, max_nodes=4096):
        """omok_env_vcf_solve on caller-held positions, turns[b] = the side to move (0 Black / 1 White): does it have a forced win by
        continuous fours within max_depth (1..16) of its moves and max_nodes (1..65536) search nodes?  (The rule: include/omok_mi355x.h.)
        Returns int32 arrays (verdict, cell, moves, nodes) [B] and pv [B][2 * max_depth - 1]: verdict 1 a win, 0 none, -1 the node budget
        ran out; cell = the first move and moves = the attacker moves up to the five (-1 and 0 unless verdict is 1); pv = attacker, forced
        reply, attacker, ... padded with -1.  Needs no net."""
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, self.hw)
        turns = np.ascontiguousarray(turns, dtype=np.uint8).reshape(-1)
        assert len(turns) == len(boards)
        verdict, cell, moves, nodes = (np.zeros(len(boards), dtype=np.int32) for _ in range(4))
        pv = np.zeros((len(boards), max(2 * int(max_depth) - 1, 1)), dtype=np.int32)
        self._chk(B.lib().omok_env_vcf_solve(self.h, B.u8ptr(boards), B.u8ptr(turns), len(boards), int(max_depth), int(max_nodes), B.iptr(verdict),
                                             B.iptr(cell), B.iptr(moves), B.iptr(nodes), B.iptr(pv)))
        return verdict, cell, moves, nodes, pv

    def env_vcf_defend(self, boards, turns, max_depth=8, max_nodes=4096):
        """omok_env_vcf_defend on caller-held positions, turns[b] = the side to move: which of its moves do not lose to the other side's
        forced win by continuous fours within max_depth (1..16) attacker moves and max_nodes (1..65536) nodes per cell?  (The rule:
        include/omok_mi355x.h.)  Returns a dict: status uint8 [B][HW] (B.VCFD_OCCUPIED / SAFE / WINS / LOSES / UNKNOWN), moves uint8 [B][HW],
        nodes and reply int32 [B][HW] (the other side's win after a stone there: its attacker moves, the nodes counted, its first move or
        -1), threat int32 [B][3] (verdict, moves, cell of the other side if the mover passed), and safe, wins, loses, unknown int32 [B]:
        the cells of each status, summed here from the status rows.  Needs no net."""
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, self.hw)
        turns = np.ascontiguousarray(turns, dtype=np.uint8).reshape(-1)
        assert len(turns) == len(boards)
        b = len(boards)
        status, moves = np.zeros((b, self.hw), dtype=np.uint8), np.zeros((b, self.hw), dtype=np.uint8)
        nodes, reply = np.zeros((b, self.hw), dtype=np.int32), np.zeros((b, self.hw), dtype=np.int32)
        threat = np.zeros((b, 3), dtype=np.int32)
        self._chk(B.lib().omok_env_vcf_defend(self.h, B.u8ptr(boards), B.u8ptr(turns), b, int(max_depth), int(max_nodes), B.u8ptr(status),
                                              B.u8ptr(moves), B.iptr(nodes), B.iptr(reply), B.iptr(threat)))
        out = {"status": status, "moves": moves, "nodes": nodes, "reply": reply, "threat": threat}
        out.update(vcf_defend_counts(status))
        return out

    def env_guard_scan(self, boards, turns, draws=None, max_depth=B.VCF_OPP_DEPTH, max_nodes=B.VCF_OPP_NODES):
        """omok_env_guard_scan on caller-held positions, turns[b] = the side to move: the move of the defending player B.OPP_GUARD (the rule:
        include/omok_mi355x.h) with the draw words draws uint32 [B] (None: all 0), and the step of its rule that decided, with max_depth
        (1..16) and max_nodes (1..4096) in place of the player's own budget.  Returns a dict of int32 [B] arrays: cell (-1 on a full board),
        step 0..5, level (the VCF rule's in steps 1, 2 and 5, the restricted rule's 3..7 in steps 3 and 4) and count (the cells the deciding
        draw chose among, else 0).  Needs no net."""
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, self.hw)
        turns = np.ascontiguousarray(turns, dtype=np.uint8).reshape(-1)
        assert len(turns) == len(boards)
        if draws is not None:
            draws = np.ascontiguousarray(draws, dtype=np.uint32).reshape(-1)
            assert len(draws) == len(boards)
        out = {name: np.zeros(len(boards), dtype=np.int32) for name in ("cell", "step", "level", "count")}
        self._chk(B.lib().omok_env_guard_scan(self.h, B.u8ptr(boards), B.u8ptr(turns), None if draws is None else draws.ctypes.data_as(C.POINTER(C.c_uint32)),
                                              len(boards), int(max_depth), int(max_nodes), *[B.iptr(out[name]) for name in ("cell", "step", "level", "count")]))
        return out

    def env_check_positions(self, boards):
        """omok_env_check_positions on caller-held boards [B][HW] (bytes): (verdict int32 [B], stones int32 [B]); verdict 0 = a legal position
        of a game in progress, 1 bad byte, 2 impossible stone counts, 3 already won, 4 full board; the side to move is stones & 1"""
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, self.hw)
        verdict = np.zeros(len(boards), dtype=np.int32)
        stones = np.zeros(len(boards), dtype=np.int32)
        self._chk(B.lib().omok_env_check_positions(self.h, B.u8ptr(boards), len(boards), B.iptr(verdict), B.iptr(stones)))
        return verdict, stones

    def env_random_positions(self, key, first_game, stones, batch):
        """omok_env_random_positions: (boards uint8 [batch][HW], ok uint8 [batch]); position b = `stones` plies of the game with global id
        first_game + b, both sides the RANDOM scripted player under RNG key `key`; ok 0 = a placement ended the game and the board stops there"""
        boards = np.zeros((int(batch), self.hw), dtype=np.uint8)
        ok = np.zeros(int(batch), dtype=np.uint8)
        self._chk(B.lib().omok_env_random_positions(self.h, int(key) & 0xFFFFFFFFFFFFFFFF, int(first_game), int(stones), int(batch),
                                                    B.u8ptr(boards), B.u8ptr(ok)))
        return boards, ok

    def env_replay(self, start_boards, moves, lengths, upto=-1):
        """omok_env_replay on caller-held records: from start_boards [B][HW] (None: empty boards) the moves moves[b][: min(lengths[b], upto)]
        (upto < 0: all; uint16 words, cell = word & 0xFF) by Environment::place_stone, stopping in front of the first illegal move and after a
        move that ends the game.  Returns (boards uint8 [B][HW], status int32 [B], played int32 [B]); a start board with a non-zero
        env_check_positions verdict v comes back unchanged with status -1 and played -v."""
        moves = np.ascontiguousarray(moves, dtype=np.uint16)
        lengths = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
        batch = len(lengths)
        moves = moves.reshape(batch, -1)
        start = None
        if start_boards is not None:
            start = np.ascontiguousarray(start_boards, dtype=np.uint8).reshape(batch, self.hw)
        boards = np.zeros((batch, self.hw), dtype=np.uint8)
        status = np.zeros(batch, dtype=np.int32)
        played = np.zeros(batch, dtype=np.int32)
        self._chk(B.lib().omok_env_replay(self.h, None if start is None else B.u8ptr(start), moves.ctypes.data_as(C.POINTER(C.c_uint16)),
                                          B.iptr(lengths), batch, moves.shape[1], int(upto), B.u8ptr(boards), B.iptr(status), B.iptr(played)))
        return boards, status, played

    def replay_augment_records(self, records_ptr, n_records, offsets, lengths, dst_ptr, cap_records):
        """omok_replay_augment_records_dev on caller-held packed records (run_slots' output, or another rank's gathered records): z back-fill and
        the five augmentations of Trainer::train (src/trainer.rs:207-324) into dst_ptr, games in the order of `offsets` / `lengths` (host arrays, one
        entry per game: first record and record count in the device buffer records_ptr of n_records records).  Both pointers are device pointers
        (e.g. a torch uint8 tensor's data_ptr()).  Returns 6 * sum(lengths); at most cap_records records are written."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        lengths = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
        if len(offsets) != len(lengths):
            raise ValueError(f"{len(offsets)} offsets for {len(lengths)} lengths")
        n = B.lib().omok_replay_augment_records_dev(self.h, C.c_void_p(records_ptr), int(n_records), offsets.ctypes.data_as(C.POINTER(C.c_int64)),
                                                    B.iptr(lengths), len(lengths), C.c_void_p(dst_ptr), int(cap_records))
        if n < 0:
            raise B.OmokError(int(n), B.lib().omok_last_error(self.h).decode())
        return int(n)

    def encode_nn_input(self, boards, turns, mode=B.MODE_PLAYER):
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, self.hw)
        turns = np.ascontiguousarray(turns, dtype=np.uint8).reshape(-1)
        out = np.zeros((boards.shape[0], 3 * self.hw), dtype=np.float32)
        self._chk(B.lib().omok_encode_nn_input(self.h, B.u8ptr(boards), B.u8ptr(turns), boards.shape[0], mode, B.fptr(out)))
        return out.reshape(-1, self.n, self.n, 3)

    # ---- stats ------------------------------------------------------------------------------
    def operand_rows(self, first_row, rows):
        """uint8 [rows][omok_operand_row_bytes]: the fc0 operand rows the last forward left (omok_debug_operand_rows)."""
        nb = int(B.lib().omok_operand_row_bytes(self.h))
        if nb < 0:
            raise B.OmokError(nb, "no operand rows in this net mode")
        out = np.empty((rows, nb), dtype=np.uint8)
        self._chk(B.lib().omok_debug_operand_rows(self.h, first_row, rows, out.ctypes.data_as(C.c_void_p)))
        return out

    def set_base_cache(self, on=True):
        self._chk(B.lib().omok_debug_set_base_cache(self.h, int(bool(on))))

    def set_lazy_policy(self, on=True):
        """False: the run loops' rounds scatter every request's policy eagerly, as omok_execute and the step-wise calls do (same bits: tests)."""
        self._chk(B.lib().omok_debug_set_lazy_policy(self.h, int(bool(on))))

    def lazy_policy_stats(self):
        """raw policy rows turned into probabilities so far: {"noise": at the root-noise site, "descent": in a descent}"""
        out = (C.c_uint64 * 2)()
        self._chk(B.lib().omok_debug_lazy_policy_stats(self.h, out))
        return {"noise": int(out[0]), "descent": int(out[1])}

    def set_window_rects(self, on=True):
        """False: fc0 window tiles walk their bin's whole 7x7 window instead of the rectangle their rows can differ in (same bits: tests)."""
        self._chk(B.lib().omok_debug_set_window_rects(self.h, int(bool(on))))

    def set_children_kernel(self, which=2):
        """2: k_sib_children2 (default), 1: k_sib_children on the difference path of sibling rounds (A-B / tests)."""
        self._chk(B.lib().omok_debug_set_children_kernel(self.h, int(which)))

    def last_plan(self):
        """what the last net forward decided (omok_debug_last_plan): dict of B.PLAN_NAMES, "path" as a name of B.PLAN_PATHS"""
        out = np.zeros(len(B.PLAN_NAMES), dtype=np.int32)
        n = self._chk(B.lib().omok_debug_last_plan(self.h, B.iptr(out), out.size))
        assert n == out.size
        d = dict(zip(B.PLAN_NAMES, (int(x) for x in out)))
        d["path"] = B.PLAN_PATHS[d["path"]]
        return d

    def set_profiling(self, on=True):
        """True / 1: time every launch; N > 1: time one search round in N (stats are scaled); False: off."""
        self._chk(B.lib().omok_set_profiling(self.h, int(on)))

    def stats(self):
        s = (C.c_double * len(B.STAT_NAMES))()
        self._chk(B.lib().omok_get_stats(self.h, s))
        return dict(zip(B.STAT_NAMES, list(s)))

    def reset_stats(self):
        self._chk(B.lib().omok_reset_stats(self.h))


class Environment:
    """environment::Environment (environment/src/lib.rs:62-166): the caller holds board / turn / legal_move_count, the
    device rules kernel applies place_stone to them (omok_env_place_stone, batch of one)."""

    def __init__(self, engine):
        self.eng = engine
        self._board = np.zeros((1, engine.hw), dtype=np.uint8)   # Environment::new (:73-79)
        self._turn = np.zeros(1, dtype=np.uint8)
        self._legal = np.full(1, engine.hw, dtype=np.uint16)

    board = property(lambda s: s._board[0])
    turn = property(lambda s: int(s._turn[0]))
    legal_move_count = property(lambda s: int(s._legal[0]))

    def place_stone(self, index):
        s = int(self.eng.env_place_stone(self._board, self._turn, self._legal, [int(index)])[0])
        return None if s < 0 else s

    @staticmethod
    def check_positions(engine, boards):
        """(verdict [B], stones [B]) of caller-supplied boards [B][HW]: Engine.env_check_positions"""
        return engine.env_check_positions(boards)

    @staticmethod
    def random_positions(engine, key, first_game, stones, batch):
        """(boards [batch][HW], ok [batch]) of random openings with `stones` stones: Engine.env_random_positions"""
        return engine.env_random_positions(key, first_game, stones, batch)

    def encode_board(self, turn):
        """Environment::encode_board(turn): the first 2*HW floats of the NN input with that perspective."""
        t = np.array([turn], dtype=np.uint8)
        return self.eng.encode_nn_input(self.board[None], t, B.MODE_PLAYER).reshape(-1)[: 2 * self.eng.hw].copy()


class SelfPlay:
    """G games x (black agent, white agent): the reference's self-play phase on one GPU."""

    def __init__(self, engine):
        self.eng = engine
        self.h = engine.h
        self.n, self.hw, self.games = engine.n, engine.hw, engine.games
        self._chk = engine._chk

    def reset(self):
        self._chk(B.lib().omok_selfplay_reset(self.h))

    def reset_from(self, boards):
        """Agent::new for both agents of every game on the given positions (omok_selfplay_reset_from): boards [G][HW] Stone bytes, all with
        the same stone count, each a legal position of a game in progress (Environment.check_positions).  The episode starts at ply =
        stone count; a rejected call (OmokError -5 / -1) leaves the engine as it was."""
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1)
        assert boards.size == self.games * self.hw
        self._chk(B.lib().omok_selfplay_reset_from(self.h, B.u8ptr(boards)))

    def match_reset_from(self, split, boards):
        """Match episode on the given positions (omok_match_reset_from): boards [G][HW] as for reset_from, split as for match_reset (in games
        [0, split) net 1 owns the Black tree, whichever side is to move).  A rejected call (OmokError -3 / -1 / -5) leaves the engine as it was."""
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1)
        assert boards.size == self.games * self.hw
        self._chk(B.lib().omok_match_reset_from(self.h, int(split), B.u8ptr(boards)))

    def root_stats(self):
        """(root_n uint32 [G], root_w float32 [G]) of the side-to-move agents (omok_root_stats); 0 for finished games"""
        n = np.zeros(self.games, dtype=np.uint32)
        w = np.zeros(self.games, dtype=np.float32)
        self._chk(B.lib().omok_root_stats(self.h, n.ctypes.data_as(C.POINTER(C.c_uint32)), B.fptr(w)))
        return n, w

    def match_reset(self, split):
        """Match episode (omok_match_reset): in games [0, split) net 1 plays Black and net 2 White, in [split, G) the reverse; every
        evaluation uses the net of the tree it serves until the next reset().  A whole match is run(..., threshold=0)."""
        self._chk(B.lib().omok_match_reset(self.h, int(split)))

    def set_episode(self, episode):
        """index of the RNG stream the NEXT reset uses (each reset = one trainer iteration advances it by itself)"""
        self._chk(B.lib().omok_set_episode(self.h, int(episode)))

    def compute_policy(self):
        """Agent::compute_policy of the side-to-move agents: (pi [G][HW], has [G]); has == 0 where the reference returns None"""
        pi = np.zeros((self.games, self.hw), dtype=np.float32)
        has = np.zeros(self.games, dtype=np.uint8)
        self._chk(B.lib().omok_compute_policy(self.h, B.fptr(pi), B.u8ptr(has)))
        return pi, has

    def play_actions(self, actions):
        """externally chosen moves: ensure_action_exists + play_action on both agents of every live game"""
        a = np.ascontiguousarray(actions, dtype=np.int32)
        assert a.size == self.games
        self._chk(B.lib().omok_play_actions(self.h, B.iptr(a)))

    def set_actions(self, actions):
        """step-wise form of play_actions (mirror_generate / mirror_eval|inject / mirror_apply follow)"""
        a = np.ascontiguousarray(actions, dtype=np.int32)
        assert a.size == self.games
        self._chk(B.lib().omok_set_actions(self.h, B.iptr(a)))

    def opponent_actions(self, kind):
        """the scripted player's move (B.OPP_NAIVE / B.OPP_RANDOM, src/trainer.rs:508-534, 452-455; B.OPP_THREAT, the threat-aware rule; B.OPP_VCF, the same with the
        forced-win solver; B.OPP_GUARD, the defending player that consults the forced-loss map) for the side to move of every live game, chosen on the device and staged like set_actions (the mirror step / advance follow); -1 for finished games"""
        a = np.zeros(self.games, dtype=np.int32)
        self._chk(B.lib().omok_opponent_actions(self.h, int(kind), B.iptr(a)))
        return a

    def versus_run(self, kind, opponent_side, count, batch_size, epsilon=0.25, alpha=0.03, max_plies=0):
        """Evaluation episode after reset() (omok_versus_run): the scripted player `kind` (B.OPP_NAIVE, B.OPP_RANDOM, B.OPP_THREAT, B.OPP_VCF or B.OPP_GUARD) plays the colour opponent_side (0 = Black, moves
        first: play_against_naive_player, src/trainer.rs:487-603; 1 = White: _play_against_random_player, :400-485), the net the other with
        `count` simulations and sample_action(Best).  Returns ((black_win, white_win, draw), stats)."""
        s = (C.c_double * len(B.STAT_NAMES))()
        res = np.zeros(3, dtype=np.int32)
        self._chk(B.lib().omok_versus_run(self.h, int(kind), int(opponent_side), count, batch_size, epsilon, alpha, max_plies, B.iptr(res), s))
        return tuple(int(x) for x in res), dict(zip(B.STAT_NAMES, list(s)))

    def root_children(self, game, side):
        """(actions, n, w, p) of the root's children in insertion order"""
        cap = self.hw
        a = np.zeros(cap, dtype=np.int32)
        n = np.zeros(cap, dtype=np.uint32)
        w = np.zeros(cap, dtype=np.float32)
        p = np.zeros(cap, dtype=np.float32)
        k = self._chk(B.lib().omok_root_children(self.h, game, side, B.iptr(a), n.ctypes.data_as(C.POINTER(C.c_uint32)), B.fptr(w), B.fptr(p), cap))
        return a[:k], n[:k], w[:k], p[:k]

    @property
    def ply(self):
        return self._chk(B.lib().omok_current_ply(self.h))

    @property
    def alive_count(self):
        return self._chk(B.lib().omok_alive_count(self.h))

    def game_info(self):
        alive = np.zeros(self.games, dtype=np.uint8)
        status = np.zeros(self.games, dtype=np.uint8)
        plies = np.zeros(self.games, dtype=np.int32)
        self._chk(B.lib().omok_game_info(self.h, B.u8ptr(alive), B.u8ptr(status), B.iptr(plies)))
        return alive, status, plies

    def game_log(self, on=True):
        """omok_game_log_enable: True = keep a move log from the next reset on (19 B per game and cell, allocated now), False = stop and free.
        Changes no result; run_slots refuses while it is on (run_slots_logged is the slots-mode run that keeps the moves)."""
        self._chk(B.lib().omok_game_log_enable(self.h, int(bool(on))))

    def game_records(self, first_game=0, games=None, meta=None):
        """the move log of games [first_game, first_game + games) since the last reset (omok_game_log_read) with their status and plies
        (omok_game_info) as a records.GameRecords"""
        from . import records as R
        games = self.games - first_game if games is None else int(games)
        rows = max(games, 0)  # (a range the library rejects is left to the library)
        u32p = C.POINTER(C.c_uint32)
        start = np.zeros((rows, self.hw), dtype=np.uint8)
        lengths = np.zeros(rows, dtype=np.int32)
        moves = np.zeros((rows, self.hw), dtype=np.uint16)
        root_n, child_n = np.zeros((rows, self.hw), dtype=np.uint32), np.zeros((rows, self.hw), dtype=np.uint32)
        root_w, child_w = np.zeros((rows, self.hw), dtype=np.float32), np.zeros((rows, self.hw), dtype=np.float32)
        self._chk(B.lib().omok_game_log_read(self.h, int(first_game), games, B.u8ptr(start), B.iptr(lengths), moves.ctypes.data_as(C.POINTER(C.c_uint16)),
                                             root_n.ctypes.data_as(u32p), B.fptr(root_w), child_n.ctypes.data_as(u32p), B.fptr(child_w)))
        _, status, plies = self.game_info()
        return R.GameRecords.from_log(self.n, start, lengths, moves, root_n, root_w, child_n, child_w,
                                      status[first_game:first_game + games], plies[first_game:first_game + games], meta)

    def execute(self, count, batch_size, epsilon=0.25, alpha=0.03):
        self._chk(B.lib().omok_execute(self.h, count, batch_size, epsilon, alpha))

    def execute_shared(self, count, batch_size, epsilon=0.25, alpha=0.03, waves=8):
        """MCTSExecutor::run: one tree (games = 1) searched by `waves` wavefronts"""
        self._chk(B.lib().omok_execute_shared(self.h, count, batch_size, epsilon, alpha, waves))

    def execute_shared_recorded(self, count, batch_size, epsilon=0.25, alpha=0.03, waves=8):
        """omok_execute_shared_recorded: returns a list of groups, each (sim_order [wave ids], backup_order [wave ids], p [req][HW], v [req])."""
        rounds = -(-count // batch_size)
        groups = -(-rounds // waves)
        per = waves * batch_size
        so = np.zeros((groups, per), dtype=np.uint8)
        bo = np.zeros((groups, per), dtype=np.uint8)
        gc = np.zeros((groups, 3), dtype=np.int32)
        cap = rounds * batch_size
        p = np.zeros((cap, self.hw), dtype=np.float32)
        v = np.zeros(cap, dtype=np.float32)
        ng, nr = C.c_int32(), C.c_int32()
        self._chk(B.lib().omok_execute_shared_recorded(self.h, count, batch_size, epsilon, alpha, waves, B.u8ptr(so), B.u8ptr(bo), B.iptr(gc), B.fptr(p), B.fptr(v),
                                                       cap, C.byref(ng), C.byref(nr)))
        out, base = [], 0
        for g in range(ng.value):
            ns, nb, nq = (int(x) for x in gc[g])
            out.append((so[g, :ns].copy(), bo[g, :nb].copy(), p[base:base + nq].copy(), v[base:base + nq].copy()))
            base += nq
        return out

    def sample_actions(self, temperature=1.0, threshold=30):
        a = np.zeros(self.games, dtype=np.int32)
        self._chk(B.lib().omok_sample_actions(self.h, temperature, threshold, B.iptr(a)))
        return a

    def advance(self):
        self._chk(B.lib().omok_advance(self.h))

    def run(self, count, batch_size, epsilon=0.25, alpha=0.03, temperature=1.0, threshold=30, max_plies=0):
        s = (C.c_double * len(B.STAT_NAMES))()
        self._chk(B.lib().omok_selfplay_run(self.h, count, batch_size, epsilon, alpha, temperature, threshold, max_plies, s))
        return dict(zip(B.STAT_NAMES, list(s)))

    def run_slots(self, total_games, count, batch_size, records_ptr, cap_records, epsilon=0.25, alpha=0.03, temperature=1.0, threshold=30):
        """Slots mode (omok_selfplay_run_slots): `total_games` games on the engine's slots, finished slots restarted with the next game
        index.  `records_ptr` = device buffer of cap_records x replay_record_bytes (e.g. a torch uint8 tensor's data_ptr()).
        Returns (stats, n_records, offsets[int64], lengths[int32], status[int32]) indexed by game index."""
        s = (C.c_double * len(B.STAT_NAMES))()
        off = np.zeros(total_games, dtype=np.int64)
        ln = np.zeros(total_games, dtype=np.int32)
        stt = np.zeros(total_games, dtype=np.int32)
        n = C.c_int64()
        self._chk(B.lib().omok_selfplay_run_slots(self.h, total_games, count, batch_size, epsilon, alpha, temperature, threshold,
                                                  C.c_void_p(records_ptr), cap_records, off.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  ln.ctypes.data_as(C.POINTER(C.c_int32)), stt.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  C.byref(n), s))
        return dict(zip(B.STAT_NAMES, list(s))), int(n.value), off, ln, stt

    def run_slots_logged(self, total_games, count, batch_size, records_ptr, cap_records, log_ptr, epsilon=0.25, alpha=0.03, temperature=1.0, threshold=30):
        """run_slots with the move log packed out beside the records (omok_selfplay_run_slots_logged; game_log(True) and a reset first):
        `log_ptr` = device buffer of cap_records x 20 B, entry offsets[i] + p = move p of game index i (slots_game_records reads it).
        Returns what run_slots returns; afterwards game_records() is refused until the next reset."""
        s = (C.c_double * len(B.STAT_NAMES))()
        off = np.zeros(total_games, dtype=np.int64)
        ln = np.zeros(total_games, dtype=np.int32)
        stt = np.zeros(total_games, dtype=np.int32)
        n = C.c_int64()
        self._chk(B.lib().omok_selfplay_run_slots_logged(self.h, total_games, count, batch_size, epsilon, alpha, temperature, threshold,
                                                         C.c_void_p(records_ptr), cap_records, C.c_void_p(log_ptr), off.ctypes.data_as(C.POINTER(C.c_int64)),
                                                         ln.ctypes.data_as(C.POINTER(C.c_int32)), stt.ctypes.data_as(C.POINTER(C.c_int32)),
                                                         C.byref(n), s))
        return dict(zip(B.STAT_NAMES, list(s))), int(n.value), off, ln, stt

    def slots_game_records(self, log, n_records, offsets, lengths, status, meta=None):
        """the games of a run_slots_logged as a records.GameRecords in game-index order: `log` = the log buffer (a torch uint8 tensor on
        the device, or its device pointer), n_records / offsets / lengths / status = what the run returned.  One device-to-host copy."""
        import torch
        from . import records as R
        nbytes = int(n_records) * R.ENTRY_BYTES
        if isinstance(log, torch.Tensor):
            host = log.reshape(-1)[:nbytes].cpu().numpy()
        else:
            host = np.empty(nbytes, dtype=np.uint8)
            if nbytes:
                err = C.CDLL("libamdhip64.so").hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(int(log)), C.c_size_t(nbytes), 2)  # 2 = hipMemcpyDeviceToHost
                if int(err) != 0:
                    raise RuntimeError(f"slots_game_records: the device-to-host copy of {nbytes} bytes failed ({err})")
        return R.GameRecords.from_packed(self.n, host.reshape(int(n_records), R.ENTRY_BYTES), offsets, lengths, status, meta)

    # ---- step-wise (parity tests) -----------------------------------------------------------
    def round_generate(self, rnd, batch_size, epsilon=0.25, alpha=0.03):
        n = C.c_int32()
        self._chk(B.lib().omok_round_generate(self.h, rnd, batch_size, epsilon, alpha, C.byref(n)))
        self._nreq = n.value
        return n.value

    def round_inputs(self):
        out = np.zeros((self._nreq, 3 * self.hw), dtype=np.float32)
        if self._nreq:
            self._chk(B.lib().omok_round_inputs(self.h, B.fptr(out)))
        return out

    def round_eval(self):
        self._chk(B.lib().omok_round_eval(self.h))
        p = np.zeros((self._nreq, self.hw), dtype=np.float32)
        v = np.zeros(self._nreq, dtype=np.float32)
        if self._nreq:
            self._chk(B.lib().omok_round_outputs(self.h, B.fptr(p), B.fptr(v)))
        return p, v

    def round_logits(self):
        """pre-softmax policy logits [n][HW] and pre-tanh values [n] of the round just evaluated (call between round_eval and round_scatter)"""
        lg = np.zeros((self._nreq, self.hw), dtype=np.float32)
        vp = np.zeros(self._nreq, dtype=np.float32)
        if self._nreq:
            self._chk(B.lib().omok_round_logits(self.h, B.fptr(lg), B.fptr(vp)))
        return lg, vp

    def round_inject(self, p, v):
        p = np.ascontiguousarray(p, dtype=np.float32)
        v = np.ascontiguousarray(v, dtype=np.float32)
        if self._nreq:
            self._chk(B.lib().omok_round_inject(self.h, B.fptr(p), B.fptr(v)))

    def round_scatter(self):
        self._chk(B.lib().omok_round_scatter(self.h))

    def mirror_generate(self):
        n = C.c_int32()
        self._chk(B.lib().omok_mirror_generate(self.h, C.byref(n)))
        self._nmir = n.value
        return n.value

    def mirror_inputs(self):
        out = np.zeros((self._nmir, 3 * self.hw), dtype=np.float32)
        if self._nmir:
            self._chk(B.lib().omok_mirror_inputs(self.h, B.fptr(out)))
        return out

    def mirror_eval(self):
        self._chk(B.lib().omok_mirror_eval(self.h))
        p = np.zeros((self._nmir, self.hw), dtype=np.float32)
        if self._nmir:
            self._chk(B.lib().omok_mirror_outputs(self.h, B.fptr(p)))
        return p

    def mirror_inject(self, p):
        p = np.ascontiguousarray(p, dtype=np.float32)
        if self._nmir:
            self._chk(B.lib().omok_mirror_inject(self.h, B.fptr(p)))

    def mirror_apply(self):
        self._chk(B.lib().omok_mirror_apply(self.h))

    # ---- inspection -------------------------------------------------------------------------
    def tree_dump(self, game, side):
        cap = self.eng.max_nodes
        ints = np.zeros((cap, 8), dtype=np.int32)
        floats = np.zeros((cap, 1 + self.hw), dtype=np.float32)
        n = self._chk(B.lib().omok_tree_dump(self.h, game, side, B.iptr(ints), B.fptr(floats), cap))
        return ints[:n].copy(), floats[:n].copy()

    def tree_root(self, game, side):
        rn, rw, nn, nt = C.c_uint32(), C.c_float(), C.c_int32(), C.c_int32()
        self._chk(B.lib().omok_tree_root(self.h, game, side, C.byref(rn), C.byref(rw), C.byref(nn), C.byref(nt)))
        return rn.value, rw.value, nn.value, nt.value

    def replay(self, game):
        cap = self.hw
        boards = np.zeros((cap, self.hw), dtype=np.uint8)
        turns = np.zeros(cap, dtype=np.uint8)
        pi = np.zeros((cap, self.hw), dtype=np.float32)
        z = np.zeros(cap, dtype=np.float32)
        n = self._chk(B.lib().omok_replay_game(self.h, game, B.u8ptr(boards), B.u8ptr(turns), B.fptr(pi), B.fptr(z), cap))
        return boards[:n], turns[:n], pi[:n], z[:n]

    def replay_augmented(self, game):
        """Trainer::train replay post-processing for one game (src/trainer.rs:207-324): z back-fill, then the game's
        transitions followed by their 5 augmentations each (rot90, rot180, rot270, flipH, flipV)."""
        cap = 6 * self.hw
        boards = np.zeros((cap, self.hw), dtype=np.uint8)
        turns = np.zeros(cap, dtype=np.uint8)
        pi = np.zeros((cap, self.hw), dtype=np.float32)
        z = np.zeros(cap, dtype=np.float32)
        n = self._chk(B.lib().omok_replay_augmented_game(self.h, game, B.u8ptr(boards), B.u8ptr(turns), B.fptr(pi), B.fptr(z), cap))
        return boards[:n], turns[:n], pi[:n], z[:n]

    def replay_augment_into(self, dev_ptr, cap_records):
        n = B.lib().omok_replay_augment_dev(self.h, C.c_void_p(dev_ptr), cap_records)
        if n < 0:
            raise B.OmokError(int(n), B.lib().omok_last_error(self.h).decode())
        return int(n)

    def replay_record_bytes(self):
        return self._chk(B.lib().omok_replay_record_bytes(self.h))

    def replay_pack_into(self, dev_ptr, cap_records):
        n = B.lib().omok_replay_pack_dev(self.h, C.c_void_p(dev_ptr), cap_records)
        if n < 0:
            raise B.OmokError(int(n), B.lib().omok_last_error(self.h).decode())
        return int(n)


def analyze(engine, boards, count, batch_size, epsilon=0.0, alpha=0.03):
    """Batched analysis: searches the given positions (boards [G][HW] Stone bytes, G = the engine's games, equal stone counts) with `count`
    simulations each, from fresh agents (SelfPlay.reset_from).  Returns (pi [G][HW] = Agent::compute_policy of the side to move, root_n [G],
    root_w [G]).  epsilon = 0: no Dirichlet noise on the roots."""
    sp = SelfPlay(engine)
    sp.reset_from(boards)
    sp.execute(count, batch_size, epsilon, alpha)
    pi, _ = sp.compute_policy()
    n, w = sp.root_stats()
    return pi, n, w
