"""One-GPU (or one-process-per-GPU) mirror of Trainer::train (src/trainer.rs:69-386) over the HIP engine.

Per iteration, like the reference: clear the replay memory (:77-78), play `episode_count` self-play games (:81-205, on
the engine), back-fill z and augment (:207-324, on the device), cap the memory at `replay_memory_size` (:326-328), run
`parameter_update_count` training steps on `parameter_update_batch_size` transitions (:329-357), save the model
(`saves/<model_name>`, :375, ModelIO format), and every `evaluate_every` iterations play `evaluate_games` games against the scripted
naive player (:380-394, 487-603: `Trainer.evaluate`; Parameters.evaluate_opponent = "threat" puts the threat-aware player in its place).  Plots (:371-376) are not part of this mirror.  Parameters and defaults:
src/config.rs:83-110 (episode_count 50, evaluate_count 600, test_evaluate_count 800, ...).
Multi-GPU: every rank plays its own `episode_count` games (global ids rank*episode_count + g) and trains data-parallel
(gradients averaged per step: by the torch phase's all-reduce, or by the engine in rank order with train_backend="hip_dp"), so all ranks
hold identical weights after every iteration.
Parameters.selfplay_slots = S > 0 plays the iteration's `episode_count` games in slots mode (omok_selfplay_run_slots) on an engine of
min(S, episode_count) games: a slot whose game is over takes the next game index, so the trees resident in memory no longer grow with
episode_count.  The raw records it hands back are back-filled and augmented on the device by omok_replay_augment_records_dev into the
game-index order the episode path produces; everything after that is the same code.  0 (the default) is the episode path.
Trainer(save_selfplay_games=DIR) keeps every self-play game: each iteration writes DIR/selfplay_iter{iteration:06d}.rank{rank}.npz, a
records.GameRecords (every move with the mover's root and chosen-child statistics; `python -m omok_ai_amd.records show FILE --game i`), from the
engine's move log on the episode path and from omok_selfplay_run_slots_logged in slots mode: the same arrays either way, and the same weights as without it.
"""
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import api, dist, weights
from . import train as T


@dataclass
class Parameters:  # src/config.rs:83-110
    model_name: str = "alpha-zero"
    replay_memory_size: int = 600_000
    episode_count: int = 50
    evaluate_count: int = 600
    evaluate_batch_size: int = 16
    epsilon: float = 0.25
    alpha: float = 0.03
    temperature: float = 1.0
    temperature_threshold: int = 30
    parameter_update_count: int = 600
    parameter_update_batch_size: int = 128
    test_evaluate_count: int = 800  # simulations per move of the net in the evaluation games (src/config.rs:31,103)
    evaluate_every: int = 10        # `iteration % 10 == 0` (src/trainer.rs:380)
    evaluate_games: int = 100       # play_against_naive_player(100, ..) (:384)
    selfplay_slots: int = 0         # 0 = one episode of episode_count games (omok_selfplay_run); S > 0 = the same games in slots mode on min(S, episode_count) slots (omok_selfplay_run_slots; no reference counterpart)
    evaluate_opponent: str = "naive"  # the scripted player of the evaluation games: "naive" (the reference's, :508-534), "threat" (the threat-aware player, OMOK_OPP_THREAT), "vcf" (that player with the forced-win solver, OMOK_OPP_VCF), "guard" (the defending player, OMOK_OPP_GUARD) or "random" (:452-455)
    train_backend: str = "torch"    # the training phase (:329-357): "torch" = autograd (train.py), "hip" = the engine's native step (omok_train_run, one rank), "hip_dp" = the native step in two halves with the ranks' gradients averaged in between (any world size)


class Trainer:
    def __init__(self, params=None, board_size=15, seed=0, save_dir="saves", max_nodes=None, max_tables=None, precision_rows=256, precision_search_rounds=True,
                 save_selfplay_games=None):
        self.p = params or Parameters()
        self.n = board_size
        self.rank, self.local_rank, self.world = dist.shard_info()
        if self.p.train_backend not in ("torch", "hip", "hip_dp"):
            raise ValueError(f"train_backend {self.p.train_backend!r}: expected \"torch\", \"hip\" or \"hip_dp\"")
        if self.p.evaluate_opponent not in api.B.SCRIPTED_PLAYERS:
            raise ValueError(f"evaluate_opponent {self.p.evaluate_opponent!r}: expected \"naive\", \"threat\", \"vcf\", \"guard\" or \"random\"")
        if self.p.train_backend == "hip" and self.world > 1:
            raise RuntimeError("train_backend=\"hip\" runs on one rank only: the native step does not average gradients over ranks "
                               f"(world size {self.world}); use train_backend=\"hip_dp\" or \"torch\" for data-parallel training")
        if self.p.selfplay_slots < 0:
            raise ValueError(f"selfplay_slots {self.p.selfplay_slots}: expected 0 (episode) or a number of slots > 0")
        self.slots = min(self.p.selfplay_slots, self.p.episode_count)  # 0 = the episode path
        self._raw = None  # slots mode: the raw records of an iteration, episode_count * N * N at the most (allocated by the first iteration)
        self.device = f"cuda:{self.local_rank}"
        self.save_dir = save_dir
        self.precision_rows = precision_rows  # independent check of the net outputs after every weight update (0 = off)
        self.precision_search_rounds = precision_search_rounds  # ... and of the search rounds' own path (sibling base + difference rows)
        self.last_precision = None
        self.seed = seed
        self.last_evaluation = None  # result of the last games against the scripted player evaluate_opponent (evaluate)
        sims = -(-self.p.evaluate_count // self.p.evaluate_batch_size) * self.p.evaluate_batch_size
        max_nodes = max_nodes or min(16384, 4 * sims + 1024)
        self.engine = api.Engine(board_size=board_size, games=self.slots or self.p.episode_count, max_nodes=max_nodes,
                                 max_tables=max_tables or max(256, max_nodes // 4), max_batch_k=self.p.evaluate_batch_size,
                                 device=self.local_rank, seed=seed, game_offset=dist.game_offset(self.rank, self.p.episode_count))
        path = os.path.join(save_dir, self.p.model_name)
        if os.path.exists(path):  # Trainer::new -> this.load(model_name) (:63-65, :628-636)
            self.engine.load(path)
            tensors = self._engine_tensors()
        else:
            tensors = weights.init_random(board_size, seed=seed)
            self.engine.load_weights(tensors)
        self.phase = T.TrainPhase(board_size, tensors, self.device)  # the optimizer state lives across iterations like the session's
        if self.p.train_backend in ("hip", "hip_dp"):  # ... here in the engine; self.phase.net only mirrors the variables (precision check, tests)
            self.engine.train_begin(self.p.parameter_update_batch_size)
        self.selfplay = api.SelfPlay(self.engine)
        self.save_selfplay_games = save_selfplay_games  # a directory: every iteration's self-play games are written there (None = no move log is kept)
        self._raw_log = None  # slots mode with the games kept: the packed move log beside _raw, 20 B per record
        if save_selfplay_games is not None:
            self.selfplay.game_log(True)  # from the next reset on: every iteration starts with one
        self.iteration = 0
        it_path = path + ".iteration"  # (not in the reference, whose thread_rng is fresh on every start): a resumed run must
        if os.path.exists(path) and os.path.exists(it_path):  # not replay the RNG streams of the iterations it has already played;
            self.iteration = int(open(it_path).read().strip() or 0)  # a counter without its checkpoint is stale and ignored

    def _engine_tensors(self):
        tmp = os.path.join(self.save_dir, f".{self.p.model_name}.rank{self.rank}.tmp")
        self.engine.save(tmp)
        from . import model_file
        tensors = model_file.load(tmp)[1]
        os.remove(tmp)
        return tensors

    def _mirror_engine_weights(self):
        with torch.no_grad():
            for var, t in zip(self.phase.net.vars, self.engine.read_weights()):
                var.copy_(torch.from_numpy(t).reshape(var.shape))

    def _train_data_parallel(self, records):
        """The update loop (:329-357) with the native step cut in two: every rank takes the gradients of a batch of ITS records (key = seed +
        iteration * 7919 + rank: at rank 0 the key of "hip"), the ranks' slabs are all-gathered, and every engine applies their rank-order
        average (omok_train_apply), so the replicas stay bit-equal.  Every rank runs parameter_update_count steps whatever its record count (>= 1),
        so the collectives pair up; a rank without a single record (unreachable with episode_count >= 1: a game records its first move) is
        found on ALL ranks before the loop, so that none is left waiting in a collective.  Returns the log line's means of the last <= 100 steps, summed in fp32 in step order like omok_train_run."""
        p, eng = self.p, self.engine
        n_records, key = records.shape[0], self.seed + self.iteration * 7919 + self.rank
        if dist.min_over_ranks(n_records, self.device) < 1:
            raise RuntimeError("train_backend=\"hip_dp\": a rank holds no replay record, so it cannot take part in the updates")
        slab = torch.empty(eng.train_gradient_count(), dtype=torch.float32, device=self.device)
        counted = min(p.parameter_update_count, 100)
        sums = np.zeros(3, np.float32)
        for s in range(p.parameter_update_count):
            idx = eng.train_batch_indices(n_records, p.parameter_update_batch_size, key, s)
            eng.train_backward(records.data_ptr(), n_records, idx, slab.data_ptr())
            gathered = dist.gather_gradients(slab)
            if gathered.is_cuda:
                torch.cuda.current_stream(gathered.device).synchronize()  # the engine reads the slabs on its own stream
            step = eng.train_apply(gathered.data_ptr(), self.world)
            if s >= p.parameter_update_count - counted:
                sums += np.asarray(step, np.float32)
        eng.commit()
        v_loss, p_loss, loss = (float(v) for v in sums / np.float32(max(counted, 1)))
        return v_loss, p_loss, loss

    def _save_selfplay_games(self, read, log):
        """this iteration's self-play games (read(meta) -> records.GameRecords) into save_selfplay_games; like the precision check, a failure
        is logged, never fatal: the training state does not depend on the file"""
        p = self.p
        try:
            os.makedirs(self.save_selfplay_games, exist_ok=True)
            meta = {"kind": "selfplay", "iteration": self.iteration, "seed": self.seed, "sims": p.evaluate_count, "batch": p.evaluate_batch_size,
                    "slots": self.slots, "game_offset": dist.game_offset(self.rank, p.episode_count)}
            read(meta).save(os.path.join(self.save_selfplay_games, f"selfplay_iter{self.iteration:06d}.rank{self.rank}.npz"))
        except Exception as ex:  # noqa: BLE001
            log(f"[iter={self.iteration}] WARNING: the self-play games were not saved: {ex!r}")

    def train(self, iteration_count, log=print):
        p = self.p
        rec = self.selfplay.replay_record_bytes()
        for _ in range(iteration_count):
            self.selfplay.set_episode(self.iteration)  # RNG stream of this iteration (key = seed + iteration * golden ratio)
            self.iteration += 1
            self.engine.reset_stats()  # (per-iteration counters in the log line)
            self.selfplay.reset()  # fresh agents; the engine's replay buffer is cleared with them (:77-93)
            if self.slots:  # the same games by index (keyed by game_offset + index) on fewer slots; raw records in completion order
                cap = p.episode_count * self.n * self.n
                if self._raw is None:
                    self._raw = torch.empty(cap * rec, dtype=torch.uint8, device=self.device)
                if self.save_selfplay_games is None:
                    stats, n_raw, offsets, lengths, _ = self.selfplay.run_slots(p.episode_count, p.evaluate_count, p.evaluate_batch_size, self._raw.data_ptr(), cap,
                                                                                p.epsilon, p.alpha, p.temperature, p.temperature_threshold)
                else:
                    if self._raw_log is None:
                        self._raw_log = torch.empty(cap * api.B.lib().omok_game_log_entry_bytes(), dtype=torch.uint8, device=self.device)
                    stats, n_raw, offsets, lengths, status = self.selfplay.run_slots_logged(p.episode_count, p.evaluate_count, p.evaluate_batch_size, self._raw.data_ptr(),
                                                                                            cap, self._raw_log.data_ptr(), p.epsilon, p.alpha, p.temperature,
                                                                                            p.temperature_threshold)
                    self._save_selfplay_games(lambda meta: self.selfplay.slots_game_records(self._raw_log, n_raw, offsets, lengths, status, meta), log)
                total = 6 * int(lengths.sum())
                buf = torch.empty(max(total, 1) * rec, dtype=torch.uint8, device=self.device)
                got = self.engine.replay_augment_records(self._raw.data_ptr(), n_raw, offsets, lengths, buf.data_ptr(), total)
            else:
                stats = self.selfplay.run(p.evaluate_count, p.evaluate_batch_size, p.epsilon, p.alpha, p.temperature,
                                          p.temperature_threshold, 0)
                if self.save_selfplay_games is not None:
                    self._save_selfplay_games(lambda meta: self.selfplay.game_records(meta=meta), log)
                _, _, plies = self.selfplay.game_info()
                total = 6 * int(plies.sum())
                buf = torch.empty(max(total, 1) * rec, dtype=torch.uint8, device=self.device)
                got = self.selfplay.replay_augment_into(buf.data_ptr(), total)
            records = buf[: got * rec].reshape(got, rec)
            if got > p.replay_memory_size:  # pop_front until the memory fits (:326-328)
                records = records[got - p.replay_memory_size:]
            if p.train_backend == "hip":  # the whole phase in one call on the engine's own fp32 variables; it commits them itself
                v_loss, p_loss, loss = self.engine.train_run(records.data_ptr(), records.shape[0], p.parameter_update_count,
                                                             p.parameter_update_batch_size, key=self.seed + self.iteration * 7919)
                self._mirror_engine_weights()
            elif p.train_backend == "hip_dp":
                v_loss, p_loss, loss = self._train_data_parallel(records)
                self._mirror_engine_weights()
            else:
                v_loss, p_loss, loss = self.phase.run(records, p.parameter_update_count, p.parameter_update_batch_size,
                                                      seed=self.iteration * 7919 + self.rank)
                self.phase.push_to(self.engine)
            # new weights -> omok_net_commit -> the engine re-measured fc0's operand format on its probe set; the probe's
            # figures are kept for the log, and the outputs are checked independently below (a probe is a measurement, not a proof)
            st = self.engine.stats()
            fmt = api.B.FC0_FORMATS[int(st["fc0_format"])]  # the format THIS engine runs (its probe saw plain rows and, if its rounds are large enough, a sibling round)
            self.last_precision = {"fc0_format": fmt, "probe_rows": int(st["probe_rows"]), "probe_outside": int(st["probe_outside"]),
                                   "probe_fp6": (st["probe_dp_fp6"], st["probe_dv_fp6"]), "probe_f16": (st["probe_dp_f16"], st["probe_dv_f16"])}
            if self.precision_rows > 0 and fmt != "f32":  # independent check on rows of this iteration's replay buffer (spread over the buffer); on by default
                # The check engines are FORCED into the training engine's format: left to their own probes they would validate whatever a 64-game engine chooses
                # (never mixed).  A failure of the check (e.g. no memory for its engines) is logged, never fatal: the training state above is already consistent.
                try:
                    from . import precision
                    forced = precision.FORCED_MODE[fmt]
                    idx = torch.linspace(0, records.shape[0] - 1, min(self.precision_rows, records.shape[0]), device=records.device).long()
                    x, _, _ = T.decode_records(records[idx], self.n)
                    chk = precision.measure(self.phase.net.tensors(), self.n, x.reshape(x.shape[0], -1).cpu().numpy(), device=self.local_rank,
                                            batch_k=p.evaluate_batch_size, net_mode=forced)
                    self.last_precision["check"] = chk
                    if chk["fc0_format"] != fmt:
                        log(f"[iter={self.iteration}] WARNING: the precision check ran in format {chk['fc0_format']}, the engine runs {fmt}")
                    if not chk["within_contract"]:
                        log(f"[iter={self.iteration}] WARNING: net outputs differ from the fp32 kernels by |dp| {chk['max_dp']:.2e} |dv| {chk['max_dv']:.2e} "
                            f"(contract 1e-3) in format {chk['fc0_format']}")
                    if self.precision_search_rounds:  # the path the search rounds take (base row + 7x7-window difference rows), on rounds of the new net
                        games = precision.difference_path_games(self.n, p.evaluate_batch_size)  # (enough rows per round for the difference path at either board size)
                        sr = precision.measure_search_rounds(self.phase.net.tensors(), self.n, games=games, batch_k=p.evaluate_batch_size, rounds=2, plies=1,
                                                             device=self.local_rank, seed=self.iteration, net_mode=forced)
                        self.last_precision["search_rounds"] = sr
                        if sr["difference_path_rounds"] == 0:
                            log(f"[iter={self.iteration}] note: no round of the search-round check took the difference path ({sr['rows']} rows checked on the copy path)")
                        if not sr["within_contract"]:
                            log(f"[iter={self.iteration}] WARNING: search-round outputs differ from the fp32 kernels by |dp| {sr['max_dp']:.2e} |dv| {sr['max_dv']:.2e} "
                                f"(contract 1e-3) on {sr['rows']} rows")
                except Exception as ex:  # noqa: BLE001
                    self.last_precision["check_error"] = repr(ex)
                    log(f"[iter={self.iteration}] WARNING: the precision check did not run: {ex!r}")
            if self.rank == 0:  # Trainer::save (:605-626)
                os.makedirs(self.save_dir, exist_ok=True)
                final = os.path.join(self.save_dir, p.model_name)  # counter first, then the weights, each by rename: a crash in between
                with open(final + ".iteration.tmp", "w") as f:     # leaves the OLD weights with the NEW counter (an RNG stream is skipped,
                    f.write(str(self.iteration))                   # never replayed)
                os.replace(final + ".iteration.tmp", final + ".iteration")
                self.engine.save(final + ".tmp")
                os.replace(final + ".tmp", final)
            versus = ""
            if self.rank == 0 and p.evaluate_every > 0 and (self.iteration - 1) % p.evaluate_every == 0:  # `iteration % 10 == 0`, 0-based (:380)
                try:  # like the precision check: a failure (e.g. no memory for the engine) is logged, never fatal
                    black, white, draw = self.evaluate()
                    versus = (f" | {p.evaluate_games} games against the {p.evaluate_opponent} player ({p.evaluate_opponent} = Black, net = White, {p.test_evaluate_count} simulations): "
                              f"black_win={black} white_win={white} draw={draw}")
                except Exception as ex:  # noqa: BLE001
                    self.last_evaluation = {"iteration": self.iteration, "error": repr(ex)}
                    log(f"[iter={self.iteration}] WARNING: the games against the {p.evaluate_opponent} player did not run: {ex!r}")
            log(f"[iter={self.iteration}] games={int(stats['finished'])} transitions={got} loss={loss:.4f} "
                f"[v_loss={v_loss:.4f}, p_loss={p_loss:.4f}]" + versus)
        return v_loss, p_loss, loss

    def evaluate(self, openings=None, save_games=None):
        """play_against_naive_player (src/trainer.rs:487-603) with the weights just saved: `evaluate_games` games on an engine of its own
        (arenas sized for `test_evaluate_count`), the scripted naive player is Black and moves first, the net answers as White with
        `test_evaluate_count` simulations and sample_action(Best).  The reference prints Black's wins as "Win" although Black is the naive
        player (:387-393); train() logs the three counts by colour, on the iteration's line.  openings: None = every game from the empty board
        like the reference, or [evaluate_games, HW] Stone bytes = the position each game starts from (equal stone counts; the side the stone
        count gives moves first, the naive player stays Black).  save_games: a path = the games' records (records.GameRecords: every move, the
        naive player's marked external, with the net's root and chosen-child statistics) are written there as one .npz; None = no move log is
        kept.  Parameters.evaluate_opponent ("naive" by default) names the scripted player: "threat", the threat-aware player of
        include/omok_mi355x.h, keeps telling nets apart that all beat the naive player in every game; it is named in the log line, in
        last_evaluation and in the records' meta.  Returns (black_win, white_win, draw)."""
        p = self.p
        sims = -(-p.test_evaluate_count // p.evaluate_batch_size) * p.evaluate_batch_size
        max_nodes = min(16384, 4 * sims + 1024)
        eng = api.Engine(board_size=self.n, games=p.evaluate_games, max_nodes=max_nodes, max_tables=max(256, max_nodes // 4),
                         max_batch_k=p.evaluate_batch_size, device=self.local_rank, seed=self.seed + 1)  # (seed + 1: streams of its own, not the self-play games')
        try:
            eng.load(os.path.join(self.save_dir, p.model_name))
            sp = api.SelfPlay(eng)
            sp.set_episode(self.iteration - 1)
            if save_games is not None:
                sp.game_log(True)
            if openings is None:
                sp.reset()
            else:
                sp.reset_from(np.ascontiguousarray(openings, dtype=np.uint8).reshape(p.evaluate_games, self.n * self.n))
            (black, white, draw), _ = sp.versus_run(api.B.SCRIPTED_PLAYERS[p.evaluate_opponent], 0, p.test_evaluate_count, p.evaluate_batch_size, p.epsilon, p.alpha)
            if save_games is not None:
                sp.game_records(meta={"kind": "evaluate", "net": os.path.join(self.save_dir, p.model_name), "iteration": self.iteration,
                                      "opponent": p.evaluate_opponent, "opponent_side": 0, "sims": p.test_evaluate_count, "batch": p.evaluate_batch_size,
                                      "seed": self.seed + 1, "openings": openings is not None}).save(save_games)
        finally:
            eng.close()
        self.last_evaluation = {"iteration": self.iteration, "games": p.evaluate_games, "opponent": p.evaluate_opponent, "black_win": black, "white_win": white, "draw": draw}
        return black, white, draw

    def close(self):
        self.engine.close()
