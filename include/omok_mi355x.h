/*
 * omok_mi355x.h — C ABI of the MI355X-native self-play engine (libomok_mi355x.so).
 *
 * Drop-in boundary for the `environment` + `mcts` + `alpha-zero` self-play path of
 * AcrylicShrimp/omok-ai.  The reference has no FFI; the path sits behind Rust crate `pub` APIs.
 * Each entry point below names the reference interface it replaces (file:line in the reference
 * tree).  Plain pointers and sizes only; every buffer is caller-owned host memory unless the
 * name ends in `_dev`.  All device state is owned by the opaque handle.
 *
 * Conventions
 *   - return value: 0 = OK, < 0 = error (OMOK_ERR_*); omok_last_error() gives the text.
 *     Nothing throws or aborts across this boundary (the reference returns Result<_, Status>
 *     / Option and its callers unwrap()).
 *   - enums are the reference's declaration order (environment/src/lib.rs:5-9,22-25,46-51):
 *       Stone {Empty=0, Black=1, White=2}; Turn {Black=0, White=1};
 *       GameStatus {InProgress=0, Draw=1, BlackWin=2, WhiteWin=3}; Option::None -> -1.
 *   - a handle is single-owner (one host thread per GPU); calls block until the work they
 *     describe is complete (mirrors Session::run) unless documented otherwise.
 *   - RNG: the reference is unseeded (thread_rng).  This library defines the stream
 *     (Philox4x32-10, see DESIGN.md "RNG contract"); `seed` and `game_offset` select it.
 */
#ifndef OMOK_MI355X_H
#define OMOK_MI355X_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OMOK_OK 0
#define OMOK_ERR_INVALID (-1)     /* bad argument */
#define OMOK_ERR_HIP (-2)         /* HIP runtime failure (no GPU, OOM, launch error) */
#define OMOK_ERR_STATE (-3)       /* call order violated / net not loaded */
#define OMOK_ERR_OVERFLOW (-4)    /* a tree arena (max_nodes / max_tables) overflowed */
#define OMOK_ERR_ILLEGAL (-5)     /* illegal game operation (Option::None in the reference) */

#define OMOK_MODE_PLAYER 0   /* EnvTurnMode::Player   (alpha-zero/src/encoder.rs:4-8) */
#define OMOK_MODE_OPPONENT 1 /* EnvTurnMode::Opponent */

#define OMOK_NET_F16X3 0 /* split-operand MFMA (x = hi + lo, hi = f16(x): f16 main term + two correction terms, fp32 accumulate).  The
                            correction terms of trunk, fc1 and heads are f16; those of fc0 (68 % of the flops) are block-scaled fp6 (products good to
                            ~2^-15) or f16 (~2^-22, ~2x the fc0 time): omok_net_commit evaluates a fixed probe set of 2048 positions in both
                            formats and with the fp32 kernels and keeps fp6 only while its worst |dp|, |dv| stay within 3e-4 = 0.3 of the
                            1e-3 contract on AgentModel::evaluate_pv's outputs (OMOK_STAT_FC0_FORMAT / OMOK_STAT_PROBE_*) */
#define OMOK_NET_F32 1   /* plain fp32 VALU kernels (debug / A-B reference on the GPU) */
#define OMOK_NET_F16X3_ROWS 2 /* OMOK_NET_F16X3 with every request row evaluated on its own: at board_size 15 the search rounds of
                                 OMOK_NET_F16X3 evaluate sibling requests as one base position + per-child differences, so a
                                 row's p / v carry rounding that depends on its siblings (~5e-5, inside the 1e-3 contract); _ROWS switches
                                 that off (results bit-identical to omok_evaluate_pv of the same position), at ~1.7x the net time */

#define OMOK_NET_F16X3_FP6 3 /* OMOK_NET_F16X3 with fc0's correction terms forced to block-scaled fp6 (no probe) */
#define OMOK_NET_F16X3_F16 4 /* ... forced to f16 */
#define OMOK_NET_F16X3_MIXED 5 /* ... forced to the mixed format: full operand rows (base positions of sibling rounds, single rows, omok_evaluate_pv) with f16
                                  correction terms, the 7x7-window DIFFERENCE rows of sibling rounds -- where the time goes -- with block-scaled fp6 ones: the
                                  quantisation error then scales with the differences, not with the activations */

#define OMOK_MAX_ARENA 16384 /* largest max_nodes / max_tables: node and table indices are 16-bit, and the re-rooting kernel keeps
                               3 B per node + 2 B per table of scratch in LDS (82 KiB at the maximum, inside gfx950's 160 KiB) */

typedef struct omok_engine omok_engine;

typedef struct {
    int32_t board_size;  /* N: 9 (reference, environment/src/lib.rs:70) or 15 */
    int32_t games;       /* G concurrent games = episode_count (src/config.rs:90); two trees each */
    int32_t max_nodes;   /* per-tree node arena, 2 .. OMOK_MAX_ARENA (omok_create rejects more, and sizes whose re-rooting scratch
                            does not fit the device's LDS) */
    int32_t max_tables;  /* per-tree child-table arena, 1 .. OMOK_MAX_ARENA */
    int32_t max_batch_k; /* largest evaluate_batch_size that will be used (<= 64) */
    int32_t device;      /* HIP device ordinal */
    int32_t net_mode;    /* OMOK_NET_* */
    int32_t max_tree_waves; /* 0, or the largest `waves` omok_execute_shared will be called with (<= 16): sizes the net batch */
    uint64_t seed;       /* RNG seed; the Philox key of episode i is seed + i * 0x9E3779B97F4A7C15 (omok_set_episode) */
    int64_t game_offset; /* global id of game 0 (multi-GPU sharding: rank * games) */
} omok_config;

/* ---- lifetime ------------------------------------------------------------------------- */
int omok_create(const omok_config* cfg, omok_engine** out);
void omok_destroy(omok_engine* e);
const char* omok_last_error(const omok_engine* e); /* e may be NULL: error of the last failed create */

/* ---- policy/value net: AgentModel (alpha-zero/src/agent_model.rs:105-134) over Network
 *      (alpha-zero/src/network.rs:51-262).  31 tensors in the reference's variable order
 *      (network.rs:78-79,113-122,149-150,162-163,201-202,240-241), conv kernels HWIO, fc [in,out].
 *      This is also the positional order of ModelIO::load (alpha-zero/src/model_io.rs:92-120). */
int omok_net_num_tensors(void);
int64_t omok_net_tensor_size(const omok_engine* e, int index);
int omok_net_load(omok_engine* e, int index, const float* data, int64_t count);
int omok_net_commit(omok_engine* e); /* pack into MFMA operand layouts; required before any eval */
/* ModelIO::load (alpha-zero/src/model_io.rs:92-120): reads the reference's weights file = bincode 1.3.3 default
 * encoding (little-endian, fixed-width u64 lengths) of SavedData{variable_names: Vec<String>, parameters: Vec<Vec<f32>>}
 * (model_io.rs:20-24).  Loading is POSITIONAL like the reference's zip over `parameters` (:98): names are ignored,
 * parameters beyond the 31st are ignored, fewer than 31 or a length that differs from the variable's element count is an
 * error (the reference fails in session.run / copy_from_slice).  Commits the net on success. */
int omok_net_load_file(omok_engine* e, const char* path);
/* ModelIO::save (model_io.rs:59-90): writes the same format from the tensors currently loaded (canonical names
 * conv_w, conv_b, residual_{i}_..., fc0_w, ...; the reference stores TF-uniquified names and never reads them back). */
int omok_net_save_file(omok_engine* e, const char* path);
/* ---- second net slot: the model of the second agent of benchmark/src/main.rs:14-108 (each Agent of benchmark/src/agent.rs holds its own
 *      AgentModel).  Same tensors, same life cycle and the same commit-time fc0 format probe (net_mode of the engine) as net 1 above; the
 *      slot's device buffers are allocated on its first load.  Only match episodes (omok_match_reset) evaluate it: every other entry point
 *      uses net 1.  The omok_debug_* switches act on net 1 only (net 2 keeps their defaults), and every OMOK_STAT_* figure that describes a
 *      net -- fc0 format and probe, children-kernel launches, the work counters -- describes net 1 (in a match: net 1's share of the rows);
 *      net 2's commit outcome and the rows each net evaluated are in omok_net2_info. */
int omok_net2_load(omok_engine* e, int index, const float* data, int64_t count);
int omok_net2_commit(omok_engine* e);
/* ModelIO::load (model_io.rs:92-120) into net 2, as omok_net_load_file; commits net 2 on success */
int omok_net2_load_file(omok_engine* e, const char* path);
/* Net 2's commit outcome (OMOK_STAT_FC0_FORMAT / OMOK_STAT_PROBE_OUTSIDE keep describing net 1): *fc0_format = -1 (fp32 kernels), 0 fp6,
 * 1 f16, 2 mixed; *probe_outside as OMOK_STAT_PROBE_OUTSIDE.  evals [2] (may be NULL): rows evaluated by net 1 / net 2 in match episodes
 * since omok_reset_stats (search rounds and mirror evaluations).  Each pointer may be NULL.  OMOK_ERR_STATE before omok_net2_commit. */
int omok_net2_info(omok_engine* e, int32_t* fc0_format, int32_t* probe_outside, double* evals);
/* AgentModel::evaluate_pv (agent_model.rs:116-134): in [B][N][N][3] f32 (encoder.rs layout),
 * p [B][N*N] softmax probabilities, v [B] tanh.  evaluate_p (:105-114) = same with v NULL. */
int omok_evaluate_pv(omok_engine* e, const float* in, int32_t batch, float* p, float* v);
/* The same forward, returning what sits in front of the last two ops of the graph: logits [B][N*N] = input of the Softmax
 * (network.rs:236-247), vpre [B] = input of the Tanh (network.rs:197-200; may be NULL).  Precision evidence / debugging: the
 * reference API has no such call. */
int omok_evaluate_logits(omok_engine* e, const float* in, int32_t batch, float* logits, float* vpre);

/* ---- environment crate on device (environment/src/lib.rs:62-166), batched.
 *      Plays `len` moves per row from Environment::new(); status_out[b][i] is the
 *      Option<GameStatus> of move i (-1 = None: occupied cell, the board is left unchanged).
 *      boards_out [B][N*N] Stone bytes, turns_out [B], legal_out [B] (legal_move_count). */
int omok_env_play(omok_engine* e, const int32_t* moves, int32_t batch, int32_t len,
                  int32_t* status_out, uint8_t* boards_out, uint8_t* turns_out, uint16_t* legal_out);
/* encode_nn_input (alpha-zero/src/encoder.rs:10-46) for `batch` environments given as
 * Stone-byte boards + side to move; out [batch][N][N][3] f32. */
int omok_encode_nn_input(omok_engine* e, const uint8_t* boards, const uint8_t* turns, int32_t batch,
                         int32_t mode, float* out);

/* Environment::place_stone (environment/src/lib.rs:104-166) on `batch` caller-held environments: boards [B][N*N] Stone bytes,
 * turns [B], legal [B] (legal_move_count) are updated in place; status_out[b] = Option<GameStatus> (-1 = None: the cell is
 * occupied or out of range and environment b is left unchanged).  batch = 1 is the scalar call of the Rust API. */
int omok_env_place_stone(omok_engine* e, uint8_t* boards, uint8_t* turns, uint16_t* legal, const int32_t* actions,
                         int32_t batch, int32_t* status_out);

/* Is a caller-supplied board a position a game can be in?  Extends Environment (environment/src/lib.rs:62-166), which can only be reached
 * move by move from Environment::new() (:73-79): boards [B][N*N] bytes, verdict_out[b] = the first that applies of
 *   1  a byte that is not a Stone (> 2);
 *   2  stone counts that no alternating game from Environment::new() produces (neither black = white nor black = white + 1);
 *   3  the position is already won: some stone, taken as the last one placed, gives a line total of exactly five in one of the four line
 *      pairs -- the rule of place_stone (:151-159); a run of six or more is not a win;
 *   4  no empty cell (Draw, :160-161);
 *   0  a legal position of a game in progress.
 * stones_out [B] (may be NULL) = the stone count; the side to move is stones & 1 (0 = Black).  Touches no engine state (the batched,
 * caller-held form, like omok_env_scripted_actions). */
int omok_env_check_positions(omok_engine* e, const uint8_t* boards, int32_t batch, int32_t* verdict_out, int32_t* stones_out);

/* Random openings on the device: an opening book without a file, for the match of benchmark/src/main.rs:14-108, which starts every game at
 * Environment::new() and so plays (nearly) one game per colour assignment.  Position b of boards_out [batch][N*N] (Stone bytes) is the
 * board after `stones` plies of the game with global id first_game + b in which BOTH sides are the OMOK_OPP_RANDOM player of
 * _play_against_random_player (src/trainer.rs:452-455), with RNG key `key`: ply i (side i & 1, Black first) puts its stone on the r-th empty
 * cell in ascending order, r = mulhi(x0, N*N - i), x0 = word 0 of Philox(key, 0, i, low 32 bits of 2 (first_game + b) + (i & 1), purpose 4)
 * -- the draw omok_opponent_actions makes for that game and ply; no new RNG purpose.  If a placement ends the game
 * (place_stone(..).is_terminal(), environment/src/lib.rs:104-166: exactly five in a line) placing stops, ok_out[b] = 0 and the board holds
 * the stones up to and including that one; otherwise ok_out[b] = 1 and the board has verdict 0 under omok_env_check_positions with exactly
 * `stones` stones.  0 <= stones < N*N and batch >= 1, else OMOK_ERR_INVALID.  Touches no engine state and needs no net (the batched,
 * caller-held form, like omok_env_check_positions); a position depends on (key, first_game + b, stones) only, not on how a range of games
 * is cut into calls. */
int omok_env_random_positions(omok_engine* e, uint64_t key, int64_t first_game, int32_t stones, int32_t batch, uint8_t* boards_out,
                              uint8_t* ok_out);

/* ---- self-play: G games x two agents (src/trainer.rs:81-205) ---------------------------- */
/* Agent::new for both agents of every game (alpha-zero/src/agent.rs:16-35): root policy = raw
 * evaluate_p of the empty board.  Also clears the replay buffer.  Every reset is one trainer iteration
 * (src/trainer.rs:74-93, fresh thread_rng draws): it takes RNG stream `episode` and advances the counter; the first reset
 * after omok_create is episode 0. */
int omok_selfplay_reset(omok_engine* e);
/* Agent::new for both agents of every game (alpha-zero/src/agent.rs:16-35) on a GIVEN environment instead of Environment::new(): extends
 * omok_selfplay_reset to opening books, tactical test positions, resume / take-back (gui/src/main.rs:42-47 can only restart from empty) and
 * batched analysis.  boards [G][N*N] Stone bytes, the position of each game.  Root policy of both trees = evaluate_p of the position in
 * Player mode (agent.rs:19-20; the G positions are evaluated as one batch in game order, bit-identical to omok_evaluate_pv of the same G
 * rows) with every occupied cell set to 0 and, iff f32::EPSILON <= sum, scaled by 1 / sum -- the arithmetic of ensure_action_exists
 * (agent.rs:166-171), which every policy the reference stores on a non-empty board went through.  Roots carry no history: n = 0, w = 0,
 * no action.  The games' plies and omok_current_ply start at the stone count (side to move = stones & 1, RNG counters of DESIGN 5); the
 * Boltzmann threshold of omok_sample_actions keeps counting the moves sampled (trainer.rs:139); the replay buffer is cleared and holds only
 * moves sampled after the reset.  Episode counter and RNG stream as omok_selfplay_reset.
 * OMOK_ERR_ILLEGAL if omok_env_check_positions gives a position a verdict other than 0, OMOK_ERR_INVALID if the stone counts differ (all
 * games of an episode share the side to move, trainer.rs:96-97); the message names the first offending game.  A rejected call leaves the
 * engine exactly as it was.  With no stone on any board this IS omok_selfplay_reset.
 * Afterwards every self-play call works as after omok_selfplay_reset, omok_execute_shared(_recorded) on a one-game engine and
 * omok_versus_run included; omok_selfplay_run_slots returns OMOK_ERR_STATE (refilled slots would start from the empty board). */
int omok_selfplay_reset_from(omok_engine* e, const uint8_t* boards);
/* Match episode: net 1 against net 2 (benchmark/src/main.rs:14-108).  Agent::new of every agent with its OWN net (agent.rs:16-35): in games
 * [0, split) net 1 plays Black (tree side 0) and net 2 White (side 1); in games [split, G) the colours are reversed (main.rs plays half of
 * its games each way).  0 <= split <= G.  RNG streams, the episode counter and the replay buffer as omok_selfplay_reset.  Until the next
 * omok_selfplay_reset every evaluation uses the net of the tree it serves: the search requests of omok_execute / omok_selfplay_run /
 * omok_round_* that of the side-to-move tree (Agent::search with its own model, main.rs:71-78,91-98), the ensure_action_exists rows of
 * omok_advance / omok_selfplay_run / omok_mirror_* that of the OPPONENT's tree (main.rs:79-82,99-102); the step-wise calls keep their row
 * order (game order).  A whole match is omok_selfplay_run (threshold = 0: sample_action(Best) every move, as main.rs:77,97); per-game
 * results from omok_game_info.  With the same weights in both slots a match reproduces omok_selfplay_reset + the same calls bit for bit
 * (board_size 9, OMOK_NET_F16X3_ROWS, OMOK_NET_F32; in the default net mode at board_size 15 each net's sibling rounds group fewer rows:
 * ~5e-5 of path-dependent rounding, see OMOK_NET_F16X3_ROWS).  omok_play_actions, omok_execute_shared(_recorded) and
 * omok_selfplay_run_slots return OMOK_ERR_STATE in a match episode.  OMOK_ERR_STATE without a committed net 2, OMOK_ERR_INVALID for a
 * split outside [0, G]. */
int omok_match_reset(omok_engine* e, int32_t split);
/* omok_match_reset on a GIVEN environment, as omok_selfplay_reset_from is omok_selfplay_reset on one: a match from an opening book
 * (benchmark/src/main.rs:14-108 can only start at Environment::new(); Agent::new of every agent with its own net, agent.rs:16-35).
 * boards [G][N*N] Stone bytes, the position of each game; split as in omok_match_reset: in games [0, split) net 1 owns the Black tree (side
 * 0) and net 2 the White tree, in [split, G) the reverse -- whichever side the position gives the move to.  Root policy of tree side * G + g
 * = evaluate_p of position g in Player mode (agent.rs:19-20) computed by net side ^ (g >= split), with every occupied cell set to 0 and then
 * scaled by 1.0f / sum iff f32::EPSILON <= sum (ensure_action_exists, agent.rs:166-171; the device function omok_selfplay_reset_from and
 * omok_advance use).  The root has n = 0, w = 0, no parent, no table, no action; legal = N*N - stones, turn = stones & 1.  Every game has one
 * tree of each net, so each net evaluates all G positions as one plain-row batch in game order: net 1's rows are bit-identical to
 * omok_evaluate_pv of the same G rows on this engine, net 2's to omok_evaluate_pv on an engine that holds net 2's weights in slot 1 (same
 * net_mode); omok_net2_info's evals count G rows for each net.  The games' plies, omok_current_ply and the ply the episode started at are
 * the stone count; the count of moves sampled (Boltzmann threshold, replay length) is 0; episode counter and RNG key as in every reset; the
 * replay buffer is cleared; the episode is a match with this split.
 * Checked in this order: net 1 committed, else OMOK_ERR_STATE; net 2 committed, else OMOK_ERR_STATE; 0 <= split <= G, else
 * OMOK_ERR_INVALID; every omok_env_check_positions verdict 0, else OMOK_ERR_ILLEGAL; equal stone counts, else OMOK_ERR_INVALID (the message
 * names the first offending game).  A rejected call leaves the engine exactly as it was: trees, games, match / split, the episode counter
 * and the replay buffer.  With no stone on any board this IS omok_match_reset.
 * Afterwards every call behaves as after omok_match_reset: omok_play_actions, omok_execute_shared(_recorded), omok_selfplay_run_slots,
 * omok_versus_run and omok_opponent_actions return OMOK_ERR_STATE. */
int omok_match_reset_from(omok_engine* e, int32_t split, const uint8_t* boards);
/* index of the RNG stream the NEXT omok_selfplay_reset uses (resuming a training run at iteration i: omok_set_episode(e, i)) */
int omok_set_episode(omok_engine* e, uint64_t episode);
/* ParallelMCTSExecutor::execute (alpha-zero/src/parallel_mcts_executor.rs:26-35) on the
 * side-to-move agents of all live games: rounds of `batch_size` simulations per tree, one net
 * forward per round, ordered scatter; simulations round up to a multiple of batch_size.
 * The search arguments, here and in every entry point below that takes them (else OMOK_ERR_INVALID, nothing changed):
 *   count >= 1, 1 <= batch_size <= max_batch_k, 0 <= epsilon <= 1 (epsilon = 0 still renormalises the root row, pme.rs:63-68; epsilon = 1
 *   leaves pure noise),
 *   0 < alpha <= OMOK_ALPHA_MAX: the Dirichlet noise is normalised Gamma(alpha) draws, alpha = k + f with k = min((int)alpha, 32) unit
 *   exponentials and an Ahrens-Dieter GS draw for f.  GS samples Gamma(f) only for f <= 1, so alpha = 33 (k = 32, f = 1) is the largest value
 *   drawn from the right distribution: above it the clamp leaves f > 1 (the mean of "Gamma(40)" comes out near 33.9), and alpha = inf has no
 *   integer part at all.  The reference hands alpha to rand_distr's Dirichlet, which has no such limit; its default is 0.03 (src/config.rs:94). */
#define OMOK_ALPHA_MAX 33
int omok_execute(omok_engine* e, int32_t count, int32_t batch_size, float epsilon, float alpha);
/* MCTSExecutor::run (alpha-zero/src/mcts_executor.rs:29-255; the executor of gui/src/agent.rs and benchmark/src/agent.rs) on an
 * engine with games = 1: ONE tree searched by `waves` wavefronts.  The reference runs its ceil(count / batch_size) rounds as
 * rayon tasks on one shared tree (relaxed atomics on n / w, the children lock in expand(), a duplicate expansion returns None
 * and drops the simulation, :171-178); here `waves` rounds run concurrently as the wavefronts of one workgroup, their requests
 * are evaluated as one batch and scattered by the same wavefronts.  waves = 1 is the sequential schedule: identical, bit for
 * bit, to omok_execute.  With waves > 1 the result depends on the interleaving, as it does in the reference. */
int omok_execute_shared(omok_engine* e, int32_t count, int32_t batch_size, float epsilon, float alpha, int32_t waves);
/* The same search under a RECORDED interleaving, for exact parity tests of waves > 1 (the reference's schedule is whatever its thread pool
 * does): every whole simulation and every backup of a scatter phase runs under the tree lock, i.e. the run is a sequential interleaving of
 * the waves' simulations -- one of the schedules the reference can produce -- and the lock order is reported so that a CPU restatement of
 * MCTSExecutor::run (mcts_executor.rs:76-255) can replay it.  G = ceil(ceil(count / batch_size) / waves) groups of `waves` rounds;
 * sim_order, backup_order [G][waves * batch_size]: wave index of the i-th simulation / backup of the group (0xFF beyond the group's
 * count); group_counts [G][3] = simulations, backups, requests; p [cap_requests][N*N], v [cap_requests]: the net outputs of all requests
 * in evaluation order (group by group, inside a group by wave then simulation); *n_groups, *n_requests. */
int omok_execute_shared_recorded(omok_engine* e, int32_t count, int32_t batch_size, float epsilon, float alpha, int32_t waves,
                                 uint8_t* sim_order, uint8_t* backup_order, int32_t* group_counts, float* p, float* v,
                                 int32_t cap_requests, int32_t* n_groups, int32_t* n_requests);
/* Agent::sample_action for every live game (agent.rs:83-137) with the trainer's mode rule
 * (trainer.rs:138-146): Boltzmann(temperature) while the game's ply < threshold, else Best.
 * Records the transition (env before the move, pi) like trainer.rs:150-173.
 * actions [G]: chosen cell, -1 for finished games.  May be NULL.
 * temperature (here and in omok_selfplay_run / _run_slots / _run_slots_logged): 1 / temperature <= OMOK_TEMPERATURE_INV_MAX in fp32, that
 * is temperature >= 0.0125, and not NaN; else OMOK_ERR_INVALID, nothing changed.  The heated weights exp(pi / T) and their sum are fp32
 * (agent.rs:119-120): pi <= 1 and at most 225 cells, so with 1 / T <= 80 the sum is at most 225 * exp(80) = 1.2e37 < FLT_MAX = 3.4e38.  The
 * first possible overflow is at 1 / T = ln(FLT_MAX) - ln(225) = 88.72 - 5.42 = 83.3.  Once a weight or the sum is inf, every normalised weight is 0 or
 * NaN and the reference panics (WeightedIndex::new(..).unwrap(), agent.rs:130); there is no move to reproduce.  temperature = +inf is
 * legal: 1 / T = 0, every visited cell weighs exp(0) = 1, the draw is uniform over the visited cells -- exactly what agent.rs:110-128
 * computes with temperature.recip() = 0. */
#define OMOK_TEMPERATURE_INV_MAX 80
int omok_sample_actions(omok_engine* e, float temperature, int32_t threshold, int32_t* actions);
/* Agent::play_action on the mover's tree, then ensure_action_exists + play_action on the
 * opponent's tree (agent.rs:144-232, trainer.rs:156-167), finished games retire
 * (trainer.rs:175-201).  Uses the actions chosen by the last omok_sample_actions. */
int omok_advance(omok_engine* e);
/* Agent::compute_policy (agent.rs:43-77) of the side-to-move agent of every game: pi [G][N*N] = child visit counts / their
 * sum; has_policy[g] = 0 where the reference returns None (finished game, no children, or no visits; the row is then 0).
 * has_policy may be NULL. */
int omok_compute_policy(omok_engine* e, float* pi, uint8_t* has_policy);
/* Externally chosen moves, actions [G] (ignored for finished games; every live game must move: all games share the side to
 * move, trainer.rs:96-97): Agent::ensure_action_exists(action) + Agent::play_action(action) on BOTH agents of each game
 * (agent.rs:144-232) -- what gui/src/agent.rs:49-66 and benchmark/src/agent.rs:34-50 do with a move their own search did not
 * pick.  One batched evaluate_p serves both agents of a game (same position).  No Transition is recorded (the trainer
 * records only moves it sampled, trainer.rs:138-173).  An occupied / out-of-range cell returns OMOK_ERR_ILLEGAL and leaves
 * every game unchanged (Option::None of play_action). */
int omok_play_actions(omok_engine* e, const int32_t* actions);
/* step-wise form for parity tests: stages the moves like omok_sample_actions does; omok_mirror_* / omok_advance follow */
int omok_set_actions(omok_engine* e, const int32_t* actions);
/* whole self-play phase of one trainer iteration (trainer.rs:95-205): repeats
 * execute/sample/advance until every game is finished or max_plies (>0) plies were played.
 * stats (may be NULL, OMOK_STAT_COUNT doubles): see OMOK_STAT_* */
int omok_selfplay_run(omok_engine* e, int32_t count, int32_t batch_size, float epsilon, float alpha,
                      float temperature, int32_t threshold, int32_t max_plies, double* stats);

/* ---- evaluation games against the scripted players of src/trainer.rs:380-394, 400-603 ---------
 * OMOK_OPP_NAIVE: the "naive" player of play_against_naive_player (trainer.rs:508-534): the LOWEST empty cell at which a stone of the side
 * to move, or a stone of the other side, ends the game -- place_stone(..).is_terminal() (environment/src/lib.rs:104-190): exactly five in a
 * line (an overline does not count) or Draw (the last empty cell); the reference breaks at the first such cell, so a block at a lower index
 * beats a win at a higher one.  Without such a cell it falls through to OMOK_OPP_RANDOM.
 * OMOK_OPP_RANDOM: legal_moves[rng.gen_range(0..len)] (trainer.rs:452-455, :534): the r-th empty cell in ascending order, r = mulhi(x0,
 * legal_move_count), x0 = word 0 of Philox(key of the episode, 0, the game's ply, 2 * (game_offset + game) + side to move, purpose 4)
 * (DESIGN.md "RNG contract").
 * OMOK_OPP_THREAT: a threat-aware player, not one of the reference's: a fixed opponent that a net does not beat merely by extending a three.  It
 * is defined by the same exact-five test alone.  For a colour c, an empty cell a and a line pair pr (0 horizontal, 1 vertical, 2 and 3 the
 * diagonals), ra and rb are the runs of consecutive c stones from a outwards along the two opposite rays, and L(c,a,pr) = 1 + ra + rb.
 *   FIVE(c,a)   L(c,a,pr) == 5 for some pr: the test above (a run of six is no five).
 *   T(c,a)      the number of winning cells a c stone at a would leave: with c at a, the cells e = a +- k d_pr, k = 1..4, over the four pairs
 *               (at most 32) that are on the board, empty, and have L(c,e,pr) == 5 along that same pair.  A completion that would make six
 *               does not count; a four against the edge or an enemy stone has T = 1.
 *   OPEN3(c,a)  for some pr, L(c,a,pr) == 3 and the two cells just beyond the run's ends are both on the board and empty.
 *   NEAR(a)     some stone of either colour lies at Chebyshev distance 1 from a.
 * With `me` the side to move and `opp` the other, the move is the LOWEST empty cell of the first level that has one:
 *   1  FIVE(me,a); or the last empty cell (Draw is terminal, as in the naive rule)
 *   2  FIVE(opp,a)
 *   3  T(me,a) >= 2: an open four, a double four, filling a split three
 *   4  T(opp,a) >= 2: denies the opponent the same, which blocks an existing open three
 *   5  OPEN3(me,a)
 *   6  the r-th cell in ascending order among the empty cells with NEAR, r = mulhi(x0, their count)
 *   7  no empty cell has NEAR (the empty board): OMOK_OPP_RANDOM's draw over all empty cells
 * x0 is the word OMOK_OPP_RANDOM draws for that game, ply and side; no new RNG purpose.  Unlike the naive rule a win beats a block at a lower
 * index, and the side to move matters.  The value 2 is no player and stays an invalid kind. */
#define OMOK_OPP_RANDOM 0
#define OMOK_OPP_NAIVE 1
#define OMOK_OPP_THREAT 3
/* OMOK_OPP_VCF: the threat-aware player with a forced-win solver.  Its rule is OMOK_OPP_THREAT's with one level put in after level 2: if
 * omok_env_vcf_solve's rule (below) with max_depth = OMOK_VCF_OPP_DEPTH and max_nodes = OMOK_VCF_OPP_NODES gives verdict 1 for the side to move,
 * it plays the solver's cell; otherwise levels 3..7 apply unchanged, with the same draw word.  It differs from OMOK_OPP_THREAT only where the
 * shortest forced win takes three or more attacker moves (a win in two is level 3's own cell).  The value 4 is no player and stays an invalid
 * kind, like 2. */
#define OMOK_OPP_VCF 5
#define OMOK_VCF_OPP_DEPTH 6
#define OMOK_VCF_OPP_NODES 256
/* OMOK_OPP_GUARD: the defending player.  It is OMOK_OPP_VCF with its move checked against the other side's win by continuous fours and, where
 * that move loses, replaced through the defender's map (omok_env_vcf_defend below): a fixed opponent that a net does not beat merely by setting
 * up a four-three.  `me` is the side to move and `opp` the other; x0 is the game's draw word, the word the other players draw for that game,
 * ply and side (no new RNG purpose); D and NB are OMOK_VCF_OPP_DEPTH and OMOK_VCF_OPP_NODES; solve is the rule of omok_env_vcf_solve,
 * unchanged; defend is the rule of omok_env_vcf_defend, unchanged, without its null move, which the player does not need.
 * Let (c0, L0, solved, n0) be OMOK_OPP_VCF's move on the position X: c0 its cell with the draw made by x0, L0 the threat rule's level, solved
 * whether the solver's level decided, n0 the number of cells its draw chose among (0 unless the draw decided).
 *   step 0         L0 = 0, the board has no empty cell: the cell is -1.
 *   step 1, own    L0 <= 2 or solved: play c0 (a five, the block of a five, the last cell, the player's own forced win).
 *   step 2, kept   R = solve(X with me at c0, opp, D, NB).  If R.verdict != 1, play c0: a budget verdict keeps the move.
 *   otherwise      take the status map of defend(X, me, D, NB).  M = the cells with OMOK_VCFD_SAFE (step 3); if there are none, M = the cells
 *                  with OMOK_VCFD_UNKNOWN (step 4); if both sets are empty, play c0 (step 5: every move loses).  No cell is WINS here, because
 *                  L0 >= 3, and c0 is LOSES, by the same solve as step 2.
 *   steps 3 and 4  the threat rule's levels 3..7 restricted to M: the LOWEST a in M of the first level that has one --
 *                    3  T(me,a) >= 2      4  T(opp,a) >= 2      5  OPEN3(me,a)
 *                    6  the r-th cell in ascending order of M with NEAR, r = mulhi(x0, their count)
 *                    7  no cell of M has NEAR: the r-th cell of M
 * The map is not monotone (see omok_env_vcf_defend), so step 2 is applied to whatever cell the VCF rule chose, from any level, and no cell of
 * the map is skipped.  By construction the player plays a LOSES cell only where no SAFE cell exists.  The value 6 is no player and stays an
 * invalid kind, like 2 and 4. */
#define OMOK_OPP_GUARD 7
/* the forced part of the rule on caller-held positions (boards [B][N*N] Stone bytes, turns [B]): forced_out[b] = the cell the NAIVE rule
 * picks before its random fallback (trainer.rs:514-531), -1 if none (always -1 for RANDOM).  (The rule tries a stone of either colour at
 * every empty cell, so the side to move does not change the answer: turns is read by no kernel.)  For OMOK_OPP_THREAT the side to move
 * decides: forced_out[b] = the cell of levels 1..5, -1 for levels 6 and 7, and a turns byte above 1 is OMOK_ERR_INVALID, checked before
 * anything is launched (kinds 0 and 1 keep ignoring turns).  OMOK_OPP_VCF likewise: the cell of levels 1..5 or the solver's cell.  OMOK_OPP_GUARD likewise: the
 * player's cell with x0 = 0 where no draw decided (omok_env_guard_scan's count = 0), else -1. */
int omok_env_scripted_actions(omok_engine* e, int32_t kind, const uint8_t* boards, const uint8_t* turns, int32_t batch, int32_t* forced_out);
/* step-wise: the scripted player's move (trainer.rs:508-534 / :452-455) for the side to move of every live game, chosen on the device and
 * staged like omok_set_actions (omok_mirror_* / omok_advance follow); actions [G] may be NULL, -1 for finished games.  OMOK_ERR_STATE in a
 * match episode, OMOK_ERR_INVALID for an unknown kind. */
int omok_opponent_actions(omok_engine* e, int32_t kind, int32_t* actions);
/* Which level of the OMOK_OPP_THREAT rule decides on caller-held positions (boards [B][N*N] Stone bytes, any other byte counts as empty;
 * turns [B] = the side to move, 0 Black / 1 White): level_out[b] = 1..7, or 0 on a board with no empty cell; cell_out[b] = the cell of levels
 * 1..5, else -1; count_out[b] = the number of cells the draw of level 6 or 7 chooses among, 0 for the other levels.  Each output may be NULL.
 * Touches no engine state and needs no net (like omok_env_check_positions).  batch < 1, NULL boards or turns, or a turns byte above 1:
 * OMOK_ERR_INVALID, with nothing written. */
int omok_env_threat_scan(omok_engine* e, const uint8_t* boards, const uint8_t* turns, int32_t batch, int32_t* cell_out, int32_t* level_out,
                         int32_t* count_out);
/* Does the side to move have a forced win by continuous fours (VCF)?  Exact under the exact-five rule: every attacker move leaves a cell that
 * completes five, so every reply is forced and only the attacker's side of the tree branches.  Not one of the reference's functions; it is
 * defined by FIVE and T above alone.  `me` is the side to move, `opp` the other; W(a) is the set of the T(me,a) empty cells that complete
 * exactly five for `me` once `me` has played a.  Inputs: a board, me, max_depth D in 1..16, max_nodes NB in 1..65536; one node counter for
 * the whole call.
 *   solve:  for d = 1 .. D:  pv = search(d);  if pv: verdict 1, moves = d, cell = pv[0]
 *           none found: verdict 0
 *   search(r):                       (the attacker is to move)
 *       count one node; if that makes the count exceed NB: the whole call ends with verdict -1
 *       if some empty a has FIVE(me,a):            return [lowest such a]
 *       if r == 1:                                 return fail
 *       Fo = the empty cells b with FIVE(opp,b)
 *       if |Fo| >= 2:                              return fail
 *       for a in ascending order over (Fo if |Fo| == 1 else all empty cells) with T(me,a) >= 1:
 *           if T(me,a) >= 2:                       return [a, lowest of W(a), second lowest of W(a)]
 *           if r >= 3:   e = the one cell of W(a); place me at a and opp at e;  pv = search(r - 1);  take both back
 *                        if pv:                    return [a, e] + pv
 *       return fail
 * Why it is sound:
 *   - Before a the attacker had no five, so every completing cell after a lies on a line through a within four steps: W(a) is all of them.
 *   - The defender has no five after a: either Fo was empty, or a took its one cell.
 *   - So the defender's only move that does not lose at once is e, and placing e cannot itself make five.
 *   - The defender's stone at e may make the defender a four: that is the |Fo| == 1 branch one level down, where the attacker must block it
 *     with a move that is itself a four.
 *   - A candidate with T = 1 is not recursed at r = 2: its one completing cell gets blocked, so search(1) cannot succeed.
 *   - Iterative deepening makes `moves` the least number of attacker moves up to and including the five, and `cell` the lowest first move
 *     that achieves it.
 * The node count is part of the result (the budget verdict depends on it): no transposition table, no pruning that changes it.
 * boards [B][N*N] Stone bytes (any other byte counts as empty), turns [B] = the side to move (0 Black / 1 White).  Per position:
 *   verdict_out  1 a forced win within D attacker moves, 0 none, -1 the node budget ran out
 *   moves_out    the attacker moves up to and including the five; 0 unless verdict is 1
 *   cell_out     the first move; -1 unless verdict is 1
 *   nodes_out    the nodes counted; NB on verdict -1
 *   pv_out       [B][2 * D - 1] cells: attacker, forced reply, attacker, ... ending with the five, padded with -1; all -1 unless verdict is 1
 * Each output may be NULL.  Touches no engine state and needs no net.  batch < 1, NULL boards or turns, a turns byte above 1, max_depth outside
 * 1..16 or max_nodes outside 1..65536: OMOK_ERR_INVALID, with nothing written and nothing launched.  (65536 nodes bounds how long one wave
 * can run; it is a condition of the call, not a tuned value.) */
int omok_env_vcf_solve(omok_engine* e, const uint8_t* boards, const uint8_t* turns, int32_t batch, int32_t max_depth, int32_t max_nodes,
                       int32_t* verdict_out, int32_t* cell_out, int32_t* moves_out, int32_t* nodes_out, int32_t* pv_out);
/* The defender's half: which moves of the side to move do not lose to the other side's win by continuous fours?  As exact as the solver:
 * solve(X, c, D, NB) below is the rule of omok_env_vcf_solve above for the side c on the position X, unchanged -- iterative deepening, one node
 * counter per call, the same candidate order.  For a position X (a byte other than 1 or 2 counts as empty), `me` the side to move, `opp` the
 * other, max_depth D in 1..16, max_nodes NB in 1..65536:
 *   the null move:   R0 = solve(X, opp, D, NB): would opp win by continuous fours if me passed?  threat = (R0.verdict, R0.moves, R0.cell)
 *   every cell a, each with a node counter of its own:
 *       a is occupied:      status OMOK_VCFD_OCCUPIED, moves 0, nodes 0, reply -1
 *       FIVE(me,a):         status OMOK_VCFD_WINS, moves 0, nodes 0, reply -1; no solve is made
 *       otherwise           R = solve(X with me at a, opp, D, NB):
 *           R.verdict 0     status OMOK_VCFD_SAFE
 *           R.verdict 1     status OMOK_VCFD_LOSES
 *           R.verdict -1    status OMOK_VCFD_UNKNOWN
 *                           moves = R.moves, nodes = R.nodes, reply = R.cell
 *   - The last empty cell needs no special case: on the full board solve counts one node per depth and returns verdict 0, so the status is
 *     OMOK_VCFD_SAFE with nodes = D, or OMOK_VCFD_UNKNOWN where NB < D.
 *   - A four of the mover's at a needs none either: it is the solver's own |Fo| == 1 branch, where opp must answer it with a move that is
 *     itself a four.  Such a move may merely postpone the loss; the status says which.
 *   - The map is NOT monotone: opp may have no win if me passes and yet have one after a stone of me's.  Under the exact-five rule a mover's
 *     stone can turn its own completing cell into a six, which removes the counter-threat that held the attack off.  So no cell is skipped
 *     because the null move is safe, and every cell is solved on its own.
 * boards [B][N*N] Stone bytes, turns [B] = the side to move (0 Black / 1 White).  Per position:
 *   status_out  [B][N*N] OMOK_VCFD_*
 *   moves_out   [B][N*N] opp's attacker moves up to and including the five after me at a; 0 unless the status is OMOK_VCFD_LOSES
 *   nodes_out   [B][N*N] the nodes that cell's solve counted; NB on OMOK_VCFD_UNKNOWN
 *   reply_out   [B][N*N] opp's first move of that win; -1 unless the status is OMOK_VCFD_LOSES
 *   threat_out  [B][3]   verdict, moves, cell of the null move
 * Each output may be NULL.  Touches no engine state and needs no net.  batch < 1, NULL boards or turns, a turns byte above 1, max_depth outside
 * 1..16 or max_nodes outside 1..65536: OMOK_ERR_INVALID, with nothing written, nothing allocated and nothing launched.  (One wave of the device
 * runs one solve: 65536 nodes bounds it here as it does in omok_env_vcf_solve.)  The number of cells per status is left to the caller: it is
 * a sum over the status row. */
#define OMOK_VCFD_OCCUPIED 0
#define OMOK_VCFD_SAFE 1
#define OMOK_VCFD_WINS 2
#define OMOK_VCFD_LOSES 3
#define OMOK_VCFD_UNKNOWN 4
int omok_env_vcf_defend(omok_engine* e, const uint8_t* boards, const uint8_t* turns, int32_t batch, int32_t max_depth, int32_t max_nodes,
                        uint8_t* status_out, uint8_t* moves_out, int32_t* nodes_out, int32_t* reply_out, int32_t* threat_out);
/* The move of OMOK_OPP_GUARD on caller-held positions, and which step of its rule decided (boards [B][N*N] Stone bytes, any other byte counts
 * as empty; turns [B] = the side to move, 0 Black / 1 White; draws [B] = the draw word x0 of every position, NULL: all 0).  The rule runs with
 * max_depth and max_nodes in place of D and NB (the player itself always uses OMOK_VCF_OPP_*).  Per position:
 *   cell_out   the move the player makes with that word, or -1 on a full board
 *   step_out   0..5, the step of the rule above that decided
 *   level_out  L0 in steps 1, 2 and 5; the restricted rule's level 3..7 in steps 3 and 4; 0 in step 0
 *   count_out  the number of cells the deciding draw chose among, else 0
 * Each output may be NULL.  Touches no engine state and needs no net.  batch < 1, NULL boards or turns, a turns byte above 1, max_depth outside
 * 1..16 or max_nodes outside 1..4096: OMOK_ERR_INVALID, with nothing written, nothing allocated and nothing launched.  (One wave of the first
 * pass runs two solves in sequence, so the cap is a sixteenth of the solver's 65536: it bounds how long a wave can run and is a condition of
 * the call, not a tuned value.) */
int omok_env_guard_scan(omok_engine* e, const uint8_t* boards, const uint8_t* turns, const uint32_t* draws, int32_t batch, int32_t max_depth,
                        int32_t max_nodes, int32_t* cell_out, int32_t* step_out, int32_t* level_out, int32_t* count_out);
/* Whole evaluation episode after a fresh omok_selfplay_reset: play_against_naive_player (trainer.rs:487-603: kind = OMOK_OPP_NAIVE,
 * opponent_side = 0, the scripted player is Black and moves first) or _play_against_random_player (:400-485: OMOK_OPP_RANDOM, opponent_side =
 * 1).  On plies where opponent_side (0 = Black, 1 = White) is to move: the scripted move as an external move (ensure_action_exists +
 * play_action, :536-538; kind may be OMOK_OPP_THREAT, OMOK_OPP_VCF or OMOK_OPP_GUARD as well).  On the others: omok_execute(count, batch_size, epsilon, alpha), sample_action(Best), play_action (:562-577).
 * Runs until every game is over or max_plies (> 0) plies were played.  results [3] (may be NULL) = black wins, white wins, draws among the
 * finished games (the reference's tuple, :602); stats as omok_selfplay_run.
 * The net's agent is the engine's tree of side 1 - opponent_side: it receives exactly the calls the reference's single Agent receives.  The
 * tree of side opponent_side is kept in step like with any external move (both agents of a game, see omok_play_actions); it is never
 * searched, and costs one shared root-row evaluation per game and ply.  Transitions are recorded on the net's plies only (the moves
 * omok_sample_actions chose): the replay buffer of an evaluation episode is not training data and is discarded by the next
 * omok_selfplay_reset.  After omok_selfplay_reset_from the episode starts at the positions' ply: opponent_side still decides who moves on which
 * ply (Black to move and opponent_side = 1: the first ply is a search).  OMOK_ERR_STATE in a match episode or when moves were played since the
 * reset, OMOK_ERR_INVALID for an unknown kind or opponent_side. */
int omok_versus_run(omok_engine* e, int32_t kind, int32_t opponent_side, int32_t count, int32_t batch_size, float epsilon, float alpha,
                    int32_t max_plies, int32_t* results, double* stats);

/* Slots mode ("continuous refill"): plays `total_games` >= games games on the engine's `games` slots; a slot whose game is over takes the
   next game index instead of idling until the episode's longest game ends.  Per-game results are those of an episode of total_games
   games (omok_selfplay_run on an engine with games = total_games): a game's RNG streams are keyed by game_offset + index and its own
   ply, trees are independent (bit for bit with board_size 9 or OMOK_NET_F16X3_ROWS / OMOK_NET_F32; in the default net mode at
   board_size 15 a row's p / v carry ~5e-5 of rounding that depends on the path a round takes, see OMOK_NET_F16X3_ROWS).  Call after
   omok_selfplay_reset (OMOK_ERR_STATE after omok_selfplay_reset_from).  Finished games' transitions are appended to records_dev (device memory, cap_records records of
   omok_replay_record_bytes, the omok_replay_pack_dev format) in completion order; per game index: game_offsets[i] = first record,
   game_lengths[i] = records, game_status[i] = OMOK_STATUS_* (arrays of total_games, may be NULL); *n_records = records written.
   Extends src/trainer.rs:95-205 (the reference removes finished games from its agent list and lets the batch shrink). */
int omok_selfplay_run_slots(omok_engine* e, int32_t total_games, int32_t count, int32_t batch_size, float epsilon, float alpha,
                            float temperature, int32_t threshold, void* records_dev, int64_t cap_records, int64_t* game_offsets,
                            int32_t* game_lengths, int32_t* game_status, int64_t* n_records, double* stats);
/* omok_selfplay_run_slots with the move log (omok_game_log_enable) packed out beside the records: the same games, the same records, the same
 * stats, and for every record the move that followed it.  log_dev = device memory of cap_records entries of omok_game_log_entry_bytes (20);
 * entry game_offsets[i] + p is move p of game index i, beside record game_offsets[i] + p (in slots mode every move is sampled, so a game has
 * as many records as moves).  Entry, little-endian, by byte offset: 0 u32 root_n, 4 f32 root_w, 8 u32 child_n, 12 f32 child_w, 16 u16 move
 * (cell | OMOK_MOVE_EXTERNAL, as omok_game_log_read), 18 u16 zero; the values are those omok_game_log_read returns for the same game of an
 * episode of total_games games.  Needs the move log on and a reset since (OMOK_ERR_STATE otherwise: omok_game_log_enable, then
 * omok_selfplay_reset); log_dev == NULL is OMOK_ERR_INVALID; every other check is omok_selfplay_run_slots', and all of them precede the
 * first allocation or write.  The engine's per-slot log is the staging area: afterwards it describes no game, and omok_game_log_read returns
 * OMOK_ERR_STATE until the next reset starts an ordinary log.  OMOK_ERR_OVERFLOW with *n_records = the count needed when the games do not
 * fit cap_records: neither buffer is written beyond it. */
int omok_selfplay_run_slots_logged(omok_engine* e, int32_t total_games, int32_t count, int32_t batch_size, float epsilon, float alpha,
                                   float temperature, int32_t threshold, void* records_dev, int64_t cap_records, void* log_dev,
                                   int64_t* game_offsets, int32_t* game_lengths, int32_t* game_status, int64_t* n_records, double* stats);
/* bytes of one entry of omok_selfplay_run_slots_logged's log_dev: 20 */
int32_t omok_game_log_entry_bytes(void);

/* step-wise form of execute() for parity tests: generate -> (eval | inject) -> scatter */
int omok_round_generate(omok_engine* e, int32_t round, int32_t batch_size, float epsilon, float alpha,
                        int32_t* n_requests);
int omok_round_inputs(omok_engine* e, float* inputs /* [n_requests][N][N][3] */);
int omok_round_eval(omok_engine* e);
int omok_round_outputs(omok_engine* e, float* p, float* v);
/* Precision evidence (tests, bench): the policy logits in front of the softmax [n_requests][HW] and the value in front of tanh [n_requests] (may be NULL)
 * of the round evaluated by omok_round_eval -- the quantities north_star's tolerance names (alpha-zero/src/network.rs:227-247), on the path the search
 * rounds take (sibling base + window differences).  Call between omok_round_eval and omok_round_scatter. */
int omok_round_logits(omok_engine* e, float* logits, float* vpre);
int omok_round_inject(omok_engine* e, const float* p, const float* v);
int omok_round_scatter(omok_engine* e);
/* step-wise form of the opponent-tree mirror eval inside omok_advance */
int omok_mirror_generate(omok_engine* e, int32_t* n_requests);
int omok_mirror_inputs(omok_engine* e, float* inputs);
int omok_mirror_eval(omok_engine* e);
int omok_mirror_outputs(omok_engine* e, float* p);
int omok_mirror_inject(omok_engine* e, const float* p);
int omok_mirror_apply(omok_engine* e);

/* ---- training phase of Trainer::train (src/trainer.rs:329-357) on the device: AgentModel::train (alpha-zero/src/agent_model.rs:136-168) in plain fp32 on
 *      the 31 raw tensors of net 1 -- the graph of network.rs:51-262, the losses of network.rs:249-253 / agent_model.rs:57-73, and the
 *      AdadeltaOptimizer of agent_model.rs:24,75-82 (lr 0.01, rho 0.95, eps 1e-8, TensorFlow ApplyAdadelta: one zero-initialised accumulator pair per
 *      variable).  Records are the packed replay records of omok_replay_augment_dev in device memory.  Every sum has a fixed order: the same calls on
 *      the same inputs leave the same bits.  All of them: OMOK_ERR_STATE before omok_train_begin; OMOK_ERR_INVALID for batch < 1, batch > max_batch,
 *      n_records < 1 or an index outside [0, n_records).  A rejected call leaves weights, accumulators and the committed state as they were. */
/* The session's optimizer state (AdadeltaOptimizer::minimize creates the accumulators, agent_model.rs:75-82) plus gradients and activations for
 * batches of up to max_batch (<= 4096) records.  Needs all 31 tensors loaded.  A second call starts a fresh optimizer. */
int omok_train_begin(omok_engine* e, int32_t max_batch);
/* frees them (omok_destroy does too) */
int omok_train_end(omok_engine* e);
/* One AgentModel::train (agent_model.rs:136-168) on records indices[0 .. batch) (a host array): encode_nn_input(Player) and encode_nn_targets
 * (encoder.rs:10-68), one minimize run, THEN the three losses evaluated after the update.  losses [3] (may be NULL) = v_loss, p_loss, loss, the
 * order of the reference's log line (trainer.rs:354-362).  Leaves net 1 uncommitted like omok_net_load: omok_net_commit before the next search. */
int omok_train_step(omok_engine* e, const void* records_dev, int64_t n_records, const int64_t* indices, int32_t batch, float* losses);
/* the forward and the three losses only (the fetches of agent_model.rs:150-166 without the minimize target): changes nothing; a held-out loss */
int omok_train_losses(omok_engine* e, const void* records_dev, int64_t n_records, const int64_t* indices, int32_t batch, float* losses);
/* The batch of step `step` of a run with RNG key `key`: choose_multiple of trainer.rs:329-350 (uniform, without replacement; the reference is
 * unseeded).  k = min(batch, n_records) indices in draw order: index i is the mulhi(x0, n_records - i)-th record, 0-based and ascending, not among
 * the first i drawn, x0 = word 0 of Philox4x32-10(key; i, step, 0, purpose 5).  out [k]; returns k. */
int omok_train_batch_indices(omok_engine* e, int64_t n_records, int32_t batch, uint64_t key, int32_t step, int64_t* out);
/* The update loop of trainer.rs:329-357: update_count steps, step s on the batch omok_train_batch_indices(n_records, batch_size, key, s) draws -- on
 * the device, with no host synchronisation between steps.  losses [3] (may be NULL) = the means of the last min(update_count, 100) steps' v_loss,
 * p_loss, loss (trainer.rs:354-362), summed on the device in step order.  Then commits net 1 as omok_net_commit does.  Weights and accumulators end
 * bit for bit as after the loop of omok_train_batch_indices + omok_train_step. */
int omok_train_run(omok_engine* e, const void* records_dev, int64_t n_records, int32_t update_count, int32_t batch_size, uint64_t key, float* losses);
/* ---- the same step in two halves, for data-parallel training (agent_model.rs:136-168 / trainer.rs:329-357 on several ranks; no reference counterpart:
 *      the reference is one process).  The engine holds no collective library: it produces gradients into caller-owned device memory, the caller moves
 *      them (an all-gather; omok_replay_pack_dev works the same way), and the engine sums the ranks' slabs IN RANK ORDER inside its Adadelta kernel, so
 *      ranks that start from equal weights stay bit-equal whatever algorithm the collective used.  Exchange layout: one fp32 slab of
 *      omok_train_gradient_count values without padding, tensor i at offset sum_{j<i} omok_net_tensor_size(j).
 *      omok_train_backward + omok_train_apply(NULL, 1) leave weights, accumulators, losses and gradients bit for bit as omok_train_step does. */
#define OMOK_TRAIN_MAX_RANKS 64
/* floats of a gradient slab: the sum of omok_net_tensor_size over the 31 tensors (agent_model.rs:136-168 / trainer.rs:329-357: one gradient per
 * variable).  A function of the board size only; needs no training state. */
int64_t omok_train_gradient_count(const omok_engine* e);
/* First half of omok_train_step (agent_model.rs:136-168 / trainer.rs:329-357): batch assembly, forward, the losses and the backward pass on records
 * indices[0 .. batch).  Writes no weight and no accumulator; the 31 gradients stay readable by omok_debug_train_gradient and, if grad_dst_dev is not
 * NULL, are also copied to that caller-owned device memory (omok_train_gradient_count floats, complete on return).  Checks and error codes of
 * omok_train_step; a rejected call changes nothing.  Marks the step pending for omok_train_apply; omok_train_step, omok_train_losses, omok_train_run,
 * omok_train_begin and omok_train_end clear that mark (they overwrite the batch). */
int omok_train_backward(omok_engine* e, const void* records_dev, int64_t n_records, const int64_t* indices, int32_t batch, void* grad_dst_dev);
/* Second half (agent_model.rs:136-168 / trainer.rs:329-357): TensorFlow ApplyAdadelta with the gradient g, then the forward and the three losses on the
 * pending batch as omok_train_step does after its update (losses [3], may be NULL).  grads_dev == NULL (ranks must be 1): g = the engine's own
 * gradient.  Else grads_dev = [ranks][omok_train_gradient_count] fp32 in device memory and, per element, g = s[0]; g += s[r] for r = 1 .. ranks - 1;
 * g *= 1.0f / (float)ranks -- plain fp32 in that order; g is what omok_debug_train_gradient reads afterwards.  Leaves net 1 uncommitted and clears
 * the pending mark.  OMOK_ERR_STATE without a pending omok_train_backward or before omok_train_begin; OMOK_ERR_INVALID for ranks < 1,
 * ranks > OMOK_TRAIN_MAX_RANKS or NULL with ranks != 1; a rejected call changes nothing. */
int omok_train_apply(omok_engine* e, const void* grads_dev, int32_t ranks, float* losses);
/* Debugging aid of the gradient tests (no reference counterpart): the gradient of tensor `index` the last omok_train_step / omok_train_run step
 * applied or the last omok_train_backward / omok_train_apply left, count = omok_net_tensor_size(index).  OMOK_ERR_STATE before the first step. */
int omok_debug_train_gradient(omok_engine* e, int32_t index, float* out, int64_t count);
/* The raw fp32 tensor `index` of net 1 as loaded or trained (Session::run fetch of a variable, model_io.rs:59-90 without the file),
 * count = omok_net_tensor_size(index). */
int omok_net_read(omok_engine* e, int32_t index, float* out, int64_t count);

/* ---- inspection ------------------------------------------------------------------------ */
int omok_alive_count(omok_engine* e);                  /* >= 0, or error */
int omok_current_ply(omok_engine* e);
int omok_game_info(omok_engine* e, uint8_t* alive, uint8_t* status, int32_t* plies); /* each [G], may be NULL */
/* canonical dump of one tree (MCTS::root / Node fields, mcts/src/node.rs:10-21):
 * ints [n][8] = parent, action, status, turn, legal_move_count, children, n, order|has_policy<<16
 * floats [n][1+N*N] = w, policy row.  returns the node count (or -count if cap is too small). */
int omok_tree_dump(omok_engine* e, int32_t game, int32_t side, int32_t* ints, float* floats, int32_t cap_nodes);
int omok_tree_root(omok_engine* e, int32_t game, int32_t side, uint32_t* root_n, float* root_w,
                   int32_t* n_nodes, int32_t* n_tables);
/* MCTS::root's n and w (mcts/src/lib.rs:34-36, node.rs:10-21) of the side-to-move agent of every game, n [G], w [G]: omok_tree_root for all
 * games in one kernel and one copy (0 for finished games).  With omok_compute_policy: what an analysis caller reads after omok_execute. */
int omok_root_stats(omok_engine* e, uint32_t* n, float* w);
/* Node::children of a root in insertion order (mcts/src/node.rs:10-21; MCTS::root, mcts/src/lib.rs:34-36): action, n, w and
 * p (= root.policy[action], which the reference keeps equal to child.p) of the first min(children, cap) children.  Returns
 * the number of children.  Any output may be NULL. */
int omok_root_children(omok_engine* e, int32_t game, int32_t side, int32_t* actions, uint32_t* n, float* w, float* p, int32_t cap);
/* Transition{env, policy, z} records of one game (trainer.rs:20-24,169-173; z as recorded at play
 * time, before the back-fill of trainer.rs:207-214).  returns the ply count. */
int omok_replay_game(omok_engine* e, int32_t game, uint8_t* boards, uint8_t* turns, float* pi, float* z,
                     int32_t cap_plies);
/* ---- game records: every move of an episode with what the mover's search knew of it -----------
 * The reference keeps a Transition for the moves the trainer sampled (src/trainer.rs:169-173) and nothing of an evaluation game or a match
 * (trainer.rs:400-603, benchmark/src/main.rs:60-105 count results only).  The move log keeps, per game, the start position and for every
 * move played since the last reset -- sampled (omok_advance, omok_selfplay_run, omok_versus_run, match episodes), scripted or supplied
 * (omok_play_actions) -- the cell, whether it was external, MCTS::root's n and w of the mover's agent (mcts/src/lib.rs:34-36, as
 * omok_root_stats returns them at that moment) and the n and w of the root's child for that cell (Node::children, mcts/src/node.rs:10-21, as
 * omok_root_children returns them; 0 / 0.0f if the root has no such child: read BEFORE Agent::ensure_action_exists, alpha-zero/src/agent.rs:144-197,
 * adds it, so a move the tree did not hold and the never-searched tree of a scripted side log what the search knew: nothing).  Written on the
 * device in front of the re-rooting of every ply; off by default, and while off the engine makes the launches and allocations it makes without it. */
#define OMOK_MOVE_CELL 255      /* 0xFF: moves[..] & OMOK_MOVE_CELL = the cell (N*N <= 225) */
#define OMOK_MOVE_EXTERNAL 256  /* 0x100: the move was not sampled from the mover's own search */
/* 1 = keep a move log from the next reset on (allocates 19 B per game and cell on first use), 0 = stop and free.  Changes no result.  Every
 * successful omok_selfplay_reset(_from) / omok_match_reset(_from) sets the log's start (its boards, or Environment::new(), environment/src/lib.rs:73-79) and the lengths to 0; a rejected
 * reset and a rejected omok_play_actions leave it as it was.  omok_selfplay_run_slots returns OMOK_ERR_STATE while the log is on (its games
 * leave their slots: omok_selfplay_run_slots_logged packs their moves out with their records). */
int omok_game_log_enable(omok_engine* e, int32_t enabled);
/* games [first_game, first_game + games): start_boards [games][N*N] Stone bytes, lengths [games] = moves since the reset (the game's plies - the
 * ply the episode started at), moves [games][N*N] (entries at and beyond the length read 0xFFFF), root_n, root_w, child_n, child_w [games][N*N]
 * (0 beyond the length); w in the perspective Node::propagate gives it (mcts/src/node.rs:83-99).  Every output may be NULL.  One synchronisation, one copy per array.
 * OMOK_ERR_STATE while the log is off or before the first reset with it on; OMOK_ERR_INVALID for a range outside [0, G]. */
int omok_game_log_read(omok_engine* e, int32_t first_game, int32_t games, uint8_t* start_boards, int32_t* lengths, uint16_t* moves,
                       uint32_t* root_n, float* root_w, uint32_t* child_n, float* child_w);
/* Batched replay on caller-held data (touches no engine state, needs no net; like omok_env_check_positions): from start_boards [batch][N*N]
 * (NULL: Environment::new()) play moves[b][0 .. min(lengths[b], upto)) (upto < 0: all; cell = word & OMOK_MOVE_CELL; moves [batch][stride])
 * by Environment::place_stone (environment/src/lib.rs:104-166), side to move = stones & 1.  Stops in front of the first move that is illegal
 * (occupied, or cell >= N*N) and after a move that ends the game.  played_out[b] = moves placed, status_out[b] = GameStatus after the last
 * one (0 if none), boards_out [batch][N*N] the position reached.  A start board whose omok_env_check_positions verdict v is not 0:
 * played_out = -v, status_out = -1, board copied unchanged.  Outputs may be NULL.  batch >= 1, stride >= 1 and 0 <= lengths[b] <= stride,
 * else OMOK_ERR_INVALID. */
int omok_env_replay(omok_engine* e, const uint8_t* start_boards, const uint16_t* moves, const int32_t* lengths, int32_t batch,
                    int32_t stride, int32_t upto, uint8_t* boards_out, int32_t* status_out, int32_t* played_out);
/* replay tuples of all games packed on the device for an RCCL gather: record = board u8[N*N],
 * turn u8, zero pad to 4, pi f32[N*N], z f32; games in id order, transitions in play order (the same bytes on every run).
 * Writes at most cap_records to dst_dev (a device pointer the caller owns, e.g. a torch tensor) and returns the record
 * count. */
int64_t omok_replay_pack_dev(omok_engine* e, void* dst_dev, int64_t cap_records);
int32_t omok_replay_record_bytes(const omok_engine* e);
/* Replay post-processing of Trainer::train (src/trainer.rs:207-324) on the device.  Per game, in game-id order (the
 * reference walks `transitions` by game index too, trainer.rs:208): the game's L transitions with z back-filled (walking backwards from the
 * last transition z alternates sign, :209-214), then 5L augmented copies, transition-major, in the reference's order
 * rotate_90, rotate_180, rotate_270, flip_horizontal, flip_vertical of board and policy (src/utils.rs:1-64), turn and z
 * unchanged.  Records as in omok_replay_pack_dev.  Returns the record count 6 * sum(L) (records beyond cap are dropped). */
int64_t omok_replay_augment_dev(omok_engine* e, void* dst_dev, int64_t cap_records);
/* The same post-processing (src/trainer.rs:207-324, src/utils.rs:1-64) on caller-held packed records -- what omok_selfplay_run_slots hands back, or
 * what another rank's omok_replay_pack_dev gathered -- when the engine no longer holds the games.  Touches no engine state and needs no net (like
 * omok_env_replay); e supplies board size, device and stream.  records_dev: n_records records of omok_replay_record_bytes in device memory, z as recorded at
 * play time; game i's game_lengths[i] transitions sit in play order at records [game_offsets[i], game_offsets[i] + game_lengths[i]) (host arrays of
 * `games`, exactly omok_selfplay_run_slots' outputs; games may lie anywhere, in any order, with gaps).  Output to dst_dev in game INDEX order, per game
 * the L back-filled transitions, then the 5L copies: byte for byte what omok_replay_augment_dev writes for an engine holding the same games in that
 * order (z of transition p = z of the game's LAST record, negated when L - 1 - p is odd; pad bytes zero).  Returns 6 * sum(L); records at or beyond
 * cap_records are dropped, never written.  `games` is not bounded by the engine's games.  records_dev and dst_dev are 4-byte aligned and do not
 * overlap.  OMOK_ERR_INVALID, with nothing enqueued and dst_dev unwritten, for a NULL pointer, cap_records < 0, games < 1, a length outside [0, N*N] (a
 * negative one is omok_selfplay_run_slots' fill of a game that never finished; length 0 contributes nothing) or a game with a positive length whose
 * records are not inside [0, n_records): omok_last_error names the first such game. */
int64_t omok_replay_augment_records_dev(omok_engine* e, const void* records_dev, int64_t n_records, const int64_t* game_offsets,
                                        const int32_t* game_lengths, int32_t games, void* dst_dev, int64_t cap_records);
/* the same for one game into host arrays ([6L][N*N] boards / pi, [6L] turns / z); returns 6L */
int omok_replay_augmented_game(omok_engine* e, int32_t game, uint8_t* boards, uint8_t* turns, float* pi, float* z,
                               int32_t cap_records);

/* Debugging aid of the parity tests (no reference counterpart): the fc0 operand rows -- the trunk's output in the layout fc0 reads,
 * DESIGN 3.1 / 3.4 -- that the LAST forward left for request rows [first_row, first_row + rows), omok_operand_row_bytes each
 * (split-precision modes; on the copy path of sibling rounds they must equal the rows of a row-by-row evaluation bit for bit). */
int64_t omok_operand_row_bytes(const omok_engine* e);
int omok_debug_operand_rows(omok_engine* e, int32_t first_row, int32_t rows, void* out);
/* Debugging aid: enabled = 0 switches the base cache of the sibling rounds off (board_size 15, DESIGN 3.3: every run's base position is
 * then evaluated in full in every round instead of being kept while its leaf stays the tree's expansion target).  Results must not
 * change by a bit (tests). */
int omok_debug_set_base_cache(omok_engine* e, int32_t enabled);
/* Debugging aid / A-B switch: which kernel evaluates the children of a sibling run on the difference path: 2 = k_sib_children2 (default: one wave
 * per child, windows that grow with the blocks), 1 = k_sib_children (a wave pair per child, the 7x7 window through every block; always used on the copy path).
 * Outputs agree within 2e-4 (tests); cached base positions are dropped (the kernels read different base-slot layouts).  In the MIXED operand format (the usual outcome of omok_net_commit's probe) only k_sib_children2 writes
 * the fp6 difference rows: which = 1 then returns OMOK_ERR_STATE instead of silently changing nothing (use OMOK_NET_F16X3_FP6 / _F16 engines for an A-B run). */
int omok_debug_set_children_kernel(omok_engine* e, int32_t which);
/* Debugging aid: enabled = 0 makes the fc0 window tiles of sibling rounds walk the whole 7x7 window of their bin instead of the rectangle of window pixels their rows can
 * differ in (a child differs from its base only within its stone's pixel +- 3 clipped to the board; outside that region its difference row holds exact zeros).
 * Results must not change by a bit (tests): skipped pixels contribute exact zeros. */
int omok_debug_set_window_rects(omok_engine* e, int32_t enabled);
/* Debugging aid / A-B switch: enabled = 0 makes the rounds of the run loops (omok_selfplay_run, the slots calls, omok_versus_run) scatter every request's policy
 * eagerly, as omok_execute, the step-wise calls and match episodes always do.  Default 1: such a round launches no softmax / scatter kernel -- the heads
 * write a request's logits into its node's policy row, marked raw, and the wave that first reads the row (a descent through the node once it is fully expanded, the
 * root's noise) turns it into the probabilities with the eager kernel's arithmetic; the mirror evaluation of such a ply stays logits in the same way.  Results must
 * not change by a bit (tests). */
int omok_debug_set_lazy_policy(omok_engine* e, int32_t enabled);
/* out[0] = raw rows turned into probabilities at the root-noise site, out[1] = in a descent, since omok_create.  Synchronises the engine's stream. */
int omok_debug_lazy_policy_stats(omok_engine* e, uint64_t* out);
/* Debugging aid of the launch-shape tests: what the LAST net forward of the engine (net 1) decided.  Writes min(cap, OMOK_PLAN_INTS) ints and returns that number:
 *   [0] path: 0 = plain rows (omok_evaluate_pv, mirror and root evaluations), 1 = sibling round on the copy path, 2 = on the difference path,
 *       3 = fp32 kernels, -1 = no forward yet;  [1] the host's bound on the rows (live games x K in a search round);
 *   [2] K split of the dense fc0 (1..64; 0 on paths 2 / 3);  [3] K split of the fc1 / heads GEMMs (1, 2, 4, 8; 0 on path 3);
 *   sibling rounds: [4] runs, [5] rows outside runs, [6] rows inside runs;  difference path, as chosen on the device: [7] runs whose base was evaluated in
 *   full, [8] fc0 window tiles, [9] first tile of the K-split set (== [8]: none), [10] its ways, [11] K split of the full-row fc0;
 *   [12] fc0 operand format as OMOK_STAT_FC0_FORMAT, [13] compute units the planners count with, [14] fc0 super-steps (2 N N), [15] 0.
 * Synchronises the engine's stream; changes no result.  The sibling-round counters are valid until the next omok_round_generate / omok_execute. */
#define OMOK_PLAN_INTS 16
int omok_debug_last_plan(omok_engine* e, int32_t* out, int32_t cap);

#define OMOK_STAT_SIMS 0        /* simulations run (incl. terminal hits / no-action sims) */
#define OMOK_STAT_EVALS 1       /* net evaluations (search requests + mirror evals + root) */
#define OMOK_STAT_PLY_GAMES 2   /* sum over plies of live games */
#define OMOK_STAT_FINISHED 3    /* games finished */
#define OMOK_STAT_MS_TREE 4     /* HIP-event ms in tree kernels (round+scan+scatter) */
#define OMOK_STAT_MS_TRUNK 5    /* ... net trunk kernel */
#define OMOK_STAT_MS_FC0 6      /* ... fc0 GEMM kernel */
#define OMOK_STAT_MS_TAIL 7     /* ... fc1/heads kernel */
#define OMOK_STAT_MS_PLY 8      /* ... sample/mirror/advance kernels */
#define OMOK_STAT_FC0_LAUNCHES 9
#define OMOK_STAT_FC0_ROWS 10   /* sum of batch rows over fc0 launches */
#define OMOK_STAT_TREE_BYTES 11 /* kernel-counted algorithmic bytes of the round kernels */
#define OMOK_STAT_ROUND_LAUNCHES 12
#define OMOK_STAT_MS_ROUND 13   /* HIP-event ms in the round (select/expand/backup) kernel only */
#define OMOK_STAT_PEAK_NODES 14  /* largest node / table arena use seen so far */
#define OMOK_STAT_PEAK_TABLES 15
#define OMOK_STAT_FC0_FORMAT 16  /* operand format of fc0's correction terms in use: 0 = block-scaled fp6, 1 = f16, 2 = mixed (f16 full rows, fp6 difference rows) (-1: OMOK_NET_F32) */
#define OMOK_STAT_PROBE_ROWS 17  /* rows of the last omok_net_commit's probe (0: no probe: forced format / OMOK_NET_F32) */
#define OMOK_STAT_PROBE_DP_FP6 18 /* the probe's max |dp|, |dv| against the fp32 kernels: fp6 correction terms ... */
#define OMOK_STAT_PROBE_DV_FP6 19
#define OMOK_STAT_PROBE_DP_F16 20 /* ... f16 correction terms */
#define OMOK_STAT_PROBE_DV_F16 21
#define OMOK_STAT_PROBE_LIMIT 22  /* fp6 is kept while both of its figures are <= this (3e-4) */
#define OMOK_STAT_PROBE_LOGIT_MAX 23 /* largest |policy logit| of the probe rows (fp32 kernels) */
#define OMOK_STAT_CHILDREN2_LAUNCHES 24 /* sibling rounds whose children ran on k_sib_children2 (difference path, default) ... */
#define OMOK_STAT_CHILDREN1_LAUNCHES 25 /* ... on k_sib_children (copy path; difference path after omok_debug_set_children_kernel(1)) */
#define OMOK_STAT_PROBE_DLOGIT_FP6 26 /* the probe's plain rows: max(|dlogit|, |dv before tanh|) against the fp32 kernels, fp6 / f16 correction terms */
#define OMOK_STAT_PROBE_DLOGIT_F16 27
#define OMOK_STAT_PROBE_ROUND_ROWS 28 /* rows of the probe's synthetic sibling round (difference path) that were checked against the fp32 kernels (0: this engine's
                                         rounds never take that path: games x max_batch_k below 3072 (board 15) / 1024 (board 9), or OMOK_NET_F16X3_ROWS) */
#define OMOK_STAT_PROBE_ROUND_FP6 29   /* [29..31] |dp|, |dv|, |dlogit| of that round with fp6 rows and fp6 difference rows */
#define OMOK_STAT_PROBE_ROUND_MIXED 32 /* [32..34] ... f16 rows, fp6 difference rows */
#define OMOK_STAT_PROBE_ROUND_F16 35   /* [35..37] ... f16 rows, f16 difference rows */
#define OMOK_STAT_PROBE_LOGIT_LIMIT 38 /* limit on the |dlogit| figures (5e-4); OMOK_STAT_PROBE_LIMIT (3e-4) is the one on |dp|, |dv| */
#define OMOK_STAT_PROBE_OUTSIDE 39 /* the probe's verdict on the format it committed: 0 = every figure inside the margin limits (OMOK_STAT_PROBE_LIMIT on |dp|, |dv|,
                                      OMOK_STAT_PROBE_LOGIT_LIMIT on the logits); 1 = the most precise split-operand format (f16 correction terms) is outside the margin but
                                      inside north_star's 1e-3 -- committed, one line on stderr; 2 = it is outside 1e-3: the engine evaluates this net with the plain fp32
                                      kernels (OMOK_STAT_FC0_FORMAT = -1, the arithmetic of agent_model.rs:116-134; slow) until the next omok_net_commit.  A forced format
                                      (OMOK_NET_F16X3_FP6 / _F16 / _MIXED) is never probed: 0 */
/* [40..49] executed work of the search rounds on the sibling paths since omok_reset_stats (bench.py's executed_flops): */
#define OMOK_STAT_WORK_DIFF_RUNS 40    /* difference path: runs of sibling requests ... */
#define OMOK_STAT_WORK_DIFF_SINGLES 41 /* ... request rows outside runs (evaluated in full) ... */
#define OMOK_STAT_WORK_DIFF_CHILDREN 42 /* ... request rows inside runs (k_sib_children2: a 5x5 / 7x7 window each) */
#define OMOK_STAT_WORK_COPY_RUNS 43    /* the same three on the copy path (k_trunk<BASE> per run, k_sib_children per row) */
#define OMOK_STAT_WORK_COPY_SINGLES 44
#define OMOK_STAT_WORK_COPY_CHILDREN 45
#define OMOK_STAT_WORK_DIFF_FULL_RUNS 46 /* runs of the difference path whose base was evaluated in full (base-cache misses + uncacheable runs) */
#define OMOK_STAT_WORK_WIN_PIXELS 47   /* window pixels walked by the fc0 window tiles (sum over tiles of their rectangles; K-split tiles: 49) */
#define OMOK_STAT_WORK_WIN_TILES 48    /* fc0 window tiles (128 slots each) */
#define OMOK_STAT_WORK_FULL_TILES 49   /* 128-row tiles of the difference path's full-row fc0 */
#define OMOK_STAT_MS_TRAIN_APPLY 50   /* HIP-event ms in omok_train_apply's Adadelta launch (under omok_set_profiling; tools/train_step_timing.py) */
#define OMOK_STAT_COUNT 51
int omok_get_stats(omok_engine* e, double* stats /* [OMOK_STAT_COUNT] */);
int omok_reset_stats(omok_engine* e);
/* Per-category HIP-event timing of the kernels on the engine's stream (off by default).  enabled = 1: every launch; enabled = N > 1:
   search rounds are timed 1 in N and omok_get_stats scales the sampled sums by rounds seen / rounds timed (an event record costs the
   queue ~5 us, six category boundaries per round: 2 % of a full round, 15 % of a thin one); ply-level work is always timed. */
int omok_set_profiling(omok_engine* e, int32_t enabled);

#ifdef __cplusplus
}
#endif
#endif
