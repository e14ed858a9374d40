// common.h — data layout in HBM and launch interface shared by the HIP translation units.
//
// One tree = one arena, owned by exactly one wavefront at a time.  Layout:
//   tree id t = side * G + game            (side 0 = black agent, 1 = white agent, trainer.rs:83-84)
//   (stride_nodes / stride_tables = the capacities rounded up to odd numbers: Store)
//   hdr    [T][stride_nodes]        16 B   NodeHdr  (Node fields of mcts/src/node.rs:10-21)
//   board  [T][stride_nodes][2*NW]     u64    black words, white words (bit a = cell a)
//   policy [T][stride_nodes][ROWP]     f32    BoardState.policy (alpha-zero/src/mcts_node.rs:10)
//   child tables [T][stride_tables][ROWP]: cn u32, cw f32, cidx u16, corder u8; owner [T][stride_tables]
//     a node's (n, w) live in its PARENT's table at index = action (coalesced PUCT scan);
//     child.p is parent.policy[action] (the reference keeps them equal at all times).
//   ROWP = HW rounded up to 64 (one wave iteration per 64 cells); pad cells: corder = 0xFF.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace omok {

constexpr uint16_t NONE16 = 0xFFFFu;
constexpr uint8_t NONE8 = 0xFFu;
constexpr int KMAX = 64;
constexpr float F32_EPS = 1.1920928955078125e-7f;

enum { ST_IN_PROGRESS = 0, ST_DRAW = 1, ST_BLACK_WIN = 2, ST_WHITE_WIN = 3 };
enum { RNG_EXPAND = 1, RNG_NOISE = 2, RNG_SAMPLE = 3, RNG_OPPONENT = 4, RNG_TRAIN_BATCH = 5 };

template <int N>
struct Geo {
    static constexpr int HW = N * N;
    static constexpr int ROWP = (HW + 63) / 64 * 64;
    static constexpr int NW = (HW + 63) / 64;
    static constexpr int IT = ROWP / 64;
};

struct __attribute__((aligned(16))) NodeHdr {
    uint16_t parent;
    uint16_t table;
    uint16_t legal;
    uint16_t nch;
    uint8_t action;
    uint8_t status;
    uint8_t turn;
    uint8_t has_policy; // 0: no row (the placeholder prior), 1: probabilities, 2: RAW -- the heads' logits as written, made into probabilities by the first reader
    uint32_t pad;
};
static_assert(sizeof(NodeHdr) == 16, "NodeHdr must be 16 bytes");

struct __attribute__((aligned(16))) TreeState {
    uint32_t n_nodes;
    uint32_t n_tables;
    uint32_t root_n;
    float root_w;
    uint32_t error;
    uint32_t n_req;
    uint32_t req_base;
    uint32_t pad;
};

struct GameState {
    uint8_t alive;
    uint8_t status;
    uint8_t external; // the pending move (last_action) was supplied by the caller (omok_play_actions), not sampled
    uint8_t harvested; // slots mode: the finished game's records have been packed out, the slot may take a new game
    int32_t plies;       // moves played
    int32_t last_action;
    int32_t mirror_idx;
    int32_t rp_len;      // transitions recorded = moves SAMPLED so far (turn_counts[index], src/trainer.rs:85,139,148)
    int32_t gid;         // game index of the slot's game (+ cfg.game_offset = the global id that keys its RNG streams); = the slot after a reset
    int32_t pad2[2];
};
static_assert(sizeof(GameState) == 32, "GameState must be 32 bytes");

struct Store {
    NodeHdr* hdr;
    uint64_t* board;
    float* policy;
    uint32_t* tcn;
    float* tcw;
    uint16_t* tcidx;
    uint8_t* tcorder;
    uint16_t* towner;
    TreeState* ts;
    uint16_t* req_node; // [T][KMAX]
    GameState* gs;      // [G]
    // dense request list of the current NN batch
    uint32_t* req_ref;  // (t << 16) | node
    uint32_t* req_aux;  // 0xFFFFFFFF none, else action | mode << 16 : stone to add before encoding
    int32_t* d_count;   // [0] = live batch size
    // replay
    uint64_t* rp_board; // [G][HW][2*NW]
    uint8_t* rp_turn;   // [G][HW]
    float* rp_pi;       // [G][HW][ROWP]
    float* rp_z;        // [G][HW]
    unsigned long long* d_bytes; // kernel-counted algorithmic bytes
    int cap_nodes, cap_tables, games;
    // Arena STRIDES per tree, in nodes / tables (>= the capacities): odd, so that the same node index of consecutive trees does not fall on the same HBM
    // channels.  With stride = capacity = 4224 (a multiple of 128: policy rows of 1 KiB -> a tree stride of 33 x 128 KiB) the policy scatter of a round -- 4096
    // trees writing the rows of about the same node indices -- ran at half the speed it has with 4225 (profiles/r04_arena_stride.txt).
    int stride_nodes, stride_tables;
};

struct RoundArgs {
    int side, round, K, ply;
    float epsilon, alpha;
    uint64_t seed; // Philox key of the current episode: cfg.seed + episode * 0x9E3779B97F4A7C15 (DESIGN.md "RNG contract")
    int64_t game_offset;
    const float* scatter_v; // non-NULL: the PREVIOUS round's backups (k_scatter with these values) run at the head of this round's kernel
    // run-loop rounds on the sibling path (no k_scan: the net's k_group derives the request offsets itself): req_cnt[g] = the game's requests of this round
    // (0 for a finished game), and workgroup 0 zeroes zero_ptr[0 .. zero_n) (the grouping counters the round's forward expects zeroed).  NULL: neither.
    int32_t* req_cnt;
    int32_t* zero_ptr;
    int zero_n;
    // lazy policy rows.  lazy_rows > 0 (with scatter_v): the previous round was a lazy one whose forward covered that many rows -- its requests' nodes
    // hold raw rows and are marked has_policy = 2 beside their backups.  lazy_stats (may be NULL): [0] += rows materialised at the noise site, [1] += in a descent.
    int lazy_rows;
    uint32_t* lazy_stats;
};

// ---- tree_kernels.hip launchers (all asynchronous on `st`) ---------------------------------
void launch_reset(int n, const Store& S, const float* root_policy_dev /*ROWP*/, hipStream_t st);
// Agent::new on caller-supplied positions (omok_selfplay_reset_from): boards_dev [G][HW] Stone bytes that passed launch_position_check,
// p_dev [G][ROWP] = evaluate_p of the positions (Player mode, game order); both trees of game g start at position g.  p2_dev non-NULL
// (omok_match_reset_from): the same rows from net 2; tree side * G + g takes the row of net side ^ (g >= split)
void launch_reset_from(int n, const Store& S, const uint8_t* boards_dev, const float* p_dev, const float* p2_dev, int split, hipStream_t st);
// random openings: position b = `stones` plies of the game with global id first_game + b, both sides the RANDOM scripted player drawing like
// launch_opponent_move's OMOK_OPP_RANDOM -> boards_dev [B][HW] Stone bytes, ok_dev [B] (0: a placement ended the game, the board stops there)
void launch_random_positions(int n, uint64_t key, int64_t first_game, int stones, int batch, uint8_t* boards_dev, uint8_t* ok_dev, hipStream_t st);
// boards_dev [B][HW] bytes -> verdict_dev [B] (0 legal and in progress, 1 bad byte, 2 impossible stone counts, 3 already won, 4 full board),
// stones_dev [B] (may be NULL)
void launch_position_check(int n, const uint8_t* boards_dev, int batch, int32_t* verdict_dev, int32_t* stones_dev, hipStream_t st);
// The move log of an engine (omok_game_log_enable): one allocation, [G][HW] each; entry i of game g = its move number i since the reset.
// Not part of Store: the kernels that exist without the log keep their arguments.
struct GameLog {
    uint32_t* root_n;     // TreeState::root_n / root_w of the mover's tree when the move was made
    float* root_w;
    uint32_t* child_n;    // the root table's entry of the chosen cell (0 / 0.0f: the tree did not hold the move)
    float* child_w;
    uint16_t* move;       // cell | 0x100 if the move was external (GameState::external)
    uint8_t* start_board; // Stone bytes of the position the episode started at
};
// entry gs.plies - start_ply of every game launch_advance is about to advance, read from the tree of `side` BEFORE ensure_action_exists
void launch_log_move(int n, const Store& S, int side, int start_ply, const GameLog& L, hipStream_t st);
// omok_env_replay: start_dev [B][HW] (NULL: empty boards) with their launch_position_check verdicts (NULL iff start_dev is), moves_dev [B][stride],
// lengths_dev [B] -> boards_out [B][HW], status_out [B], played_out [B] (each may be NULL)
void launch_replay(int n, const uint8_t* start_dev, const int32_t* verdict_dev, const uint16_t* moves_dev, const int32_t* lengths_dev, int batch, int stride,
                   int upto, uint8_t* boards_out, int32_t* status_out, int32_t* played_out, hipStream_t st);
// root_n / root_w of the trees of `side` of every game (0 for finished games)
void launch_root_stats(const Store& S, int side, uint32_t* n_dev, float* w_dev, hipStream_t st);
// slots mode (omok_selfplay_run_slots): finished games are packed out (records appended at *out_count, per-game meta by game index) and their
// slots restarted with the next game indices while any are left
struct SlotMeta { long long offset; int32_t len; int32_t status; }; // per game index: first record, records, final GameStatus
void launch_harvest(int n, const Store& S, uint8_t* mask_dev /*[G]*/, long long* slot_off_dev /*[G]*/, long long* out_count_dev, SlotMeta* meta_dev,
                    uint8_t* dst_dev, long long cap_records, hipStream_t st);
// omok_selfplay_run_slots_logged, directly after launch_harvest: log rows [0, len) of the slots its scan picked -> entries slot_off[g] + i of
// log_dst_dev (LOG_ENTRY_BYTES each, little-endian: root_n u32 at byte 0, root_w f32 at 4, child_n u32 at 8, child_w f32 at 12, move u16 at
// 16, zero u16 at 18), beside the records of the same indices; entries at or beyond cap_records are not written
constexpr int LOG_ENTRY_BYTES = 20;
void launch_harvest_log(int n, const Store& S, const GameLog& L, const uint8_t* mask_dev, const long long* slot_off_dev, uint8_t* log_dst_dev,
                        long long cap_records, hipStream_t st);
void launch_refill(int n, const Store& S, const float* root_policy_dev, int32_t* next_gid_dev, int total_games, int32_t* new_gid_dev /*[G]*/, hipStream_t st);
void launch_round(int n, const Store& S, const RoundArgs& a, hipStream_t st);
// evals_dev[0] += the round's requests; zero_ptr[0 .. zero_n) = 0 (counters the round's forward expects zeroed); fill = false: the dense
// (tree, node) list is written by the net's grouping kernel instead (run-loop rounds on the sibling path: k_group visits every request anyway)
void launch_fill(const Store& S, int side, int K, hipStream_t st); // the dense request list alone (k_fill): what launch_scan(fill = true) appends
void launch_scan(int n, const Store& S, int side, int K, hipStream_t st, unsigned long long* evals_dev = nullptr, int32_t* zero_ptr = nullptr, int zero_n = 0,
                 bool fill = true);
// one tree searched by `waves` waves (MCTSExecutor::run): sh_req [waves][KMAX] u16, sh_cnt [2 * KMAX] u32 (counts | bases)
// rec_order / rec_pos non-NULL: RECORDED mode -- every simulation (round kernel) / every backup (scatter kernel) runs under the tree lock and
// appends its wave's index to rec_order[(*rec_pos)++]: an exactly replayable interleaving (omok_execute_shared_recorded)
void launch_round_shared(int n, const Store& S, const RoundArgs& a, int rounds_total, int group, int waves, uint16_t* sh_req, uint32_t* sh_cnt,
                         hipStream_t st, uint8_t* rec_order = nullptr, uint32_t* rec_pos = nullptr);
void launch_scatter_shared(int n, const Store& S, int side, const float* p_dev, const float* v_dev, int max_count, int waves, const uint16_t* sh_req,
                           const uint32_t* sh_cnt, hipStream_t st, uint8_t* rec_order = nullptr, uint32_t* rec_pos = nullptr);
constexpr int MAX_TREE_WAVES = 16; // one workgroup of 1024 threads
constexpr int MAX_GAMES = 32767;         // games per engine (omok_create)
constexpr int SCAN_GAMES_PER_THREAD = 32; // k_scan: one workgroup of 1024 threads, each owning this many consecutive games
// backups = false: the policies only; the backups (k_scatter) are deferred to launch_backups or into the next round's kernel (RoundArgs::scatter_v)
void launch_scatter(int n, const Store& S, int side, const float* p_dev, const float* v_dev, int max_count, hipStream_t st, bool backups = true);
// raw_rows > 0: the round was a lazy one of that many rows at most: its requests' nodes are marked has_policy = 2 (raw rows, see RoundArgs::lazy_rows)
void launch_backups(int n, const Store& S, int side, const float* v_dev, hipStream_t st, int raw_rows = 0);
// every raw policy row of trees [tree_first, tree_first + trees) -> probabilities, has_policy = 1 (what a reader outside k_round runs first)
void launch_materialise(int n, const Store& S, int tree_first, int trees, hipStream_t st);
// the same from the net's logits (softmax / tanh of the split-precision path fused into the policy scatter): writes v, vpre, the trees
void launch_softmax_scatter(int n, const Store& S, int side, const float* logits_dev, int lrow, float* v_dev, float* vpre_dev, int max_count,
                            hipStream_t st, bool backups = true);
void launch_sample(int n, const Store& S, int side, int ply, float temperature, int threshold, uint64_t seed,
                   int64_t game_offset, int32_t* actions_dev, hipStream_t st);
void launch_mirror_scan(int n, const Store& S, int side, hipStream_t st);
// raw: p_dev holds the mirror evaluation's LOGITS rows ([rows][ROWP]); a node ensure_action_exists creates takes its row as a raw policy row (has_policy = 2)
void launch_advance(int n, const Store& S, int side, const float* p_dev, hipStream_t st, bool raw = false);
void launch_encode_requests(int n, const Store& S, float* out_dev /*[B][3HW]*/, int max_b, hipStream_t st);
void launch_env_play(int n, const int32_t* moves_dev, int batch, int len, int32_t* status_dev, uint8_t* boards_dev,
                     uint8_t* turns_dev, uint16_t* legal_dev, hipStream_t st);
void launch_encode_boards(int n, const uint8_t* boards_dev, const uint8_t* turns_dev, int batch, int mode,
                          float* out_dev, hipStream_t st);
void launch_replay_pack(int n, const Store& S, const long long* offsets_dev, uint8_t* dst_dev, long long cap_records, hipStream_t st);
void launch_replay_offsets(int n, const Store& S, int per_transition, long long* offsets_dev /*[games + 1]*/, hipStream_t st);
void launch_set_actions(int n, const Store& S, int side, const int32_t* actions_dev, uint32_t* d_flags /*[0] illegal, [1] missing*/, hipStream_t st);
void launch_clear_actions(const Store& S, hipStream_t st);
// the scripted players of the evaluation games (kind = OMOK_OPP_*: random and naive of src/trainer.rs:400-603, the threat-aware player, and the one
// with the forced-win solver, which alone uses depth / nodes = OMOK_VCF_OPP_DEPTH / OMOK_VCF_OPP_NODES): the move of the side to move of every live game,
// staged like launch_set_actions (external) and copied to actions_dev [G] (-1: finished game)
// OMOK_OPP_GUARD goes through launch_guard on the engine's scratch guard_out_dev [4][G] and guard_status_dev [G][HW] (unused by the other kinds)
void launch_opponent_move(int n, const Store& S, int side, int kind, uint64_t seed, int64_t game_offset, int depth, int nodes, int32_t* actions_dev, hipStream_t st,
                          int32_t* guard_out_dev = nullptr, uint8_t* guard_status_dev = nullptr);
// where the defending player's passes take their positions from: the live games' root boards of `side` with the draw word of launch_opponent_move
// (boards == nullptr: position b = game b, a finished game gets cell -1), or caller-held boards [B][HW], turns [B] and draw words [B] (NULL: all 0)
struct GuardSrc { const uint8_t* boards; const uint8_t* turns; const uint32_t* draws; int side; uint64_t seed; int64_t game_offset; };
// OMOK_OPP_GUARD's move of `batch` positions in three stream-ordered launches (first pass, map pass, pick pass; no host read-back between them):
// out_dev [4][batch] = cell, step, level, count; status_dev [batch][HW] scratch of the map pass; actions_dev (the live form, else NULL): the move staged
// like launch_opponent_move's
void launch_guard(int n, const Store& S, const GuardSrc& src, int batch, int depth, int nodes, int32_t* out_dev, uint8_t* status_dev, int32_t* actions_dev,
                  hipStream_t st);
// the same rule on caller-held positions: boards_dev [B][HW] Stone bytes, turns_dev [B] (0 / 1; read by the threat-aware kinds alone, else may be NULL)
// -> cell_dev (the cell the rule is forced to, -1 where it would draw), level_dev, count_dev [B]; each may be NULL
void launch_env_scripted(int n, int kind, const uint8_t* boards_dev, const uint8_t* turns_dev, int batch, int depth, int nodes, int32_t* cell_dev,
                         int32_t* level_dev, int32_t* count_dev, hipStream_t st);
// the forced-win solver (victory by continuous fours, omok_env_vcf_solve) on caller-held positions: depth 1..16 attacker moves, nodes 1..65536 per
// position -> verdict_dev, cell_dev, moves_dev, nodes_dev [B], pv_dev [B][2 * depth - 1]; each may be NULL
void launch_env_vcf(int n, const uint8_t* boards_dev, const uint8_t* turns_dev, int batch, int depth, int nodes, int32_t* verdict_dev, int32_t* cell_dev,
                    int32_t* moves_dev, int32_t* nodes_dev, int32_t* pv_dev, hipStream_t st);
// the defender's half (omok_env_vcf_defend): per empty cell the solver with the mover's stone there and the other side attacking, and the null move;
// a wave per (position, cell) -> status_dev, moves_dev [B][HW] bytes, nodes_dev, reply_dev [B][HW], threat_dev [B][3]; each may be NULL
void launch_env_vcf_defend(int n, const uint8_t* boards_dev, const uint8_t* turns_dev, int batch, int depth, int nodes, uint8_t* status_dev,
                           uint8_t* moves_dev, int32_t* nodes_dev, int32_t* reply_dev, int32_t* threat_dev, hipStream_t st);
void launch_policy(int n, const Store& S, int side, float* pi_dev /*[G][HW]*/, uint8_t* has_dev /*[G]*/, hipStream_t st);
void launch_env_place(int n, uint8_t* boards_dev, uint8_t* turns_dev, uint16_t* legal_dev, const int32_t* actions_dev, int batch,
                      int32_t* status_dev, hipStream_t st);
int set_advance_lds_attribute(int n, size_t bytes);
void launch_replay_augment(int n, const Store& S, const long long* offsets_dev, int game_first, int game_count, long long base_sub,
                           uint8_t* dst_dev, long long cap_records, hipStream_t st);
// the same on caller-held packed records: first_dev [m + 1] = exclusive scan of the lengths of the m non-empty games, span_dev [m] = each game's
// first source record in src_dev and first destination record in dst_dev; `transitions` = first[m] waves
struct AugSpan { long long src, dst; };
void launch_replay_augment_records(int n, const uint8_t* src_dev, const long long* first_dev, const AugSpan* span_dev, int m, long long transitions,
                                   uint8_t* dst_dev, long long cap_records, hipStream_t st);
size_t advance_lds_bytes(int cap_nodes, int cap_tables);

// match episodes (omok_match_reset; tree side * G + g is evaluated by net side ^ (g >= split)): the dense list of trees of `tree_side` in S.req_ref,
// S.d_count[0] rows -> block 0 (games < split) stays there, cnt[0] rows; block 1 is copied to ref2 / aux2, cnt[1] rows; evals[net] += the rows of each net
void launch_match_split(const Store& S, int tree_side, int split, uint32_t* ref2, uint32_t* aux2, int32_t* cnt, unsigned long long* evals, int max_rows,
                        hipStream_t st);
// block 1's outputs (v2 and / or p2 [rows][rowp], NULL: skipped) behind block 0's in v1 / p1: one array in list order
void launch_match_join(const int32_t* cnt, const float* v2, float* v1, const float* p2, float* p1, int rowp, int max_rows, hipStream_t st);
// the root policy of the trees net 2 owns (after launch_reset with net 1's)
void launch_match_roots(int n, const Store& S, const float* root_policy2, int split, hipStream_t st);

// ---- net_kernels.hip --------------------------------------------------------------------------
struct NetBuffers; // defined in net.h
} // namespace omok
