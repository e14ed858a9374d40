// engine.cpp — host side of libomok_mi355x.so: the opaque handle, HBM allocation, kernel
// orchestration and the C ABI of include/omok_mi355x.h.
//
// Mirrors the reference's host control flow:
//   omok_execute       <- ParallelMCTSExecutor::execute (alpha-zero/src/parallel_mcts_executor.rs:26-270)
//   omok_selfplay_run  <- Trainer::train self-play phase (src/trainer.rs:95-205)
// but enqueues a whole execute() (all rounds) on one HIP stream without host round trips: the
// live batch size stays on the device (Store::d_count) and the net kernels bound themselves by it.
#include "../../include/omok_mi355x.h"
#include "common.h"
#include "net.h"
#include "train.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace omok;

// ---------------------------------------------------------------------------------------------
hipEvent_t Prof::get() {
    if (n_pool > 0) return pool[--n_pool];
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
}
void Prof::begin(int cat, hipStream_t st, bool counted) {
    if (!enabled || !active) return;
    if (n_items == cap_items) {
        if (cap_items >= 8192) resolve();
        else {
            cap_items = cap_items ? cap_items * 2 : 1024;
            items = (Item*)realloc(items, sizeof(Item) * cap_items);
        }
    }
    Item it{cat, in_round, counted, get(), get()};
    hipEventRecord(it.a, st);
    items[n_items++] = it;
}
void Prof::end(hipStream_t st) {
    if (!enabled || !active || n_items == 0) return;
    hipEventRecord(items[n_items - 1].b, st);
}
void Prof::resolve() {
    if (n_items == 0) return;
    hipEventSynchronize(items[n_items - 1].b);
    if (cap_pool < n_pool + 2 * n_items) {
        cap_pool = n_pool + 2 * n_items + 64;
        pool = (hipEvent_t*)realloc(pool, sizeof(hipEvent_t) * cap_pool);
    }
    for (int i = 0; i < n_items; ++i) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, items[i].a, items[i].b) == hipSuccess) {
            const int n = items[i].counted ? 1 : 0;
            if (items[i].sampled) { ms_s[items[i].cat] += t; launches_s[items[i].cat] += n; }
            else { ms[items[i].cat] += t; launches[items[i].cat] += n; }
        }
        pool[n_pool++] = items[i].a;
        pool[n_pool++] = items[i].b;
    }
    n_items = 0;
}
void Prof::destroy() {
    resolve();
    for (int i = 0; i < n_pool; ++i) hipEventDestroy(pool[i]);
    free(pool);
    free(items);
    pool = nullptr; items = nullptr; n_pool = cap_pool = n_items = cap_items = 0;
}

// ---------------------------------------------------------------------------------------------
struct omok_engine {
    omok_config cfg{};
    int n = 0, hw = 0, rowp = 0, nw = 0, T = 0;
    Store S{};
    Net net{};
    Prof prof{};
    hipStream_t st = nullptr;
    std::vector<void*> allocs;
    std::string err;
    int ply = 0;
    int start_ply = 0;     // ply the episode started at: 0, or the stone count of the positions of omok_selfplay_reset_from
    bool reset_done = false;
    bool sampled = false;
    uint64_t episode = 0;  // index of the RNG stream the NEXT omok_selfplay_reset takes (one reset = one trainer iteration)
    uint64_t key = 0;      // Philox key of the current episode: cfg.seed + episode * 0x9E3779B97F4A7C15
    int round_reqs = -1;   // step-wise API state
    int round_cap = 0;     // alive * batch_size of the generated round: the net's max_count (same as omok_execute uses)
    int mirror_reqs = -1;
    float* d_root_policy = nullptr;
    int32_t* d_actions = nullptr;
    uint32_t* d_error = nullptr; // [0] error bits, [1] alive count
    unsigned long long* d_evals = nullptr;
    uint32_t* d_lazy = nullptr;         // [4] rows materialised at the noise site, in a descent (omok_debug_lazy_policy_stats); 2 spare
    bool lazy_policy = true;            // run-loop rounds leave raw policy rows (omok_debug_set_lazy_policy)
    int32_t* d_req_cnt = nullptr;       // [G] requests of every game in the current round (k_round -> k_group: run-loop rounds on the sibling path)
    uint16_t* d_sh_req = nullptr;       // [MAX_TREE_WAVES][KMAX] requests of the waves of a shared-tree round group
    uint32_t* d_sh_cnt = nullptr;       // [2 * KMAX] their counts | first-request offsets
    uint32_t* d_flags = nullptr;        // [0] illegal external moves, [1] live games without a move (omok_play_actions)
    float* d_pi = nullptr;              // [G][HW] omok_compute_policy
    uint8_t* d_has = nullptr;           // [G]
    long long* d_aug_offsets = nullptr; // [games + 1] first augmented-replay record of every game
    uint8_t* d_aug_scratch = nullptr;   // one game's 6 * HW records (omok_replay_augmented_game)
    // second net slot and match episodes (omok_net2_*, omok_match_reset)
    Net* net2 = nullptr;                // allocated on its first load
    bool match = false;                 // the current episode is a match: tree side * G + g is evaluated by net side ^ (g >= split) (0 = net, 1 = net2)
    int split = 0;
    int match_cnt[2] = {0, 0};          // rows of the two blocks of the pending step-wise round / mirror batch (launch_match_split)
    uint32_t* d_mref = nullptr;         // [max_b] the second block's request list
    uint32_t* d_maux = nullptr;
    int32_t* d_mcnt = nullptr;          // [0] rows of the first block (games < split), [1] of the second
    unsigned long long* d_mevals = nullptr; // [2] rows evaluated by net 1 / net 2 in match episodes
    float* d_root_policy2 = nullptr;
    Train* train = nullptr;             // buffers and optimizer state of the native training step (omok_train_begin .. omok_train_end)
    // move log (omok_game_log_enable): allocated on the first enable, freed by a disable
    bool log_on = false;
    bool log_started = false;           // a reset has set the log's start since it was enabled: moves are logged, omok_game_log_read answers
    void* log_mem = nullptr;            // the one allocation GameLog points into
    GameLog log{};
    // OMOK_OPP_GUARD on the live games: allocated on the first use of that kind (ensure_guard_scratch), freed with the engine's allocations
    int32_t* d_guard_out = nullptr;     // [4][G] cell, step, level, count: the first pass's results and its carry to the pick pass
    uint8_t* d_guard_status = nullptr;  // [G][HW] the map pass's status rows
    // host-side stats
    double sims = 0, evals = 0, ply_games = 0, finished = 0;
    uint32_t peak_nodes = 0, peak_tables = 0;
    size_t bytes = 0;
};

static std::string g_create_error;

static int fail(omok_engine* e, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (e) e->err = buf; else g_create_error = buf;
    return code;
}

#define HIPCHK(e, call)                                                                        \
    do {                                                                                       \
        hipError_t _r = (call);                                                                \
        if (_r != hipSuccess) return fail(e, OMOK_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(_r)); \
    } while (0)

// every entry point runs on the engine's own device, whatever the calling thread's current device is
#define ENTER(e)                                    \
    do {                                            \
        if (!(e)) return OMOK_ERR_INVALID;          \
        HIPCHK(e, hipSetDevice((e)->cfg.device));   \
    } while (0)

template <typename Tp>
static int dalloc(omok_engine* e, Tp** p, size_t count) {
    void* q = nullptr;
    const size_t bytes = count * sizeof(Tp);
    hipError_t r = hipMalloc(&q, bytes ? bytes : 16);
    if (r != hipSuccess) return fail(e, OMOK_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(r));
    e->allocs.push_back(q);
    e->bytes += bytes;
    *p = (Tp*)q;
    return 0;
}

// Device scratch of one call (the engine-lifetime buffers are dalloc's): whatever get() handed out is freed when the holder goes out of scope,
// on every return path.  get() returns nullptr and sets `failed` when an allocation fails; the caller reports it with fail().
struct Scratch {
    std::vector<void*> ptrs;
    bool failed = false;
    Scratch() = default;
    Scratch(Scratch&&) = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() { for (void* p : ptrs) hipFree(p); }
    template <typename Tp>
    Tp* get(size_t count) {
        void* q = nullptr;
        if (hipMalloc(&q, count * sizeof(Tp)) != hipSuccess) { failed = true; return nullptr; }
        ptrs.push_back(q);
        return (Tp*)q;
    }
};

// tiny helper kernels --------------------------------------------------------------------------
__global__ void k_count_alive(Store S, uint32_t* d_error, unsigned long long* d_evals) {
    __shared__ uint32_t s_cnt, s_err, s_mn, s_mt;
    if (threadIdx.x == 0) { s_cnt = 0; s_err = 0; s_mn = 0; s_mt = 0; }
    __syncthreads();
    uint32_t c = 0, er = 0, mn = 0, mt = 0;
    for (int g = threadIdx.x; g < S.games; g += blockDim.x) {
        c += S.gs[g].alive ? 1u : 0u;
        const TreeState a = S.ts[g], b = S.ts[S.games + g];
        er |= a.error | b.error;
        mn = max(mn, max(a.n_nodes, b.n_nodes));
        mt = max(mt, max(a.n_tables, b.n_tables));
    }
    atomicAdd(&s_cnt, c);
    atomicOr(&s_err, er);
    atomicMax(&s_mn, mn);
    atomicMax(&s_mt, mt);
    __syncthreads();
    if (threadIdx.x == 0) { d_error[0] = s_err; d_error[1] = s_cnt; d_error[2] = s_mn; d_error[3] = s_mt; }
}
__global__ void k_add_evals(const int32_t* d_count, unsigned long long* d_evals) {
    if (threadIdx.x == 0 && blockIdx.x == 0) d_evals[0] += (unsigned long long)d_count[0];
}
__global__ void k_copy_root_policy(const float* p, float* dst, int hw, int rowp) {
    const int a = threadIdx.x;
    if (a < rowp) dst[a] = a < hw ? p[a] : 0.0f;
}
__global__ void k_pack_rows(const float* src, float* dst, int hw, int rowp, int rows) { // [rows][ROWP] -> [rows][HW]
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)rows * hw) dst[i] = src[(i / hw) * rowp + (i % hw)];
}
__global__ void k_unpack_rows(const float* src, float* dst, int hw, int rowp, int rows) { // [rows][HW] -> [rows][ROWP]
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)rows * rowp) dst[i] = (int)(i % rowp) < hw ? src[(i / rowp) * hw + (i % rowp)] : 0.0f;
}

// ---------------------------------------------------------------------------------------------
extern "C" const char* omok_last_error(const omok_engine* e) { return e ? e->err.c_str() : g_create_error.c_str(); }

extern "C" void omok_destroy(omok_engine* e) {
    if (!e) return;
    hipSetDevice(e->cfg.device);
    if (e->st) hipStreamSynchronize(e->st);
    e->prof.destroy();
    net_free(e->net);
    if (e->net2) { net_free(*e->net2); delete e->net2; }
    if (e->train) { train_free(*e->train); delete e->train; }
    if (e->log_mem) hipFree(e->log_mem);
    for (void* p : e->allocs) hipFree(p);
    if (e->st) hipStreamDestroy(e->st);
    delete e;
}

// a Net of this engine's board size, net mode and batch capacity (before net_alloc)
static void configure_net(omok_engine* e, Net& net, int max_b) {
    const omok_config* cfg = &e->cfg;
    net.device = cfg->device;
    net.n = e->n;
    net.hw = e->hw;
    net.rowp = e->rowp;
    net.mode = cfg->net_mode == OMOK_NET_F32 ? OMOK_NET_F32 : OMOK_NET_F16X3;
    net.siblings = cfg->net_mode != OMOK_NET_F16X3_ROWS;
    net.fc0_policy = cfg->net_mode == OMOK_NET_F16X3_FP6 ? FC0_FP6 : cfg->net_mode == OMOK_NET_F16X3_F16 ? FC0_F16
                   : cfg->net_mode == OMOK_NET_F16X3_MIXED ? FC0_MIXED : FC0_AUTO;
    net.max_b = max_b;
    net.games = cfg->games;
    for (int i = 0; i < NET_TENSORS; ++i) net.wsize[i] = net_tensor_size(e->n, i);
}

extern "C" int omok_create(const omok_config* cfg, omok_engine** out) {
    if (!cfg || !out) return fail(nullptr, OMOK_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->board_size != 9 && cfg->board_size != 15)
        return fail(nullptr, OMOK_ERR_INVALID, "board_size must be 9 or 15 (got %d)", cfg->board_size);
    if (cfg->games < 1 || cfg->games > MAX_GAMES) return fail(nullptr, OMOK_ERR_INVALID, "games must be in [1, %d]", MAX_GAMES);
    if (cfg->max_nodes < 2 || cfg->max_nodes > OMOK_MAX_ARENA || cfg->max_tables < 1 || cfg->max_tables > OMOK_MAX_ARENA)
        return fail(nullptr, OMOK_ERR_INVALID, "max_nodes must be in [2, %d] and max_tables in [1, %d]", OMOK_MAX_ARENA, OMOK_MAX_ARENA);
    if (cfg->max_batch_k < 1 || cfg->max_batch_k > KMAX) return fail(nullptr, OMOK_ERR_INVALID, "max_batch_k must be in [1, 64]");
    if (cfg->net_mode != OMOK_NET_F16X3 && cfg->net_mode != OMOK_NET_F32 && cfg->net_mode != OMOK_NET_F16X3_ROWS && cfg->net_mode != OMOK_NET_F16X3_FP6 &&
        cfg->net_mode != OMOK_NET_F16X3_F16 && cfg->net_mode != OMOK_NET_F16X3_MIXED)
        return fail(nullptr, OMOK_ERR_INVALID, "bad net_mode");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, OMOK_ERR_HIP, "no HIP device available: this library has no CPU path");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, OMOK_ERR_INVALID, "device %d out of range (%d devices)", cfg->device, ndev);
    { // the re-rooting kernel keeps 3 B per node + 2 B per table in LDS: refuse arenas it could not launch with
        hipDeviceProp_t prop;
        const size_t lds = advance_lds_bytes(cfg->max_nodes, cfg->max_tables);
        if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) return fail(nullptr, OMOK_ERR_HIP, "hipGetDeviceProperties failed");
        const size_t limit = prop.sharedMemPerBlockOptin > prop.sharedMemPerBlock ? prop.sharedMemPerBlockOptin : prop.sharedMemPerBlock;
        if (lds > limit)
            return fail(nullptr, OMOK_ERR_INVALID, "max_nodes=%d / max_tables=%d need %zu bytes of LDS in the re-rooting kernel, the device allows %zu",
                        cfg->max_nodes, cfg->max_tables, lds, limit);
    }
    omok_engine* e = new omok_engine();
    e->cfg = *cfg;
    e->n = cfg->board_size;
    e->hw = e->n * e->n;
    e->rowp = (e->hw + 63) / 64 * 64;
    e->nw = (e->hw + 63) / 64;
    e->T = 2 * cfg->games;
    hipError_t r = hipSetDevice(cfg->device);
    if (r == hipSuccess) r = hipStreamCreateWithFlags(&e->st, hipStreamNonBlocking);
    if (r != hipSuccess) {
        g_create_error = std::string("HIP init failed: ") + hipGetErrorString(r);
        delete e;
        return OMOK_ERR_HIP;
    }
    Store& S = e->S;
    S.cap_nodes = cfg->max_nodes;
    S.cap_tables = cfg->max_tables;
    S.stride_nodes = cfg->max_nodes | 1;   // odd strides: consecutive trees on different HBM channels (common.h, Store)
    S.stride_tables = cfg->max_tables | 1;
    S.games = cfg->games;
    const size_t T = (size_t)e->T, cn = (size_t)S.stride_nodes, ct = (size_t)S.stride_tables, rp = (size_t)e->rowp;
    const size_t G = (size_t)cfg->games, HW = (size_t)e->hw;
    if (cfg->max_tree_waves < 0 || cfg->max_tree_waves > MAX_TREE_WAVES)
        { omok_destroy(e); return fail(nullptr, OMOK_ERR_INVALID, "max_tree_waves must be in [0, %d]", MAX_TREE_WAVES); }
    const size_t max_b = std::max(G, (size_t)cfg->max_tree_waves) * (size_t)cfg->max_batch_k;
    int rc = 0;
    rc |= dalloc(e, &S.hdr, T * cn);
    rc |= dalloc(e, &S.board, T * cn * 2 * e->nw);
    rc |= dalloc(e, &S.policy, T * cn * rp);
    rc |= dalloc(e, &S.tcn, T * ct * rp);
    rc |= dalloc(e, &S.tcw, T * ct * rp);
    rc |= dalloc(e, &S.tcidx, T * ct * rp);
    rc |= dalloc(e, &S.tcorder, T * ct * rp);
    rc |= dalloc(e, &S.towner, T * ct);
    rc |= dalloc(e, &S.ts, T);
    rc |= dalloc(e, &S.req_node, T * KMAX);
    rc |= dalloc(e, &S.gs, G);
    rc |= dalloc(e, &S.req_ref, max_b);
    rc |= dalloc(e, &S.req_aux, max_b);
    rc |= dalloc(e, &S.d_count, 4);
    rc |= dalloc(e, &S.rp_board, G * HW * 2 * e->nw);
    rc |= dalloc(e, &S.rp_turn, G * HW);
    rc |= dalloc(e, &S.rp_pi, G * HW * rp);
    rc |= dalloc(e, &S.rp_z, G * HW);
    rc |= dalloc(e, &S.d_bytes, 2);
    rc |= dalloc(e, &e->d_root_policy, rp);
    rc |= dalloc(e, &e->d_actions, G);
    rc |= dalloc(e, &e->d_error, 4);
    rc |= dalloc(e, &e->d_evals, 2);
    rc |= dalloc(e, &e->d_req_cnt, G);
    rc |= dalloc(e, &e->d_lazy, 4);
    rc |= dalloc(e, &e->d_sh_req, (size_t)MAX_TREE_WAVES * KMAX);
    rc |= dalloc(e, &e->d_sh_cnt, 2 * (size_t)KMAX);
    rc |= dalloc(e, &e->d_flags, 4);
    rc |= dalloc(e, &e->d_pi, G * HW);
    rc |= dalloc(e, &e->d_has, G);
    rc |= dalloc(e, &e->d_aug_offsets, G + 1);
    if (rc) {
        g_create_error = e->err;
        omok_destroy(e);
        return OMOK_ERR_HIP;
    }
    hipMemsetAsync(S.d_count, 0, 16, e->st);
    hipMemsetAsync(S.d_bytes, 0, 16, e->st);
    hipMemsetAsync(e->d_error, 0, 16, e->st);
    hipMemsetAsync(e->d_evals, 0, 16, e->st);
    hipMemsetAsync(e->d_lazy, 0, 16, e->st);
    hipMemsetAsync(S.gs, 0, sizeof(GameState) * G, e->st);
    hipMemsetAsync(S.ts, 0, sizeof(TreeState) * T, e->st);
    if (set_advance_lds_attribute(e->n, advance_lds_bytes(cfg->max_nodes, cfg->max_tables)) != 0) {
        g_create_error = "hipFuncSetAttribute(k_advance, max dynamic LDS) failed";
        omok_destroy(e);
        return OMOK_ERR_HIP;
    }
    configure_net(e, e->net, (int)max_b);
    if (net_alloc(e->net) == 0) {
        g_create_error = "net buffer allocation failed (hipMalloc)";
        omok_destroy(e);
        return OMOK_ERR_HIP;
    }
    if (hipStreamSynchronize(e->st) != hipSuccess) {
        g_create_error = "stream sync failed after init";
        omok_destroy(e);
        return OMOK_ERR_HIP;
    }
    *out = e;
    return OMOK_OK;
}

// ---- net ---------------------------------------------------------------------------------------
extern "C" int omok_net_num_tensors(void) { return NET_TENSORS; }
extern "C" int64_t omok_net_tensor_size(const omok_engine* e, int index) { return e ? net_tensor_size(e->n, index) : -1; }

static int sync_and_check(omok_engine* e, const char* what);

// net slot 1 = e->net, slot 2 = *e->net2 (allocated on its first load, with the buffers of the match episodes: engines that never load it pay nothing)
static int net2_alloc(omok_engine* e) {
    if (e->net2) return 0;
    // the match buffers first: e->net2 is set only once everything a match needs exists (a failed attempt leaves the slot empty, the next load retries;
    // buffers an earlier attempt did allocate are kept)
    const size_t mb = (size_t)e->net.max_b;
    if (!e->d_mref && dalloc(e, &e->d_mref, mb)) return OMOK_ERR_HIP;
    if (!e->d_maux && dalloc(e, &e->d_maux, mb)) return OMOK_ERR_HIP;
    if (!e->d_mcnt && dalloc(e, &e->d_mcnt, 4)) return OMOK_ERR_HIP;
    if (!e->d_mevals && dalloc(e, &e->d_mevals, 2)) return OMOK_ERR_HIP;
    if (!e->d_root_policy2 && dalloc(e, &e->d_root_policy2, (size_t)e->rowp)) return OMOK_ERR_HIP;
    HIPCHK(e, hipMemset(e->d_mcnt, 0, 16));
    HIPCHK(e, hipMemset(e->d_mevals, 0, 16));
    Net* n2 = new Net();
    configure_net(e, *n2, e->net.max_b);
    if (net_alloc(*n2) == 0) { delete n2; return fail(e, OMOK_ERR_HIP, "net 2 buffer allocation failed (hipMalloc)"); } // (net_alloc frees what it got)
    e->net2 = n2;
    return 0;
}

static int net_load_slot(omok_engine* e, int slot, int index, const float* data, int64_t count) {
    if (!e || !data) return OMOK_ERR_INVALID;
    if (index < 0 || index >= NET_TENSORS) return fail(e, OMOK_ERR_INVALID, "tensor index %d out of range", index);
    if (count != e->net.wsize[index]) return fail(e, OMOK_ERR_INVALID, "tensor %d: expected %lld values, got %lld", index, (long long)e->net.wsize[index], (long long)count);
    HIPCHK(e, hipSetDevice(e->cfg.device));
    if (slot == 2 && net2_alloc(e)) return OMOK_ERR_HIP;
    Net& net = slot == 2 ? *e->net2 : e->net;
    HIPCHK(e, hipMemcpyAsync(net.w[index], data, sizeof(float) * (size_t)count, hipMemcpyHostToDevice, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    net.loaded[index] = true;
    net.committed = false;
    return OMOK_OK;
}

static int net_commit_slot(omok_engine* e, int slot) {
    if (!e) return OMOK_ERR_INVALID;
    if (slot == 2 && !e->net2) return fail(e, OMOK_ERR_STATE, "net 2: no tensor was ever loaded");
    Net& net = slot == 2 ? *e->net2 : e->net;
    for (int i = 0; i < NET_TENSORS; ++i)
        if (!net.loaded[i]) return fail(e, OMOK_ERR_STATE, "tensor %d was never loaded", i);
    HIPCHK(e, hipSetDevice(e->cfg.device));
    if (e->round_reqs >= 0 || e->mirror_reqs >= 0) return fail(e, OMOK_ERR_STATE, "omok_net_commit while a round / mirror batch is pending");
    if (net_commit(net, e->S, e->st) != 0) return fail(e, OMOK_ERR_HIP, "weight packing / format probe failed");
    net_invalidate_sibling_cache(net); // (new weights: cached base evaluations are void)
    HIPCHK(e, hipStreamSynchronize(e->st));
    net.committed = true;
    return OMOK_OK;
}

extern "C" int omok_net_load(omok_engine* e, int index, const float* data, int64_t count) { return net_load_slot(e, 1, index, data, count); }
extern "C" int omok_net_commit(omok_engine* e) { return net_commit_slot(e, 1); }
extern "C" int omok_net2_load(omok_engine* e, int index, const float* data, int64_t count) { return net_load_slot(e, 2, index, data, count); }
extern "C" int omok_net2_commit(omok_engine* e) { return net_commit_slot(e, 2); }

extern "C" int omok_net2_info(omok_engine* e, int32_t* fc0_format, int32_t* probe_outside, double* evals) {
    if (!e) return OMOK_ERR_INVALID;
    if (!e->net2 || !e->net2->committed) return fail(e, OMOK_ERR_STATE, "net 2 not loaded/committed (omok_net2_load x31 + omok_net2_commit)");
    ENTER(e);
    const Net& n2 = *e->net2;
    if (fc0_format) *fc0_format = n2.mode == OMOK_NET_F32 ? -1 : (n2.diff_fp6 ? FC0_MIXED : n2.fc0_fmt);
    if (probe_outside) *probe_outside = n2.probe_outside;
    if (evals) {
        unsigned long long ev[2] = {0, 0};
        if (sync_and_check(e, "net2_info")) return OMOK_ERR_HIP;
        HIPCHK(e, hipMemcpy(ev, e->d_mevals, sizeof(ev), hipMemcpyDeviceToHost));
        evals[0] = (double)ev[0];
        evals[1] = (double)ev[1];
    }
    return OMOK_OK;
}

// ---- weights file: ModelIO::save / ModelIO::load (alpha-zero/src/model_io.rs:20-24,59-120) ---------------------
// bincode 1.3.3 default options: little-endian, fixed-width integers; Vec<T> = u64 length + elements; String = u64
// byte length + UTF-8 bytes.  SavedData = { variable_names: Vec<String>, parameters: Vec<Vec<f32>> }.
static const char* net_tensor_name(int i, char* buf, size_t cap) {
    static const char* head[2] = {"conv_w", "conv_b"};
    static const char* blk[7] = {"conv0_w", "conv0_b", "conv1_w(depthwise)", "conv1_w(pointwise)", "conv1_b", "conv2_w", "conv2_b"};
    static const char* tail[8] = {"fc0_w", "fc0_b", "fc1_w", "fc1_b", "v_fc0_w", "v_fc0_b", "p_fc0_w", "p_fc0_b"};
    if (i < 2) snprintf(buf, cap, "%s", head[i]);
    else if (i < 23) snprintf(buf, cap, "residual_%d_%s", (i - 2) / 7, blk[(i - 2) % 7]);
    else snprintf(buf, cap, "%s", tail[i - 23]);
    return buf;
}

static bool rd_u64(FILE* f, uint64_t* v) {
    unsigned char b[8];
    if (fread(b, 1, 8, f) != 8) return false;
    uint64_t x = 0;
    for (int i = 7; i >= 0; --i) x = (x << 8) | b[i];
    *v = x;
    return true;
}
static bool wr_u64(FILE* f, uint64_t v) {
    unsigned char b[8];
    for (int i = 0; i < 8; ++i) b[i] = (unsigned char)(v >> (8 * i));
    return fwrite(b, 1, 8, f) == 8;
}

static int net_load_file_slot(omok_engine* e, int slot, const char* path) {
    if (!e || !path) return OMOK_ERR_INVALID;
    FILE* f = fopen(path, "rb");
    if (!f) return fail(e, OMOK_ERR_INVALID, "cannot open weights file %s", path);
    fseek(f, 0, SEEK_END);
    const long long fsize = ftell(f);
    fseek(f, 0, SEEK_SET);
    int rc = OMOK_OK;
    uint64_t n_names = 0, n_params = 0;
    std::vector<std::vector<float>> params(NET_TENSORS); // validated completely before the engine is touched
    if (!rd_u64(f, &n_names) || (long long)n_names > fsize / 8) rc = fail(e, OMOK_ERR_INVALID, "weights file %s: bad name count", path);
    for (uint64_t i = 0; rc == OMOK_OK && i < n_names; ++i) { // names are skipped: the load is positional (model_io.rs:98)
        uint64_t len = 0;
        if (!rd_u64(f, &len) || (long long)len > fsize || fseek(f, (long)len, SEEK_CUR) != 0) rc = fail(e, OMOK_ERR_INVALID, "weights file %s: truncated in variable_names", path);
    }
    if (rc == OMOK_OK && (!rd_u64(f, &n_params) || (long long)n_params > fsize / 8)) rc = fail(e, OMOK_ERR_INVALID, "weights file %s: bad parameter count", path);
    if (rc == OMOK_OK && n_params < (uint64_t)NET_TENSORS)
        rc = fail(e, OMOK_ERR_INVALID, "weights file %s holds %llu parameter vectors, the net has %d variables", path, (unsigned long long)n_params, NET_TENSORS);
    for (int i = 0; rc == OMOK_OK && i < NET_TENSORS; ++i) {
        uint64_t len = 0;
        if (!rd_u64(f, &len)) { rc = fail(e, OMOK_ERR_INVALID, "weights file %s: truncated at parameter %d", path, i); break; }
        if ((int64_t)len != e->net.wsize[i]) { // Tensor::copy_from_slice panics on a length mismatch (model_io.rs:106)
            rc = fail(e, OMOK_ERR_INVALID, "weights file %s: parameter %d has %llu values, variable has %lld", path, i, (unsigned long long)len, (long long)e->net.wsize[i]);
            break;
        }
        params[i].resize((size_t)len); // (host is little-endian like the file)
        if (fread(params[i].data(), sizeof(float), (size_t)len, f) != (size_t)len) { rc = fail(e, OMOK_ERR_INVALID, "weights file %s: truncated inside parameter %d", path, i); break; }
    }
    fclose(f);
    for (int i = 0; rc == OMOK_OK && i < NET_TENSORS; ++i) rc = net_load_slot(e, slot, i, params[i].data(), (int64_t)params[i].size());
    if (rc != OMOK_OK) return rc;
    return net_commit_slot(e, slot);
}
extern "C" int omok_net_load_file(omok_engine* e, const char* path) { return net_load_file_slot(e, 1, path); }
extern "C" int omok_net2_load_file(omok_engine* e, const char* path) { return net_load_file_slot(e, 2, path); }

extern "C" int omok_net_save_file(omok_engine* e, const char* path) {
    if (!e || !path) return OMOK_ERR_INVALID;
    for (int i = 0; i < NET_TENSORS; ++i)
        if (!e->net.loaded[i]) return fail(e, OMOK_ERR_STATE, "tensor %d was never loaded", i);
    HIPCHK(e, hipSetDevice(e->cfg.device));
    FILE* f = fopen(path, "wb");
    if (!f) return fail(e, OMOK_ERR_INVALID, "cannot create weights file %s", path);
    bool ok = wr_u64(f, NET_TENSORS);
    char name[64];
    for (int i = 0; ok && i < NET_TENSORS; ++i) {
        net_tensor_name(i, name, sizeof(name));
        const size_t len = strlen(name);
        ok = wr_u64(f, len) && fwrite(name, 1, len, f) == len;
    }
    ok = ok && wr_u64(f, NET_TENSORS);
    std::vector<float> buf;
    for (int i = 0; ok && i < NET_TENSORS; ++i) {
        const size_t len = (size_t)e->net.wsize[i];
        buf.resize(len);
        if (hipMemcpy(buf.data(), e->net.w[i], sizeof(float) * len, hipMemcpyDeviceToHost) != hipSuccess) { fclose(f); return fail(e, OMOK_ERR_HIP, "weight read-back failed"); }
        ok = wr_u64(f, len) && fwrite(buf.data(), sizeof(float), len, f) == len;
    }
    ok = (fclose(f) == 0) && ok;
    return ok ? OMOK_OK : fail(e, OMOK_ERR_INVALID, "short write to %s", path);
}

static int need_net(omok_engine* e) {
    if (!e->net.committed) return fail(e, OMOK_ERR_STATE, "net not loaded/committed (omok_net_load x31 + omok_net_commit)");
    if (e->match && !e->net2->committed) return fail(e, OMOK_ERR_STATE, "match episode: net 2 was reloaded and not committed (omok_net2_commit)");
    return 0;
}

// ---- match episodes: routing --------------------------------------------------------------------
// net index 0 = e->net (net 1), 1 = *e->net2.  A dense list of the trees of `tree_side` falls into block 0 (games < split: net tree_side) and
// block 1 (games >= split: the other net), see launch_match_split.
static Net& net_at(omok_engine* e, int idx) { return idx == 0 ? e->net : *e->net2; }
static void invalidate_nets(omok_engine* e) { // the trees changed outside the search rounds: both nets' cached base evaluations are void
    net_invalidate_sibling_cache(e->net);
    if (e->net2) net_invalidate_sibling_cache(*e->net2);
}
static bool block_live(const omok_engine* e, int b) { return b == 0 ? e->split > 0 : e->split < e->cfg.games; } // (false: the block has no game)
static Store block_view(const omok_engine* e, int b) { // the block's rows as a dense list of its own
    Store V = e->S;
    if (b == 0) V.d_count = e->d_mcnt;
    else { V.req_ref = e->d_mref; V.req_aux = e->d_maux; V.d_count = e->d_mcnt + 1; }
    return V;
}
// The evaluation blocks of a batch on the trees of `tree_side`: the rows one net evaluates, as a request list of their own.  Self-play has one, net 1 on
// the whole list; a match the live ones of its two.  rows: the block's row count, or the bound the caller has for it (run loops: the count stays on the
// device); pending: a match takes the counts of the pending step-wise batch (match_counts) instead.
struct Block { Net* net; Store view; int rows, off, b; }; // off: the block's first row in the order of the whole list (pending batches)
static int eval_blocks(omok_engine* e, int tree_side, int rows, bool pending, Block out[2]) {
    if (!e->match) { out[0] = Block{&e->net, e->S, rows, 0, 0}; return 1; }
    int n = 0;
    for (int b = 0; b < 2; ++b)
        if (block_live(e, b)) out[n++] = Block{&net_at(e, tree_side ^ b), block_view(e, b), pending ? e->match_cnt[b] : rows, b ? e->match_cnt[0] : 0, b};
    return n;
}
// one forward of a block's rows by its net (search rounds: sibling_side = the trees' side; a match block's k_group takes the block's games only)
static void block_forward(omok_engine* e, const Block& B, int max_count, int sibling_side = -1, bool skip_softmax = false, bool rows_to_nodes = false) {
    Net& X = *B.net;
    if (e->match) {
        X.grp_lo = B.b ? e->split : 0;
        X.grp_hi = B.b ? e->cfg.games : e->split;
        X.grp_sub = B.b ? e->d_mcnt : nullptr;
    }
    net_forward_requests(X, B.view, max_count, e->st, &e->prof, sibling_side, skip_softmax, rows_to_nodes);
    if (e->match) {
        X.grp_hi = -1;
        X.grp_sub = nullptr;
    }
}
static void match_split(omok_engine* e, int tree_side, int max_rows) {
    launch_match_split(e->S, tree_side, e->split, e->d_mref, e->d_maux, e->d_mcnt, e->d_mevals, max_rows, e->st);
}
// block 1's v (and p) behind block 0's, in the first block's net: one array in list order for k_scatter / k_round / k_advance
static void match_join(omok_engine* e, int tree_side, bool p, int max_rows) {
    if (!block_live(e, 1)) return;
    Net &A = net_at(e, tree_side), &B = net_at(e, tree_side ^ 1);
    launch_match_join(e->d_mcnt, B.v, A.v, p ? B.p : nullptr, p ? A.p : nullptr, e->rowp, max_rows, e->st);
}
static int match_counts(omok_engine* e) { // the pending batch's block sizes -> host
    HIPCHK(e, hipMemcpyAsync(e->match_cnt, e->d_mcnt, sizeof(e->match_cnt), hipMemcpyDeviceToHost, e->st));
    return sync_and_check(e, "match counts") ? OMOK_ERR_HIP : 0;
}
static int no_match(omok_engine* e, const char* what) {
    if (e->match) return fail(e, OMOK_ERR_STATE, "%s is not available in a match episode (omok_match_reset): start self-play with omok_selfplay_reset", what);
    return 0;
}

static int check_async(omok_engine* e, const char* what) {
    hipError_t r = hipGetLastError();
    if (r != hipSuccess) return fail(e, OMOK_ERR_HIP, "%s: launch failed: %s", what, hipGetErrorString(r));
    return 0;
}

static int sync_and_check(omok_engine* e, const char* what) {
    hipError_t r = hipStreamSynchronize(e->st);
    if (r != hipSuccess) return fail(e, OMOK_ERR_HIP, "%s: %s", what, hipGetErrorString(r));
    return check_async(e, what);
}

// ---- native training step: AgentModel::train (alpha-zero/src/agent_model.rs:136-168), Trainer::train's update loop (src/trainer.rs:329-357) ----
extern "C" int omok_net_read(omok_engine* e, int32_t index, float* out, int64_t count) {
    if (!e || !out) return OMOK_ERR_INVALID;
    if (index < 0 || index >= NET_TENSORS) return fail(e, OMOK_ERR_INVALID, "tensor index %d out of range", index);
    if (count != e->net.wsize[index]) return fail(e, OMOK_ERR_INVALID, "tensor %d: expected %lld values, got %lld", index, (long long)e->net.wsize[index], (long long)count);
    if (!e->net.loaded[index]) return fail(e, OMOK_ERR_STATE, "tensor %d was never loaded", index);
    ENTER(e);
    if (sync_and_check(e, "net_read")) return OMOK_ERR_HIP;
    HIPCHK(e, hipMemcpy(out, e->net.w[index], sizeof(float) * (size_t)count, hipMemcpyDeviceToHost));
    return OMOK_OK;
}

extern "C" int omok_train_end(omok_engine* e) {
    ENTER(e);
    if (!e->train) return OMOK_OK;
    if (sync_and_check(e, "train_end")) return OMOK_ERR_HIP;
    train_free(*e->train);
    delete e->train;
    e->train = nullptr;
    return OMOK_OK;
}

extern "C" int omok_train_begin(omok_engine* e, int32_t max_batch) {
    if (!e) return OMOK_ERR_INVALID;
    if (max_batch < 1 || max_batch > TRAIN_MAX_BATCH) return fail(e, OMOK_ERR_INVALID, "max_batch %d outside [1, %d]", max_batch, TRAIN_MAX_BATCH);
    for (int i = 0; i < NET_TENSORS; ++i)
        if (!e->net.loaded[i]) return fail(e, OMOK_ERR_STATE, "tensor %d was never loaded", i);
    if (omok_train_end(e)) return OMOK_ERR_HIP; // (a second call starts a fresh optimizer)
    Train* t = new Train();
    if (train_alloc(*t, e->net, max_batch) == 0) { delete t; return fail(e, OMOK_ERR_HIP, "training buffers for batches of %d: allocation failed (hipMalloc)", max_batch); }
    e->train = t;
    return OMOK_OK;
}

// the checks the step entry points share
static int train_check(omok_engine* e, const void* records_dev, int64_t n_records, int32_t batch) {
    if (!e->train) return fail(e, OMOK_ERR_STATE, "no training state (omok_train_begin)");
    for (int i = 0; i < NET_TENSORS; ++i)
        if (!e->net.loaded[i]) return fail(e, OMOK_ERR_STATE, "tensor %d was never loaded", i);
    if (!records_dev || ((uintptr_t)records_dev & 3)) return fail(e, OMOK_ERR_INVALID, "records_dev must be a 4-byte aligned device pointer");
    if (n_records < 1 || n_records > 0x7fffffffLL) return fail(e, OMOK_ERR_INVALID, "n_records %lld outside [1, 2^31)", (long long)n_records);
    if (batch < 1 || batch > e->train->max_b) return fail(e, OMOK_ERR_INVALID, "batch %d outside [1, max_batch = %d]", batch, e->train->max_b);
    return 0;
}

static int train_fetch_losses(omok_engine* e, int first, int steps, float losses[3], const char* what) { // the sums of `steps` steps -> their means
    float h[3];
    HIPCHK(e, hipMemcpyAsync(h, e->train->losses + first, sizeof(h), hipMemcpyDeviceToHost, e->st));
    if (sync_and_check(e, what)) return OMOK_ERR_HIP;
    if (losses)
        for (int i = 0; i < 3; ++i) losses[i] = h[i] / (float)steps;
    return 0;
}

static int train_once(omok_engine* e, const void* records_dev, int64_t n_records, const int64_t* indices, int32_t batch, float losses[3], bool update) {
    if (!e || !indices) return OMOK_ERR_INVALID;
    if (int rc = train_check(e, records_dev, n_records, batch)) return rc;
    for (int i = 0; i < batch; ++i)
        if (indices[i] < 0 || indices[i] >= n_records) return fail(e, OMOK_ERR_INVALID, "indices[%d] = %lld outside [0, %lld)", i, (long long)indices[i], (long long)n_records);
    ENTER(e);
    Train& T = *e->train;
    T.pending = 0; // (the batch buffers of a pending omok_train_backward are overwritten)
    HIPCHK(e, hipMemcpyAsync(T.idx, indices, sizeof(int64_t) * (size_t)batch, hipMemcpyHostToDevice, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st)); // (the caller's array may go away)
    if (update) e->net.committed = false;   // like omok_net_load: the packed operands no longer match Net::w[]
    train_step(T, e->net, records_dev, batch, update, false, e->st);
    return train_fetch_losses(e, 0, 1, losses, update ? "train_step" : "train_losses");
}

extern "C" int omok_train_step(omok_engine* e, const void* records_dev, int64_t n_records, const int64_t* indices, int32_t batch, float* losses) {
    return train_once(e, records_dev, n_records, indices, batch, losses, true);
}
extern "C" int omok_train_losses(omok_engine* e, const void* records_dev, int64_t n_records, const int64_t* indices, int32_t batch, float* losses) {
    return train_once(e, records_dev, n_records, indices, batch, losses, false);
}

extern "C" int omok_train_batch_indices(omok_engine* e, int64_t n_records, int32_t batch, uint64_t key, int32_t step, int64_t* out) {
    if (!e || !out) return OMOK_ERR_INVALID;
    if (!e->train) return fail(e, OMOK_ERR_STATE, "no training state (omok_train_begin)");
    if (n_records < 1 || n_records > 0x7fffffffLL) return fail(e, OMOK_ERR_INVALID, "n_records %lld outside [1, 2^31)", (long long)n_records);
    if (batch < 1 || batch > e->train->max_b) return fail(e, OMOK_ERR_INVALID, "batch %d outside [1, max_batch = %d]", batch, e->train->max_b);
    if (step < 0) return fail(e, OMOK_ERR_INVALID, "step %d is negative", step);
    ENTER(e);
    const int k = (int)std::min<int64_t>(batch, n_records);
    train_draw(*e->train, n_records, k, key, step, e->st);
    HIPCHK(e, hipMemcpyAsync(out, e->train->idx, sizeof(int64_t) * (size_t)k, hipMemcpyDeviceToHost, e->st));
    if (sync_and_check(e, "train_batch_indices")) return OMOK_ERR_HIP;
    return k;
}

extern "C" int omok_train_run(omok_engine* e, const void* records_dev, int64_t n_records, int32_t update_count, int32_t batch_size, uint64_t key, float* losses) {
    if (!e) return OMOK_ERR_INVALID;
    if (int rc = train_check(e, records_dev, n_records, batch_size)) return rc;
    if (update_count < 0) return fail(e, OMOK_ERR_INVALID, "update_count %d is negative", update_count);
    if (e->round_reqs >= 0 || e->mirror_reqs >= 0) return fail(e, OMOK_ERR_STATE, "omok_train_run while a round / mirror batch is pending (it commits the net)");
    ENTER(e);
    Train& T = *e->train;
    T.pending = 0;
    const int k = (int)std::min<int64_t>(batch_size, n_records), counted = std::min(update_count, 100); // trainer.rs:354-362: the log line averages the last 100 steps
    HIPCHK(e, hipMemsetAsync(T.losses, 0, sizeof(float) * 8, e->st));
    if (update_count > 0) e->net.committed = false;
    for (int s = 0; s < update_count; ++s) { // no host synchronisation between the steps: the draw, the step and the running sums stay on the device
        train_draw(T, n_records, k, key, s, e->st);
        train_step(T, e->net, records_dev, k, true, s >= update_count - counted, e->st);
    }
    if (int rc = train_fetch_losses(e, 4, std::max(counted, 1), losses, "train_run")) return rc;
    return net_commit_slot(e, 1);
}

// ---- the step in two halves: a data-parallel host moves the gradient slabs between them (trainer.rs:329-357 on several ranks) ----
extern "C" int64_t omok_train_gradient_count(const omok_engine* e) {
    if (!e) return OMOK_ERR_INVALID;
    int64_t count = 0;
    for (int i = 0; i < NET_TENSORS; ++i) count += e->net.wsize[i];
    return count;
}

extern "C" int omok_train_backward(omok_engine* e, const void* records_dev, int64_t n_records, const int64_t* indices, int32_t batch, void* grad_dst_dev) {
    if (!e || !indices) return OMOK_ERR_INVALID;
    if (int rc = train_check(e, records_dev, n_records, batch)) return rc;
    for (int i = 0; i < batch; ++i)
        if (indices[i] < 0 || indices[i] >= n_records) return fail(e, OMOK_ERR_INVALID, "indices[%d] = %lld outside [0, %lld)", i, (long long)indices[i], (long long)n_records);
    if ((uintptr_t)grad_dst_dev & 3) return fail(e, OMOK_ERR_INVALID, "grad_dst_dev must be a 4-byte aligned device pointer (or NULL)");
    ENTER(e);
    Train& T = *e->train;
    T.pending = 0;
    HIPCHK(e, hipMemcpyAsync(T.idx, indices, sizeof(int64_t) * (size_t)batch, hipMemcpyHostToDevice, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st)); // (the caller's array may go away)
    train_backward(T, e->net, records_dev, batch, e->st);
    if (grad_dst_dev) HIPCHK(e, hipMemcpyAsync(grad_dst_dev, T.grad, sizeof(float) * (size_t)T.off[NET_TENSORS], hipMemcpyDeviceToDevice, e->st));
    if (sync_and_check(e, "train_backward")) return OMOK_ERR_HIP; // the slab is complete on return: the caller's collective may run on any stream
    T.pending = batch;
    return OMOK_OK;
}

extern "C" int omok_train_apply(omok_engine* e, const void* grads_dev, int32_t ranks, float* losses) {
    if (!e) return OMOK_ERR_INVALID;
    if (!e->train) return fail(e, OMOK_ERR_STATE, "no training state (omok_train_begin)");
    if (e->train->pending < 1) return fail(e, OMOK_ERR_STATE, "no pending gradients (omok_train_backward, with no other omok_train_* call since)");
    if (ranks < 1 || ranks > OMOK_TRAIN_MAX_RANKS) return fail(e, OMOK_ERR_INVALID, "ranks %d outside [1, %d]", ranks, OMOK_TRAIN_MAX_RANKS);
    if (!grads_dev && ranks != 1) return fail(e, OMOK_ERR_INVALID, "grads_dev is NULL: the engine's own gradient is one rank's, not %d", ranks);
    if ((uintptr_t)grads_dev & 3) return fail(e, OMOK_ERR_INVALID, "grads_dev must be a 4-byte aligned device pointer (or NULL)");
    for (int i = 0; i < NET_TENSORS; ++i)
        if (!e->net.loaded[i]) return fail(e, OMOK_ERR_STATE, "tensor %d was never loaded", i);
    ENTER(e);
    Train& T = *e->train;
    const int k = T.pending;
    T.pending = 0;
    e->net.committed = false; // like omok_train_step
    e->prof.begin(PC_TRAIN_APPLY, e->st);
    train_update(T, e->net, (const float*)grads_dev, ranks, e->st);
    e->prof.end(e->st);
    train_evaluate(T, e->net, k, false, e->st);
    return train_fetch_losses(e, 0, 1, losses, "train_apply");
}

extern "C" int omok_debug_train_gradient(omok_engine* e, int32_t index, float* out, int64_t count) {
    if (!e || !out) return OMOK_ERR_INVALID;
    if (!e->train || !e->train->has_grad) return fail(e, OMOK_ERR_STATE, "no gradient yet (omok_train_begin + omok_train_step)");
    if (index < 0 || index >= NET_TENSORS) return fail(e, OMOK_ERR_INVALID, "tensor index %d out of range", index);
    if (count != e->net.wsize[index]) return fail(e, OMOK_ERR_INVALID, "tensor %d: expected %lld values, got %lld", index, (long long)e->net.wsize[index], (long long)count);
    ENTER(e);
    if (sync_and_check(e, "train_gradient")) return OMOK_ERR_HIP;
    HIPCHK(e, hipMemcpy(out, e->train->grad + e->train->off[index], sizeof(float) * (size_t)count, hipMemcpyDeviceToHost));
    return OMOK_OK;
}

// `rows` rows of src ([rows][stride]) as [rows][HW] into p, and as many values of vsrc into v (NULL: skipped), through net's staging buffer; no synchronisation
static int rows_to_host(omok_engine* e, Net& net, const float* src, int stride, const float* vsrc, int rows, float* p, float* v) {
    float* d_pack = net.in_f32; // (the forward is over: its input rows are free)
    const size_t tot = (size_t)rows * e->hw;
    k_pack_rows<<<(unsigned)((tot + 255) / 256), 256, 0, e->st>>>(src, d_pack, e->hw, stride, rows);
    HIPCHK(e, hipMemcpyAsync(p, d_pack, sizeof(float) * tot, hipMemcpyDeviceToHost, e->st));
    if (v) HIPCHK(e, hipMemcpyAsync(v, vsrc, sizeof(float) * rows, hipMemcpyDeviceToHost, e->st));
    return 0;
}

// omok_evaluate_pv, and with `logits` the debug / evidence entry point omok_evaluate_logits: the same forward, but the PRE-softmax policy logits and
// the PRE-tanh value (network.rs:188-247 before the Tanh / Softmax ops), so that precision can be stated on logits as well as on the outputs the
// reference API returns
static int evaluate_inputs(omok_engine* e, bool logits, const float* in, int32_t batch, float* p, float* v) {
    if (!e || !in || !p || batch < 0) return OMOK_ERR_INVALID;
    if (need_net(e)) return OMOK_ERR_STATE;
    if (e->round_reqs >= 0 || e->mirror_reqs >= 0) // the forward reuses the request counter and the output rows of the pending batch
        return fail(e, OMOK_ERR_STATE, logits ? "omok_evaluate_logits while a round / mirror batch is pending"
                                              : "omok_evaluate_pv between omok_round_generate / omok_mirror_generate and their scatter / apply");
    HIPCHK(e, hipSetDevice(e->cfg.device));
    Net& net = e->net;
    const size_t in_row = 3 * (size_t)e->hw;
    const int piece = logits && net.mode == OMOK_NET_F32 ? std::min(net.chunk, net.max_b) : net.max_b; // (OMOK_NET_F32 keeps the logits of its last chunk only)
    for (int32_t done = 0; done < batch; done += piece) {
        const int b = std::min<int32_t>(piece, batch - done);
        HIPCHK(e, hipMemcpyAsync(net.in_f32, in + (size_t)done * in_row, sizeof(float) * in_row * b, hipMemcpyHostToDevice, e->st));
        HIPCHK(e, hipMemcpyAsync(e->S.d_count, &b, sizeof(int32_t), hipMemcpyHostToDevice, e->st));
        net_forward_inputs(net, e->S, b, e->st, &e->prof);
        int stride = e->rowp;
        const float* src = logits ? net_logits(net, &stride) : net.p;
        if (rows_to_host(e, net, src, stride, logits ? net.vpre : net.v, b, p + (size_t)done * e->hw, v ? v + done : nullptr)) return OMOK_ERR_HIP;
        if (sync_and_check(e, logits ? "evaluate_logits" : "evaluate_pv")) return OMOK_ERR_HIP;
        e->evals += b;
    }
    return OMOK_OK;
}
extern "C" int omok_evaluate_pv(omok_engine* e, const float* in, int32_t batch, float* p, float* v) { return evaluate_inputs(e, false, in, batch, p, v); }
extern "C" int omok_evaluate_logits(omok_engine* e, const float* in, int32_t batch, float* logits, float* vpre) { return evaluate_inputs(e, true, in, batch, logits, vpre); }

// ---- environment -------------------------------------------------------------------------------
// Caller-held positions onto the device, in the caller's scratch: boards [B][HW] and, where given, turns [B], and a slab of out_words 4-byte words for
// the call's results.  check_turns: the side to move decides the answer, so a turns byte above 1 is refused before anything is allocated or launched.
struct DevPositions { uint8_t *boards, *turns; int32_t* out; };
static int upload_positions(omok_engine* e, Scratch& sc, const char* what, const uint8_t* boards, const uint8_t* turns, int32_t batch, bool check_turns,
                            size_t out_words, DevPositions& d) {
    const size_t B = (size_t)batch;
    for (size_t b = 0; check_turns && b < B; ++b)
        if (turns[b] > 1) return fail(e, OMOK_ERR_INVALID, "%s: turns[%zu] = %d is neither 0 (Black) nor 1 (White)", what, b, (int)turns[b]);
    d.boards = sc.get<uint8_t>(B * e->hw);
    d.turns = turns ? sc.get<uint8_t>(B) : nullptr;
    d.out = sc.get<int32_t>(out_words);
    if (sc.failed) return fail(e, OMOK_ERR_HIP, "%s: device allocation failed", what);
    hipMemcpyAsync(d.boards, boards, B * e->hw, hipMemcpyHostToDevice, e->st);
    if (turns) hipMemcpyAsync(d.turns, turns, B, hipMemcpyHostToDevice, e->st);
    return OMOK_OK;
}
// columns i = 0 .. k - 1 of a device slab [k][B] of int32 -> host[i], where that is not NULL
static void download_columns(omok_engine* e, const int32_t* d_slab, size_t B, int k, int32_t* const* host) {
    for (int i = 0; i < k; ++i)
        if (host[i]) hipMemcpyAsync(host[i], d_slab + i * B, B * 4, hipMemcpyDeviceToHost, e->st);
}
// its row-shaped sibling: `count` elements of a device array [B][k] as they lie -> host, where that is not NULL
template <typename T>
static void download_rows(omok_engine* e, const T* d_rows, size_t count, T* host) {
    if (host) hipMemcpyAsync(host, d_rows, count * sizeof(T), hipMemcpyDeviceToHost, e->st);
}

extern "C" int omok_env_play(omok_engine* e, const int32_t* moves, int32_t batch, int32_t len, int32_t* status_out,
                             uint8_t* boards_out, uint8_t* turns_out, uint16_t* legal_out) {
    if (!e || batch < 1 || len < 0 || (len > 0 && !moves)) return OMOK_ERR_INVALID;
    HIPCHK(e, hipSetDevice(e->cfg.device));
    const size_t ml = (size_t)batch * (size_t)(len > 0 ? len : 1);
    Scratch sc;
    int32_t *d_moves = sc.get<int32_t>(ml), *d_status = sc.get<int32_t>(ml);
    uint8_t *d_boards = sc.get<uint8_t>((size_t)batch * e->hw), *d_turns = sc.get<uint8_t>((size_t)batch);
    uint16_t* d_legal = sc.get<uint16_t>((size_t)batch);
    if (sc.failed) return fail(e, OMOK_ERR_HIP, "env_play: device allocation failed");
    if (len > 0) hipMemcpyAsync(d_moves, moves, ml * 4, hipMemcpyHostToDevice, e->st);
    launch_env_play(e->n, d_moves, batch, len, d_status, d_boards, d_turns, d_legal, e->st);
    if (status_out && len > 0) hipMemcpyAsync(status_out, d_status, ml * 4, hipMemcpyDeviceToHost, e->st);
    if (boards_out) hipMemcpyAsync(boards_out, d_boards, (size_t)batch * e->hw, hipMemcpyDeviceToHost, e->st);
    if (turns_out) hipMemcpyAsync(turns_out, d_turns, (size_t)batch, hipMemcpyDeviceToHost, e->st);
    if (legal_out) hipMemcpyAsync(legal_out, d_legal, (size_t)batch * 2, hipMemcpyDeviceToHost, e->st);
    return sync_and_check(e, "env_play") ? OMOK_ERR_HIP : OMOK_OK;
}

extern "C" int omok_encode_nn_input(omok_engine* e, const uint8_t* boards, const uint8_t* turns, int32_t batch,
                                    int32_t mode, float* out) {
    if (!e || !boards || !turns || !out || batch < 1 || (mode != 0 && mode != 1)) return OMOK_ERR_INVALID;
    HIPCHK(e, hipSetDevice(e->cfg.device));
    Scratch sc;
    DevPositions d;
    const size_t words = (size_t)batch * 3 * e->hw; // (float planes in the 4-byte slab)
    if (const int rc = upload_positions(e, sc, "encode_nn_input", boards, turns, batch, false, words, d)) return rc;
    launch_encode_boards(e->n, d.boards, d.turns, batch, mode, (float*)d.out, e->st);
    hipMemcpyAsync(out, d.out, words * 4, hipMemcpyDeviceToHost, e->st);
    return sync_and_check(e, "encode_nn_input") ? OMOK_ERR_HIP : OMOK_OK;
}

// ---- self-play ---------------------------------------------------------------------------------
static int read_status(omok_engine* e, uint32_t* err_bits, uint32_t* alive) {
    k_count_alive<<<1, 1024, 0, e->st>>>(e->S, e->d_error, e->d_evals);
    uint32_t h[4] = {0, 0, 0, 0};
    HIPCHK(e, hipMemcpyAsync(h, e->d_error, 16, hipMemcpyDeviceToHost, e->st));
    if (sync_and_check(e, "status readback")) return OMOK_ERR_HIP;
    if (err_bits) *err_bits = h[0];
    if (alive) *alive = h[1];
    if (h[2] > e->peak_nodes) e->peak_nodes = h[2];
    if (h[3] > e->peak_tables) e->peak_tables = h[3];
    return 0;
}

static int tree_error(omok_engine* e, uint32_t bits) {
    if (bits & 1u) return fail(e, OMOK_ERR_OVERFLOW, "a tree arena overflowed (max_nodes=%d, max_tables=%d; peak use %u nodes, %u tables): raise them", e->cfg.max_nodes, e->cfg.max_tables, e->peak_nodes, e->peak_tables);
    if (bits & 4u) return fail(e, OMOK_ERR_ILLEGAL, "sample_action on a tree with no visited children (run execute first)");
    if (bits) return fail(e, OMOK_ERR_ILLEGAL, "illegal tree operation (error bits 0x%x)", bits);
    return 0;
}

// Agent::new: evaluate_p on the empty board in Player mode (agent.rs:19-20); the result is the same for every tree of a fixed net, so it is
// computed once per net
static int enqueue_root_policy(omok_engine* e, Net& net, float* dst) {
    std::vector<float> in(3 * (size_t)e->hw, 0.0f);
    for (int i = 2 * e->hw; i < 3 * e->hw; ++i) in[i] = 1.0f; // Black to move (encoder.rs:34-37)
    const int one = 1;
    HIPCHK(e, hipMemcpyAsync(net.in_f32, in.data(), sizeof(float) * in.size(), hipMemcpyHostToDevice, e->st));
    HIPCHK(e, hipMemcpyAsync(e->S.d_count, &one, sizeof(int32_t), hipMemcpyHostToDevice, e->st));
    net_forward_inputs(net, e->S, 1, e->st, &e->prof);
    k_copy_root_policy<<<1, 256, 0, e->st>>>(net.p, dst, e->hw, e->rowp);
    HIPCHK(e, hipStreamSynchronize(e->st)); // (the host input buffer goes out of scope)
    e->evals += 1;
    return 0;
}

// what the four reset entry points ask of the nets: net 1 committed; a match: net 2 too, and the split in range
static int check_reset(omok_engine* e, bool match, int split) {
    if (!e->net.committed) return fail(e, OMOK_ERR_STATE, "net not loaded/committed (omok_net_load x31 + omok_net_commit)");
    if (!match) return 0;
    if (!e->net2 || !e->net2->committed) return fail(e, OMOK_ERR_STATE, "net 2 not loaded/committed (omok_net2_load x31 + omok_net2_commit)");
    if (split < 0 || split > e->cfg.games) return fail(e, OMOK_ERR_INVALID, "split %d outside [0, games = %d]", split, e->cfg.games);
    return 0;
}

// the host's bookkeeping of a successful reset; start_ply: the stone count of the positions (a game's ply is its stone count: side = ply & 1, the RNG counters)
static void begin_episode(omok_engine* e, bool match, int split, int start_ply) {
    e->key = e->cfg.seed + e->episode * 0x9E3779B97F4A7C15ULL; // a fresh RNG stream per episode (the reference draws thread_rng anew, trainer.rs:71-93)
    e->episode += 1;                                           // (every reset is one trainer iteration)
    e->ply = e->start_ply = start_ply;
    e->log_started = e->log_on;
    e->reset_done = true;
    e->sampled = false;
    e->round_reqs = e->mirror_reqs = -1;
    e->match = match;
    e->split = match ? split : 0;
}

static int reset_episode(omok_engine* e, bool match, int split) {
    if (enqueue_root_policy(e, e->net, e->d_root_policy)) return OMOK_ERR_HIP;
    if (match && enqueue_root_policy(e, *e->net2, e->d_root_policy2)) return OMOK_ERR_HIP;
    launch_reset(e->n, e->S, e->d_root_policy, e->st);
    if (match) launch_match_roots(e->n, e->S, e->d_root_policy2, split, e->st);
    if (e->log_on) hipMemsetAsync(e->log.start_board, 0, (size_t)e->cfg.games * e->hw, e->st); // the log starts at Environment::new()
    invalidate_nets(e);
    if (sync_and_check(e, match ? "match_reset" : "selfplay_reset")) return OMOK_ERR_HIP;
    begin_episode(e, match, split, 0);
    return OMOK_OK;
}

extern "C" int omok_selfplay_reset(omok_engine* e) {
    if (!e) return OMOK_ERR_INVALID;
    if (int rc = check_reset(e, false, 0)) return rc;
    HIPCHK(e, hipSetDevice(e->cfg.device));
    return reset_episode(e, false, 0);
}

// benchmark/src/main.rs:14-108: net 1 against net 2, Agent::new of each agent with its own model (agent.rs:16-35)
extern "C" int omok_match_reset(omok_engine* e, int32_t split) {
    if (!e) return OMOK_ERR_INVALID;
    if (int rc = check_reset(e, true, split)) return rc;
    HIPCHK(e, hipSetDevice(e->cfg.device));
    return reset_episode(e, true, split);
}

// ---- episodes from given positions ----------------------------------------------------------------
static const char* verdict_text(int v) {
    switch (v) {
    case 1: return "a byte that is not a Stone (> 2)";
    case 2: return "stone counts that no alternating game produces";
    case 3: return "the position is already won";
    case 4: return "no empty cell (Draw)";
    default: return "legal";
    }
}

// uploads `batch` boards into the caller's scratch and runs k_position_check on them; *d_boards_out (may be NULL) = the device copy
static int check_positions(omok_engine* e, Scratch& sc, const uint8_t* boards, int batch, int32_t* verdict_out, int32_t* stones_out, uint8_t** d_boards_out) {
    const size_t B = (size_t)batch;
    DevPositions d;
    if (const int rc = upload_positions(e, sc, "position check", boards, nullptr, batch, false, 2 * B, d)) return rc; // [2][B] verdicts, stone counts
    launch_position_check(e->n, d.boards, batch, d.out, d.out + B, e->st);
    int32_t* const host[2] = {verdict_out, stones_out};
    download_columns(e, d.out, B, 2, host);
    if (sync_and_check(e, "position check")) return OMOK_ERR_HIP;
    if (d_boards_out) *d_boards_out = d.boards;
    return OMOK_OK;
}

// the rules of Environment::place_stone (environment/src/lib.rs:104-166) read backwards: can an alternating game from Environment::new() be in
// this position, still in progress?
extern "C" int omok_env_check_positions(omok_engine* e, const uint8_t* boards, int32_t batch, int32_t* verdict_out, int32_t* stones_out) {
    if (!e || !boards || !verdict_out || batch < 1) return OMOK_ERR_INVALID;
    ENTER(e);
    Scratch sc;
    return check_positions(e, sc, boards, batch, verdict_out, stones_out, nullptr);
}

// Agent::new (agent.rs:16-35) for the agents of every game on a given environment: evaluate_p of the position in Player mode (:19-20), masked
// and renormalised over its stones like every policy the reference stores on a non-empty board (ensure_action_exists, :166-171).  The part
// omok_selfplay_reset_from and omok_match_reset_from share: check, upload, encode, one plain-row forward of the G positions per net, the root
// kernel and the bookkeeping.  match: tree side * G + g takes the row of net side ^ (g >= split).  The caller has checked the nets and split.
static int reset_from_positions(omok_engine* e, const uint8_t* boards, bool match, int split) {
    const char* what = match ? "match_reset_from" : "selfplay_reset_from";
    const int G = e->cfg.games;
    std::vector<int32_t> verdict((size_t)G), stones((size_t)G);
    Scratch sc;
    uint8_t* d_boards = nullptr;
    if (check_positions(e, sc, boards, G, verdict.data(), stones.data(), &d_boards)) return OMOK_ERR_HIP;
    // nothing of the engine has been touched so far: a rejected call leaves trees, games, episode counter and replay buffer as they were
    for (int g = 0; g < G; ++g)
        if (verdict[g] != 0) return fail(e, OMOK_ERR_ILLEGAL, "game %d: verdict %d (%s)", g, verdict[g], verdict_text(verdict[g]));
    for (int g = 1; g < G; ++g)
        if (stones[g] != stones[0])
            return fail(e, OMOK_ERR_INVALID, "game %d has %d stones, game 0 has %d: all games of an episode share the side to move", g, stones[g], stones[0]);
    const int s0 = stones[0];
    if (s0 == 0) return reset_episode(e, match, split); // Environment::new() everywhere: the ordinary reset's own path (one empty-board row per net, nothing to mask)
    uint8_t* d_turns = sc.get<uint8_t>((size_t)G);
    if (!d_turns) return fail(e, OMOK_ERR_HIP, "%s: device allocation failed", what);
    // the G positions as plain rows in game order: the launch omok_evaluate_pv makes for the same rows (G <= the net batch); in a match every
    // game has one tree of each net, so each net evaluates all G rows
    hipMemsetAsync(d_turns, s0 & 1, (size_t)G, e->st);
    hipMemcpyAsync(e->S.d_count, &G, sizeof(int32_t), hipMemcpyHostToDevice, e->st);
    for (int i = 0; i < (match ? 2 : 1); ++i) {
        Net& X = net_at(e, i);
        e->prof.begin(PC_PLY, e->st);
        launch_encode_boards(e->n, d_boards, d_turns, G, OMOK_MODE_PLAYER, X.in_f32, e->st);
        e->prof.end(e->st);
        net_forward_inputs(X, e->S, G, e->st, &e->prof);
        if (match) k_add_evals<<<1, 64, 0, e->st>>>(e->S.d_count, e->d_mevals + i); // rows per net (omok_net2_info)
    }
    e->prof.begin(PC_PLY, e->st);
    launch_reset_from(e->n, e->S, d_boards, e->net.p, match ? e->net2->p : nullptr, split, e->st);
    e->prof.end(e->st);
    if (e->log_on) hipMemcpyAsync(e->log.start_board, d_boards, (size_t)G * e->hw, hipMemcpyDeviceToDevice, e->st); // the log starts at the given positions
    invalidate_nets(e);
    if (sync_and_check(e, what)) return OMOK_ERR_HIP;
    e->evals += match ? 2 * G : G;
    begin_episode(e, match, split, s0);
    return OMOK_OK;
}

extern "C" int omok_selfplay_reset_from(omok_engine* e, const uint8_t* boards) {
    if (!e || !boards) return OMOK_ERR_INVALID;
    if (int rc = check_reset(e, false, 0)) return rc;
    ENTER(e);
    return reset_from_positions(e, boards, false, 0);
}

// omok_match_reset on given environments: an opening book for benchmark/src/main.rs:14-108, Agent::new of every agent with its own net
extern "C" int omok_match_reset_from(omok_engine* e, int32_t split, const uint8_t* boards) {
    if (!e || !boards) return OMOK_ERR_INVALID;
    if (int rc = check_reset(e, true, split)) return rc;
    ENTER(e);
    return reset_from_positions(e, boards, true, split);
}

// Random openings: the board after `stones` plies of a game both of whose sides are the RANDOM scripted player (src/trainer.rs:452-455), on
// caller-held memory like omok_env_check_positions; ok = 0 where a placement ended the game (the board holds the stones up to that one)
extern "C" int omok_env_random_positions(omok_engine* e, uint64_t key, int64_t first_game, int32_t stones, int32_t batch, uint8_t* boards_out,
                                         uint8_t* ok_out) {
    if (!e || !boards_out || !ok_out) return OMOK_ERR_INVALID;
    if (stones < 0 || stones >= e->hw) return fail(e, OMOK_ERR_INVALID, "stones %d outside [0, %d)", stones, e->hw);
    if (batch < 1) return fail(e, OMOK_ERR_INVALID, "batch %d < 1", batch);
    ENTER(e);
    const size_t B = (size_t)batch;
    Scratch sc;
    uint8_t* d_out = sc.get<uint8_t>(B * e->hw + B); // [B][HW] boards, then [B] ok
    if (!d_out) return fail(e, OMOK_ERR_HIP, "env_random_positions: device allocation failed");
    e->prof.begin(PC_PLY, e->st); // (timed only under omok_set_profiling: tools/reset_from_timing.py)
    launch_random_positions(e->n, key, first_game, stones, batch, d_out, d_out + B * e->hw, e->st);
    e->prof.end(e->st);
    hipMemcpyAsync(boards_out, d_out, B * e->hw, hipMemcpyDeviceToHost, e->st);
    hipMemcpyAsync(ok_out, d_out + B * e->hw, B, hipMemcpyDeviceToHost, e->st);
    return sync_and_check(e, "env_random_positions") ? OMOK_ERR_HIP : OMOK_OK;
}

static int need_reset(omok_engine* e) {
    if (!e->reset_done) return fail(e, OMOK_ERR_STATE, "omok_selfplay_reset has not been called");
    return 0;
}

// the net whose v holds the backups' values of a round on `side` (match episodes: the first block's, after match_join)
static Net& backup_net(omok_engine* e, int side) { return e->match ? net_at(e, side) : e->net; }

// May this round of the run loop be a lazy one?  Non-match engines whose forward is a split-precision one that covers the batch and whose logits rows are
// as long as a policy row; the round's backups must be deferred ones (they mark the rows).  Returns the row bound of the round's forward, 0: an eager round.
static int lazy_round_rows(const omok_engine* e, int rows_cap) {
    if (!e->lazy_policy || e->match || !net_logits_cover_batch(e->net, rows_cap) || !net_rows_fit_policy(e->net)) return 0;
    return rows_cap;
}

// a block's forward and the scatter of its policies (backups_inline: the scatter kernel runs the round's backups too).  lazy: no scatter kernel at all -- the heads write
// the logits rows into the nodes' policy rows and v / vpre themselves; the deferred backups mark the rows raw (lazy_round_rows)
static void forward_and_scatter(omok_engine* e, const Block& B, int side, int rows_cap, bool backups_inline, bool lazy = false) {
    Net& X = *B.net;
    // the split-precision net hands over its logits: softmax / tanh run inside the policy scatter (no [requests][ROWP] round trip of p)
    const bool fused = net_logits_cover_batch(X, rows_cap);
    block_forward(e, B, rows_cap, side, fused, lazy);
    if (lazy) return;
    e->prof.begin(PC_TREE_OTHER, e->st);
    if (fused) {
        int lrow = 0;
        const float* lg = net_logits(X, &lrow);
        launch_softmax_scatter(e->n, B.view, side, lg, lrow, X.v, X.vpre, rows_cap, e->st, backups_inline);
    } else launch_scatter(e->n, B.view, side, X.p, X.v, rows_cap, e->st, backups_inline);
    e->prof.end(e->st);
}

// defer_backups (run loops): this round's backups are not launched here; pending_backups: the previous round's run at the head of this round's
// kernel.  The caller launches the last round's backups itself (launch_backups).
// A round of a match episode: the one request list in two blocks, one forward per net on its own block, the policies scattered block by block,
// then v of the second block joined behind the first's (in the first block's net, which the backups read).
// lazy (run loops, with defer_backups): this round leaves raw policy rows; pending_raw_rows: the round whose backups are pending did (its row bound).
static void enqueue_round(omok_engine* e, int round, int K, float eps, float alpha, bool eval_and_scatter, int alive, bool defer_backups = false,
                          bool pending_backups = false, bool lazy = false, int pending_raw_rows = 0) {
    const int side = e->ply & 1;
    // run-loop rounds whose forward groups the requests by parent (sib_round): no k_scan and no k_fill.  k_round zeroes the grouping counters and leaves every
    // game's request count; k_group derives the request offsets and the round's total from them and writes the dense request list.  The step-wise API and match
    // episodes keep the separate kernels (the step-wise callers read the request list before the forward).
    const int max_req = std::min(alive * K, e->net.max_b);
    const bool sib_round = !e->match && eval_and_scatter && net_round_takes_sibling_path(e->net, max_req);
    RoundArgs a{side, round, K, e->ply, eps, alpha, e->key, e->cfg.game_offset, pending_backups ? backup_net(e, side).v : nullptr,
                sib_round ? e->d_req_cnt : nullptr, sib_round ? e->net.d_gcnt : nullptr, sib_round ? NET_GCNT_INTS : 0,
                pending_backups ? pending_raw_rows : 0, e->d_lazy};
    e->prof.round_begin();
    e->prof.begin(PC_ROUND, e->st);
    launch_round(e->n, e->S, a, e->st);
    e->prof.end(e->st);
    e->prof.begin(PC_TREE_OTHER, e->st);
    if (!sib_round) launch_scan(e->n, e->S, side, K, e->st, e->d_evals);
    if (e->match) match_split(e, side, max_req);
    else { // the hand-over to the forward of net 1
        e->net.gcnt_zeroed = e->net.fill_in_group = sib_round;
        e->net.scan_cnt = sib_round ? e->d_req_cnt : nullptr;
        e->net.scan_evals = e->d_evals;
        e->net.fill_side = side;
        e->net.fill_k = K;
    }
    e->prof.end(e->st);
    if (eval_and_scatter) {
        Block blk[2];
        const int nb = eval_blocks(e, side, alive * K, false, blk);
        for (int i = 0; i < nb; ++i) forward_and_scatter(e, blk[i], side, alive * K, !e->match && !defer_backups, lazy);
        if (e->match) { // the blocks' scatters ran no backups: they read one v array in list order
            e->prof.begin(PC_TREE_OTHER, e->st);
            match_join(e, side, false, max_req);
            if (!defer_backups) launch_backups(e->n, e->S, side, net_at(e, side).v, e->st);
            e->prof.end(e->st);
        }
    }
    e->prof.round_end();
}

// run_loop: the caller is one of the whole-episode loops (play_ply), whose rounds may be lazy ones; omok_execute keeps the eager kernels
static int enqueue_execute(omok_engine* e, int count, int K, float eps, float alpha, int alive, bool run_loop = false) {
    int processed = 0, round = 0;
    const int raw_rows = run_loop ? lazy_round_rows(e, alive * K) : 0;
    while (processed < count) { // pme.rs:39-42,207
        enqueue_round(e, round, K, eps, alpha, true, alive, true, round > 0, raw_rows > 0, raw_rows);
        processed += K;
        round += 1;
    }
    if (round > 0) { // the last round's backups
        e->prof.begin(PC_TREE_OTHER, e->st);
        launch_backups(e->n, e->S, e->ply & 1, backup_net(e, e->ply & 1).v, e->st, raw_rows);
        e->prof.end(e->st);
    }
    return round;
}

static int check_exec_args(omok_engine* e, int count, int K, float eps, float alpha) {
    if (count < 1) return fail(e, OMOK_ERR_INVALID, "count must be >= 1");
    if (K < 1 || K > e->cfg.max_batch_k) return fail(e, OMOK_ERR_INVALID, "batch_size %d outside [1, max_batch_k=%d]", K, e->cfg.max_batch_k);
    if (!(alpha > 0.0f && alpha <= (float)OMOK_ALPHA_MAX)) return fail(e, OMOK_ERR_INVALID, "alpha must be in (0, %d]", OMOK_ALPHA_MAX);
    if (!(eps >= 0.0f && eps <= 1.0f)) return fail(e, OMOK_ERR_INVALID, "epsilon must be in [0,1]");
    return 0;
}

// Boltzmann(temperature) of omok_sample_actions: the heated weights exp(pi / T) and their fp32 sum must stay finite (omok_mi355x.h); NaN fails both
// comparisons, +inf passes (1 / T = 0: uniform over the visited cells, as in the reference)
static int check_temperature(omok_engine* e, float temperature) {
    if (!(temperature > 0.0f && 1.0f / temperature <= (float)OMOK_TEMPERATURE_INV_MAX))
        return fail(e, OMOK_ERR_INVALID, "temperature must be >= 1 / %d", OMOK_TEMPERATURE_INV_MAX);
    return 0;
}

// what every entry point that searches asks first: the nets, an episode, the search arguments (temperature: the sampling of the run loops)
static int check_search(omok_engine* e, int count, int K, float eps, float alpha, float temperature = 1.0f) {
    if (need_net(e) || need_reset(e)) return OMOK_ERR_STATE;
    if (check_exec_args(e, count, K, eps, alpha)) return OMOK_ERR_INVALID;
    return check_temperature(e, temperature);
}

extern "C" int omok_execute(omok_engine* e, int32_t count, int32_t batch_size, float epsilon, float alpha) {
    if (!e) return OMOK_ERR_INVALID;
    if (int rc = check_search(e, count, batch_size, epsilon, alpha)) return rc;
    HIPCHK(e, hipSetDevice(e->cfg.device));
    uint32_t bits = 0, alive = 0;
    if (read_status(e, &bits, &alive)) return OMOK_ERR_HIP;
    const int rounds = enqueue_execute(e, count, batch_size, epsilon, alpha, (int)alive);
    e->sims += (double)rounds * batch_size * alive;
    if (read_status(e, &bits, &alive)) return OMOK_ERR_HIP;
    return tree_error(e, bits);
}

// MCTSExecutor::run (alpha-zero/src/mcts_executor.rs:29-255): ONE tree, rounds as concurrent tasks.  `waves` rounds run at a time
// on the shared tree of game 0 (one workgroup of `waves` wavefronts); their requests form one net batch.
// With a RECORDED interleaving (rec, tests): every simulation and every backup of the scatter phase runs under the tree lock and the lock order is
// written down, group by group, together with the net outputs of the group's requests -- everything a CPU restatement of MCTSExecutor::run needs
// to replay the run exactly (tests/test_gpu_shared_tree.py).  Recording reads every group back: without it nothing here waits for the device.
struct SharedRecording {
    uint8_t *sim_order, *backup_order; // [groups][waves * batch_size] wave ids in lock order
    int32_t* group_counts;             // [groups][3] simulations, backups, requests
    float *p, *v;                      // [cap_requests][HW], [cap_requests]
    int32_t cap_requests, *n_groups, *n_requests;
};
static int execute_shared(omok_engine* e, const char* who, int count, int K, float epsilon, float alpha, int waves, const SharedRecording* rec) {
    if (int rc = check_search(e, count, K, epsilon, alpha)) return rc;
    if (no_match(e, who)) return OMOK_ERR_STATE;
    if (e->cfg.games != 1) return fail(e, OMOK_ERR_INVALID, "%s searches ONE tree: create the engine with games = 1 (got %d)", who, e->cfg.games);
    if (waves < 1 || waves > MAX_TREE_WAVES || waves * K > e->net.max_b) // (cfg.max_tree_waves sizes the net batch: it binds through max_b)
        return fail(e, OMOK_ERR_INVALID, "waves must be in [1, %d] and waves * batch_size <= %d (the net batch, sized by max(games, max_tree_waves = %d) * max_batch_k)",
                    MAX_TREE_WAVES, e->net.max_b, e->cfg.max_tree_waves);
    ENTER(e);
    const size_t per = (size_t)waves * K;
    Scratch sc;
    uint8_t* d_rec = rec ? sc.get<uint8_t>(2 * per) : nullptr;  // [2][per] wave ids: simulations, backups
    uint32_t* d_pos = rec ? sc.get<uint32_t>(2) : nullptr;      // [2]
    if (sc.failed) return fail(e, OMOK_ERR_HIP, "recorded mode: device allocation failed");
    std::vector<float> prow(rec ? per * e->rowp : 0);
    uint32_t bits = 0, alive = 0;
    if (read_status(e, &bits, &alive)) return OMOK_ERR_HIP;
    const int side = e->ply & 1;
    RoundArgs a{side, 0, 0, e->ply, epsilon, alpha, e->key, e->cfg.game_offset};
    launch_materialise(e->n, e->S, side * e->cfg.games, 1, e->st); // (k_round_shared has its own copy of the descent: it meets no raw row an earlier run loop left)
    e->prof.begin(PC_ROUND, e->st);
    launch_round(e->n, e->S, a, e->st); // K = 0, round 0: the root's Dirichlet noise only (mcts_executor.rs:38-68)
    e->prof.end(e->st);
    int exec_count = count / K; // :70-74
    if (exec_count * K != count) exec_count += 1;
    a.K = K;
    int group = 0, total_req = 0;
    for (; group * waves < exec_count; ++group) {
        if (rec) {
            hipMemsetAsync(d_rec, 0xFF, 2 * per, e->st);
            hipMemsetAsync(d_pos, 0, 8, e->st);
        }
        e->prof.begin(PC_ROUND, e->st);
        launch_round_shared(e->n, e->S, a, exec_count, group, waves, e->d_sh_req, e->d_sh_cnt, e->st, d_rec, d_pos);
        k_add_evals<<<1, 64, 0, e->st>>>(e->S.d_count, e->d_evals);
        e->prof.end(e->st);
        int32_t cnt = 0;
        if (rec) {
            if (hipMemcpyAsync(&cnt, e->S.d_count, 4, hipMemcpyDeviceToHost, e->st) != hipSuccess || sync_and_check(e, "execute_shared_recorded")) return OMOK_ERR_HIP;
            if (total_req + cnt > rec->cap_requests) return fail(e, OMOK_ERR_INVALID, "recorded mode: more than cap_requests = %d requests", rec->cap_requests);
        }
        if (!rec || cnt > 0) net_forward_requests(e->net, e->S, waves * K, e->st, &e->prof); // (recorded: a group without requests has no forward)
        if (cnt > 0) {
            hipMemcpyAsync(prow.data(), e->net.p, sizeof(float) * (size_t)cnt * e->rowp, hipMemcpyDeviceToHost, e->st);
            hipMemcpyAsync(rec->v + total_req, e->net.v, sizeof(float) * cnt, hipMemcpyDeviceToHost, e->st);
        }
        e->prof.begin(PC_TREE_OTHER, e->st);
        launch_scatter_shared(e->n, e->S, side, e->net.p, e->net.v, waves * K, waves, e->d_sh_req, e->d_sh_cnt, e->st, rec ? d_rec + per : nullptr, rec ? d_pos + 1 : nullptr);
        e->prof.end(e->st);
        if (!rec) continue;
        uint32_t pos[2] = {0, 0};
        hipMemcpyAsync(rec->sim_order + (size_t)group * per, d_rec, per, hipMemcpyDeviceToHost, e->st);
        hipMemcpyAsync(rec->backup_order + (size_t)group * per, d_rec + per, per, hipMemcpyDeviceToHost, e->st);
        hipMemcpyAsync(pos, d_pos, 8, hipMemcpyDeviceToHost, e->st);
        if (sync_and_check(e, "execute_shared_recorded")) return OMOK_ERR_HIP;
        for (int r = 0; r < cnt; ++r) memcpy(rec->p + (size_t)(total_req + r) * e->hw, prow.data() + (size_t)r * e->rowp, sizeof(float) * e->hw);
        rec->group_counts[3 * group] = (int32_t)pos[0];
        rec->group_counts[3 * group + 1] = (int32_t)pos[1];
        rec->group_counts[3 * group + 2] = cnt;
        total_req += cnt;
    }
    if (rec) {
        *rec->n_groups = group;
        *rec->n_requests = total_req;
    }
    e->sims += (double)exec_count * K * alive;
    if (read_status(e, &bits, &alive)) return OMOK_ERR_HIP;
    return tree_error(e, bits);
}

extern "C" int omok_execute_shared(omok_engine* e, int32_t count, int32_t batch_size, float epsilon, float alpha, int32_t waves) {
    if (!e) return OMOK_ERR_INVALID;
    return execute_shared(e, "omok_execute_shared", count, batch_size, epsilon, alpha, waves, nullptr);
}

extern "C" int omok_execute_shared_recorded(omok_engine* e, int32_t count, int32_t batch_size, float epsilon, float alpha, int32_t waves,
                                            uint8_t* sim_order, uint8_t* backup_order, int32_t* group_counts, float* p, float* v,
                                            int32_t cap_requests, int32_t* n_groups, int32_t* n_requests) {
    if (!e || !sim_order || !backup_order || !group_counts || !p || !v || !n_groups || !n_requests) return OMOK_ERR_INVALID;
    const SharedRecording rec{sim_order, backup_order, group_counts, p, v, cap_requests, n_groups, n_requests};
    return execute_shared(e, "omok_execute_shared_recorded", count, batch_size, epsilon, alpha, waves, &rec);
}

static void enqueue_sample(omok_engine* e, float temperature, int threshold) {
    e->prof.begin(PC_PLY, e->st);
    launch_sample(e->n, e->S, e->ply & 1, e->ply, temperature, threshold, e->key, e->cfg.game_offset, e->d_actions, e->st);
    e->prof.end(e->st);
}

// the scripted player's move of every live game (OMOK_OPP_*: the evaluation games further down), staged where the search's sample would be
// (OMOK_OPP_GUARD: three launches under the one event pair, on the scratch the caller made sure of with ensure_guard_scratch)
static void enqueue_opponent_move(omok_engine* e, int kind) {
    e->prof.begin(PC_PLY, e->st);
    launch_opponent_move(e->n, e->S, e->ply & 1, kind, e->key, e->cfg.game_offset, OMOK_VCF_OPP_DEPTH, OMOK_VCF_OPP_NODES, e->d_actions, e->st,
                         e->d_guard_out, e->d_guard_status);
    e->prof.end(e->st);
}

extern "C" int omok_sample_actions(omok_engine* e, float temperature, int32_t threshold, int32_t* actions) {
    if (!e) return OMOK_ERR_INVALID;
    if (need_reset(e)) return OMOK_ERR_STATE;
    if (check_temperature(e, temperature)) return OMOK_ERR_INVALID;
    HIPCHK(e, hipSetDevice(e->cfg.device));
    enqueue_sample(e, temperature, threshold);
    if (actions) HIPCHK(e, hipMemcpyAsync(actions, e->d_actions, sizeof(int32_t) * e->cfg.games, hipMemcpyDeviceToHost, e->st));
    uint32_t bits = 0;
    if (read_status(e, &bits, nullptr)) return OMOK_ERR_HIP;
    e->sampled = true;
    return tree_error(e, bits);
}

// the move log's entry of this ply, directly in front of the re-rooting (k_advance) that forgets what the search knew of the move; nothing
// is launched while the log is off
static void enqueue_log_move(omok_engine* e, int side) {
    if (e->log_on && e->log_started) launch_log_move(e->n, e->S, side, e->start_ply, e->log, e->st);
}

// the re-rooting of a ply whose mirror batch (at most max_rows rows) has been evaluated: the policies of the opponent's new roots in one array (a match: the
// second block's behind the first's), the move log's entry, k_advance
// raw (lazy plies of the run loops): the mirror forward stopped behind the heads; a node k_advance creates takes its LOGITS row as a raw policy row
static void enqueue_advance(omok_engine* e, int max_rows, bool raw = false) {
    const int side = e->ply & 1;
    if (e->match) match_join(e, 1 - side, true, max_rows);
    enqueue_log_move(e, side);
    int lrow = 0;
    launch_advance(e->n, e->S, side, raw ? net_logits(e->net, &lrow) : backup_net(e, 1 - side).p, e->st, raw);
    invalidate_nets(e);
}

// run_loop: one of the whole-episode loops (play_ply); its mirror evaluation may stay logits (lazy_round_rows: the row of a new root is read by its noise)
static void enqueue_mirror_and_advance(omok_engine* e, int alive, bool run_loop = false) {
    const bool raw = run_loop && lazy_round_rows(e, alive) > 0;
    const int side = e->ply & 1;
    e->prof.begin(PC_PLY, e->st);
    launch_mirror_scan(e->n, e->S, side, e->st);
    k_add_evals<<<1, 64, 0, e->st>>>(e->S.d_count, e->d_evals);
    if (e->match) match_split(e, 1 - side, alive); // ensure_action_exists on the opponent's tree: the opponent's net (benchmark/src/main.rs:79-82,99-102)
    e->prof.end(e->st);
    Block blk[2];
    const int nb = eval_blocks(e, 1 - side, alive, false, blk);
    for (int i = 0; i < nb; ++i) block_forward(e, blk[i], alive, -1, raw);
    e->prof.begin(PC_PLY, e->st);
    enqueue_advance(e, alive, raw);
    e->prof.end(e->st);
}

// ---- the ply driver: what the whole-episode calls and the step-wise ones share --------------------------------------------------------------
struct Search { int count, K; float epsilon, alpha, temperature; int threshold; };

// one ply up to its re-rooting, all enqueued: the move -- the search's (execute, sample) or, scripted >= 0, that scripted player's -- then the mirror step and the advance
static void play_ply(omok_engine* e, const Search& s, int alive, int scripted = -1) {
    if (scripted >= 0) enqueue_opponent_move(e, scripted);
    else {
        const int rounds = enqueue_execute(e, s.count, s.K, s.epsilon, s.alpha, alive, true);
        enqueue_sample(e, s.temperature, s.threshold);
        e->sims += (double)rounds * s.K * alive;
    }
    enqueue_mirror_and_advance(e, alive, true);
}

// ends a ply: the one status read-back and the host's accounting.  *alive: the games that moved -> the games still alive; count_finished: the difference
// is games that ended (slots mode counts its games itself).  Returns the tree-error code.
static int end_ply(omok_engine* e, uint32_t* alive, bool count_finished = true) {
    uint32_t bits = 0, after = 0;
    if (read_status(e, &bits, &after)) return OMOK_ERR_HIP;
    e->ply_games += *alive;
    if (count_finished) e->finished += (double)*alive - (double)after;
    e->ply += 1;
    e->sampled = false;
    *alive = after;
    return tree_error(e, bits);
}

extern "C" int omok_advance(omok_engine* e) {
    if (!e) return OMOK_ERR_INVALID;
    if (need_net(e) || need_reset(e)) return OMOK_ERR_STATE;
    if (!e->sampled) return fail(e, OMOK_ERR_STATE, "omok_sample_actions must precede omok_advance");
    HIPCHK(e, hipSetDevice(e->cfg.device));
    uint32_t bits = 0, alive = 0;
    if (read_status(e, &bits, &alive)) return OMOK_ERR_HIP;
    enqueue_mirror_and_advance(e, (int)alive);
    return end_ply(e, &alive);
}

extern "C" int omok_selfplay_run(omok_engine* e, int32_t count, int32_t batch_size, float epsilon, float alpha,
                                 float temperature, int32_t threshold, int32_t max_plies, double* stats) {
    if (!e) return OMOK_ERR_INVALID;
    if (int rc = check_search(e, count, batch_size, epsilon, alpha, temperature)) return rc;
    HIPCHK(e, hipSetDevice(e->cfg.device));
    const Search s{count, batch_size, epsilon, alpha, temperature, threshold};
    uint32_t bits = 0, alive = 0;
    if (read_status(e, &bits, &alive)) return OMOK_ERR_HIP;
    for (int plies = 0; alive > 0 && (max_plies <= 0 || plies < max_plies); ++plies) { // trainer.rs:95
        play_ply(e, s, (int)alive);
        if (int rc = end_ply(e, &alive)) return rc;
    }
    e->sampled = false; // (also where no ply was played)
    if (stats) return omok_get_stats(e, stats);
    return OMOK_OK;
}

// Slots mode: the engine's `games` slots are kept full.  Same games, same results as an episode of `total_games` games (every game
// is keyed by its index: RNG streams by cfg.game_offset + index and the game's own ply; trees are independent), but a slot whose game
// is over takes the next index instead of idling until the longest game of the episode ends (the last 40 % of an episode's rounds
// hold < 10 % of its rows).  Games start on even engine plies only (one `side` per ply: a slot may wait one ply), finished games'
// transitions are packed out (k_replay_pack records) before their slot is reused.
// Both entry points: `logged` = omok_selfplay_run_slots_logged, which also packs the engine's per-slot move log (the staging area
// enqueue_log_move fills as in any episode: a refilled slot starts at plies = 0 on an even engine ply, so entry gs.plies of the tree of
// ply & 1 is the game's own move number and side) out to log_dev with every harvest.  Without it the launches are the ones they were.
static int run_slots(omok_engine* e, bool logged, int32_t total_games, int32_t count, int32_t batch_size, float epsilon, float alpha, float temperature,
                     int32_t threshold, void* records_dev, int64_t cap_records, void* log_dev, int64_t* game_offsets, int32_t* game_lengths,
                     int32_t* game_status, int64_t* n_records, double* stats) {
    const char* who = logged ? "omok_selfplay_run_slots_logged" : "omok_selfplay_run_slots";
    if (!e) return OMOK_ERR_INVALID;
    if (int rc = check_search(e, count, batch_size, epsilon, alpha, temperature)) return rc;
    const int G = e->cfg.games;
    if (total_games < G) return fail(e, OMOK_ERR_INVALID, "total_games (%d) must be >= the engine's game slots (%d)", total_games, G);
    if (!records_dev || cap_records < 1) return fail(e, OMOK_ERR_INVALID, "records buffer required (omok_replay_record_bytes per record)");
    if (logged && !log_dev) return fail(e, OMOK_ERR_INVALID, "log buffer required (cap_records entries of omok_game_log_entry_bytes)");
    if (no_match(e, who)) return OMOK_ERR_STATE;
    if (e->start_ply != 0) return fail(e, OMOK_ERR_STATE, "%s after omok_selfplay_reset_from: refilled slots would start from the empty board", who);
    if (e->ply != 0) return fail(e, OMOK_ERR_STATE, "%s starts from a fresh omok_selfplay_reset (ply %d)", who, e->ply);
    if (!logged && e->log_on)
        return fail(e, OMOK_ERR_STATE, "omok_selfplay_run_slots with the move log on: its games leave their slots (omok_selfplay_run_slots_logged packs their moves out, or omok_game_log_enable(e, 0) first)");
    if (logged && !e->log_on) return fail(e, OMOK_ERR_STATE, "omok_selfplay_run_slots_logged needs the move log (omok_game_log_enable(e, 1), then the reset)");
    if (logged && !e->log_started) return fail(e, OMOK_ERR_STATE, "omok_selfplay_run_slots_logged: no reset since the move log was enabled (omok_game_log_enable, then omok_selfplay_reset)");
    ENTER(e);
    // a slot's rows hold one game after another: once the run has begun the per-slot log describes no game, whatever way the run ends
    struct LogEnds { omok_engine* e; bool on; ~LogEnds() { if (on) e->log_started = false; } } log_ends{e, logged};
    Scratch sc;
    uint8_t* d_mask = sc.get<uint8_t>(G);
    long long *d_slot_off = sc.get<long long>(G), *d_out = sc.get<long long>(1);
    int32_t *d_next = sc.get<int32_t>(1), *d_new = sc.get<int32_t>(G);
    SlotMeta* d_meta = sc.get<SlotMeta>((size_t)total_games);
    if (sc.failed) return fail(e, OMOK_ERR_HIP, "slots mode: device allocation failed");
    hipMemsetAsync(d_out, 0, 8, e->st);
    hipMemsetAsync(d_meta, 0xFF, sizeof(SlotMeta) * (size_t)total_games, e->st);
    hipMemcpyAsync(d_next, &G, 4, hipMemcpyHostToDevice, e->st); // the reset started games 0 .. G-1
    const Search s{count, batch_size, epsilon, alpha, temperature, threshold};
    uint32_t bits = 0, alive = 0;
    if (read_status(e, &bits, &alive)) return OMOK_ERR_HIP;
    int rc = OMOK_OK;
    while (alive > 0) {
        play_ply(e, s, (int)alive);
        e->prof.begin(PC_PLY, e->st);
        launch_harvest(e->n, e->S, d_mask, d_slot_off, d_out, d_meta, (uint8_t*)records_dev, cap_records, e->st);
        if (logged) launch_harvest_log(e->n, e->S, e->log, d_mask, d_slot_off, (uint8_t*)log_dev, cap_records, e->st);
        if (e->ply & 1) launch_refill(e->n, e->S, e->d_root_policy, d_next, total_games, d_new, e->st); // (the ply that ends here is odd: the next one is even)
        invalidate_nets(e);
        e->prof.end(e->st);
        rc = end_ply(e, &alive, false);
        if (rc == OMOK_ERR_HIP) return rc;
        if (rc != OMOK_OK) break;
        if (alive == 0 && (e->ply & 1)) { // every slot is waiting for an even ply with games left to start: let the ply pass
            int32_t next = 0;
            hipMemcpy(&next, d_next, 4, hipMemcpyDeviceToHost);
            if (next >= total_games) break;
            e->ply += 1;
            launch_refill(e->n, e->S, e->d_root_policy, d_next, total_games, d_new, e->st);
            invalidate_nets(e);
            if (read_status(e, &bits, &alive)) return OMOK_ERR_HIP;
        }
    }
    e->sampled = false; // (also where no ply was played)
    long long out = 0;
    hipMemcpy(&out, d_out, 8, hipMemcpyDeviceToHost);
    if (n_records) *n_records = out;
    if (rc == OMOK_OK && out > cap_records) rc = fail(e, OMOK_ERR_OVERFLOW, "slots mode: %lld records do not fit the buffer (%lld)", out, (long long)cap_records);
    if (game_offsets || game_lengths || game_status) {
        std::vector<SlotMeta> meta((size_t)total_games);
        hipMemcpy(meta.data(), d_meta, sizeof(SlotMeta) * meta.size(), hipMemcpyDeviceToHost);
        for (int i = 0; i < total_games; ++i) {
            if (game_offsets) game_offsets[i] = meta[i].offset;
            if (game_lengths) game_lengths[i] = meta[i].len;
            if (game_status) game_status[i] = meta[i].status;
        }
    }
    e->finished += (double)total_games;
    if (rc != OMOK_OK) return rc;
    if (stats) return omok_get_stats(e, stats);
    return OMOK_OK;
}

extern "C" int omok_selfplay_run_slots(omok_engine* e, int32_t total_games, int32_t count, int32_t batch_size, float epsilon, float alpha,
                                       float temperature, int32_t threshold, void* records_dev, int64_t cap_records, int64_t* game_offsets,
                                       int32_t* game_lengths, int32_t* game_status, int64_t* n_records, double* stats) {
    return run_slots(e, false, total_games, count, batch_size, epsilon, alpha, temperature, threshold, records_dev, cap_records, nullptr, game_offsets,
                     game_lengths, game_status, n_records, stats);
}

extern "C" int omok_selfplay_run_slots_logged(omok_engine* e, int32_t total_games, int32_t count, int32_t batch_size, float epsilon, float alpha,
                                              float temperature, int32_t threshold, void* records_dev, int64_t cap_records, void* log_dev,
                                              int64_t* game_offsets, int32_t* game_lengths, int32_t* game_status, int64_t* n_records, double* stats) {
    return run_slots(e, true, total_games, count, batch_size, epsilon, alpha, temperature, threshold, records_dev, cap_records, log_dev, game_offsets,
                     game_lengths, game_status, n_records, stats);
}

extern "C" int32_t omok_game_log_entry_bytes(void) { return LOG_ENTRY_BYTES; }

extern "C" int omok_set_episode(omok_engine* e, uint64_t episode) {
    if (!e) return OMOK_ERR_INVALID;
    e->episode = episode;
    return OMOK_OK;
}

// Agent::compute_policy for every game (agent.rs:43-77)
extern "C" int omok_compute_policy(omok_engine* e, float* pi, uint8_t* has_policy) {
    if (!e || !pi) return OMOK_ERR_INVALID;
    if (need_reset(e)) return OMOK_ERR_STATE;
    ENTER(e);
    launch_policy(e->n, e->S, e->ply & 1, e->d_pi, e->d_has, e->st);
    HIPCHK(e, hipMemcpyAsync(pi, e->d_pi, sizeof(float) * (size_t)e->cfg.games * e->hw, hipMemcpyDeviceToHost, e->st));
    if (has_policy) HIPCHK(e, hipMemcpyAsync(has_policy, e->d_has, (size_t)e->cfg.games, hipMemcpyDeviceToHost, e->st));
    return sync_and_check(e, "compute_policy") ? OMOK_ERR_HIP : OMOK_OK;
}

// Externally chosen moves: Agent::ensure_action_exists + Agent::play_action on BOTH agents of every live game
// (agent.rs:144-232; the flow of gui/src/agent.rs:49-66 and benchmark/src/agent.rs:34-50 for a move the search did not pick).
static int stage_actions(omok_engine* e, const int32_t* actions) {
    uint32_t flags[4] = {0, 0, 0, 0};
    HIPCHK(e, hipMemsetAsync(e->d_flags, 0, 16, e->st));
    HIPCHK(e, hipMemcpyAsync(e->d_actions, actions, sizeof(int32_t) * e->cfg.games, hipMemcpyHostToDevice, e->st));
    launch_set_actions(e->n, e->S, e->ply & 1, e->d_actions, e->d_flags, e->st);
    HIPCHK(e, hipMemcpyAsync(flags, e->d_flags, 16, hipMemcpyDeviceToHost, e->st));
    if (sync_and_check(e, "play_actions")) return OMOK_ERR_HIP;
    if (flags[0] || flags[1]) { // nothing has been played yet: drop the staged moves, the position is unchanged
        launch_clear_actions(e->S, e->st);
        if (sync_and_check(e, "play_actions")) return OMOK_ERR_HIP;
        if (flags[0]) return fail(e, OMOK_ERR_ILLEGAL, "%u illegal move(s): cell occupied or out of range (place_stone -> None)", flags[0]);
        return fail(e, OMOK_ERR_INVALID, "%u live game(s) without a move: every live game moves in a ply (all games share the side to move)", flags[1]);
    }
    return OMOK_OK;
}

extern "C" int omok_set_actions(omok_engine* e, const int32_t* actions) {
    if (!e || !actions) return OMOK_ERR_INVALID;
    if (need_reset(e)) return OMOK_ERR_STATE;
    ENTER(e);
    const int rc = stage_actions(e, actions);
    if (rc == OMOK_OK) e->sampled = true;
    return rc;
}

extern "C" int omok_play_actions(omok_engine* e, const int32_t* actions) {
    if (!e || !actions) return OMOK_ERR_INVALID;
    if (need_net(e) || need_reset(e)) return OMOK_ERR_STATE;
    if (no_match(e, "omok_play_actions")) return OMOK_ERR_STATE;
    ENTER(e);
    const int rc = stage_actions(e, actions);
    if (rc != OMOK_OK) return rc;
    e->sampled = true;
    return omok_advance(e);
}

// ---- evaluation games against the scripted players (src/trainer.rs:380-394, 400-603) -----------
static int check_opponent_kind(omok_engine* e, int kind) {
    if (kind != OMOK_OPP_RANDOM && kind != OMOK_OPP_NAIVE && kind != OMOK_OPP_THREAT && kind != OMOK_OPP_VCF && kind != OMOK_OPP_GUARD)
        return fail(e, OMOK_ERR_INVALID, "unknown scripted player %d (OMOK_OPP_RANDOM, OMOK_OPP_NAIVE, OMOK_OPP_THREAT, OMOK_OPP_VCF, OMOK_OPP_GUARD)", kind);
    return 0;
}
// the engine-owned scratch of OMOK_OPP_GUARD's three passes on the live games; an engine that never plays that kind allocates nothing
static int ensure_guard_scratch(omok_engine* e, int kind) {
    if (kind != OMOK_OPP_GUARD || e->d_guard_status) return 0;
    const size_t G = (size_t)e->cfg.games;
    if (dalloc(e, &e->d_guard_out, 4 * G)) return OMOK_ERR_HIP;
    return dalloc(e, &e->d_guard_status, G * e->hw) ? OMOK_ERR_HIP : 0;
}

// the rule of a scripted player on caller-held positions (each output may be NULL).  The threat-aware kinds read the side to move; the naive rule
// tests a stone of either colour at every empty cell (trainer.rs:518,524-527) and the random one has no forced cell, so neither reads turns: any
// byte passes there and nothing of it is uploaded
static int env_scripted(omok_engine* e, const char* what, int kind, const uint8_t* boards, const uint8_t* turns, int32_t batch, int32_t* cell_out,
                        int32_t* level_out, int32_t* count_out) {
    ENTER(e);
    const size_t B = (size_t)batch;
    const bool sided = kind == OMOK_OPP_THREAT || kind == OMOK_OPP_VCF;
    Scratch sc;
    DevPositions d;
    if (const int rc = upload_positions(e, sc, what, boards, sided ? turns : nullptr, batch, sided, 3 * B, d)) return rc;
    int32_t* const host[3] = {cell_out, level_out, count_out};
    launch_env_scripted(e->n, kind, d.boards, d.turns, batch, OMOK_VCF_OPP_DEPTH, OMOK_VCF_OPP_NODES, host[0] ? d.out : nullptr, host[1] ? d.out + B : nullptr,
                        host[2] ? d.out + 2 * B : nullptr, e->st);
    download_columns(e, d.out, B, 3, host);
    return sync_and_check(e, what) ? OMOK_ERR_HIP : OMOK_OK;
}

// which level of the threat-aware rule decides on caller-held positions, its cell, and how many cells its draw chooses among
extern "C" int omok_env_threat_scan(omok_engine* e, const uint8_t* boards, const uint8_t* turns, int32_t batch, int32_t* cell_out, int32_t* level_out,
                                    int32_t* count_out) {
    if (!e || !boards || !turns || batch < 1) return OMOK_ERR_INVALID;
    return env_scripted(e, "env_threat_scan", OMOK_OPP_THREAT, boards, turns, batch, cell_out, level_out, count_out);
}

// does the side to move have a forced win by continuous fours?  (the rule: include/omok_mi355x.h; each output may be NULL)
extern "C" int omok_env_vcf_solve(omok_engine* e, const uint8_t* boards, const uint8_t* turns, int32_t batch, int32_t max_depth, int32_t max_nodes,
                                  int32_t* verdict_out, int32_t* cell_out, int32_t* moves_out, int32_t* nodes_out, int32_t* pv_out) {
    if (!e || !boards || !turns || batch < 1) return OMOK_ERR_INVALID;
    if (max_depth < 1 || max_depth > 16) return fail(e, OMOK_ERR_INVALID, "env_vcf_solve: max_depth %d outside 1..16", max_depth);
    if (max_nodes < 1 || max_nodes > 65536) return fail(e, OMOK_ERR_INVALID, "env_vcf_solve: max_nodes %d outside 1..65536", max_nodes);
    ENTER(e);
    const size_t B = (size_t)batch, len = (size_t)(2 * max_depth - 1);
    Scratch sc;
    DevPositions d;
    if (const int rc = upload_positions(e, sc, "env_vcf_solve", boards, turns, batch, true, (4 + len) * B, d)) return rc;
    int32_t* const host[4] = {verdict_out, cell_out, moves_out, nodes_out};
    e->prof.begin(PC_PLY, e->st); // (timed only under omok_set_profiling: tools/vcf_defend_timing.py)
    launch_env_vcf(e->n, d.boards, d.turns, batch, max_depth, max_nodes, host[0] ? d.out : nullptr, host[1] ? d.out + B : nullptr,
                   host[2] ? d.out + 2 * B : nullptr, host[3] ? d.out + 3 * B : nullptr, pv_out ? d.out + 4 * B : nullptr, e->st);
    e->prof.end(e->st);
    download_columns(e, d.out, B, 4, host);
    if (pv_out) hipMemcpyAsync(pv_out, d.out + 4 * B, len * B * 4, hipMemcpyDeviceToHost, e->st);
    return sync_and_check(e, "env_vcf_solve") ? OMOK_ERR_HIP : OMOK_OK;
}

// which moves of the side to move do not lose to the other side's forced win by continuous fours?  (the rule: include/omok_mi355x.h; each output
// may be NULL).  The slab: nodes, reply [B][HW], threat [B][3], then the status and moves bytes [B][HW], each rounded up to whole words
extern "C" int omok_env_vcf_defend(omok_engine* e, const uint8_t* boards, const uint8_t* turns, int32_t batch, int32_t max_depth, int32_t max_nodes,
                                   uint8_t* status_out, uint8_t* moves_out, int32_t* nodes_out, int32_t* reply_out, int32_t* threat_out) {
    if (!e || !boards || !turns || batch < 1) return OMOK_ERR_INVALID;
    if (max_depth < 1 || max_depth > 16) return fail(e, OMOK_ERR_INVALID, "env_vcf_defend: max_depth %d outside 1..16", max_depth);
    if (max_nodes < 1 || max_nodes > 65536) return fail(e, OMOK_ERR_INVALID, "env_vcf_defend: max_nodes %d outside 1..65536", max_nodes);
    ENTER(e);
    const size_t B = (size_t)batch, cells = B * e->hw, byte_words = (cells + 3) / 4;
    Scratch sc;
    DevPositions d;
    if (const int rc = upload_positions(e, sc, "env_vcf_defend", boards, turns, batch, true, 2 * cells + 3 * B + 2 * byte_words, d)) return rc;
    int32_t *d_nodes = d.out, *d_reply = d.out + cells, *d_threat = d.out + 2 * cells;
    uint8_t *d_status = (uint8_t*)(d_threat + 3 * B), *d_moves = d_status + 4 * byte_words;
    e->prof.begin(PC_PLY, e->st); // (timed only under omok_set_profiling: tools/vcf_defend_timing.py)
    launch_env_vcf_defend(e->n, d.boards, d.turns, batch, max_depth, max_nodes, status_out ? d_status : nullptr, moves_out ? d_moves : nullptr,
                          nodes_out ? d_nodes : nullptr, reply_out ? d_reply : nullptr, threat_out ? d_threat : nullptr, e->st);
    e->prof.end(e->st);
    download_rows(e, d_status, cells, status_out);
    download_rows(e, d_moves, cells, moves_out);
    download_rows(e, d_nodes, cells, nodes_out);
    download_rows(e, d_reply, cells, reply_out);
    download_rows(e, d_threat, 3 * B, threat_out);
    return sync_and_check(e, "env_vcf_defend") ? OMOK_ERR_HIP : OMOK_OK;
}

// OMOK_OPP_GUARD on caller-held positions: the three passes in the call's own scratch (the engine's state is not touched).  The slab: cell, step,
// level, count [B] (the passes' carry as well, so all four are always written on the device), the draw words [B], then the status rows [B][HW]
static int env_guard(omok_engine* e, const char* what, const uint8_t* boards, const uint8_t* turns, const uint32_t* draws, int32_t batch, int depth, int nodes,
                     int32_t* const* host) {
    ENTER(e);
    const size_t B = (size_t)batch, cells = B * e->hw;
    Scratch sc;
    DevPositions d;
    if (const int rc = upload_positions(e, sc, what, boards, turns, batch, true, 5 * B + (cells + 3) / 4, d)) return rc;
    uint32_t* d_draws = draws ? (uint32_t*)(d.out + 4 * B) : nullptr;
    if (draws) hipMemcpyAsync(d_draws, draws, B * 4, hipMemcpyHostToDevice, e->st);
    e->prof.begin(PC_PLY, e->st); // (timed only under omok_set_profiling)
    launch_guard(e->n, e->S, GuardSrc{d.boards, d.turns, d_draws, 0, 0, 0}, batch, depth, nodes, d.out, (uint8_t*)(d.out + 5 * B), nullptr, e->st);
    e->prof.end(e->st);
    download_columns(e, d.out, B, 4, host);
    return sync_and_check(e, what) ? OMOK_ERR_HIP : OMOK_OK;
}

// the defending player's move and the step of its rule that decided (the rule: include/omok_mi355x.h; each output may be NULL)
extern "C" int omok_env_guard_scan(omok_engine* e, const uint8_t* boards, const uint8_t* turns, const uint32_t* draws, int32_t batch, int32_t max_depth,
                                   int32_t max_nodes, int32_t* cell_out, int32_t* step_out, int32_t* level_out, int32_t* count_out) {
    if (!e || !boards || !turns || batch < 1) return OMOK_ERR_INVALID;
    if (max_depth < 1 || max_depth > 16) return fail(e, OMOK_ERR_INVALID, "env_guard_scan: max_depth %d outside 1..16", max_depth);
    if (max_nodes < 1 || max_nodes > 4096) return fail(e, OMOK_ERR_INVALID, "env_guard_scan: max_nodes %d outside 1..4096", max_nodes);
    int32_t* const host[4] = {cell_out, step_out, level_out, count_out};
    return env_guard(e, "env_guard_scan", boards, turns, draws, batch, max_depth, max_nodes, host);
}

// the cell a scripted player's rule is forced to (-1 where it would draw) on caller-held positions: for the naive player the forced part of
// trainer.rs:514-531 under the rules of environment/src/lib.rs:104-190
extern "C" int omok_env_scripted_actions(omok_engine* e, int32_t kind, const uint8_t* boards, const uint8_t* turns, int32_t batch, int32_t* forced_out) {
    if (!e || !boards || !turns || !forced_out || batch < 1) return OMOK_ERR_INVALID;
    if (check_opponent_kind(e, kind)) return OMOK_ERR_INVALID;
    if (kind == OMOK_OPP_GUARD) { // the player's cell with x0 = 0 where no draw decided
        std::vector<int32_t> cell((size_t)batch), count((size_t)batch);
        int32_t* const host[4] = {cell.data(), nullptr, nullptr, count.data()};
        if (const int rc = env_guard(e, "env_scripted_actions", boards, turns, nullptr, batch, OMOK_VCF_OPP_DEPTH, OMOK_VCF_OPP_NODES, host)) return rc;
        for (size_t b = 0; b < (size_t)batch; ++b) forced_out[b] = count[b] == 0 ? cell[b] : -1;
        return OMOK_OK;
    }
    return env_scripted(e, "env_scripted_actions", kind, boards, turns, batch, forced_out, nullptr, nullptr);
}

// the scripted player's move of every live game (trainer.rs:508-534 naive, :452-455 random), staged like omok_set_actions
extern "C" int omok_opponent_actions(omok_engine* e, int32_t kind, int32_t* actions) {
    if (!e) return OMOK_ERR_INVALID;
    if (need_reset(e)) return OMOK_ERR_STATE;
    if (no_match(e, "omok_opponent_actions")) return OMOK_ERR_STATE;
    if (check_opponent_kind(e, kind)) return OMOK_ERR_INVALID;
    ENTER(e);
    if (const int rc = ensure_guard_scratch(e, kind)) return rc;
    enqueue_opponent_move(e, kind);
    if (actions) HIPCHK(e, hipMemcpyAsync(actions, e->d_actions, sizeof(int32_t) * e->cfg.games, hipMemcpyDeviceToHost, e->st));
    if (sync_and_check(e, "opponent_actions")) return OMOK_ERR_HIP;
    e->sampled = true;
    return OMOK_OK;
}

// play_against_naive_player (trainer.rs:487-603; opponent_side 0) / _play_against_random_player (:400-485; opponent_side 1): the scripted
// player's plies are external moves (ensure_action_exists + play_action, :536-538 / :457-459), the net's plies are execute + sample_action(Best)
// + play_action (:562-577 / :416-431)
extern "C" int omok_versus_run(omok_engine* e, int32_t kind, int32_t opponent_side, int32_t count, int32_t batch_size, float epsilon, float alpha,
                               int32_t max_plies, int32_t* results, double* stats) {
    if (!e) return OMOK_ERR_INVALID;
    if (int rc = check_search(e, count, batch_size, epsilon, alpha)) return rc;
    if (no_match(e, "omok_versus_run")) return OMOK_ERR_STATE;
    if (check_opponent_kind(e, kind)) return OMOK_ERR_INVALID;
    if (opponent_side != 0 && opponent_side != 1) return fail(e, OMOK_ERR_INVALID, "opponent_side %d is neither 0 (Black) nor 1 (White)", opponent_side);
    if (e->ply != e->start_ply)
        return fail(e, OMOK_ERR_STATE, "omok_versus_run starts at a fresh reset: %d move(s) were played since (the episode is at ply %d)", e->ply - e->start_ply, e->ply);
    HIPCHK(e, hipSetDevice(e->cfg.device));
    if (const int rc = ensure_guard_scratch(e, kind)) return rc;
    const Search s{count, batch_size, epsilon, alpha, 1.0f, 0}; // threshold 0: sample_action(Best) on every ply of the net (:576, :430)
    uint32_t bits = 0, alive = 0;
    if (read_status(e, &bits, &alive)) return OMOK_ERR_HIP;
    for (int plies = 0; alive > 0 && (max_plies <= 0 || plies < max_plies); ++plies) {
        play_ply(e, s, (int)alive, (e->ply & 1) == opponent_side ? kind : -1); // the scripted player's plies search nothing: no sims
        if (int rc = end_ply(e, &alive)) return rc;
    }
    e->sampled = false; // (also where no ply was played)
    if (results) {
        std::vector<GameState> gs((size_t)e->cfg.games);
        HIPCHK(e, hipMemcpyAsync(gs.data(), e->S.gs, sizeof(GameState) * gs.size(), hipMemcpyDeviceToHost, e->st));
        if (sync_and_check(e, "versus_run")) return OMOK_ERR_HIP;
        results[0] = results[1] = results[2] = 0;
        for (const GameState& g : gs) {
            if (g.alive) continue;
            if (g.status == ST_BLACK_WIN) results[0] += 1;
            else if (g.status == ST_WHITE_WIN) results[1] += 1;
            else if (g.status == ST_DRAW) results[2] += 1;
        }
    }
    if (stats) return omok_get_stats(e, stats);
    return OMOK_OK;
}

// children of a root in insertion order (Node::children of MCTS::root, mcts/src/node.rs:10-21): action, n, w, p
extern "C" int omok_root_children(omok_engine* e, int32_t game, int32_t side, int32_t* actions, uint32_t* n, float* w, float* p, int32_t cap) {
    if (!e || game < 0 || game >= e->cfg.games || (side != 0 && side != 1) || cap < 0) return OMOK_ERR_INVALID;
    ENTER(e);
    const size_t t = (size_t)side * e->cfg.games + game, rp = (size_t)e->rowp, nw2 = 2 * (size_t)e->nw;
    const size_t tn = t * (size_t)e->S.stride_nodes, tt = t * (size_t)e->S.stride_tables;
    NodeHdr h0;
    launch_materialise(e->n, e->S, (int)t, 1, e->st); // (a raw root row of a lazy round -> the probabilities read below)
    HIPCHK(e, hipMemcpyAsync(&h0, e->S.hdr + tn, sizeof(h0), hipMemcpyDeviceToHost, e->st));
    if (sync_and_check(e, "root_children")) return OMOK_ERR_HIP;
    if (h0.table == NONE16 || h0.nch == 0) return 0;
    std::vector<uint32_t> cn(rp);
    std::vector<float> cw(rp), pol(rp);
    std::vector<uint8_t> co(rp);
    std::vector<uint64_t> bb(nw2);
    const size_t row = (tt + h0.table) * rp;
    hipMemcpyAsync(cn.data(), e->S.tcn + row, 4 * rp, hipMemcpyDeviceToHost, e->st);
    hipMemcpyAsync(cw.data(), e->S.tcw + row, 4 * rp, hipMemcpyDeviceToHost, e->st);
    hipMemcpyAsync(co.data(), e->S.tcorder + row, rp, hipMemcpyDeviceToHost, e->st);
    hipMemcpyAsync(pol.data(), e->S.policy + tn * rp, 4 * rp, hipMemcpyDeviceToHost, e->st);
    hipMemcpyAsync(bb.data(), e->S.board + tn * nw2, 8 * nw2, hipMemcpyDeviceToHost, e->st);
    if (sync_and_check(e, "root_children")) return OMOK_ERR_HIP;
    for (int a = 0; a < e->hw; ++a) {
        const int rank = co[a];
        if (rank == NONE8 || rank >= cap) continue;
        if (actions) actions[rank] = a;
        if (n) n[rank] = cn[a];
        if (w) w[rank] = cw[a];
        if (p) { // child.p == root.policy[action] (node.rs:76, pme.rs:71-75,256-261)
            const bool occ = ((bb[a / 64] | bb[e->nw + a / 64]) >> (a % 64)) & 1ULL;
            p[rank] = h0.has_policy ? pol[a] : ((occ || h0.legal == 0) ? 0.0f : 1.0f / (float)h0.legal);
        }
    }
    return h0.nch;
}

// Environment::place_stone on caller-held environments (environment/src/lib.rs:104-166), batched
extern "C" int omok_env_place_stone(omok_engine* e, uint8_t* boards, uint8_t* turns, uint16_t* legal, const int32_t* actions,
                                    int32_t batch, int32_t* status_out) {
    if (!e || !boards || !turns || !legal || !actions || !status_out || batch < 1) return OMOK_ERR_INVALID;
    ENTER(e);
    const size_t B = (size_t)batch;
    Scratch sc;
    DevPositions d;
    if (const int rc = upload_positions(e, sc, "env_place_stone", boards, turns, batch, false, 3 * B, d)) return rc; // the slab: actions, status, legal (2 B each)
    int32_t *d_act = d.out, *d_status = d.out + B;
    uint16_t* d_legal = (uint16_t*)(d.out + 2 * B);
    hipMemcpyAsync(d_legal, legal, B * 2, hipMemcpyHostToDevice, e->st);
    hipMemcpyAsync(d_act, actions, B * 4, hipMemcpyHostToDevice, e->st);
    launch_env_place(e->n, d.boards, d.turns, d_legal, d_act, batch, d_status, e->st);
    hipMemcpyAsync(boards, d.boards, B * e->hw, hipMemcpyDeviceToHost, e->st);
    hipMemcpyAsync(turns, d.turns, B, hipMemcpyDeviceToHost, e->st);
    hipMemcpyAsync(legal, d_legal, B * 2, hipMemcpyDeviceToHost, e->st);
    hipMemcpyAsync(status_out, d_status, B * 4, hipMemcpyDeviceToHost, e->st);
    return sync_and_check(e, "env_place_stone") ? OMOK_ERR_HIP : OMOK_OK;
}

// ---- step-wise API (parity tests) --------------------------------------------------------------
extern "C" int omok_round_generate(omok_engine* e, int32_t round, int32_t batch_size, float epsilon, float alpha, int32_t* n_requests) {
    if (!e) return OMOK_ERR_INVALID;
    if (need_reset(e)) return OMOK_ERR_STATE;
    if (check_exec_args(e, 1, batch_size, epsilon, alpha)) return OMOK_ERR_INVALID;
    HIPCHK(e, hipSetDevice(e->cfg.device));
    enqueue_round(e, round, batch_size, epsilon, alpha, false, e->cfg.games);
    int32_t cnt = 0;
    HIPCHK(e, hipMemcpyAsync(&cnt, e->S.d_count, sizeof(int32_t), hipMemcpyDeviceToHost, e->st));
    uint32_t bits = 0, alive = 0;
    if (read_status(e, &bits, &alive)) return OMOK_ERR_HIP;
    if (e->match && match_counts(e)) return OMOK_ERR_HIP;
    e->sims += (double)batch_size * alive;
    e->round_reqs = cnt;
    e->round_cap = (int)alive * batch_size;
    if (n_requests) *n_requests = cnt;
    return tree_error(e, bits);
}

static int requests_to_inputs(omok_engine* e, int cnt, float* inputs) {
    if (cnt <= 0) return OMOK_OK;
    launch_encode_requests(e->n, e->S, e->net.in_f32, cnt, e->st);
    HIPCHK(e, hipMemcpyAsync(inputs, e->net.in_f32, sizeof(float) * 3 * (size_t)e->hw * cnt, hipMemcpyDeviceToHost, e->st));
    return sync_and_check(e, "request inputs") ? OMOK_ERR_HIP : OMOK_OK;
}

static int outputs_to_host(omok_engine* e, Net& net, int cnt, float* p, float* v) {
    if (cnt <= 0) return OMOK_OK;
    if (rows_to_host(e, net, net.p, e->rowp, net.v, cnt, p, v)) return OMOK_ERR_HIP;
    return sync_and_check(e, "outputs") ? OMOK_ERR_HIP : OMOK_OK;
}

static int inject_outputs(omok_engine* e, Net& net, int cnt, const float* p, const float* v) {
    if (cnt <= 0) return OMOK_OK;
    float* d_pack = net.in_f32;
    HIPCHK(e, hipMemcpyAsync(d_pack, p, sizeof(float) * (size_t)cnt * e->hw, hipMemcpyHostToDevice, e->st));
    const size_t tot = (size_t)cnt * e->rowp;
    k_unpack_rows<<<(unsigned)((tot + 255) / 256), 256, 0, e->st>>>(d_pack, net.p, e->hw, e->rowp, cnt);
    if (v) HIPCHK(e, hipMemcpyAsync(net.v, v, sizeof(float) * cnt, hipMemcpyHostToDevice, e->st));
    return sync_and_check(e, "inject") ? OMOK_ERR_HIP : OMOK_OK;
}

// the rows of the pending step-wise batch on the trees of `side`, block by block (the list's row order: block i's rows start at blk[i].off and are in its net's buffers)
static int pending_outputs(omok_engine* e, int side, int rows, float* p, float* v) {
    Block blk[2];
    const int nb = eval_blocks(e, side, rows, true, blk);
    for (int i = 0; i < nb; ++i)
        if (outputs_to_host(e, *blk[i].net, blk[i].rows, p + (size_t)blk[i].off * e->hw, v ? v + blk[i].off : nullptr)) return OMOK_ERR_HIP;
    return OMOK_OK;
}
static int pending_inject(omok_engine* e, int side, int rows, const float* p, const float* v) {
    Block blk[2];
    const int nb = eval_blocks(e, side, rows, true, blk);
    for (int i = 0; i < nb; ++i)
        if (inject_outputs(e, *blk[i].net, blk[i].rows, p + (size_t)blk[i].off * e->hw, v ? v + blk[i].off : nullptr)) return OMOK_ERR_HIP;
    return OMOK_OK;
}

extern "C" int omok_round_inputs(omok_engine* e, float* inputs) {
    if (!e || !inputs) return OMOK_ERR_INVALID;
    ENTER(e);
    if (e->round_reqs < 0) return fail(e, OMOK_ERR_STATE, "no generated round");
    return requests_to_inputs(e, e->round_reqs, inputs);
}
extern "C" int omok_round_eval(omok_engine* e) {
    ENTER(e);
    if (need_net(e)) return OMOK_ERR_STATE;
    if (e->round_reqs < 0) return fail(e, OMOK_ERR_STATE, "no generated round");
    if (e->round_reqs == 0) return OMOK_OK;
    Block blk[2];
    const int nb = eval_blocks(e, e->ply & 1, e->round_reqs, true, blk);
    for (int i = 0; i < nb; ++i)
        if (blk[i].rows > 0) block_forward(e, blk[i], e->round_cap, e->ply & 1);
    return sync_and_check(e, "round_eval") ? OMOK_ERR_HIP : OMOK_OK;
}
extern "C" int omok_round_outputs(omok_engine* e, float* p, float* v) {
    if (!e || !p) return OMOK_ERR_INVALID;
    ENTER(e);
    if (e->round_reqs < 0) return fail(e, OMOK_ERR_STATE, "no generated round");
    return pending_outputs(e, e->ply & 1, e->round_reqs, p, v);
}
// the pre-softmax policy logits and the pre-tanh value of the pending round's evaluation (precision evidence for the path the search rounds take)
extern "C" int omok_round_logits(omok_engine* e, float* logits, float* vpre) {
    if (!e || !logits) return OMOK_ERR_INVALID;
    ENTER(e);
    if (e->round_reqs < 0) return fail(e, OMOK_ERR_STATE, "no generated round");
    Block blk[2];
    const int nb = eval_blocks(e, e->ply & 1, e->round_reqs, true, blk);
    for (int i = 0; i < nb; ++i) { // (match episodes: block by block, each from its own net)
        Net& net = *blk[i].net;
        const int rows = blk[i].rows, off = blk[i].off;
        if (rows == 0) continue;
        if (net.mode == OMOK_NET_F32 && rows > net.chunk)
            return fail(e, OMOK_ERR_STATE, "omok_round_logits: OMOK_NET_F32 keeps the logits of its last chunk of %d rows only", net.chunk);
        int stride = 0;
        const float* lg = net_logits(net, &stride);
        if (rows_to_host(e, net, lg, stride, net.vpre, rows, logits + (size_t)off * e->hw, vpre ? vpre + off : nullptr)) return OMOK_ERR_HIP;
        if (sync_and_check(e, "round_logits")) return OMOK_ERR_HIP;
    }
    return OMOK_OK;
}
extern "C" int omok_round_inject(omok_engine* e, const float* p, const float* v) {
    if (!e || !p || !v) return OMOK_ERR_INVALID;
    ENTER(e);
    if (e->round_reqs < 0) return fail(e, OMOK_ERR_STATE, "no generated round");
    return pending_inject(e, e->ply & 1, e->round_reqs, p, v);
}
extern "C" int omok_round_scatter(omok_engine* e) {
    ENTER(e);
    if (e->round_reqs < 0) return fail(e, OMOK_ERR_STATE, "no generated round");
    const int side = e->ply & 1;
    Block blk[2];
    const int nb = eval_blocks(e, side, e->round_reqs, true, blk);
    for (int i = 0; i < nb; ++i)
        if (blk[i].rows > 0) launch_scatter(e->n, blk[i].view, side, blk[i].net->p, blk[i].net->v, blk[i].rows, e->st, !e->match);
    if (e->match && e->round_reqs > 0) { // the blocks' scatters ran no backups: they read one v array in list order
        match_join(e, side, false, e->round_reqs);
        launch_backups(e->n, e->S, side, net_at(e, side).v, e->st);
    }
    e->round_reqs = -1;
    return sync_and_check(e, "round_scatter") ? OMOK_ERR_HIP : OMOK_OK;
}

extern "C" int omok_mirror_generate(omok_engine* e, int32_t* n_requests) {
    ENTER(e);
    if (need_reset(e)) return OMOK_ERR_STATE;
    if (!e->sampled) return fail(e, OMOK_ERR_STATE, "omok_sample_actions must precede the mirror step");
    launch_mirror_scan(e->n, e->S, e->ply & 1, e->st);
    k_add_evals<<<1, 64, 0, e->st>>>(e->S.d_count, e->d_evals);
    if (e->match) match_split(e, 1 - (e->ply & 1), e->cfg.games);
    int32_t cnt = 0;
    HIPCHK(e, hipMemcpyAsync(&cnt, e->S.d_count, sizeof(int32_t), hipMemcpyDeviceToHost, e->st));
    if (sync_and_check(e, "mirror_generate")) return OMOK_ERR_HIP;
    if (e->match && match_counts(e)) return OMOK_ERR_HIP;
    e->mirror_reqs = cnt;
    if (n_requests) *n_requests = cnt;
    return OMOK_OK;
}
extern "C" int omok_mirror_inputs(omok_engine* e, float* inputs) {
    if (!e || !inputs) return OMOK_ERR_INVALID;
    ENTER(e);
    if (e->mirror_reqs < 0) return fail(e, OMOK_ERR_STATE, "no generated mirror batch");
    return requests_to_inputs(e, e->mirror_reqs, inputs);
}
extern "C" int omok_mirror_eval(omok_engine* e) {
    ENTER(e);
    if (need_net(e)) return OMOK_ERR_STATE;
    if (e->mirror_reqs < 0) return fail(e, OMOK_ERR_STATE, "no generated mirror batch");
    Block blk[2];
    const int nb = eval_blocks(e, 1 - (e->ply & 1), e->mirror_reqs, true, blk);
    for (int i = 0; i < nb; ++i)
        if (blk[i].rows > 0) block_forward(e, blk[i], blk[i].rows);
    return sync_and_check(e, "mirror_eval") ? OMOK_ERR_HIP : OMOK_OK;
}
extern "C" int omok_mirror_outputs(omok_engine* e, float* p) {
    if (!e || !p) return OMOK_ERR_INVALID;
    ENTER(e);
    if (e->mirror_reqs < 0) return fail(e, OMOK_ERR_STATE, "no generated mirror batch");
    return pending_outputs(e, 1 - (e->ply & 1), e->mirror_reqs, p, nullptr);
}
extern "C" int omok_mirror_inject(omok_engine* e, const float* p) {
    if (!e || !p) return OMOK_ERR_INVALID;
    ENTER(e);
    if (e->mirror_reqs < 0) return fail(e, OMOK_ERR_STATE, "no generated mirror batch");
    return pending_inject(e, 1 - (e->ply & 1), e->mirror_reqs, p, nullptr);
}
extern "C" int omok_mirror_apply(omok_engine* e) {
    ENTER(e);
    if (e->mirror_reqs < 0) return fail(e, OMOK_ERR_STATE, "no generated mirror batch");
    uint32_t bits = 0, alive = 0;
    if (read_status(e, &bits, &alive)) return OMOK_ERR_HIP;
    enqueue_advance(e, e->cfg.games);
    e->mirror_reqs = -1;
    return end_ply(e, &alive);
}

// ---- game records: the move log and the batched replay ------------------------------------------------
// One record per move of src/trainer.rs:95-205 / benchmark/src/main.rs:60-105 (the reference keeps the Transition of sampled moves only,
// trainer.rs:169-173): allocated on the first enable, started by every successful reset, written by k_log_move in front of k_advance.
extern "C" int omok_game_log_enable(omok_engine* e, int32_t enabled) {
    if (!e) return OMOK_ERR_INVALID;
    ENTER(e);
    if (!enabled) {
        if (e->log_mem) {
            HIPCHK(e, hipStreamSynchronize(e->st));
            hipFree(e->log_mem);
            e->bytes -= (size_t)e->cfg.games * e->hw * 19;
        }
        e->log_mem = nullptr;
        e->log = GameLog{};
        e->log_on = e->log_started = false;
        return OMOK_OK;
    }
    if (e->log_on) return OMOK_OK;
    const size_t cells = (size_t)e->cfg.games * e->hw; // 4 + 4 + 4 + 4 + 2 + 1 = 19 B per cell, the widest arrays first: every one is aligned
    hipError_t r = hipMalloc(&e->log_mem, cells * 19);
    if (r != hipSuccess) { e->log_mem = nullptr; return fail(e, OMOK_ERR_HIP, "move log: hipMalloc(%zu bytes) failed: %s", cells * 19, hipGetErrorString(r)); }
    uint8_t* p = (uint8_t*)e->log_mem;
    e->log.root_n = (uint32_t*)p;
    e->log.root_w = (float*)(p + cells * 4);
    e->log.child_n = (uint32_t*)(p + cells * 8);
    e->log.child_w = (float*)(p + cells * 12);
    e->log.move = (uint16_t*)(p + cells * 16);
    e->log.start_board = p + cells * 18;
    e->bytes += cells * 19;
    e->log_on = true;
    e->log_started = false; // from the next reset on
    return OMOK_OK;
}

extern "C" int omok_game_log_read(omok_engine* e, int32_t first_game, int32_t games, uint8_t* start_boards, int32_t* lengths, uint16_t* moves,
                                  uint32_t* root_n, float* root_w, uint32_t* child_n, float* child_w) {
    if (!e) return OMOK_ERR_INVALID;
    if (!e->log_on) return fail(e, OMOK_ERR_STATE, "the move log is off (omok_game_log_enable)");
    if (!e->log_started) return fail(e, OMOK_ERR_STATE, "no reset since the move log was enabled: it starts at the next reset");
    if (first_game < 0 || games < 0 || (int64_t)first_game + games > e->cfg.games)
        return fail(e, OMOK_ERR_INVALID, "games [%d, %d + %d) outside [0, %d]", first_game, first_game, games, e->cfg.games);
    if (games == 0) return OMOK_OK;
    ENTER(e);
    const size_t hw = (size_t)e->hw, off = (size_t)first_game * hw, cells = (size_t)games * hw;
    std::vector<GameState> gs((size_t)games);
    HIPCHK(e, hipMemcpyAsync(gs.data(), e->S.gs + first_game, sizeof(GameState) * gs.size(), hipMemcpyDeviceToHost, e->st));
    if (start_boards) HIPCHK(e, hipMemcpyAsync(start_boards, e->log.start_board + off, cells, hipMemcpyDeviceToHost, e->st));
    if (moves) HIPCHK(e, hipMemcpyAsync(moves, e->log.move + off, cells * 2, hipMemcpyDeviceToHost, e->st));
    if (root_n) HIPCHK(e, hipMemcpyAsync(root_n, e->log.root_n + off, cells * 4, hipMemcpyDeviceToHost, e->st));
    if (root_w) HIPCHK(e, hipMemcpyAsync(root_w, e->log.root_w + off, cells * 4, hipMemcpyDeviceToHost, e->st));
    if (child_n) HIPCHK(e, hipMemcpyAsync(child_n, e->log.child_n + off, cells * 4, hipMemcpyDeviceToHost, e->st));
    if (child_w) HIPCHK(e, hipMemcpyAsync(child_w, e->log.child_w + off, cells * 4, hipMemcpyDeviceToHost, e->st));
    if (sync_and_check(e, "game_log_read")) return OMOK_ERR_HIP;
    // a reset sets the lengths to 0 and leaves the arrays as they were: what lies at and beyond a game's length is blanked here
    for (size_t g = 0; g < (size_t)games; ++g) {
        int len = gs[g].plies - e->start_ply;
        len = len < 0 ? 0 : (len > e->hw ? e->hw : len);
        if (lengths) lengths[g] = len;
        for (size_t i = g * hw + (size_t)len; i < (g + 1) * hw; ++i) {
            if (moves) moves[i] = 0xFFFFu;
            if (root_n) root_n[i] = 0u;
            if (root_w) root_w[i] = 0.0f;
            if (child_n) child_n[i] = 0u;
            if (child_w) child_w[i] = 0.0f;
        }
    }
    return OMOK_OK;
}

// Environment::place_stone (environment/src/lib.rs:104-166) move by move on caller-held records: touches no engine state, needs no net
extern "C" int omok_env_replay(omok_engine* e, const uint8_t* start_boards, const uint16_t* moves, const int32_t* lengths, int32_t batch, int32_t stride,
                               int32_t upto, uint8_t* boards_out, int32_t* status_out, int32_t* played_out) {
    if (!e || !moves || !lengths) return OMOK_ERR_INVALID;
    if (batch < 1) return fail(e, OMOK_ERR_INVALID, "batch %d < 1", batch);
    if (stride < 1) return fail(e, OMOK_ERR_INVALID, "stride %d < 1", stride);
    for (int b = 0; b < batch; ++b)
        if (lengths[b] < 0 || lengths[b] > stride) return fail(e, OMOK_ERR_INVALID, "game %d: length %d outside [0, stride = %d]", b, lengths[b], stride);
    ENTER(e);
    const size_t B = (size_t)batch, hw = (size_t)e->hw;
    Scratch sc;
    uint8_t* d_start = nullptr;
    std::vector<int32_t> host((size_t)2 * B); // verdicts | lengths
    if (start_boards && check_positions(e, sc, start_boards, batch, host.data(), nullptr, &d_start)) return OMOK_ERR_HIP;
    memcpy(host.data() + B, lengths, B * 4);
    // one allocation: verdicts, lengths, status, played (4 B each), moves (2 B), boards (1 B)
    uint8_t* d = sc.get<uint8_t>(B * 16 + B * stride * 2 + B * hw);
    if (!d) return fail(e, OMOK_ERR_HIP, "env_replay: device allocation failed");
    int32_t *d_verdict = (int32_t*)d, *d_len = d_verdict + B, *d_status = d_len + B, *d_played = d_status + B;
    uint16_t* d_moves = (uint16_t*)(d + B * 16);
    uint8_t* d_boards = d + B * 16 + B * stride * 2;
    hipMemcpyAsync(d_verdict, host.data(), B * 8, hipMemcpyHostToDevice, e->st);
    hipMemcpyAsync(d_moves, moves, B * stride * 2, hipMemcpyHostToDevice, e->st);
    e->prof.begin(PC_PLY, e->st); // (timed only under omok_set_profiling: tools/game_log_timing.py)
    launch_replay(e->n, d_start, d_start ? d_verdict : nullptr, d_moves, d_len, batch, stride, upto, d_boards, d_status, d_played, e->st);
    e->prof.end(e->st);
    if (boards_out) hipMemcpyAsync(boards_out, d_boards, B * hw, hipMemcpyDeviceToHost, e->st);
    if (status_out) hipMemcpyAsync(status_out, d_status, B * 4, hipMemcpyDeviceToHost, e->st);
    if (played_out) hipMemcpyAsync(played_out, d_played, B * 4, hipMemcpyDeviceToHost, e->st);
    return sync_and_check(e, "env_replay") ? OMOK_ERR_HIP : OMOK_OK;
}

// ---- inspection ----------------------------------------------------------------------------------
extern "C" int omok_alive_count(omok_engine* e) {
    ENTER(e);
    uint32_t bits = 0, alive = 0;
    if (read_status(e, &bits, &alive)) return OMOK_ERR_HIP;
    return (int)alive;
}
extern "C" int omok_current_ply(omok_engine* e) { return e ? e->ply : OMOK_ERR_INVALID; }

extern "C" int omok_game_info(omok_engine* e, uint8_t* alive, uint8_t* status, int32_t* plies) {
    if (!e) return OMOK_ERR_INVALID;
    ENTER(e);
    std::vector<GameState> gs((size_t)e->cfg.games);
    HIPCHK(e, hipMemcpyAsync(gs.data(), e->S.gs, sizeof(GameState) * gs.size(), hipMemcpyDeviceToHost, e->st));
    if (sync_and_check(e, "game_info")) return OMOK_ERR_HIP;
    for (size_t g = 0; g < gs.size(); ++g) {
        if (alive) alive[g] = gs[g].alive;
        if (status) status[g] = gs[g].status;
        if (plies) plies[g] = gs[g].plies;
    }
    return OMOK_OK;
}

extern "C" int omok_tree_root(omok_engine* e, int32_t game, int32_t side, uint32_t* root_n, float* root_w, int32_t* n_nodes, int32_t* n_tables) {
    if (!e || game < 0 || game >= e->cfg.games || (side != 0 && side != 1)) return OMOK_ERR_INVALID;
    ENTER(e);
    TreeState ts;
    HIPCHK(e, hipMemcpyAsync(&ts, e->S.ts + (size_t)side * e->cfg.games + game, sizeof(ts), hipMemcpyDeviceToHost, e->st));
    if (sync_and_check(e, "tree_root")) return OMOK_ERR_HIP;
    if (root_n) *root_n = ts.root_n;
    if (root_w) *root_w = ts.root_w;
    if (n_nodes) *n_nodes = (int32_t)ts.n_nodes;
    if (n_tables) *n_tables = (int32_t)ts.n_tables;
    return OMOK_OK;
}

// root_n / root_w of the side-to-move tree of every game: what an analysis caller reads beside omok_compute_policy
extern "C" int omok_root_stats(omok_engine* e, uint32_t* n, float* w) {
    if (!e || !n || !w) return OMOK_ERR_INVALID;
    if (need_reset(e)) return OMOK_ERR_STATE;
    ENTER(e);
    const size_t G = (size_t)e->cfg.games;
    uint32_t* d_n = (uint32_t*)e->d_pi; // (omok_compute_policy's staging buffer, [G][HW] f32: 2 G words fit)
    float* d_w = e->d_pi + G;
    launch_root_stats(e->S, e->ply & 1, d_n, d_w, e->st);
    std::vector<uint32_t> host(2 * G);
    HIPCHK(e, hipMemcpyAsync(host.data(), e->d_pi, 8 * G, hipMemcpyDeviceToHost, e->st));
    if (sync_and_check(e, "root_stats")) return OMOK_ERR_HIP;
    memcpy(n, host.data(), 4 * G);
    memcpy(w, host.data() + G, 4 * G);
    return OMOK_OK;
}

extern "C" int omok_tree_dump(omok_engine* e, int32_t game, int32_t side, int32_t* ints, float* floats, int32_t cap_nodes) {
    if (!e || !ints || !floats || game < 0 || game >= e->cfg.games || (side != 0 && side != 1)) return OMOK_ERR_INVALID;
    ENTER(e);
    const size_t t = (size_t)side * e->cfg.games + game;
    launch_materialise(e->n, e->S, (int)t, 1, e->st); // (raw rows of lazy rounds: the caller sees has_policy = 1 and the eager kernels' bits; changes no later result)
    TreeState ts;
    HIPCHK(e, hipMemcpyAsync(&ts, e->S.ts + t, sizeof(ts), hipMemcpyDeviceToHost, e->st));
    if (sync_and_check(e, "tree_dump")) return OMOK_ERR_HIP;
    const int nn = (int)ts.n_nodes, nt = (int)ts.n_tables;
    if (nn > cap_nodes) return -nn;
    const size_t rp = (size_t)e->rowp, nw2 = 2 * (size_t)e->nw;
    std::vector<NodeHdr> hdr((size_t)nn);
    std::vector<uint64_t> board((size_t)nn * nw2);
    std::vector<float> pol((size_t)nn * rp), cw((size_t)nt * rp);
    std::vector<uint32_t> cn((size_t)nt * rp);
    std::vector<uint8_t> co((size_t)nt * rp);
    const size_t tn = t * (size_t)e->S.stride_nodes, tt = t * (size_t)e->S.stride_tables;
    hipMemcpyAsync(hdr.data(), e->S.hdr + tn, sizeof(NodeHdr) * nn, hipMemcpyDeviceToHost, e->st);
    hipMemcpyAsync(board.data(), e->S.board + tn * nw2, 8 * nw2 * nn, hipMemcpyDeviceToHost, e->st);
    hipMemcpyAsync(pol.data(), e->S.policy + tn * rp, 4 * rp * nn, hipMemcpyDeviceToHost, e->st);
    if (nt) {
        hipMemcpyAsync(cn.data(), e->S.tcn + tt * rp, 4 * rp * nt, hipMemcpyDeviceToHost, e->st);
        hipMemcpyAsync(cw.data(), e->S.tcw + tt * rp, 4 * rp * nt, hipMemcpyDeviceToHost, e->st);
        hipMemcpyAsync(co.data(), e->S.tcorder + tt * rp, rp * nt, hipMemcpyDeviceToHost, e->st);
    }
    if (sync_and_check(e, "tree_dump")) return OMOK_ERR_HIP;
    const int hw = e->hw;
    for (int i = 0; i < nn; ++i) {
        const NodeHdr& h = hdr[i];
        int32_t* o = ints + (size_t)i * 8;
        float* f = floats + (size_t)i * (1 + hw);
        uint32_t n = ts.root_n;
        float w = ts.root_w;
        int order = -1;
        if (i != 0) {
            const size_t slot = (size_t)hdr[h.parent].table * rp + h.action;
            n = cn[slot]; w = cw[slot]; order = co[slot];
        }
        o[0] = h.parent == NONE16 ? -1 : h.parent;
        o[1] = h.action == NONE8 ? -1 : h.action;
        o[2] = h.status; o[3] = h.turn; o[4] = h.legal; o[5] = h.nch; o[6] = (int32_t)n;
        o[7] = (order & 0xffff) | ((int32_t)h.has_policy << 16);
        f[0] = w;
        for (int a = 0; a < hw; ++a) {
            float v;
            if (h.has_policy) v = pol[(size_t)i * rp + a];
            else {
                const bool occ = ((board[(size_t)i * nw2 + a / 64] | board[(size_t)i * nw2 + e->nw + a / 64]) >> (a % 64)) & 1ULL;
                v = (occ || h.legal == 0) ? 0.0f : 1.0f / (float)h.legal;
            }
            f[1 + a] = v;
        }
    }
    return nn;
}

extern "C" int omok_replay_game(omok_engine* e, int32_t game, uint8_t* boards, uint8_t* turns, float* pi, float* z, int32_t cap_plies) {
    if (!e || game < 0 || game >= e->cfg.games) return OMOK_ERR_INVALID;
    ENTER(e);
    GameState gs;
    HIPCHK(e, hipMemcpyAsync(&gs, e->S.gs + game, sizeof(gs), hipMemcpyDeviceToHost, e->st));
    if (sync_and_check(e, "replay_game")) return OMOK_ERR_HIP;
    const int plies = gs.rp_len < e->hw ? gs.rp_len : e->hw;
    const int n = plies < cap_plies ? plies : cap_plies;
    if (n <= 0) return plies;
    const size_t rp = (size_t)e->rowp, nw2 = 2 * (size_t)e->nw, hw = (size_t)e->hw;
    std::vector<uint64_t> b((size_t)n * nw2);
    std::vector<float> ppi((size_t)n * rp);
    const size_t rec = (size_t)game * hw;
    hipMemcpyAsync(b.data(), e->S.rp_board + rec * nw2, 8 * nw2 * n, hipMemcpyDeviceToHost, e->st);
    hipMemcpyAsync(ppi.data(), e->S.rp_pi + rec * rp, 4 * rp * n, hipMemcpyDeviceToHost, e->st);
    if (turns) hipMemcpyAsync(turns, e->S.rp_turn + rec, (size_t)n, hipMemcpyDeviceToHost, e->st);
    if (z) hipMemcpyAsync(z, e->S.rp_z + rec, 4 * (size_t)n, hipMemcpyDeviceToHost, e->st);
    if (sync_and_check(e, "replay_game")) return OMOK_ERR_HIP;
    for (int p = 0; p < n; ++p)
        for (size_t a = 0; a < hw; ++a) {
            if (boards) {
                const bool bl = (b[(size_t)p * nw2 + a / 64] >> (a % 64)) & 1ULL, wh = (b[(size_t)p * nw2 + e->nw + a / 64] >> (a % 64)) & 1ULL;
                boards[(size_t)p * hw + a] = bl ? 1 : (wh ? 2 : 0);
            }
            if (pi) pi[(size_t)p * hw + a] = ppi[(size_t)p * rp + a];
        }
    return plies;
}

extern "C" int32_t omok_replay_record_bytes(const omok_engine* e) {
    if (!e) return OMOK_ERR_INVALID;
    return (e->hw + 1 + 3) / 4 * 4 + 4 * e->hw + 4;
}

extern "C" int64_t omok_replay_pack_dev(omok_engine* e, void* dst_dev, int64_t cap_records) {
    if (!e || !dst_dev || cap_records < 0) return OMOK_ERR_INVALID;
    if (hipSetDevice(e->cfg.device) != hipSuccess) return OMOK_ERR_HIP;
    launch_replay_offsets(e->n, e->S, 1, e->d_aug_offsets, e->st);
    launch_replay_pack(e->n, e->S, e->d_aug_offsets, (uint8_t*)dst_dev, cap_records, e->st);
    long long total = 0;
    if (hipMemcpyAsync(&total, e->d_aug_offsets + e->cfg.games, 8, hipMemcpyDeviceToHost, e->st) != hipSuccess) return OMOK_ERR_HIP;
    if (sync_and_check(e, "replay_pack")) return OMOK_ERR_HIP;
    return total;
}

// ---- replay post-processing (src/trainer.rs:207-324) ----------------------------------------------------------------
extern "C" int64_t omok_replay_augment_dev(omok_engine* e, void* dst_dev, int64_t cap_records) {
    if (!e || !dst_dev || cap_records < 0) return OMOK_ERR_INVALID;
    if (hipSetDevice(e->cfg.device) != hipSuccess) return OMOK_ERR_HIP;
    e->prof.begin(PC_PLY, e->st); // (timed only under omok_set_profiling: tools/selfplay_slots_timing.py)
    launch_replay_offsets(e->n, e->S, 6, e->d_aug_offsets, e->st);
    launch_replay_augment(e->n, e->S, e->d_aug_offsets, 0, e->cfg.games, 0, (uint8_t*)dst_dev, cap_records, e->st);
    e->prof.end(e->st);
    long long total = 0;
    if (hipMemcpyAsync(&total, e->d_aug_offsets + e->cfg.games, 8, hipMemcpyDeviceToHost, e->st) != hipSuccess) return OMOK_ERR_HIP;
    if (sync_and_check(e, "replay_augment")) return OMOK_ERR_HIP;
    return total;
}

// the same on caller-held packed records (slots mode, records gathered from other ranks): touches no engine state, needs no net
extern "C" int64_t omok_replay_augment_records_dev(omok_engine* e, const void* records_dev, int64_t n_records, const int64_t* game_offsets,
                                                   const int32_t* game_lengths, int32_t games, void* dst_dev, int64_t cap_records) {
    if (!e) return OMOK_ERR_INVALID;
    if (games < 1) return fail(e, OMOK_ERR_INVALID, "games %d < 1", games);
    if (!records_dev || !game_offsets || !game_lengths || !dst_dev) return fail(e, OMOK_ERR_INVALID, "replay_augment_records: NULL pointer");
    if (n_records < 0 || cap_records < 0) return fail(e, OMOK_ERR_INVALID, "n_records %lld / cap_records %lld < 0", (long long)n_records, (long long)cap_records);
    if (((uintptr_t)records_dev | (uintptr_t)dst_dev) & 3) return fail(e, OMOK_ERR_INVALID, "records_dev and dst_dev must be 4-byte aligned");
    // first [m + 1] = exclusive scan of the m non-empty games' lengths, then span [m] (k_replay_augment_records); destination bases = scan of 6 L
    std::vector<long long> first(1, 0);
    std::vector<AugSpan> span;
    long long total = 0;
    for (int i = 0; i < games; ++i) {
        const long long L = game_lengths[i], off = game_offsets[i];
        if (L < 0 || L > e->hw)
            return fail(e, OMOK_ERR_INVALID, "game %d: length %lld outside [0, %d]%s", i, L, e->hw, L < 0 ? " (a game that never finished?)" : "");
        if (L == 0) continue;
        if (off < 0 || off > n_records - L)
            return fail(e, OMOK_ERR_INVALID, "game %d: offset %lld + length %lld outside [0, n_records = %lld]", i, off, L, (long long)n_records);
        span.push_back({off, 6 * total});
        total += L;
        first.push_back(total);
    }
    if (total == 0) return 0;
    ENTER(e);
    const size_t m = span.size(), first_bytes = (m + 1) * sizeof(long long);
    Scratch sc;
    uint8_t* d = sc.get<uint8_t>(first_bytes + m * sizeof(AugSpan));
    if (!d) return fail(e, OMOK_ERR_HIP, "replay_augment_records: device allocation failed");
    hipMemcpyAsync(d, first.data(), first_bytes, hipMemcpyHostToDevice, e->st);
    hipMemcpyAsync(d + first_bytes, span.data(), m * sizeof(AugSpan), hipMemcpyHostToDevice, e->st);
    e->prof.begin(PC_PLY, e->st); // (timed only under omok_set_profiling: tools/selfplay_slots_timing.py)
    launch_replay_augment_records(e->n, (const uint8_t*)records_dev, (const long long*)d, (const AugSpan*)(d + first_bytes), (int)m, total,
                                  (uint8_t*)dst_dev, cap_records, e->st);
    e->prof.end(e->st);
    return sync_and_check(e, "replay_augment_records") ? OMOK_ERR_HIP : 6 * total;
}

extern "C" int omok_replay_augmented_game(omok_engine* e, int32_t game, uint8_t* boards, uint8_t* turns, float* pi, float* z, int32_t cap_records) {
    if (!e || game < 0 || game >= e->cfg.games || cap_records < 0) return OMOK_ERR_INVALID;
    HIPCHK(e, hipSetDevice(e->cfg.device));
    const size_t hw = (size_t)e->hw, brd = (hw + 1 + 3) / 4 * 4, rec = brd + 4 * hw + 4, max_rec = 6 * hw;
    if (!e->d_aug_scratch && dalloc(e, &e->d_aug_scratch, max_rec * rec)) return OMOK_ERR_HIP;
    long long off[2] = {0, 0};
    launch_replay_offsets(e->n, e->S, 6, e->d_aug_offsets, e->st);
    HIPCHK(e, hipMemcpyAsync(off, e->d_aug_offsets + game, 16, hipMemcpyDeviceToHost, e->st));
    if (sync_and_check(e, "replay_augmented_game")) return OMOK_ERR_HIP;
    const int total = (int)(off[1] - off[0]);
    const int n = total < cap_records ? total : cap_records;
    if (n <= 0) return total;
    launch_replay_augment(e->n, e->S, e->d_aug_offsets, game, 1, off[0], e->d_aug_scratch, (long long)max_rec, e->st);
    std::vector<uint8_t> host((size_t)total * rec);
    HIPCHK(e, hipMemcpyAsync(host.data(), e->d_aug_scratch, host.size(), hipMemcpyDeviceToHost, e->st));
    if (sync_and_check(e, "replay_augmented_game")) return OMOK_ERR_HIP;
    for (int i = 0; i < n; ++i) {
        const uint8_t* r = host.data() + (size_t)i * rec;
        if (boards) memcpy(boards + (size_t)i * hw, r, hw);
        if (turns) turns[i] = r[hw];
        if (pi) memcpy(pi + (size_t)i * hw, r + brd, 4 * hw);
        if (z) memcpy(z + i, r + brd + 4 * hw, 4);
    }
    return total;
}

// fc0 operand rows (the trunk's output as fc0 reads it) of the LAST forward: `rows` rows from `first_row`, omok_operand_row_bytes each
extern "C" int64_t omok_operand_row_bytes(const omok_engine* e) { return e && e->net.mode != OMOK_NET_F32 ? (int64_t)e->net.row_u4 * 16 : OMOK_ERR_INVALID; }
extern "C" int omok_debug_operand_rows(omok_engine* e, int32_t first_row, int32_t rows, void* out) {
    if (!e || !out || first_row < 0 || rows < 0 || first_row + rows > e->net.max_b || e->net.mode == OMOK_NET_F32) return OMOK_ERR_INVALID;
    ENTER(e);
    HIPCHK(e, hipMemcpyAsync(out, (const char*)e->net.a_fc0 + (size_t)first_row * e->net.row_u4 * 16, (size_t)rows * e->net.row_u4 * 16, hipMemcpyDeviceToHost, e->st));
    return sync_and_check(e, "debug_operand_rows") ? OMOK_ERR_HIP : OMOK_OK;
}

extern "C" int omok_debug_set_base_cache(omok_engine* e, int32_t enabled) {
    if (!e) return OMOK_ERR_INVALID;
    e->net.base_cache = enabled != 0;
    net_invalidate_sibling_cache(e->net);
    if (e->net2) { // (a match episode's second net, if it is loaded: the same switch)
        e->net2->base_cache = enabled != 0;
        net_invalidate_sibling_cache(*e->net2);
    }
    return OMOK_OK;
}

extern "C" int omok_debug_set_lazy_policy(omok_engine* e, int32_t enabled) {
    if (!e) return OMOK_ERR_INVALID;
    e->lazy_policy = enabled != 0; // (raw rows that exist stay valid: every reader handles them whatever the switch says)
    return OMOK_OK;
}
extern "C" int omok_debug_lazy_policy_stats(omok_engine* e, uint64_t* out) {
    if (!e || !out) return OMOK_ERR_INVALID;
    ENTER(e);
    uint32_t c[2] = {0, 0};
    HIPCHK(e, hipMemcpyAsync(c, e->d_lazy, sizeof(c), hipMemcpyDeviceToHost, e->st));
    if (sync_and_check(e, "lazy_policy_stats")) return OMOK_ERR_HIP;
    out[0] = c[0];
    out[1] = c[1];
    return OMOK_OK;
}

extern "C" int omok_debug_set_window_rects(omok_engine* e, int32_t enabled) {
    if (!e) return OMOK_ERR_INVALID;
    e->net.win_rects = enabled != 0;
    return OMOK_OK;
}

extern "C" int omok_debug_set_children_kernel(omok_engine* e, int32_t which) {
    if (!e) return OMOK_ERR_INVALID;
    if (which != 1 && which != 2) return fail(e, OMOK_ERR_INVALID, "children kernel %d (1 = k_sib_children, 2 = k_sib_children2)", which);
    if (which == 1 && e->net.mode != OMOK_NET_F32 && e->net.diff_fp6)  // (the mixed format's difference rows are written by k_sib_children2 only: the switch would silently do nothing)
        return fail(e, OMOK_ERR_STATE, "omok_debug_set_children_kernel(1): the engine runs the mixed operand format, whose difference path exists in k_sib_children2 only "
                                       "(create the engine with OMOK_NET_F16X3_FP6 or _F16 to compare the two kernels)");
    e->net.sib_v2 = which == 2;
    net_invalidate_sibling_cache(e->net); // (the two kernels read different base-slot layouts)
    return OMOK_OK;
}

// what the LAST forward of net 1 decided: the host's choices (Net::plan_*) + the counters k_group / bin_prefix_role left in d_gcnt (a sibling round's stay there until the
// next round is generated)
extern "C" int omok_debug_last_plan(omok_engine* e, int32_t* out, int32_t cap) {
    if (!e || !out || cap < 0) return OMOK_ERR_INVALID;
    ENTER(e);
    const Net& net = e->net;
    int32_t plan[OMOK_PLAN_INTS] = {};
    plan[0] = net.plan_path; plan[1] = net.plan_rows; plan[2] = net.plan_nsplit; plan[3] = net.plan_tsplit;
    plan[12] = net.mode == OMOK_NET_F32 ? -1 : net.diff_fp6 ? FC0_MIXED : net.fc0_fmt;
    plan[13] = net.n_cu;
    plan[14] = 2 * net.hw;
    if (sync_and_check(e, "debug_last_plan")) return OMOK_ERR_HIP;
    if ((net.plan_path == 1 || net.plan_path == 2) && net.d_gcnt) {
        int32_t c[NET_GCNT_HEAD_INTS];
        HIPCHK(e, hipMemcpy(c, net.d_gcnt, sizeof(c), hipMemcpyDeviceToHost));
        plan[4] = c[NET_GCNT_RUNS]; plan[5] = c[NET_GCNT_SINGLES]; plan[6] = c[NET_GCNT_ROWS_IN_RUNS];
        if (net.plan_path == 2) {
            plan[7] = c[NET_GCNT_FULL_EVALS]; plan[8] = c[NET_GCNT_WIN_TILES]; plan[9] = c[NET_GCNT_SPLIT_TILE0]; plan[10] = c[NET_GCNT_WIN_WAYS];
            plan[11] = c[NET_GCNT_FULL_WAYS];
        }
    }
    const int n = cap < OMOK_PLAN_INTS ? cap : OMOK_PLAN_INTS;
    for (int i = 0; i < n; ++i) out[i] = plan[i];
    return n;
}

extern "C" int omok_get_stats(omok_engine* e, double* stats) {
    if (!e || !stats) return OMOK_ERR_INVALID;
    HIPCHK(e, hipSetDevice(e->cfg.device));
    if (sync_and_check(e, "get_stats")) return OMOK_ERR_HIP;
    e->prof.resolve();
    unsigned long long ev = 0, by = 0;
    HIPCHK(e, hipMemcpy(&ev, e->d_evals, 8, hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemcpy(&by, e->S.d_bytes, 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < OMOK_STAT_COUNT; ++i) stats[i] = 0.0;
    stats[OMOK_STAT_SIMS] = e->sims;
    stats[OMOK_STAT_EVALS] = e->evals + (double)ev;
    stats[OMOK_STAT_PLY_GAMES] = e->ply_games;
    stats[OMOK_STAT_FINISHED] = e->finished;
    stats[OMOK_STAT_MS_TREE] = e->prof.total_ms(PC_ROUND) + e->prof.total_ms(PC_TREE_OTHER);
    stats[OMOK_STAT_MS_TRUNK] = e->prof.total_ms(PC_TRUNK);
    stats[OMOK_STAT_MS_FC0] = e->prof.total_ms(PC_FC0);
    stats[OMOK_STAT_MS_TAIL] = e->prof.total_ms(PC_TAIL);
    stats[OMOK_STAT_MS_PLY] = e->prof.total_ms(PC_PLY);
    stats[OMOK_STAT_MS_TRAIN_APPLY] = e->prof.total_ms(PC_TRAIN_APPLY);
    stats[OMOK_STAT_FC0_LAUNCHES] = e->prof.total_launches(PC_FC0);
    stats[OMOK_STAT_FC0_ROWS] = e->evals + (double)ev;
    stats[OMOK_STAT_TREE_BYTES] = (double)by;
    stats[OMOK_STAT_ROUND_LAUNCHES] = e->prof.total_launches(PC_ROUND);
    stats[OMOK_STAT_MS_ROUND] = e->prof.total_ms(PC_ROUND);
    stats[OMOK_STAT_PEAK_NODES] = (double)e->peak_nodes;
    stats[OMOK_STAT_PEAK_TABLES] = (double)e->peak_tables;
    stats[OMOK_STAT_FC0_FORMAT] = e->net.mode == OMOK_NET_F32 ? -1.0 : (e->net.diff_fp6 ? (double)FC0_MIXED : (double)e->net.fc0_fmt);
    stats[OMOK_STAT_PROBE_ROWS] = e->net.probe[6] != 0.0f ? (double)e->net.probe[0] : 0.0;
    stats[OMOK_STAT_PROBE_DP_FP6] = e->net.probe[1];
    stats[OMOK_STAT_PROBE_DV_FP6] = e->net.probe[2];
    stats[OMOK_STAT_PROBE_DP_F16] = e->net.probe[3];
    stats[OMOK_STAT_PROBE_DV_F16] = e->net.probe[4];
    stats[OMOK_STAT_PROBE_LIMIT] = NET_PROBE_LIMIT;
    stats[OMOK_STAT_PROBE_LOGIT_MAX] = e->net.probe[5];
    stats[OMOK_STAT_CHILDREN2_LAUNCHES] = e->net.children_launches[0];
    stats[OMOK_STAT_CHILDREN1_LAUNCHES] = e->net.children_launches[1];
    stats[OMOK_STAT_PROBE_DLOGIT_FP6] = e->net.probe[7];
    stats[OMOK_STAT_PROBE_DLOGIT_F16] = e->net.probe[8];
    stats[OMOK_STAT_PROBE_ROUND_ROWS] = e->net.probe[9];
    for (int i = 0; i < 9; ++i) stats[OMOK_STAT_PROBE_ROUND_FP6 + i] = e->net.probe[10 + i];
    stats[OMOK_STAT_PROBE_LOGIT_LIMIT] = NET_PROBE_LOGIT_LIMIT;
    stats[OMOK_STAT_PROBE_OUTSIDE] = (double)e->net.probe_outside;
    if (e->net.d_work) { // executed-work counters of the sibling rounds (device side: k_group, bin_prefix_role)
        unsigned long long w[NET_WORK_COUNT];
        if (hipMemcpy(w, e->net.d_work, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess) return OMOK_ERR_HIP;
        for (int i = 0; i < 10; ++i) stats[OMOK_STAT_WORK_DIFF_RUNS + i] = (double)w[i];
    }
    return OMOK_OK;
}

extern "C" int omok_reset_stats(omok_engine* e) {
    ENTER(e);
    if (sync_and_check(e, "reset_stats")) return OMOK_ERR_HIP;
    e->prof.resolve();
    for (int i = 0; i < PC_COUNT; ++i) { e->prof.ms[i] = 0; e->prof.launches[i] = 0; e->prof.ms_s[i] = 0; e->prof.launches_s[i] = 0; }
    e->prof.rounds_seen = e->prof.rounds_timed = 0;
    e->sims = e->evals = e->ply_games = e->finished = 0;
    e->peak_nodes = e->peak_tables = 0;
    e->net.children_launches[0] = e->net.children_launches[1] = 0.0;
    hipMemset(e->d_evals, 0, 16);
    hipMemset(e->S.d_bytes, 0, 16);
    if (e->net.d_work) hipMemset(e->net.d_work, 0, sizeof(unsigned long long) * NET_WORK_COUNT);
    if (e->d_mevals) hipMemset(e->d_mevals, 0, 16);
    return OMOK_OK;
}

extern "C" int omok_set_profiling(omok_engine* e, int32_t enabled) {
    if (!e) return OMOK_ERR_INVALID;
    if (enabled < 0) return OMOK_ERR_INVALID;
    e->prof.resolve();
    e->prof.enabled = enabled != 0;
    e->prof.every = enabled > 1 ? enabled : 1;
    return OMOK_OK;
}
