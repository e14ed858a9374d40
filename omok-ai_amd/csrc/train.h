// train.h — state of the native training step (AgentModel::train, alpha-zero/src/agent_model.rs:136-168) shared by engine.cpp and train_kernels.hip
#pragma once
#include "net.h"

namespace omok {

constexpr int TRAIN_MAX_BATCH = 4096;       // omok_train_begin's largest max_batch (the batch draw keeps its sorted list in LDS)
constexpr float TRAIN_LEARNING_RATE = 0.01f; // AgentModel::LEARNING_RATE (agent_model.rs:24)
constexpr float TRAIN_RHO = 0.95f;           // tensorflow-rust AdadeltaOptimizer defaults (ApplyAdadelta)
constexpr float TRAIN_EPSILON = 1e-8f;
constexpr float TRAIN_SLOPE = 0.2f;          // LeakyReLU alpha of the whole graph (network.rs)
constexpr size_t TRAIN_WS_FLOATS = (size_t)4 << 20; // split-K partial slab: splits x M x N never exceeds it (train_kernels.hip: plan of launch_gemm)

struct Train {
    int n = 0, hw = 0, max_b = 0;
    int rec = 0, brd = 0;            // bytes of a replay record, offset of its pi
    int64_t off[NET_TENSORS + 1] = {}; // tensor i's slice of the slabs below: [off[i], off[i + 1])
    float* acc = nullptr;            // Adadelta accumulators (zero-initialised), [off[31]]
    float* accu = nullptr;           // ... accumulated updates
    float* grad = nullptr;           // gradients of the last step
    bool has_grad = false;
    int pending = 0;                 // batch of an omok_train_backward whose omok_train_apply is still due (its batch buffers are intact), 0 = none
    // the step's batch
    int64_t* idx = nullptr;          // [max_b] record indices (uploaded, or drawn on the device)
    float *x0 = nullptr, *pi = nullptr, *z = nullptr; // encode_nn_input(Player) [B][3 HW], targets [B][HW], [B]
    // saved activations, rows = B * HW pixels (NHWC), all AFTER their LeakyReLU: x > 0 <=> pre-activation > 0
    float* a0 = nullptr;             // conv_in [rows][128]
    float *h[3] = {}, *d[3] = {}, *g[3] = {}, *x[3] = {}; // per block: 1x1 down [rows][32], depthwise, pointwise, block output [rows][128]
    float *h0 = nullptr, *h1 = nullptr; // fc0 / fc1 [B][512]
    float *logits = nullptr, *vpre = nullptr; // [B][HW], [B]
    // gradient scratch
    float *dx[2] = {}, *dm[2] = {};  // [rows][128] x 2, [rows][32] x 2
    float *dh0 = nullptr, *dh1 = nullptr, *dlogits = nullptr, *dvpre = nullptr;
    float* ws = nullptr;             // split-K partials [TRAIN_WS_FLOATS]
    float* colpart = nullptr;        // partial column sums (bias gradients, depthwise taps)
    float* loss_rows = nullptr;      // [B][2] per-sample v / p loss
    float* losses = nullptr;         // [0..2] v_loss, p_loss, loss of the last evaluation; [4..6] their running sums (omok_train_run)
    size_t bytes = 0;
};

// Allocates everything for batches of up to max_b records of net's board size (accumulators zeroed); returns bytes, 0 on failure (nothing is kept)
size_t train_alloc(Train& T, const Net& net, int max_b);
void train_free(Train& T);
// Batch draw of step `step` under `key` (purpose RNG_TRAIN_BATCH): k = min(batch, R) distinct record indices in draw order -> T.idx
void train_draw(Train& T, int64_t n_records, int k, uint64_t key, int step, hipStream_t st);
// One AgentModel::train on the k records T.idx names: forward + losses; update: backward, Adadelta on net.w[] in place, then forward + losses again.
// T.losses[0..2] = v_loss, p_loss, loss; accumulate: also added to T.losses[4..6].
void train_step(Train& T, Net& net, const void* records_dev, int k, bool update, bool accumulate, hipStream_t st);
// The same step in two halves (omok_train_backward / omok_train_apply; agent_model.rs:136-168, trainer.rs:329-357 for data-parallel hosts).
// train_backward: assemble, forward, losses with gradients, backward -> T.grad; writes no weight and no accumulator.
void train_backward(Train& T, const Net& net, const void* records_dev, int k, hipStream_t st);
// train_update: ApplyAdadelta on net.w[] with T.grad (grads_dev NULL), or with the rank-order average of grads_dev [ranks][T.off[31]], which it also
// leaves in T.grad.  train_evaluate: forward + the three losses on the batch train_backward assembled -> T.losses[0..2]
// (accumulate: also added to T.losses[4..6]).
void train_update(Train& T, Net& net, const float* grads_dev, int ranks, hipStream_t st);
void train_evaluate(Train& T, const Net& net, int k, bool accumulate, hipStream_t st);

} // namespace omok
