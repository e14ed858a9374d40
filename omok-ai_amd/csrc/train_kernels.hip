// train_kernels.hip — the training step on the device: AgentModel::train (alpha-zero/src/agent_model.rs:136-168) in plain fp32.
//
// Restates, on the 31 raw tensors of Net::w[] (reference order, conv kernels HWIO, fc [in, out]):
//   graph      alpha-zero/src/network.rs:51-262, network-utils/src/lib.rs:95-262 (conv2d / depthwise / BiasAdd), :386-461 (bottleneck block)
//   losses     network.rs:249-253 (softmax cross entropy with labels pi), agent_model.rs:57-73 (v_loss, loss)
//   optimizer  agent_model.rs:24,75-82: AdadeltaOptimizer, lr 0.01, rho 0.95, eps 1e-8 (TensorFlow ApplyAdadelta)
//   batches    src/trainer.rs:329-350 (choose_multiple), alpha-zero/src/encoder.rs:10-68 (inputs and targets)
// Activations are NHWC rows (row = sample * HW + pixel), so every 1x1 convolution and every fully connected layer is one GEMM; fc0 reads the last
// block's rows as [B][HW * 128].  Every buffer keeps the value AFTER its LeakyReLU: the slope of the backward pass needs only the sign.
// Determinism: no floating-point atomics; split-K partials, bias sums, tap sums and loss means are added in a fixed order that depends on the
// shapes only, so the same step on the same inputs leaves the same bits.
#include "train.h"

#include <algorithm>

namespace omok {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- GEMM: C[M][N] = epilogue(op(A)[M][K] . op(B)[K][N]) on v_mfma_f32_32x32x2_f32 ------------------------------------------------------
// AT = false: A(m, k) = A[m * lda + k]; true: A[k * lda + m] (weight gradients: X^T . dY).  BT = false: B(k, n) = B[k * ldb + n]; true: B[n * ldb + k]
// (data gradients: dY . W^T).  A workgroup of 4 waves owns a 64 x 64 tile (one 32 x 32 accumulator per wave) and the K range of its blockIdx.z.
// splits == 1: the epilogue runs here; else the raw sums go to ws[z][M][N] and k_gemm_reduce adds them in z order.
struct GemmArgs {
    const float *A, *B;
    float* C;
    const float* bias; // [N] or NULL
    const float* R;    // added, laid out like C, or NULL (may be C itself)
    const float* P;    // act 2: the saved activation the slope is taken from, laid out like C
    float* ws;
    int M, N, K, kchunk, splits, act; // act 0 none, 1 LeakyReLU, 2 times LeakyReLU'(P)
    long long lda, ldb, ldc;
};

__device__ inline float gemm_epilogue(const GemmArgs& g, float v, int m, int n) {
    const size_t o = (size_t)m * g.ldc + n;
    if (g.bias) v += g.bias[n];
    if (g.R) v += g.R[o];
    if (g.act == 1) v = v > 0.0f ? v : TRAIN_SLOPE * v;
    else if (g.act == 2) v *= g.P[o] > 0.0f ? 1.0f : TRAIN_SLOPE; // 0.2 at exactly 0, as torch and TensorFlow
    return v;
}

template <bool AT, bool BT>
__global__ __launch_bounds__(256) void k_gemm(GemmArgs g) {
    __shared__ float As[16][65], Bs[16][65];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w & 1, wn = w >> 1;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int k_begin = blockIdx.z * g.kchunk, k_end = min(g.K, k_begin + g.kchunk);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int k0 = k_begin; k0 < k_end; k0 += 16) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            int m, k;
            if (AT) { m = tid & 63; k = (tid >> 6) + 4 * p; } else { k = tid & 15; m = (tid >> 4) + 16 * p; }
            const int gm = m0 + m, gka = k0 + k;
            float v = 0.0f;
            if (gm < g.M && gka < k_end) v = AT ? g.A[(size_t)gka * g.lda + gm] : g.A[(size_t)gm * g.lda + gka];
            As[k][m] = v;
            int n;
            if (BT) { k = tid & 15; n = (tid >> 4) + 16 * p; } else { n = tid & 63; k = (tid >> 6) + 4 * p; }
            const int gn = n0 + n, gkb = k0 + k;
            v = 0.0f;
            if (gn < g.N && gkb < k_end) v = BT ? g.B[(size_t)gn * g.ldb + gkb] : g.B[(size_t)gkb * g.ldb + gn];
            Bs[k][n] = v;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 8; ++s) { // lane l: A[row l & 31][k = l >> 5], B[k = l >> 5][col l & 31]
            const float a = As[2 * s + (lane >> 5)][wm * 32 + (lane & 31)];
            const float b = Bs[2 * s + (lane >> 5)][wn * 32 + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    const int gn = n0 + wn * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) { // C/D: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
        const int gm = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (gm < g.M && gn < g.N) {
            if (g.splits > 1) g.ws[((size_t)blockIdx.z * g.M + gm) * g.N + gn] = acc[r];
            else g.C[(size_t)gm * g.ldc + gn] = gemm_epilogue(g, acc[r], gm, gn);
        }
    }
}

__global__ __launch_bounds__(256) void k_gemm_reduce(GemmArgs g) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, mn = (size_t)g.M * g.N;
    if (i >= mn) return;
    float v = 0.0f;
    for (int s = 0; s < g.splits; ++s) v += g.ws[(size_t)s * mn + i];
    const int m = (int)(i / g.N), n = (int)(i % g.N);
    g.C[(size_t)m * g.ldc + n] = gemm_epilogue(g, v, m, n);
}

enum { GEMM_NN = 0, GEMM_NT = 1, GEMM_TN = 2 };

static void launch_gemm(const Train& T, hipStream_t st, int form, const float* A, long long lda, const float* B, long long ldb, float* C, long long ldc,
                        int M, int N, int K, const float* bias = nullptr, const float* R = nullptr, int act = 0, const float* P = nullptr) {
    GemmArgs g{A, B, C, bias, R, P, T.ws, M, N, K, 0, 1, act, lda, ldb, ldc};
    const int tm = (M + 63) / 64, tn = (N + 63) / 64, tiles = tm * tn;
    g.kchunk = (K + 15) / 16 * 16;
    if (tiles < 512) { // too few tiles for 256 CUs: split K.  splits * tiles <= 1024 and M N <= 4096 tiles, so the partials fit TRAIN_WS_FLOATS
        const int want = std::max(1, std::min(1024 / tiles, (K + 31) / 32));
        g.kchunk = ((K + want - 1) / want + 15) / 16 * 16;
        g.splits = (K + g.kchunk - 1) / g.kchunk;
    }
    const dim3 grid(tn, tm, g.splits);
    if (form == GEMM_NN) k_gemm<false, false><<<grid, 256, 0, st>>>(g);
    else if (form == GEMM_NT) k_gemm<false, true><<<grid, 256, 0, st>>>(g);
    else k_gemm<true, false><<<grid, 256, 0, st>>>(g);
    if (g.splits > 1) k_gemm_reduce<<<(unsigned)(((size_t)M * N + 255) / 256), 256, 0, st>>>(g);
}

// ---- column sums (bias gradients): out[n] = sum_m Y[m][n], chunks of 64 rows, then the chunks in order -------------------------------
__global__ __launch_bounds__(256) void k_colsum_part(const float* __restrict__ Y, int M, int N, float* __restrict__ part) {
    const int n = blockIdx.y * 256 + threadIdx.x;
    if (n >= N) return;
    const int r0 = blockIdx.x * 64, r1 = min(M, r0 + 64);
    float s = 0.0f;
    for (int r = r0; r < r1; ++r) s += Y[(size_t)r * N + n];
    part[(size_t)blockIdx.x * N + n] = s;
}
__global__ __launch_bounds__(256) void k_colsum_final(const float* __restrict__ part, int chunks, int N, float* __restrict__ out) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float s = 0.0f;
    for (int c = 0; c < chunks; ++c) s += part[(size_t)c * N + n];
    out[n] = s;
}
static void launch_colsum(const Train& T, hipStream_t st, const float* Y, int M, int N, float* out) {
    const int chunks = (M + 63) / 64;
    k_colsum_part<<<dim3(chunks, (N + 255) / 256), 256, 0, st>>>(Y, M, N, T.colpart);
    k_colsum_final<<<(N + 255) / 256, 256, 0, st>>>(T.colpart, chunks, N, out);
}

// ---- depthwise 3x3 SAME, no bias (network-utils/src/lib.rs:172-262): taps [ky][kx][c] ------------------------------------------------
// forward: d[y][x][c] = sum_t h[y + ky - 1][x + kx - 1][c] w[t][c];  data gradient: dh[y][x][c] = sum_t dd[y - ky + 1][x - kx + 1][c] w[t][c], then
// times LeakyReLU'(h)
template <bool BACKWARD>
__global__ __launch_bounds__(256) void k_depthwise(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ slope_of,
                                                   float* __restrict__ out, int n, int rows) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)rows * NM) return;
    const int c = (int)(i % NM), row = (int)(i / NM), hw = n * n;
    const int pix = row % hw, y = pix / n, x = pix % n;
    const size_t base = (size_t)(row - pix) * NM + c;
    float s = 0.0f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int yy = BACKWARD ? y - ky + 1 : y + ky - 1, xx = BACKWARD ? x - kx + 1 : x + kx - 1;
            if (yy >= 0 && yy < n && xx >= 0 && xx < n) s += in[base + (size_t)(yy * n + xx) * NM] * w[(ky * 3 + kx) * NM + c];
        }
    if (BACKWARD) s *= slope_of[i] > 0.0f ? 1.0f : TRAIN_SLOPE;
    out[i] = s;
}
// tap gradient: dw[t][c] = sum over samples, pixels of h[y + ky - 1][x + kx - 1][c] dd[y][x][c]: one workgroup per sample, then the samples in order
__global__ __launch_bounds__(288) void k_depthwise_taps(const float* __restrict__ h, const float* __restrict__ dd, int n, float* __restrict__ part) {
    const int t = threadIdx.x / NM, c = threadIdx.x % NM, ky = t / 3, kx = t % 3, hw = n * n;
    const size_t base = (size_t)blockIdx.x * hw * NM + c;
    float s = 0.0f;
    for (int y = 0; y < n; ++y) {
        const int yy = y + ky - 1;
        if (yy < 0 || yy >= n) continue;
        for (int x = 0; x < n; ++x) {
            const int xx = x + kx - 1;
            if (xx < 0 || xx >= n) continue;
            s += h[base + (size_t)(yy * n + xx) * NM] * dd[base + (size_t)(y * n + x) * NM];
        }
    }
    part[(size_t)blockIdx.x * 288 + threadIdx.x] = s;
}

// ---- batch assembly: encode_nn_input(Player) (encoder.rs:10-46) and the targets (:48-68) from packed replay records -------------------
// record: board u8[HW], turn u8, pad to 4, pi f32[HW], z f32 (omok_replay_augment_dev).  Input row [3 HW]: cell a -> (2a, 2a + 1) = (stone of the side
// to move, stone of the opponent), [2 HW, 3 HW) = 1 where Black is to move
__global__ __launch_bounds__(256) void k_assemble(const uint8_t* __restrict__ records, const int64_t* __restrict__ idx, int hw, int rec, int brd,
                                                  float* __restrict__ x0, float* __restrict__ pi, float* __restrict__ z) {
    const int b = blockIdx.x;
    const uint8_t* r = records + (size_t)idx[b] * rec;
    const int turn = r[hw], mine = turn == 0 ? 1 : 2;
    for (int m = threadIdx.x; m < 3 * hw; m += 256) {
        float v;
        if (m < 2 * hw) {
            const int s = r[m >> 1];
            v = s == 0 ? 0.0f : (((m & 1) == 0) == (s == mine) ? 1.0f : 0.0f);
        } else {
            v = turn == 0 ? 1.0f : 0.0f;
        }
        x0[(size_t)b * 3 * hw + m] = v;
    }
    const float* f = (const float*)(r + brd);
    for (int a = threadIdx.x; a < hw; a += 256) pi[(size_t)b * hw + a] = f[a];
    if (threadIdx.x == 0) z[b] = f[hw];
}

// ---- losses and the gradients of the two heads: one wave per sample ------------------------------------------------------------------
__device__ inline float wave_sum(float v) { // butterfly: a fixed order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// p_loss_b = -sum pi log_softmax(logits) (network.rs:249-253), v_loss_b = (z - tanh(vpre))^2 (agent_model.rs:57-67);
// dlogits = (softmax sum(pi) - pi) / B, dvpre = 2 (v - z)(1 - v^2) / B (NULL: losses only)
__global__ __launch_bounds__(64) void k_losses(const float* __restrict__ logits, const float* __restrict__ vpre, const float* __restrict__ pi,
                                               const float* __restrict__ z, int hw, float inv_b, float* __restrict__ rows, float* __restrict__ dlogits,
                                               float* __restrict__ dvpre) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* l = logits + (size_t)b * hw;
    const float* t = pi + (size_t)b * hw;
    float mx = -INFINITY;
    for (int a = lane; a < hw; a += 64) mx = fmaxf(mx, l[a]);
    mx = wave_max(mx);
    float se = 0.0f, sp = 0.0f;
    for (int a = lane; a < hw; a += 64) { se += expf(l[a] - mx); sp += t[a]; }
    se = wave_sum(se);
    sp = wave_sum(sp);
    const float log_z = mx + logf(se);
    float ce = 0.0f;
    for (int a = lane; a < hw; a += 64) {
        const float ls = l[a] - log_z;
        ce -= t[a] * ls;
        if (dlogits) dlogits[(size_t)b * hw + a] = (expf(ls) * sp - t[a]) * inv_b;
    }
    ce = wave_sum(ce);
    if (lane == 0) {
        const double v = tanh((double)vpre[b]), dv = (double)z[b] - v; // one scalar per sample: in f64, so that the value head's gradients carry the rounding
        rows[2 * b] = (float)(dv * dv);                                // of vpre alone (the bias gradient is a sum of B of these with cancellation)
        rows[2 * b + 1] = ce;
        if (dvpre) dvpre[b] = (float)(2.0 * (v - (double)z[b]) * (1.0 - v * v) * (double)inv_b);
    }
}
// the means over the batch in sample order -> out[0..2] = v_loss, p_loss, loss; accumulate: out[4..6] += them (omok_train_run, step order)
__global__ void k_loss_means(const float* __restrict__ rows, int k, float* __restrict__ out, int accumulate) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float sv = 0.0f, sp = 0.0f;
    for (int b = 0; b < k; ++b) { sv += rows[2 * b]; sp += rows[2 * b + 1]; }
    const float v = sv / (float)k, p = sp / (float)k, l = v + p;
    out[0] = v; out[1] = p; out[2] = l;
    if (accumulate) { out[4] += v; out[5] += p; out[6] += l; }
}

// ---- Adadelta (TensorFlow ApplyAdadelta) on all 31 variables in one launch -----------------------------------------------------------
struct AdadeltaArgs {
    float* w[NET_TENSORS];
    long long off[NET_TENSORS + 1];
    int blk[NET_TENSORS + 1]; // first workgroup of tensor i (1024 elements per workgroup)
};
__global__ __launch_bounds__(256) void k_adadelta(AdadeltaArgs a, const float* __restrict__ grad, float* __restrict__ acc, float* __restrict__ accu) {
    int t = 0;
    while (t + 1 < NET_TENSORS && (int)blockIdx.x >= a.blk[t + 1]) ++t;
    const long long size = a.off[t + 1] - a.off[t];
    const long long e0 = (long long)((int)blockIdx.x - a.blk[t]) * 1024 + threadIdx.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long e = e0 + 256 * j;
        if (e >= size) break;
        const size_t s = (size_t)(a.off[t] + e);
        const float g = grad[s];
        const float ac = TRAIN_RHO * acc[s] + (1.0f - TRAIN_RHO) * g * g;
        const float upd = sqrtf(accu[s] + TRAIN_EPSILON) / sqrtf(ac + TRAIN_EPSILON) * g;
        acc[s] = ac;
        accu[s] = TRAIN_RHO * accu[s] + (1.0f - TRAIN_RHO) * upd * upd;
        a.w[t][e] -= TRAIN_LEARNING_RATE * upd;
    }
}
// The data-parallel update (omok_train_apply): the same launch shape on the ranks' gradient slabs [ranks][count].  Per element the slabs are added in
// rank order and the sum scaled by 1 / ranks -- plain fp32 adds and one multiply, nothing contracted into them, so every rank that holds the same slabs
// forms the same bits whatever collective moved them -- the averaged gradient is kept in `grad` (omok_debug_train_gradient), then ApplyAdadelta as above.
// Streaming: ranks x 4 B read, grad written, acc / accu / w read and written per element; tensor offsets are only 4-byte aligned (the head biases have HW
// elements), so the accesses stay one dword per lane, 256 B per wave and instruction.
__device__ inline float rank_average(const float* __restrict__ slabs, size_t s, int ranks, size_t count, float scale) {
#pragma clang fp contract(off)
    float g = slabs[s];
    for (int r = 1; r < ranks; ++r) g += slabs[(size_t)r * count + s];
    return g * scale;
}
__global__ __launch_bounds__(256) void k_adadelta_ranks(AdadeltaArgs a, const float* __restrict__ slabs, int ranks, float scale, float* __restrict__ grad,
                                                        float* __restrict__ acc, float* __restrict__ accu) {
    int t = 0;
    while (t + 1 < NET_TENSORS && (int)blockIdx.x >= a.blk[t + 1]) ++t;
    const long long size = a.off[t + 1] - a.off[t];
    const long long e0 = (long long)((int)blockIdx.x - a.blk[t]) * 1024 + threadIdx.x;
    const size_t count = (size_t)a.off[NET_TENSORS];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long e = e0 + 256 * j;
        if (e >= size) break;
        const size_t s = (size_t)(a.off[t] + e);
        const float g = rank_average(slabs, s, ranks, count, scale);
        grad[s] = g;
        const float ac = TRAIN_RHO * acc[s] + (1.0f - TRAIN_RHO) * g * g; // (the lines of k_adadelta, which keeps its own device code)
        const float upd = sqrtf(accu[s] + TRAIN_EPSILON) / sqrtf(ac + TRAIN_EPSILON) * g;
        acc[s] = ac;
        accu[s] = TRAIN_RHO * accu[s] + (1.0f - TRAIN_RHO) * upd * upd;
        a.w[t][e] -= TRAIN_LEARNING_RATE * upd;
    }
}

// ---- batch draw (src/trainer.rs:329-350 choose_multiple: uniform, without replacement) ------------------------------------------------
// index i = the mulhi(x0, R - i)-th record, 0-based ascending, not among the first i drawn; x0 = word 0 of Philox4x32-10(key; i, step, 0,
// RNG_TRAIN_BATCH).  One wave; `chosen` is the sorted list of the indices drawn so far: c[j] - j never decreases, so the records in front of the
// answer are the j with c[j] - j <= r.
__device__ inline uint32_t philox_x(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}
__global__ __launch_bounds__(64) void k_draw(uint64_t key, uint32_t step, uint32_t n_records, int k, int64_t* __restrict__ out) {
    __shared__ uint32_t chosen[TRAIN_MAX_BATCH + 64];
    const int lane = threadIdx.x;
    for (int i = 0; i < k; ++i) {
        const uint32_t r = __umulhi(philox_x(key, (uint32_t)i, step, 0u, RNG_TRAIN_BATCH), n_records - (uint32_t)i);
        int cnt = 0;
        for (int j = lane; j < i; j += 64) cnt += chosen[j] - (uint32_t)j <= r ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        const uint32_t v = r + (uint32_t)cnt;
        __syncthreads();
        for (int c = (i - 1) / 64; i > 0 && c >= cnt / 64; --c) { // make room at position cnt: the entries behind it move up by one, highest chunk first
            const int j = c * 64 + lane;
            const bool mv = j >= cnt && j < i;
            const uint32_t val = mv ? chosen[j] : 0u;
            __syncthreads();
            if (mv) chosen[j + 1] = val;
            __syncthreads();
        }
        if (lane == 0) { chosen[cnt] = v; out[i] = (int64_t)v; }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
size_t train_alloc(Train& T, const Net& net, int max_b) {
    T.n = net.n; T.hw = net.hw; T.max_b = max_b;
    T.brd = (T.hw + 1 + 3) / 4 * 4;
    T.rec = T.brd + 4 * T.hw + 4;
    T.off[0] = 0;
    for (int i = 0; i < NET_TENSORS; ++i) T.off[i + 1] = T.off[i] + net.wsize[i];
    const size_t total = (size_t)T.off[NET_TENSORS], B = (size_t)max_b, hw = (size_t)T.hw, rows = B * hw;
    bool ok = true;
    auto A = [&](float** p, size_t n, bool zero = false) {
        if (!ok) return;
        if (hipMalloc((void**)p, sizeof(float) * n) != hipSuccess) { *p = nullptr; ok = false; return; }
        if (zero && hipMemset(*p, 0, sizeof(float) * n) != hipSuccess) ok = false;
        T.bytes += sizeof(float) * n;
    };
    A(&T.acc, total, true);
    A(&T.accu, total, true);
    A(&T.grad, total, true);
    A((float**)&T.idx, 2 * B);
    A(&T.x0, rows * 3); A(&T.pi, rows); A(&T.z, B);
    A(&T.a0, rows * NC);
    for (int i = 0; i < 3; ++i) { A(&T.h[i], rows * NM); A(&T.d[i], rows * NM); A(&T.g[i], rows * NM); A(&T.x[i], rows * NC); }
    A(&T.h0, B * NF); A(&T.h1, B * NF); A(&T.logits, rows); A(&T.vpre, B);
    for (int i = 0; i < 2; ++i) { A(&T.dx[i], rows * NC); A(&T.dm[i], rows * NM); }
    A(&T.dh0, B * NF); A(&T.dh1, B * NF); A(&T.dlogits, rows); A(&T.dvpre, B);
    A(&T.ws, TRAIN_WS_FLOATS);
    A(&T.colpart, std::max((rows + 63) / 64 * NF, B * 288));
    A(&T.loss_rows, 2 * B);
    A(&T.losses, 8, true);
    if (!ok) { train_free(T); return 0; }
    T.has_grad = false;
    return T.bytes;
}

void train_free(Train& T) {
    float** ptrs[] = {&T.acc, &T.accu, &T.grad, (float**)&T.idx, &T.x0, &T.pi, &T.z, &T.a0, &T.h[0], &T.h[1], &T.h[2], &T.d[0], &T.d[1], &T.d[2],
                      &T.g[0], &T.g[1], &T.g[2], &T.x[0], &T.x[1], &T.x[2], &T.h0, &T.h1, &T.logits, &T.vpre, &T.dx[0], &T.dx[1], &T.dm[0], &T.dm[1],
                      &T.dh0, &T.dh1, &T.dlogits, &T.dvpre, &T.ws, &T.colpart, &T.loss_rows, &T.losses};
    for (float** p : ptrs) { if (*p) hipFree(*p); *p = nullptr; }
    T.bytes = 0;
}

void train_draw(Train& T, int64_t n_records, int k, uint64_t key, int step, hipStream_t st) {
    k_draw<<<1, 64, 0, st>>>(key, (uint32_t)step, (uint32_t)n_records, k, T.idx);
}

// network.rs:51-262 on the assembled batch: activations stay in T for the backward pass
static void forward(Train& T, const Net& net, int k, hipStream_t st) {
    float* const* w = net.w;
    const int hw = T.hw, rows = k * hw;
    launch_gemm(T, st, GEMM_NN, T.x0, 3, w[0], NC, T.a0, NC, rows, NC, 3, w[1], nullptr, 1);
    const float* x = T.a0;
    for (int i = 0; i < 3; ++i) { // bottleneck block (network-utils/src/lib.rs:386-461): 1x1 down, depthwise 3x3, pointwise + bias, 1x1 up + bias, add, activation
        float* const* b = w + 2 + 7 * i;
        launch_gemm(T, st, GEMM_NN, x, NC, b[0], NM, T.h[i], NM, rows, NM, NC, b[1], nullptr, 1);
        k_depthwise<false><<<(unsigned)(((size_t)rows * NM + 255) / 256), 256, 0, st>>>(T.h[i], b[2], nullptr, T.d[i], T.n, rows);
        launch_gemm(T, st, GEMM_NN, T.d[i], NM, b[3], NM, T.g[i], NM, rows, NM, NM, b[4], nullptr, 1);
        launch_gemm(T, st, GEMM_NN, T.g[i], NM, b[5], NC, T.x[i], NC, rows, NC, NM, b[6], x, 1);
        x = T.x[i];
    }
    const int kf = hw * NC;
    launch_gemm(T, st, GEMM_NN, x, kf, w[23], NF, T.h0, NF, k, NF, kf, w[24], nullptr, 1);
    launch_gemm(T, st, GEMM_NN, T.h0, NF, w[25], NF, T.h1, NF, k, NF, NF, w[26], nullptr, 1);
    launch_gemm(T, st, GEMM_NN, T.h1, NF, w[27], 1, T.vpre, 1, k, 1, NF, w[28]);
    launch_gemm(T, st, GEMM_NN, T.h1, NF, w[29], hw, T.logits, hw, k, hw, NF, w[30]);
}

static void losses(Train& T, int k, bool grads, bool accumulate, hipStream_t st) {
    k_losses<<<k, 64, 0, st>>>(T.logits, T.vpre, T.pi, T.z, T.hw, 1.0f / (float)k, T.loss_rows, grads ? T.dlogits : nullptr, grads ? T.dvpre : nullptr);
    k_loss_means<<<1, 64, 0, st>>>(T.loss_rows, k, T.losses, accumulate ? 1 : 0);
}

// gradients of all 31 variables -> T.grad (from T.dlogits / T.dvpre and the saved activations)
static void backward(Train& T, const Net& net, int k, hipStream_t st) {
    float* const* w = net.w;
    float* gr[NET_TENSORS];
    for (int i = 0; i < NET_TENSORS; ++i) gr[i] = T.grad + T.off[i];
    const int hw = T.hw, rows = k * hw, kf = hw * NC;
    // heads
    launch_gemm(T, st, GEMM_TN, T.h1, NF, T.dlogits, hw, gr[29], hw, NF, hw, k);
    launch_colsum(T, st, T.dlogits, k, hw, gr[30]);
    launch_gemm(T, st, GEMM_TN, T.h1, NF, T.dvpre, 1, gr[27], 1, NF, 1, k);
    launch_colsum(T, st, T.dvpre, k, 1, gr[28]);
    launch_gemm(T, st, GEMM_NT, T.dvpre, 1, w[27], 1, T.dh1, NF, k, NF, 1);
    launch_gemm(T, st, GEMM_NT, T.dlogits, hw, w[29], hw, T.dh1, NF, k, NF, hw, nullptr, T.dh1, 2, T.h1);
    // fc1
    launch_gemm(T, st, GEMM_TN, T.h0, NF, T.dh1, NF, gr[25], NF, NF, NF, k);
    launch_colsum(T, st, T.dh1, k, NF, gr[26]);
    launch_gemm(T, st, GEMM_NT, T.dh1, NF, w[25], NF, T.dh0, NF, k, NF, NF, nullptr, nullptr, 2, T.h0);
    // fc0: its weight gradient is [HW 128][512] summed over the batch only
    launch_gemm(T, st, GEMM_TN, T.x[2], kf, T.dh0, NF, gr[23], NF, kf, NF, k);
    launch_colsum(T, st, T.dh0, k, NF, gr[24]);
    float *dy = T.dx[0], *dprev = T.dx[1];
    launch_gemm(T, st, GEMM_NT, T.dh0, NF, w[23], NF, dy, kf, k, kf, NF, nullptr, nullptr, 2, T.x[2]);
    for (int i = 2; i >= 0; --i) { // dy = gradient in front of the block's last activation
        float* const* b = w + 2 + 7 * i;
        float* const* gb = gr + 2 + 7 * i;
        const float* xin = i == 0 ? T.a0 : T.x[i - 1];
        launch_gemm(T, st, GEMM_TN, T.g[i], NM, dy, NC, gb[5], NC, NM, NC, rows);
        launch_colsum(T, st, dy, rows, NC, gb[6]);
        launch_gemm(T, st, GEMM_NT, dy, NC, b[5], NC, T.dm[0], NM, rows, NM, NC, nullptr, nullptr, 2, T.g[i]);
        launch_gemm(T, st, GEMM_TN, T.d[i], NM, T.dm[0], NM, gb[3], NM, NM, NM, rows);
        launch_colsum(T, st, T.dm[0], rows, NM, gb[4]);
        launch_gemm(T, st, GEMM_NT, T.dm[0], NM, b[3], NM, T.dm[1], NM, rows, NM, NM);
        k_depthwise_taps<<<k, 288, 0, st>>>(T.h[i], T.dm[1], T.n, T.colpart);
        k_colsum_final<<<2, 256, 0, st>>>(T.colpart, k, 288, gb[2]);
        k_depthwise<true><<<(unsigned)(((size_t)rows * NM + 255) / 256), 256, 0, st>>>(T.dm[1], b[2], T.h[i], T.dm[0], T.n, rows);
        launch_gemm(T, st, GEMM_TN, xin, NC, T.dm[0], NM, gb[0], NM, NC, NM, rows);
        launch_colsum(T, st, T.dm[0], rows, NM, gb[1]);
        launch_gemm(T, st, GEMM_NT, T.dm[0], NM, b[0], NM, dprev, NC, rows, NC, NM, nullptr, dy, 2, xin); // + the skip connection's share
        std::swap(dy, dprev);
    }
    launch_gemm(T, st, GEMM_TN, T.x0, 3, dy, NC, gr[0], NC, 3, NC, rows);
    launch_colsum(T, st, dy, rows, NC, gr[1]);
}

static AdadeltaArgs adadelta_args(const Train& T, const Net& net) {
    AdadeltaArgs a;
    a.blk[0] = 0;
    for (int i = 0; i < NET_TENSORS; ++i) {
        a.w[i] = net.w[i];
        a.off[i] = T.off[i];
        a.blk[i + 1] = a.blk[i] + (int)((net.wsize[i] + 1023) / 1024);
    }
    a.off[NET_TENSORS] = T.off[NET_TENSORS];
    return a;
}

static void adadelta(Train& T, Net& net, hipStream_t st) {
    const AdadeltaArgs a = adadelta_args(T, net);
    k_adadelta<<<a.blk[NET_TENSORS], 256, 0, st>>>(a, T.grad, T.acc, T.accu);
}

// The step in two halves, where the gradients can leave and enter (omok_train_backward / omok_train_apply); train_step below runs the same halves.
void train_backward(Train& T, const Net& net, const void* records_dev, int k, hipStream_t st) {
    k_assemble<<<k, 256, 0, st>>>((const uint8_t*)records_dev, T.idx, T.hw, T.rec, T.brd, T.x0, T.pi, T.z);
    forward(T, net, k, st);
    losses(T, k, true, false, st);
    backward(T, net, k, st);
    T.has_grad = true;
}

void train_update(Train& T, Net& net, const float* grads_dev, int ranks, hipStream_t st) {
    if (!grads_dev) { adadelta(T, net, st); return; }
    const AdadeltaArgs a = adadelta_args(T, net);
    k_adadelta_ranks<<<a.blk[NET_TENSORS], 256, 0, st>>>(a, grads_dev, ranks, 1.0f / (float)ranks, T.grad, T.acc, T.accu);
    T.has_grad = true;
}

void train_evaluate(Train& T, const Net& net, int k, bool accumulate, hipStream_t st) {
    forward(T, net, k, st); // agent_model.rs:150-166: the three losses are fetched after the minimize run
    losses(T, k, false, accumulate, st);
}

void train_step(Train& T, Net& net, const void* records_dev, int k, bool update, bool accumulate, hipStream_t st) {
    if (!update) {
        k_assemble<<<k, 256, 0, st>>>((const uint8_t*)records_dev, T.idx, T.hw, T.rec, T.brd, T.x0, T.pi, T.z);
        train_evaluate(T, net, k, accumulate, st);
        return;
    }
    train_backward(T, net, records_dev, k, st);
    train_update(T, net, nullptr, 1, st);
    train_evaluate(T, net, k, accumulate, st);
}

} // namespace omok
