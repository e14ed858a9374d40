// net_kernels.hip — forward of the policy/value net (alpha-zero/src/network.rs:51-262, builders
// network-utils/src/lib.rs:95-170,172-262,285-330,386-461) for gfx950.
//
// OMOK_NET_F16X3 (default): every contraction uses SPLIT operands: x = hi + lo with hi = f16(x), product =
// hi*hi + lo*hi + hi*lo in an fp32 accumulator.  Trunk, fc1 and heads run the three terms on
// v_mfma_f32_32x32x16_f16 (lo = f16(x - hi)); fc0 runs hi*hi on the f16 MFMA and the two correction terms on the
// block-scaled fp6 MFMA (k_fc0_mx).  Plain fp16/bf16 inputs miss the 1e-3 parity bar on this net (random-init
// logits have std ~9; tools/precision_study.py); the split lands at 1e-5 (f16 terms) .. 1e-4 (fp6 terms).
//
// Everything is computed TRANSPOSED: D[out-feature, column] = W^T[out, in] * X[in, column] with the
// column (pixel in the trunk, sample in the fc layers) on the MFMA lane.  A 32x32 accumulator
// tile then IS the next layer's B operand (no LDS round trip): registers 8s..8s+7 of lane-half h
// are the 8 k-values of k-step s, in the permuted order
//     kperm(T, s, h, j) = 32*T + 16*s + 8*(j>>2) + 4*h + (j&3)
// and every weight matrix is packed on the host in exactly that k order (pack_A below).
//
//   k_trunk   one workgroup = one sample, one wave = one 32-pixel tile: conv_in (one MFMA k-step) ->
//             3 x { 1x1 128->32, depthwise 3x3 through an LDS halo grid, 1x1 32->32, 1x1 32->128 +
//             residual } with all weights LDS-resident -> fc0 operand rows (f16 hi | fp6 residual) in HBM
//   k_fc0_mx  fc0: 512 features x 128 samples per workgroup, one wave per SIMD, LDS-DMA rings
//   k_gemm_t  D^T[M x samples] = Wp[M x K] * Act^T, 8 waves, LDS ring: fc1, heads
//   k_tail_fused  fc1 and the heads of a whole-K round in one launch: k_gemm_t's fc1 loop, h1 handed to the heads loop through LDS in chunks of 8 k-steps
//   k_softmax policy softmax + value tanh
//
// OMOK_NET_F32: naive fp32 VALU kernels (k-ascending sums), debug / A-B reference on the GPU.
#include "net.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace omok {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

enum { EPI_SPLIT = 0, EPI_LOGITS = 1, EPI_PARTIAL = 2 }; // GEMM epilogues
constexpr int GT_BS = 128;                               // samples per GEMM workgroup

__host__ __device__ inline int kperm(int T, int s, int h, int j) { return 32 * T + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3); }
// LeakyRelu alpha 0.2 (TF default) = max(x, 0.2x).  One v_mul + one v_max: fmaxf() would add a
// canonicalising v_max per operand under IEEE mode.
__device__ inline float lrelu(float x) {
    const float y = 0.2f * x;
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
    return r;
}

typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ inline void nt_store(const uint4& v, uint4* p) { __builtin_nontemporal_store(u32x4{v.x, v.y, v.z, v.w}, (u32x4*)p); }
__device__ inline uint4 nt_load(const uint4* p) { const u32x4 v = __builtin_nontemporal_load((const u32x4*)p); return make_uint4(v[0], v[1], v[2], v[3]); }
typedef unsigned int u32x6 __attribute__((ext_vector_type(6)));
typedef float f32x16v __attribute__((ext_vector_type(16)));
typedef _Float16 half32 __attribute__((ext_vector_type(32)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
// x = hi + lo with hi = f16(x) (v_cvt_pk_f16_f32, round to nearest: two values per instruction) and
// lo = f16(x - hi) computed by ONE mixed-precision fma per value (v_fma_mix{lo,hi}_f16 reads hi as f16 and x as
// f32 and writes the f16 half directly): 1.5 VALU per value.  The trunk is VALU-bound, not MFMA-bound.
__device__ inline void split8(const float* v, half8& hi, half8& lo) {
    union { uint32_t u[4]; half8 h; } H, L;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float a = v[2 * j], b = v[2 * j + 1];
        const uint32_t ph = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){a, b}, half2v));
        uint32_t pl;
        asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(pl) : "v"(ph), "v"(a));
        asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(pl) : "v"(ph), "v"(b));
        H.u[j] = ph;
        L.u[j] = pl;
    }
    hi = H.h;
    lo = L.h;
}
// LeakyRelu on a pair: a multiply + two v_max.  The multiply is left to the compiler: `(f32x2){a, b} * 0.2f` comes out as two v_mul_f32 in 114 of
// k_sib_children2's 216 pairs (tools/isa_hist.py); forcing v_pk_mul_f32 saved 115 VALU per child and no time (profiles/r06_ab_children_diet.txt).
__device__ inline f32x2 lrelu2(float a, float b) {
    const f32x2 y = (f32x2){a, b} * 0.2f;
    f32x2 r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r[0]) : "v"(a), "v"(y[0]));
    asm("v_max_f32 %0, %1, %2" : "=v"(r[1]) : "v"(b), "v"(y[1]));
    return r;
}
#define LRELU16(X)                                           \
    do {                                                     \
        _Pragma("unroll") for (int i_ = 0; i_ < 16; i_ += 2) { \
            const f32x2 r_ = lrelu2((X)[i_], (X)[i_ + 1]);   \
            (X)[i_] = r_[0];                                 \
            (X)[i_ + 1] = r_[1];                             \
        }                                                    \
    } while (0)
// Lanes of ONE wave exchanging data through LDS (a lane stages its pixel's pieces, other lanes read them back): the hardware executes
// a wave's LDS instructions in order, but the COMPILER reasons per lane -- on the path of a lane that skips the staging stores (a pad
// pixel) it may take the read-back for a repeat of the previous pass's load of the same address and reuse that value (seen: hipcc 7.2
// moved the ds_read into the `if (valid)` block of the stores).  A wavefront-scope fence costs no instruction and forbids exactly that.
#define WAVE_LDS_FENCE() __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront")
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16((a), (b), (c), 0, 0, 0)
#define MFMA3(ah, al, bh, bl, c)   \
    do {                           \
        (c) = MFMA16((ah), (bh), (c)); \
        (c) = MFMA16((al), (bh), (c)); \
        (c) = MFMA16((ah), (bl), (c)); \
    } while (0)

// ===============================================================================================
// OMOK_NET_F32 kernels
// ===============================================================================================
template <int ACT> // 0 none, 1 lrelu, 2 lrelu(x + res), 3 tanh
__global__ void k32_linear(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ b,
                           const float* res, float* out, int rows_per_sample, int cin, int cout,
                           const int32_t* __restrict__ d_count, int base, int chunk) {
    int cnt = d_count[0] - base;
    if (cnt > chunk) cnt = chunk;
    const size_t total = (size_t)(cnt > 0 ? cnt : 0) * rows_per_sample * cout;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t row = i / cout;
        const int o = (int)(i % cout);
        const float* x = in + row * cin;
        float acc = 0.0f;
        for (int k = 0; k < cin; ++k) acc += x[k] * w[(size_t)k * cout + o];
        acc += b[o];
        if (ACT == 2) acc += res[row * cout + o];
        if (ACT == 1 || ACT == 2) acc = acc > 0.0f ? acc : 0.2f * acc;
        if (ACT == 3) acc = tanhf(acc);
        out[row * cout + o] = acc;
    }
}

__global__ void k32_depthwise(const float* __restrict__ in, const float* __restrict__ w, float* __restrict__ out, int n,
                              const int32_t* __restrict__ d_count, int base, int chunk) {
    int cnt = d_count[0] - base;
    if (cnt > chunk) cnt = chunk;
    const int hw = n * n;
    const size_t total = (size_t)(cnt > 0 ? cnt : 0) * hw * NM;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % NM);
        const size_t pix = i / NM;
        const int px = (int)(pix % hw);
        const size_t s = pix / hw;
        const int y = px / n, x = px % n;
        float acc = 0.0f;
        for (int dy = 0; dy < 3; ++dy)
            for (int dx = 0; dx < 3; ++dx) {
                const int yy = y + dy - 1, xx = x + dx - 1;
                if (yy < 0 || yy >= n || xx < 0 || xx >= n) continue;
                acc += in[(s * hw + (size_t)(yy * n + xx)) * NM + c] * w[(dy * 3 + dx) * NM + c];
            }
        out[i] = acc;
    }
}

__global__ void k32_softmax(const float* __restrict__ logits, float* __restrict__ p, int hw, int rowp,
                            const int32_t* __restrict__ d_count, int base, int chunk) {
    int cnt = d_count[0] - base;
    if (cnt > chunk) cnt = chunk;
    const int s = blockIdx.x;
    if (s >= cnt) return;
    const int lane = threadIdx.x;
    const float* l = logits + (size_t)s * hw;
    float mx = -INFINITY;
    for (int a = lane; a < hw; a += 64) mx = fmaxf(mx, l[a]);
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.0f;
    for (int a = lane; a < hw; a += 64) sum += expf(l[a] - mx);
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    float* po = p + (size_t)(base + s) * rowp;
    for (int a = lane; a < rowp; a += 64) po[a] = a < hw ? expf(l[a] - mx) / sum : 0.0f;
}

__global__ void k32_tanh(const float* __restrict__ in, float* __restrict__ out, const int32_t* __restrict__ d_count, int base, int chunk) {
    int cnt = d_count[0] - base;
    if (cnt > chunk) cnt = chunk;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cnt) out[i] = tanhf(in[i]);
}

static void forward_f32(Net& net, const Store& S, int max_count, hipStream_t st, Prof* prof) {
    const int hw = net.hw, n = net.n;
    const int grid = 2048, blk = 256;
    for (int base = 0; base < max_count; base += net.chunk) {
        const int ch = net.chunk;
        const float* in = net.in_f32 + (size_t)base * 3 * hw;
        if (prof) prof->begin(PC_TRUNK, st);
        k32_linear<1><<<grid, blk, 0, st>>>(in, net.w[0], net.w[1], nullptr, net.sx, hw, 3, NC, S.d_count, base, ch);
        for (int b = 0; b < 3; ++b) {
            float* const* t = net.w + 2 + 7 * b;
            k32_linear<1><<<grid, blk, 0, st>>>(net.sx, t[0], t[1], nullptr, net.sh, hw, NC, NM, S.d_count, base, ch);
            k32_depthwise<<<grid, blk, 0, st>>>(net.sh, t[2], net.sd, n, S.d_count, base, ch);
            k32_linear<1><<<grid, blk, 0, st>>>(net.sd, t[3], t[4], nullptr, net.sg, hw, NM, NM, S.d_count, base, ch);
            k32_linear<2><<<grid, blk, 0, st>>>(net.sg, t[5], t[6], net.sx, net.sx, hw, NM, NC, S.d_count, base, ch);
        }
        if (prof) { prof->end(st); prof->begin(PC_FC0, st); }
        k32_linear<1><<<grid, blk, 0, st>>>(net.sx, net.w[23], net.w[24], nullptr, net.s0, 1, NC * hw, NF, S.d_count, base, ch);
        if (prof) { prof->end(st); prof->begin(PC_TAIL, st); }
        k32_linear<1><<<grid, blk, 0, st>>>(net.s0, net.w[25], net.w[26], nullptr, net.s1, 1, NF, NF, S.d_count, base, ch);
        k32_linear<0><<<grid, blk, 0, st>>>(net.s1, net.w[27], net.w[28], nullptr, net.vpre + base, 1, NF, 1, S.d_count, base, ch);
        k32_tanh<<<(ch + 255) / 256, 256, 0, st>>>(net.vpre + base, net.v + base, S.d_count, base, ch);
        k32_linear<0><<<grid, blk, 0, st>>>(net.s1, net.w[29], net.w[30], nullptr, net.sh, 1, NF, hw, S.d_count, base, ch);
        k32_softmax<<<ch, 64, 0, st>>>(net.sh, net.p, hw, net.rowp, S.d_count, base, ch);
        if (prof) prof->end(st);
    }
}

// ===============================================================================================
// OMOK_NET_F16X3: trunk
// ===============================================================================================
// Packed trunk weights (f16, 1 KiB fragments of [lane 64][8]): per block 36 fragments:
//   L0 hi[8 ks] | L0 lo[8] | L1 hi[2] | L1 lo[2] | L2 hi[4 m][2 ks] | L2 lo[4][2]
// followed (global memory only, not LDS-resident) by the conv_in fragments hi[4 m] | lo[4 m]:
//   k-step of 16 with k = 0..2 the three input floats of the pixel, k = 3 the bias (input 1.0).
// fp32 side table (floats): per block { dw[9][32], b0[32], b1[32], b2[128] }
constexpr int TR_FRAGS_PER_BLOCK = 36;
constexpr int TR_WBYTES = 3 * TR_FRAGS_PER_BLOCK * 1024;
constexpr int TR_CONV_FRAGS = 8;
constexpr int TR_SIDE_PER_BLOCK = 9 * NM + NM + NM + NC; // 480 floats
constexpr int TR_SIDE_FLOATS = 3 * TR_SIDE_PER_BLOCK;    // 1440
constexpr int GRID_STRIDE = 36; // floats per halo-grid row (32 + 4 pad: conflict-free b128 reads)
// fc0 operand row: per (pixel tile, channel half q) one dense 6-KiB block = f16 part [32 pxl][128 B], then residual
// part [32 pxl][64 B] (uint4 units below)
constexpr int OP_BLK_U4 = 384, OP_LO_U4 = 256;
// FC0_F16 format of the same row (Net::fc0_fmt): the residual part of a block holds f16 residuals f16(x - hi) in the layout of the
// hi part ([32 pxl][piece (2j+h) 8][16 B]) instead of fp6 codes + scales: blocks of 8 KiB
constexpr int OPX_BLK_U4 = 512;
constexpr int fmt_blk_u4(bool f16lo) { return f16lo ? OPX_BLK_U4 : OP_BLK_U4; }
// The fc0 correction terms run on fp6 (e2m3) operands with per-lane E8M0 block scales ("MX6"; the fp8 format with global scales it replaced:
// docs/experiments/r15_retired_fp8_format.diff).
// MX6 block scales: 2^(floor(log2(amax * 32/31)) - 2).  With the plain floor(log2 amax) a block whose largest magnitude lies in [7.75, 8) x scale rounds up
// past e2m3's largest code (7.5) and saturates: up to 6 % error on the block's largest element in ~6 % of the blocks -- the outliers a max-error probe sees.
// The residual's scale comes from a block maximum of its own.  Taking it from the bound |x - f16(x)| <= 2^(floor(log2 |x|) - 11) instead saves 16 VALU per
// block in the trunk epilogue (trunk -2 %) and moved N = 9 max|dv| from 3.6e-4 to 5.9e-4: not taken.
constexpr float MX6_AMAX_ADJ = 32.0f / 31.0f;
constexpr int MX_SA = 2;        // (MxScales: global scales of the retired fp8 format.  Nothing on the device reads them any more; they stay only because k_fc0_mx's signature was not to change --
                                //  a follow-up removes MX_SA, MxScales, fc0_scales and Net::mx_sw together with that parameter)

// V2 children kernel (k_sib_children2, difference path): a base slot holds, PIXEL-major (a lane = (pixel, half h) of the MFMA accumulators reads its own
// pixel's bytes, and the two halves' four 16-B pieces together use every byte of the pixel's lines: planes by piece -- adjacent pixels adjacent -- fetched
// 2.5x the bytes through the L1 and were 20 % slower), uint4 units:
//   grids  [(blk * 2 + kind) * HW + pixel][8 pieces]: kind 0 = h (depthwise input), 1 = d (depthwise output) of block blk; piece 2 g + h = channels 8 g + 4 h .. + 3
//   x2     48 HW + [pixel][32 pieces]: the residual stream in front of block 2; piece 8 m + 2 g + h = channels 32 m + 8 g + 4 h .. + 3
constexpr int SIB2_U4_PER_PX = 80;
__host__ __device__ constexpr size_t sib2_slot_u4(int n) { return (size_t)n * n * SIB2_U4_PER_PX; }
__host__ __device__ constexpr size_t sib2_grid(int hw, int blk, int kind, int px, int g, int h) { return ((size_t)(blk * 2 + kind) * hw + px) * 8 + 2 * g + h; }
__host__ __device__ constexpr size_t sib2_x2(int hw, int px, int m, int g, int h) { return (size_t)48 * hw + (size_t)px * 32 + 8 * m + 2 * g + h; }

template <int N>
struct TrunkGeo {
    static constexpr int HW = N * N;
    static constexpr int TILES = (HW + 31) / 32;
    static constexpr int KSTEPS = HW * 8;          // fc0 k-steps (valid pixels only)
    // fc0 operand row: TILES x 2 dense blocks of OP_BLK_U4 (+ Net::row_pad so the row stride is not a power of two,
    // which would put every sample row on the same memory channels)
    static constexpr int ROW_U4 = TILES * 2 * OP_BLK_U4;
    static constexpr int GRID_ROWS = (N + 2) * (N + 2) + 1; // +1: the 3x6 window of the last strip may touch one row more
    static constexpr int GRID_BYTES = GRID_ROWS * GRID_STRIDE * 4;
    // samples per workgroup: at N = 9 a sample is only 3 waves and the LDS-resident weights allow one workgroup per CU,
    // so two samples (each with its own halo grid) share a workgroup and its barriers; at N = 15 two grids do not fit
    static constexpr int SPW = N == 9 ? 2 : 1;
    static constexpr int LDS_BYTES = TR_WBYTES + SPW * GRID_BYTES + TR_SIDE_FLOATS * 4;
    static constexpr int SW = N == 9 ? 5 : 4;      // depthwise strip width in pixels (N = 9: 2 strips of 5 = 144 items <= 192 threads)
    static constexpr int SPR = (N + SW - 1) / SW;  // strips per board row
    static constexpr int DW_ITEMS = N * SPR * 8;   // (row, strip, 4-channel group)
    static constexpr int THREADS = TILES * 64;
    static constexpr int DW_ITER = (DW_ITEMS + THREADS - 1) / THREADS;
    static constexpr int WG_THREADS = SPW * THREADS;
};

// ===============================================================================================
// OMOK_NET_F16X3: the trunk's tile arithmetic, defined ONCE for k_trunk, k_sib_children and k_sib_children2
// ===============================================================================================
// The three kernels push a 32-pixel tile (one wave: pixel = lane & 31, h = lane >> 5 the accumulator half) through the same network, and the rows they
// write must agree to the bit (the copy path's rows equal a full evaluation's; the two children kernels of the difference path are tested against each other).
// So every piece of per-tile arithmetic lives here: the kernels differ in where a tile's pixels come from, in the depthwise between L0 and L1, and in where the
// operand-row entries go.  Arguments are explicit and nothing is captured: ldsW / lside = the LDS-resident weights and side table, x = the tile's residual stream.
// Two exceptions, each measured (profiles/r15_trunk_shared_kernel_stats.txt): k_trunk keeps L0 as inline text and k_sib_children2 its own base_fetch; the reasons stand there.

// One-time prologue of a workgroup: conversions saturate (MODE.FP16_OVFL), trunk weights and side table into LDS (the caller zeroes its grids and synchronises).
// SKIP_U4: the first uint4s of the weights are not copied (their LDS stays unwritten; the layout and every offset are the same): k_sib_children2 passes block 0's L0
// fragments, which it never reads.
// DMA: the weights go to LDS by LDS-DMA (dma16s, the form k_fc0_mx streams with), one instruction per fragment of 64 lanes x 16 B, the fragments dealt to the waves -- the
// same bytes at the same addresses without the round trip through VGPRs, whose ~14 dependent load -> store trips per thread were most of a 7.5-us prologue.
// Nothing waits here: the caller runs its own fills, then trunk_lds_dma_wait() in front of its barrier.
template <bool NT>
__device__ inline void dma16s(const uint4* sbase, uint32_t voff, const uint4* lds);
template <int SKIP_U4 = 0, bool DMA = false>
__device__ __forceinline__ void trunk_lds_prologue(unsigned char* smem, float* lside, const uint4* __restrict__ wt, const float* __restrict__ side, int tid) {
    static_assert(SKIP_U4 % 64 == 0 && TR_WBYTES % 1024 == 0, "whole fragments");
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 23, 1), 1"); // fp6 / f16 conversions saturate (MODE.FP16_OVFL)
    if constexpr (DMA) {
        const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nwv = (int)blockDim.x >> 6;
        for (int f = SKIP_U4 / 64 + wv; f < TR_WBYTES / 1024; f += nwv) dma16s<false>(wt + f * 64, (uint32_t)(tid & 63) * 16u, (const uint4*)smem + f * 64);
    } else
        for (int i = SKIP_U4 + tid; i < TR_WBYTES / 16; i += blockDim.x) ((uint4*)smem)[i] = wt[i];
    for (int i = tid; i < TR_SIDE_FLOATS; i += blockDim.x) lside[i] = side[i];
}
__device__ __forceinline__ void trunk_lds_dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); } // (the DMAs are issued from asm: the compiler does not count them)
// The conv_in fragments of k_sib_children (k_sib_children2 reads the conv tables instead; k_conv_tables fetches them once): 32 registers that are only needed at the top of a pass.  They are fetched again at the END of every pass (from
// L2, under the stores) instead of living through the blocks, where they pushed lane-constant addresses into scratch whose
// reloads (a dozen dependent round trips in the store phase) cost more than the whole arithmetic of the pass
__device__ __forceinline__ void load_conv_w(const half8* convW, int lane, half8 (&cwh)[4], half8 (&cwl)[4]) {
    typedef const __attribute__((address_space(1))) half8* gptr_t; // (global, not generic: a flat load would also count as an LDS access)
    unsigned long long cpv = (unsigned long long)convW;
    asm volatile("" : "+s"(cpv)); // (opaque: keeps the loads inside the loop)
    gptr_t cp = (gptr_t)cpv;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        cwh[m] = cp[m * 64 + lane];
        cwl[m] = cp[(4 + m) * 64 + lane];
    }
}
// The three input bits of board pixel px (flat encoder.rs layout, Player mode) from the position's words in LDS: wsrc[0..NW)
// black, [NW..2 NW) white (one u64 each), turn = side to move
template <int N>
__device__ __forceinline__ void input_bits(const uint64_t* wsrc, int turn, int px, uint32_t (&bits)[3]) {
    constexpr int HW = N * N, NW = Geo<N>::NW;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int m = 3 * px + c;
        if (m >= 2 * HW) { bits[c] = turn == 0 ? 1u : 0u; continue; }   // encoder.rs:34-37
        const int cell = m >> 1;
        const bool want_black = ((m & 1) == 0) == (turn == 0);           // even slot = the side to move's stones (encoder.rs:24-27)
        const uint64_t w = wsrc[(want_black ? 0 : NW) + (cell >> 6)];
        bits[c] = (uint32_t)((w >> (cell & 63)) & 1ULL);
    }
}
// conv_in's B operand from the pixel's three input bits, written down as f16 0 / 1 (1.0 = 0x3C00; no float conversion, no operand split):
// k = (f0, f1, f2, 1) on lane-half 0, zeros on half 1 and in the remaining 12 k slots
__device__ __forceinline__ half8 conv_in_operand(int h, uint32_t b0, uint32_t b1, uint32_t b2) {
    union { uint32_t u[4]; half8 v; } Bq;
    Bq.u[0] = h == 0 ? (b0 * 0x3C00u) | (b1 * 0x3C000000u) : 0u;
    Bq.u[1] = h == 0 ? (b2 * 0x3C00u) | 0x3C000000u : 0u;
    Bq.u[2] = 0u;
    Bq.u[3] = 0u;
    return Bq.v;
}
// conv_in 1x1 3->128 + bias + lrelu as one 16-deep k-step.  SPLIT_B: the inputs are floats with a residual bl (k_trunk<FROM_F32>); board inputs are 0 / 1 and
// the bias 1: exact in f16, bl unused
template <bool SPLIT_B>
__device__ __forceinline__ void conv_in_tile(const half8 (&cwh)[4], const half8 (&cwl)[4], const half8& bh, const half8& bl, f32x16 (&x)[4]) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
        for (int i = 0; i < 16; ++i) x[m][i] = 0.0f;
        x[m] = MFMA16(cwh[m], bh, x[m]);
        x[m] = MFMA16(cwl[m], bh, x[m]);
        if (SPLIT_B) x[m] = MFMA16(cwh[m], bl, x[m]);
        LRELU16(x[m]);
    }
}
// L0 of block blk: 1x1 128 -> 32, bias as the initial accumulator (the caller applies the LeakyReLU on the way to its depthwise grid)
__device__ __forceinline__ void L0_tile(const half8* ldsW, const float* lside, int h, int lane, const f32x16 (&x)[4], int blk, f32x16& acc) {
    const half8* W = ldsW + (size_t)blk * TR_FRAGS_PER_BLOCK * 64;
    const float* b0 = lside + blk * TR_SIDE_PER_BLOCK + 9 * NM;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 bv = *(const f32x4*)(b0 + 8 * g + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[4 * g + i] = bv[i];
    }
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = x[ks >> 1][8 * (ks & 1) + j];
        half8 bh, bl;
        split8(v, bh, bl);
        const half8 ah = W[(0 + ks) * 64 + lane], al = W[(8 + ks) * 64 + lane];
        MFMA3(ah, al, bh, bl, acc);
    }
}
// Conv tables (Net::conv_tab): a board pixel's three input bits are f16 0 / 1 and k = 3 carries the bias, so conv_in's output of a pixel takes one of EIGHT values, and so
// does block 0's L0 (a 1x1 layer on that output).  Both depend on the weights only, so they are computed once per commit and k_sib_children2 reads them instead of running
// conv_in_tile and block 0's L0_tile in every pass.  Pattern = b0 | b1 << 1 | b2 << 2; fp32, rows padded so that lanes of different (pattern, h) read different 16-B slots:
//   T0[pattern][CT_T0_STRIDE]  conv_in after LeakyReLU, channel 32 m + 8 g + 4 h + i = x[m][4 g + i]
//   T1[pattern][CT_T1_STRIDE]  L0_tile's accumulator of block 0 (before LeakyReLU), channel 8 g + 4 h + i = acc[4 g + i]
constexpr int CT_T0_STRIDE = NC + 8, CT_T1_STRIDE = NM + 8; // 136, 40 floats: slot (2 p + h) mod 16, (10 p + h) mod 16 -- distinct over p = 0..7, h = 0..1
constexpr int CT_T1_OFF = 8 * CT_T0_STRIDE;
constexpr int CT_FLOATS = CT_T1_OFF + 8 * CT_T1_STRIDE; // 1408 floats = 5632 B
static_assert(NC == 128 && NM == 32 && CT_FLOATS % 4 == 0, "conv table layout");
// One wave, at the end of net_pack: pixel p = 0..7 of the tile carries pattern p (the other pixels run along).  The device functions are the ones the trunk kernels call
// (their weight pointers address global memory here), and an MFMA output column depends on its own B column only: an entry is the bit pattern any lane with that input computes.
__global__ __launch_bounds__(64) void k_conv_tables(const uint4* __restrict__ wt, const float* __restrict__ side, float* __restrict__ tab) {
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 23, 1), 1"); // MODE.FP16_OVFL as in trunk_lds_prologue
    const int lane = threadIdx.x, h = lane >> 5, pat = lane & 7;
    half8 cwh[4], cwl[4];
    load_conv_w((const half8*)(wt + TR_WBYTES / 16), lane, cwh, cwl);
    const half8 bq = conv_in_operand(h, pat & 1, (pat >> 1) & 1, (pat >> 2) & 1);
    f32x16 x[4], acc;
    conv_in_tile<false>(cwh, cwl, bq, bq, x);
    L0_tile((const half8*)wt, side, h, lane, x, 0, acc);
    if ((lane & 31) >= 8) return;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
            *(f32x4*)(tab + pat * CT_T0_STRIDE + 32 * m + 8 * g + 4 * h) = (f32x4){x[m][4 * g], x[m][4 * g + 1], x[m][4 * g + 2], x[m][4 * g + 3]};
        *(f32x4*)(tab + CT_T1_OFF + pat * CT_T1_STRIDE + 8 * g + 4 * h) = (f32x4){acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
    }
}
// L1 and L2 of block blk from the pixel's depthwise outputs d[16]: pointwise 32 -> 32 + bias + lrelu, then 1x1 32 -> 128 + bias + residual (accumulated onto x), lrelu
__device__ __forceinline__ void L1L2_tile(const half8* ldsW, const float* lside, int h, int lane, f32x16 (&x)[4], int blk, const float* d) {
    const half8* W = ldsW + (size_t)blk * TR_FRAGS_PER_BLOCK * 64;
    const float* sd = lside + blk * TR_SIDE_PER_BLOCK;
    const float *b1 = sd + 10 * NM, *b2 = b1 + NM;
    f32x16 accg;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 bv = *(const f32x4*)(b1 + 8 * g + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; ++i) accg[4 * g + i] = bv[i];
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        half8 bh, bl;
        split8(d + 8 * ks, bh, bl);
        const half8 ah = W[(16 + ks) * 64 + lane], al = W[(18 + ks) * 64 + lane];
        MFMA3(ah, al, bh, bl, accg);
    }
    float gv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) gv[i] = accg[i];
    LRELU16(gv);
    half8 gh[2], gl[2];
    split8(gv, gh[0], gl[0]);
    split8(gv + 8, gh[1], gl[1]);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 bv = *(const f32x4*)(b2 + 32 * m + 8 * g + 4 * h);
#pragma unroll
            for (int i = 0; i < 4; ++i) x[m][4 * g + i] += bv[i];
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const half8 ah = W[(20 + m * 2 + ks) * 64 + lane], al = W[(28 + m * 2 + ks) * 64 + lane];
            MFMA3(ah, al, gh[ks], gl[ks], x[m]);
        }
        LRELU16(x[m]);
    }
}
// ---- fc0 operand-row entries of a pixel, the VALUE part (registers in, pieces out).  Per channel half q a lane holds 32 values of its pixel: x[2 q + mm][8 sx + j],
//      and piece mm * 2 + sx is the 16 B of 8 f16 values the lane contributes to the pixel's 128-B f16 part.  Staging through LDS, read-back and the destination
//      of the stores are each kernel's own. ----
// FC0_F16 format: the four f16 hi pieces and the four f16 residual pieces f16(x - hi) of channel half q (split8: 1.5 VALU per value, no block maxima, no fp6 packing)
__device__ __forceinline__ void entry_f16_pieces(const f32x16 (&x)[4], int q, half8 (&hi8)[4], half8 (&lo8)[4]) {
#pragma unroll
    for (int mm = 0; mm < 2; ++mm)
#pragma unroll
        for (int sx = 0; sx < 2; ++sx) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = x[2 * q + mm][8 * sx + j];
            split8(v, hi8[mm * 2 + sx], lo8[mm * 2 + sx]);
        }
}
// fp6 format, first half: f16 hi piece mm * 2 + sx of channel half q (round to nearest), its 8 residuals (one mixed-precision fma per value) into res[] at
// their slots 16 mm + 8 sx + j, and the running block maxima of the values and of the residuals
__device__ __forceinline__ uint4 entry_fp6_hi_piece(const f32x16 (&x)[4], int q, int mm, int sx, float (&res)[32], float& amax_v, float& amax_l) {
    union { uint32_t u[4]; uint4 v; } H;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const float v0 = x[2 * q + mm][8 * sx + 2 * jj], v1 = x[2 * q + mm][8 * sx + 2 * jj + 1];
        const uint32_t ph = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){v0, v1}, half2v));
        H.u[jj] = ph;
        float l0, l1;
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l0) : "v"(ph), "v"(v0));
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(l1) : "v"(ph), "v"(v1));
        const int slot = 16 * mm + 8 * sx + 2 * jj; // slot of v0
        res[slot] = l0; res[slot + 1] = l1;
        // (from asm: fmaxf() drags a canonicalising v_max per operand along under IEEE mode)
        asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(amax_v) : "v"(v0), "v"(v1));
        asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(amax_l) : "v"(l0), "v"(l1));
    }
    return H.v;
}
// fp6 format, second half: the E8M0 bytes of the two block scales 2^(floor(log2 max) - 2) (e2m3 emax = 2; hi copy | residual << 8) and the packed fp6 residuals
// of the lane's 32 values (natural slot order 16 mm + reg)
__device__ __forceinline__ u32x6 entry_fp6_residuals(const float (&res)[32], float amax_v, float amax_l, uint32_t& esc) {
    int eh = (int)((__float_as_uint(amax_v * MX6_AMAX_ADJ) >> 23) & 0xFFu) - 2, el = (int)((__float_as_uint(amax_l * MX6_AMAX_ADJ) >> 23) & 0xFFu) - 2;
    eh = eh < 1 ? 1 : eh;
    el = el < 1 ? 1 : el;
    esc = (uint32_t)eh | ((uint32_t)el << 8);
    f32x16v ev, od; // v_cvt_scalef32_2xpk16_fp6_f32 interleaves its two sources: field 2i = ev[i], 2i+1 = od[i]
#pragma unroll
    for (int i = 0; i < 16; ++i) { ev[i] = res[2 * i]; od[i] = res[2 * i + 1]; }
    return __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(ev, od, __uint_as_float((uint32_t)el << 23));
}
// fp6 format: the lane's share of the 64-B residual part of (pixel, q) into the pixel's staging row:
// [h0 dwords 0..3][h1 dwords 0..3][h0 dwords 4,5 | h1 dwords 4,5][scale bytes h0, h1 | pad]
__device__ __forceinline__ void entry_fp6_stage(uint4* stage_w, int q, int h, u32x6 lo6, uint32_t esc) {
    stage_w[q * 4 + h] = make_uint4(lo6[0], lo6[1], lo6[2], lo6[3]);
    ((uint2*)(stage_w + q * 4 + 2))[h] = make_uint2(lo6[4], lo6[5]);
    ((uint16_t*)(stage_w + q * 4 + 3))[h] = (uint16_t)esc;
}
// ---- difference path: the BASE's operand entries of a lane's pixel (its own 4 f16 pieces and residual half per channel half q) and their subtraction from the
//      child's finished residual stream, dequantised exactly as fc0 multiplies them ----
struct BaseEntry {
    uint4 hi[2][4]; // the lane's four f16 pieces per channel half q
    u32x6 lo[2];    // fp6 format: its six dwords of packed fp6 residuals (one vector: as uint4 + uint2 members the compiler keeps them in scratch) ...
    uint32_t sc[2]; // ... and its scale bytes
};
template <bool F16LO>
__device__ __forceinline__ void base_fetch(BaseEntry& be, const uint4* frow, int px, int h) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const uint4* bp = frow + (size_t)((px >> 5) * 2 + q) * fmt_blk_u4(F16LO);
#pragma unroll
        for (int p4 = 0; p4 < 4; ++p4) be.hi[q][p4] = bp[(px & 31) * 8 + p4 * 2 + h];
        if (F16LO) continue; // (the f16 residual pieces: base_sub_f16lo, fetched behind the hi parts' subtraction -- 32 more registers do not fit beside L1L2)
        const uint4* lp = bp + OP_LO_U4 + (px & 31) * 4;
        const uint4 l4 = lp[h];
        const uint2 l2 = ((const uint2*)(lp + 2))[h];
        be.lo[q] = (u32x6){l4.x, l4.y, l4.z, l4.w, l2.x, l2.y};
        be.sc[q] = ((const uint16_t*)(lp + 3))[h];
    }
}
// x -= the f16 pieces `pc` (the lane's 4 pieces of channel half q: hi or residual part of the base's entries)
__device__ __forceinline__ void sub_pieces(f32x16 (&x)[4], int q, const uint4 (&pc)[4]) {
#pragma unroll
    for (int mm = 0; mm < 2; ++mm)
#pragma unroll
        for (int sx = 0; sx < 2; ++sx) {
            const uint4 hq = pc[mm * 2 + sx];
            const uint32_t hu[4] = {hq.x, hq.y, hq.z, hq.w};
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                float v0 = x[2 * q + mm][8 * sx + 2 * jj], v1 = x[2 * q + mm][8 * sx + 2 * jj + 1];
                asm("v_fma_mix_f32 %0, %1, -1.0, %0 op_sel_hi:[1,0,0]" : "+v"(v0) : "v"(hu[jj]));
                asm("v_fma_mix_f32 %0, %1, -1.0, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(v1) : "v"(hu[jj]));
                x[2 * q + mm][8 * sx + 2 * jj] = v0;
                x[2 * q + mm][8 * sx + 2 * jj + 1] = v1;
            }
        }
}
// FC0_F16 rows: x - hi - lo, exactly the base as fc0 multiplies it
__device__ __forceinline__ void base_sub_f16lo(f32x16 (&x)[4], const BaseEntry& be, const uint4* frow, int px, int h) {
    uint4 lo[2][4];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const uint4* bp = frow + (size_t)((px >> 5) * 2 + q) * OPX_BLK_U4 + OP_LO_U4;
#pragma unroll
        for (int p4 = 0; p4 < 4; ++p4) lo[q][p4] = bp[(px & 31) * 8 + p4 * 2 + h];
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) sub_pieces(x, q, be.hi[q]);
#pragma unroll
    for (int q = 0; q < 2; ++q) sub_pieces(x, q, lo[q]);
}
// fp6 rows: x - hi - fp6 residual * 2^scale
__device__ __forceinline__ void base_subtract(f32x16 (&x)[4], const BaseEntry& be) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        union { half32 v; uint32_t u[16]; } L; // residuals * 2^(scale - 127), element = slot 16 mm + reg (tools/probe/fp6_decode_probe.hip)
        L.v = __builtin_amdgcn_cvt_scalef32_pk32_f16_fp6(be.lo[q], __uint_as_float((be.sc[q] >> 8) << 23));
#pragma unroll
        for (int mm = 0; mm < 2; ++mm)
#pragma unroll
            for (int sx = 0; sx < 2; ++sx) {
                const uint4 hq = be.hi[q][mm * 2 + sx];
                const uint32_t hu[4] = {hq.x, hq.y, hq.z, hq.w};
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    float v0 = x[2 * q + mm][8 * sx + 2 * jj], v1 = x[2 * q + mm][8 * sx + 2 * jj + 1];
                    const uint32_t ph = hu[jj], pl = L.u[8 * mm + 4 * sx + jj];
                    asm("v_fma_mix_f32 %0, %1, -1.0, %0 op_sel_hi:[1,0,0]" : "+v"(v0) : "v"(ph));
                    asm("v_fma_mix_f32 %0, %1, -1.0, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(v1) : "v"(ph));
                    asm("v_fma_mix_f32 %0, %1, -1.0, %0 op_sel_hi:[1,0,0]" : "+v"(v0) : "v"(pl));
                    asm("v_fma_mix_f32 %0, %1, -1.0, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(v1) : "v"(pl));
                    x[2 * q + mm][8 * sx + 2 * jj] = v0;
                    x[2 * q + mm][8 * sx + 2 * jj + 1] = v1;
                }
            }
    }
}

// Difference path: the round's slot layout (bin starts, window tiles and their order, K splits: bin_prefix_role below, behind k_group) is derived by ONE workgroup from
// k_group's counters.  It runs as workgroup 0 of the base pass's launch (k_trunk<.., BASE, DELTA>), whose sample workgroups read none of what it writes.
struct BinPrefixArgs {
    int32_t* cnt;            // Net::d_gcnt
    int32_t* bin_start;      // [225] first slot of a P0's rows
    int32_t* tile_info;      // [tile_cap] tiles, [tile_cap ..) the whole-K launch's order
    uint2* slot_desc;        // the single rows' (request row, fp32 fc0 row)
    const int32_t* singles;
    unsigned long long* work; // Net::d_work
    int n_cu, max_fways, max_wways, part_w_rows, facc_single_base, part_f_rows, nsup_full, bn, use_rects, tile_cap;
};
template <int NT> // NT = threads of the workgroup
__device__ __forceinline__ void bin_prefix_role(unsigned char* lds, const BinPrefixArgs& a);

template <int N, bool FROM_F32, bool BASE = false, bool DELTA = false, bool F16LO = false> // BASE: the base pass of the sibling path (see k_group / k_sib_children below), DELTA: the
                                                                                           // difference path, F16LO: operand rows in the FC0_F16 format (f16 residuals)
__global__ __launch_bounds__(TrunkGeo<N>::WG_THREADS) void k_trunk(const uint32_t* __restrict__ req_ref, const uint32_t* __restrict__ req_aux,
                                                                    const uint64_t* __restrict__ board, const NodeHdr* __restrict__ hdr,
                                                                    const int32_t* __restrict__ d_count, int cap_nodes, const float* __restrict__ in_f32,
                                                                    const uint4* __restrict__ wt, const float* __restrict__ side,
                                                                    uint4* __restrict__ a_out, size_t row_u4, int max_count,
                                                                    const int32_t* __restrict__ row_list, const int32_t* __restrict__ d_nrows,
                                                                    const uint2* __restrict__ groups, float* __restrict__ hscr,
                                                                    const int32_t* __restrict__ d_out_base, uint4* __restrict__ a_base,
                                                                    const int32_t* __restrict__ d_nrows2, uint4* __restrict__ sib2, BinPrefixArgs bp) {
    // BASE && DELTA: workgroup 0 of the launch derives the round's slot layout (bin_prefix_role; bp, unused otherwise) and the sample workgroups are 1 .. gridDim.x - 1.
    // sib2 != NULL (BASE | DELTA only): the base's h and d grids and its residual stream in front of block 2 go to the base slot in the layout
    // k_sib_children2 reads (sib2_grid, sib2_x2) instead of the h grids to hscr.
    // row_list != NULL: the kernel evaluates the request rows row_list[0 .. d_nrows[0]) (the rows outside the sibling runs).
    // BASE: sample i is the BASE position of sibling run groups[i] -- the parent's board with the children's side to move; the
    // depthwise inputs of its three blocks go to hscr[i][blk][pixel][32] and its operand row into every child row of the run
    // (copy path) or, DELTA (difference path), to the compact row i (fc0 of this round's evaluated positions) AND to base slot groups[i].y of
    // a_base (what the children read, this round and while the slot's tag stays: the h grids go to hscr[slot] likewise); with DELTA the rows
    // of a row list go to compact rows d_out_base[0] + i (behind the runs').
    constexpr int BLK_U4 = fmt_blk_u4(F16LO);
    using TG = TrunkGeo<N>;
    constexpr int HW = TG::HW, NW = Geo<N>::NW;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int ROLE_WGS = (BASE && DELTA) ? 1 : 0;
    if constexpr (ROLE_WGS != 0) {
        if (blockIdx.x == 0) { // (the first workgroup dispatched; its tables take the LDS the trunk's weights would)
            bin_prefix_role<TrunkGeo<N>::WG_THREADS>(smem, bp);
            return;
        }
    }
    const int wg = (int)blockIdx.x - ROLE_WGS, n_wg = (int)gridDim.x - ROLE_WGS; // sample workgroup, of how many
    const half8* ldsW = (const half8*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave index: uniform, and the compiler knows it (scalar loads / SALU below)
    const int slot = wv / TG::TILES, tile = wv % TG::TILES;      // sample slot of the workgroup, pixel tile
    const int stid = tid - slot * TG::THREADS;                              // thread index inside the sample
    float* grid = (float*)(smem + TR_WBYTES) + slot * (TG::GRID_BYTES / 4);
    const float* lside = (const float*)(smem + TR_WBYTES + TG::SPW * TG::GRID_BYTES);
    const int h = lane >> 5;
    // ---- one-time: weights, side table, zero halo grid ----
    trunk_lds_prologue<0, BASE && DELTA>(smem, (float*)lside, wt, side, tid); // (the difference path's base pass: LDS-DMA, as k_sib_children2)
    for (int i = tid; i < TG::SPW * (TG::GRID_BYTES / 4); i += blockDim.x) ((float*)(smem + TR_WBYTES))[i] = 0.0f;
    if constexpr (BASE && DELTA) trunk_lds_dma_wait();
    __syncthreads();
    int count = (row_list || BASE) ? d_nrows[0] : d_count[0];
    // BASE with d_nrows2: behind the runs' base positions the same launch evaluates the round's SINGLE rows (row_list, d_nrows2[0] of them: requests
    // outside sibling runs -- their own board, no h grids, no base slot); a launch of their own cost 18 us per round for a handful of rows
    const int n_base = count;
    if (BASE && d_nrows2) count += d_nrows2[0];
    if (count > max_count) count = max_count;
    auto single = [&](int i) { return BASE && i >= n_base; };
    auto rowof = [&](int i) { return BASE ? i : (row_list ? (int)row_list[i] : i); };                 // output row (and request row) of sample i
    auto refof = [&](int i) { return BASE ? (single(i) ? req_ref[row_list[i - n_base]] : req_ref[groups[i].x]) : req_ref[rowof(i)]; }; // BASE: the run's first child
    auto auxof = [&](int i) { return BASE ? 0xFFFFFFFFu : req_aux[rowof(i)]; };
    // depthwise work items are dealt to lanes in the order of the ds_read_b128 lane groups ({0-3,12-15,20-27},
    // {4-11,16-19,28-31} per half): each group then holds two strips 8 pixels apart = 16 distinct 16-B slots of the
    // 256-B bank row (halo-grid row stride 36 floats); lane order gave a 2-way conflict on every window read
    const int l31 = lane & 31;
    const int dw_tid = (stid & ~31) | (l31 < 4 ? l31 : l31 < 12 ? l31 + 4 : l31 < 16 ? l31 - 8 : l31 < 20 ? l31 + 8 : l31 < 28 ? l31 - 4 : l31);
    const int pxl = lane & 31;
    const int px = tile * 32 + pxl;
    const bool valid = px < HW;
    const int pxc = valid ? px : HW - 1;
    const int gi = (pxc / N + 1) * (N + 2) + (pxc % N + 1);
    bool st_ok[4];
    int st_gi[4]; // halo-grid rows of the pixels this lane stores in the operand-row epilogue (pixel 8i + lane/8 of the tile)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = tile * 32 + 8 * i + (lane >> 3);
        const int pc = p < HW ? p : HW - 1;
        st_gi[i] = (pc / N + 1) * (N + 2) + (pc % N + 1);
        st_ok[i] = p < HW;
    }
    const half8* convW = (const half8*)(wt + TR_WBYTES / 16);
    // input decode (board bits -> conv_in operand), lane-constant part: see the sample loop
    const int dec_base = 48 * tile; // first cell of the tile's 48-cell window (m = 96 * tile)
    const int dec_wlo = dec_base >> 6, dec_sh = dec_base & 63;
    uint32_t dec_mask[3][4], dec_shift[3];
    bool dec_plane[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int m = 3 * pxc + c;
        dec_plane[c] = m >= 2 * HW;
        const int rel = dec_plane[c] ? 0 : (m >> 1) - dec_base; // 0..47
        const int piece = ((m & 1) ? 2 : 0) + (rel >= 32 ? 1 : 0); // mine / theirs x low / high piece
        dec_shift[c] = (uint32_t)(rel >= 32 ? rel - 16 : rel);
#pragma unroll
        for (int q = 0; q < 4; ++q) dec_mask[c][q] = piece == q ? 0xFFFFFFFFu : 0u;
    }

    // Inputs of a sample are fetched one sample ahead, BEFORE the output stores of the current sample are
    // issued: vmcnt retires in order, so the (younger) stores never sit in front of a load we wait for and
    // they drain to HBM underneath the next sample's compute.  Barriers below wait for LDS only.
    struct SampleIn {
        uint64_t bb[2 * NW];
        uint32_t aux;
        int turn;
        float f[3];
    };
    auto load_in = [&](int b, uint32_t ref, uint32_t aux, bool own_board) {
        SampleIn in;
        in.aux = aux;
        in.turn = 0;
        in.f[0] = in.f[1] = in.f[2] = 0.0f;
#pragma unroll
        for (int i = 0; i < 2 * NW; ++i) in.bb[i] = 0ULL;
        if (FROM_F32) {
            const float* f = in_f32 + (size_t)b * 3 * HW + 3 * pxc;
            in.f[0] = f[0]; in.f[1] = f[1]; in.f[2] = f[2];
        } else {
            const size_t tn = (size_t)(ref >> 16) * (size_t)cap_nodes + (size_t)(ref & 0xFFFFu);
            size_t tb = tn;
            if (BASE && !own_board) tb = (size_t)(ref >> 16) * (size_t)cap_nodes + (size_t)(((const uint32_t*)hdr)[tn * 4] & 0xFFFFu); // NodeHdr::parent: the board without the child's stone
#pragma unroll
            for (int i = 0; i < 2 * NW; ++i) in.bb[i] = board[tb * (2 * NW) + i];
            in.turn = (int)((((const uint32_t*)hdr)[tn * 4 + 2] >> 16) & 0xFFu); // NodeHdr::turn (byte 10) through a dword: scalar load
        }
        return in;
    };
    // conv_in fragments stay in registers for the whole persistent loop (8 x 4 VGPRs): re-fetching them per sample
    // put 8 loads in front of every sample's first MFMA, and their wait also drained the previous sample's stores
    half8 cwh[4], cwl[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        cwh[m] = convW[m * 64 + lane];
        cwl[m] = convW[(4 + m) * 64 + lane];
    }
    auto lds_barrier = [&]() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    const int b_first = wg * TG::SPW + slot;
    const int b_stride = n_wg * TG::SPW;
    uint32_t ref_n = 0, aux_n = 0xFFFFFFFFu;
    if (!FROM_F32 && b_first < count) { ref_n = refof(b_first); aux_n = auxof(b_first); }
    SampleIn in = load_in(b_first < count ? rowof(b_first) : 0, ref_n, aux_n, single(b_first));

    for (int b0 = wg * TG::SPW; b0 < count; b0 += b_stride) { // uniform trip count over the workgroup (barriers inside)
        const int bi = b0 + slot;
        const bool active = bi < count; // a slot without a sample in the last pass runs along (for the barriers) and stores nothing
        const int b = active ? rowof(bi) : 0;
        const int bi_next = bi + b_stride;
        const bool has_next = bi_next < count;
        const int b_next = has_next ? rowof(bi_next) : 0;
        if (!FROM_F32 && has_next) { ref_n = refof(bi_next); aux_n = auxof(bi_next); } // used at the end of this sample
        // ---- conv_in 1x1 3->128 + bias + lrelu as one 16-deep k-step: k = (f0, f1, f2, 1, 0...) on lane-half 0, where f0..f2 are
        //      the pixel's three input floats in the flat encoder.rs layout ----
        half8 bh, bl;
        if (FROM_F32) {
            float v[8];
            v[0] = h == 0 ? in.f[0] : 0.0f; v[1] = h == 0 ? in.f[1] : 0.0f; v[2] = h == 0 ? in.f[2] : 0.0f; v[3] = h == 0 ? 1.0f : 0.0f;
            v[4] = 0.0f; v[5] = 0.0f; v[6] = 0.0f; v[7] = 0.0f;
            split8(v, bh, bl);
        } else {
            // Board inputs are bits.  The flat layout puts (mine, theirs) of cell m >> 1 at m = 3 px + c (m < 2 HW) and the turn
            // plane behind it, so the 32 pixels of a tile touch the 48 consecutive cells from 48 * tile on: everything up to a
            // 48-bit window of each colour is wave-uniform (scalar unit), and a lane only picks its three bits out of the windows
            // (lane-constant selectors, precomputed) and writes them down as f16 0 / 1 (conv_in_operand).
            uint64_t bb[2 * NW];
#pragma unroll
            for (int i = 0; i < 2 * NW; ++i) bb[i] = in.bb[i];
            const uint32_t aux = in.aux;
            int turn = in.turn, mode = 0;
            if (aux != 0xFFFFFFFFu) { // clone + place_stone(action), Opponent mode (agent.rs:154-158)
                const int action = (int)(aux & 0xFFFFu);
                mode = (int)(aux >> 16) & 1;
                bool occ = false;
#pragma unroll
                for (int i = 0; i < NW; ++i) occ = occ || ((action >> 6) == i && (((bb[i] | bb[NW + i]) >> (action & 63)) & 1ULL));
                if (!occ) {
#pragma unroll
                    for (int i = 0; i < NW; ++i) {
                        const uint64_t bit = (action >> 6) == i ? (1ULL << (action & 63)) : 0ULL;
                        bb[i] |= turn == 0 ? bit : 0ULL;
                        bb[NW + i] |= turn == 0 ? 0ULL : bit;
                    }
                    turn = 1 - turn;
                }
            }
            const int persp = mode == 0 ? turn : 1 - turn; // encoder.rs:24-27
            // 48-bit windows [cell_base, cell_base + 48) of the two colours as seen from `persp`, in two overlapping 32-bit pieces
            // (bits 0..31 and 16..47): a lane's bit index is then a 32-bit extract
            uint64_t wm = 0, wt = 0;
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                const uint64_t mi = persp == 0 ? bb[i] : bb[NW + i], ti = persp == 0 ? bb[NW + i] : bb[i];
                if (i == dec_wlo) { wm |= mi >> dec_sh; wt |= ti >> dec_sh; }
                if (i == dec_wlo + 1 && dec_sh != 0) { wm |= mi << (64 - dec_sh); wt |= ti << (64 - dec_sh); }
            }
            const uint32_t pieces[4] = {(uint32_t)wm, (uint32_t)(wm >> 16), (uint32_t)wt, (uint32_t)(wt >> 16)};
            const uint32_t tbit = turn == 0 ? 1u : 0u; // encoder.rs:34-37: the turn plane is 1 where Black is to move
            uint32_t bits[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t src = (pieces[0] & dec_mask[c][0]) | (pieces[1] & dec_mask[c][1]) | (pieces[2] & dec_mask[c][2]) | (pieces[3] & dec_mask[c][3]);
                const uint32_t bit = (src >> dec_shift[c]) & 1u;
                bits[c] = dec_plane[c] ? tbit : bit;
            }
            bh = conv_in_operand(h, bits[0], bits[1], bits[2]);
            bl = bh; // (unused: the inputs are exact in f16)
        }
        f32x16 x[4];
        conv_in_tile<FROM_F32>(cwh, cwl, bh, bl, x);
        // ---- 3 bottleneck residual blocks ----
#pragma unroll 1
        for (int blk = 0; blk < 3; ++blk) {
            const float* dwt = lside + blk * TR_SIDE_PER_BLOCK;
            const bool to_sib2 = BASE && DELTA && sib2 != nullptr && active && !single(bi) && valid;
            uint4* sb2 = nullptr;
            if (BASE && DELTA) sb2 = sib2 + (size_t)(to_sib2 ? groups[bi].y : 0u) * sib2_slot_u4(N);
            if (to_sib2 && blk == 2) { // the residual stream in front of block 2: what the children's outer ring continues from
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        sb2[sib2_x2(HW, px, m, g, h)] = __builtin_bit_cast(uint4, (f32x4){x[m][4 * g], x[m][4 * g + 1], x[m][4 * g + 2], x[m][4 * g + 3]});
            }
            f32x16 acc;
            { // L0: 1x1 128 -> 32, bias as the initial accumulator.  L0_tile's text, inline: as a call k_trunk's N = 9 fp6 instantiations spill a conv_in fragment
                const half8* W = ldsW + (size_t)blk * TR_FRAGS_PER_BLOCK * 64;
                const float* b0 = lside + blk * TR_SIDE_PER_BLOCK + 9 * NM;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 bv = *(const f32x4*)(b0 + 8 * g + 4 * h);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[4 * g + i] = bv[i];
                }
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = x[ks >> 1][8 * (ks & 1) + j];
                    half8 bh, bl;
                    split8(v, bh, bl);
                    const half8 ah = W[(0 + ks) * 64 + lane], al = W[(8 + ks) * 64 + lane];
                    MFMA3(ah, al, bh, bl, acc);
                }
            }
            float d[16];
            // (no barrier here: a pixel's grid row is written below and was last read -- as depthwise output of the
            //  previous block, or as staging row of the previous sample's operand stores -- by this same lane; the other
            //  waves' window reads of it ended before B3 and their write-backs before B4 of the previous block)
            if (valid) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 o;
                    const f32x2 r0 = lrelu2(acc[4 * g], acc[4 * g + 1]), r1 = lrelu2(acc[4 * g + 2], acc[4 * g + 3]);
                    o[0] = r0[0]; o[1] = r0[1]; o[2] = r1[0]; o[3] = r1[1];
                    *(f32x4*)(grid + gi * GRID_STRIDE + 8 * g + 4 * h) = o;
                    if (to_sib2) sb2[sib2_grid(HW, blk, 0, px, g, h)] = __builtin_bit_cast(uint4, o);
                }
            }
            lds_barrier(); // B2: h of the whole sample is in the halo grid
            if (BASE && active && !single(bi) && !(DELTA && sib2)) { // the base's depthwise input of this block -> scratch: the children's halo rings read it (225 pixels x 8 pieces of 16 B)
                for (int i = stid; i < HW * 8; i += TG::THREADS) {
                    const int p = i >> 3, piece = i & 7;
                    *(uint4*)(hscr + ((size_t)(DELTA ? (int)groups[bi].y : b) * 3 + blk) * (HW * NM) + p * NM + piece * 4) =
                        *(const uint4*)(grid + ((p / N + 1) * (N + 2) + (p % N + 1)) * GRID_STRIDE + piece * 4);
                }
            }
            // depthwise 3x3 SAME (zero halo), no bias.  Work item = (board row, 4-pixel strip, 4-channel
            // group): one 3x6 window of b128 loads serves 4 output pixels; taps in (dy,dx) order.
            f32x4 dout[TG::DW_ITER][TG::SW];
#pragma unroll
            for (int it = 0; it < TG::DW_ITER; ++it) {
                const int item = dw_tid + it * TG::THREADS;
                const int itc = item < TG::DW_ITEMS ? item : 0;
                const int cg = itc & 7, strip = itc >> 3;
                const int y = strip / TG::SPR, x0 = (strip % TG::SPR) * TG::SW;
                const float* gp = grid + (y * (N + 2) + x0) * GRID_STRIDE + 4 * cg;
                f32x4 win[3][TG::SW + 2];
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < TG::SW + 2; ++dx) win[dy][dx] = *(const f32x4*)(gp + (dy * (N + 2) + dx) * GRID_STRIDE);
                f32x4 w9[9];
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) w9[tap] = *(const f32x4*)(dwt + tap * NM + 4 * cg);
#pragma unroll
                for (int p = 0; p < TG::SW; ++p) {
                    f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int tap = 0; tap < 9; ++tap) {
                        const f32x4 hv = win[tap / 3][p + tap % 3];
#pragma unroll
                        for (int c = 0; c < 4; ++c) o[c] += hv[c] * w9[tap][c];
                    }
                    dout[it][p] = o;
                }
            }
            lds_barrier(); // B3: all windows are in registers; the grid can be overwritten in place
#pragma unroll
            for (int it = 0; it < TG::DW_ITER; ++it) {
                const int item = dw_tid + it * TG::THREADS;
                if (item < TG::DW_ITEMS) {
                    const int cg = item & 7, strip = item >> 3;
                    const int y = strip / TG::SPR, x0 = (strip % TG::SPR) * TG::SW;
#pragma unroll
                    for (int p = 0; p < TG::SW; ++p)
                        if (x0 + p < N) *(f32x4*)(grid + ((y + 1) * (N + 2) + x0 + p + 1) * GRID_STRIDE + 4 * cg) = dout[it][p];
                }
            }
            lds_barrier(); // B4: depthwise output of the whole sample is in the grid
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 dv = *(const f32x4*)(grid + gi * GRID_STRIDE + 8 * g + 4 * h);
#pragma unroll
                for (int i = 0; i < 4; ++i) d[4 * g + i] = dv[i];
                if (to_sib2) sb2[sib2_grid(HW, blk, 1, px, g, h)] = __builtin_bit_cast(uint4, dv);
            }
            L1L2_tile(ldsW, lside, h, lane, x, blk, d);
        }
        in = load_in(has_next ? b_next : b, ref_n, aux_n, single(has_next ? bi_next : bi)); // next sample's inputs first (see load_in)
        // ---- fc0 operand row (k_fc0_mx): per (tile, channel half q) one 6-KiB block: f16 hi pieces [pxl 32][piece
        //      (2j+h) 8][16 B] with j = 2*(m&1)+s, then the 64-B residual part per pixel: packed fp6 (e2m3) codes of x - hi and the two E8M0 block scales (entry_fp6_stage)
        //      (the fp6 copy of hi is derived inside k_fc0_mx).  One K=64 super-step of fc0 = one pixel of one block. ----
        //      Stores go through the sample's own halo-grid rows (free between the last depthwise read and the next
        //      sample's first write; a wave touches only its own pixels' interior rows, so no barrier): a lane holds six
        //      16-B pieces of ITS pixel, i.e. a direct store instruction touches 64 different cache lines with 16 B each
        //      (one texture-path cycle per line).  Transposed through LDS, 8 adjacent lanes write one pixel's 128-B run:
        //      8 full lines per instruction.  Three passes of 128 B per pixel: f16 part of q = 0, of q = 1, both residual parts.
        //      (Lanes past the last pixel skip the LDS write; the read-back side then stores the clamped pixel's data into
        //      the pad slots of the row: no branch around the global stores, so the compiler counts them exactly.)
        // BASE: the row is stored into EVERY child row of the run (the rows fc0 reads must exist; k_sib_children then overwrites
        // each child's 7x7 window): `row` = the first child's row, the others follow at the row stride
        uint32_t orow = (uint32_t)b;
        const bool sgl = single(bi);
        if (BASE) orow = DELTA ? (uint32_t)(active ? bi : 0) : (active ? (sgl ? (uint32_t)row_list[bi - n_base] : groups[bi].x) : 0u);
        else if (DELTA && row_list) orow = (uint32_t)(d_out_base[0] + (active ? bi : 0));
        uint4* row = a_out + (size_t)orow * row_u4;
        uint4* row2 = (BASE && DELTA && !sgl) ? a_base + (size_t)(active ? groups[bi].y : 0u) * row_u4 : nullptr; // the base slot
        const int copies = (BASE && !DELTA) ? (active ? (sgl ? 1 : (int)groups[bi].y) : 0) : 1;
        uint4* stage_w = (uint4*)(grid + gi * GRID_STRIDE);          // this lane's pixel row (8 slots of 16 B)
        if constexpr (F16LO) {
            // FC0_F16: four passes of 128 B per pixel through the same staging rows -- per channel half q the f16 hi pieces, then the
            // f16 residual pieces
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                half8 hi8[4], lo8[4];
                entry_f16_pieces(x, q, hi8, lo8);
#pragma unroll
                for (int part = 0; part < 2; ++part) {
                    if (valid) {
#pragma unroll
                        for (int p4 = 0; p4 < 4; ++p4) stage_w[p4 * 2 + h] = __builtin_bit_cast(uint4, part ? lo8[p4] : hi8[p4]);
                    }
                    WAVE_LDS_FENCE();
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const uint4 v = *(const uint4*)(grid + st_gi[i] * GRID_STRIDE + 4 * (lane & 7));
                        if (i == 3) WAVE_LDS_FENCE();
                        if (st_ok[i] && active) {
                            uint4* dst = &row[(size_t)(tile * 2 + q) * BLK_U4 + part * OP_LO_U4 + (8 * i + (lane >> 3)) * 8 + (lane & 7)];
                            if (BASE && !DELTA) for (int c = 0; c < copies; ++c) nt_store(v, dst + (size_t)c * row_u4);
                            else if (DELTA) { *dst = v; if (BASE && row2) row2[dst - row] = v; }
                            else nt_store(v, dst);
                        }
                    }
                }
            }
        } else {
        u32x6 lo6[2];        // fp6 residuals of the lane's 32 values per channel half q
        uint32_t esc[2];     // E8M0 bytes of the two block scales
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            float res[32], amax_v = 0.0f, amax_l = 0.0f;
#pragma unroll
            for (int mm = 0; mm < 2; ++mm)
#pragma unroll
                for (int sx = 0; sx < 2; ++sx) {
                    const uint4 hv = entry_fp6_hi_piece(x, q, mm, sx, res, amax_v, amax_l);
                    if (valid) stage_w[(mm * 2 + sx) * 2 + h] = hv;
                }
            WAVE_LDS_FENCE();
            lo6[q] = entry_fp6_residuals(res, amax_v, amax_l, esc[q]);
            // read back: lanes 8i'..8i'+7 hold the 8 pieces of pixel 8i + i' of the tile
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint4 v = *(const uint4*)(grid + st_gi[i] * GRID_STRIDE + 4 * (lane & 7));
                if (st_ok[i] && active) {
                    uint4* dst = &row[(size_t)(tile * 2 + q) * OP_BLK_U4 + (8 * i + (lane >> 3)) * 8 + (lane & 7)];
                    if (BASE && !DELTA) for (int c = 0; c < copies; ++c) nt_store(v, dst + (size_t)c * row_u4);
                    else if (DELTA) { *dst = v; if (BASE && row2) row2[dst - row] = v; } // (read again right away: by fc0; by the children of the run)
                    else nt_store(v, dst);
                }
            }
            WAVE_LDS_FENCE();
        }
        if (valid) {
#pragma unroll
            for (int q = 0; q < 2; ++q) entry_fp6_stage(stage_w, q, h, lo6[q], esc[q]);
        }
        WAVE_LDS_FENCE();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 v = *(const uint4*)(grid + st_gi[i] * GRID_STRIDE + 4 * (lane & 7));
            const int q = (lane >> 2) & 1;
            if (st_ok[i] && active) {
                uint4* dst = &row[(size_t)(tile * 2 + q) * OP_BLK_U4 + OP_LO_U4 + (8 * i + (lane >> 3)) * 4 + (lane & 3)];
                if (BASE && !DELTA) for (int c = 0; c < copies; ++c) nt_store(v, dst + (size_t)c * row_u4);
                else if (DELTA) { *dst = v; if (BASE && row2) row2[dst - row] = v; }
                else nt_store(v, dst);
            }
        }
        } // (fp6 format)
    }
}

// ===============================================================================================
// OMOK_NET_F16X3: SIBLING requests of a search round (N = 15): k_group, bin_prefix_role, k_trunk<.., BASE>, k_sib_children, fc0 window tiles
// ===============================================================================================
// The K requests a tree contributes to a round are, almost always, children of ONE leaf (tree_kernels.hip: between two backups
// the PUCT descent reaches the same leaf, and a round has no backups except terminal ones; measured over a configs[1] episode:
// runs of 14.4-15.8 siblings at every ply, < 0.2 % of the rows outside runs).  Siblings are positions that differ in one stone,
// and the trunk is local: 1x1 convolutions plus three 3x3 depthwise stages.  A child's trunk activations therefore equal those
// of a shared BASE position (the parent's board with the child's side to move) everywhere outside the 7x7 window around the
// pixel its stone changes (the flat encoder.rs layout puts the stone's float into pixel (2a + 1) / 3).  Per round:
//   k_group          runs of siblings in the request list (first row, length >= SIB_MIN), the rows inside runs, the other rows
//   k_trunk<BASE>    the whole trunk once per run for the base position; the depthwise inputs (h grids) of its three blocks go
//                    to a scratch; its fc0 operand row goes
//                      COPY path        into EVERY child row of the run (the rows a dense fc0 reads must exist);
//                      DIFFERENCE path  once, to full row `run`
//   k_sib_children   per child ONE 7x7 window (49 pixels = two 32-pixel MFMA tiles = a wave pair; four children per workgroup
//                    pass): conv_in and the three blocks on the window only, the depthwise halo ring taken from the base's h
//                    grid of the same block; the window's 49 pixel entries
//                      COPY path        overwrite the base's in the child's row -> dense fc0 as for any other rows;
//                      DIFFERENCE path  minus the base's entries (as fc0 sees them) -> the slot's difference row; fc0 is linear:
//                                       fc0(child) = fc0(full row of the run) + W[window pixels] * difference row, 98 of the 450
//                                       super-steps per child (launch_fc0_delta: k_fc0_mx<EPI_PARTIAL> on the full rows, then
//                                       k_fc0_mx<.., WIN> on tiles of slots that share a window)
//   k_trunk<rows>    the rows outside runs, as before (DIFFERENCE path: into full rows behind the runs')
// COPY path: every pixel goes through the same operations in the same order as in k_trunk (MFMA columns are independent, the
// depthwise taps accumulate in (dy, dx) order, operand-row entries are per pixel), so the rows are BIT-IDENTICAL to a full
// evaluation.  DIFFERENCE path: one more rounding (the quantisation of the difference), |dp| < 1e-4 measured; rounds of fewer than
// 3072 rows stay on the copy path (forward_f16x3).  DESIGN.md 3.3.
#ifndef SIB_WAYS_N
#define SIB_WAYS_N 2 // (round 4, -DSIB_WAYS_N=4 measured on whole configs[1] episodes: 567.2 / 567.9 against 566.5 games/s with 2 -- four slots hit 88 % instead of 86 % of the runs and
                     //  cost 3.5 GB more: not worth it.  Round 24, with a tree's first TWO runs of a round in the slots (k_group): over a configs[1] episode 13.7 % of the runs
                     //  are evaluated in full with 2 slots (17.0 % while only the first run had one), 11.5 % with 4; the benchmark line 635.8 / 633.9 / 637.1 with 2 against
                     //  634.5 / 639.5 / 639.9 games/s with 4, interleaved on one box: the runs do not separate, 2 stays.  At least 2: the two runs never share a way)
#endif
constexpr int SIB_WAYS = SIB_WAYS_N;              // cached base evaluations per game (most recently used leaves of its tree)
static_assert(SIB_WAYS >= 2 && SIB_WAYS <= 16, "k_group gives a tree's first two runs of a round one way each");
constexpr int SIB_MIN = 3;                       // runs shorter than this go to k_trunk (a base pass would not pay)
constexpr int SIB_WIN = 7, SIB_GW = SIB_WIN + 2; // window side, child grid side (window + halo ring)
constexpr int SIB_CGRID_ROWS = SIB_GW * SIB_GW + 1;
constexpr int SIB_CGRID_BYTES = SIB_CGRID_ROWS * GRID_STRIDE * 4; // 11808
constexpr int sib_hb_floats(int n) { return n * n * NM; } // one base h grid in the scratch: [pixel][32]
constexpr int SIB_PAIR_CUT1 = 289, SIB_PAIR_CUT2 = 578, SIB_PAIR_CUT3 = 801; // shares of a workgroup's children per wave pair, cumulative / 1024 (k_sib_children)
// difference path: window bins (window origin (wy0, wx0) in 0..8 each), the single rows as bin SIB_BINS, counters, difference rows
constexpr int SIB_ORG = 15 - SIB_WIN + 1, SIB_BINS = SIB_ORG * SIB_ORG; // 9, 81: bin = wy0 * 9 + wx0 for EVERY board size (N = 9: origins 0..2, 9 bins in use)
constexpr int SIB_CNT_INTS = NET_GCNT_INTS;                                // ints of d_gcnt (net.h: the NET_GCNT_* enum)
constexpr int SIB_WPX = SIB_WIN * SIB_WIN;                                // 49 window pixels = 98 fc0 super-steps
constexpr int SIB_DROW_U4 = SIB_WPX * 2 * 12;                             // 1176 uint4 = 18816 B: [q][w] 128-B f16 parts, [q][w] 64-B residual parts
constexpr int SIB_DLO_U4 = SIB_WPX * 2 * 8;                               // 784: first residual part
constexpr int SIBX_DROW_U4 = SIB_WPX * 2 * 16;                            // FC0_F16: 1568 uint4 = 25088 B: [q][w] 128-B f16 parts, [q][w] 128-B f16 residual parts

__device__ inline void sib_window(int n, int action, int& wy0, int& wx0) { // the 7x7 window (clamped to the n x n board) around the pixel the stone's float lands in
    const int pc = (2 * action + 1) / 3;
    wy0 = pc / n - SIB_WIN / 2;
    wx0 = pc % n - SIB_WIN / 2;
    wy0 = wy0 < 0 ? 0 : (wy0 > n - SIB_WIN ? n - SIB_WIN : wy0);
    wx0 = wx0 < 0 ? 0 : (wx0 > n - SIB_WIN ? n - SIB_WIN : wx0);
}

// cnt = Net::d_gcnt (NET_GCNT_*): runs, rows outside runs, rows inside runs.  sib_rows[i] = descriptor of a row inside a run: (request row, run
// index, node record index t * stride_nodes + node, turn | action << 8); a run's rows are adjacent.
// sib_slot[i] (difference path, else NULL) = net pixel of the child's stone (P0) << 24 | rank of the row among that pixel's rows (any order: a row's
// result does not depend on its slot).
// One wave per tree, GROUP_TREES trees per workgroup: the workgroup counts in LDS and claims its ranges of the global lists with one
// atomic per counter (per-row atomics on 3 + 81 addresses serialised in L2: 0.24 ms per round).
// MATCH (match episodes, Net::grp_*): the games [g_lo, g_hi) only, request rows relative to row_sub[0] (the forward's own list; NULL: 0).
// scan_cnt != NULL (!MATCH, run-loop rounds: no k_scan ran): the games' request counts of this round as k_round left them, dense (0 for a finished game).  The
// workgroup derives what k_scan would have: the first request row of its trees = the counts of all games in front of its first one (every workgroup sums them for
// itself, coalesced: no workgroup waits for another) + the prefix over its own trees, stored to TreeState::req_base of live trees; the workgroup of the last game
// stores the round's total to S.d_count[0] and adds it to evals[0].
constexpr int GROUP_TREES = 16;
template <bool MATCH>
__global__ __launch_bounds__(64 * GROUP_TREES) void k_group(Store S, int side, uint2* __restrict__ groups, int32_t* __restrict__ singles,
                                                             uint4* __restrict__ sib_rows, int32_t* __restrict__ cnt, uint32_t* __restrict__ sib_slot,
                                                             int32_t* __restrict__ tags, uint2* __restrict__ comp, int bn, int do_fill,
                                                             unsigned long long* __restrict__ work, int g_lo, int g_hi, const int32_t* __restrict__ row_sub,
                                                             const int32_t* __restrict__ scan_cnt, unsigned long long* __restrict__ evals) {
    // Difference path (sib_slot != NULL): base slots.  The first TWO runs of a tree (request order) use the game's SIB_WAYS slots (SIB_WAYS g + way), whose
    // content is reused while a tag names the run's parent (a leaf is its tree's expansion target for ~14 rounds).  A second run is, four times in five, the
    // leaf the tree expands NEXT: the old leaf fills up partway through the round's K simulations and the rest of them are children of the new one.  While only
    // the first run had a slot that leaf was evaluated twice, now and as the first run of the following round; with a slot of its own the following round hits
    // (tools/base_cache_sim.py, N = 15, 800 simulations, K = 16, 16 games x 30 plies: 990 of 24 000 tree-rounds hold a second run, 806 of them lead the next round,
    // evaluated runs 3 883 -> 3 082 of 24 990).  One lane decides for both runs: both parents are looked up before a victim is chosen, a miss takes a way the
    // other run does not use (the first run's children read its slot in the launch that writes the second run's base), and the second run's tag goes in front.
    // Runs from the third on (rare) take a slot behind the games', are always evaluated and leave no tag.  comp[] lists the (first request row, slot)
    // pairs to evaluate: the misses and the uncacheable runs, which is what NET_WORK_DIFF_FULL counts.
    constexpr int NP0 = 225, L_P0 = 3, L_FULL = L_P0 + NP0, L_UNC = L_FULL + 1, LC = L_UNC + 1; // [NET_GCNT_RUNS, _SINGLES, _ROWS_IN_RUNS] as in d_gcnt | [L_P0 +] children per net pixel of their stone (P0) | full evaluations, uncacheable runs
    static_assert(NET_GCNT_ROWS_IN_RUNS + 1 == L_P0 && NET_GCNT_UNCACHEABLE == NET_GCNT_FULL_EVALS + 1, "k_group's local counters mirror d_gcnt");
    __shared__ int l_cnt[LC], l_base[LC];
    __shared__ int l_front[GROUP_TREES], l_n[GROUP_TREES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int g = (MATCH ? g_lo : 0) + blockIdx.x * GROUP_TREES + (tid >> 6);
    const int g_end = MATCH ? g_hi : S.games;
    const bool scan = !MATCH && scan_cnt != nullptr;
    if (scan) { // the requests of the games in front of the workgroup's first: a partial sum per wave
        int s = 0;
        for (int i = tid; i < (int)blockIdx.x * GROUP_TREES; i += 64 * GROUP_TREES) s += scan_cnt[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) l_front[tid >> 6] = s;
    }
    if (tid < LC) l_cnt[tid] = 0;
    __syncthreads();
    int n = 0;
    TreeState ts{};
    const int t = side * S.games + (g < g_end ? g : 0);
    const bool live = g < g_end && S.gs[g].alive;
    if (live) {
        ts = S.ts[t];
        n = (int)ts.n_req;
        if (MATCH && row_sub) ts.req_base -= (uint32_t)row_sub[0];
    }
    if (scan) {
        if (lane == 0) l_n[tid >> 6] = n;
        __syncthreads();
        int front = 0, mine = 0, total = 0;
#pragma unroll
        for (int w = 0; w < GROUP_TREES; ++w) {
            front += l_front[w];
            mine += w < (tid >> 6) ? l_n[w] : 0;
            total += l_n[w];
        }
        ts.req_base = (uint32_t)(front + mine);
        if (live && lane == 0) S.ts[t].req_base = ts.req_base;
        if (blockIdx.x == gridDim.x - 1 && tid == 0) {
            S.d_count[0] = front + total;
            if (evals) evals[0] += (unsigned long long)(front + total); // (the evaluation counter of the stats)
        }
    }
    int parent = -1 - lane; // distinct for the lanes beyond the list
    uint32_t tn = 0, ta = 0;
    if (lane < n) {
        const uint32_t node = S.req_node[(size_t)t * KMAX + lane];
        tn = (uint32_t)t * (uint32_t)S.stride_nodes + node;
        if (do_fill) { // k_fill's work (tree_kernels.hip): the dense (tree, node) list in tree order, then simulation order
            S.req_ref[ts.req_base + (uint32_t)lane] = ((uint32_t)t << 16) | node;
            S.req_aux[ts.req_base + (uint32_t)lane] = 0xFFFFFFFFu;
        }
        const NodeHdr hd = S.hdr[tn];
        parent = hd.parent;
        ta = (uint32_t)hd.turn | ((uint32_t)hd.action << 8);
    }
    const int prev = __shfl_up(parent, 1, 64);
    const bool start = lane < n && (lane == 0 || parent != prev);
    const unsigned long long starts = __ballot(start);
    // the run a lane belongs to: its start = highest start bit at or below the lane; its end = the next start bit above (or n)
    const unsigned long long below = starts & ((lane == 63 ? 0ULL : (1ULL << (lane + 1))) - 1ULL);
    const int rs = below ? 63 - __clzll((long long)below) : 0;
    const unsigned long long above = starts & ~((1ULL << rs) | ((1ULL << rs) - 1ULL));
    const int re = above ? __ffsll((long long)above) - 1 : n;
    const int len = re - rs;
    const bool in_run = lane < n && len >= SIB_MIN;
    int gslot = 0, rbase = 0, bin = 0, rank = 0, sidx = 0;
    int bslot = -1, mi = -1, ex = -1; // base slot (>= 0: decided), index in the evaluation list (-1: cache hit), index among the uncacheable runs
    const unsigned long long qual = __ballot(start && len >= SIB_MIN);
    if (start && len >= SIB_MIN) {
        gslot = atomicAdd(&l_cnt[NET_GCNT_RUNS], 1);
        rbase = atomicAdd(&l_cnt[NET_GCNT_ROWS_IN_RUNS], len);
    }
    if (sib_slot && qual) { // (both wave-uniform: the shuffles below are executed by whole waves)
        // The tree's first two qualifying runs, in request order: lane f1 decides for both (the second run's parent comes by shuffle, its way goes back by shuffle).
        const unsigned long long qual2 = qual & (qual - 1ULL);
        const int f1 = __ffsll((long long)qual) - 1, f2 = qual2 ? __ffsll((long long)qual2) - 1 : -1;
        const int p2 = __shfl(parent, f2 < 0 ? f1 : f2, 64);
        int second = -1; // what lane f1 decided for the second run: way | miss << 8
        if (lane == f1) {
            // SIB_WAYS slots per game, most recently used first; a tag = leaf node | slot << 16, -1 = empty (one slot hits 77 % of the
            // runs of a configs[1] episode, two 86 %, four 88 %: the descent alternates between a few leaves while their scores cross)
            const bool two = f2 >= 0 && p2 != parent; // (two runs of ONE leaf with a short run between them share the leaf's base: one lookup, one evaluation)
            int tg[SIB_WAYS], w1 = -1, w2 = -1;
            unsigned used = 0u;
#pragma unroll
            for (int i = 0; i < SIB_WAYS; ++i) {
                tg[i] = tags[SIB_WAYS * g + i];
                used |= tg[i] >= 0 ? 1u << (tg[i] >> 16) : 0u;
            }
            // both lookups come before any victim is chosen: a run that hits keeps its way
#pragma unroll
            for (int i = SIB_WAYS - 1; i >= 0; --i) {
                if (tg[i] >= 0 && (tg[i] & 0xFFFF) == parent) w1 = tg[i] >> 16;
                if (two && tg[i] >= 0 && (tg[i] & 0xFFFF) == p2) w2 = tg[i] >> 16;
            }
            // a miss: the lowest way never used, else the least recently used one -- of the ways the other run does not use in this round (the first run's children
            // read its slot in the launch in which the second run's base is written: the two never share a way)
            auto victim = [&](unsigned taken) {
                const unsigned free_ways = ~(used | taken) & ((1u << SIB_WAYS) - 1u);
                if (free_ways) return __ffs((int)free_ways) - 1;
                int v = 0;
#pragma unroll
                for (int i = 0; i < SIB_WAYS; ++i)
                    if (tg[i] >= 0 && !((taken >> (tg[i] >> 16)) & 1u)) v = tg[i] >> 16;
                return v;
            };
            const bool miss1 = w1 < 0, miss2 = two && w2 < 0;
            if (miss1) {
                w1 = victim(w2 >= 0 ? 1u << w2 : 0u);
                mi = atomicAdd(&l_cnt[L_FULL], 1);
            }
            if (miss2) w2 = victim(1u << w1);
            // tag order: the second run's leaf (the leaf the tree expands now), the first run's, the others in their old order
            int nt[SIB_WAYS], k = 0;
            if (two) nt[k++] = p2 | (w2 << 16);
            nt[k++] = parent | (w1 << 16);
#pragma unroll
            for (int i = 0; i < SIB_WAYS; ++i) {
                const int w = tg[i] >= 0 ? tg[i] >> 16 : -1;
                if (k < SIB_WAYS && w != w1 && (!two || w != w2)) nt[k++] = tg[i];
            }
            for (; k < SIB_WAYS; ++k) nt[k] = -1;
#pragma unroll
            for (int i = 0; i < SIB_WAYS; ++i)
                if (nt[i] != tg[i]) tags[SIB_WAYS * g + i] = nt[i];
            bslot = SIB_WAYS * g + w1;
            second = f2 >= 0 ? (two ? w2 : w1) | (miss2 ? 256 : 0) : -1;
        }
        second = __shfl(second, f1, 64);
        if (start && len >= SIB_MIN && lane != f1) {
            if (lane == f2) {
                bslot = SIB_WAYS * g + (second & 255);
                if (second & 256) mi = atomicAdd(&l_cnt[L_FULL], 1);
            } else { // from the third run on: a slot behind the games', always evaluated, no tag
                ex = atomicAdd(&l_cnt[L_UNC], 1);
                mi = atomicAdd(&l_cnt[L_FULL], 1);
            }
        }
    }
    gslot = __shfl(gslot, rs, 64);
    rbase = __shfl(rbase, rs, 64);
    // Difference path: a run's rows are listed by the COLUMN of their stone's net pixel (then row, then request order) instead of request order.  k_sib_children2's
    // eight waves take eight consecutive entries, and what they read of the run's base slot is the union of their windows: neighbours in this order overlap, so a pass
    // pulls ~28 KB per child through L2 instead of ~35 (the stone's pixel lies in rows 0..9, columns 0..14: the column separates more).  Which wave evaluates a
    // row changes nothing in the row.
    int pos_in_run = lane - rs;
    if (sib_slot) {
        const int pc = (2 * (int)(ta >> 8) + 1) / 3;
        const int key = in_run ? (((pc % 15) * 16 + pc / 15) << 6) | lane : 0x7FFFFFFF;
        int rank_in_run = 0;
        for (int j = 0; j < n; ++j) { // (n = the tree's requests of this round, wave-uniform; a run is at most that long)
            const int other = __shfl(key, (rs + j) & 63, 64);
            rank_in_run += (j < len && other < key) ? 1 : 0;
        }
        if (in_run) pos_in_run = rank_in_run;
    }
    if (in_run) {
        if (sib_slot) {
            // slots are handed out per net PIXEL of the child's stone (P0), not per window bin: a bin's rows are then ordered by P0, and an fc0 window tile
            // only has to walk the window pixels its own rows can differ in (bin_prefix_role: the tile's rectangle)
            bin = (2 * (int)(ta >> 8) + 1) / 3;
            rank = atomicAdd(&l_cnt[L_P0 + bin], 1);
        }
    } else if (lane < n) sidx = atomicAdd(&l_cnt[NET_GCNT_SINGLES], 1);
    __syncthreads();
    if (tid < LC && l_cnt[tid] > 0 && (tid < L_P0 || sib_slot))
        l_base[tid] = atomicAdd(&cnt[tid < L_P0 ? tid : (tid < L_FULL ? NET_GCNT_P0 + (tid - L_P0) : NET_GCNT_FULL_EVALS + (tid - L_FULL))], l_cnt[tid]);
    // executed-work counters of the stats (Net::d_work: never read by a kernel): runs, single rows, rows in runs per path; the runs evaluated in full
    if (tid < L_P0 && l_cnt[tid] > 0) atomicAdd(&work[(sib_slot ? NET_WORK_DIFF : NET_WORK_COPY) + tid], (unsigned long long)l_cnt[tid]);
    if (tid == L_FULL && sib_slot && l_cnt[tid] > 0) atomicAdd(&work[NET_WORK_DIFF_FULL], (unsigned long long)l_cnt[tid]);
    __syncthreads();
    if (start && len >= SIB_MIN) {
        groups[l_base[NET_GCNT_RUNS] + gslot] = make_uint2(ts.req_base + (uint32_t)lane, (uint32_t)len);
        if (sib_slot) {
            if (ex >= 0) bslot = SIB_WAYS * S.games + l_base[L_UNC] + ex;
            if (mi >= 0) comp[l_base[L_FULL] + mi] = make_uint2(ts.req_base + (uint32_t)lane, (uint32_t)bslot);
        }
    }
    bslot = __shfl(bslot, rs, 64);
    if (in_run) {
        const int ri = l_base[NET_GCNT_ROWS_IN_RUNS] + rbase + pos_in_run;
        sib_rows[ri] = make_uint4(ts.req_base + (uint32_t)lane, sib_slot ? (uint32_t)bslot : (uint32_t)(l_base[NET_GCNT_RUNS] + gslot), tn, ta);
        if (sib_slot) sib_slot[ri] = ((uint32_t)bin << 24) | (uint32_t)(l_base[L_P0 + bin] + rank);
    } else if (lane < n) singles[l_base[NET_GCNT_SINGLES] + sidx] = (int32_t)(ts.req_base + (uint32_t)lane);
}

// Difference path: slots.  Every bin's rows get consecutive slots, bins padded to whole 128-sample fc0 tiles (a tile's super-steps are
// its bin's window); the single rows are bin SIB_BINS (no window: their tiles only run the epilogue on their own full row).
// Bins are laid out DEAREST FIRST (round 5): interior bins (one P0 each: the whole 7x7 window differs), edge bins (4 P0s, rectangles of 28 .. 49 pixels), corner bins
// (16 P0s, 16 .. 49 pixels), then a tail of interior bins for the K-split set, the single rows last (sib_bin_at).  The whole-K launch deals its tiles in rounds of n_cu workgroups (position p = round * n_cu + xcd * n_cu / 8 + i, an
// XCD's chunk of a round = consecutive tiles = a few bins' weight slices through one L2), so round 1 holds the full-price tiles and a CU's second tile is a cheap
// one: the 18 % of window pixels the rectangles skip then shorten the launch (in the old corner-first order with an eighth of the tiles per XCD, the XCDs of the interior
// bins ran two full-price tiles per CU and nothing was gained).  T tiles take ceil(T / CUs) rounds of workgroups: the tiles of the last, partial round are instead
// split over K (NET_GCNT_WIN_WAYS ways, fp32 partials + k_win_finish), so that the round costs 1 / ways of a full one.  The split set is made of
// WHOLE bins from the end of the layout (tiles >= NET_GCNT_SPLIT_TILE0): a row's bin -- unlike its slot -- is a function of the position alone, so
// the summation order of a row never depends on the order in which k_group's atomics handed out the slots.
__device__ inline int sib_bin_at(int pos, int bn) { // layout position -> bin: interior bins, edge bins, corner bins, a tail of interior bins, the single rows
    if (pos >= SIB_BINS) return SIB_BINS;
    constexpr int E = SIB_ORG - 2; // 7 edge bins per side, 7 x 7 interior bins
    // the TAIL: small bins (one P0 each) at the end of the layout, so that the K-split set -- whole bins from the end, see below -- can be cut close to the partial round
    // it covers (behind the corner bins it would start up to 55 tiles early).  N = 15: the interior bins of window rows 5..7; N = 9: its only interior bin
    const int head = bn > 9 ? 4 * E : 0;
    auto interior = [&](int i) { return (1 + i / E) * SIB_ORG + 1 + i % E; };
    if (pos < head) return interior(pos);
    pos -= head;
    if (pos < 4 * E) {
        const int sd = pos / E, i = 1 + pos % E;
        return sd == 0 ? i : sd == 1 ? (SIB_ORG - 1) * SIB_ORG + i : sd == 2 ? i * SIB_ORG : i * SIB_ORG + SIB_ORG - 1;
    }
    pos -= 4 * E;
    if (pos < 4) return (pos >> 1) * (SIB_ORG - 1) * SIB_ORG + (pos & 1) * (SIB_ORG - 1);              // corners
    return interior(head + pos - 4);
}
// Round 5: a bin's rows are ordered by the net pixel P0 of their stone (k_group hands out slots per P0), and a child's trunk output differs from its base's only within
// P0 +- 3 CLIPPED TO THE BOARD -- for the 176 of 225 pixels near an edge that is less than the 7x7 window the bin shares (a corner bin collects 16 pixels whose
// regions run from 4x4 to 7x7).  k_sib_children2 writes exact zeros outside a child's own region, so a tile may skip every window pixel outside the union of its rows'
// regions: tile_info carries that rectangle (window coordinates), fc0 walks rect pixels only -- 19 % fewer window super-steps at N = 15, 31 % at N = 9.  Zero pixels
// contribute exact zeros and the rectangle is walked row-major, so a row's sum does not depend on which rectangle its tile got (slots still come from atomics).
// Tiles of the K-split set keep the full window (their split boundaries are positions in the 98 super-steps).
__device__ inline void sib_p0_range(int bn, int o, int& lo, int& hi) { // net-pixel rows (columns) whose 7-wide window starts at origin o
    lo = o == 0 ? 0 : o + SIB_WIN / 2;
    hi = o == bn - SIB_WIN ? bn - 1 : o + SIB_WIN / 2;
}
__host__ __device__ inline void tile_rect(int ti, int& y0, int& y1, int& x0, int& x1) { // the rectangle of window pixels in a tile_info word (bin_prefix_role packs it)
    y0 = (ti >> 16) & 7; y1 = (ti >> 19) & 7; x0 = (ti >> 22) & 7; x1 = (ti >> 25) & 7;
}
constexpr int BP_MAXT = 2048; // bin_prefix_role: tiles of the whole-K launch it can order by cost (more: layout order)
// ONE workgroup of NT threads (every loop strides by NT): workgroup 0 of the base pass's launch (k_trunk<.., BASE, DELTA>, 512 or 384 threads).  It reads k_group's
// counters (P0 counts, singles, full evaluations) and the single rows' list, all complete at the launch's start; it writes the derived counters of d_gcnt, bin_start,
// tile_info, the single rows' slot_desc and d_work -- none of which the launch's sample workgroups touch (they read d_comp, d_singles and the two counters
// NET_GCNT_FULL_EVALS / _SINGLES); the first readers (k_sib_children2: bin_start; the fc0 launches) come behind the kernel boundary.
// lds: the workgroup's dynamic LDS, of which the tables take the first BinPrefixLds bytes.
struct BinPrefixLds {
    int hist[64], s_area;
    int tile0[SIB_BINS + 2], binc[SIB_BINS + 1], bcnt[SIB_BINS + 1], order[SIB_BINS + 1], start_at[SIB_BINS + 2], p0c[225], p0o[225], s_split, s_ntiles;
    unsigned char cost[BP_MAXT];
};
static_assert(sizeof(BinPrefixLds) <= TrunkGeo<9>::LDS_BYTES && sizeof(BinPrefixLds) <= TrunkGeo<15>::LDS_BYTES, "the role's tables come out of the trunk workgroup's LDS");
template <int NT>
__device__ __forceinline__ void bin_prefix_role(unsigned char* lds, const BinPrefixArgs& a) {
    int32_t* __restrict__ cnt = a.cnt;
    int32_t* __restrict__ bin_start = a.bin_start;
    int32_t* __restrict__ tile_info = a.tile_info;
    uint2* __restrict__ slot_desc = a.slot_desc;
    const int32_t* __restrict__ singles = a.singles;
    unsigned long long* __restrict__ work = a.work;
    const int n_cu = a.n_cu, max_fways = a.max_fways, max_wways = a.max_wways, part_w_rows = a.part_w_rows, facc_single_base = a.facc_single_base,
              part_f_rows = a.part_f_rows, nsup_full = a.nsup_full, bn = a.bn, use_rects = a.use_rects, tile_cap = a.tile_cap;
    BinPrefixLds& L = *(BinPrefixLds*)lds;
    unsigned char* cost = L.cost;
    int *hist = L.hist, &s_area = L.s_area, *tile0 = L.tile0, *binc = L.binc, *bcnt = L.bcnt, *order = L.order, *start_at = L.start_at, *p0c = L.p0c, *p0o = L.p0o,
        &s_split = L.s_split, &s_ntiles = L.s_ntiles;
    const int tid = threadIdx.x;
    for (int i = tid; i < 225; i += NT) p0c[i] = i < bn * bn ? cnt[NET_GCNT_P0 + i] : 0;
    if (tid < 64) hist[tid] = 0;
    if (tid == 0) s_area = 0;
    __syncthreads();
    int c = 0, oy = 0, ox = 0, ylo = 0, yhi = -1, xlo = 0, xhi = -1;
    if (tid < SIB_BINS) {
        oy = tid / SIB_ORG; ox = tid % SIB_ORG;
        if (oy <= bn - SIB_WIN && ox <= bn - SIB_WIN) {
            sib_p0_range(bn, oy, ylo, yhi);
            sib_p0_range(bn, ox, xlo, xhi);
        }
        for (int y = ylo; y <= yhi; ++y)
            for (int x = xlo; x <= xhi; ++x) { p0o[y * bn + x] = c; c += p0c[y * bn + x]; } // (offset of the P0's rows inside the bin: row-major P0 order)
    } else if (tid == SIB_BINS) c = cnt[NET_GCNT_SINGLES];
    if (tid <= SIB_BINS) { bcnt[tid] = c; binc[tid] = (c + GT_BS - 1) / GT_BS; order[tid] = sib_bin_at(tid, bn); } // (tiles per bin and the layout order in parallel:
    __syncthreads();                                                                                                     //  the serial part below only adds)
    if (tid < 64) { // wave 0: exclusive scan of the bins' tile counts in layout order (82 positions = two passes of 64 lanes), then the split point
        int carry = 0, ntiles = 0;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int pos = half * 64 + tid, b = pos <= SIB_BINS ? order[pos] : 0, v = pos <= SIB_BINS ? binc[b] : 0;
            int incl = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int u = __shfl_up(incl, o, 64);
                if (tid >= o) incl += u;
            }
            if (pos <= SIB_BINS) { tile0[b] = carry + incl - v; start_at[pos] = carry + incl - v; }
            carry += __shfl(incl, 63, 64);
        }
        ntiles = carry;
        if (tid == 0) start_at[SIB_BINS + 1] = ntiles;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        int t_split = ntiles - (ntiles < n_cu ? ntiles : ntiles % n_cu); // first tile of the partial round ...
        if (t_split < ntiles) {                                           // ... moved down to the start of its bin: the largest bin start <= t_split
            int best = 0;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int pos = half * 64 + tid, st = pos <= SIB_BINS ? start_at[pos] : 0;
                best = st <= t_split && st > best ? st : best;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { const int u = __shfl_xor(best, o, 64); best = u > best ? u : best; }
            t_split = best;
        }
      if (tid == 0) {
        int ways = ntiles > t_split ? n_cu / (ntiles - t_split) : 1;
        if (ways > max_wways) ways = max_wways;
        if (ntiles > t_split && ways > part_w_rows / ((ntiles - t_split) * GT_BS)) ways = part_w_rows / ((ntiles - t_split) * GT_BS); // (partials slab)
        while (ways > 1 && (ways - 1) * ((2 * SIB_WPX + ways - 1) / ways) >= 2 * SIB_WPX) --ways; // (no empty split of the 98 super-steps)
        if (ways < 2) { ways = 1; t_split = ntiles; }
        cnt[NET_GCNT_FULL_ROWS] = cnt[NET_GCNT_FULL_EVALS] + cnt[NET_GCNT_SINGLES]; // positions evaluated in full this round: runs without a cached base, then the single rows
        const int ftiles = (cnt[NET_GCNT_FULL_ROWS] + GT_BS - 1) / GT_BS; // fc0 of the full rows: K split so that one round of workgroups covers it;
        int fways = ftiles > 0 ? n_cu / ftiles : 1;              // partials [split][row < ftiles * 128]: as many ways as the slab holds
        const int fcap = (ftiles > 0 ? ftiles : 1) * GT_BS;
        if (fways > part_f_rows / fcap) fways = part_f_rows / fcap;
        fways = fways < 1 ? 1 : (fways > max_fways ? max_fways : fways);
        // no empty split: with ceil(nsup / ways) super-steps each, the last of `ways` splits must still start inside K (N = 9: 162 super-steps
        // in 30 ways of 6 would leave splits 27..29 empty -- their workgroups would stream weights from beyond the matrix)
        while (fways > 1 && (fways - 1) * ((nsup_full + fways - 1) / fways) >= nsup_full) --fways;
        cnt[NET_GCNT_FULL_WAYS] = fways;
        cnt[NET_GCNT_FULL_STRIDE] = fcap;
        cnt[NET_GCNT_WIN_TILES] = ntiles;
        cnt[NET_GCNT_SPLIT_TILE0] = t_split;
        cnt[NET_GCNT_WIN_WAYS] = ways;
        s_split = t_split;
        s_ntiles = ntiles;
      }
    }
    __syncthreads();
    constexpr int FULL_RECT = (0 << 16) | ((SIB_WIN - 1) << 19) | (0 << 22) | ((SIB_WIN - 1) << 25);
    if (tid < SIB_BINS) {
        cnt[NET_GCNT_BINS + tid] = c; // (the bin's total: diagnostics)
        const int off = tile0[tid] * GT_BS;
        for (int y = ylo; y <= yhi; ++y)
            for (int x = xlo; x <= xhi; ++x) bin_start[y * bn + x] = off + p0o[y * bn + x]; // first slot of the P0's rows
    }
    // one thread per tile: its bin (layout position by a search over start_at), its live slots, its rectangle = union of the regions (P0 +- 3, clipped to the board) of
    // the P0s with rows in the tile, in window coordinates; cost = the rectangle's pixels
    const int ntiles = s_ntiles, t_split = s_split;
    for (int T = tid; T < ntiles; T += NT) {
        int pos = 0;
        for (int step = 64; step > 0; step >>= 1)
            if (pos + step <= SIB_BINS && start_at[pos + step] <= T) pos += step;
        const int b = order[pos], t = T - tile0[b], cb = bcnt[b];
        const int lo = t * GT_BS, hi = cb - lo < GT_BS ? cb : lo + GT_BS;
        int rect = FULL_RECT, area = b < SIB_BINS ? SIB_WPX : 1;
        if (use_rects && b < SIB_BINS && T < t_split) {
            const int by = b / SIB_ORG, bx = b % SIB_ORG;
            int y0, y1, x0, x1;
            sib_p0_range(bn, by, y0, y1);
            sib_p0_range(bn, bx, x0, x1);
            int ry0 = SIB_WIN, ry1 = -1, rx0 = SIB_WIN, rx1 = -1;
            for (int y = y0; y <= y1; ++y)
                for (int x = x0; x <= x1; ++x) {
                    const int n = p0c[y * bn + x], o = p0o[y * bn + x];
                    if (n > 0 && o < hi && o + n > lo) {
                        const int a0 = (y - 3 < 0 ? 0 : y - 3) - by, a1 = (y + 3 > bn - 1 ? bn - 1 : y + 3) - by;
                        const int c0 = (x - 3 < 0 ? 0 : x - 3) - bx, c1 = (x + 3 > bn - 1 ? bn - 1 : x + 3) - bx;
                        ry0 = a0 < ry0 ? a0 : ry0; ry1 = a1 > ry1 ? a1 : ry1;
                        rx0 = c0 < rx0 ? c0 : rx0; rx1 = c1 > rx1 ? c1 : rx1;
                    }
                }
            if (ry1 >= ry0 && rx1 >= rx0 && ry0 >= 0 && rx0 >= 0 && ry1 < SIB_WIN && rx1 < SIB_WIN) {
                rect = (ry0 << 16) | (ry1 << 19) | (rx0 << 22) | (rx1 << 25);
                area = (ry1 - ry0 + 1) * (rx1 - rx0 + 1);
            }
        }
        tile_info[T] = b | ((hi - lo) << 8) | rect;
        if (T < t_split && T < BP_MAXT) { cost[T] = (unsigned char)area; atomicAdd(&hist[area], 1); }
        if (b < SIB_BINS) atomicAdd(&s_area, area); // (window pixels this round's tiles walk: the stats' executed-work count)
    }
    __syncthreads();
    if (tid == 0) {
        atomicAdd(&work[NET_WORK_WIN_PIXELS], (unsigned long long)s_area);
        atomicAdd(&work[NET_WORK_WIN_TILES], (unsigned long long)(ntiles - binc[SIB_BINS]));
        atomicAdd(&work[NET_WORK_FULL_TILES], (unsigned long long)((cnt[NET_GCNT_FULL_ROWS] + GT_BS - 1) / GT_BS));
    }
    // Order of the whole-K launch (tiles below t_split).  With rectangles a tile costs 16 .. 49 window pixels, and a launch of two rounds of workgroups takes as long as
    // its slowest CU's two tiles: in layout order the CUs of the interior bins ran two full-price tiles and the 18 % of skipped work bought nothing.  The tiles are
    // sorted by cost, descending and STABLY (a bin's tiles stay together: the workgroups of one XCD stream its weight slice together) -- a counting sort, one wave
    // matching equal costs with ballots chunk by chunk -- and the launch deals positions in rounds of 8 x 32 workgroups, XCD x taking chunk x of even rounds and chunk
    // 7 - x of odd ones (k_fc0_*): the CU with a full-price tile gets a cheap second one.  Best case with two whole tiles per CU: 49 + 35 of 98.
    {
        int* tile_order = tile_info + tile_cap;
        __syncthreads();
        const int n = t_split <= BP_MAXT ? t_split : 0;
        if (tid == 0) cnt[NET_GCNT_TILE_ORDER] = tile_cap;
        if (tid < 64) {
            // first position of every cost bucket, dearest first: lane a keeps bucket a's running start in a register
            const int hv = hist[63 - tid];
            int incl = hv;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int u = __shfl_up(incl, o, 64);
                if (tid >= o) incl += u;
            }
            int my_start = __shfl(incl - hv, 63 - tid, 64);
            const unsigned long long lt = (1ULL << tid) - 1ULL;
            for (int c0 = 0; c0 < n; c0 += 64) {
                const int T = c0 + tid, cT = T < n ? (int)cost[T] : -1;
                unsigned long long todo = __ballot(T < n);
                int pos = 0;
                while (todo) { // one pass per distinct cost of the chunk (a few: neighbouring tiles have neighbouring P0s)
                    const int lead = __ffsll((long long)todo) - 1, lc = __shfl(cT, lead, 64);
                    const unsigned long long m = __ballot(cT == lc);
                    const int base = __shfl(my_start, lc, 64);
                    if (cT == lc) pos = base + __popcll(m & lt);
                    if (tid == lc) my_start += __popcll(m);
                    todo &= ~m;
                }
                if (T < n) tile_order[pos] = T;
            }
        }
        for (int T = n + tid; T < t_split; T += NT) tile_order[T] = T; // (n = 0: more tiles than the table holds)
    }
    const int nsing = cnt[NET_GCNT_SINGLES], s0 = tile0[SIB_BINS] * GT_BS;
    for (int i = tid; i < nsing; i += NT) slot_desc[s0 + i] = make_uint2((uint32_t)singles[i], (uint32_t)(facc_single_base + i)); // (fp32 fc0 row index)
}

// tiles of the K-split set (see bin_prefix_role): partials in split order + the slot's full row + bias, LeakyReLU, hi|lo operand row
__global__ __launch_bounds__(256) void k_win_finish(const float* __restrict__ part, size_t cap_rows, const int32_t* __restrict__ cnt,
                                                    const int32_t* __restrict__ tile_info, const uint2* __restrict__ slot_desc,
                                                    const float* __restrict__ facc, const float* __restrict__ bias, uint4* __restrict__ out_split,
                                                    size_t out_row_u4) {
    const int nt = cnt[NET_GCNT_WIN_TILES], t0 = cnt[NET_GCNT_SPLIT_TILE0], ways = cnt[NET_GCNT_WIN_WAYS];
    if (ways < 2) return;
    cap_rows = (size_t)(nt - t0) * GT_BS; // the split set's slots, densely
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; // (local slot, mt 16, s 2, h 2)
    const size_t local = i >> 6;
    const int tile = t0 + (int)(local / GT_BS);
    if (tile >= nt || (int)(local % GT_BS) >= ((tile_info[tile] >> 8) & 0xFF)) return;
    const uint2 dsc = slot_desc[(size_t)t0 * GT_BS + local];
    const int piece = (int)(i & 63), mt = piece >> 2, sx = (piece >> 1) & 1, h = piece & 1;
    const int n0 = 32 * mt + 16 * sx + 4 * h; // j = 0..3 -> n0 + j ; j = 4..7 -> n0 + 8 + (j - 4)
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.0f;
    for (int sp = 0; sp < ways; ++sp) {
        const float* p = part + ((size_t)sp * cap_rows + local) * NF + n0;
        const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] += a[j]; v[4 + j] += b[j]; }
    }
    const float* fa = facc + (size_t)dsc.y * NF + n0;
    const f32x4 fa0 = *(const f32x4*)fa, fa1 = *(const f32x4*)(fa + 8);
    const f32x4 ba = *(const f32x4*)(bias + n0), bb = *(const f32x4*)(bias + n0 + 8);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = lrelu((v[j] + fa0[j]) + ba[j]); v[4 + j] = lrelu((v[4 + j] + fa1[j]) + bb[j]); }
    half8 hi, lo;
    split8(v, hi, lo);
    uint4* row = out_split + (size_t)dsc.x * out_row_u4 + (size_t)(2 * mt + sx) * 4;
    row[h] = *(const uint4*)&hi;
    row[2 + h] = *(const uint4*)&lo;
}

struct FaccReduceArgs { // what the reduce needs beyond d_gcnt; part == NULL: the launch does not carry the role
    const float* part;
    float* facc;
    const uint2* comp;
    int facc_single_base;
};
// full-row partial sums of fc0 -> one fp32 row per full row, in split order: split 0 first, then splits 1 .. nsplit - 1
// (evaluated row i: i < nmiss -> the base slot comp[i].y, else the single row i - nmiss behind the base slots)
// The arithmetic, once: the calling thread takes the items first, first + step, ... (an item = four features of one evaluated row).  Called by k_facc_reduce and, on the
// product's path, by every workgroup of k_sib_children2 (a role of that launch).  A thin round has up to 64 splits and at most one item per thread, so its
// time is the chain of loads of one item: eight splits' loads are issued together, the adds keep the order.
__device__ __forceinline__ void facc_reduce_items(const float* __restrict__ part, const int32_t* __restrict__ d_nrows, const int32_t* __restrict__ d_nsplit,
                                                  float* __restrict__ facc, const uint2* __restrict__ comp, const int32_t* __restrict__ d_nmiss, int facc_single_base,
                                                  size_t first, size_t step) {
    const size_t total = (size_t)d_nrows[0] * (NF / 4);
    const int nsplit = d_nsplit[0], nmiss = d_nmiss[0];
    const size_t split_floats = (size_t)d_nsplit[NET_GCNT_FULL_STRIDE - NET_GCNT_FULL_WAYS] * NF; // (d_nsplit = d_gcnt + NET_GCNT_FULL_WAYS)
    for (size_t i = first; i < total; i += step) {
        const float* p = part + i * 4;
        f32x4 a = *(const f32x4*)p;
        int sp = 1;
        for (; sp + 8 <= nsplit; sp += 8) {
            f32x4 b[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) b[u] = *(const f32x4*)(p + (size_t)(sp + u) * split_floats);
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] += b[u][j];
        }
        for (; sp < nsplit; ++sp) {
            const f32x4 b = *(const f32x4*)(p + (size_t)sp * split_floats);
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] += b[j];
        }
        const int row = (int)(i / (NF / 4));
        const size_t dst = row < nmiss ? (size_t)comp[row].y : (size_t)(facc_single_base + (row - nmiss));
        *(f32x4*)(facc + dst * NF + (i % (NF / 4)) * 4) = a;
    }
}
// (a launch of its own where the children kernel does not carry the role: k_sib_children<DELTA> behind omok_debug_set_children_kernel, and the TPROF instantiation)
__global__ __launch_bounds__(256) void k_facc_reduce(const float* __restrict__ part, const int32_t* __restrict__ d_nrows, const int32_t* __restrict__ d_nsplit,
                                                     float* __restrict__ facc, const uint2* __restrict__ comp, const int32_t* __restrict__ d_nmiss, int facc_single_base) {
    facc_reduce_items(part, d_nrows, d_nsplit, facc, comp, d_nmiss, facc_single_base, (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

// DELTA (difference path): a_out holds the FULL rows (one per run, written by k_trunk<BASE | DELTA>); the child's window entries are
// stored as DIFFERENCES to the base's entries (dequantised: f16 hi + fp6 residual * 2^scale, exactly what fc0 will multiply), in the
// same entry format, into the child's slot row of d_rows: fc0(child) = fc0(base row) + W[window] * difference row.
template <bool DELTA, bool F16LO = false, int N = 15> // F16LO: operand / difference rows in the FC0_F16 format (f16 residuals)
__global__ __launch_bounds__(512) void k_sib_children(const uint64_t* __restrict__ board, const uint4* __restrict__ wt, const float* __restrict__ side,
                                                      uint4* __restrict__ a_out, size_t row_u4, const uint4* __restrict__ sib_rows,
                                                      const int32_t* __restrict__ d_cnt, const float* __restrict__ hscr,
                                                      const uint32_t* __restrict__ sib_slot, const int32_t* __restrict__ bin_start,
                                                      uint4* __restrict__ d_rows, uint2* __restrict__ slot_desc,
                                                      unsigned long long* __restrict__ /* (k_sib_children2's profile buffer: the two kernels share a launch signature) */) {
    constexpr int BLK_U4 = fmt_blk_u4(F16LO);
    constexpr int DROW_U4 = F16LO ? SIBX_DROW_U4 : SIB_DROW_U4;
    constexpr int SIB_HB_FLOATS = sib_hb_floats(N);
    constexpr int SWW = 4; // depthwise strips of the 7-wide window: 4 | 3 pixels
    constexpr int NW = Geo<N>::NW;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const half8* ldsW = (const half8*)smem;
    float* grid = (float*)(smem + TR_WBYTES);                                       // four child grids
    const float* lside = (const float*)(smem + TR_WBYTES + 4 * SIB_CGRID_BYTES);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, l31 = lane & 31;
    trunk_lds_prologue(smem, (float*)lside, wt, side, tid);
    for (int i = tid; i < SIB_CGRID_BYTES; i += blockDim.x) grid[i] = 0.0f; // (4 grids x 11808 / 4 floats)
    // A child = a wave pair, and everything a pair writes in LDS is its own (child grid, staging rows, board words): the barriers below
    // are PAIR barriers (a flag per wave in LDS, the LDS executes a wave's accesses in order), not workgroup barriers.  The four pairs
    // then need not march in step -- they are started a quarter of a pass apart, so that the two waves of a SIMD (pairs p and p + 2) are
    // half a pass apart: one is in its matrix phases while the other reads windows or waits for memory.
    __shared__ volatile int pbar[8]; // (a static LDS object: through a pointer into `smem` the accesses became FLAT instructions, whose
                                     //  waits also drain every outstanding global store and load)
    if (tid < 8) pbar[tid] = 0;
    __syncthreads();
    typedef volatile __attribute__((address_space(3))) int* lds_flag_t; // (an LDS-typed pointer: captured in the lambda as a generic one it is flat again)
    const lds_flag_t flag_mine = (lds_flag_t)(volatile int*)&pbar[wv], flag_mate = (lds_flag_t)(volatile int*)&pbar[wv ^ 1];
    int pbar_k = 0;
    auto bar_post = [&]() { // "my LDS accesses so far are done"
        ++pbar_k;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) *flag_mine = pbar_k;
    };
    auto bar_wait = [&]() { // until the mate has posted as often as this wave
        while (__builtin_amdgcn_readfirstlane(*flag_mate) < pbar_k) __builtin_amdgcn_s_sleep(1);
        asm volatile("" ::: "memory");
    };
    auto lds_barrier = [&]() { bar_post(); bar_wait(); };
    for (int i = 0; i < (wv >> 1); ++i) __builtin_amdgcn_s_sleep(118); // (64 clocks per unit: a quarter of a ~30 k-cycle pass per pair index)
    const int nsib = d_cnt[NET_GCNT_ROWS_IN_RUNS];
    const half8* convW = (const half8*)(wt + TR_WBYTES / 16);
    half8 cwh[4], cwl[4]; // conv_in fragments: fetched again at the end of every pass (load_conv_w)
    load_conv_w(convW, lane, cwh, cwl);
    // wave pair = child, wave parity = window tile
    const int pair = wv >> 1, wt2 = wv & 1, ptid = tid & 127;
    const int c_w = 32 * wt2 + l31;            // window pixel of this lane, row-major in the 7x7 window
    const bool c_valid = c_w < SIB_WIN * SIB_WIN;
    const int c_wc = c_valid ? c_w : SIB_WIN * SIB_WIN - 1;
    const int c_wy = c_wc / SIB_WIN, c_wx = c_wc % SIB_WIN;
    const int c_gi = (c_wy + 1) * SIB_GW + (c_wx + 1);
    float* cgrid = grid + pair * (SIB_CGRID_BYTES / 4);

    // operand-row entries of the tile's pixels (staging and stores as in k_trunk's epilogue): channel half q of the lane's pixel staged at `stage_w`, then
    // the pixel `rp` whose 8 pieces lanes 8i..8i+7 read back from `rd_rows[i]` is stored at its place in `row`
    auto store_rows = [&](const f32x16 (&x)[4], uint4* row, bool lane_valid, float* stage_row, const int (&rd_gi)[4], const int (&rd_px)[4],
                          const bool (&rd_ok)[4], float* gbase) {
        uint4* stage_w = (uint4*)stage_row;
        if constexpr (F16LO) { // four passes of 128 B per pixel: per channel half q the f16 hi pieces, then the f16 residual pieces
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                half8 hi8[4], lo8[4];
                entry_f16_pieces(x, q, hi8, lo8);
#pragma unroll
                for (int part = 0; part < 2; ++part) {
                    if (lane_valid) {
#pragma unroll
                        for (int p4 = 0; p4 < 4; ++p4) stage_w[p4 * 2 + h] = __builtin_bit_cast(uint4, part ? lo8[p4] : hi8[p4]);
                    }
                    WAVE_LDS_FENCE();
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const uint4 v = *(const uint4*)(gbase + rd_gi[i] * GRID_STRIDE + 4 * (lane & 7));
                        if (i == 3) WAVE_LDS_FENCE();
                        if (rd_ok[i]) {
                            if (DELTA) nt_store(v, &row[part * SIB_DLO_U4 + (q * SIB_WPX + rd_px[i]) * 8 + (lane & 7)]);
                            else nt_store(v, &row[(size_t)((rd_px[i] >> 5) * 2 + q) * BLK_U4 + part * OP_LO_U4 + (rd_px[i] & 31) * 8 + (lane & 7)]);
                        }
                    }
                }
            }
            return;
        }
        u32x6 lo6[2];
        uint32_t esc[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            float res[32], amax_v = 0.0f, amax_l = 0.0f;
#pragma unroll
            for (int mm = 0; mm < 2; ++mm)
#pragma unroll
                for (int sx = 0; sx < 2; ++sx) {
                    const uint4 hv = entry_fp6_hi_piece(x, q, mm, sx, res, amax_v, amax_l);
                    if (lane_valid) stage_w[(mm * 2 + sx) * 2 + h] = hv;
                }
            WAVE_LDS_FENCE();
            lo6[q] = entry_fp6_residuals(res, amax_v, amax_l, esc[q]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint4 v = *(const uint4*)(gbase + rd_gi[i] * GRID_STRIDE + 4 * (lane & 7));
                if (rd_ok[i]) { // (DELTA: rd_px = the window pixel index, row = the slot's difference row)
                    if (DELTA) nt_store(v, &row[(q * SIB_WPX + rd_px[i]) * 8 + (lane & 7)]);
                    else nt_store(v, &row[(size_t)((rd_px[i] >> 5) * 2 + q) * OP_BLK_U4 + (rd_px[i] & 31) * 8 + (lane & 7)]);
                }
            }
            WAVE_LDS_FENCE();
        }
        if (lane_valid) {
#pragma unroll
            for (int q = 0; q < 2; ++q) entry_fp6_stage(stage_w, q, h, lo6[q], esc[q]);
        }
        WAVE_LDS_FENCE();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 v = *(const uint4*)(gbase + rd_gi[i] * GRID_STRIDE + 4 * (lane & 7));
            const int q = (lane >> 2) & 1;
            if (rd_ok[i]) {
                if (DELTA) nt_store(v, &row[SIB_DLO_U4 + (q * SIB_WPX + rd_px[i]) * 4 + (lane & 3)]);
                else nt_store(v, &row[(size_t)((rd_px[i] >> 5) * 2 + q) * OP_BLK_U4 + OP_LO_U4 + (rd_px[i] & 31) * 4 + (lane & 3)]);
            }
        }
    };

    // A child's descriptor and board words are fetched ONE PASS AHEAD (a dependent pair of loads: their latency runs under the
    // current pass), its halo ring ONE BLOCK ahead.
    f32x16 x[4];
    // ... and inside the workgroup every PAIR takes its own contiguous part of that range and walks it at its own pace: pairs share nothing but
    // read-only LDS, and the waves launched first (pairs 0, 1) get the issue slots of their SIMDs first -- in lockstep the workgroup ran at
    // the pace of pairs 2, 3 (2.42 M cycles per launch against 2.01 M for pair 0).  The parts are sized by those speeds (SIB_PAIR_CUT / 1024).
    constexpr int pass_stride = 1;
    const int per_wg = (nsib + (int)gridDim.x - 1) / (int)gridDim.x;
    const int wg_begin = (int)blockIdx.x * per_wg < nsib ? (int)blockIdx.x * per_wg : nsib, wg_end = wg_begin + per_wg < nsib ? wg_begin + per_wg : nsib;
    const int cut_lo = pair == 0 ? 0 : pair == 1 ? SIB_PAIR_CUT1 : pair == 2 ? SIB_PAIR_CUT2 : SIB_PAIR_CUT3;
    const int cut_hi = pair == 0 ? SIB_PAIR_CUT1 : pair == 1 ? SIB_PAIR_CUT2 : pair == 2 ? SIB_PAIR_CUT3 : 1024;
    const int e_begin = wg_begin + (int)(((long long)(wg_end - wg_begin) * cut_lo) >> 10), e_end = wg_begin + (int)(((long long)(wg_end - wg_begin) * cut_hi) >> 10);
    auto entry_of = [&](int e0) { return e0 < e_end ? e0 : (e_begin < nsib ? e_begin : 0); }; // this pair's child in the pass at e0
    auto fetch_desc = [&](int e0) { return sib_rows[entry_of(e0)]; };
    auto fetch_slot = [&](int e0) { return DELTA ? sib_slot[entry_of(e0)] : 0u; };
    auto fetch_word = [&](const uint4& ent) { // lanes 0..7: the child's board words
        uint64_t word = 0ULL;
        if (lane < 2 * NW) word = board[(size_t)ent.z * (2 * NW) + lane];
        return word;
    };
    auto window_of = [&](const uint4& ent, int& wy0, int& wx0) { sib_window(N, (int)((ent.w >> 8) & 0xFFu), wy0, wx0); }; // NodeHdr::action: the child's stone
    auto ring_fetch = [&](const float* hb, int blk, int wy0, int wx0, uint4 (&ring)[2]) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = ptid + 128 * u, cell = e >> 3, piece = e & 7; // ring cell 0..31: top row 9, bottom row 9, left 7, right 7
            int gy, gx;
            if (cell < 9) { gy = 0; gx = cell; }
            else if (cell < 18) { gy = SIB_GW - 1; gx = cell - 9; }
            else if (cell < 25) { gy = cell - 17; gx = 0; }
            else { gy = cell - 24; gx = SIB_GW - 1; }
            const int by = wy0 + gy - 1, bx = wx0 + gx - 1;
            ring[u] = make_uint4(0u, 0u, 0u, 0u);
            if (by >= 0 && by < N && bx >= 0 && bx < N) ring[u] = *(const uint4*)(hb + (size_t)blk * SIB_HB_FLOATS + (by * N + bx) * NM + piece * 4);
        }
    };
    int ring_off[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int e = ptid + 128 * u, cell = e >> 3, piece = e & 7;
        const int gy = cell < 9 ? 0 : cell < 18 ? SIB_GW - 1 : cell < 25 ? cell - 17 : cell - 24;
        const int gx = cell < 9 ? cell : cell < 18 ? cell - 9 : cell < 25 ? 0 : SIB_GW - 1;
        ring_off[u] = (gy * SIB_GW + gx) * GRID_STRIDE + piece * 4;
    }
    BaseEntry be; // DELTA: the base's operand entries of this lane's pixel, fetched behind the last depthwise and subtracted from the finished residual stream
    uint4 ring[2];
    int wy0 = 0, wx0 = 0; // the current child's window
    const float* hb = hscr;
    // L0 -> child grid (+ halo ring) -> depthwise over the window -> d
    auto block_front = [&](int blk, float (&d)[16], bool fetch_next_ring) {
        const float* dwt = lside + blk * TR_SIDE_PER_BLOCK;
        f32x16 acc;
        L0_tile(ldsW, lside, h, lane, x, blk, acc);
        if (c_valid) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 o;
                const f32x2 r0 = lrelu2(acc[4 * g], acc[4 * g + 1]), r1 = lrelu2(acc[4 * g + 2], acc[4 * g + 3]);
                o[0] = r0[0]; o[1] = r0[1]; o[2] = r1[0]; o[3] = r1[1];
                *(f32x4*)(cgrid + c_gi * GRID_STRIDE + 8 * g + 4 * h) = o;
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) *(uint4*)(cgrid + ring_off[u]) = ring[u]; // halo ring <- the base's h of this block (zero outside the board)
        lds_barrier(); // B2
        if (fetch_next_ring) ring_fetch(hb, blk + 1, wy0, wx0, ring);
        // depthwise over the 7x7 window: (row, strip of 4 | 3 pixels, 4-channel group) = 112 items for the pair's 128 threads
        f32x4 dout[SWW];
        const int item = ptid < 7 * 2 * 8 ? ptid : 0;
        const int cg = item & 7, strip = item >> 3;
        const int y = strip >> 1, x0 = (strip & 1) * SWW;
        {
            const float* gp = cgrid + (y * SIB_GW + x0) * GRID_STRIDE + 4 * cg;
            f32x4 win[3][SWW + 2];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < SWW + 2; ++dx) win[dy][dx] = *(const f32x4*)(gp + (dy * SIB_GW + dx) * GRID_STRIDE);
            f32x4 w9[9];
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) w9[tap] = *(const f32x4*)(dwt + tap * NM + 4 * cg);
            bar_post(); // B3, first half: this wave's window reads have returned; the arithmetic runs under the mate's
#pragma unroll
            for (int p = 0; p < SWW; ++p) {
                f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const f32x4 hv = win[tap / 3][p + tap % 3];
#pragma unroll
                    for (int c = 0; c < 4; ++c) o[c] += hv[c] * w9[tap][c];
                }
                dout[p] = o;
            }
        }
        bar_wait(); // B3, second half: the grid can be overwritten in place
        if (ptid < 7 * 2 * 8) {
#pragma unroll
            for (int p = 0; p < SWW; ++p)
                if (x0 + p < SIB_WIN) *(f32x4*)(cgrid + ((y + 1) * SIB_GW + x0 + p + 1) * GRID_STRIDE + 4 * cg) = dout[p];
        }
        lds_barrier(); // B4
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 dv = *(const f32x4*)(cgrid + c_gi * GRID_STRIDE + 8 * g + 4 * h);
#pragma unroll
            for (int i = 0; i < 4; ++i) d[4 * g + i] = dv[i];
        }
    };
    // A workgroup takes a CONTIGUOUS range of the rows (a run's children are adjacent: the 16 children of a run are four consecutive
    // passes of one workgroup, so the base's h grids and operand row come from HBM once and from this XCD's L2 afterwards; dealt
    // round-robin, a run's children went to four workgroups on four XCDs: 2.9 GB of fetches per round for 0.7 GB of data)
    uint4 ent_c = fetch_desc(e_begin), ent_n = fetch_desc(e_begin + pass_stride);
    uint32_t slot_c = fetch_slot(e_begin), slot_n = fetch_slot(e_begin + pass_stride);
    uint64_t word_c = fetch_word(ent_c);
    window_of(ent_c, wy0, wx0);
    ring_fetch(hscr + (size_t)ent_c.y * 3 * SIB_HB_FLOATS, 0, wy0, wx0, ring);
    for (int e0 = e_begin; e0 < e_end; e0 += pass_stride) { // one child per pass and pair; uniform over the pair
        const bool act = e0 < e_end;
        const uint4 ent = ent_c;
        const int crow = (int)ent.x;
        hb = hscr + (size_t)ent.y * 3 * SIB_HB_FLOATS;
        const int turn = (int)(ent.w & 0xFFu);
        window_of(ent, wy0, wx0);
        const int q = (wy0 + c_wy) * N + (wx0 + c_wx);                                      // this lane's board pixel
        int slot = 0;
        if (DELTA) slot = bin_start[slot_c >> 24] + (int)(slot_c & 0xFFFFFFu);
        uint4* crow_p = DELTA ? d_rows + (size_t)slot * DROW_U4 : a_out + (size_t)crow * row_u4;
        uint64_t* cw = (uint64_t*)(cgrid + (SIB_CGRID_ROWS - 1) * GRID_STRIDE) + wt2 * 8; // the child's 8 board words: the grid's pad row, one copy per wave
        if (lane < 2 * NW) cw[lane] = word_c;
        // the next pass's board words (its descriptor arrived a pass ago) and the descriptor of the pass after that
        const uint64_t word_n = fetch_word(ent_n);
        const uint4 ent_nn = fetch_desc(e0 + 2 * pass_stride);
        const uint32_t slot_nn = fetch_slot(e0 + 2 * pass_stride);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        uint32_t bits[3];
        input_bits<N>(cw, turn, q, bits);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        {
            const half8 bq = conv_in_operand(h, bits[0], bits[1], bits[2]);
            conv_in_tile<false>(cwh, cwl, bq, bq, x);
        }
        float d[16];
#pragma unroll 1
        for (int blk = 0; blk < 2; ++blk) {
            block_front(blk, d, true);
            L1L2_tile(ldsW, lside, h, lane, x, blk, d);
        }
        block_front(2, d, false);
        if (DELTA) base_fetch<F16LO>(be, a_out + (size_t)ent.y * row_u4, q, h);
        L1L2_tile(ldsW, lside, h, lane, x, 2, d);
        { // the window's 49 pixel entries: over the copied base row, or (DELTA) as differences into the slot's row
            int rd_gi[4], rd_px[4];
            bool rd_ok[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int w = 32 * wt2 + 8 * i + (lane >> 3);
                asm volatile("" : "+v"(w)); // (opaque: the store addresses are a few adds per pass; hoisted out of the loop as lane-constant
                                            //  64-bit offsets they were spilled, and every reload's wait drained the stores in flight)
                const int wc = w < SIB_WPX ? w : SIB_WPX - 1;
                rd_gi[i] = (wc / SIB_WIN + 1) * SIB_GW + (wc % SIB_WIN + 1);
                rd_px[i] = DELTA ? wc : (wy0 + wc / SIB_WIN) * N + (wx0 + wc % SIB_WIN);
                rd_ok[i] = w < SIB_WPX && act;
            }
            if (DELTA) {
                if constexpr (F16LO) base_sub_f16lo(x, be, a_out + (size_t)ent.y * row_u4, q, h);
                else base_subtract(x, be);
                if (act && wt2 == 0 && lane == 0) slot_desc[slot] = make_uint2((uint32_t)crow, ent.y);
            }
            // the next pass's first halo ring before this pass's stores queue up behind it
            window_of(ent_n, wy0, wx0);
            ring_fetch(hscr + (size_t)ent_n.y * 3 * SIB_HB_FLOATS, 0, wy0, wx0, ring);
            store_rows(x, crow_p, c_valid, cgrid + c_gi * GRID_STRIDE, rd_gi, rd_px, rd_ok, cgrid);
        }
        load_conv_w(convW, lane, cwh, cwl);
        ent_c = ent_n;
        ent_n = ent_nn;
        slot_c = slot_n;
        slot_n = slot_nn;
        word_c = word_n;
        // (no barrier here: the staging rows a wave read back are its own pixels' rows, the board words its own copy; the mate's next
        //  accesses to this wave's rows are window reads behind B2 of the next pass)
    }
}

// ===============================================================================================
// k_sib_children2: the children of the difference path, ONE WAVE PER CHILD, windows that grow with the blocks
// ===============================================================================================
// A child differs from its base position in one input pixel P0, so its trunk activations differ from the base's only inside P0's
// 3x3 / 5x5 / 7x7 neighbourhood after block 0 / 1 / 2.  k_sib_children evaluates the whole 7x7 window (two 32-pixel tiles = a wave pair)
// through every block; here ONE 32-lane tile holds the 5x5 window (clamped to the board, nested in the 7x7 one) through conv_in, blocks 0
// and 1 and the first layer of block 2, and only block 2's last two layers run on both the 5x5 tile and the 24 pixels of the outer ring:
// 200 MFMAs per child instead of 340, no pair barriers (everything in LDS is the wave's own), two children per SIMD.  The depthwise uses
// its linearity: d_child = d_base + dw(h_child - h_base), where the difference is non-zero only inside the 5x5 tile -- so the tile's LDS
// grid is 25 cells without a halo, and the base pass stores its h AND d grids and its residual stream in front of block 2 (for the ring)
// pixel-major in the piece order of the accumulators (sib2_grid, sib2_x2).  Results are within rounding of k_sib_children's (a different summation order in the
// depthwise) and need not be bit-identical -- on the rows the tests compare they are, every layer boundary re-quantising to ~22 bits -- so the difference path
// is tolerance-checked; the copy path (rows bit-identical to a full evaluation by construction) keeps k_sib_children.
// conv_in and block 0's L0 are not computed here: a pixel's three input bits select one of eight rows of the conv tables (k_conv_tables, once per commit; copied to
// LDS in the prologue), which hold the bits conv_in_tile / L0_tile give for that input -- 168 MFMAs per child, and no conv_in fragments to keep or fetch again.
constexpr int V2_TW = 5, V2_TPX = V2_TW * V2_TW;          // tile window side, pixels
constexpr int V2_RING = SIB_WPX - V2_TPX;                 // 24
constexpr int V2_ZERO_CELL = 32, V2_WORD_CELL = 33;       // cells 0..31: tile grid / staging rows
constexpr int V2_CELLS = 34;
constexpr int V2_WAVE_FLOATS = V2_CELLS * GRID_STRIDE;
constexpr int V2_TAB_OFF = TR_WBYTES + TR_SIDE_FLOATS * 4 + 8 * V2_WAVE_FLOATS * 4; // the conv tables, behind the waves' cells
constexpr int V2_LDS = V2_TAB_OFF + CT_FLOATS * 4;
static_assert(V2_TAB_OFF % 16 == 0, "the conv tables are read as b128");
static_assert(V2_LDS <= 160 * 1024, "k_sib_children2 LDS");
#define OL() ({ int lq_ = lane; asm volatile("" : "+v"(lq_)); lq_; })
#define TILE_A(LQ) (((LQ) & 31) < V2_TPX ? ((LQ) & 31) : V2_TPX - 1)
#define RING_B(LQ) (((LQ) & 31) < V2_RING ? ((LQ) & 31) : V2_RING - 1)
// F16LO: the BASE's operand rows are in the FC0_F16 format; OUT_F16: so are the difference rows written here.  <true, ..., false> is the FC0_MIXED format:
// full rows with f16 residuals, difference rows with block-scaled fp6 residuals.
constexpr int TP_STAMPS = 32, TP_LAUNCHES = 128; // TPROF's per-workgroup stamps: behind the 32 phase sums, a ring of 128 launches
template <bool F16LO, int N, bool TPROF = false, bool OUT_F16 = F16LO> // TPROF (OMOK_SIB_PROF=2, timing only): shader-clock cycles per phase of waves 0 and 5, summed over their passes, into tprof[]
__global__ __launch_bounds__(512) void k_sib_children2(const uint64_t* __restrict__ board, const uint4* __restrict__ wt, const float* __restrict__ side,
                                                       uint4* __restrict__ a_out, size_t row_u4, const uint4* __restrict__ sib_rows,
                                                       const int32_t* __restrict__ d_cnt, const uint4* __restrict__ sib2,
                                                       const uint32_t* __restrict__ sib_slot, const int32_t* __restrict__ bin_start,
                                                       uint4* __restrict__ d_rows, uint2* __restrict__ slot_desc, unsigned long long* __restrict__ tprof,
                                                       const uint4* __restrict__ conv_tab, const FaccReduceArgs fr) {
    unsigned long long tp_acc[12] = {}, tp_last = 0;
    auto TP = [&](int phase) { // (phase = what ended here)
        if (TPROF) {
            const unsigned long long now = __builtin_readcyclecounter();
            tp_acc[phase] += now - tp_last;
            tp_last = now;
        }
    };
    constexpr int DROW_U4 = OUT_F16 ? SIBX_DROW_U4 : SIB_DROW_U4;
    constexpr int HW = N * N, NW = Geo<N>::NW;
    constexpr size_t SLOT_U4 = sib2_slot_u4(N);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const half8* ldsW = (const half8*)smem;
    const float* lside = (const float*)(smem + TR_WBYTES);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* wgrid = (float*)(smem + TR_WBYTES + TR_SIDE_FLOATS * 4) + wv * V2_WAVE_FLOATS; // this wave's cells
    const int h = lane >> 5;
    // TPROF, round 25: per launch and workgroup the constant-rate clock (100 MHz) at entry, behind the prologue's barrier and at the end of its last wave, and the prologue's
    // shader-clock cycles -> tprof[TP_STAMPS + ((launch % TP_LAUNCHES) * workgroups + workgroup) * 4 ..]; launch = a ticket from tprof[31] / workgroups
    unsigned long long tp_t0 = 0, tp_c0 = 0;
    if (TPROF) { tp_t0 = wall_clock64(); tp_c0 = __builtin_readcyclecounter(); }
    // Block 0's L0 fragments (hi[8] | lo[8], the first 16 of the block) stay out of the copy: block 0's L0 comes from the conv table, and the two L0_tile calls below take
    // blk1 and blk2 (L1L2_tile reads fragments 16..35 of its block)
    trunk_lds_prologue<16 * 64, true>(smem, (float*)lside, wt, side, tid);
    for (int i = tid; i < 8 * V2_WAVE_FLOATS; i += blockDim.x) ((float*)(smem + TR_WBYTES + TR_SIDE_FLOATS * 4))[i] = 0.0f;
    for (int i = tid; i < CT_FLOATS / 4; i += blockDim.x) ((uint4*)(smem + V2_TAB_OFF))[i] = conv_tab[i];
    const float* ltab = (const float*)(smem + V2_TAB_OFF); // conv tables: T0 at 0, T1 at CT_T1_OFF
    // Round 6: the children of a workgroup are handed out from a counter in LDS instead of every wave taking every eighth entry.  The second wave of a SIMD (waves 4..7)
    // runs ~15 % slower than the first (issue arbitration favours the older wave: profiles/r05_children_store_order.txt, item 7), so with equal shares waves 0..3 end early
    // and the others finish alone; handed out on demand, all eight end together.  A child's arithmetic does not depend on the wave that takes it: same bits.
    __shared__ int s_next_entry;
    if (tid == 0) {
        const int nsib0 = d_cnt[NET_GCNT_ROWS_IN_RUNS], per0 = (nsib0 + (int)gridDim.x - 1) / (int)gridDim.x;
        const int wb0 = (int)blockIdx.x * per0 < nsib0 ? (int)blockIdx.x * per0 : nsib0;
        s_next_entry = wb0 + 16; // (entries wb0 .. wb0 + 15: the waves' first two passes)
    }
    __shared__ unsigned long long* s_tp_rec;
    if (TPROF && tid == 0) {
        s_tp_rec = tprof + TP_STAMPS + ((atomicAdd(&tprof[31], 1ULL) / gridDim.x % TP_LAUNCHES) * gridDim.x + blockIdx.x) * 4;
        s_tp_rec[2] = 0; // (the waves' ends: atomicMax below)
    }
    trunk_lds_dma_wait();
    __syncthreads(); // (the only workgroup barrier: from here on a wave touches read-only LDS and its own cells)
    if (TPROF && tid == 0) {
        s_tp_rec[0] = tp_t0;
        s_tp_rec[1] = wall_clock64();
        s_tp_rec[3] = __builtin_readcyclecounter() - tp_c0;
    }
    // Role of this launch (round 25): the full rows' fc0 partials -> facc, this workgroup's grid-stride share, once.  The full-row fc0 ran in the launch before; nothing in this
    // launch reads facc or writes the partials, and the first readers of facc (the window-tile launch, k_win_finish) come behind the kernel boundary: no workgroup waits.
    // Items go to the launch's waves 64 at a time, workgroup after workgroup, and inside a workgroup to waves 4..7 first (they wait below): a thin round's few items
    // (256 games: 512 waves' worth) lie on two waves of EVERY workgroup instead of on all waves of the first 64.
    if (fr.part)
        facc_reduce_items(fr.part, d_cnt + NET_GCNT_FULL_ROWS, d_cnt + NET_GCNT_FULL_WAYS, fr.facc, fr.comp, d_cnt + NET_GCNT_FULL_EVALS, fr.facc_single_base,
                          ((size_t)((wv + 4) & 7) * gridDim.x + blockIdx.x) * 64 + lane, (size_t)gridDim.x * blockDim.x);
    for (int i = 0; i < (wv >> 2); ++i) __builtin_amdgcn_s_sleep(120); // the two waves of a SIMD (w, w + 4) start about half a pass apart
    const int nsib = d_cnt[NET_GCNT_ROWS_IN_RUNS];

    // difference-row entries of a tile's pixels, in the layout of k_sib_children<DELTA>'s (staging rows = this wave's cells 0..31)
    // `far`: this lane's pixel lies outside the child's own region (P0 +- 3, clipped to the board -- at an edge that is less than the 7x7 window its bin shares): there the child
    // equals its base, and the lane stores EXACT zeros instead of the base row's quantisation remainder (~2^-22 of the activation), so that an fc0 window tile may skip the pixel
    // or not (bin_prefix_role: the tile's rectangle) without changing a bit of the row's sum.
    auto store_rows = [&](const f32x16 (&x)[4], uint4* row, bool lane_valid, const int (&rd_px)[4], const bool (&rd_ok)[4], bool far) {
        const int lq = OL();
        uint4* stage_w = (uint4*)(wgrid + (lq & 31) * GRID_STRIDE);
        int rd_gi[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) rd_gi[i] = 8 * i + (lq >> 3);
        if constexpr (OUT_F16) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                half8 hi8[4], lo8[4];
                entry_f16_pieces(x, q, hi8, lo8);
#pragma unroll
                for (int part = 0; part < 2; ++part) {
                    if (lane_valid) {
#pragma unroll
                        for (int p4 = 0; p4 < 4; ++p4) stage_w[p4 * 2 + h] = far ? make_uint4(0u, 0u, 0u, 0u) : __builtin_bit_cast(uint4, part ? lo8[p4] : hi8[p4]);
                    }
                    WAVE_LDS_FENCE();
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const uint4 v = *(const uint4*)(wgrid + rd_gi[i] * GRID_STRIDE + 4 * (lane & 7));
                        if (i == 3) WAVE_LDS_FENCE();
                        if (rd_ok[i]) nt_store(v, &row[part * SIB_DLO_U4 + (q * SIB_WPX + rd_px[i]) * 8 + (lane & 7)]);
                    }
                }
            }
            return;
        }
        u32x6 lo6[2];
        uint32_t esc[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            float res[32], amax_v = 0.0f, amax_l = 0.0f;
#pragma unroll
            for (int mm = 0; mm < 2; ++mm)
#pragma unroll
                for (int sx = 0; sx < 2; ++sx) {
                    const uint4 hv = entry_fp6_hi_piece(x, q, mm, sx, res, amax_v, amax_l);
                    if (lane_valid) stage_w[(mm * 2 + sx) * 2 + h] = far ? make_uint4(0u, 0u, 0u, 0u) : hv;
                }
            WAVE_LDS_FENCE();
            lo6[q] = entry_fp6_residuals(res, amax_v, amax_l, esc[q]);
            if (far) lo6[q] = (u32x6){0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint4 v = *(const uint4*)(wgrid + rd_gi[i] * GRID_STRIDE + 4 * (lane & 7));
                if (rd_ok[i]) nt_store(v, &row[(q * SIB_WPX + rd_px[i]) * 8 + (lane & 7)]);
            }
            WAVE_LDS_FENCE();
        }
        if (lane_valid) {
#pragma unroll
            for (int q = 0; q < 2; ++q) entry_fp6_stage(stage_w, q, h, lo6[q], esc[q]);
        }
        WAVE_LDS_FENCE();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 v = *(const uint4*)(wgrid + rd_gi[i] * GRID_STRIDE + 4 * (lane & 7));
            const int q = (lane >> 2) & 1;
            if (rd_ok[i]) nt_store(v, &row[SIB_DLO_U4 + (q * SIB_WPX + rd_px[i]) * 4 + (lane & 3)]);
        }
        WAVE_LDS_FENCE();
    };
    BaseEntry be; // the base's operand entries of this lane's pixel
    // base_fetch's text as a lambda of this kernel: called as the shared function, the fp6 instantiations no longer keep the entry's loads in flight under L1L2_tile
    // (their counted vmcnt waits in base_subtract become one wait) and measured 1 % slower
    auto base_fetch_here = [&](const uint4* frow, int px) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const uint4* bp = frow + (size_t)((px >> 5) * 2 + q) * fmt_blk_u4(F16LO);
#pragma unroll
            for (int p4 = 0; p4 < 4; ++p4) be.hi[q][p4] = bp[(px & 31) * 8 + p4 * 2 + h];
            if (F16LO) continue;
            const uint4* lp = bp + OP_LO_U4 + (px & 31) * 4;
            const uint4 l4 = lp[h];
            const uint2 l2 = ((const uint2*)(lp + 2))[h];
            be.lo[q] = (u32x6){l4.x, l4.y, l4.z, l4.w, l2.x, l2.y};
            be.sc[q] = ((const uint16_t*)(lp + 3))[h];
        }
    };

    f32x16 x[4];
    // every wave walks its own contiguous part of the workgroup's contiguous range (a run's children are adjacent: its base comes
    // from HBM once and from this XCD's L2 afterwards)
    const int per_wg = (nsib + (int)gridDim.x - 1) / (int)gridDim.x;
    const int wg_begin = (int)blockIdx.x * per_wg < nsib ? (int)blockIdx.x * per_wg : nsib, wg_end = wg_begin + per_wg < nsib ? wg_begin + per_wg : nsib;
    // (equal shares: the in-kernel counters show waves 4..7 18 % slower per child than the four launched first, but shares of 134 .. 146 / 1024 for waves 0..3
    //  measured the same as 128: A-B builds, 144.7 - 148.8 ms of trunk kernels per three plies with no order in them)
    // the 8 waves take consecutive entries: a run's ~15 siblings are in flight together on ONE CU, and what one wave pulled into this XCD's L2 the others find there
    // (FETCH_SIZE per launch -30 % against contiguous shares per wave, same time: profiles/r04_children_traffic_experiments.txt)
    constexpr int ESTR = 8;
    const int e_begin = wg_begin + wv, e_end = wg_end;
    auto entry_of = [&](int e0) { return e0 < e_end ? e0 : (e_begin < e_end ? e_begin : 0); };
    auto fetch_word = [&](const uint4& ent) {
        uint64_t word = 0ULL;
        if (lane < 2 * NW) word = board[(size_t)ent.z * (2 * NW) + lane];
        return word;
    };
    uint4 ent_c = sib_rows[entry_of(e_begin)], ent_n = sib_rows[entry_of(e_begin + ESTR)];
    uint32_t slot_c = sib_slot[entry_of(e_begin)], slot_n = sib_slot[entry_of(e_begin + ESTR)];
    uint64_t word_c = fetch_word(ent_c);
    int e_nn_keep = 0;
    int e_next = e_begin + ESTR; // entry of the next pass (its descriptor is in ent_n); the one after that comes from the counter
    for (int e0 = e_begin; e0 < e_end; e0 = e_next, e_next = e_nn_keep) {
        if (TPROF) tp_last = __builtin_readcyclecounter();
        // lane "constants" (tile pixel (ty, tx) of the 5x5 window, ring index, depthwise strip item) are derived again in every phase from an opaque
        // copy of the lane index (OL): hoisted out of the loop or to the top of the pass, they and the addresses built on them were spilled to scratch
        const uint4 ent = ent_c;
        const int crow = (int)ent.x;
        const int turn = (int)(ent.w & 0xFFu);
        // windows: 7x7 around P0 clamped to the board (the difference row's), the 5x5 tile clamped likewise (nested in it)
        const int pc = (2 * (int)((ent.w >> 8) & 0xFFu) + 1) / 3, py = pc / N, pxx = pc % N;
        int wy0, wx0;
        sib_window(N, (int)((ent.w >> 8) & 0xFFu), wy0, wx0);
        int vy0 = py - V2_TW / 2, vx0 = pxx - V2_TW / 2;
        vy0 = vy0 < 0 ? 0 : (vy0 > N - V2_TW ? N - V2_TW : vy0);
        vx0 = vx0 < 0 ? 0 : (vx0 > N - V2_TW ? N - V2_TW : vx0);
        const int oy = vy0 - wy0, ox = vx0 - wx0; // 0..2: where the tile sits in the 7x7 window
        int bpxA; // this lane's board pixel in the tile
        {
            const int tA = TILE_A(OL());
            bpxA = (vy0 + tA / V2_TW) * N + vx0 + tA % V2_TW;
        }
        // ring pixel `r` of the 7x7 window (those outside the tile): oy rows above, 2 - oy below, then per tile row ox pixels left, 2 - ox right
        auto ring_at = [&](int r, int& wy, int& wx) {
            if (r < 2 * SIB_WIN) {
                const int fr = r >= SIB_WIN ? 1 : 0;
                wx = r - SIB_WIN * fr;
                wy = fr < oy ? fr : fr + V2_TW;
            } else {
                const int r2 = r - 2 * SIB_WIN, s = r2 & 1;
                wy = oy + (r2 >> 1);
                wx = s < ox ? s : s + V2_TW;
            }
        };
        int bpxB; // ... and on the ring
        {
            int wyB, wxB;
            ring_at(RING_B(OL()), wyB, wxB);
            bpxB = (wy0 + wyB) * N + wx0 + wxB;
        }
        const int slot = bin_start[slot_c >> 24] + (int)(slot_c & 0xFFFFFFu);
        uint4* crow_p = d_rows + (size_t)slot * DROW_U4;
        const uint4* sb = sib2 + (size_t)ent.y * SLOT_U4;
        const uint4* frow = a_out + (size_t)ent.y * row_u4;
        // block 0's pieces of the base (h at P0 only, d): asked for first, so that their way from L2 passes under the input bits and the table reads (nothing else is left
        // between the top of the pass and their use: block 0's L0, whose MFMAs covered it, is a table row now)
        uint4 hb0[4], db0[4];
        {
            const bool p0 = (OL() & 31) == (py - vy0) * V2_TW + (pxx - vx0);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                hb0[g] = make_uint4(0u, 0u, 0u, 0u);
                if (p0) hb0[g] = sb[sib2_grid(HW, 0, 0, bpxA, g, h)];
                db0[g] = sb[sib2_grid(HW, 0, 1, bpxA, g, h)];
            }
        }
        uint64_t* cw = (uint64_t*)(wgrid + V2_WORD_CELL * GRID_STRIDE);
        if (lane < 2 * NW) cw[lane] = word_c;
        const uint64_t word_n = fetch_word(ent_n);
        int e_nn = 0;
        if (lane == 0) e_nn = atomicAdd(&s_next_entry, 1);
        e_nn = __builtin_amdgcn_readfirstlane(e_nn);
        e_nn_keep = e_nn;
        const uint4 ent_nn = sib_rows[entry_of(e_nn)];
        const uint32_t slot_nn = sib_slot[entry_of(e_nn)];
        WAVE_LDS_FENCE();
        uint32_t bits[3];
        input_bits<N>(cw, turn, bpxA, bits);
        const int pat = (int)(bits[0] | bits[1] << 1 | bits[2] << 2);
        { // conv_in of this lane's pixel: the row of its input pattern in the conv table (what conv_in_tile computes from these bits, bit for bit)
            const float* t0 = ltab + pat * CT_T0_STRIDE + 4 * h;
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 v = *(const f32x4*)(t0 + 32 * m + 8 * g);
#pragma unroll
                    for (int i = 0; i < 4; ++i) x[m][4 * g + i] = v[i];
                }
        }
        TP(0);
        // h_child - h_base of the tile -> the wave's cells; `hb` / `db`: the base's h and d pieces of this lane's pixel
        auto grid_write = [&](const f32x16& acc, const uint4 (&hb)[4]) {
            const int lq = OL(), tA = TILE_A(lq);
            if ((lq & 31) < V2_TPX) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 b = __builtin_bit_cast(f32x4, hb[g]);
                    const f32x2 r0 = lrelu2(acc[4 * g], acc[4 * g + 1]), r1 = lrelu2(acc[4 * g + 2], acc[4 * g + 3]);
                    f32x4 o;
                    o[0] = r0[0] - b[0]; o[1] = r0[1] - b[1]; o[2] = r1[0] - b[2]; o[3] = r1[1] - b[3];
                    *(f32x4*)(wgrid + tA * GRID_STRIDE + 8 * g + 4 * h) = o;
                }
            }
            WAVE_LDS_FENCE();
        };
        float d[16];
        // depthwise of the difference over the 5x5 tile (zero outside it) + the base's depthwise output: item = (tile row, 4-channel group), one 3x5 window of
        // b128 reads serves the row's 5 pixels; rows outside the tile get zero weights; outputs in place, then every lane takes its pixel's 16 channels
        auto strip_dw = [&](const float* dwt, const uint4 (&db)[4]) {
            {
                const int lq = OL();
                const int sy = (lq >> 3) < V2_TW ? (lq >> 3) : V2_TW - 1, scg = lq & 7; // lanes >= 40 run along
                const bool s_act = (lq >> 3) < V2_TW;
                f32x4 dout[V2_TW];
#pragma unroll
                for (int p = 0; p < V2_TW; ++p) dout[p] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) { // one window row at a time (registers)
                    const int yr = sy + dy - 1;
                    const int yy = yr < 0 ? 0 : (yr > V2_TW - 1 ? V2_TW - 1 : yr);
                    const float rowok = (yr >= 0 && yr <= V2_TW - 1) ? 1.0f : 0.0f;
                    f32x4 win[V2_TW], w3[3];
#pragma unroll
                    for (int xx = 0; xx < V2_TW; ++xx) win[xx] = *(const f32x4*)(wgrid + (yy * V2_TW + xx) * GRID_STRIDE + 4 * scg);
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) w3[dx] = *(const f32x4*)(dwt + (dy * 3 + dx) * NM + 4 * scg) * rowok;
#pragma unroll
                    for (int p = 0; p < V2_TW; ++p)
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx) {
                            const int xx = p + dx - 1;
                            if (xx < 0 || xx > V2_TW - 1) continue;
#pragma unroll
                            for (int c = 0; c < 4; ++c) dout[p][c] += win[xx][c] * w3[dx][c];
                        }
                }
                WAVE_LDS_FENCE(); // (every lane's window is in registers: the cells can be overwritten in place)
                if (s_act) {
#pragma unroll
                    for (int p = 0; p < V2_TW; ++p) *(f32x4*)(wgrid + (sy * V2_TW + p) * GRID_STRIDE + 4 * scg) = dout[p];
                }
                WAVE_LDS_FENCE();
            }
            const int tA = TILE_A(OL());
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 dv = *(const f32x4*)(wgrid + tA * GRID_STRIDE + 8 * g + 4 * h);
                const f32x4 b = __builtin_bit_cast(f32x4, db[g]);
#pragma unroll
                for (int i = 0; i < 4; ++i) d[4 * g + i] = b[i] + dv[i];
            }
            WAVE_LDS_FENCE();
        };
        { // ---- block 0: h differs from the base's in ONE pixel (P0): its difference goes to one cell, and every tile pixel next to P0 adds one tap of it ----
            int blk0 = 0;
            asm volatile("" : "+s"(blk0));
            const int tP = (py - vy0) * V2_TW + (pxx - vx0); // P0's pixel index in the tile (wave-uniform)
            const int lq = OL(), tA = TILE_A(lq);
            const bool at_p0 = (lq & 31) == tP;
            const uint4 (&hb)[4] = hb0, (&db)[4] = db0; // (fetched at the top of the pass)
            if (at_p0) { // block 0's L0 is needed at P0 only: L0_tile's accumulator for the pixel's input pattern, from the conv table
                const float* t1 = ltab + CT_T1_OFF + pat * CT_T1_STRIDE + 4 * h;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 b = __builtin_bit_cast(f32x4, hb[g]);
                    const f32x4 a4 = *(const f32x4*)(t1 + 8 * g);
                    const f32x2 r0 = lrelu2(a4[0], a4[1]), r1 = lrelu2(a4[2], a4[3]);
                    f32x4 o;
                    o[0] = r0[0] - b[0]; o[1] = r0[1] - b[1]; o[2] = r1[0] - b[2]; o[3] = r1[1] - b[3];
                    *(f32x4*)(wgrid + 8 * g + 4 * h) = o; // cell 0
                }
            }
            TP(1); // (block 0's share of "L0 x3" is now the table read and P0's cell)
            WAVE_LDS_FENCE();
            const int ey = py - vy0 - tA / V2_TW + 1, ex = pxx - vx0 - tA % V2_TW + 1; // P0 as a tap of this lane's pixel: (ey, ex) in 0..2 if adjacent
            const bool adj = ey >= 0 && ey <= 2 && ex >= 0 && ex <= 2;
            const float* wt0 = lside + blk0 * TR_SIDE_PER_BLOCK + (adj ? ey * 3 + ex : 0) * NM;
            const float adjf = adj ? 1.0f : 0.0f;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 dv = *(const f32x4*)(wgrid + 8 * g + 4 * h);
                const f32x4 wv4 = *(const f32x4*)(wt0 + 8 * g + 4 * h) * adjf;
                const f32x4 b = __builtin_bit_cast(f32x4, db[g]);
#pragma unroll
                for (int i = 0; i < 4; ++i) d[4 * g + i] = b[i] + dv[i] * wv4[i];
            }
            WAVE_LDS_FENCE();
            TP(2);
            L1L2_tile(ldsW, lside, h, lane, x, blk0, d);
            TP(3);
        }
        { // ---- block 1: differences in the 3x3 around P0 ----
            int blk1 = 1;
            asm volatile("" : "+s"(blk1));
            uint4 hb[4], db[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                hb[g] = sb[sib2_grid(HW, 1, 0, bpxA, g, h)];
                db[g] = sb[sib2_grid(HW, 1, 1, bpxA, g, h)];
            }
            f32x16 acc;
            L0_tile(ldsW, lside, h, lane, x, blk1, acc);
            TP(1);
            grid_write(acc, hb);
            strip_dw(lside + blk1 * TR_SIDE_PER_BLOCK, db);
            TP(2);
            L1L2_tile(ldsW, lside, h, lane, x, blk1, d);
            TP(3);
        }
        // ---- block 2: L0 on the tile; depthwise outputs on the tile AND the ring ----
        float dBk[16];
        int blk2 = 2;
        asm volatile("" : "+s"(blk2)); // (opaque: as a constant, every LDS address of the block's weights and side table became a register of its own, hoisted and spilled)
        {
            uint4 hb[4], db[4], dbB[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                hb[g] = sb[sib2_grid(HW, 2, 0, bpxA, g, h)];
                dbB[g] = sb[sib2_grid(HW, 2, 1, bpxB, g, h)];
                db[g] = sb[sib2_grid(HW, 2, 1, bpxA, g, h)];
            }
            f32x16 acc;
            L0_tile(ldsW, lside, h, lane, x, blk2, acc);
            TP(1);
            grid_write(acc, hb);
            const float* dwt = lside + blk2 * TR_SIDE_PER_BLOCK;
            // ring first (it reads the difference cells the tile's depthwise then overwrites in place): a pixel outside the tile has at most 3 taps inside it.
            // Its depthwise outputs (dBk) wait in registers while the tile goes through the last two layers and its stores
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 b = __builtin_bit_cast(f32x4, dbB[g]);
#pragma unroll
                for (int i = 0; i < 4; ++i) dBk[4 * g + i] = b[i];
            }
            {
                const int lq = OL();
                const bool validB = (lq & 31) < V2_RING;
                int wyB, wxB;
                ring_at(RING_B(lq), wyB, wxB);
                const int ry = wyB - oy, rx = wxB - ox; // relative to the tile: -2..6
                const int ylo = ry - 1 < 0 ? 0 : ry - 1, yhi = ry + 1 > V2_TW - 1 ? V2_TW - 1 : ry + 1;
                const int xlo = rx - 1 < 0 ? 0 : rx - 1, xhi = rx + 1 > V2_TW - 1 ? V2_TW - 1 : rx + 1;
                const int cy = yhi - ylo + 1 > 0 ? yhi - ylo + 1 : 0, cx = xhi - xlo + 1 > 0 ? xhi - xlo + 1 : 0;
                const int cnt = validB ? cy * cx : 0; // <= 3
#pragma unroll 1
                for (int k = 0; k < 3; ++k) { // (rolled: unrolled, the scheduler issues every tap's reads first and the registers spill)
                    const int iy = cx > 0 ? (cx == 1 ? k : (cx == 2 ? k >> 1 : k / 3)) : 0, ix = k - iy * cx;
                    const bool ok = k < cnt;
                    const int ny = ylo + iy, nx = xlo + ix;
                    const int cell = ok ? ny * V2_TW + nx : V2_ZERO_CELL;
                    const int tap = ok ? (ny - ry + 1) * 3 + (nx - rx + 1) : 0;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4 hv = *(const f32x4*)(wgrid + cell * GRID_STRIDE + 8 * g + 4 * h);
                        const f32x4 wv4 = *(const f32x4*)(dwt + tap * NM + 8 * g + 4 * h);
#pragma unroll
                        for (int i = 0; i < 4; ++i) dBk[4 * g + i] += hv[i] * wv4[i];
                    }
                }
            }
            WAVE_LDS_FENCE();
            strip_dw(dwt, db);
        }
        TP(4);
        base_fetch_here(frow, bpxA);
        L1L2_tile(ldsW, lside, h, lane, x, blk2, d);
        TP(5);
        {
            int rd_px[4];
            bool rd_ok[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int t = 8 * i + (lane >> 3);
                asm volatile("" : "+v"(t));
                const int tc = t < V2_TPX ? t : V2_TPX - 1;
                rd_px[i] = (oy + tc / V2_TW) * SIB_WIN + ox + tc % V2_TW;
                rd_ok[i] = t < V2_TPX;
            }
            if constexpr (F16LO) base_sub_f16lo(x, be, frow, bpxA, h);
            else base_subtract(x, be);
            if (lane == 0) slot_desc[slot] = make_uint2((uint32_t)crow, ent.y);
            TP(6);
            bool farA;
            {
                int bq = bpxA;
                asm volatile("" : "+v"(bq));
                const int yA = bq / N, xA = bq - yA * N;
                farA = (yA - py > 3 || py - yA > 3 || xA - pxx > 3 || pxx - xA > 3);
            }
            store_rows(x, crow_p, (OL() & 31) < V2_TPX, rd_px, rd_ok, farA);
            TP(7);
        }
        // ---- the ring: residual stream of the BASE in front of block 2 + this child's depthwise outputs ----
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 v = __builtin_bit_cast(f32x4, sb[sib2_x2(HW, bpxB, m, g, h)]);
#pragma unroll
                for (int i = 0; i < 4; ++i) x[m][4 * g + i] = v[i];
            }
        base_fetch_here(frow, bpxB);
#pragma unroll
        for (int i = 0; i < 16; ++i) d[i] = dBk[i];
        TP(8);
        L1L2_tile(ldsW, lside, h, lane, x, blk2, d);
        TP(9);
        {
            int rd_px[4];
            bool rd_ok[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int t = 8 * i + (lane >> 3);
                asm volatile("" : "+v"(t));
                int wy, wx;
                ring_at(t < V2_RING ? t : V2_RING - 1, wy, wx);
                rd_px[i] = wy * SIB_WIN + wx;
                rd_ok[i] = t < V2_RING;
            }
            if constexpr (F16LO) base_sub_f16lo(x, be, frow, bpxB, h);
            else base_subtract(x, be);
            TP(10);
            bool farB;
            {
                int bq = bpxB;
                asm volatile("" : "+v"(bq));
                const int yB = bq / N, xB = bq - yB * N;
                farB = (yB - py > 3 || py - yB > 3 || xB - pxx > 3 || pxx - xB > 3);
            }
            store_rows(x, crow_p, (OL() & 31) < V2_RING, rd_px, rd_ok, farB);
        }
        ent_c = ent_n;
        ent_n = ent_nn;
        slot_c = slot_n;
        slot_n = slot_nn;
        word_c = word_n;
        TP(11);
    }
    if (TPROF && lane == 0 && (wv == 0 || wv == 5))
        for (int i = 0; i < 12; ++i) atomicAdd(&tprof[(wv ? 16 : 0) + i], tp_acc[i]);
    if (TPROF && lane == 0) atomicMax(&s_tp_rec[2], wall_clock64());
}

#undef OL
#undef TILE_A
#undef RING_B
// ===============================================================================================
// OMOK_NET_F16X3: fc0 with block-scaled fp6 correction terms
// ===============================================================================================
// x*w = hi*hi (f16 MFMA) + lo*hi + hi*lo.  The two correction terms are 2^-11 of the product, so 4 significant bits
// keep the total at ~2^-15 relative: they run on v_mfma_scale_f32_32x32x64_f8f6f4 with fp6 (e2m3) operands and one E8M0
// scale byte per lane and 32-element K block (MX6; the first version used fp8 e4m3 with global scales).
// Per K = 64 the matrix pipe executes 4 f16 + 2 fp6 MFMAs of 32 cycles instead of 12 f16 MFMAs.  Probed on the device:
//   tools/probe/fp6_probe.hip  lane l = row/col l&31, k = 32*(l>>5) + i in bits [6i, 6i+5] of the lane's 192 bits; the lane's
//                              scale byte (selected by opsel) scales exactly that block by 2^(byte-127); the packed converts
//                              divide by the scale and keep element order (pk32) / interleave their two sources (2xpk16)
//   tools/probe/mx_probe.hip   the same for fp8;  shape_probe.hip / mx_rate.hip  the rates of the instruction mixes
//
// Tile = 512 features x 128 samples per workgroup, 4 waves (one per SIMD).  A K=64 super-step is consumed in 4 stages,
// one per group of 4 m-tiles: weights (24 KiB per stage) flow through a 4-slot LDS ring, the sample operands of a
// super-step (24 KiB) are double-buffered and stay in registers for its 4 stages (details at the kernel).
typedef int v8i __attribute__((ext_vector_type(8)));
#define VMCNT(n) ((((n) & 15) | (((n) >> 4) << 14)) | (7 << 4) | (15 << 8)) // s_waitcnt immediate: vmcnt(n) only
constexpr int MXS_FR = 24;              // fragments per weight stage (4 m-tiles x {hi j0..j3, lo8 half0, half1}) and per
constexpr int MXS_U4 = MXS_FR * 64;     // sample-operand buffer (4 sample tiles x the same 6); uint4 units
constexpr int MXS_SLOTS = 4;            // weight ring depth: three stages stay in flight behind the one being read

struct MxScales { int wa_hi, wa_lo, ab_hi, ab_lo; float w_mul, a_mul; }; // E8M0 bytes (A = weights, B = samples) + 2^SW, 2^SA

// LDS-DMA as inline asm: hipcc's waitcnt pass orders every later ds_read against builtin LDS-DMA with vmcnt(0),
// which drains the whole prefetch ring once per stage; issued from asm the pass does not see it and the counted
// waits below (also asm) are the only ordering.  m0 = LDS byte address of lane 0's 16 bytes.
__device__ inline void dma16(const uint4* g, const uint4* lds) {
    const uint32_t a = (uint32_t)(size_t)(const __attribute__((address_space(3))) void*)lds;
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(a) : "memory", "m0");
}
// same with a wave-uniform 64-bit base in SGPRs and a 32-bit byte offset per lane: no 64-bit vector add per DMA
template <bool NT = false>
__device__ inline void dma16s(const uint4* sbase, uint32_t voff, const uint4* lds) {
    const uint32_t a = (uint32_t)(size_t)(const __attribute__((address_space(3))) void*)lds;
    if (NT) asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1 nt" ::"v"(voff), "s"(sbase), "s"(a) : "memory", "m0");
    else asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(a) : "memory", "m0");
}

// Workgroup = 4 waves (one per SIMD, each with the full 512-register file): wave w owns m-tile 4g+w of every
// group g for ALL four sample tiles, i.e. 16 accumulator tiles (256 registers).  The sample operands of a
// super-step are read from LDS once and stay in registers for its 4 stages; a weight fragment is read from LDS by
// exactly one wave.  LDS traffic per stage drops from 144 KiB (8-wave form) to ~48 KiB and the matrix pipe is fed
// by one wave with 4 independent accumulator chains.
constexpr bool A_NT = true;     // the sample-operand stream is read once: non-temporal, so it does not displace the weight stream in L2
// fp6 (e2m3) copy of 32 f16 values (4 consecutive 8-element pieces, natural slot order) = x / 2^(E - 127).  The hi*lo / lo*hi correction
// terms only need ~3 bits, so the fp6 "hi" operands are derived from the f16 fragments on the otherwise idle VALU
// instead of being streamed (25 % fewer bytes through the LDS-DMA path, which bounds this kernel).
__device__ inline v8i f16x32_to_fp6(const half8& p0, const half8& p1, const half8& p2, const half8& p3, uint32_t e8m0) {
    typedef _Float16 half16 __attribute__((ext_vector_type(16)));
    const half16 lo = __builtin_shufflevector(p0, p1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    const half16 hi = __builtin_shufflevector(p2, p3, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    const half32 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27,
                                             28, 29, 30, 31);
    const u32x6 r = __builtin_amdgcn_cvt_scalef32_pk32_fp6_f16(v, __uint_as_float(e8m0 << 23));
    return v8i{(int)r[0], (int)r[1], (int)r[2], (int)r[3], (int)r[4], (int)r[5], 0, 0};
}
// fp6 x fp6 block-scaled MFMA; SEL_A / SEL_B = byte of the scale registers that holds this operand's E8M0 block scale
#define MFMA6(A, B, ACC, SEL_A, SA, SEL_B, SB)                                                                                  \
    ((SEL_B) == 0 ? __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4((A), (B), (ACC), 2, 2, (SEL_A), (int)(SA), 0, (int)(SB))  \
   : (SEL_B) == 1 ? __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4((A), (B), (ACC), 2, 2, (SEL_A), (int)(SA), 1, (int)(SB))  \
   : (SEL_B) == 2 ? __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4((A), (B), (ACC), 2, 2, (SEL_A), (int)(SA), 2, (int)(SB))  \
                  : __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4((A), (B), (ACC), 2, 2, (SEL_A), (int)(SA), 3, (int)(SB)))
// XCD-aware dealing of a 1-D grid's work items: workgroups go to the 8 XCDs round-robin (workgroup id % 8) and every XCD has its own L2, so XCD x takes a
// contiguous eighth of the items.  The dense split-K launches order their items split-major (all tiles of K split 0, then split 1, ...): the tiles of a split stream
// the same weight slice and then share it through ONE L2 (dealt tile-major, 8 tiles x 16 splits put tile t on XCD t: every L2 streamed the whole 45 MB matrix).
// The grid must hold ceil(total / 8) * 8 workgroups.
__device__ inline bool xcd_item(int total, int& item) {
    const int per_xcd = (total + 7) >> 3, j = (int)blockIdx.x >> 3;
    item = ((int)blockIdx.x & 7) * per_xcd + j;
    return j < per_xcd && item < total;
}
constexpr bool STAGGER = false; // (skewing the waves by s_nops after the barrier: 3.52 -> 3.88 ms, the delay costs more than it saves)
// ---- fc0: which tile and which part of K a workgroup owns, and what it does with its accumulators (k_fc0_mx and k_fc0_x3 share both) ----
struct Fc0Tile {
    int b0, count;                 // first sample (WIN: slot) of the tile; samples at or beyond `count` are not stored
    int ubeg, ksup;                // first super-step and number of super-steps of this workgroup's part of K
    int split_y, part_row0;        // EPI_PARTIAL: K split index; WIN: first slot of the K-split set (partials are indexed by the slot inside it)
    size_t out_row_u4;             // EPI_SPLIT: output row stride; EPI_PARTIAL: rows of the partial slab per split
    int win_oy, win_ox;            // WIN: origin of the bin's 7x7 window on the board
    int wr_y0, wr_x0, wr_w, wr_n, wr_inv; // WIN: the tile's rectangle of window pixels (bin_prefix_role): origin, width, super-steps (2 per pixel), 65536 / width + 1
    // WIN: super-step j of the tile's rectangle -> super-step u = 2 w + q of the 7x7 window (steps past the end -- prefetches -- re-read the last)
    __device__ __forceinline__ int win_u(int j) const {
        j = j < wr_n ? j : wr_n - 1;
        j = j < 0 ? 0 : j;
        const int wl = j >> 1, ry = (wl * wr_inv) >> 16, rx = wl - ry * wr_w;
        return 2 * ((wr_y0 + ry) * SIB_WIN + wr_x0 + rx) + (j & 1);
    }
};
// The arguments are the kernels' (ksup: the host's super-steps per workgroup, out_row_u4: its row stride).  false: the workgroup has no work.
template <int EPI, bool WIN>
__device__ __forceinline__ bool fc0_map_tile(Fc0Tile& t, int ksup, size_t out_row_u4, int full_tiles, int last_cnt, const int32_t* __restrict__ d_count,
                                             int max_count, const int32_t* __restrict__ tile_info) {
    t.b0 = blockIdx.x * GT_BS;
    t.ubeg = 0; t.part_row0 = 0; t.split_y = (int)blockIdx.y;
    t.win_oy = 0; t.win_ox = 0;
    t.wr_y0 = 0; t.wr_x0 = 0; t.wr_w = SIB_WIN; t.wr_n = 2 * SIB_WPX; t.wr_inv = 65536 / SIB_WIN + 1;
    if (WIN) { // d_count = Net::d_gcnt.  EPI_SPLIT: the tiles below the K-split set, whole K; EPI_PARTIAL: the tiles from NET_GCNT_SPLIT_TILE0 on, K split NET_GCNT_WIN_WAYS ways
        // Workgroups go to the 8 XCDs round-robin and every XCD has its own L2: XCD x takes a contiguous eighth of the tiles (tiles are
        // ordered by bin = by weight slice), so the workgroups that share an L2 stream the same 9 MB of weights in step instead of
        // every L2 streaming every slice (dealt round-robin, 46 % of the weight reads missed L2: 2.5 GB per launch, HBM-bound).
        const int nt = d_count[NET_GCNT_WIN_TILES], t_split = d_count[NET_GCNT_SPLIT_TILE0];
        const int n_here = EPI == EPI_PARTIAL ? nt - t_split : t_split;
        int tile, ways = 1;
        if (EPI == EPI_PARTIAL) { // 1-D grid over (tile of the split set, split): tiles x ways <= CUs (a 2-D grid of mostly idle, LDS-heavy workgroups
                                  // costs more to dispatch than the work takes); XCD x takes consecutive tiles, each with all its splits
            ways = d_count[NET_GCNT_WIN_WAYS];
            int item;
            if (n_here <= 0 || !xcd_item(n_here * ways, item)) return false;
            t.split_y = item % ways;
            tile = t_split + item / ways;
            t.part_row0 = t_split * GT_BS;
            out_row_u4 = (size_t)n_here * GT_BS; // partials: [split][slot inside the split set]
        } else { // position p of the cost-sorted order (bin_prefix_role), dealt in rounds of 8 x 32 workgroups: XCD x = blockIdx & 7 takes chunk x of an even round and chunk
                 // 7 - x of an odd one (the XCD with the dearest tiles of round 1 gets the cheapest of round 2)
            const int per_x = (int)gridDim.x >> 3, cu_x = per_x < 32 ? per_x : 32, j = (int)blockIdx.x >> 3, r = j / cu_x; // (32 CUs per XCD)
            const int xc = (int)blockIdx.x & 7, p = r * (8 * cu_x) + ((r & 1) ? 7 - xc : xc) * cu_x + j % cu_x;
            if (p >= n_here) return false;
            tile = tile_info[d_count[NET_GCNT_TILE_ORDER] + p];
        }
        t.b0 = tile * GT_BS;
        const int ti = tile_info[tile], bin = ti & 0xFF;
        t.count = t.b0 + ((ti >> 8) & 0xFF);
        // the tile's rectangle of window pixels (bin_prefix_role): rows wr_y0 .. y1, columns wr_x0 .. x1 of the 7x7 window; super-step j of the tile = pixel j / 2 of the rectangle in
        // row-major order, channel half j & 1
        int wr_y1, wr_x1;
        tile_rect(ti, t.wr_y0, wr_y1, t.wr_x0, wr_x1);
        t.wr_w = wr_x1 - t.wr_x0 + 1;
        t.wr_n = 2 * (wr_y1 - t.wr_y0 + 1) * t.wr_w;
        t.wr_inv = 65536 / t.wr_w + 1; // (j / 2) / wr_w = ((j / 2) * wr_inv) >> 16 for j / 2 < 49
        const int nsup = bin < SIB_BINS ? t.wr_n : 0, per = (nsup + ways - 1) / ways;
        t.ubeg = t.split_y * per;
        ksup = nsup - t.ubeg < per ? nsup - t.ubeg : per;
        t.win_oy = bin < SIB_BINS ? bin / SIB_ORG : 0; // (the single rows' bin has no window: its tiles run no super-step, and their prologue's prefetches
        t.win_ox = bin < SIB_BINS ? bin % SIB_ORG : 0; //  must stay inside the matrix)
    } else {
        const int nsup = full_tiles * 64 + 2 * last_cnt;
        t.count = d_count[0];
        if (t.count > max_count) t.count = max_count;
        if (EPI == EPI_PARTIAL && tile_info) { // full rows of the difference path (d_count = d_gcnt + NET_GCNT_FULL_ROWS, tile_info = d_gcnt + NET_GCNT_FULL_WAYS): the number
            // of K splits and the partial slab's row stride were chosen on the device (bin_prefix_role); uneven split.
            // 1-D grid over (split, tile) items dealt by xcd_item -- a (tiles_max x ways_max) grid of which a few dozen workgroups have work
            // costs more to dispatch (~65-100 workgroups per us) than the work takes
            const int ways = tile_info[0], per = (nsup + ways - 1) / ways;
            const int tiles = (t.count + GT_BS - 1) / GT_BS;
            int item;
            if (tiles == 0 || !xcd_item(tiles * ways, item)) return false;
            t.split_y = item / tiles;
            t.b0 = (item % tiles) * GT_BS;
            out_row_u4 = (size_t)tile_info[NET_GCNT_FULL_STRIDE - NET_GCNT_FULL_WAYS];
            t.ubeg = t.split_y * per;
            ksup = nsup - t.ubeg < per ? nsup - t.ubeg : per;
        } else {
            if (EPI == EPI_PARTIAL) { // K split chosen on the host: 1-D grid over (split, tile) items, `ksup` super-steps per split, out_row_u4 = tiles x 128 rows of partials per split
                const int tiles = (int)(out_row_u4 / GT_BS), ways = (nsup + ksup - 1) / ksup;
                int item;
                if (!xcd_item(tiles * ways, item)) return false;
                t.split_y = item / tiles;
                t.b0 = (item % tiles) * GT_BS;
                t.ubeg = t.split_y * ksup; // (uneven split: the last split takes what is left; the host never makes it empty)
                ksup = nsup - t.ubeg < ksup ? nsup - t.ubeg : ksup;
            }
            if (t.b0 >= t.count) return false;
        }
        // an empty split (never chosen on purpose) contributes zeros and must not stream from beyond the matrix
        if (EPI == EPI_PARTIAL && t.ubeg >= nsup) { t.ubeg = nsup - 1; ksup = 0; }
    }
    t.ksup = ksup < 0 ? 0 : ksup; // (a split that starts behind the end of K)
    t.out_row_u4 = out_row_u4;
    return true;
}
// accumulator g of a wave = m-tile 4g + wave of the tile's 128 samples.  EPI_PARTIAL: fp32 partials into the slab; EPI_SPLIT: bias, LeakyReLU, hi|lo operand row
// (WIN: of the slot's request row, with the fp32 fc0 row of the slot's full row added first: slot_desc = (request row, full row))
template <int EPI, bool WIN>
__device__ __forceinline__ void fc0_epilogue(const f32x16 (&acc)[4][4], const Fc0Tile& t, int wave, int lane, const float* __restrict__ bias,
                                             uint4* __restrict__ out_split, float* __restrict__ out_part, const uint2* __restrict__ slot_desc,
                                             const float* __restrict__ facc) {
    const int h = lane >> 5;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        int sample = t.b0 + 32 * c + (lane & 31);
        if (sample >= t.count) continue;
        const float* fa = nullptr;
        if (WIN && EPI == EPI_PARTIAL) sample -= t.part_row0; // partials are indexed by the slot inside the split set
        if (WIN && EPI != EPI_PARTIAL) { // slot -> (request row, full row)
            const uint2 dsc = slot_desc[sample];
            sample = (int)dsc.x;
            fa = facc + (size_t)dsc.y * NF;
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int mt = 4 * g + wave;
            if (EPI == EPI_PARTIAL) {
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    f32x4 o;
#pragma unroll
                    for (int q = 0; q < 4; ++q) o[q] = acc[g][c][4 * q4 + q];
                    *(f32x4*)(out_part + ((size_t)t.split_y * t.out_row_u4 + sample) * NF + 32 * mt + 8 * q4 + 4 * h) = o;
                }
            } else {
                float y[16];
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const f32x4 bv = *(const f32x4*)(bias + 32 * mt + 8 * q4 + 4 * h);
                    f32x4 fv = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (WIN) fv = *(const f32x4*)(fa + 32 * mt + 8 * q4 + 4 * h);
#pragma unroll
                    for (int q = 0; q < 4; ++q) y[4 * q4 + q] = WIN ? (acc[g][c][4 * q4 + q] + fv[q]) + bv[q] : acc[g][c][4 * q4 + q] + bv[q];
                }
#pragma unroll
                for (int sx = 0; sx < 2; ++sx) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = lrelu(y[8 * sx + j]);
                    half8 hi, lo;
                    split8(v, hi, lo);
                    uint4* row = out_split + (size_t)sample * t.out_row_u4 + (size_t)(2 * mt + sx) * 4;
                    row[h] = *(const uint4*)&hi;
                    row[2 + h] = *(const uint4*)&lo;
                }
            }
        }
    }
}
// WIN (difference path of the sibling rounds, N = 15): workgroup = one tile of 128 SLOTS whose rows share a 7x7 window (tile_info: bin |
// live slots << 8; d_count = the path's counters, Net::d_gcnt).  `act` holds the slots' difference rows (SIB_DROW_U4: 98 super-steps =
// 49 window pixels x 2 channel halves), the weight stages of super-step (w, q) are those of the window pixel's board pixel, and the
// epilogue adds the fp32 fc0 row of the slot's FULL row (facc: the run's base position; slot_desc = (request row, full row)).  Tiles
// of the single rows (bin SIB_BINS) have no super-steps at all.
template <int EPI, bool WIN = false>
__global__ __launch_bounds__(256) void k_fc0_mx(const uint4* __restrict__ wp, const uint4* __restrict__ act, int ksup,
                                                size_t act_row_u4, int full_tiles, int last_cnt, MxScales sc,
                                                const float* __restrict__ bias, uint4* __restrict__ out_split, size_t out_row_u4,
                                                float* __restrict__ out_part, const int32_t* __restrict__ d_count, int max_count,
                                                const int32_t* __restrict__ tile_info, const uint2* __restrict__ slot_desc,
                                                const float* __restrict__ facc, int bn) {
    // (bn: board side, WIN only)  Static LDS objects, one per weight-ring slot: hipcc orders a ds_read after an LDS-DMA write by object (alias
    // scopes of distinct LDS variables), and with one dynamic array it drains ALL outstanding DMA (vmcnt(0)) before
    // the first LDS read of every stage.  With separate objects it waits exactly for the last DMA into the slot read.
    __shared__ uint4 ldsA[2 * MXS_U4];        // [2]{ f16 [128 samples][8 pieces] | fp6 residual part [128 samples][4 pieces] }
    __shared__ uint4 ldsW0[MXS_U4], ldsW1[MXS_U4], ldsW2[MXS_U4], ldsW3[MXS_U4]; // [4 i][6 frag][64] each
    auto ring = [&](int slot) -> uint4* { return slot == 0 ? ldsW0 : slot == 1 ? ldsW1 : slot == 2 ? ldsW2 : ldsW3; };
    Fc0Tile t;
    if (!fc0_map_tile<EPI, WIN>(t, ksup, out_row_u4, full_tiles, last_cnt, d_count, max_count, tile_info)) return;
    const int b0 = t.b0, ubeg = t.ubeg, win_oy = t.win_oy, win_ox = t.win_ox;
    ksup = t.ksup;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6); // 0..3 = m-tile inside a group
    const int h = lane >> 5;

    auto uoff = [&](int u) { // (block, pixel) of super-step u inside a sample row, packed as block * 32 + pixel
        if (WIN) return t.win_u(u); // difference rows: super-step u = 2 w + q of the window
        const int full = full_tiles * 64;
        int tile, q, pl;
        if (u < full) { tile = u >> 6; q = (u >> 5) & 1; pl = u & 31; }
        else { const int r = u - full; tile = full_tiles; q = r / last_cnt; pl = r % last_cnt; }
        return (tile * 2 + q) * 32 + pl;
    };
    // absolute super-step (= weight stage group) of this workgroup's local super-step ul
    auto ustep = [&](int ul) {
        if (!WIN) return ubeg + ul;
        const int u = t.win_u(ubeg + ul);
        const int w = u >> 1, qq = u & 1, wy = w / SIB_WIN, wx = w - wy * SIB_WIN;
        const int px = (win_oy + wy) * bn + win_ox + wx;
        return px < full_tiles * 32 ? (px >> 5) * 64 + qq * 32 + (px & 31) : full_tiles * 64 + qq * last_cnt + (px - full_tiles * 32);
    };
    // a wave stages exactly the 6 weight fragments it consumes (m-tile `wave` of the stage's group): the weight ring is
    // wave-private, ordered by this wave's own vmcnt, and needs no workgroup barrier
    const uint4* wsrc = wp + (size_t)(wave * 6) * 64; // wave-uniform; lanes add lane * 16 B
    const uint32_t w_voff = lane * 16;
    int w_dma_off = wave * 6 * 64, w_rd_off = wave * 6 * 64 + lane;
    asm volatile("" : "+s"(w_dma_off));
    asm volatile("" : "+v"(w_rd_off));
    auto issue_w1 = [&](int uabs, int g, int slot, int k) { // fragment k of this wave's 6, stage g of absolute super-step uabs
        dma16s(wsrc + ((size_t)uabs * 4 + g) * MXS_U4 + k * 64, w_voff, ring(slot) + w_dma_off + k * 64);
    };
    // Sample operands of a super-step: per sample 128 B of f16 pieces (2j+h) and 64 B of fp6 residuals and their scale bytes (read_lo6)
    // (two regions of the row's dense (tile, q) block).  The DMA reads them with ADJACENT LANES ON ADJACENT 16-B PIECES of one sample (8
    // lanes = the 128-B f16 part, 4 lanes = the 64-B residual part): the texture path coalesces neighbouring lanes only,
    // and the MFMA lane order (lane = sample) made every lane its own 16-B request -- 64 requests per instruction
    // and as much address-path time for these 20 % of the bytes as for all the weights.  Wave w stages sample tile w:
    // k = 0..3: f16 part of samples 8k..8k+7 of the tile, k = 4,5: residual part of samples 16(k-4)..+15.
    // LDS image: f16 [128 samples][8 pieces], then the residual parts [128 samples][4 pieces]; the piece index is XOR-swizzled with
    // the sample index (on the global side, inside the contiguous segment) so that the ds_read_b128 of an MFMA
    // fragment (lane = sample, 128-B / 64-B stride) is bank-conflict free for its four 16-lane groups.
    const uint4* abase = act + (size_t)(b0 + 32 * wave) * act_row_u4; // wave-uniform
    uint32_t a_voff[6];                                               // per-lane byte offsets of the 6 pieces
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (k < 4) {
            const int st = 8 * k + (lane >> 3); // sample within the tile
            a_voff[k] = (uint32_t)(((size_t)st * act_row_u4 + (size_t)((lane & 7) ^ ((st >> 1) & 7))) * 16);
        } else {
            const int st = 16 * (k - 4) + (lane >> 2);
            a_voff[k] = (uint32_t)(((size_t)st * act_row_u4 + (size_t)((lane & 3) ^ ((st >> 2) & 3))) * 16);
        }
    }
    auto issue_a1 = [&](int uo, int buf, int k) {
        const int dst = k < 4 ? (wave * 4 + k) * 64 : 1024 + (wave * 2 + (k - 4)) * 64;
        const int blk = uo >> 5, pl = uo & 31; // f16 part: 8 uint4 per pixel; residual part: 4 per pixel behind the 32 x 8
        if (WIN) {
            const int e = (uo & 1) * SIB_WPX + (uo >> 1); // difference row: [q][w] f16 parts, then [q][w] residual parts
            dma16s<A_NT>(abase + (k < 4 ? e * 8 : SIB_DLO_U4 + e * 4), a_voff[k], ldsA + buf * MXS_U4 + dst);
        } else
        dma16s<A_NT>(abase + blk * OP_BLK_U4 + (k < 4 ? pl * 8 : OP_LO_U4 + pl * 4), a_voff[k], ldsA + buf * MXS_U4 + dst);
    };
    // LDS read offsets (uint4 units) of this lane's pieces inside sample tile 0; tile c adds 256 / 128
    const int sl = lane & 31;
    int a_rd_hi[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) a_rd_hi[j] = sl * 8 + ((2 * j + h) ^ ((sl >> 1) & 7));
    // the 64 B of a sample's residual part = [h0 fp6 dwords 0..3][h1 dwords 0..3][h0 dwords 4,5 | h1 dwords 4,5][scale bytes | pad]
    const int a_rd_lo6 = 1024 + sl * 4 + (h ^ ((sl >> 2) & 3));                          // uint4 index of this lane's first 16 B
    const int a_rd_tail = (1024 + sl * 4 + (2 ^ ((sl >> 2) & 3))) * 16 + 8 * h;         // byte offset of its last 8 B
    const int a_rd_esc = (1024 + sl * 4 + (3 ^ ((sl >> 2) & 3))) * 16 + 2 * h;          // byte offset of its two scale bytes (hi copy, residual)
    uint32_t sc_hi = 0, sc_lo = 0, sc_hi_n = 0, sc_lo_n = 0; // E8M0 bytes of the 4 sample tiles (byte c), current / next super-step
    auto read_lo6 = [&](const uint4* LA, int c, v8i& a6, uint32_t& e_hi, uint32_t& e_lo) { // sample tile c of the buffer at LA
        const unsigned char* Bp = (const unsigned char*)LA + c * 2048;
        const uint4 q0 = LA[c * 128 + a_rd_lo6];
        const uint2 q1 = *(const uint2*)(Bp + a_rd_tail);
        const uint32_t e = *(const uint16_t*)(Bp + a_rd_esc);
        a6 = v8i{(int)q0.x, (int)q0.y, (int)q0.z, (int)q0.w, (int)q1.x, (int)q1.y, 0, 0};
        e_hi |= (e & 0xFFu) << (8 * c);
        e_lo |= (e >> 8) << (8 * c);
    };
    // conversions saturate instead of producing NaN (MODE.FP16_OVFL, probed: tools/probe/cvt_probe.hip)
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 23, 1), 1");
    f32x16 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][c][r] = 0.0f;

    half8 bh[4][4];  // sample operands of the current super-step (f16 pieces)
    v8i a8l[4], a8h[4];
    uint4 wc[6];     // this wave's weight fragments of the current stage
    { // prologue, in the issue order of the steady state's last four stages: sample operands of super-step 0, weight stages
      // 0..2, the first two pieces of super-step 1, weight stage 3  (per wave: 8 + 24 DMA instructions)
        const int uo = uoff(ubeg), uo1 = uoff(ubeg + 1), us0 = ustep(0);
#pragma unroll
        for (int k = 0; k < 6; ++k) issue_a1(uo, 0, k);
#pragma unroll
        for (int st = 0; st < 3; ++st)
#pragma unroll
            for (int k = 0; k < 6; ++k) issue_w1(us0, st, st, k);
        issue_a1(uo1, 1, 0);
        issue_a1(uo1, 1, 1);
#pragma unroll
        for (int k = 0; k < 6; ++k) issue_w1(us0, 3, 3, k);
        asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); // A(0) and W(0) landed
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) bh[c][j] = *(const half8*)(ldsA + c * 256 + a_rd_hi[j]);
#pragma unroll
        for (int c = 0; c < 4; ++c) read_lo6(ldsA, c, a8l[c], sc_hi, sc_lo);
#pragma unroll
        for (int k = 0; k < 6; ++k) wc[k] = ldsW0[w_rd_off + k * 64];
    }
    // One wave per SIMD: nothing but this wave's own instruction stream hides anything, and an MFMA only covers what
    // is issued in ITS gap (tools/probe/overlap_probe.hip: an 8-pass f16 MFMA hides ~4-5 single-issue instructions, a
    // trailing block of VALU hides nothing; one LDS-DMA costs ~60 cycles of issue).  So every MFMA below is followed by
    // its own small group of fillers and a scheduling barrier pins the group to the gap:
    //   f16 MFMA gaps   : the fp6 derivations (one packed convert per 32 values: the weight block, at g = 0 also the sample tiles),
    //                     at g = 3 the LDS read that replaces the piece just consumed, at the end the next stage's
    //                     weight fragments LDS -> registers
    //   block-scaled gaps : one LDS-DMA each (16-pass MFMA = 64 cycles)
    // Stage q = (ul, g) lives in ring slot g.  The DMA of stage q+4 goes to slot g itself (its fragments were read into
    // registers during stage q-1): four stages of weights are in flight or resident.  Per block-scaled phase the DMA order is [2 sample pieces (g < 3)], 6 weights.
    // One workgroup barrier per super-step (top of g = 3): behind it the NEXT super-step's sample operands replace the
    // current ones in registers piece by piece, each right after its last MFMA.
#define GAP() __builtin_amdgcn_sched_barrier(0)
    for (int ul = 0; ul < ksup; ++ul) {
        const int ub = ul & 1;
        const int uo_next = uoff(ubeg + ul + 1), uo_next2 = uoff(ubeg + ul + 2);
        const int us_next = ustep(ul + 1); // stage q + 4 = (ul + 1, g)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            half8 ah[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) ah[j] = __builtin_bit_cast(half8, wc[j]);
            const v8i w8l = v8i{(int)wc[4].x, (int)wc[4].y, (int)wc[4].z, (int)wc[4].w, (int)wc[5].x, (int)wc[5].y, 0, 0};
            const uint32_t wsc = wc[5].z; // E8M0 bytes of this lane's weight block (byte 0: fp6 copy of hi, byte 1: residual)
            // this stage's DMA refills ring slot g, the slot `wc` was read from one stage ago: those reads have returned
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            v8i w6h = {0, 0, 0, 0, 0, 0, 0, 0}; // fp6 copy of ah[0..3]
            if (g == 3) { // every wave's share of A(ul+1) must have landed before anyone reads it: its last pieces were
                          // issued at the head of stage g = 1, with 6 + 6 weight pieces behind them
                asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                // the barrier releases the four waves in the same cycle and they would then reach every DMA gap together
                // (one texture path per CU, 16 cycles per piece): skew them by 16 cycles each
                if (STAGGER)
                    for (int i = 0; i < wave; ++i) asm volatile("s_nop 15");
            }
            const uint4* LAn = ldsA + (ub ^ 1) * MXS_U4;
            uint4 wn[6];
            // DMA piece d = 0..7 of this stage: [2 sample pieces (g < 3)], 6 weight pieces; spread over the stage's 24
            // MFMA gaps (the four waves share one texture path: 30 pieces x 16 cycles per stage and CU)
            auto dma_piece = [&](int d) { // sample pieces run two super-steps ahead: A(ul+1) pieces 2..5 at g = 0, 1; A(ul+2) pieces 0, 1 at
                // g = 3, behind the barrier (its buffer held A(ul), which every wave finished reading before that barrier)
                if (g == 2) {
                    if (d < 6) issue_w1(us_next, g, g, d);
                } else if (d < 2) {
                    if (g == 3) issue_a1(uo_next2, ub, d);
                    else issue_a1(uo_next, ub ^ 1, 2 + 2 * g + d);
                } else {
                    issue_w1(us_next, g, g, d - 2);
                }
            };
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    acc[g][c] = MFMA16(ah[j], bh[c][j], acc[g][c]);
                    // one packed convert per 32 values: the weight block in the first gap, sample tile c in gap (1, c) of g = 0
                    if (j == 0 && c == 0) w6h = f16x32_to_fp6(ah[0], ah[1], ah[2], ah[3], wsc & 0xFFu);
                    if (g == 0 && j == 1) a8h[c] = f16x32_to_fp6(bh[c][0], bh[c][1], bh[c][2], bh[c][3], (sc_hi >> (8 * c)) & 0xFFu);
                    if (g == 3) bh[c][j] = *(const half8*)(LAn + c * 256 + a_rd_hi[j]); // next super-step's piece
                    if (j == 3) { // stage q+1's weights (issued during stage q-3): everything but the pieces of stages q-2, q-1
                                  // (8 each, 6 for a g = 2 stage) and the first 4 of this stage has landed
                        if (c == 0) {
                            if (g == 0 || g == 3) asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
                            else asm volatile("s_waitcnt vmcnt(20)" ::: "memory");
                        }
                        if (c >= 1) {
                            wn[2 * (c - 1)] = ring((g + 1) & 3)[w_rd_off + (2 * (c - 1)) * 64];
                            wn[2 * (c - 1) + 1] = ring((g + 1) & 3)[w_rd_off + (2 * (c - 1) + 1) * 64];
                        }
                    }
                    if ((4 * j + c) % 3 == 1 && 4 * j + c <= 13) dma_piece((4 * j + c) / 3); // gaps 1, 4, 7, 10, 13 -> d = 0..4 (after the wait above)
                    GAP();
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                acc[g][c] = MFMA6(w6h, a8l[c], acc[g][c], 0, wsc, c, sc_lo); // (fp6 copy of w) x (residual of x)
                if (c == 0) dma_piece(5);
                if (c == 3) dma_piece(6);
                if (g == 3) read_lo6(LAn, c, a8l[c], sc_hi_n, sc_lo_n);
                GAP();
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                acc[g][c] = MFMA6(w8l, a8h[c], acc[g][c], 1, wsc, c, sc_hi); // (residual of w) x (fp6 copy of x)
                if (c == 2) dma_piece(7);
                GAP();
            }
            if (g == 3) { sc_hi = sc_hi_n; sc_lo = sc_lo_n; sc_hi_n = 0; sc_lo_n = 0; }
#pragma unroll
            for (int k = 0; k < 6; ++k) wc[k] = wn[k];
        }
    }
#undef GAP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 23, 1), 0");

    fc0_epilogue<EPI, WIN>(acc, t, wave, lane, bias, out_split, out_part, slot_desc, facc);
}

// ===============================================================================================
// OMOK_NET_F16X3, FC0_F16 operand format: fc0 with f16 correction terms
// ===============================================================================================
// x*w = hi*hi + lo*hi + hi*lo with hi = f16(x), lo = f16(x - hi) on BOTH sides: three f16 MFMAs per product, the arithmetic of the trunk,
// fc1 and the heads (products good to ~2^-22; the fp6 correction terms of k_fc0_mx stop at ~2^-15, which is what the 1e-3 contract
// feels on nets whose head outputs are large: net_commit measures and chooses, Net::fc0_policy).  Same tile and the same machinery as
// k_fc0_mx -- 512 features x 128 samples per workgroup, one wave per SIMD with 16 accumulator tiles, wave-private weight rings filled by
// LDS-DMA and ordered by counted vmcnt waits, double-buffered sample operands, one workgroup barrier per step -- but a step is a HALF
// super-step: K = 32 = one pixel x 32 channels (m = 2q + mm), so that a weight stage (4 m-tiles x {hi s0, hi s1, lo s0, lo s1} =
// 16 KiB) and a sample buffer (128 samples x (64 B hi + 64 B lo) = 16 KiB) keep the LDS at 96 KiB.  Per stage and wave: 24 MFMAs, 4-6 DMA
// pieces, 4 weight reads; no converts at all.  Same arguments as k_fc0_mx (ksup / ubeg count K = 64 super-steps).
constexpr int X3_FR = 16;
constexpr int X3_U4 = X3_FR * 64; // uint4 per weight stage and per sample buffer
template <int EPI, bool WIN>
__global__ __launch_bounds__(256) void k_fc0_x3(const uint4* __restrict__ wp, const uint4* __restrict__ act, int ksup, size_t act_row_u4, int full_tiles,
                                                int last_cnt, const float* __restrict__ bias, uint4* __restrict__ out_split, size_t out_row_u4,
                                                float* __restrict__ out_part, const int32_t* __restrict__ d_count, int max_count,
                                                const int32_t* __restrict__ tile_info, const uint2* __restrict__ slot_desc,
                                                const float* __restrict__ facc, int bn) {
    __shared__ uint4 ldsA[2 * X3_U4];         // [2]{ hi [128 samples][4 pieces] | lo [128 samples][4 pieces] }
    __shared__ uint4 ldsW0[X3_U4], ldsW1[X3_U4], ldsW2[X3_U4], ldsW3[X3_U4]; // one object per ring slot (see k_fc0_mx)
    auto ring = [&](int slot) -> uint4* { return slot == 0 ? ldsW0 : slot == 1 ? ldsW1 : slot == 2 ? ldsW2 : ldsW3; };
    // (which tile, which part of K: fc0_map_tile)
    Fc0Tile t;
    if (!fc0_map_tile<EPI, WIN>(t, ksup, out_row_u4, full_tiles, last_cnt, d_count, max_count, tile_info)) return;
    const int b0 = t.b0, ubeg = t.ubeg, win_oy = t.win_oy, win_ox = t.win_ox;
    ksup = t.ksup;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5;
    const int kh = 2 * ksup; // half-steps of this workgroup; local half-step vl = 2 * (local super-step) + mm

    // uint4 offset of the hi part of local half-step vl inside a sample row (the residual part follows at `lo_off`); half-steps past the
    // end (prefetches) re-read the last one
    const int lo_off = WIN ? SIB_DLO_U4 : OP_LO_U4;
    auto a_off = [&](int vl) {
        vl = vl < kh ? vl : kh - 1;
        vl = vl < 0 ? 0 : vl;
        const int u = ubeg + (vl >> 1), mm = vl & 1;
        if (WIN) {
            const int uc = t.win_u(u);
            return ((uc & 1) * SIB_WPX + (uc >> 1)) * 8 + 4 * mm; // difference row: [q][w] parts, super-step u = 2 w + q
        }
        const int full = full_tiles * 64;
        int tile, q, pl;
        if (u < full) { tile = u >> 6; q = (u >> 5) & 1; pl = u & 31; }
        else { const int r = u - full; tile = full_tiles; q = r / last_cnt; pl = r % last_cnt; if (q > 1) { q = 1; pl = last_cnt - 1; } }
        return (tile * 2 + q) * OPX_BLK_U4 + pl * 8 + 4 * mm;
    };
    // weight stage group (4 stages) of local half-step vl: absolute half-step of the packed matrix
    auto w_half = [&](int vl) {
        vl = vl < 0 ? 0 : vl;
        const int ul = vl >> 1, mm = vl & 1;
        int us;
        if (!WIN) us = ubeg + ul;
        else {
            const int u = t.win_u(ubeg + ul);
            const int w = u >> 1, qq = u & 1, wy = w / SIB_WIN, wx = w - wy * SIB_WIN;
            const int px = (win_oy + wy) * bn + win_ox + wx;
            us = px < full_tiles * 32 ? (px >> 5) * 64 + qq * 32 + (px & 31) : full_tiles * 64 + qq * last_cnt + (px - full_tiles * 32);
        }
        return us * 2 + mm;
    };
    const uint4* wsrc = wp + (size_t)(wave * 4) * 64; // this wave's 4 fragments of a stage (m-tile 4g + wave); lanes add lane * 16 B
    const uint32_t w_voff = lane * 16;
    int w_dma_off = wave * 4 * 64, w_rd_off = wave * 4 * 64 + lane;
    asm volatile("" : "+s"(w_dma_off));
    asm volatile("" : "+v"(w_rd_off));
    auto issue_w = [&](int habs, int g, int slot, int k) { dma16s(wsrc + ((size_t)habs * 4 + g) * X3_U4 + k * 64, w_voff, ring(slot) + w_dma_off + k * 64); };
    // sample operands of a half-step: per sample 64 B of hi pieces (2s+h) and 64 B of residual pieces, fetched with 4 adjacent lanes on
    // the 4 adjacent pieces of one sample; wave w stages sample tile w: piece k = 2 * part + half = samples 16 half .. +15 of the tile.
    // LDS slot (sample, p) holds piece p ^ ((sample >> 2) & 3): the MFMA-fragment ds_read_b128 (lane = sample, 64-B stride) is then
    // conflict-free (the layout of k_fc0_mx's residual part)
    const uint4* abase = act + (size_t)(b0 + 32 * wave) * act_row_u4;
    uint32_t a_voff[2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int st = 16 * half + (lane >> 2);
        a_voff[half] = (uint32_t)(((size_t)st * act_row_u4 + (size_t)((lane & 3) ^ ((st >> 2) & 3))) * 16);
    }
    auto issue_a = [&](int aoff, int buf, int k) {
        const int part = k >> 1, half = k & 1;
        dma16s<A_NT>(abase + aoff + part * lo_off, a_voff[half], ldsA + buf * X3_U4 + part * 512 + (wave * 2 + half) * 64);
    };
    const int sl = lane & 31;
    int a_rd[2]; // uint4 index of this lane's piece 2s + h inside sample tile 0 of a buffer's hi part (tile c adds 128, the residual part 512)
#pragma unroll
    for (int sx = 0; sx < 2; ++sx) a_rd[sx] = sl * 4 + ((2 * sx + h) ^ ((sl >> 2) & 3));

    f32x16 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][c][r] = 0.0f;
    half8 bh[4][2], bl[4][2]; // sample operands of the current half-step: [sample tile][k-step s]
    uint4 wc[4];              // this wave's weight fragments of the current stage: hi s0, hi s1, lo s0, lo s1
    { // prologue, in the issue order of the steady state's last four stages (the counted waits below assume it): A(0), weight stages 0..2,
      // the first two pieces of A(1), weight stage 3: 22 DMA instructions per wave
        const int a0 = a_off(0), a1 = a_off(1), h0 = w_half(0);
#pragma unroll
        for (int k = 0; k < 4; ++k) issue_a(a0, 0, k);
#pragma unroll
        for (int st = 0; st < 3; ++st)
#pragma unroll
            for (int k = 0; k < 4; ++k) issue_w(h0, st, st, k);
        issue_a(a1, 1, 0);
        issue_a(a1, 1, 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) issue_w(h0, 3, 3, k);
        asm volatile("s_waitcnt vmcnt(14)" ::: "memory"); // A(0) and W(0, 0) landed
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int sx = 0; sx < 2; ++sx) {
                bh[c][sx] = *(const half8*)(ldsA + c * 128 + a_rd[sx]);
                bl[c][sx] = *(const half8*)(ldsA + 512 + c * 128 + a_rd[sx]);
            }
#pragma unroll
        for (int k = 0; k < 4; ++k) wc[k] = ldsW0[w_rd_off + k * 64];
    }
#define GAP() __builtin_amdgcn_sched_barrier(0)
    // Stage q = (vl, g) lives in ring slot g; its DMA refills slot g with stage q + 4 = (vl + 1, g) (the slot's fragments went to registers
    // during stage q - 1).  DMA pieces per stage, in issue order: g = 0: A(vl + 1) pieces 2, 3 + 4 weights; g = 1, 2: 4 weights; g = 3
    // (behind the barrier that proves every wave has read A(vl)'s buffer): A(vl + 2) pieces 0, 1 + 4 weights.  Counted waits: the next
    // stage's weights (issued three stages ago) have landed when at most {16, 16, 14, 14} younger pieces are outstanding at gap 17 of
    // g = 0..3; A(vl + 1) has landed at the top of g = 3 when at most 12 are.
    for (int vl = 0; vl < kh; ++vl) {
        const int vb = vl & 1;
        const int a_next = a_off(vl + 1), a_next2 = a_off(vl + 2);
        const int h_next = w_half(vl + 1);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            half8 ah[2], al[2];
#pragma unroll
            for (int sx = 0; sx < 2; ++sx) { ah[sx] = __builtin_bit_cast(half8, wc[sx]); al[sx] = __builtin_bit_cast(half8, wc[2 + sx]); }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // (the reads of slot g, issued one stage ago, have returned: its refill may start)
            if (g == 3) {
                asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
            }
            const uint4* LAn = ldsA + (vb ^ 1) * X3_U4;
            uint4 wn[4];
            auto dma_piece = [&](int d) {
                if (g == 0 || g == 3) {
                    if (d < 2) { if (g == 3) issue_a(a_next2, vb, d); else issue_a(a_next, vb ^ 1, 2 + d); }
                    else if (d < 6) issue_w(h_next, g, g, d - 2);
                } else if (d < 4) issue_w(h_next, g, g, d);
            };
#pragma unroll
            for (int sx = 0; sx < 2; ++sx) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
#pragma unroll
                    for (int term = 0; term < 3; ++term) {
                        const int t = (sx * 4 + c) * 3 + term; // MFMA gap 0..23 of the stage
                        acc[g][c] = MFMA16(term == 1 ? al[sx] : ah[sx], term == 2 ? bl[c][sx] : bh[c][sx], acc[g][c]);
                        if (t % 3 == 1 && t <= 16) dma_piece(t / 3);
                        if (t == 17) {
                            if (g < 2) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
                            else asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
                        }
                        if (t >= 18 && t < 22) wn[t - 18] = ring((g + 1) & 3)[w_rd_off + (t - 18) * 64];
                        if (g == 3 && term == 2) { // the next half-step's operands replace this pair right behind its last MFMA
                            bh[c][sx] = *(const half8*)(LAn + c * 128 + a_rd[sx]);
                            bl[c][sx] = *(const half8*)(LAn + 512 + c * 128 + a_rd[sx]);
                        }
                        GAP();
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) wc[k] = wn[k];
        }
    }
#undef GAP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    fc0_epilogue<EPI, WIN>(acc, t, wave, lane, bias, out_split, out_part, slot_desc, facc);
}

// ===============================================================================================
// OMOK_NET_F16X3: transposed GEMM  D^T[MT*32 x 128 samples] = Wp * Act^T
// ===============================================================================================
// Wp : [ksteps][MT][hi|lo][lane][8] f16 (1 KiB fragments), Act: rows of [ksteps][hi h0|hi h1|lo h0|lo h1]
// 8 waves: wm = wave>>1 owns MT/4 m-tiles, ws = wave&1 owns 2 of the 4 sample tiles.

// The main loop, shared by k_gemm_t and k_tail_fused's fc1 phase: k-steps [kbeg, kbeg + ksteps) of the workgroup's 128 samples through a ring of NST slots of
// (MT * 2 + 8) KiB at `lds`, into acc[i][c] = m-tile wm * MT/4 + i, sample tile 2 ws + c.  The last NST - 1 k-steps stage nothing: behind their barriers
// tail_issue(j), j = 0 .. NST - 2, may issue XT LDS-DMA instructions each for the caller's next phase (into ring slots whose last read that barrier proves); they are
// younger than every k-step's pieces and still in flight on return (XT = 0: nothing is).
template <int MT, int NST, int XT, class TailIssue>
__device__ __forceinline__ void gemm_t_mainloop(uint4* lds, const uint4* __restrict__ wp, const uint4* __restrict__ act, int ksteps, int kbeg, size_t act_row_u4, int k_full,
                                                int last_cnt, int lo_off, int b0, int wave, int lane, f32x16 (&acc)[MT / 4][2], TailIssue tail_issue) {
    constexpr int MTW = MT / 4;
    constexpr int WFR = MT * 2;            // weight fragments per k-step
    constexpr int NFR = WFR + 8;           // + 4 sample tiles x (hi, lo)
    constexpr int LPW = NFR / 8;           // LDS-DMA instructions per wave per k-step (NFR is a multiple of 8)
    constexpr int STAGE_U4 = NFR * 64;
    // NST ring slots: NST-2 k-steps stay in flight behind the one being read
    static_assert(NFR % 8 == 0, "fragment count must split evenly over 8 waves");
    static_assert(XT == 0 || NST == 3 || NST == 4, "the counted waits of the last k-steps know these depths");
    const int wm = wave >> 1, ws = wave & 1;
    const int h = lane >> 5;

    // staging plan: this wave owns fragments f = wave + 8*i of every k-step.
    // f < WFR: weight fragment (1 KiB, linear, advancing WFR KiB per k-step);  else activation fragment
    // (sample tile ct, part hi/lo): lane (c = lane&31, h) fetches the 16-byte piece at uint4 offset
    // ko(k-step) + part*lo_off + h of sample row b0 + 32*ct + c.
    const uint4* src[LPW];
    bool is_w[LPW];
#pragma unroll
    for (int i = 0; i < LPW; ++i) {
        const int f = wave + 8 * i;
        is_w[i] = f < WFR;
        if (f < WFR) {
            src[i] = wp + (size_t)f * 64 + lane;
        } else {
            const int a = f - WFR, ct = a >> 1, part = a & 1;
            const size_t row = (size_t)(b0 + 32 * ct + (lane & 31));
            src[i] = act + row * act_row_u4 + (size_t)(part * lo_off + h);
        }
    }
    int kt = kbeg; // next k-step to stage
    int ko_cur = 0;
    auto issue_begin = [&]() { // uint4 offset of k-step kt inside an activation row: 4 per k-step; the k-steps of a
        // partial last pixel tile (fc0 only) sit in 128-uint4 blocks holding last_cnt k-steps each
        ko_cur = kt < k_full ? 4 * kt : ((k_full >> 5) + (kt - k_full) / last_cnt) * 128 + ((kt - k_full) % last_cnt) * 4;
    };
    auto issue_one = [&](int i, int slot) { // one LDS-DMA instruction (1 KiB fragment) of k-step kt into ring slot `slot`
        const uint4* g = is_w[i] ? src[i] + (size_t)kt * (WFR * 64) : src[i] + ko_cur;
        dma16(g, lds + slot * STAGE_U4 + (wave + 8 * i) * 64); // from asm: see dma16 (no compiler vmcnt(0) before the ds_reads)
    };
    auto issue = [&](int slot) {
        issue_begin();
#pragma unroll
        for (int i = 0; i < LPW; ++i) issue_one(i, slot);
        kt += 1;
    };
#pragma unroll
    for (int i = 0; i < MTW; ++i)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][c][r] = 0.0f;

#pragma unroll
    for (int p = 0; p < NST - 1; ++p)
        if (p < ksteps) issue(p);
    int slot = 0, nslot = NST - 1;
    for (int t = 0; t < ksteps; ++t) {
        // retire k-step t (this wave's share; later k-steps stay in flight), then make every wave's share visible
        // (with a tail_issue: its pieces behind the barriers of the k-steps before this one are younger still)
        const int rem = ksteps - 1 - t;
        if (rem >= NST - 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPW * (NST - 2)) : "memory");
        else if (rem == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPW + (NST - 3) * XT) : "memory");
        else if (XT != 0 && rem == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * XT) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // (a tail_issue overwrites the slot read one k-step ago: that k-step's ds_reads have returned, not merely been issued, before this wave says so at the barrier;
        //  the staging of the steady state gets the same from the loop's back edge)
        if (XT != 0 && rem <= NST - 2) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // the staging of k-step t+NST-1 (its slot was last read at k-step t-1: safe behind the barrier) is
        // interleaved with the MFMAs so that the DMA issue cost hides under matrix-pipe time
        const bool stage = t + NST - 1 < ksteps;
        if (stage) issue_begin();
        else if (XT != 0) tail_issue(NST - 2 - rem);
        const half8* L = (const half8*)(lds + slot * STAGE_U4);
        half8 bh[2], bl[2], ah[MTW], al[MTW];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            bh[c] = L[(WFR + (2 * ws + c) * 2 + 0) * 64 + lane];
            bl[c] = L[(WFR + (2 * ws + c) * 2 + 1) * 64 + lane];
        }
#pragma unroll
        for (int i = 0; i < MTW; ++i) {
            ah[i] = L[((wm * MTW + i) * 2 + 0) * 64 + lane];
            al[i] = L[((wm * MTW + i) * 2 + 1) * 64 + lane];
        }
        // term-major: the 2 MTW accumulators of the wave take the hi x hi products, then all take lo x hi, then hi x lo -- consecutive MFMAs are independent (a dependent one
        // is 2 MTW instructions away instead of 2) and every accumulator still sums its three terms in the same order: same bits
#pragma unroll
        for (int term = 0; term < 3; ++term)
#pragma unroll
            for (int i = 0; i < MTW; ++i) {
#pragma unroll
                for (int c = 0; c < 2; ++c) acc[i][c] = MFMA16(term == 1 ? al[i] : ah[i], term == 2 ? bl[c] : bh[c], acc[i][c]);
                if (stage && term == 0) {
#pragma unroll
                    for (int q = i; q < LPW; q += MTW) issue_one(q, nslot);
                }
            }
        if (stage) kt += 1;
        slot = slot + 1 == NST ? 0 : slot + 1;
        nslot = nslot + 1 == NST ? 0 : nslot + 1;
    }
}

// Where an EPI_LOGITS epilogue puts row d (LogitsDst, net.h).  No request list: the dense rows of out_logits.  With one (the run loop's lazy rounds):
// request d's row IS its node's policy row -- the same 16-byte pieces from the same lanes, only the row's base differs -- and the lane that holds output HW (the value
// in front of tanh) also writes vpre[d] and v[d], as k_softmax does for the dense rows.
__device__ inline float* logits_row(const LogitsDst& D, float* out_logits, size_t sample, int width) {
    if (!D.req_ref) return out_logits + sample * width;
    const uint32_t ref = D.req_ref[sample];
    return D.policy + ((size_t)(ref >> 16) * (size_t)D.stride_nodes + (size_t)(ref & 0xFFFFu)) * width;
}
// (two steps, so that an unrolled epilogue holds ONE tanhf: logits_value_pick in front of every piece's store -- o = outputs [col, col + 4) of the row, a few selects --
//  and logits_value_store once per sample behind its pieces; `have`: this lane held output HW of the sample)
__device__ inline void logits_value_pick(const LogitsDst& D, int col, const f32x4& o, float& x, bool& have) {
    const int q = D.hw - col;
    const bool mine = (unsigned)q < 4u;
    x = mine ? (q == 0 ? o[0] : q == 1 ? o[1] : q == 2 ? o[2] : o[3]) : x;
    have = have || mine;
}
__device__ inline void logits_value_store(const LogitsDst& D, size_t sample, float x, bool have) {
    if (D.req_ref && have) {
        D.vpre[sample] = x;
        D.v[sample] = tanhf(x);
    }
}

template <int MT, int EPI, int TAG, int NST>
__global__ __launch_bounds__(512) void k_gemm_t(const uint4* __restrict__ wp, const uint4* __restrict__ act, int ksteps,
                                                size_t act_row_u4, int k_full, int last_cnt, int lo_off,
                                                const float* __restrict__ bias, uint4* __restrict__ out_split,
                                                size_t out_row_u4, float* __restrict__ out_logits, const int32_t* __restrict__ d_count,
                                                int max_count, LogitsDst D) {
    constexpr int MTW = MT / 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint4* lds = (uint4*)smem;
    int count = d_count[0];
    if (count > max_count) count = max_count;
    const int b0 = blockIdx.x * GT_BS;
    if (b0 >= count) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, ws = wave & 1;
    const int h = lane >> 5;
    // split-K (EPI_PARTIAL, small batches): blockIdx.y owns the k-steps [kbeg, kbeg + ksteps)
    const int kbeg = EPI == EPI_PARTIAL ? (int)blockIdx.y * ksteps : 0;
    f32x16 acc[MTW][2];
    gemm_t_mainloop<MT, NST, 0>(lds, wp, act, ksteps, kbeg, act_row_u4, k_full, last_cnt, lo_off, b0, wave, lane, acc, [](int) {});

    // ---- epilogue ----
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int sample = b0 + 32 * (2 * ws + c) + (lane & 31);
        if (sample >= count) continue;
        float* lrow = EPI == EPI_LOGITS ? logits_row(D, out_logits, (size_t)sample, MT * 32) : nullptr;
        float vx = 0.0f;
        bool vhave = false;
#pragma unroll
        for (int i = 0; i < MTW; ++i) {
            const int mt = wm * MTW + i;
            float y[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 bv = *(const f32x4*)(bias + 32 * mt + 8 * g + 4 * h);
#pragma unroll
                for (int q = 0; q < 4; ++q) y[4 * g + q] = acc[i][c][4 * g + q] + bv[q];
            }
            if (EPI == EPI_PARTIAL) { // raw fp32 partial sums [split][row][MT*32]; bias/activation in k_splitk_finish
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 o;
#pragma unroll
                    for (int q = 0; q < 4; ++q) o[q] = acc[i][c][4 * g + q];
                    *(f32x4*)(out_logits + ((size_t)blockIdx.y * out_row_u4 + sample) * (MT * 32) + 32 * mt + 8 * g + 4 * h) = o;
                }
            } else if (EPI == EPI_SPLIT) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = lrelu(y[8 * s + j]);
                    half8 hi, lo;
                    split8(v, hi, lo);
                    uint4* row = out_split + (size_t)sample * out_row_u4 + (size_t)(2 * mt + s) * 4;
                    row[h] = *(const uint4*)&hi;
                    row[2 + h] = *(const uint4*)&lo;
                }
            } else {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 o;
#pragma unroll
                    for (int q = 0; q < 4; ++q) o[q] = y[4 * g + q];
                    *(f32x4*)(lrow + 32 * mt + 8 * g + 4 * h) = o;
                    logits_value_pick(D, 32 * mt + 8 * g + 4 * h, o, vx, vhave);
                }
            }
        }
        if (EPI == EPI_LOGITS) logits_value_store(D, (size_t)sample, vx, vhave);
    }
}

// ===============================================================================================
// OMOK_NET_F16X3: fc1 and the heads in one launch (whole-K rounds): h1 stays on the CU
// ===============================================================================================
// fc1's accumulator tile IS the heads' B operand, in the same lane: EPI_SPLIT stores, for m-tile mt and half s, the lane's hi at row[(2 mt + s) 4 + h] and its lo at
// row[(2 mt + s) 4 + 2 + h], and the heads' staging fetches row[4 ks + 2 part + h] of sample b0 + 32 ct + (lane & 31) into the same lane: k-step ks = 2 mt + s of the
// heads is the register content of the wave that owns fc1 m-tile mt for sample tile ct.  The whole h1 tile (256 KiB) does not fit in LDS and never has to: the heads take
// their k-steps in ascending order, which is the order of the fc1 waves' wm.
//   fc1 phase    gemm_t_mainloop<16, 3> (k_gemm_t's loop: same ring, waits, wave-to-tile map and MFMA order), then bias, LeakyReLU and split8 as EPI_SPLIT does them,
//                into registers (the 128 accumulator registers become 128 of hi|lo fragments)
//   hand-over    chunk p = the heads' k-steps 8 p .. 8 p + 7 = what the two waves with wm == p hold: they write it as 1-KiB fragments [lane] (the image a k_gemm_t
//                ring slot holds), barrier, all eight waves read the fragments of their own two sample tiles; a barrier in front of the next chunk's writes proves
//                the last reads of this one
//   heads phase  k_gemm_t<MTH>'s loop (wm owns MTH / 4 m-tiles, ws two sample tiles; hi x hi, lo x hi, hi x lo term-major) with only the weight fragments streamed:
//                a ring of 3 slots of 2 MTH KiB, one barrier per k-step, counted vmcnt waits; slots 0 and 1 are issued behind the last two barriers of the fc1 phase
// LDS (160 KiB): fc1 ring slots S0 S1 S2 of 40 KiB at 0, 40, 80 KiB.  fc1's last k-steps 29, 30, 31 sit in S2, S0, S1, so behind the barrier of k-step 30 S2 is free
// (heads slot H0 at 80 KiB) and behind that of k-step 31 S0 is (H1 at 0, H2 behind it).  The chunk buffer is the 64 KiB from 96 KiB on: S2's upper part and the 40 KiB
// the fc1 ring leaves unused, so chunk 0 is written while slower waves still read S1.
// Every fc1 and heads accumulator sums the products k_gemm_t's sum in the same order, and the fragments are the same split8 of the same fp32 values: same bits.
template <int MTH>
__global__ __launch_bounds__(512) void k_tail_fused(const uint4* __restrict__ wp_fc1, const uint4* __restrict__ act, const float* __restrict__ bias_fc1,
                                                    const uint4* __restrict__ wp_heads, const float* __restrict__ bias_heads, float* __restrict__ out_logits,
                                                    const int32_t* __restrict__ d_count, int max_count, LogitsDst D) {
    constexpr int MTW = MTH / 4;           // heads m-tiles per wave
    constexpr int WFR = MTH * 2;           // heads weight fragments per k-step
    constexpr int LPW = WFR / 8;           // LDS-DMA instructions per wave per heads k-step
    constexpr int FC1_STAGE_U4 = 40 * 64;  // one fc1 ring slot
    constexpr int H0_U4 = 2 * FC1_STAGE_U4, HST_U4 = WFR * 64; // heads ring: slot 0 at H0_U4, slots 1, 2 at 0 and HST_U4
    constexpr int CHUNK_U4 = 96 * 64;      // chunk buffer: [k-step 8][sample tile 4][hi, lo][lane]
    static_assert(WFR % 8 == 0 && 2 * HST_U4 <= FC1_STAGE_U4 && H0_U4 + HST_U4 <= CHUNK_U4, "heads ring inside the freed fc1 slots");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint4* lds = (uint4*)smem;
    int count = d_count[0];
    if (count > max_count) count = max_count;
    const int b0 = blockIdx.x * GT_BS;
    if (b0 >= count) return; // (workgroup-uniform: every barrier below is reached by all eight waves)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, ws = wave & 1;
    const int h = lane >> 5;

    const uint4* hsrc = wp_heads + (size_t)wave * 64 + lane; // this wave's heads weight fragments: f = wave + 8 i of every k-step
    auto hslot = [&](int slot) { return lds + (slot == 0 ? H0_U4 : (slot - 1) * HST_U4); };
    auto hissue_one = [&](int ks, int slot, int i) { dma16(hsrc + (size_t)ks * (WFR * 64) + i * 8 * 64, hslot(slot) + (wave + 8 * i) * 64); };
    auto hissue = [&](int ks, int slot) {
#pragma unroll
        for (int i = 0; i < LPW; ++i) hissue_one(ks, slot, i);
    };

    // ---- fc1 phase ----
    uint4 fr[4][2][2][2]; // h1 fragments of this wave: [m-tile i][sample tile c][half s = k-step 2 (4 wm + i) + s][hi, lo]
    {
        f32x16 acc[4][2];
        gemm_t_mainloop<16, 3, LPW>(lds, wp_fc1, act, 32, 0, 128, 32, 1, 2, b0, wave, lane, acc, [&](int j) { hissue(j, j); });
        // one m-tile at a time (its 16 bias values, then both sample tiles), so that the fragments take the accumulators' registers over as these die
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int mt = wm * 4 + i;
            f32x4 bv[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) bv[g] = *(const f32x4*)(bias_fc1 + 32 * mt + 8 * g + 4 * h);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                float y[16];
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int q = 0; q < 4; ++q) y[4 * g + q] = acc[i][c][4 * g + q] + bv[g][q];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = lrelu(y[8 * s + j]);
                    half8 hi, lo;
                    split8(v, hi, lo);
                    fr[i][c][s][0] = *(const uint4*)&hi;
                    fr[i][c][s][1] = *(const uint4*)&lo;
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // ---- heads phase ----
    f32x16 acc[MTW][2];
#pragma unroll
    for (int i = 0; i < MTW; ++i)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][c][r] = 0.0f;
    uint4* chunk = lds + CHUNK_U4;
    int slot = 0, nslot = 2;
    for (int p = 0; p < 4; ++p) {
        if (p) { // every wave has read the last k-step of chunk p - 1
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
        if (wm == p) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int c = 0; c < 2; ++c)
#pragma unroll
                        for (int part = 0; part < 2; ++part) chunk[(((2 * i + s) * 4 + 2 * ws + c) * 2 + part) * 64 + lane] = fr[i][c][s][part];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the chunk's writes have left this wave before the barrier below
        for (int kk = 0; kk < 8; ++kk) {
            const int ks = 8 * p + kk;
            // heads weights of k-step ks have landed (k-step ks + 1's stay in flight) and this wave's ds_reads of k-step ks - 1 have returned (the compiler moves MFMAs,
            // not LDS reads, across the barrier: the slot they read is refilled behind it); then every wave's share and chunk p are visible
            if (ks < 31) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(LPW) : "memory");
            else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            const bool stage = ks + 2 < 32; // into the slot read at k-step ks - 1: free behind this barrier
            const half8* L = (const half8*)hslot(slot);
            const half8* C = (const half8*)chunk + (size_t)(kk * 8) * 64 + lane;
            half8 bh[2], bl[2], ah[MTW], al[MTW];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                bh[c] = C[((2 * ws + c) * 2 + 0) * 64];
                bl[c] = C[((2 * ws + c) * 2 + 1) * 64];
            }
#pragma unroll
            for (int i = 0; i < MTW; ++i) {
                ah[i] = L[((wm * MTW + i) * 2 + 0) * 64 + lane];
                al[i] = L[((wm * MTW + i) * 2 + 1) * 64 + lane];
            }
#pragma unroll
            for (int term = 0; term < 3; ++term)
#pragma unroll
                for (int i = 0; i < MTW; ++i) {
#pragma unroll
                    for (int c = 0; c < 2; ++c) acc[i][c] = MFMA16(term == 1 ? al[i] : ah[i], term == 2 ? bl[c] : bh[c], acc[i][c]);
                    if (stage && term == 0) {
#pragma unroll
                        for (int q = i; q < LPW; q += MTW) hissue_one(ks + 2, nslot, q);
                    }
                }
            slot = slot + 1 == 3 ? 0 : slot + 1;
            nslot = nslot + 1 == 3 ? 0 : nslot + 1;
        }
    }

    // ---- epilogue (EPI_LOGITS) ----
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int sample = b0 + 32 * (2 * ws + c) + (lane & 31);
        if (sample >= count) continue;
        float* lrow = logits_row(D, out_logits, (size_t)sample, MTH * 32);
        float vx = 0.0f;
        bool vhave = false;
#pragma unroll
        for (int i = 0; i < MTW; ++i) {
            const int mt = wm * MTW + i;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 bv = *(const f32x4*)(bias_heads + 32 * mt + 8 * g + 4 * h);
                f32x4 o;
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q] = acc[i][c][4 * g + q] + bv[q];
                *(f32x4*)(lrow + 32 * mt + 8 * g + 4 * h) = o;
                logits_value_pick(D, 32 * mt + 8 * g + 4 * h, o, vx, vhave);
            }
        }
        logits_value_store(D, (size_t)sample, vx, vhave);
    }
}

// ===============================================================================================
// OMOK_NET_F16X3: the same GEMM with WAVE-PRIVATE weight rings (round 6; fc1 and the heads of whole-K launches)
// ===============================================================================================
// k_gemm_t stages a k-step's 40 fragments with all 8 waves and meets at a workgroup barrier per k-step of 16 (24 MFMAs per wave between barriers), and its sample fragments
// are gathered lane = sample (every lane its own 32-B segment).  Here wave w owns m-tiles [w MT/8, (w + 1) MT/8) for ALL four sample tiles: the weight fragments it
// consumes (MT/4 per k-step) go through a ring of its own -- 3 k-steps deep, filled by LDS-DMA and ordered by its own counted vmcnt waits, no barrier -- and only the
// sample operands are shared: a CHUNK of two k-steps (128 samples x 128 contiguous bytes: [k0: hi h0, hi h1, lo h0, lo h1][k1: ...]) per workgroup barrier, triple-buffered,
// DMA'd with 8 adjacent lanes on the 8 pieces of one sample (whole lines) and XOR-swizzled like k_fc0_mx's sample image so that the MFMA-fragment reads (lane = sample,
// 128-B stride) are conflict-free.  One barrier per 2 k-steps; the waves of a SIMD are not held in step by the weights.  Every accumulator sums its k-steps in order and its
// three terms as k_gemm_t does (hi x hi, lo x hi, hi x lo): same bits.
// vmcnt book-keeping (per wave, issue order): prologue B0 A0 B1 A1 A2; chunk c issues B(c+2) behind its barrier, A(2c+3) inside k-step 2c, A(2c+4) inside k-step 2c+1
// (indices past the end are clamped: re-reads into slots nobody reads again, so that the counts stay uniform).  At the top of chunk c the younger issues are
// B(c+1) A(2c+1) A(2c+2); in front of k-step 2c+1 they are A(2c+2) B(c+2) A(2c+3): 2 + 2 AF pieces both times.
// Measured (profiles/r06_ab_gemm_w.txt, three interleaved A-B pairs of the first three plies of configs[1]): tail group 25.8 -> 26.1 ms per 150 rounds and every OTHER
// group 1.2 - 1.4 % slower beside it (the package is at its power limit: a kernel that keeps its pipes busier between barriers lowers the clock for its neighbours and
// gains nothing itself).  Built, bit-identical (tests/test_gpu_tail_gemm.py), default OFF: OMOK_GEMM_W=1 selects it.
constexpr int GW_DA = 3, GW_NB = 3;
constexpr int gemm_w_lds(int mt) { return (8 * GW_DA * (mt / 8) * 2 + GW_NB * 16) * 1024; }
template <int MT, int EPI>
__global__ __launch_bounds__(512) void k_gemm_w(const uint4* __restrict__ wp, const uint4* __restrict__ act, int ksteps, size_t act_row_u4,
                                                const float* __restrict__ bias, uint4* __restrict__ out_split, size_t out_row_u4,
                                                float* __restrict__ out_logits, const int32_t* __restrict__ d_count, int max_count, LogitsDst D) {
    static_assert(MT % 8 == 0 && EPI != EPI_PARTIAL, "k_gemm_w: whole-K launches of at least one m-tile per wave");
    constexpr int MTW = MT / 8;               // m-tiles per wave
    constexpr int AF = MTW * 2;               // weight fragments (hi, lo) per wave and k-step
    constexpr int B_U4 = 128 * 8;             // one sample chunk: [128 samples][8 pieces of 16 B]
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int count = d_count[0];
    if (count > max_count) count = max_count;
    const int b0 = blockIdx.x * GT_BS;
    if (b0 >= count) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, sl = lane & 31;
    uint4* aring = (uint4*)smem + (size_t)wave * (GW_DA * AF * 64);   // this wave's ring: [slot][fragment][lane]
    uint4* ldsB = (uint4*)smem + (size_t)8 * GW_DA * AF * 64;          // [buffer][sample][piece ^ swizzle]
    const int nchunks = ksteps >> 1;                                   // (ksteps is even: 32)
    const uint4* asrc = wp + (size_t)(wave * AF) * 64 + lane;          // + kt * (MT * 2 * 64) + i * 64
    const uint4* bsrc[2];                                              // this wave's two DMA pieces of a chunk: samples 16 wave + 8 e + (lane >> 3), piece lane & 7
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int s = 16 * wave + 8 * e + (lane >> 3);
        bsrc[e] = act + (size_t)(b0 + s) * act_row_u4 + (size_t)((lane & 7) ^ ((s >> 1) & 7)); // + chunk * 8
    }
    auto issueA = [&](int kt, int slot) {
        kt = kt < ksteps ? kt : ksteps - 1;
#pragma unroll
        for (int i = 0; i < AF; ++i) dma16(asrc + (size_t)kt * (MT * 2 * 64) + i * 64, aring + (slot * AF + i) * 64);
    };
    auto issueA1 = [&](int kt, int slot, int i) {
        kt = kt < ksteps ? kt : ksteps - 1;
        dma16(asrc + (size_t)kt * (MT * 2 * 64) + i * 64, aring + (slot * AF + i) * 64);
    };
    auto issueB = [&](int ch, int buf) {
        ch = ch < nchunks ? ch : nchunks - 1;
#pragma unroll
        for (int e = 0; e < 2; ++e) dma16(bsrc[e] + ch * 8, ldsB + buf * B_U4 + (2 * wave + e) * 64);
    };
    f32x16 acc[MTW][4];
#pragma unroll
    for (int i = 0; i < MTW; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][c][r] = 0.0f;
    // read offsets (uint4) of this lane's pieces inside sample tile 0 of a chunk buffer: logical piece kk * 4 + part * 2 + h of sample sl
    int b_rd[2][2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int p = 0; p < 2; ++p) b_rd[kk][p] = sl * 8 + ((kk * 4 + p * 2 + h) ^ ((sl >> 1) & 7));
    issueB(0, 0);
    issueA(0, 0);
    issueB(1, 1);
    issueA(1, 1);
    issueA(2, 2);
    int sa = 0, bb = 0;
    for (int c = 0; c < nchunks; ++c) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 + 2 * AF) : "memory"); // this wave's share of B(c) and its A(2c) have landed
        __builtin_amdgcn_s_barrier();                                       // every wave's share of B(c) is visible; B(c - 1)'s buffer is free
        asm volatile("" ::: "memory");
        issueB(c + 2, bb == 0 ? 2 : bb - 1);
        const uint4* LB = ldsB + bb * B_U4;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            if (kk == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 + 2 * AF) : "memory"); // A(2c + 1) has landed
            const uint4* LA = aring + sa * AF * 64 + lane;
            half8 ah[MTW], al[MTW], bh[4], bl[4];
#pragma unroll
            for (int i = 0; i < MTW; ++i) {
                ah[i] = __builtin_bit_cast(half8, LA[(2 * i) * 64]);
                al[i] = __builtin_bit_cast(half8, LA[(2 * i + 1) * 64]);
            }
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                bh[ct] = __builtin_bit_cast(half8, LB[ct * 256 + b_rd[kk][0]]);
                bl[ct] = __builtin_bit_cast(half8, LB[ct * 256 + b_rd[kk][1]]);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the slot's fragments are in registers: its refill may be issued
#pragma unroll
            for (int term = 0; term < 3; ++term)
#pragma unroll
                for (int i = 0; i < MTW; ++i) {
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) acc[i][ct] = MFMA16(term == 1 ? al[i] : ah[i], term == 2 ? bl[ct] : bh[ct], acc[i][ct]);
                    if (term == 0) {
                        issueA1(2 * c + kk + 3, sa, 2 * i);
                        issueA1(2 * c + kk + 3, sa, 2 * i + 1);
                    }
                }
            sa = sa + 1 == GW_DA ? 0 : sa + 1;
        }
        bb = bb + 1 == GW_NB ? 0 : bb + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- epilogue (k_gemm_t's, accumulator (i, ct) = m-tile wave * MTW + i, sample tile ct) ----
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const int sample = b0 + 32 * ct + sl;
        if (sample >= count) continue;
        float* lrow = EPI == EPI_LOGITS ? logits_row(D, out_logits, (size_t)sample, MT * 32) : nullptr;
        float vx = 0.0f;
        bool vhave = false;
#pragma unroll
        for (int i = 0; i < MTW; ++i) {
            const int mt = wave * MTW + i;
            float y[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 bv = *(const f32x4*)(bias + 32 * mt + 8 * g + 4 * h);
#pragma unroll
                for (int q = 0; q < 4; ++q) y[4 * g + q] = acc[i][ct][4 * g + q] + bv[q];
            }
            if (EPI == EPI_SPLIT) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = lrelu(y[8 * s + j]);
                    half8 hi, lo;
                    split8(v, hi, lo);
                    uint4* row = out_split + (size_t)sample * out_row_u4 + (size_t)(2 * mt + s) * 4;
                    row[h] = *(const uint4*)&hi;
                    row[2 + h] = *(const uint4*)&lo;
                }
            } else {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 o;
#pragma unroll
                    for (int q = 0; q < 4; ++q) o[q] = y[4 * g + q];
                    *(f32x4*)(lrow + 32 * mt + 8 * g + 4 * h) = o;
                    logits_value_pick(D, 32 * mt + 8 * g + 4 * h, o, vx, vhave);
                }
            }
        }
        if (EPI == EPI_LOGITS) logits_value_store(D, (size_t)sample, vx, vhave);
    }
}

// split-K finish: sums the partials in split order (deterministic), + bias, LeakyReLU, writes the hi|lo operand row
__global__ __launch_bounds__(256) void k_splitk_finish(const float* __restrict__ part, int nsplit, size_t cap_rows,
                                                       const float* __restrict__ bias, uint4* __restrict__ out_split, size_t out_row_u4,
                                                       const int32_t* __restrict__ d_count, int max_count) {
    int count = d_count[0];
    if (count > max_count) count = max_count;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; // (sample, mt 16, s 2, h 2)
    const size_t sample = i >> 6;
    if (sample >= (size_t)count) return;
    const int piece = (int)(i & 63), mt = piece >> 2, s = (piece >> 1) & 1, h = piece & 1;
    const int n0 = 32 * mt + 16 * s + 4 * h; // j = 0..3 -> n0 + j ; j = 4..7 -> n0 + 8 + (j - 4)
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.0f;
    for (int sp = 0; sp < nsplit; ++sp) {
        const float* p = part + ((size_t)sp * cap_rows + sample) * NF + n0;
        const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] += a[j]; v[4 + j] += b[j]; }
    }
    const f32x4 ba = *(const f32x4*)(bias + n0), bb = *(const f32x4*)(bias + n0 + 8);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = lrelu(v[j] + ba[j]); v[4 + j] = lrelu(v[4 + j] + bb[j]); }
    half8 hi, lo;
    split8(v, hi, lo);
    uint4* row = out_split + sample * out_row_u4 + (size_t)(2 * mt + s) * 4;
    row[h] = *(const uint4*)&hi;
    row[2 + h] = *(const uint4*)&lo;
}

// split-K finish of the heads: partials in split order + bias -> logits rows
__global__ __launch_bounds__(256) void k_splitk_logits(const float* __restrict__ part, int nsplit, size_t cap_rows, int width, const float* __restrict__ bias,
                                                       float* __restrict__ logits, const int32_t* __restrict__ d_count, int max_count, LogitsDst D) {
    int count = d_count[0];
    if (count > max_count) count = max_count;
    const size_t per_row = (size_t)width / 4, total = (size_t)count * per_row;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t row = i / per_row, col = (i % per_row) * 4;
        f32x4 a = *(const f32x4*)(part + row * width + col);
        for (int sp = 1; sp < nsplit; ++sp) {
            const f32x4 b = *(const f32x4*)(part + ((size_t)sp * cap_rows + row) * width + col);
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] += b[j];
        }
        const f32x4 bv = *(const f32x4*)(bias + col);
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] += bv[j];
        *(f32x4*)(logits_row(D, logits, row, width) + col) = a;
        float vx = 0.0f;
        bool vhave = false;
        logits_value_pick(D, (int)col, a, vx, vhave);
        logits_value_store(D, row, vx, vhave);
    }
}

// policy softmax (network.rs:236-247) + value tanh (network.rs:197-200); one wave per sample
__global__ __launch_bounds__(64) void k_softmax(const float* __restrict__ logits, int lrow, int hw, int rowp, float* __restrict__ p,
                                                float* __restrict__ v, float* __restrict__ vpre, const int32_t* __restrict__ d_count, int max_count) {
    int count = d_count[0];
    if (count > max_count) count = max_count;
    const int lane = threadIdx.x;
    for (int s = blockIdx.x; s < count; s += gridDim.x) {
        const float* l = logits + (size_t)s * lrow;
        float mx = -INFINITY;
        for (int a = lane; a < hw; a += 64) mx = fmaxf(mx, l[a]);
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        float sum = 0.0f, e[4] = {0.0f, 0.0f, 0.0f, 0.0f}; // rowp <= 256: at most 4 cells per lane
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int a = lane + 64 * i;
            if (a < hw) { e[i] = expf(l[a] - mx); sum += e[i]; }
        }
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int a = lane + 64 * i;
            if (a < rowp) p[(size_t)s * rowp + a] = a < hw ? e[i] / sum : 0.0f;
        }
        if (lane == 0) { v[s] = tanhf(l[hw]); vpre[s] = l[hw]; }
    }
}

// ===============================================================================================
// host: packing + launch
// ===============================================================================================
static inline void split_h(float x, _Float16& hi, _Float16& lo) {
    hi = (_Float16)x;
    lo = (_Float16)(x - (float)hi);
}

// Packs W (element (k, m) via getw) into [ksteps][MT][hi|lo][lane][8]; kidx(ks, h, j) -> source k
template <typename GetW, typename KIdx>
static void pack_A(std::vector<_Float16>& out, int ksteps, int MT, GetW getw, KIdx kidx) {
    out.assign((size_t)ksteps * MT * 2 * 64 * 8, (_Float16)0.0f);
    for (int ks = 0; ks < ksteps; ++ks)
        for (int mt = 0; mt < MT; ++mt)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int r = l & 31, h = l >> 5;
                    const float w = getw(kidx(ks, h, j), 32 * mt + r);
                    _Float16 hi, lo;
                    split_h(w, hi, lo);
                    const size_t base = (((size_t)ks * MT + mt) * 2) * 512 + (size_t)l * 8 + j;
                    out[base] = hi;
                    out[base + 512] = lo;
                }
}

// fp6 e2m3 (1 sign, 2 exponent, 3 mantissa; subnormal step 0.125, normals 1..7.5, no NaN / Inf): round to nearest even, saturating
static uint8_t to_e2m3(float x) {
    const uint8_t sign = x < 0.0f ? 0x20 : 0x00;
    const float a = fabsf(x);
    if (!(a == a)) return sign;
    if (a >= 7.5f) return sign | 0x1f;
    int best = 0;
    float bd = 1e30f;
    for (int c = 0; c < 32; ++c) {
        const int ex = c >> 3, m = c & 7;
        const float v = ex == 0 ? m * 0.125f : (1.0f + m * 0.125f) * (float)(1 << (ex - 1));
        const float d = fabsf(v - a);
        if (d < bd || (d == bd && !(c & 1))) { bd = d; best = c; }
    }
    return sign | (uint8_t)best;
}
// E8M0 byte of the MX block scale for a block whose largest magnitude is amax: 2^(floor(log2 amax) - 2) (e2m3 emax = 2)
static int mx6_scale_byte(float amax) {
    if (!(amax > 0.0f)) return 1;
    int e;
    frexpf(amax * MX6_AMAX_ADJ, &e); // x = m * 2^e, m in [0.5, 1): floor(log2 x) = e - 1
    int E = 127 + (e - 1) - 2;
    return E < 1 ? 1 : (E > 254 ? 254 : E);
}

static int heads_mt(int hw) { return ((hw + 1 + 31) / 32 + 3) / 4 * 4; }

const float* net_logits(const Net& net, int* row_stride) {
    if (net.mode == OMOK_NET_F32) { *row_stride = net.hw; return net.sh; } // forward_f32 leaves the chunk's logits in sh
    *row_stride = heads_mt(net.hw) * 32;
    return net.s0;
}

size_t net_alloc(Net& net) {
    const size_t hw = net.hw, rp = net.rowp;
    const size_t mb = ((size_t)net.max_b + GT_BS - 1) / GT_BS * GT_BS;
    size_t bytes = 0;
    auto A = [&](void** p, size_t n) {
        if (hipMalloc(p, n ? n : 16) != hipSuccess) return false;
        hipMemset(*p, 0, n ? n : 16);
        bytes += n;
        return true;
    };
    bool ok = true;
    for (int i = 0; i < NET_TENSORS && ok; ++i) ok = A((void**)&net.w[i], sizeof(float) * (size_t)net.wsize[i]);
    ok = ok && A((void**)&net.p, sizeof(float) * mb * rp);
    ok = ok && A((void**)&net.v, sizeof(float) * mb);
    ok = ok && A((void**)&net.vpre, sizeof(float) * mb);
    ok = ok && A((void**)&net.in_f32, sizeof(float) * mb * 3 * hw);
    net.cfg_mode = net.mode;
    if (net.mode == OMOK_NET_F32) {
        net.chunk = (int)std::min<size_t>(mb, 1024);
        const size_t c = net.chunk;
        ok = ok && A((void**)&net.sx, sizeof(float) * c * hw * NC);
        ok = ok && A((void**)&net.sh, sizeof(float) * c * hw * NM);
        ok = ok && A((void**)&net.sd, sizeof(float) * c * hw * NM);
        ok = ok && A((void**)&net.sg, sizeof(float) * c * hw * NM);
        ok = ok && A((void**)&net.s0, sizeof(float) * c * NF);
        ok = ok && A((void**)&net.s1, sizeof(float) * c * NF);
    } else {
        const size_t ks0 = hw * 8;
        const size_t row_pad = 80;
        net.row_u4_fmt[FC0_FP6] = (size_t)((hw + 31) / 32) * 2 * OP_BLK_U4 + row_pad;
        net.row_u4_fmt[FC0_F16] = (size_t)((hw + 31) / 32) * 2 * OPX_BLK_U4 + row_pad;
        net.row_u4 = net.row_u4_fmt[net.fc0_fmt];
        const size_t row_u4 = net.row_u4_fmt[FC0_F16]; // buffers are sized for the larger format: the format can change at every commit
        ok = ok && A(&net.wt_trunk, TR_WBYTES + TR_CONV_FRAGS * 1024);
        ok = ok && A((void**)&net.wt_first, sizeof(float) * (TR_SIDE_FLOATS + 2 * NF + heads_mt(net.hw) * 32));
        ok = ok && A((void**)&net.conv_tab, sizeof(float) * CT_FLOATS);
        ok = ok && A(&net.wt_fc0, (ks0 + 4) * (size_t)MXS_FR * 1024); // hw*2 super-steps x 4 stages (= ks0) + 4 stages of padding (prefetch depth)
        ok = ok && A(&net.wt_fc0x, (2 * ks0 + 8) * (size_t)X3_FR * 1024); // FC0_F16: hw*4 half-steps x 4 stages + 8 stages of padding
        ok = ok && A(&net.wt_fc1, (size_t)32 * 16 * 2 * 1024);
        ok = ok && A(&net.wt_heads, (size_t)32 * heads_mt(net.hw) * 2 * 1024);
        ok = ok && A(&net.a_fc0, mb * row_u4 * 16 + 2 * OPX_BLK_U4 * 16); // + slack: the prefetch of the super-step past the last one reads one block beyond the row
        ok = ok && A(&net.h0, mb * 32 * 64 * 2);       // h0 and h1 rows (2 KiB each)
        ok = ok && A((void**)&net.s0, sizeof(float) * mb * heads_mt(net.hw) * 32); // logits
        { // sibling path of the trunk (k_group / k_trunk_sib): run lists and the per-workgroup base scratch
            ok = ok && A((void**)&net.d_groups, sizeof(uint2) * (mb / SIB_MIN + 1));
            ok = ok && A((void**)&net.d_singles, sizeof(int32_t) * mb);
            ok = ok && A((void**)&net.d_gcnt, sizeof(int32_t) * SIB_CNT_INTS);
            ok = ok && A((void**)&net.d_work, sizeof(unsigned long long) * NET_WORK_COUNT);
            if (ok) hipMemset(net.d_work, 0, sizeof(unsigned long long) * NET_WORK_COUNT);
            ok = ok && A((void**)&net.d_sib_rows, sizeof(uint4) * mb);
            net.base_slots = (size_t)SIB_WAYS * net.games + mb / SIB_MIN + 1; // SIB_WAYS slots per game + the other runs a round can hold
            // V2 children (Net::sib_v2, the default; omok_debug_set_children_kernel(1): k_sib_children on the difference path too): a base slot holds 1280 B per pixel instead of 3 h grids
            ok = ok && A((void**)&net.sib_h, net.base_slots * std::max<size_t>(sizeof(float) * 3 * (size_t)sib_hb_floats(net.n), sib2_slot_u4(net.n) * 16)); // (either kernel's slots: omok_debug_set_children_kernel)
            // difference path: slots (bins padded to whole tiles), their difference rows
            net.d_slots = mb + (size_t)(SIB_BINS + 1) * GT_BS;
            ok = ok && A((void**)&net.d_sib_slot, sizeof(uint32_t) * mb);
            ok = ok && A((void**)&net.d_bin_start, sizeof(int32_t) * 256);
            ok = ok && A((void**)&net.d_tile_info, sizeof(int32_t) * 2 * (net.d_slots / GT_BS)); // [tile] info, then [position] the whole-K launch's tile order
            ok = ok && A(&net.d_slot_desc, sizeof(uint2) * net.d_slots);
            ok = ok && A(&net.d_rows, net.d_slots * (size_t)SIBX_DROW_U4 * 16);
            ok = ok && A(&net.a_base, net.base_slots * row_u4 * 16);
            ok = ok && A((void**)&net.facc, sizeof(float) * (net.base_slots + mb) * NF);
            ok = ok && A((void**)&net.d_tags, sizeof(int32_t) * (size_t)SIB_WAYS * (size_t)(net.games > 0 ? net.games : 1));
            ok = ok && A(&net.d_comp, sizeof(uint2) * (mb / SIB_MIN + 1));
            hipDeviceProp_t prop;
            net.n_cu = (hipGetDeviceProperties(&prop, net.device) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256; // (the one query: every planner reads net.n_cu)
            net.part_w_rows = std::min<size_t>((size_t)net.n_cu * GT_BS, net.d_slots); // K-split window tiles: at most one round of workgroups, 7 ways
            ok = ok && A((void**)&net.part_w, sizeof(float) * net.part_w_rows * 7 * NF);
        }
        net.part_rows = mb * 8 > 32768 ? mb * 8 : 32768;                                // split-K partials: rows x split ways (2 KiB each)
        ok = ok && A((void**)&net.part, sizeof(float) * net.part_rows * NF);
    }
    if (!ok) { net_free(net); return 0; }
    net.bytes = bytes;
    return bytes;
}

void net_free(Net& net) {
    if (net.s0_x3 || net.s0_f32) { // (a split-precision engine that has taken the fp32 fallback holds two buffers behind s0)
        net.s0 = nullptr;
        if (net.s0_x3) hipFree(net.s0_x3);
        if (net.s0_f32) hipFree(net.s0_f32);
        net.s0_x3 = net.s0_f32 = nullptr;
    }
    void** ptrs[] = {(void**)&net.p, (void**)&net.v, (void**)&net.vpre, (void**)&net.in_f32, (void**)&net.sx, (void**)&net.sh, (void**)&net.sd,
                     (void**)&net.sg, (void**)&net.s0, (void**)&net.s1, &net.wt_trunk, (void**)&net.wt_first, (void**)&net.conv_tab, &net.wt_fc0,
                     &net.wt_fc0x, &net.wt_fc1, &net.wt_heads, &net.a_fc0, &net.h0, (void**)&net.part, (void**)&net.d_groups,
                     (void**)&net.d_singles, (void**)&net.d_gcnt, (void**)&net.d_work, (void**)&net.sib_h, (void**)&net.d_sib_rows, (void**)&net.d_sib_slot,
                     (void**)&net.d_bin_start, (void**)&net.d_tile_info, &net.d_slot_desc, &net.d_rows, (void**)&net.part_w, &net.a_base, (void**)&net.facc, (void**)&net.d_tags, &net.d_comp};
    for (void** p : ptrs) { if (*p) hipFree(*p); *p = nullptr; }
    for (int i = 0; i < NET_TENSORS; ++i) { if (net.w[i]) hipFree(net.w[i]); net.w[i] = nullptr; }
}

static int net_probe(Net& net, const Store& S, hipStream_t st);
static int net_pack(Net& net, hipStream_t st);

void net_set_fc0_format(Net& net, int fmt) { // FC0_FP6 / FC0_F16 / FC0_MIXED
    net.fc0_fmt = fmt == FC0_FP6 ? FC0_FP6 : FC0_F16;
    net.diff_fp6 = fmt == FC0_MIXED;
    net.row_u4 = net.row_u4_fmt[net.fc0_fmt];
    net.sib_cache_valid = false; // (cached base rows are in the other format)
}

// The last rung of the format ladder: a split-precision engine whose probe is outside the 1e-3 contract even with f16 correction terms evaluates with the fp32 kernels
// (scratch for chunks of up to 1024 rows, allocated at the first such commit) until a later commit is inside again.
static int net_enter_f32_fallback(Net& net) {
    const size_t hw = net.hw, mb = ((size_t)net.max_b + GT_BS - 1) / GT_BS * GT_BS;
    if (!net.s0_f32) {
        const size_t c = std::min<size_t>(mb, 1024);
        bool ok = hipMalloc((void**)&net.sx, sizeof(float) * c * hw * NC) == hipSuccess;
        ok = ok && hipMalloc((void**)&net.sh, sizeof(float) * c * hw * NM) == hipSuccess;
        ok = ok && hipMalloc((void**)&net.sd, sizeof(float) * c * hw * NM) == hipSuccess;
        ok = ok && hipMalloc((void**)&net.sg, sizeof(float) * c * hw * NM) == hipSuccess;
        ok = ok && hipMalloc((void**)&net.s0_f32, sizeof(float) * c * NF) == hipSuccess;
        ok = ok && hipMalloc((void**)&net.s1, sizeof(float) * c * NF) == hipSuccess;
        if (!ok) return -1;
        net.s0_x3 = net.s0;
    }
    net.chunk = (int)std::min<size_t>(mb, 1024);
    net.s0 = net.s0_f32;
    net.mode = OMOK_NET_F32;
    net.sib_cache_valid = false;
    return 0;
}

int net_commit(Net& net, const Store& S, hipStream_t st) {
    if (net.cfg_mode == OMOK_NET_F32) return 0;
    if (net.mode != net.cfg_mode) { // (the previous commit had fallen back to the fp32 kernels: the new weights get their own verdict)
        net.mode = net.cfg_mode;
        net.s0 = net.s0_x3;
    }
    net.probe_outside = 0;
    const int rc = net_pack(net, st);
    if (rc != 0) return rc;
    static const char* force = getenv("OMOK_FC0_FMT"); // fp6 | f16: overrides the engine's policy (A-B runs)
    int policy = net.fc0_policy;
    if (force && !strcmp(force, "fp6")) policy = FC0_FP6;
    if (force && !strcmp(force, "f16")) policy = FC0_F16;
    if (force && !strcmp(force, "mixed")) policy = FC0_MIXED;
    for (int i = 0; i < 24; ++i) net.probe[i] = 0.0f;
    if (policy != FC0_AUTO) { net_set_fc0_format(net, policy); return 0; } // (a forced format is the caller's decision: no probe, no fallback)
    const int prc = net_probe(net, S, st);
    if (prc != 0) return prc;
    if (net.probe_outside == 2 && net_enter_f32_fallback(net) != 0) return -1;
    return 0;
}

static int net_pack(Net& net, hipStream_t st) {
    const int hw = net.hw;
    std::vector<std::vector<float>> T(NET_TENSORS);
    for (int i = 0; i < NET_TENSORS; ++i) {
        T[i].resize((size_t)net.wsize[i]);
        if (hipMemcpy(T[i].data(), net.w[i], sizeof(float) * T[i].size(), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    }
    // ---- trunk fragments ----
    std::vector<_Float16> trunk((size_t)(TR_WBYTES + TR_CONV_FRAGS * 1024) / 2, (_Float16)0.0f);
    std::vector<float> side((size_t)TR_SIDE_FLOATS + 2 * NF + heads_mt(hw) * 32, 0.0f);
    auto put = [&](int blk, int frag, const std::vector<_Float16>& src, int ksteps, int MT, int part, int ks, int mt) {
        const size_t s = (((size_t)ks * MT + mt) * 2 + part) * 512;
        memcpy(&trunk[((size_t)blk * TR_FRAGS_PER_BLOCK + frag) * 512], &src[s], 1024);
    };
    for (int b = 0; b < 3; ++b) {
        const float *w0 = T[2 + 7 * b].data(), *b0 = T[3 + 7 * b].data(), *dw = T[4 + 7 * b].data(), *pw = T[5 + 7 * b].data(),
                    *b1 = T[6 + 7 * b].data(), *w2 = T[7 + 7 * b].data(), *b2 = T[8 + 7 * b].data();
        std::vector<_Float16> p0, p1, p2;
        auto kchain = [](int ks, int h, int j) { return kperm(ks >> 1, ks & 1, h, j); };
        pack_A(p0, 8, 1, [&](int k, int m) { return w0[k * NM + m]; }, kchain);
        pack_A(p1, 2, 1, [&](int k, int m) { return pw[k * NM + m]; }, kchain);
        pack_A(p2, 2, 4, [&](int k, int m) { return w2[k * NC + m]; }, kchain);
        for (int ks = 0; ks < 8; ++ks) { put(b, 0 + ks, p0, 8, 1, 0, ks, 0); put(b, 8 + ks, p0, 8, 1, 1, ks, 0); }
        for (int ks = 0; ks < 2; ++ks) { put(b, 16 + ks, p1, 2, 1, 0, ks, 0); put(b, 18 + ks, p1, 2, 1, 1, ks, 0); }
        for (int m = 0; m < 4; ++m)
            for (int ks = 0; ks < 2; ++ks) { put(b, 20 + m * 2 + ks, p2, 2, 4, 0, ks, m); put(b, 28 + m * 2 + ks, p2, 2, 4, 1, ks, m); }
        float* sd = side.data() + b * TR_SIDE_PER_BLOCK;
        memcpy(sd, dw, sizeof(float) * 9 * NM); // [3][3][32][1] -> [tap][c]
        memcpy(sd + 9 * NM, b0, sizeof(float) * NM);
        memcpy(sd + 10 * NM, b1, sizeof(float) * NM);
        memcpy(sd + 11 * NM, b2, sizeof(float) * NC);
    }
    { // conv_in as one 16-deep k-step: k = 0..2 input floats, k = 3 bias (network.rs:65-76)
        const float *cw = T[0].data(), *cb = T[1].data();
        std::vector<_Float16> pc;
        pack_A(pc, 1, 4, [&](int k, int m) { return k < 3 ? cw[k * NC + m] : (k == 3 ? cb[m] : 0.0f); },
               [](int, int h, int j) { return 8 * h + j; });
        for (int m = 0; m < 4; ++m) {
            memcpy(&trunk[((size_t)3 * TR_FRAGS_PER_BLOCK + m) * 512], &pc[((size_t)m * 2 + 0) * 512], 1024);
            memcpy(&trunk[((size_t)3 * TR_FRAGS_PER_BLOCK + 4 + m) * 512], &pc[((size_t)m * 2 + 1) * 512], 1024);
        }
    }
    // biases of fc0, fc1, heads behind the trunk side table
    float* bias_fc0 = side.data() + TR_SIDE_FLOATS;
    float* bias_fc1 = bias_fc0 + NF;
    float* bias_heads = bias_fc1 + NF;
    memcpy(bias_fc0, T[24].data(), sizeof(float) * NF);
    memcpy(bias_fc1, T[26].data(), sizeof(float) * NF);
    memcpy(bias_heads, T[30].data(), sizeof(float) * hw);
    bias_heads[hw] = T[28][0];
    // ---- fc0 (k_fc0_mx): super-steps (K = 64 = one pixel x 64 channels) enumerate (tile, q, pixel-in-tile) over
    //      the valid pixels; stage (u, g) = 32 fragments: [i: m-tile 4g+i][hi j0..j3 | w_hi8 half0, half1 | w_lo8
    //      half0, half1].  Source row of fc0_w = px*128 + 32*m + kperm-order channel (flatten index (y*N+x)*128+c). ----
    std::vector<_Float16> pk;
    {
        const float* w = T[23].data();
        const int tiles = (hw + 31) / 32;
        float wmax = 0.0f;
        for (size_t i = 0; i < T[23].size(); ++i) wmax = fmaxf(wmax, fabsf(w[i]));
        int SW = wmax > 0.0f ? (int)floorf(log2f(240.0f / wmax)) : 0;
        if (SW < -20) SW = -20;
        if (SW > 40) SW = 40;
        net.mx_sw = SW;
        std::vector<uint8_t> buf;
        std::vector<int> upx, uq;
        for (int tile = 0; tile < tiles; ++tile)
            for (int q = 0; q < 2; ++q)
                for (int pl = 0; pl < 32 && tile * 32 + pl < hw; ++pl) { upx.push_back(tile * 32 + pl); uq.push_back(q); }
        const size_t nsup = upx.size();
        buf.assign((nsup * 4 + 4) * MXS_FR * 1024, 0);
        for (size_t u = 0; u < nsup; ++u)
            for (int g = 0; g < 4; ++g)
                for (int i = 0; i < 4; ++i) {
                    uint8_t* st = buf.data() + ((u * 4 + g) * MXS_FR + (size_t)i * 6) * 1024;
                    const int mt = 4 * g + i;
                    for (int l = 0; l < 64; ++l) {
                        const int r = l & 31, hh = l >> 5, n = 32 * mt + r;
                        { // fragments 4, 5 = [lane][fp6 dwords 0..3] | [lane][fp6 dwords 4, 5 | scale bytes (hi copy, residual) | 0]
                            float whf[32], wlf[32], ah = 0.0f, al = 0.0f;
                            for (int slot = 0; slot < 32; ++slot) {
                                const int mm = slot >> 4, reg = slot & 15;
                                const size_t k = (size_t)upx[u] * NC + kperm(2 * uq[u] + mm, reg >> 3, hh, reg & 7);
                                const float wv = w[k * NF + n];
                                whf[slot] = (float)(_Float16)wv;
                                wlf[slot] = wv - whf[slot];
                                ah = fmaxf(ah, fabsf(whf[slot]));
                                al = fmaxf(al, fabsf(wlf[slot]));
                            }
                            const int Eh = mx6_scale_byte(ah), El = mx6_scale_byte(al);
                            uint32_t pk6[6] = {0, 0, 0, 0, 0, 0};
                            for (int slot = 0; slot < 32; ++slot) {
                                const uint32_t code = to_e2m3(ldexpf(wlf[slot], 127 - El));
                                const int bit = 6 * slot;
                                pk6[bit >> 5] |= code << (bit & 31);
                                if ((bit & 31) > 26) pk6[(bit >> 5) + 1] |= code >> (32 - (bit & 31));
                            }
                            memcpy(st + (size_t)4 * 1024 + (size_t)l * 16, pk6, 16);
                            const uint32_t tail[4] = {pk6[4], pk6[5], (uint32_t)Eh | ((uint32_t)El << 8), 0u};
                            memcpy(st + (size_t)5 * 1024 + (size_t)l * 16, tail, 16);
                        }
                        for (int slot = 0; slot < 32; ++slot) { // byte slot = 16*(m&1) + reg, reg = 8*s + jj
                            const int mm = slot >> 4, reg = slot & 15;
                            const int m = 2 * uq[u] + mm;
                            const size_t k = (size_t)upx[u] * NC + kperm(m, reg >> 3, hh, reg & 7);
                            const float wv = w[k * NF + n];
                            const _Float16 wh = (_Float16)wv;
                            const int j = 2 * mm + (reg >> 3), jj = reg & 7; // f16 piece j, element jj
                            memcpy(st + (size_t)j * 1024 + (size_t)l * 16 + jj * 2, &wh, 2);
                        }
                    }
                }
        if (hipMemcpyAsync(net.wt_fc0, buf.data(), buf.size(), hipMemcpyHostToDevice, st) != hipSuccess) return -1;
        hipStreamSynchronize(st);
        // ---- fc0, FC0_F16 format (k_fc0_x3): half-step v = 2 u + mm (K = 32: m = 2 q + mm of super-step u's pixel); stage (v, g) = 16 fragments
        //      [i: m-tile 4g+i][hi s0 | hi s1 | lo s0 | lo s1], fragment = [lane (r, hh)][8]: k = px*128 + kperm(m, s, hh, j), lo = f16(w - f16(w)) ----
        std::vector<_Float16> xb(((size_t)nsup * 2 * 4 + 8) * X3_FR * 512, (_Float16)0.0f);
        for (size_t u = 0; u < nsup; ++u)
            for (int mm = 0; mm < 2; ++mm)
                for (int g = 0; g < 4; ++g)
                    for (int i = 0; i < 4; ++i) {
                        _Float16* stg = xb.data() + ((((size_t)u * 2 + mm) * 4 + g) * X3_FR + (size_t)i * 4) * 512;
                        const int mt = 4 * g + i, m = 2 * uq[u] + mm;
                        for (int sx = 0; sx < 2; ++sx)
                            for (int l = 0; l < 64; ++l) {
                                const int r = l & 31, hh = l >> 5, n = 32 * mt + r;
                                for (int j = 0; j < 8; ++j) {
                                    const size_t k = (size_t)upx[u] * NC + kperm(m, sx, hh, j);
                                    _Float16 wh, wl;
                                    split_h(w[k * NF + n], wh, wl);
                                    stg[(size_t)sx * 512 + l * 8 + j] = wh;
                                    stg[(size_t)(2 + sx) * 512 + l * 8 + j] = wl;
                                }
                            }
                    }
        if (hipMemcpyAsync(net.wt_fc0x, xb.data(), xb.size() * 2, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
        hipStreamSynchronize(st);
    }
    {
        const float* w = T[25].data();
        pack_A(pk, 32, 16, [&](int k, int m) { return w[(size_t)k * NF + m]; },
               [](int ks, int h, int j) { return kperm(ks >> 1, ks & 1, h, j); });
        if (hipMemcpyAsync(net.wt_fc1, pk.data(), pk.size() * 2, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
        hipStreamSynchronize(st);
    }
    {
        const float *pw = T[29].data(), *vw = T[27].data();
        const int MT = heads_mt(hw);
        pack_A(pk, 32, MT, [&](int k, int m) { return m < hw ? pw[(size_t)k * hw + m] : (m == hw ? vw[k] : 0.0f); },
               [](int ks, int h, int j) { return kperm(ks >> 1, ks & 1, h, j); });
        if (hipMemcpyAsync(net.wt_heads, pk.data(), pk.size() * 2, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
        hipStreamSynchronize(st);
    }
    if (hipMemcpyAsync(net.wt_trunk, trunk.data(), trunk.size() * 2, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    if (hipMemcpyAsync(net.wt_first, side.data(), side.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    k_conv_tables<<<1, 64, 0, st>>>((const uint4*)net.wt_trunk, net.wt_first, net.conv_tab); // (behind the two uploads it reads)
    hipStreamSynchronize(st);
    return 0;
}

template <int N, bool FROM_F32, bool BASE = false, bool DELTA = false, bool F16LO = false>
static void launch_trunk(Net& net, const Store& S, int max_count, hipStream_t st, const int32_t* row_list = nullptr, const int32_t* d_nrows = nullptr,
                         const int32_t* d_out_base = nullptr, const int32_t* d_nrows2 = nullptr, bool v2 = false, const BinPrefixArgs* role = nullptr) {
    using TG = TrunkGeo<N>;
    static bool attr_done[64] = {}; // per device: the attribute belongs to the device's copy of the code object
    auto kern = k_trunk<N, FROM_F32, BASE, DELTA, F16LO>;
    if (!attr_done[net.device & 63]) {
        hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, TG::LDS_BYTES);
        attr_done[net.device & 63] = true;
    }
    const int wgs = (max_count + TG::SPW - 1) / TG::SPW;
    // BASE && DELTA: workgroup 0 is bin_prefix_role (`role`: its arguments), the sample workgroups follow -- 256 workgroups in all as before, so that every one is
    // resident from the start (the trunk's LDS allows one per CU): the role's CU idles behind it for the rest of the launch instead of a 257th workgroup starting late
    constexpr int ROLE_WGS = (BASE && DELTA) ? 1 : 0;
    const int grid = (wgs < 256 - ROLE_WGS ? wgs : 256 - ROLE_WGS) + ROLE_WGS;
    kern<<<grid, TG::WG_THREADS, TG::LDS_BYTES, st>>>(S.req_ref, S.req_aux, S.board, S.hdr, S.d_count, S.stride_nodes, net.in_f32, (const uint4*)net.wt_trunk, net.wt_first,
                                                       (uint4*)net.a_fc0, net.row_u4, max_count, row_list, d_nrows,
                                                       (BASE && DELTA) ? (const uint2*)net.d_comp : (const uint2*)net.d_groups, net.sib_h, d_out_base, (uint4*)net.a_base,
                                                       d_nrows2, v2 ? (uint4*)net.sib_h : nullptr, role ? *role : BinPrefixArgs{});
}

// the same in the engine's current operand format (F16LO = FC0_F16 rows)
template <int N, bool FROM_F32, bool BASE = false, bool DELTA = false>
static void launch_trunk_fmt(Net& net, const Store& S, int max_count, hipStream_t st, const int32_t* row_list = nullptr, const int32_t* d_nrows = nullptr,
                             const int32_t* d_out_base = nullptr, const int32_t* d_nrows2 = nullptr, bool v2 = false, const BinPrefixArgs* role = nullptr) {
    if (net.fc0_fmt == FC0_F16) launch_trunk<N, FROM_F32, BASE, DELTA, true>(net, S, max_count, st, row_list, d_nrows, d_out_base, d_nrows2, v2, role);
    else launch_trunk<N, FROM_F32, BASE, DELTA, false>(net, S, max_count, st, row_list, d_nrows, d_out_base, d_nrows2, v2, role);
}

template <int MT, int EPI, int TAG, int NST = 3>
static void launch_gemm(const void* wp, const void* act, int ksteps, size_t act_row_u4, int k_full, int last_cnt, int lo_off,
                        const float* bias, void* out_split, size_t out_row_u4, float* out_logits, const Store& S, int max_count,
                        hipStream_t st, int device, int nsplit = 1, const LogitsDst& D = LogitsDst{}) {
    constexpr int LDS = (MT * 2 + 8) * 1024 * NST;
    static bool attr_done[64] = {};
    auto kern = k_gemm_t<MT, EPI, TAG, NST>;
    if (!attr_done[device & 63]) {
        hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
        attr_done[device & 63] = true;
    }
    const dim3 grid((max_count + GT_BS - 1) / GT_BS, nsplit);
    kern<<<grid, 512, LDS, st>>>((const uint4*)wp, (const uint4*)act, ksteps, act_row_u4, k_full, last_cnt, lo_off, bias, (uint4*)out_split,
                                  out_row_u4, out_logits, S.d_count, max_count, D);
}

template <int MTH>
static void launch_tail_fused(const void* wp_fc1, const void* act, const float* bias_fc1, const void* wp_heads, const float* bias_heads, float* out_logits, const Store& S,
                              int max_count, hipStream_t st, int device, const LogitsDst& D) {
    constexpr int LDS = 160 * 1024;
    static bool attr_done[64] = {};
    auto kern = k_tail_fused<MTH>;
    if (!attr_done[device & 63]) {
        hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
        attr_done[device & 63] = true;
    }
    kern<<<dim3((max_count + GT_BS - 1) / GT_BS), 512, LDS, st>>>((const uint4*)wp_fc1, (const uint4*)act, bias_fc1, (const uint4*)wp_heads, bias_heads, out_logits, S.d_count,
                                                                 max_count, D);
}

template <int MT, int EPI>
static void launch_gemm_w(const void* wp, const void* act, int ksteps, size_t act_row_u4, const float* bias, void* out_split, size_t out_row_u4, float* out_logits,
                          const Store& S, int max_count, hipStream_t st, int device, const LogitsDst& D = LogitsDst{}) {
    constexpr int LDS = gemm_w_lds(MT);
    static_assert(LDS <= 160 * 1024, "k_gemm_w LDS");
    static bool attr_done[64] = {};
    auto kern = k_gemm_w<MT, EPI>;
    if (!attr_done[device & 63]) {
        hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
        attr_done[device & 63] = true;
    }
    kern<<<dim3((max_count + GT_BS - 1) / GT_BS), 512, LDS, st>>>((const uint4*)wp, (const uint4*)act, ksteps, act_row_u4, bias, (uint4*)out_split, out_row_u4, out_logits,
                                                                 S.d_count, max_count, D);
}

// K splits of the difference path's fc0 launches (chosen on the device, bin_prefix_role): the full rows up to 30 ways as far as the
// partial slab holds ways x (the launch's row capacity); window tiles of the split set up to 14 ways (7 super-steps each)
constexpr int SIB_MAX_WWAYS = 14;
// (capped on the device by the slab: part_rows / (tiles of full rows x 128), and by CUs / tiles; 30 until round 4; per full round in the mixed format: k_fc0_x3 on the
//  full rows 73.7 -> 64.5 us, k_facc_reduce 9.6 -> 13.2 us)
constexpr int SIB_MAX_FWAYS = 64;
__global__ void k_zero_ints(int32_t* __restrict__ p, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) p[i] = 0;
}
// delta = false: copy path (the base row is stored into every child row, the children overwrite their windows; fc0 unchanged).
// delta = true: difference path (full rows for the runs' bases and the single rows, difference rows for the children; fc0 = launch_fc0_delta).
typedef void (*sib_kernel_t)(const uint64_t*, const uint4*, const float*, uint4*, size_t, const uint4*, const int32_t*, const float*, const uint32_t*, const int32_t*,
                             uint4*, uint2*, unsigned long long*);
static sib_kernel_t sib_kernel(bool delta, bool x16, int n) { // k_sib_children<DELTA, F16LO, N>
    if (n == 9) return delta ? (x16 ? k_sib_children<true, true, 9> : k_sib_children<true, false, 9>)
                             : (x16 ? k_sib_children<false, true, 9> : k_sib_children<false, false, 9>);
    return delta ? (x16 ? k_sib_children<true, true, 15> : k_sib_children<true, false, 15>)
                 : (x16 ? k_sib_children<false, true, 15> : k_sib_children<false, false, 15>);
}
typedef void (*sib2_kernel_t)(const uint64_t*, const uint4*, const float*, uint4*, size_t, const uint4*, const int32_t*, const uint4*, const uint32_t*, const int32_t*,
                              uint4*, uint2*, unsigned long long*, const uint4*, const FaccReduceArgs);
static sib2_kernel_t sib2_kernel(bool x16, int n, bool mixed = false) { // k_sib_children2<F16LO, N, false, OUT_F16>
    if (mixed) return n == 9 ? k_sib_children2<true, 9, false, false> : k_sib_children2<true, 15, false, false>;
    if (n == 9) return x16 ? k_sib_children2<true, 9> : k_sib_children2<false, 9>;
    return x16 ? k_sib_children2<true, 15> : k_sib_children2<false, 15>;
}
static void launch_fc0_full_rows(Net& net, int max_count, hipStream_t st);
// Returns true if the full rows' fc0 rows (facc) are complete behind its launches: the difference path with k_sib_children2, where the full-row fc0 runs in front of the
// children and the children launch reduces its partials.  Else launch_fc0_delta runs both.
static bool launch_trunk_siblings(Net& net, const Store& S, int side, int max_count, hipStream_t st, bool delta, Prof* prof) {
    constexpr int LDS = TR_WBYTES + 4 * SIB_CGRID_BYTES + TR_SIDE_FLOATS * 4;
    static_assert(LDS + 32 <= 160 * 1024, "k_sib_children LDS (+ the static pair-barrier flags)");
    static bool attr_done[64] = {};
    if (!attr_done[net.device & 63]) {
        for (int d = 0; d < 2; ++d)
            for (int x = 0; x < 2; ++x)
                for (int n : {9, 15}) hipFuncSetAttribute((const void*)sib_kernel(d != 0, x != 0, n), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
        for (int x = 0; x < 3; ++x)
            for (int n : {9, 15}) hipFuncSetAttribute((const void*)sib2_kernel(x != 0, n, x == 2), hipFuncAttributeMaxDynamicSharedMemorySize, V2_LDS);
        attr_done[net.device & 63] = true;
    }
    const bool x16 = net.fc0_fmt == FC0_F16;
    if (!net.gcnt_zeroed) k_zero_ints<<<1, 128, 0, st>>>(net.d_gcnt, SIB_CNT_INTS); // (a hipMemsetAsync of these 448 bytes is a 13-us fill kernel)
    const int do_fill = net.fill_in_group ? 1 : 0;
    const int32_t* scan_cnt = net.scan_cnt; // (non-NULL: no k_scan ran, k_group derives the request offsets)
    net.gcnt_zeroed = net.fill_in_group = false; // (one round's worth: the engine sets them per round)
    net.scan_cnt = nullptr;
    if (delta && (!net.sib_cache_valid || !net.base_cache)) { // the trees changed since the last search round: no cached base is valid
        hipMemsetAsync(net.d_tags, 0xFF, sizeof(int32_t) * (size_t)net.games * SIB_WAYS, st);
        net.sib_cache_valid = true;
    }
    if (net.grp_hi >= 0) { // match episode: this net's games only
        const int ng = net.grp_hi - net.grp_lo;
        k_group<true><<<ng > 0 ? (ng + GROUP_TREES - 1) / GROUP_TREES : 1, 64 * GROUP_TREES, 0, st>>>(S, side, (uint2*)net.d_groups, net.d_singles, (uint4*)net.d_sib_rows,
                                                                    net.d_gcnt, delta ? net.d_sib_slot : nullptr, net.d_tags, (uint2*)net.d_comp, net.n, do_fill,
                                                                    net.d_work, net.grp_lo, net.grp_hi, net.grp_sub, nullptr, nullptr);
    } else
        k_group<false><<<(S.games + GROUP_TREES - 1) / GROUP_TREES, 64 * GROUP_TREES, 0, st>>>(S, side, (uint2*)net.d_groups, net.d_singles, (uint4*)net.d_sib_rows, net.d_gcnt,
                                                                                     delta ? net.d_sib_slot : nullptr, net.d_tags, (uint2*)net.d_comp, net.n, do_fill, net.d_work,
                                                                                     0, 0, nullptr, scan_cnt, net.scan_evals);
    if (!delta) {
        // (the copy path keeps the runs' h grids in sib_h[run index]: the slots the difference path caches bases in -- cached bases are void)
        net.sib_cache_valid = false;
        // base positions of the runs, then the rows outside runs
        if (net.n == 9) launch_trunk_fmt<9, false, true>(net, S, max_count, st, net.d_singles, net.d_gcnt + NET_GCNT_RUNS, nullptr, net.d_gcnt + NET_GCNT_SINGLES);
        else launch_trunk_fmt<15, false, true>(net, S, max_count, st, net.d_singles, net.d_gcnt + NET_GCNT_RUNS, nullptr, net.d_gcnt + NET_GCNT_SINGLES);
        net.children_launches[1] += 1.0;
        sib_kernel(false, x16, net.n)<<<256, 512, LDS, st>>>(S.board, (const uint4*)net.wt_trunk, net.wt_first, (uint4*)net.a_fc0, net.row_u4,
                                                             (const uint4*)net.d_sib_rows, net.d_gcnt, net.sib_h, nullptr, nullptr, nullptr, nullptr, nullptr);
        return false;
    }
    static const int tprof_mode = getenv("OMOK_SIB_PROF") ? atoi(getenv("OMOK_SIB_PROF")) : 0; // timing experiments only (N = 15, fp6 format): 2 = k_sib_children2's phase profile
    const bool mixed = x16 && net.diff_fp6; // FC0_MIXED: full rows f16, difference rows fp6 (k_sib_children2 only)
    const bool v2 = net.sib_v2 || mixed;
    // per-tile rectangles of window pixels (bin_prefix_role): only k_sib_children2 writes the exact zeros outside a child's own region that make a row's sum independent of its tile
    const bool rects = v2 && net.win_rects;
    // the round's slot layout (bin_prefix_role) is derived by workgroup 0 of the base pass's launch
    const BinPrefixArgs role{net.d_gcnt, net.d_bin_start, net.d_tile_info, (uint2*)net.d_slot_desc, net.d_singles, net.d_work, net.n_cu,
                             SIB_MAX_FWAYS, SIB_MAX_WWAYS, (int)std::min<size_t>(net.part_w_rows * 7, (size_t)1 << 30), (int)net.base_slots,
                             (int)std::min<size_t>(net.part_rows, (size_t)1 << 30), 2 * net.hw, net.n, rects ? 1 : 0, (int)(net.d_slots / GT_BS)};
    // runs without a cached base -> compact rows [0, misses) + their base slots; then the single rows -> compact rows [misses, misses + singles)
    if (net.n == 9) launch_trunk_fmt<9, false, true, true>(net, S, max_count, st, net.d_singles, net.d_gcnt + NET_GCNT_FULL_EVALS, nullptr, net.d_gcnt + NET_GCNT_SINGLES, v2, &role);
    else launch_trunk_fmt<15, false, true, true>(net, S, max_count, st, net.d_singles, net.d_gcnt + NET_GCNT_FULL_EVALS, nullptr, net.d_gcnt + NET_GCNT_SINGLES, v2, &role);
    static const bool stats = getenv("OMOK_SIB_STATS") && atoi(getenv("OMOK_SIB_STATS")); // diagnostics only: synchronises every round
    if (stats) {
        // per round: runs, runs evaluated in full (base-cache misses + uncacheable runs), singles, rows in runs, window tiles, first tile of the split set, its ways, full-row K split
        static const int shown[8] = {NET_GCNT_RUNS, NET_GCNT_FULL_EVALS, NET_GCNT_SINGLES, NET_GCNT_ROWS_IN_RUNS, NET_GCNT_WIN_TILES, NET_GCNT_SPLIT_TILE0, NET_GCNT_WIN_WAYS, NET_GCNT_FULL_WAYS};
        static long long acc[8] = {}, launches = 0;
        int32_t c[NET_GCNT_HEAD_INTS];
        hipStreamSynchronize(st);
        hipMemcpy(c, net.d_gcnt, sizeof(c), hipMemcpyDeviceToHost);
        for (int i = 0; i < 8; ++i) acc[i] += c[shown[i]];
        if ((launches + 1) % 50 == 0) { // this round's window tiles: the work their rectangles leave
            const int nt = c[NET_GCNT_WIN_TILES], whole = c[NET_GCNT_SPLIT_TILE0];
            std::vector<int32_t> ti((size_t)(nt > 0 ? nt : 1));
            hipMemcpy(ti.data(), net.d_tile_info, sizeof(int32_t) * ti.size(), hipMemcpyDeviceToHost);
            long long tot = 0;
            for (int t = 0; t < whole && t < nt; ++t) {
                int y0, y1, x0, x1;
                tile_rect(ti[t], y0, y1, x0, x1);
                tot += (y1 - y0 + 1) * (x1 - x0 + 1);
            }
            fprintf(stderr, "[sib stats] whole-K window tiles: %d, rectangle pixels %lld = %.3f of full 7x7 windows\n", whole, tot, (double)tot / (49.0 * (whole > 0 ? whole : 1)));
        }
        if (++launches % 50 == 0) {
            fprintf(stderr, "[sib stats] rounds %lld: per round runs %.0f (evaluated in full %.0f) singles %.0f rows-in-runs %.0f (run length %.2f) window tiles %.1f (split set from %.1f, %.1f ways) full-row K split %.1f\n",
                    launches, acc[0] / 50.0, acc[1] / 50.0, acc[2] / 50.0, acc[3] / 50.0, acc[0] ? (double)acc[3] / acc[0] : 0.0, acc[4] / 50.0, acc[5] / 50.0, acc[6] / 50.0, acc[7] / 50.0);
            for (int i = 0; i < 8; ++i) acc[i] = 0;
        }
    }
    if (v2 && tprof_mode == 2 && !x16 && net.n == 15) {
        static unsigned long long* d_tp = nullptr;
        static unsigned long long acc[32] = {};
        static int launches = 0;
        constexpr size_t TP_BYTES = 256 + (size_t)TP_LAUNCHES * 256 * 4 * 8;
        if (!d_tp) { hipMalloc(&d_tp, TP_BYTES); hipMemset(d_tp, 0, TP_BYTES); hipFuncSetAttribute((const void*)k_sib_children2<false, 15, true>, hipFuncAttributeMaxDynamicSharedMemorySize, V2_LDS); }
        k_sib_children2<false, 15, true><<<256, 512, V2_LDS, st>>>(S.board, (const uint4*)net.wt_trunk, net.wt_first, (uint4*)net.a_base, net.row_u4, (const uint4*)net.d_sib_rows,
                                                                   net.d_gcnt, (const uint4*)net.sib_h, net.d_sib_slot, net.d_bin_start, (uint4*)net.d_rows, (uint2*)net.d_slot_desc,
                                                                   d_tp, (const uint4*)net.conv_tab, FaccReduceArgs{});
        if (++launches % 100 == 0) {
            hipStreamSynchronize(st);
            hipMemcpy(acc, d_tp, 256, hipMemcpyDeviceToHost);
            static const char* names[12] = {"inputs+conv table", "P0's table row + L0 x2", "grid+strip dw+read d (blocks 0,1)", "L1L2 (blocks 0,1)", "block 2: grid + ring + tile dw", "L1L2 tile",
                                            "base subtract tile", "stores tile", "x2 + base fetch ring", "L1L2 ring", "base subtract ring", "stores ring"};
            for (int w = 0; w < 2; ++w) {
                double tot = 0;
                for (int i = 0; i < 12; ++i) tot += (double)acc[16 * w + i];
                fprintf(stderr, "[sib2 prof] wave %d, %d launches x 256 workgroups: ", w ? 5 : 0, launches);
                for (int i = 0; i < 12; ++i) fprintf(stderr, "%s %.1f%%  ", names[i], 100.0 * (double)acc[16 * w + i] / tot);
                fprintf(stderr, " | %.0f cycles per workgroup and launch\n", tot / 256.0 / launches);
            }
        }
        if (launches % TP_LAUNCHES == 0) { // the last 128 launches' stamps: the prologue per workgroup, and how far the launch's last workgroup ends behind the median one
            static std::vector<unsigned long long> rec((size_t)TP_LAUNCHES * 256 * 4);
            hipStreamSynchronize(st);
            hipMemcpy(rec.data(), d_tp + TP_STAMPS, rec.size() * 8, hipMemcpyDeviceToHost);
            double pro_med = 0, pro_max = 0, cyc_med = 0, cyc_max = 0, dur = 0, tail = 0, tail_max = 0;
            for (int l = 0; l < TP_LAUNCHES; ++l) {
                std::vector<double> pro, cyc, end;
                unsigned long long t0 = ~0ULL;
                for (int w = 0; w < 256; ++w) {
                    const unsigned long long* r = &rec[((size_t)l * 256 + w) * 4];
                    t0 = std::min(t0, r[0]);
                    pro.push_back((double)(r[1] - r[0]) * 0.01); // us (100 MHz)
                    cyc.push_back((double)r[3]);
                    end.push_back((double)r[2]);
                }
                std::sort(pro.begin(), pro.end()); std::sort(cyc.begin(), cyc.end()); std::sort(end.begin(), end.end());
                const double d = (end[255] - (double)t0) * 0.01, tl = (end[255] - end[128]) * 0.01;
                pro_med += pro[128]; pro_max += pro[255]; cyc_med += cyc[128]; cyc_max += cyc[255]; dur += d; tail += tl / d; tail_max = std::max(tail_max, tl / d);
            }
            const double n = TP_LAUNCHES;
            fprintf(stderr, "[sib2 stamps] launches %d..%d: prologue (entry to behind the barrier) per workgroup, mean over launches of the median %.2f us = %.0f shader cycles, of the "
                            "slowest %.2f us = %.0f cycles; launch (first entry to last end) %.1f us; (last - median workgroup end) / launch: mean %.2f %%, largest %.2f %%\n",
                    launches - TP_LAUNCHES, launches - 1, pro_med / n, cyc_med / n, pro_max / n, cyc_max / n, dur / n, 100.0 * tail / n, 100.0 * tail_max);
        }
        return false;
    }
    net.children_launches[v2 ? 0 : 1] += 1.0;
    if (v2) {
        // the full rows' fc0 needs the base pass only; in front of the children, these reduce its partials and k_facc_reduce's launch is gone from the chain (PC_FC0's time;
        // the category's launch is counted where forward_f16x3 begins it)
        if (prof) { prof->end(st); prof->begin(PC_FC0, st, false); }
        launch_fc0_full_rows(net, max_count, st);
        if (prof) { prof->end(st); prof->begin(PC_TRUNK, st, false); }
        sib2_kernel(x16, net.n, mixed)<<<256, 512, V2_LDS, st>>>(S.board, (const uint4*)net.wt_trunk, net.wt_first, (uint4*)net.a_base, net.row_u4, (const uint4*)net.d_sib_rows,
                                                          net.d_gcnt, (const uint4*)net.sib_h, net.d_sib_slot, net.d_bin_start, (uint4*)net.d_rows, (uint2*)net.d_slot_desc, nullptr,
                                                          (const uint4*)net.conv_tab, FaccReduceArgs{net.part, net.facc, (const uint2*)net.d_comp, (int)net.base_slots});
        return true;
    }
    sib_kernel(true, x16, net.n)<<<256, 512, LDS, st>>>(S.board, (const uint4*)net.wt_trunk, net.wt_first, (uint4*)net.a_base, net.row_u4,
                                                        (const uint4*)net.d_sib_rows, net.d_gcnt, net.sib_h, net.d_sib_slot, net.d_bin_start,
                                                        (uint4*)net.d_rows, (uint2*)net.d_slot_desc, nullptr);
    return false;
}

// One fc0 launch: kernel <EPI, WIN> on operands of format `fmt` -- FC0_FP6: k_fc0_mx on net.wt_fc0 with its block scales, FC0_F16: k_fc0_x3 on net.wt_fc0x.  `grid` workgroups;
// the other arguments are the kernels' own, the same for both.
static MxScales fc0_scales(const Net& net) { return MxScales{127 - net.mx_sw, 127 - (net.mx_sw + 11), 127 - MX_SA, 127 - (MX_SA + 11), ldexpf(1.0f, net.mx_sw), ldexpf(1.0f, MX_SA)}; }
template <int EPI, bool WIN>
static void launch_fc0(const Net& net, int fmt, int grid, hipStream_t st, const void* act, int ksup, size_t act_row_u4, const float* bias, uint4* out_split, size_t out_row_u4,
                       float* out_part, const int32_t* d_count, int max_count, const int32_t* tile_info = nullptr, const void* slot_desc = nullptr, const float* facc = nullptr) {
    const int full_tiles = net.hw / 32, last_cnt = (net.hw % 32) ? (net.hw % 32) : 1;
    if (fmt == FC0_F16)
        k_fc0_x3<EPI, WIN><<<dim3(grid, 1), 256, 0, st>>>((const uint4*)net.wt_fc0x, (const uint4*)act, ksup, act_row_u4, full_tiles, last_cnt, bias, out_split, out_row_u4, out_part,
                                                          d_count, max_count, tile_info, (const uint2*)slot_desc, facc, net.n);
    else
        k_fc0_mx<EPI, WIN><<<dim3(grid, 1), 256, 0, st>>>((const uint4*)net.wt_fc0, (const uint4*)act, ksup, act_row_u4, full_tiles, last_cnt, fc0_scales(net), bias, out_split,
                                                          out_row_u4, out_part, d_count, max_count, tile_info, (const uint2*)slot_desc, facc, net.n);
}
// fc0 of the difference path's full rows (the runs' bases evaluated this round and the single rows: ~16x fewer than requests) into fp32 split-K partials, in the format of
// full operand rows.  Their live count is only known on the device: bin_prefix_role chose the K split and the partial slab's row stride (NET_GCNT_FULL_WAYS,
// NET_GCNT_FULL_STRIDE).  It reads a_fc0, which the base pass wrote: launch_trunk_siblings puts it in front of k_sib_children2, which then reduces the partials.
static void launch_fc0_full_rows(Net& net, int max_count, hipStream_t st) {
    const int n_cu = net.n_cu, tiles_max = (max_count + GT_BS - 1) / GT_BS;
    const int32_t* cnt = net.d_gcnt;
    const int fgrid = ((tiles_max > n_cu ? tiles_max : n_cu) + 7) / 8 * 8; // (tiles x ways <= CUs by construction unless there are more tiles than CUs: then 1 way; whole eighths: xcd_item)
    launch_fc0<EPI_PARTIAL, false>(net, net.fc0_fmt, fgrid, st, net.a_fc0, net.hw * 2, net.row_u4, net.wt_first + TR_SIDE_FLOATS, nullptr, (size_t)tiles_max * GT_BS, net.part,
                                   cnt + NET_GCNT_FULL_ROWS, max_count, cnt + NET_GCNT_FULL_WAYS);
}

// fc0 of a sibling round on the difference path: fp32 fc0 rows of the full rows (launch_fc0_full_rows + the reduce; facc_done: launch_trunk_siblings ran both, the reduce
// as a role of k_sib_children2), then one window tile per 128 slots: 98 of the 450 super-steps, + the slot's full row, bias, LeakyReLU, hi|lo.
static void launch_fc0_delta(Net& net, int max_count, const float* bias_fc0, uint4* h0, hipStream_t st, bool facc_done) {
    const int n_cu = net.n_cu;
    const int tiles_max = (max_count + GT_BS - 1) / GT_BS;
    const int32_t* cnt = net.d_gcnt;
    if (!facc_done) {
        launch_fc0_full_rows(net, max_count, st);
        k_facc_reduce<<<512, 256, 0, st>>>(net.part, cnt + NET_GCNT_FULL_ROWS, cnt + NET_GCNT_FULL_WAYS, net.facc, (const uint2*)net.d_comp, cnt + NET_GCNT_FULL_EVALS, (int)net.base_slots);
    }
    // window tiles, in the format of the difference rows (FC0_MIXED: fp6 behind f16 full rows): whole rounds of workgroups at full K, the tiles of the last partial round
    // split over K (bin_prefix_role)
    const int dfmt = (net.fc0_fmt != FC0_F16 || net.diff_fp6) ? FC0_FP6 : FC0_F16;
    const size_t drow_u4 = dfmt == FC0_F16 ? SIBX_DROW_U4 : SIB_DROW_U4;
    const int wtiles_max = (tiles_max + SIB_BINS + 1 + 7) / 8 * 8 + 8; // (the XCD-aware tile mapping rounds an eighth of the tiles up)
    launch_fc0<EPI_SPLIT, true>(net, dfmt, (wtiles_max + 255) / 256 * 256, st, net.d_rows, 0, drow_u4, bias_fc0, h0, 128, nullptr, cnt, max_count, net.d_tile_info, net.d_slot_desc,
                                net.facc);
    const int stiles = wtiles_max < n_cu + 8 ? wtiles_max : n_cu + 8;
    launch_fc0<EPI_PARTIAL, true>(net, dfmt, n_cu + 8, st, net.d_rows, 0, drow_u4, bias_fc0, nullptr, net.part_w_rows, net.part_w, cnt, max_count, net.d_tile_info, net.d_slot_desc);
    k_win_finish<<<(unsigned)(((size_t)stiles * GT_BS * 64 + 255) / 256), 256, 0, st>>>(net.part_w, net.part_w_rows, cnt, net.d_tile_info, (const uint2*)net.d_slot_desc, net.facc,
                                                                                         bias_fc0, h0, 128);
}

static int sib_env() { // OMOK_TRUNK_SIB: 0: every row through k_trunk, 1: copy path, 2: difference path
    static const int use_sib = getenv("OMOK_TRUNK_SIB") ? atoi(getenv("OMOK_TRUNK_SIB")) : 2;
    return use_sib;
}
// THE decision whether a forward of request rows groups them by parent (launch_trunk_siblings): forward_f16x3 takes it from here, and so does the engine's
// prediction of it (net_round_takes_sibling_path), on which it hands the request-list fill and the zeroing of d_gcnt to that path
// Rounds below this many request rows take the copy path (forward_f16x3).  N = 15: 3072 in the fp6 format (measured break-even between 2048 and 4096 rows); with f16 full
// rows the copy path's dense fc0 costs 1.5x more while the difference path's window tiles stay fp6 (FC0_MIXED): break-even between 1024 and 2048 rows (per three plies at
// 2048 / 2560 rows: copy 65.4 / 74.7 ms, difference 60.2 / 63.4 ms; at 1024 rows 51.4 against 56.0)
static int sib_delta_min_rows(const Net& net) {
    static const int delta_min_env = getenv("OMOK_SIB_DELTA_MIN") ? atoi(getenv("OMOK_SIB_DELTA_MIN")) : 0;
    if (delta_min_env > 0) return delta_min_env;
    if (net.n != 15) return 1024;
    return net.diff_fp6 ? 2048 : 3072;
}
static bool sibling_path(const Net& net, bool from_f32, int sib_side) { return !from_f32 && sib_side >= 0 && sib_env() && net.siblings && net.d_groups; }
bool net_round_takes_sibling_path(const Net& net, int max_count) {
    if (net.mode == OMOK_NET_F32 || max_count <= 0) return false;
    return sibling_path(net, false, 0);
}
// The engine skipped k_fill / the zeroing of d_gcnt for this round (Net::fill_in_group, Net::gcnt_zeroed) because it expected the sibling path: a forward that
// does not take it would read a request list nobody wrote.  That is a disagreement between engine.cpp's prediction (net_round_takes_sibling_path) and this file's
// decision -- a programming error -- but never a reason to take the host process down from inside a library: the forward writes the list itself and says so once.
static void recover_handed_over_fill(Net& net, const Store& S, hipStream_t st, const char* where) {
    if (!net.fill_in_group) return;
    static bool said = false;
    if (!said) {
        said = true;
        fprintf(stderr, "omok_mi355x: internal inconsistency (recovered): the round's request-list fill was handed to the sibling path, but the forward (%s) does not take it; "
                        "the list is written here instead\n", where);
    }
    if (net.scan_cnt) launch_scan(net.n, S, net.fill_side, net.fill_k, st, net.scan_evals, nullptr, 0, true); // (no k_scan ran either: request offsets, then the list)
    else launch_fill(S, net.fill_side, net.fill_k, st);
    net.fill_in_group = net.gcnt_zeroed = false;
    net.scan_cnt = nullptr;
}
// K split of the dense fc0 (plain rows, copy path).  Small batches (late plies of an episode) cannot fill the CUs with 128-sample tiles: K is split into fp32 partials
// that a second kernel finishes, so that the workgroups fill whole waves of CUs (one workgroup per CU at a time: 144 KiB of LDS): with T tiles of 128 samples and
// d-way split-K the launch takes ceil(T*d / CUs) / d units of time.  T = 300 (59 % of the games alive at 4096 x K = 16) costs 2 units unsplit and 1.2 with d = 5; late
// plies (T << CUs) get their parallelism from d alone.  The fp32 partials of d splits must fit the slab.
static int fc0_dense_nsplit(int rows, int nsup, int n_cu, size_t part_rows) {
    const int tiles128 = (rows + GT_BS - 1) / GT_BS;
    int nsplit = 1;
    double best = 1e30;
    // Up to 64 ways (round 4; 16 before): a thin round's few tiles then spread over all CUs -- per three plies at 16 / 32 / 64 live games: fp6 42.7 / 44.0 / 45.6 ->
    // 38.0 / 39.3 / 42.3 ms, mixed (f16 rows) 48.0 / 49.1 / 51.5 -> 40.1 / 41.7 / 47.8 ms.  (Round 2 had measured 30 ways slower than 15 at 8 tiles; with the items
    // dealt per XCD -- xcd_item -- it is the other way round.)
    constexpr int dmax = 64;
    for (int d = 1; d <= dmax; ++d) { // (uneven splits: ceil(nsup / d) super-steps per split, the last one shorter but never empty)
        const int per = (nsup + d - 1) / d;
        if ((d - 1) * per >= nsup) continue;
        if (d > 1 && (size_t)d * (size_t)(tiles128 * GT_BS) > part_rows) continue;
        const double waves = (double)(((size_t)tiles128 * d + n_cu - 1) / n_cu);
        const double cost = waves * (per + 4) * (d > 1 ? 1.04 : 1.0); // (+ pipeline fill and epilogue of a workgroup; partials round trip)
        if (cost < best - 1e-9) { best = cost; nsplit = d; }
    }
    return nsplit;
}
// K split of fc1 and the heads: 32 k-steps in a row per 128-sample tile; a batch of few tiles (thin rounds) leaves most CUs idle behind a chain of 32 dependent
// stages, so K is split over blockIdx.y (a power of two of the 32 k-steps, >= 4 k-steps each) into the fp32 partial slab and finished as fc0 is
static int tail_tsplit(int rows, int n_cu, size_t part_rows) {
    const int tiles_t = (rows + GT_BS - 1) / GT_BS;
    int tsplit = 1;
    while (tsplit < 8 && tiles_t * tsplit * 2 <= n_cu && (size_t)(tsplit * 2) * (size_t)(tiles_t * GT_BS) <= part_rows) tsplit *= 2;
    return tsplit;
}
static void forward_f16x3(Net& net, const Store& S, int max_count, bool from_f32, hipStream_t st, Prof* prof, int sib_side = -1, bool skip_softmax = false,
                          bool rows_to_nodes = false) {
    const int hw = net.hw;
    const int use_sib = sib_env();
    const bool sib = sibling_path(net, from_f32, sib_side);
    if (!sib) recover_handed_over_fill(net, S, st, "forward_f16x3 on plain rows");
    // Small rounds (the thin tail of an episode) take the copy path: the difference path needs one fc0 tile per non-empty window bin
    // (81 + 1) however few rows there are, the copy path rows / 128 tiles of the full K -- measured break-even between 2048 and 4096 rows.  The choice is a
    // function of the host's bound on the request count (alive games x K) only, so a run is reproducible.
    // (N = 9: 9 window bins + the single rows = 10 tiles at least)
    const bool delta = sib && use_sib >= 2 && max_count >= sib_delta_min_rows(net);
    if (prof) prof->begin(PC_TRUNK, st);
    bool facc_done = false;
    if (sib) facc_done = launch_trunk_siblings(net, S, sib_side, max_count, st, delta, prof);
    else if (net.n == 9) { if (from_f32) launch_trunk_fmt<9, true>(net, S, max_count, st); else launch_trunk_fmt<9, false>(net, S, max_count, st); }
    else {
        if (from_f32) launch_trunk_fmt<15, true>(net, S, max_count, st);
        else launch_trunk_fmt<15, false>(net, S, max_count, st);
    }
    if (prof) { prof->end(st); prof->begin(PC_FC0, st); }
    const float* bias_fc0 = net.wt_first + TR_SIDE_FLOATS;
    const float* bias_fc1 = bias_fc0 + NF;
    const float* bias_heads = bias_fc1 + NF;
    uint4* h0 = (uint4*)net.h0;
    const size_t mb = ((size_t)net.max_b + GT_BS - 1) / GT_BS * GT_BS;
    uint4* h1 = h0 + mb * 128; // 32 k-steps * 4 uint4 per row
    net.plan_path = sib ? (delta ? 2 : 1) : 0;
    net.plan_rows = max_count;
    net.plan_nsplit = 0;
    if (delta) launch_fc0_delta(net, max_count, bias_fc0, h0, st, facc_done);
    else { // dense fc0: whole K, or split K into fp32 partials + finish (sum in split order + bias + LeakyReLU + hi|lo)
        const int nsup = hw * 2, tiles128 = (max_count + GT_BS - 1) / GT_BS;
        const int nsplit = net.plan_nsplit = fc0_dense_nsplit(max_count, nsup, net.n_cu, net.part_rows);
        if (nsplit == 1) launch_fc0<EPI_SPLIT, false>(net, net.fc0_fmt, tiles128, st, net.a_fc0, nsup, net.row_u4, bias_fc0, h0, 128, nullptr, S.d_count, max_count);
        else {
            const size_t cap_rows = (size_t)tiles128 * GT_BS;
            launch_fc0<EPI_PARTIAL, false>(net, net.fc0_fmt, (tiles128 * nsplit + 7) / 8 * 8, st, net.a_fc0, (nsup + nsplit - 1) / nsplit, net.row_u4, bias_fc0, nullptr, cap_rows,
                                           net.part, S.d_count, max_count);
            k_splitk_finish<<<(unsigned)(((size_t)max_count * 64 + 255) / 256), 256, 0, st>>>(net.part, nsplit, cap_rows, bias_fc0, h0, 128, S.d_count, max_count);
        }
    }
    if (prof) { prof->end(st); prof->begin(PC_TAIL, st); }
    // fc1 and heads: whole K, or K split over blockIdx.y (tail_tsplit)
    const int MT = heads_mt(hw);
    // rows_to_nodes (with skip_softmax): the logits rows go into the requests' policy rows, v and vpre are written here (LogitsDst); the rows are as long as a policy row
    LogitsDst D{};
    if (rows_to_nodes && skip_softmax && MT * 32 == net.rowp) D = LogitsDst{S.req_ref, S.policy, net.v, net.vpre, S.stride_nodes, hw};
    const int tiles_t = (max_count + GT_BS - 1) / GT_BS;
    const int tsplit = net.plan_tsplit = tail_tsplit(max_count, net.n_cu, net.part_rows);
    const size_t cap_t = (size_t)tiles_t * GT_BS;
    const size_t fin_threads = (size_t)max_count * 64;
    if (tsplit == 1) {
        // whole-K rounds: k_tail_fused (fc1 and the heads in one launch, h1 is not written); OMOK_GEMM_W=1 selects the two k_gemm_w launches (wave-private weight rings,
        // one barrier per two k-steps; same bits, measured no faster: see the kernel) for A-B runs and the tests that compare the outputs bit for bit; the N = 9 heads
        // (4 m-tiles: less than one per wave) then stay on k_gemm_t
        const char* gw_env = getenv("OMOK_GEMM_W");
        const bool gw = gw_env && gw_env[0] == '1';
        if (!gw) {
            if (MT == 8) launch_tail_fused<8>(net.wt_fc1, h0, bias_fc1, net.wt_heads, bias_heads, net.s0, S, max_count, st, net.device, D);
            else launch_tail_fused<4>(net.wt_fc1, h0, bias_fc1, net.wt_heads, bias_heads, net.s0, S, max_count, st, net.device, D);
        } else {
            launch_gemm_w<16, EPI_SPLIT>(net.wt_fc1, h0, 32, 128, bias_fc1, h1, 128, nullptr, S, max_count, st, net.device);
            if (MT == 8) launch_gemm_w<8, EPI_LOGITS>(net.wt_heads, h1, 32, 128, bias_heads, nullptr, 0, net.s0, S, max_count, st, net.device, D);
            else launch_gemm<4, EPI_LOGITS, 2>(net.wt_heads, h1, 32, 128, 32, 1, 2, bias_heads, nullptr, 0, net.s0, S, max_count, st, net.device, 1, D);
        }
    } else {
        launch_gemm<16, EPI_PARTIAL, 1>(net.wt_fc1, h0, 32 / tsplit, 128, 32, 1, 2, bias_fc1, nullptr, cap_t, net.part, S, max_count, st, net.device, tsplit);
        k_splitk_finish<<<(unsigned)((fin_threads + 255) / 256), 256, 0, st>>>(net.part, tsplit, cap_t, bias_fc1, h1, 128, S.d_count, max_count);
        if (MT == 8) launch_gemm<8, EPI_PARTIAL, 2>(net.wt_heads, h1, 32 / tsplit, 128, 32, 1, 2, bias_heads, nullptr, cap_t, net.part, S, max_count, st, net.device, tsplit);
        else launch_gemm<4, EPI_PARTIAL, 2>(net.wt_heads, h1, 32 / tsplit, 128, 32, 1, 2, bias_heads, nullptr, cap_t, net.part, S, max_count, st, net.device, tsplit);
        const unsigned lg = (unsigned)(((size_t)max_count * (MT * 8) + 255) / 256);
        k_splitk_logits<<<lg < 2048 ? lg : 2048, 256, 0, st>>>(net.part, tsplit, cap_t, MT * 32, bias_heads, net.s0, S.d_count, max_count, D);
    }
    const int sg = max_count < 32768 ? max_count : 32768; // one wave per row up to 32 waves per SIMD: the row loop is a chain of dependent loads
    if (!skip_softmax) k_softmax<<<sg, 64, 0, st>>>(net.s0, MT * 32, hw, net.rowp, net.p, net.v, net.vpre, S.d_count, max_count);
    if (prof) prof->end(st);
}

// ===============================================================================================
// commit-time probe: which operand format fc0 may use (Net::fc0_policy = FC0_AUTO)
// ===============================================================================================
// NET_PROBE_ROWS deterministic positions in the encoder.rs layout (Player mode): two fifths nearly empty boards (the positions search rounds
// of the first plies see: the largest errors were measured there), two fifths up to ~60 % full, a fifth of any density; both sides to move; stones by a hash of (row, cell).
__device__ inline uint32_t probe_mix(uint32_t x) { x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16; return x; }
__global__ void k_probe_inputs(float* __restrict__ in, int hw, int rows, int row0) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * hw) return;
    const int r = i / hw, a = i % hw, gr = row0 + r;
    const uint32_t hr = probe_mix(0x9E3779B9u * (uint32_t)(gr + 1));
    const uint32_t kind = (uint32_t)gr % 5u;                                      // occupied share of the board in 1 / 1024:
    const uint32_t dens = kind < 2 ? (hr >> 8) % 40u : kind < 4 ? (hr >> 8) % 600u : (hr >> 8) % 1024u; // 40 % of the rows < 4 %, 40 % < 59 %, 20 % any
    const uint32_t hc = probe_mix(hr ^ (0x85EBCA6Bu * (uint32_t)(a + 1)));
    const bool occ = (hc & 1023u) < dens, black = (hc >> 10) & 1u;
    const int turn = (int)(hr & 1u);                                             // 0 = Black to move
    const bool mine = black == (turn == 0);
    float* o = in + (size_t)r * 3 * hw;
    o[2 * a] = occ && mine ? 1.0f : 0.0f;
    o[2 * a + 1] = occ && !mine ? 1.0f : 0.0f;
    o[2 * hw + a] = turn == 0 ? 1.0f : 0.0f;
}

// The probe's SIBLING ROUNDS (round 4): what a search round evaluates is not a batch of plain rows but runs of siblings -- one base position per run, a
// 7x7-window difference row per child -- so the probe also plays one synthetic round through that very path: a Store of `S.games` one-level
// trees, tree t = a parent position (node 0; drawn like the probe's plain rows, at most ~half full) + pk children (one more stone of the side to move, on
// distinct empty cells) that are the round's requests, in the layout k_group / k_trunk<BASE> / k_sib_children2 read (hdr, board, ts, req_node, gs, req_ref).
__global__ __launch_bounds__(64) void k_probe_store(Store S, int n, int pk) {
    const int t = blockIdx.x, lane = threadIdx.x, hw = n * n, nw = (hw + 63) / 64;
    const uint32_t hr = probe_mix(0x9E3779B9u * (uint32_t)(t + 7919));
    const uint32_t kind = (uint32_t)t % 5u;
    const uint32_t dens = kind < 2 ? (hr >> 8) % 40u : (hr >> 8) % 500u; // two fifths nearly empty boards, the rest up to ~49 % full
    const int turn = (int)(hr & 1u);
    uint64_t bw[4] = {0, 0, 0, 0}, ww[4] = {0, 0, 0, 0};
    int stones = 0;
    for (int j = 0; j < nw; ++j) {
        const int a = j * 64 + lane;
        const uint32_t hc = probe_mix(hr ^ (0x85EBCA6Bu * (uint32_t)(a + 1)));
        const bool occ = a < hw && (hc & 1023u) < dens, black = (hc >> 10) & 1u;
        bw[j] = __ballot(occ && black);
        ww[j] = __ballot(occ && !black);
        stones += __popcll(bw[j] | ww[j]);
    }
    if (hw - stones <= pk) { // (never fewer empty cells than children: the request list would hold rows nobody wrote; wave-uniform)
        for (int j = 0; j < 4; ++j) bw[j] = ww[j] = 0ULL;
        stones = 0;
    }
    const size_t tn = (size_t)t * (size_t)S.stride_nodes;
    const int legal = hw - stones;
    // the children's cells: the first pk empty ones along c_k = (start + 7 k) mod hw (7 is coprime with 81 and 225)
    const int start = (int)((hr >> 3) % (uint32_t)hw);
    int found = 0;
    for (int k0 = 0; k0 < hw && found < pk; k0 += 64) {
        const int k = k0 + lane, c = (start + 7 * k) % hw;
        const bool empty = k < hw && !(((bw[c >> 6] | ww[c >> 6]) >> (c & 63)) & 1ULL);
        const unsigned long long m = __ballot(empty);
        const int idx = found + __popcll(m & ((1ULL << lane) - 1ULL));
        if (empty && idx < pk) {
            NodeHdr h;
            h.parent = 0; h.table = NONE16; h.legal = (uint16_t)(legal - 1); h.nch = 0; h.action = (uint8_t)c; h.status = ST_IN_PROGRESS;
            h.turn = (uint8_t)(1 - turn); h.has_policy = 0; h.pad = 0;
            S.hdr[tn + 1 + idx] = h;
            for (int j = 0; j < nw; ++j) {
                const uint64_t bit = (c >> 6) == j ? (1ULL << (c & 63)) : 0ULL;
                S.board[(tn + 1 + idx) * (size_t)(2 * nw) + j] = bw[j] | (turn == 0 ? bit : 0ULL);
                S.board[(tn + 1 + idx) * (size_t)(2 * nw) + nw + j] = ww[j] | (turn == 0 ? 0ULL : bit);
            }
            S.req_node[(size_t)t * KMAX + idx] = (uint16_t)(1 + idx);
            S.req_ref[(size_t)t * pk + idx] = ((uint32_t)t << 16) | (uint32_t)(1 + idx);
            S.req_aux[(size_t)t * pk + idx] = 0xFFFFFFFFu;
        }
        found += __popcll(m);
    }
    if (lane == 0) {
        NodeHdr h;
        h.parent = NONE16; h.table = NONE16; h.legal = (uint16_t)legal; h.nch = (uint16_t)pk; h.action = 0; h.status = ST_IN_PROGRESS;
        h.turn = (uint8_t)turn; h.has_policy = 0; h.pad = 0;
        S.hdr[tn] = h;
        for (int j = 0; j < nw; ++j) { S.board[tn * (size_t)(2 * nw) + j] = bw[j]; S.board[tn * (size_t)(2 * nw) + nw + j] = ww[j]; }
        TreeState ts{};
        ts.n_nodes = (uint32_t)(1 + pk); ts.n_req = (uint32_t)pk; ts.req_base = (uint32_t)(t * pk);
        S.ts[t] = ts;
        GameState g{};
        g.alive = 1; g.gid = t;
        S.gs[t] = g;
    }
}

struct ProbeErr { float dp = 0.0f, dv = 0.0f, dl = 0.0f; }; // max |dp|, |dv|, max(|dlogit|, |dv before tanh|)
static inline void probe_acc(float& m, float a, float b) {
    const float d = fabsf(a - b);
    if (!(d <= m)) m = d == d ? d : INFINITY; // (a NaN counts as a miss)
}

static int net_probe(Net& net, const Store& S, hipStream_t st) {
    const int hw = net.hw, rp = net.rowp, R = NET_PROBE_ROWS;
    const int CH = net.max_b < 128 ? net.max_b : 128;
    Net f32 = net; // a view whose fp32 scratch pointers are temporaries (forward_f32 reads in_f32 and writes p / v / vpre of the engine)
    f32.mode = OMOK_NET_F32;
    f32.chunk = CH;
    float* tmp[6] = {};
    const size_t sz[6] = {(size_t)CH * hw * NC, (size_t)CH * hw * NM, (size_t)CH * hw * NM, (size_t)CH * hw * NM, (size_t)CH * NF, (size_t)CH * NF};
    bool ok = true;
    for (int i = 0; i < 6 && ok; ++i) ok = hipMalloc((void**)&tmp[i], sizeof(float) * sz[i]) == hipSuccess;
    f32.sx = tmp[0]; f32.sh = tmp[1]; f32.sd = tmp[2]; f32.sg = tmp[3]; f32.s0 = tmp[4]; f32.s1 = tmp[5];
    int lrow = 0;
    const float* d_logits = net_logits(net, &lrow); // (split-precision forwards leave [row][lrow] here: hw policy logits, then the value in front of tanh)
    std::vector<float> hp[3], hv[3], hvp[3], hl((size_t)CH * hw), hlg((size_t)CH * lrow);
    for (int k = 0; k < 3; ++k) { hp[k].resize((size_t)CH * rp); hv[k].resize(CH); hvp[k].resize(CH); }
    ProbeErr plain[2];
    float lmax = 0.0f;
    const int fmt_before = net.diff_fp6 ? FC0_MIXED : net.fc0_fmt;
    // ---- part 1: plain rows (omok_evaluate_pv, mirror evaluations, single rows; the FULL rows of every path) in the fp6 and the f16 format ----
    for (int base = 0; base < R && ok; base += CH) {
        const int b = R - base < CH ? R - base : CH;
        k_probe_inputs<<<(b * hw + 255) / 256, 256, 0, st>>>(net.in_f32, hw, b, base);
        ok = ok && hipMemcpyAsync(S.d_count, &b, sizeof(int32_t), hipMemcpyHostToDevice, st) == hipSuccess;
        forward_f32(f32, S, b, st, nullptr);
        ok = ok && hipMemcpyAsync(hp[2].data(), net.p, sizeof(float) * (size_t)b * rp, hipMemcpyDeviceToHost, st) == hipSuccess;
        ok = ok && hipMemcpyAsync(hv[2].data(), net.v, sizeof(float) * b, hipMemcpyDeviceToHost, st) == hipSuccess;
        ok = ok && hipMemcpyAsync(hvp[2].data(), net.vpre, sizeof(float) * b, hipMemcpyDeviceToHost, st) == hipSuccess;
        ok = ok && hipMemcpyAsync(hl.data(), f32.sh, sizeof(float) * (size_t)b * hw, hipMemcpyDeviceToHost, st) == hipSuccess;
        ok = ok && hipStreamSynchronize(st) == hipSuccess;
        for (size_t i = 0; i < (size_t)b * hw; ++i) lmax = fmaxf(lmax, fabsf(hl[i]));
        for (int fmt = 0; fmt < 2 && ok; ++fmt) {
            net_set_fc0_format(net, fmt);
            forward_f16x3(net, S, b, true, st, nullptr);
            ok = ok && hipMemcpyAsync(hp[fmt].data(), net.p, sizeof(float) * (size_t)b * rp, hipMemcpyDeviceToHost, st) == hipSuccess;
            ok = ok && hipMemcpyAsync(hv[fmt].data(), net.v, sizeof(float) * b, hipMemcpyDeviceToHost, st) == hipSuccess;
            ok = ok && hipMemcpyAsync(hlg.data(), d_logits, sizeof(float) * (size_t)b * lrow, hipMemcpyDeviceToHost, st) == hipSuccess;
            ok = ok && hipStreamSynchronize(st) == hipSuccess && hipGetLastError() == hipSuccess;
            if (!ok) break;
            for (int r = 0; r < b; ++r) {
                for (int a = 0; a < hw; ++a) {
                    probe_acc(plain[fmt].dp, hp[fmt][(size_t)r * rp + a], hp[2][(size_t)r * rp + a]);
                    probe_acc(plain[fmt].dl, hlg[(size_t)r * lrow + a], hl[(size_t)r * hw + a]);
                }
                probe_acc(plain[fmt].dv, hv[fmt][r], hv[2][r]);
                probe_acc(plain[fmt].dl, hlg[(size_t)r * lrow + hw], hvp[2][r]);
            }
        }
    }
    // ---- part 2: one synthetic sibling round on the difference path (only if this engine's rounds can be large enough to take it) in fp6 / mixed / f16 ----
    ProbeErr rounds[3];
    int round_rows = 0, checked = 0;
    const int delta_min = net.n == 15 ? 3072 : 1024; // (forward_f16x3's threshold in the fp6 format: the largest of the three)
    int pg = net.games < 256 ? net.games : 256, pk = pg > 0 ? net.max_b / pg : 0; // trees, children per tree: 256 x 16 = 4096 rows where the engine is large enough
    if (pk > 32) pk = 32;
    if (pk > 16 && pg * 16 >= delta_min) pk = 16;
    const bool can_round = ok && net.siblings && net.d_groups && sib_env() >= 2 && pg > 0 && pk >= SIB_MIN && pg * pk >= delta_min;
    if (can_round) {
        const int rows = pg * pk, nw = (hw + 63) / 64, NSEL = rows < 512 ? rows : 512, step = rows / NSEL;
        Store PS{};
        PS.games = pg; PS.cap_nodes = pk + 1; PS.stride_nodes = (pk + 1) | 1; PS.cap_tables = PS.stride_tables = 1;
        void* d[8] = {};
        const size_t bytes[8] = {sizeof(NodeHdr) * (size_t)pg * PS.stride_nodes, 8 * (size_t)pg * PS.stride_nodes * 2 * nw, sizeof(TreeState) * (size_t)pg,
                                 2 * (size_t)pg * KMAX, sizeof(GameState) * (size_t)pg, 4 * (size_t)(rows + NSEL), 4 * (size_t)(rows + NSEL), 16};
        for (int i = 0; i < 8 && ok; ++i) ok = hipMalloc(&d[i], bytes[i]) == hipSuccess;
        if (ok) {
            PS.hdr = (NodeHdr*)d[0]; PS.board = (uint64_t*)d[1]; PS.ts = (TreeState*)d[2]; PS.req_node = (uint16_t*)d[3]; PS.gs = (GameState*)d[4];
            PS.req_ref = (uint32_t*)d[5]; PS.req_aux = (uint32_t*)d[6]; PS.d_count = (int32_t*)d[7];
            hipMemsetAsync(d[3], 0, bytes[3], st);
            hipMemsetAsync(d[5], 0, bytes[5], st);
            hipMemsetAsync(d[6], 0xFF, bytes[6], st);
            k_probe_store<<<pg, 64, 0, st>>>(PS, net.n, pk);
            std::vector<uint32_t> sel(NSEL);
            for (int j = 0; j < NSEL; ++j) { const int r = j * step; sel[j] = ((uint32_t)(r / pk) << 16) | (uint32_t)(1 + r % pk); } // (= req_ref[r] as k_probe_store writes it)
            ok = ok && hipMemcpyAsync(PS.req_ref + rows, sel.data(), 4 * (size_t)NSEL, hipMemcpyHostToDevice, st) == hipSuccess;
            std::vector<float> rp_[3], rv_[3], rl_[3];
            static const int fmts[3] = {FC0_FP6, FC0_MIXED, FC0_F16};
            for (int k = 0; k < 3 && ok; ++k) {
                net_set_fc0_format(net, fmts[k]);
                ok = ok && hipMemcpyAsync(PS.d_count, &rows, sizeof(int32_t), hipMemcpyHostToDevice, st) == hipSuccess;
                forward_f16x3(net, PS, rows, false, st, nullptr, 0);
                rp_[k].resize((size_t)rows * rp); rv_[k].resize(rows); rl_[k].resize((size_t)rows * lrow);
                ok = ok && hipMemcpyAsync(rp_[k].data(), net.p, sizeof(float) * (size_t)rows * rp, hipMemcpyDeviceToHost, st) == hipSuccess;
                ok = ok && hipMemcpyAsync(rv_[k].data(), net.v, sizeof(float) * rows, hipMemcpyDeviceToHost, st) == hipSuccess;
                ok = ok && hipMemcpyAsync(rl_[k].data(), d_logits, sizeof(float) * (size_t)rows * lrow, hipMemcpyDeviceToHost, st) == hipSuccess;
                ok = ok && hipStreamSynchronize(st) == hipSuccess && hipGetLastError() == hipSuccess;
            }
            // the fp32 kernels on NSEL of those request rows (every step-th), chunk by chunk
            Store PR = PS;
            for (int base = 0; base < NSEL && ok; base += CH) {
                const int b = NSEL - base < CH ? NSEL - base : CH;
                PR.req_ref = PS.req_ref + rows + base;
                PR.req_aux = PS.req_aux + rows + base;
                ok = ok && hipMemcpyAsync(PS.d_count, &b, sizeof(int32_t), hipMemcpyHostToDevice, st) == hipSuccess;
                launch_encode_requests(net.n, PR, net.in_f32, b, st);
                forward_f32(f32, PR, b, st, nullptr);
                ok = ok && hipMemcpyAsync(hp[2].data(), net.p, sizeof(float) * (size_t)b * rp, hipMemcpyDeviceToHost, st) == hipSuccess;
                ok = ok && hipMemcpyAsync(hv[2].data(), net.v, sizeof(float) * b, hipMemcpyDeviceToHost, st) == hipSuccess;
                ok = ok && hipMemcpyAsync(hvp[2].data(), net.vpre, sizeof(float) * b, hipMemcpyDeviceToHost, st) == hipSuccess;
                ok = ok && hipMemcpyAsync(hl.data(), f32.sh, sizeof(float) * (size_t)b * hw, hipMemcpyDeviceToHost, st) == hipSuccess;
                ok = ok && hipStreamSynchronize(st) == hipSuccess && hipGetLastError() == hipSuccess;
                if (!ok) break;
                for (int k = 0; k < 3; ++k)
                    for (int r = 0; r < b; ++r) {
                        const size_t row = (size_t)(base + r) * step;
                        for (int a = 0; a < hw; ++a) {
                            probe_acc(rounds[k].dp, rp_[k][row * rp + a], hp[2][(size_t)r * rp + a]);
                            probe_acc(rounds[k].dl, rl_[k][row * lrow + a], hl[(size_t)r * hw + a]);
                        }
                        probe_acc(rounds[k].dv, rv_[k][row], hv[2][r]);
                        probe_acc(rounds[k].dl, rl_[k][row * lrow + hw], hvp[2][r]);
                    }
                checked += b;
            }
            round_rows = rows;
        }
        for (int i = 0; i < 8; ++i) if (d[i]) hipFree(d[i]);
    }
    for (int i = 0; i < 6; ++i) if (tmp[i]) hipFree(tmp[i]);
    if (!ok) { net_set_fc0_format(net, fmt_before); return -1; }
    // ---- the choice: the fastest format whose every measured figure is inside the limits (fp6 < mixed (+2..3 %) < f16 (+20 %)) ----
    auto inside = [](const ProbeErr& e) { return e.dp <= NET_PROBE_LIMIT && e.dv <= NET_PROBE_LIMIT && e.dl <= NET_PROBE_LOGIT_LIMIT; };
    const bool have_rounds = round_rows > 0 && checked > 0;
    const bool fp6_ok = inside(plain[0]) && (!have_rounds || inside(rounds[0]));
    // (mixed and f16 share their full rows -- plain[1] is the same for both -- so only the difference path can tell them apart; without difference-path rounds the
    //  mixed format IS the f16 format)
    const bool mixed_ok = have_rounds && inside(rounds[1]);
    const int chosen = fp6_ok ? FC0_FP6 : mixed_ok ? FC0_MIXED : FC0_F16;
    net_set_fc0_format(net, chosen);
    // ---- the verdict on what was chosen: its full rows (plain) and, where measured, its difference-path round.  f16 is the end of the ladder, so its figures can be
    //      outside the margin limits -- never silently (round 4 committed the headline net at |dlogit| 5.2e-4 > 5e-4 without a word) -- and outside the contract.
    auto contract = [](const ProbeErr& e) { return e.dp <= NET_PROBE_CONTRACT && e.dv <= NET_PROBE_CONTRACT && e.dl <= NET_PROBE_CONTRACT; };
    const ProbeErr& cp = plain[chosen == FC0_FP6 ? 0 : 1];
    const ProbeErr& cr = rounds[chosen == FC0_FP6 ? 0 : chosen == FC0_MIXED ? 1 : 2];
    net.probe_outside = (inside(cp) && (!have_rounds || inside(cr))) ? 0 : (contract(cp) && (!have_rounds || contract(cr))) ? 1 : 2;
    if (net.probe_outside) {
        static bool said[3] = {};
        if (!said[net.probe_outside]) {
            said[net.probe_outside] = true;
            fprintf(stderr, "omok_mi355x: net_commit: the %s operand format measures |dp| %.2e |dv| %.2e |dlogit| %.2e on plain rows%s against the fp32 kernels (max |logit| %.0f): %s\n",
                    chosen == FC0_FP6 ? "fp6" : chosen == FC0_MIXED ? "mixed" : "f16", cp.dp, cp.dv, cp.dl, have_rounds ? " (+ a sibling round)" : "", lmax,
                    net.probe_outside == 1 ? "outside the probe's margin (3e-4 / 5e-4), inside the 1e-3 contract -- committed (OMOK_STAT_PROBE_OUTSIDE = 1)"
                                           : "OUTSIDE the 1e-3 contract with the most precise split-operand format -- this net is evaluated with the fp32 kernels (slow; OMOK_STAT_PROBE_OUTSIDE = 2)");
        }
    }
    net.probe[0] = (float)R;
    net.probe[1] = plain[0].dp; net.probe[2] = plain[0].dv;
    net.probe[3] = plain[1].dp; net.probe[4] = plain[1].dv;
    net.probe[5] = lmax;
    net.probe[6] = 1.0f;
    net.probe[7] = plain[0].dl; net.probe[8] = plain[1].dl;
    net.probe[9] = (float)checked;
    for (int k = 0; k < 3; ++k) { net.probe[10 + 3 * k] = rounds[k].dp; net.probe[11 + 3 * k] = rounds[k].dv; net.probe[12 + 3 * k] = rounds[k].dl; }
    static const bool verbose = getenv("OMOK_PROBE_LOG") && atoi(getenv("OMOK_PROBE_LOG"));
    if (verbose)
        fprintf(stderr, "[net probe] N=%d plain rows %d: fp6 |dp| %.2e |dv| %.2e |dlogit| %.2e, f16 %.2e %.2e %.2e (max |logit| %.1f); sibling round of %d rows (%d checked): "
                        "fp6 %.2e %.2e %.2e, mixed %.2e %.2e %.2e, f16 %.2e %.2e %.2e -> %s\n", net.n, R, plain[0].dp, plain[0].dv, plain[0].dl, plain[1].dp, plain[1].dv, plain[1].dl,
                lmax, round_rows, checked, rounds[0].dp, rounds[0].dv, rounds[0].dl, rounds[1].dp, rounds[1].dv, rounds[1].dl, rounds[2].dp, rounds[2].dv, rounds[2].dl,
                chosen == FC0_FP6 ? "fp6" : chosen == FC0_MIXED ? "mixed" : "f16");
    return 0;
}

bool net_logits_cover_batch(const Net& net, int max_count) { return net.mode != OMOK_NET_F32 && max_count <= net.max_b; }

bool net_rows_fit_policy(const Net& net) { return net.mode != OMOK_NET_F32 && heads_mt(net.hw) * 32 == net.rowp; }

void net_forward_requests(Net& net, const Store& S, int max_count, hipStream_t st, Prof* prof, int sibling_side, bool skip_softmax, bool rows_to_nodes) {
    if (max_count <= 0) return;
    if (max_count > net.max_b) max_count = net.max_b;
    if (net.mode == OMOK_NET_F32) {
        recover_handed_over_fill(net, S, st, "fp32 kernels");
        launch_encode_requests(net.n, S, net.in_f32, max_count, st);
        forward_f32(net, S, max_count, st, prof);
        net.plan_path = 3; net.plan_rows = max_count; net.plan_nsplit = net.plan_tsplit = 0;
    } else {
        forward_f16x3(net, S, max_count, false, st, prof, sibling_side, skip_softmax, rows_to_nodes);
    }
}

void net_forward_inputs(Net& net, const Store& S, int count, hipStream_t st, Prof* prof) {
    if (count <= 0) return;
    if (net.mode == OMOK_NET_F32) {
        forward_f32(net, S, count, st, prof);
        net.plan_path = 3; net.plan_rows = count; net.plan_nsplit = net.plan_tsplit = 0;
    } else forward_f16x3(net, S, count, true, st, prof);
}

} // namespace omok
