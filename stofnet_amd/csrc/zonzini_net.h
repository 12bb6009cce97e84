// What the inference file (zonzini.hip) and the training file (zonzini_train.hip) of the Zonzini baselines share: the
// geometry of the two nets, the packed weight blob and the three forward kernels.  The kernels take a TRAIN flag: false is
// the inference chain; true additionally writes what the backward pass needs (a selector byte per stored activation, the
// pooled features and fc1's output) and computes every value with the same instructions in the same order, so the training
// forward's y is bitwise the inference y.
//
//   x [N, 1, L] -> 4 (Small) or 5 (Large) x { Conv1d(k = 10, stride 2) -> ReLU -> MaxPool1d(2) } -> mean over time
//   -> Linear(C, 1024) -> ReLU -> Linear(1024, 1) -> y [N, 1]
//
// Activations between layers are channel-last fp32, act[n][t][Cpad] (Cpad = C rounded up to 4; pad channels hold 0).
//
//   zz_conv1_kernel      layer 1 (Cin = 1, K = 10) on the vector pipe: one thread per (row, pooled time, channel)
//   zz_conv_kernel       layers 2..: conv + bias + ReLU + max-pool as one implicit GEMM on v_mfma_f32_32x32x2_f32.
//                        M = (row, pooled time p) flattened over the batch, N = output channel, K = (tap, input channel).
//                        With the channel-last layout and stride 2 the K span of conv output t is the contiguous run
//                        act[n][2t .. 2t + 9][0 .. Cpad), so the A operand is a straight load.  Pooled output p needs conv
//                        outputs 2p and 2p + 1 (windows at input rows 4p and 4p + 2): two accumulators share every B
//                        fragment; the odd conv output the pool drops is never computed, the pre-pool activations never
//                        leave the registers.  Epilogue relu(max(a, b) + bias), NaN-propagating like max_pool1d / ReLU.
//   zz_head_kernel       mean over the last pooled length, fc1 + ReLU, fc2, HEAD_ROWS rows per work-group so that
//                        fc1's weight streams once for all of them; optional feature output.
//
// Every output element is one fixed-order chain (MFMA k order, fixed loops, fixed reduction trees, no atomics): a row's
// result does not depend on the batch it is in or on its position there.
//
// Selector byte of a stored element (TRAIN): 0 = the output is not > 0 (no gradient; pad channels too), 1 = conv output 2p
// won the pool, 2 = conv output 2p + 1 won.  A tie goes to 2p, as max_pool1d's backward gives the first maximum the gradient.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "mfma32_frag.h"
#include "stof_common.h"

namespace {

using namespace stof_frag;

constexpr int KW = 10;                 // kernel_size of every conv
constexpr int FC1 = 1024;              // fc1 width
constexpr int MAXL = 5;                // conv layers of the Large net
constexpr int HEAD_ROWS = 16;          // rows per work-group of the head
constexpr int HEAD_THREADS = FC1;     // one fc1 unit per thread
constexpr int CONV_WAVES = 4;          // waves per work-group of zz_conv_kernel: 2 M tiles x 2 N tiles

struct Geometry {
    int layers;
    int cout[MAXL];                    // output channels of conv layer i
    int cpad[MAXL];                    // stored channels of its activation (multiple of 4)
    int min_len;
};

inline bool geometry(const stof_zonzini_desc* d, Geometry& g) {
    if (!d) return false;
    static const int small_c[4] = {16, 32, 64, 64};
    static const int large_c[5] = {50, 100, 150, 200, 250};
    if (d->variant == STOF_ZONZINI_SMALL) {
        g.layers = 4; g.min_len = 936;
        for (int i = 0; i < 4; ++i) g.cout[i] = small_c[i];
    } else if (d->variant == STOF_ZONZINI_LARGE) {
        g.layers = 5; g.min_len = 3752;
        for (int i = 0; i < 5; ++i) g.cout[i] = large_c[i];
    } else {
        return false;
    }
    for (int i = 0; i < g.layers; ++i) g.cpad[i] = (g.cout[i] + 3) & ~3;
    return true;
}

inline int ntiles(int c) { return (c + 31) / 32; }
inline int64_t pooled_len(int64_t l) { return l < KW ? 0 : ((l - KW) / 2 + 1) / 2; }

// Packed blob (floats, every section starts on a 256-byte boundary):
//   c1w [cpad0][10], c1b [cpad0]                                               layer 1
//   for layer i >= 1: frag [ntiles(cout)][K / 8][64 lanes][4], bias [32 ntiles]  K = 10 cpad[i-1], k = tap * cpad[i-1] + ci;
//       lane l, element s of K group q holds W[32 tile + (l & 31)][k = 8 q + 4 (l >> 5) + s] (0 outside the real channels):
//       the A operand of lane l reads act[.. + 8 q + 4 (l >> 5) .. + 3] with the same k order, one float4 each
//   fc1t [C][1024] (fc1.weight transposed), fc1b [1024], fc2w [1024], fc2b [1]
struct Layout {
    int64_t c1w, c1b, frag[MAXL], bias[MAXL], fc1t, fc1b, fc2w, fc2b, total;
};

inline Layout layout(const Geometry& g) {
    Layout o{};
    int64_t at = 0;
    o.c1w = at; at = align_up(at + (int64_t)g.cpad[0] * KW);
    o.c1b = at; at = align_up(at + g.cpad[0]);
    for (int i = 1; i < g.layers; ++i) {
        const int64_t K = (int64_t)KW * g.cpad[i - 1];
        o.frag[i] = at; at = align_up(at + (int64_t)ntiles(g.cout[i]) * (K / 8) * 256);
        o.bias[i] = at; at = align_up(at + 32 * ntiles(g.cout[i]));
    }
    const int C = g.cout[g.layers - 1];
    o.fc1t = at; at = align_up(at + (int64_t)C * FC1);
    o.fc1b = at; at = align_up(at + FC1);
    o.fc2w = at; at = align_up(at + FC1);
    o.fc2b = at; at = align_up(at + 1);
    o.total = at;
    return o;
}

__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b); }
__device__ __forceinline__ float nan_relu(float v) { return v > 0.f ? v : (v != v ? v : 0.f); }
// selector of relu(max(a, e) + b) given v = max(a, e) + b: the reference compares relu(a + b) with relu(e + b)
__device__ __forceinline__ uint8_t pool_sel(float a, float e, float b, float v) {
    return v > 0.f ? ((e + b) > (a + b) ? 2 : 1) : 0;
}

// ---------------------------------------------------------------------------------------------------------------- layer 1
// out[(n, p)][c] = relu(max(conv(4p), conv(4p + 2)) + b[c]) for c < cout, 0 for the pad channels.  conv(t) = sum over
// taps j in order of w[c][j] x[n][t + j] (fma chain).
template <bool TRAIN>
__global__ __launch_bounds__(256) void zz_conv1_kernel(const float* __restrict__ x, long long L, long long Lp, int cout, int cpad,
                                                       const float* __restrict__ w, const float* __restrict__ b,
                                                       float* __restrict__ out, long long total, uint8_t* __restrict__ sel) {
    const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= total) return;
    const int c = (int)(o % cpad);
    const long long m = o / cpad, n = m / Lp, p = m % Lp;
    if (c >= cout) {
        out[o] = 0.f;
        if constexpr (TRAIN) sel[o] = 0;
        return;
    }
    const float* xs = x + n * L + 4 * p;              // reads x[4p .. 4p + 11] <= 4 Lp + 7 <= L - 1
    float xv[KW + 2];
#pragma unroll
    for (int j = 0; j < KW + 2; ++j) xv[j] = xs[j];
    float a = 0.f, e = 0.f;
#pragma unroll
    for (int j = 0; j < KW; ++j) {
        const float wj = w[c * KW + j];
        a = fmaf(wj, xv[j], a);
        e = fmaf(wj, xv[j + 2], e);
    }
    const float v = nan_max(a, e) + b[c];
    out[o] = nan_relu(v);
    if constexpr (TRAIN) sel[o] = pool_sel(a, e, b[c], v);
}

// ------------------------------------------------------------------------------------------------------- layers 2 .. n
// Work-group: 4 waves = 2 M tiles (32 pooled outputs each) x 2 N tiles (32 output channels each).  Wave (mt, nt) keeps two
// 32 x 32 accumulators (conv outputs 2p and 2p + 1) and walks K in groups of 8: per group one float4 of A per accumulator
// and one float4 of B per lane, four MFMAs per accumulator.  The next group's operands are loaded before this group's MFMAs.
template <bool TRAIN>
__global__ __launch_bounds__(64 * CONV_WAVES) void zz_conv_kernel(const float* __restrict__ in, long long Lin, int cpad_in,
                                                                  long long M, long long Lp, int cout, int cpad_out,
                                                                  int n_tiles, const float4* __restrict__ frag,
                                                                  const float* __restrict__ bias, float* __restrict__ out,
                                                                  uint8_t* __restrict__ sel) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nt = blockIdx.y * 2 + (wave & 1);
    if (nt >= n_tiles) return;
    const long long m0 = ((long long)blockIdx.x * 2 + (wave >> 1)) * 32;
    if (m0 >= M) return;
    const int i = lane & 31, h = lane >> 5;
    long long m = m0 + i;
    if (m >= M) m = M - 1;                            // tail rows compute a duplicate and store nothing
    const long long n = m / Lp, p = m % Lp;
    // even window: rows 4p .. 4p + 9, odd window: rows 4p + 2 .. 4p + 11 (<= Lin - 1 for every p < Lp)
    const float* a_even = in + (n * Lin + 4 * p) * cpad_in + 4 * h;
    const float* a_odd = a_even + 2 * cpad_in;
    const int groups = KW * cpad_in / 8;
    const float4* bq = frag + (long long)nt * groups * 64 + lane;
    f32x16 acc_e = {}, acc_o = {};
    float4 ae = *reinterpret_cast<const float4*>(a_even);
    float4 ao = *reinterpret_cast<const float4*>(a_odd);
    float4 bw = bq[0];
    for (int q = 0; q < groups; ++q) {
        const float4 ce = ae, co = ao, cb = bw;
        if (q + 1 < groups) {
            ae = *reinterpret_cast<const float4*>(a_even + 8 * (q + 1));
            ao = *reinterpret_cast<const float4*>(a_odd + 8 * (q + 1));
            bw = bq[(long long)(q + 1) * 64];
        }
        acc_e = __builtin_amdgcn_mfma_f32_32x32x2f32(ce.x, cb.x, acc_e, 0, 0, 0);
        acc_o = __builtin_amdgcn_mfma_f32_32x32x2f32(co.x, cb.x, acc_o, 0, 0, 0);
        acc_e = __builtin_amdgcn_mfma_f32_32x32x2f32(ce.y, cb.y, acc_e, 0, 0, 0);
        acc_o = __builtin_amdgcn_mfma_f32_32x32x2f32(co.y, cb.y, acc_o, 0, 0, 0);
        acc_e = __builtin_amdgcn_mfma_f32_32x32x2f32(ce.z, cb.z, acc_e, 0, 0, 0);
        acc_o = __builtin_amdgcn_mfma_f32_32x32x2f32(co.z, cb.z, acc_o, 0, 0, 0);
        acc_e = __builtin_amdgcn_mfma_f32_32x32x2f32(ce.w, cb.w, acc_e, 0, 0, 0);
        acc_o = __builtin_amdgcn_mfma_f32_32x32x2f32(co.w, cb.w, acc_o, 0, 0, 0);
    }
    // C/D map: column (output channel) = lane & 31, row (pooled output) = (r & 3) + 8 (r >> 2) + 4 h
    const int c = nt * 32 + i;
    if (c >= cpad_out) return;
    const float bc = c < cout ? bias[c] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long long row = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row < M) {
            const float v = nan_max(acc_e[r], acc_o[r]) + bc;
            out[row * cpad_out + c] = c < cout ? nan_relu(v) : 0.f;
            if constexpr (TRAIN) sel[row * cpad_out + c] = c < cout ? pool_sel(acc_e[r], acc_o[r], bc, v) : (uint8_t)0;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ head
// Rows r0 .. r0 + 15 of the batch: f[r][c] = (sum over p in order of act[r][p][c]) / Lp; thread j is fc1 unit j:
// h = relu(b1[j] + sum over c in order of W1[j][c] f[r][c]); y[r] = b2 + the fixed-order sum of w2[j] h over the units
// (butterfly inside each wave, then the 16 waves in order).  TRAIN: hidden [N][1024] receives h.
template <bool TRAIN>
__global__ __launch_bounds__(HEAD_THREADS) void zz_head_kernel(const float* __restrict__ act, long long N, long long Lp, int C,
                                                               int cpad, const float* __restrict__ fc1t,
                                                               const float* __restrict__ fc1b, const float* __restrict__ fc2w,
                                                               const float* __restrict__ fc2b, float* __restrict__ y,
                                                               float* __restrict__ features, float* __restrict__ hidden) {
    __shared__ float4 f[256][HEAD_ROWS / 4];                 // [channel][row]
    __shared__ float red[HEAD_ROWS][HEAD_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long r0 = (long long)blockIdx.x * HEAD_ROWS;
    const float len = (float)Lp;
    float* const fs = reinterpret_cast<float*>(f);
    for (int q = t; q < HEAD_ROWS * C; q += HEAD_THREADS) {
        const int r = q / C, c = q % C;
        long long n = r0 + r;
        if (n >= N) n = N - 1;
        const float* a = act + n * Lp * cpad + c;
        float s = 0.f;
        for (long long p = 0; p < Lp; ++p) s += a[p * cpad];
        const float v = s / len;
        fs[c * HEAD_ROWS + r] = v;
        if (features != nullptr && r0 + r < N) features[(r0 + r) * C + c] = v;
    }
    __syncthreads();
    const int j = t;
    float h[HEAD_ROWS];
#pragma unroll
    for (int r = 0; r < HEAD_ROWS; ++r) h[r] = 0.f;
    for (int c = 0; c < C; ++c) {
        const float wv = fc1t[(long long)c * FC1 + j];
#pragma unroll
        for (int r4 = 0; r4 < HEAD_ROWS / 4; ++r4) {
            const float4 v = f[c][r4];
            h[4 * r4] = fmaf(wv, v.x, h[4 * r4]);
            h[4 * r4 + 1] = fmaf(wv, v.y, h[4 * r4 + 1]);
            h[4 * r4 + 2] = fmaf(wv, v.z, h[4 * r4 + 2]);
            h[4 * r4 + 3] = fmaf(wv, v.w, h[4 * r4 + 3]);
        }
    }
    const float bj = fc1b[j], w2 = fc2w[j];
#pragma unroll
    for (int r = 0; r < HEAD_ROWS; ++r) {
        const float hr = nan_relu(h[r] + bj);
        if constexpr (TRAIN) {
            if (r0 + r < N) hidden[(r0 + r) * FC1 + j] = hr;
        }
        float v = w2 * hr;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) red[r][wave] = v;
    }
    __syncthreads();
    if (t < HEAD_ROWS && r0 + t < N) {
        float s = 0.f;
        for (int w = 0; w < HEAD_THREADS / 64; ++w) s += red[t][w];
        y[r0 + t] = s + fc2b[0];
    }
}

}  // namespace
