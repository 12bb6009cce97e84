// The input end that EDSR_1D and ESPCN_1D train through (edsr_train.hip, espcn_train.hip): a convolution 1 -> 64 of K = 3 or 5
// taps with its activation, forward, weight gradient and data gradient, on the vector pipe in exact fp32, plus the host glue
// that every entry point of the two files repeats.  x / dx are [N][L], the activations channel-last [N][L][64], un-gapped and
// 16-byte aligned; the rows of all waveforms are one flat sequence of N L rows and every row end is a predicate on t = row % L.
//
// Thread = (row slot tid >> 4, channels 4 q .. 4 q + 3): a row is 16 lanes of 16 bytes, a wave four rows.  `Act` is the model's
// activation:
//   fwd(v)                  the activation itself
//   bwd(g, g2, saved, at)   the float4 at `at` of g' = the gradient through the activation, from the saved output
//   zero_fed_row_ends       what the forward does with a tap that leaves the waveform: feed a zero into the fmaf (true) or skip
//                           the tap (false).  The two differ for a non-finite weight and in the sign of a zero, and each model
//                           keeps the form it was recorded with.
// The orders below are part of the results' bits (tests/test_gpu_train_ends_bits.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "stof_common.h"
#include "wgrad_reduce.h"

namespace {

constexpr int ENDS_C = 64;                  // channels of the activation
constexpr int ENDS_TILE = 64;               // rows per work-group of the element-wise kernels (4 passes of 16 rows)
constexpr int ENDS_CHUNK = 256;             // rows per chunk of the weight-gradient kernels (16 passes of 16 rows)
constexpr int ENDS_DTILE = 256;             // outputs per work-group of the data gradient
constexpr int ENDS_DROWS = 272;             // its tile with the K / 2-row halos, as 17 passes of 16 rows
constexpr int64_t MAX_ROWS = (1ll << 25) - 1;        // N L 64 stays below 2^31

__device__ inline float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// tap d of a K-tap window around sample t stays inside the waveform (0 <= t < L: one side can leave)
template <int K>
__device__ inline bool tap_inside(int t, int d, int L) {
    return d < K / 2 ? t + d - K / 2 >= 0 : d > K / 2 ? t + d - K / 2 < L : true;
}

// One output: bias, then taps 0 .. K - 1 as one fmaf chain.  A thread's 4 K weights and four biases stay in registers for the
// four rows it writes.
template <int K, class Act>
__device__ inline void ends_in_fwd(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                   float* __restrict__ y, int total, int L) {
    const int q = threadIdx.x & 15, slot = threadIdx.x >> 4;
    float wr[4][K], br[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        br[i] = b[4 * q + i];
#pragma unroll
        for (int d = 0; d < K; ++d) wr[i][d] = w[(4 * q + i) * K + d];
    }
    const int r0 = blockIdx.x * ENDS_TILE + slot;
    if (r0 >= total) return;
    int t = r0 % L;
#pragma unroll
    for (int it = 0; it < ENDS_TILE / 16; ++it) {
        const int row = r0 + 16 * it;
        if (row >= total) break;
        float xv[K];
        bool ok[K];
#pragma unroll
        for (int d = 0; d < K; ++d) {
            ok[d] = tap_inside<K>(t, d, L);
            xv[d] = ok[d] ? x[row + d - K / 2] : 0.f;
        }
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float acc = br[i];
#pragma unroll
            for (int d = 0; d < K; ++d) acc = (Act::zero_fed_row_ends || ok[d]) ? fmaf(wr[i][d], xv[d], acc) : acc;
            o[i] = Act::fwd(acc);
        }
        *reinterpret_cast<float4*>(y + (size_t)row * ENDS_C + 4 * q) = make_float4(o[0], o[1], o[2], o[3]);
        t += 16;
        if (t >= L) t %= L;
    }
}

// dw[f][d] = sum_rows g'[row][f] x[t + d - K / 2], db[f] = sum_rows g'[row][f].  A work-group walks its 256-row chunks in a fixed
// assignment (chunk k -> work-group k mod grid); a thread keeps K + 1 sums per channel [tap 0 .. K - 1 | plain sum]; the 16 row
// slots fold pairwise in a fixed order through LDS, ((0 + 1) + (2 + 3)) + .. per group of four, then (s0 + s1) + (s2 + s3).
// ONE partial per work-group: [f * K + d] (64 K), then [64 K + f]; no float atomics.
template <int K>
constexpr int ends_wgrad_floats() { return ENDS_C * (K + 1); }

template <int K, class Act>
__device__ inline void ends_in_wgrad(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ g2,
                                     const float* __restrict__ saved, float* __restrict__ copies, int total, int L) {
    constexpr int E = ends_wgrad_floats<K>();
    __shared__ __attribute__((aligned(16))) float red[16 * E];
    const int tid = threadIdx.x, q = tid & 15, slot = tid >> 4;
    float acc[4][K + 1];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < K + 1; ++k) acc[i][k] = 0.f;
    for (long long c0 = (long long)blockIdx.x * ENDS_CHUNK; c0 < total; c0 += (long long)gridDim.x * ENDS_CHUNK) {
        const int r0 = (int)c0 + slot;
        int t = r0 % L;
#pragma unroll 4
        for (int it = 0; it < ENDS_CHUNK / 16; ++it) {
            const int row = r0 + 16 * it;
            if (row >= total) break;
            const float4 v = Act::bwd(g, g2, saved, (size_t)row * ENDS_C + 4 * q);
            const float gv[4] = {v.x, v.y, v.z, v.w};
            float xv[K];
#pragma unroll
            for (int d = 0; d < K; ++d) xv[d] = tap_inside<K>(t, d, L) ? x[row + d - K / 2] : 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int d = 0; d < K; ++d) acc[i][d] = fmaf(gv[i], xv[d], acc[i][d]);
                acc[i][K] += gv[i];
            }
            t += 16;
            if (t >= L) t %= L;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < K + 1; ++k) red[slot * E + (q * 4 + i) * (K + 1) + k] = acc[i][k];
    __syncthreads();
    for (int el = tid; el < E; el += 256) {
        float s[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            s[k] = (red[(4 * k) * E + el] + red[(4 * k + 1) * E + el]) + (red[(4 * k + 2) * E + el] + red[(4 * k + 3) * E + el]);
        const int f = el / (K + 1), k = el % (K + 1);
        copies[(size_t)blockIdx.x * E + (k < K ? f * K + k : ENDS_C * K + f)] = (s[0] + s[1]) + (s[2] + s[3]);
    }
}

// dx[row] = out_scale * sum_d p_d[row - d + K / 2] with p_d[row] = sum_f w[f][d] g'[row][f], a term dropped where its row leaves
// the waveform.  A work-group takes 256 outputs: the 16 lanes of a row each form their four channels' share of the K dot
// products (channels inner), a fixed xor butterfly m = 8, 4, 2, 1 over the 16 lanes adds them, the (256 + 2 (K / 2)) x K sums go
// through LDS; an output adds the centre tap, then for o = 1 .. K / 2 the tap of row + o, then the tap of row - o.
template <int K, class Act>
__device__ inline void ends_in_dgrad(const float* __restrict__ g, const float* __restrict__ g2, const float* __restrict__ saved,
                                     const float* __restrict__ w, float* __restrict__ dx, int total, int L, float out_scale) {
    constexpr int H = K / 2;
    __shared__ float ps[K][ENDS_DROWS];                      // [tap][row r0 - H + j], j < 256 + 2 H
    const int tid = threadIdx.x, q = tid & 15, slot = tid >> 4;
    float wr[4][K];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int d = 0; d < K; ++d) wr[i][d] = w[(4 * q + i) * K + d];
    const long long r0 = (long long)blockIdx.x * ENDS_DTILE;
    for (int j = slot; j < ENDS_DROWS; j += 16) {            // (every lane of a wave stays in the loop: the butterfly needs all 16)
        const long long row = r0 - H + j;
        float p[K];
#pragma unroll
        for (int d = 0; d < K; ++d) p[d] = 0.f;
        if (j < ENDS_DTILE + 2 * H && row >= 0 && row < total) {
            const float4 v = Act::bwd(g, g2, saved, (size_t)row * ENDS_C + 4 * q);
            const float gv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int d = 0; d < K; ++d)
#pragma unroll
                for (int i = 0; i < 4; ++i) p[d] = fmaf(wr[i][d], gv[i], p[d]);
        }
#pragma unroll
        for (int d = 0; d < K; ++d) {
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) p[d] += __shfl_xor(p[d], m, 16);
        }
        if (q == 0) {
#pragma unroll
            for (int d = 0; d < K; ++d) ps[d][j] = p[d];
        }
    }
    __syncthreads();
    const long long row = r0 + tid;
    if (row >= total) return;
    const int t = (int)(row % L), j = tid + H;
    float s = ps[H][j];
#pragma unroll
    for (int o = 1; o <= H; ++o) {
        if (t + o < L) s += ps[H - o][j + o];
        if (t >= o) s += ps[H + o][j - o];
    }
    dx[row] = s * out_scale;
}

// -------------------------------------------------------------------------------------------------------- host glue
// N L within the range of the 32-bit indices (N, L >= 1)
inline bool rows_ok(int64_t N, int64_t L) { return N <= MAX_ROWS / L; }
// partials (work-groups) of a weight-gradient launch: one per chunk, `max_copies` at the most
inline int wgrad_copies(int64_t rows, int chunk, int max_copies) {
    const int64_t chunks = (rows + chunk - 1) / chunk;
    return (int)(chunks < max_copies ? chunks : max_copies);
}

// The argument checks of an entry point over N L rows, in the order the ABI promises: a negative size is a bad argument, an
// empty batch is done (STOF_OK) before any pointer is looked at, then a NULL pointer, then the row limit.  ENDS_GO: launch.
constexpr int ENDS_GO = -1;
template <class... P>
inline int check_rows(int64_t N, int64_t L, const P*... ptrs) {
    if (N < 0 || L < 0) return STOF_ERR_BAD_ARG;
    if (N == 0 || L == 0) return STOF_OK;
    if ((... || !ptrs)) return STOF_ERR_BAD_ARG;
    if (!rows_ok(N, L)) return STOF_ERR_UNSUPPORTED;
    return ENDS_GO;
}
// The same for a weight gradient: dw (ndw floats) and db (ndb floats) must be there even for an empty batch, which zeroes
// them; the workspace size is checked between the pointers and the row limit.
template <class... P>
inline int check_wgrad_rows(int64_t N, int64_t L, float* dw, size_t ndw, float* db, size_t ndb, size_t workspace_bytes, size_t needed,
                            hipStream_t s, const P*... ptrs) {
    if (N < 0 || L < 0 || !dw || !db) return STOF_ERR_BAD_ARG;
    if (N == 0 || L == 0) {
        if (hipMemsetAsync(dw, 0, ndw * sizeof(float), s) != hipSuccess || hipMemsetAsync(db, 0, ndb * sizeof(float), s) != hipSuccess)
            return STOF_ERR_HIP;
        return STOF_OK;
    }
    if ((... || !ptrs)) return STOF_ERR_BAD_ARG;
    if (workspace_bytes < needed) return STOF_ERR_WORKSPACE;
    if (!rows_ok(N, L)) return STOF_ERR_UNSUPPORTED;
    return ENDS_GO;
}

}  // namespace
