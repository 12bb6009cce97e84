// EDSR_1D and ESPCN_1D, the two baselines of the reference that ride on SampleShuffle1D (models/edsr_1d.py,
// models/espcn_1d.py), on gfx950, inference only, exact fp32 (v_mfma_f32_32x32x2_f32).
//
// ---- EDSR_1D(1, 64, B, r) ----------------------------------------------------------------------------------------------
//   x [N, 1, L] -> conv_input 1 -> 64 (k 3) + ReLU = first
//               -> B x (conv1 64 -> 64 (k 3) + ReLU, conv2 64 -> 64 (k 3), + block input)
//               -> conv_mid 64 -> 64 (k 3) + first = trunk
//               -> SampleShuffle1D(r) -> conv_output 64 / r -> 1 (k 3)                               -> y [N, 1, L r]
// Activations are channel-last fp32 with GAP zero rows around every waveform (as in sincnet.hip):
//   buffer row GAP + n (L + GAP) + t holds act[n][t][0 .. 64); the GAP rows before it are zero.
// The zero rows are the padding = 1 zeros, so the K span (tap, input channel) of output (n, t) is the contiguous run of
// rows t - 1 .. t + 1.  Three buffers: first (the long skip), cur, tmp.
//
//   ed_gaps_kernel   zeroes the GAP rows of the three buffers (the workspace is not assumed to be clean)
//   ed_in_kernel     conv_input + ReLU on the vector pipe, one thread per (output, 4 channels)
//   ed_conv_kernel   64 -> 64, k 3 as one implicit GEMM, M = (row, t) flattened over the batch, N = 64, K = 192.  A wave
//                    owns 32 outputs x 64 channels (two 32 x 32 accumulators share every A fragment); below NARROW_M
//                    outputs a wave owns one 32-channel tile (same k order: results are bitwise the same).  Epilogue:
//                    + bias, optional + residual (read from a second buffer at the element the thread writes, so the
//                    residual buffer may be the output buffer; the halo always comes from another buffer), optional
//                    ReLU, optional dense copy [N, L, 64].
//   ed_out_kernel    shuffle + conv_output on the vector pipe.  The shuffled map is S[c][w r + k] = trunk[w][k C + c]
//                    (C = 64 / r), so the C channels of shuffled sample m' are the contiguous floats m' C .. m' C + C - 1
//                    of the waveform's [L][64] block; m' = -1 and m' = L r fall into the zero GAP rows.  One thread per
//                    output sample m: bias, then taps d = 0..2 over channels c = 0..C-1 as one fma chain.
//
// ---- ESPCN_1D(r) -------------------------------------------------------------------------------------------------------
//   x [N, 1, L] -> conv1 1 -> 64 (k 5) + tanh -> conv2 64 -> 32 (k 3) + tanh -> conv3 32 -> r (k 3)
//               -> SampleShuffle1D(r) (one channel survives: the channel-last conv3 output is the shuffled row) -> sigmoid
//   es_kernel        one launch.  A work-group owns ES_T = 126 samples of one row:
//                      1. xs  = x[t0 - 4 .. t0 + 130), zeros outside [0, L)
//                      2. a1  = tanh(conv1) at t0 - 2 .. t0 + 128 on the vector pipe -> LDS, 0 outside [0, L)
//                      3. a2  = tanh(conv2) at t0 - 1 .. t0 + 127 on MFMA (K = 192 from a1, eight partial sums) -> LDS, 0
//                         outside [0, L)
//                      4. conv3 at t0 .. t0 + 126 on MFMA (K = 96 from a2, r padded to 32 or 64 columns) + bias -> the
//                         logits tile in LDS (over a1), then one coalesced pass: logits (optional) and sigmoid -> y
//                    The zeros outside [0, L) are the padding of conv2 / conv3 (zeros of a1 / a2, not tanh(bias)).
//
// Every output element is one fixed-order chain (MFMA k order, fixed fma loops, no atomics) inside a tile that is fixed
// by (row, t), so a row's result does not depend on its batch, its chunk or its position there.  NaN propagates as in
// torch: the sums, tanhf, expf and the ReLU form v < 0 ? 0 : v all keep it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include "mfma32_frag.h"
#include "stof_common.h"

namespace {

using namespace stof_frag;

constexpr int C = 64;                      // EDSR num_features
constexpr int GAP = 1;                     // zero rows between waveforms (= the padding of every EDSR conv)
constexpr int KC = 3 * C;                  // K of the 64 -> 64 convs
constexpr int GC = KC / 8;                 // K groups of 8
constexpr int FRAG_C = 2 * GC * 64 * 4;    // floats of one 64 -> 64 weight in fragment order
constexpr int64_t NARROW_M = 64 * 1024;    // below N L = this, waves of ed_conv_kernel own one N tile instead of two
constexpr int MAX_BLOCKS = 1024;

constexpr int ES_T = 126;                  // samples per work-group of es_kernel (a2 needs ES_T + 2 = 4 waves x 32 rows)
constexpr int ES_XS = ES_T + 8;            // staged x
constexpr int ES_R1 = 68, ES_ROWS1 = ES_T + 4;    // a1: row stride (floats), rows t0 - 2 .. t0 + ES_T + 1
constexpr int ES_R2 = 36, ES_ROWS2 = ES_T + 4;    // a2: rows t0 - 1 .. t0 + ES_T (+ 2 rows only the two unused outputs read)
constexpr int ES_G2 = 3 * 64 / 8, ES_G3 = 3 * 32 / 8;

// EDSR blob (floats, every section starts on a 256-byte boundary), B = num_blocks, Cq = 64 / r:
//   cin   [4][64]                   rows 0..2 = conv_input.weight[c][0][tap], row 3 = conv_input.bias
//   B x ( frag [2][24][64][4], bias [64] ) for conv1, then the same for conv2, of every block in order
//   frag, bias of conv_mid
//   cout  [3][Cq] = conv_output.weight[0][c][tap] as [tap][c], then conv_output.bias (1 float)
// Fragment order: lane l, element e of K group q of N tile nt holds W[32 nt + (l & 31)][k = 8 q + 4 (l >> 5) + e] with
// k = tap * 64 + input channel.
struct EdLayout {
    int64_t cin, conv0, cout, total;       // conv layer j (0 .. 2B) at conv0 + j * (FRAG_C + 64): frag, then bias
};

EdLayout ed_layout(const stof_edsr_desc* d) {
    EdLayout o{};
    int64_t at = 0;
    o.cin = at; at = align_up(at + 4 * C);
    o.conv0 = at; at += (int64_t)(2 * d->num_blocks + 1) * (FRAG_C + C);
    o.cout = at; at = align_up(at + 3 * (C / d->upscale_factor) + 1);
    o.total = at;
    return o;
}

bool ed_desc_ok(const stof_edsr_desc* d) {
    if (!d || d->num_blocks < 0 || d->num_blocks > MAX_BLOCKS) return false;
    const int r = d->upscale_factor;
    return r >= 1 && r <= 64 && (r & (r - 1)) == 0;
}

int64_t ed_buffer_floats(int64_t N, int64_t L) { return align_up((N * (L + GAP) + GAP) * C); }

// ESPCN blob (floats, 256-byte aligned sections), NT = r <= 32 ? 1 : 2:
//   c1    [6][64]                   rows 0..4 = conv1.weight[c][0][tap], row 5 = conv1.bias
//   frag2 [24][64][4]               conv2, k = tap * 64 + input channel (32 output channels = one N tile)
//   b2    [32] (section of 64)
//   frag3 [NT][12][64][4]           conv3, k = tap * 32 + input channel, output channels >= r are zero
//   b3    [64]                      conv3.bias, zero from r on
struct EsLayout {
    int64_t c1, frag2, b2, frag3, b3, total;
};

int es_nt(const stof_espcn_desc* d) { return d->upscale_factor <= 32 ? 1 : 2; }

EsLayout es_layout(const stof_espcn_desc* d) {
    EsLayout o{};
    int64_t at = 0;
    o.c1 = at; at = align_up(at + 6 * 64);
    o.frag2 = at; at = align_up(at + ES_G2 * 256);
    o.b2 = at; at = align_up(at + 32);
    o.frag3 = at; at = align_up(at + (int64_t)es_nt(d) * ES_G3 * 256);
    o.b3 = at; at = align_up(at + 64);
    o.total = at;
    return o;
}

bool es_desc_ok(const stof_espcn_desc* d) { return d && d->upscale_factor >= 1 && d->upscale_factor <= 64; }

__device__ __forceinline__ float relu(float v) { return v < 0.f ? 0.f : v; }   // keeps NaN (v > 0 ? v : 0 would not)

// ------------------------------------------------------------------------------------------------------------- gaps
__global__ __launch_bounds__(256) void ed_gaps_kernel(float* __restrict__ b0, float* __restrict__ b1, float* __restrict__ b2,
                                                      long long L, long long total) {
    const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // (gap g, gap row, channel)
    if (o >= total) return;
    const long long g = o / (GAP * C), w = o % (GAP * C);
    const long long at = g * (L + GAP) * C + w;
    b0[at] = 0.f;
    b1[at] = 0.f;
    b2[at] = 0.f;
}

// -------------------------------------------------------------------------------------------------------- conv_input
// Thread o: flattened output m = o / 16, channels 4 (o % 16) .. + 3: bias, then taps 0..2 as one fma chain.
__global__ __launch_bounds__(256) void ed_in_kernel(const float* __restrict__ x, long long M, long long L,
                                                    const float* __restrict__ cin, float* __restrict__ out) {
    const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= M * 16) return;
    const long long m = o >> 4, n = m / L, t = m - n * L;
    const int c = 4 * (int)(o & 15);
    const float xv[3] = {t > 0 ? x[m - 1] : 0.f, x[m], t < L - 1 ? x[m + 1] : 0.f};
    float4 acc = *reinterpret_cast<const float4*>(cin + 3 * C + c);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float4 w = *reinterpret_cast<const float4*>(cin + j * C + c);
        acc.x = fmaf(w.x, xv[j], acc.x);
        acc.y = fmaf(w.y, xv[j], acc.y);
        acc.z = fmaf(w.z, xv[j], acc.z);
        acc.w = fmaf(w.w, xv[j], acc.w);
    }
    *reinterpret_cast<float4*>(out + (GAP + n * GAP + m) * C + c) = make_float4(relu(acc.x), relu(acc.y), relu(acc.z), relu(acc.w));
}

// ---------------------------------------------------------------------------------------------------- 64 -> 64 convs
// Wave (blockIdx.x, w) owns flattened outputs m0 .. m0 + 31 (m = n L + t) and N tiles blockIdx.y NTW .. + NTW - 1.  Lane
// (i = l & 31, h = l >> 5) reads rows t - 1 .. t + 1 of its own waveform (the GAP rows supply the padding) at
// k = 8 q + 4 h .. + 3; the next group's operands are loaded before this group's MFMAs.
// C/D map: column (channel) = lane & 31, row (output) = (r & 3) + 8 (r >> 2) + 4 h.
template <int NTW, bool RELU, bool RES>
__global__ __launch_bounds__(256) void ed_conv_kernel(const float* __restrict__ in, unsigned M, unsigned L,
                                                      const float4* __restrict__ frag, const float* __restrict__ bias,
                                                      const float* res, float* out, float* __restrict__ dense) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned m0 = ((unsigned)blockIdx.x * 4 + wave) * 32;
    if (m0 >= M) return;
    const int i = lane & 31, h = lane >> 5;
    unsigned m = m0 + i;
    if (m >= M) m = M - 1;                            // tail lanes compute a duplicate and store nothing
    const unsigned n = m / L;
    const float* a = in + ((long long)GAP + (long long)n * GAP + m - 1) * C + 4 * h;
    const int nt0 = blockIdx.y * NTW;
    const float4* bq = frag + (long long)nt0 * GC * 64 + lane;
    f32x16 acc[NTW] = {};
    mfma32_k_loop<NTW, GC>(a, bq, acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned row = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row >= M) continue;
        const unsigned rn = row / L;
        const long long at = ((long long)GAP + (long long)rn * GAP + row) * C + 32 * nt0 + i;
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) {
            float v = acc[nt][r] + bias[32 * (nt0 + nt) + i];
            if (RES) v += res[at + 32 * nt];
            if (RELU) v = relu(v);
            out[at + 32 * nt] = v;
            if (dense) dense[(long long)row * C + 32 * (nt0 + nt) + i] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------- shuffle + conv_output
// Thread: output sample o = n (L r) + m.  base points at float 0 of waveform n's [L][64] block; the taps read the CQ
// floats at (m + d - 1) CQ (the float before / after the block lies in a zero GAP row).
template <int CQ>
__global__ __launch_bounds__(256) void ed_out_kernel(const float* __restrict__ in, long long total, long long L, long long Lr,
                                                     const float* __restrict__ cout, float* __restrict__ y) {
    const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= total) return;
    const long long n = o / Lr, m = o - n * Lr;
    const float* p = in + (GAP + n * (L + GAP)) * C + (m - 1) * CQ;
    float acc = cout[3 * CQ];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float* pd = p + d * CQ;
        const float* w = cout + d * CQ;
        if constexpr (CQ >= 4) {
#pragma unroll
            for (int c = 0; c < CQ; c += 4) {
                const float4 v = *reinterpret_cast<const float4*>(pd + c);
                acc = fmaf(w[c], v.x, acc);
                acc = fmaf(w[c + 1], v.y, acc);
                acc = fmaf(w[c + 2], v.z, acc);
                acc = fmaf(w[c + 3], v.w, acc);
            }
        } else {
#pragma unroll
            for (int c = 0; c < CQ; ++c) acc = fmaf(w[c], pd[c], acc);
        }
    }
    y[o] = acc;
}

// ------------------------------------------------------------------------------------------------------------- ESPCN
// Work-group blockIdx.x = (row n, tile): samples t0 .. t0 + ES_T - 1.  LDS rows: xs[j] = x[t0 - 4 + j];
// a1 row j = position t0 - 2 + j; a2 row j = position t0 - 1 + j.  Wave w owns a2 rows 32 w .. + 31 in step 3 and
// outputs t0 + 32 w .. + 31 in step 4 (outputs 126, 127 of the tile are computed and dropped; they read a2 rows 128,
// 129, which nothing writes).
template <int NT>
__global__ __launch_bounds__(256) void es_kernel(const float* __restrict__ x, long long L, long long tblocks, int r,
                                                 const float* __restrict__ c1, const float4* __restrict__ frag2,
                                                 const float* __restrict__ b2, const float4* __restrict__ frag3,
                                                 const float* __restrict__ b3, float* __restrict__ y,
                                                 float* __restrict__ logits) {
    __shared__ float xs[ES_XS];
    __shared__ __attribute__((aligned(16))) float a1[ES_ROWS1 * ES_R1];
    __shared__ __attribute__((aligned(16))) float a2[ES_ROWS2 * ES_R2];
    const long long n = blockIdx.x / tblocks, t0 = (long long)(blockIdx.x % tblocks) * ES_T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, h = lane >> 5;
    // 1
    if (tid < ES_XS) {
        const long long t = t0 - 4 + tid;
        xs[tid] = (t >= 0 && t < L) ? x[n * L + t] : 0.f;
    }
    __syncthreads();
    // 2: thread = channel lane of rows wave, wave + 4, ...
    {
        float w[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) w[j] = c1[j * 64 + lane];
        const float b = c1[5 * 64 + lane];
        for (int row = wave; row < ES_ROWS1; row += 4) {
            const long long p = t0 - 2 + row;
            float acc = b;
#pragma unroll
            for (int j = 0; j < 5; ++j) acc = fmaf(w[j], xs[row + j], acc);
            a1[row * ES_R1 + lane] = (p >= 0 && p < L) ? tanhf(acc) : 0.f;
        }
    }
    __syncthreads();
    // 3: a2 row 32 wave + i needs a1 rows 32 wave + i .. + 2
    {
        const float* a = a1 + (32 * wave + i) * ES_R1 + 4 * h;
        const float4* bq = frag2 + lane;
        // Eight accumulators, K group q into accumulator q & 7 (one per 8-channel group, summed over the taps), added up
        // in order at the end: a single chain of 192 products loses about 3 bits more in the trained checkpoints, whose
        // conv2 sums cancel (sum |w| = 156) and whose conv3 amplifies the loss.  The chains are independent MFMAs as well.
        f32x16 acc8[8] = {};
        float4 bv = bq[0];
#pragma unroll
        for (int q = 0; q < ES_G2; ++q) {
            const float4 av = *reinterpret_cast<const float4*>(a + (q >> 3) * ES_R1 + 8 * (q & 7));
            const float4 cb = bv;
            if (q + 1 < ES_G2) bv = bq[(q + 1) * 64];
            acc8[q & 7] = MFMA32(av.x, cb.x, acc8[q & 7]);
            acc8[q & 7] = MFMA32(av.y, cb.y, acc8[q & 7]);
            acc8[q & 7] = MFMA32(av.z, cb.z, acc8[q & 7]);
            acc8[q & 7] = MFMA32(av.w, cb.w, acc8[q & 7]);
        }
        f32x16 acc = acc8[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) acc += acc8[j];
        const float b = b2[i];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = 32 * wave + (e & 3) + 8 * (e >> 2) + 4 * h;
            const long long p = t0 - 1 + row;
            a2[row * ES_R2 + i] = (p >= 0 && p < L) ? tanhf(acc[e] + b) : 0.f;
        }
    }
    __syncthreads();
    // 4: output 32 wave + i needs a2 rows 32 wave + i .. + 2; the logits tile [ES_T][r] goes over a1
    {
        const float* a = a2 + (32 * wave + i) * ES_R2 + 4 * h;
        const float4* bq = frag3 + lane;
        f32x16 acc[NT] = {};
        for (int q = 0; q < ES_G3; ++q) {
            const float4 av = *reinterpret_cast<const float4*>(a + (q >> 2) * ES_R2 + 8 * (q & 3));
            float4 cb[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) cb[nt] = bq[(nt * ES_G3 + q) * 64];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = MFMA32(av.x, cb[nt].x, acc[nt]);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = MFMA32(av.y, cb[nt].y, acc[nt]);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = MFMA32(av.z, cb[nt].z, acc[nt]);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = MFMA32(av.w, cb[nt].w, acc[nt]);
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int j = 32 * nt + i;
            if (j >= r) continue;
            const float b = b3[j];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int u = 32 * wave + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (u < ES_T) a1[u * r + j] = acc[nt][e] + b;
            }
        }
    }
    __syncthreads();
    const long long left = L - t0;
    const int count = (int)(left < ES_T ? left : ES_T) * r;
    const long long at = (n * L + t0) * r;
    for (int k = tid; k < count; k += 256) {
        const float v = a1[k];
        if (logits) logits[at + k] = v;
        y[at + k] = 1.f / (1.f + expf(-v));
    }
}

// -------------------------------------------------------------------------------------------------------- launches
template <int NTW, bool RELU, bool RES>
void launch_conv(dim3 grid, hipStream_t s, const float* in, unsigned M, unsigned L, const float* frag, const float* bias,
                 const float* res, float* out, float* dense) {
    hipLaunchKernelGGL((ed_conv_kernel<NTW, RELU, RES>), grid, dim3(256), 0, s, in, M, L, reinterpret_cast<const float4*>(frag),
                       bias, res, out, dense);
}

template <int CQ>
void launch_out(hipStream_t s, const float* in, long long total, long long L, long long Lr, const float* cout, float* y) {
    hipLaunchKernelGGL(ed_out_kernel<CQ>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, total, L, Lr, cout, y);
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------- EDSR
extern "C" size_t stof_edsr_packed_bytes(const stof_edsr_desc* desc) {
    if (!ed_desc_ok(desc)) return 0;
    return (size_t)ed_layout(desc).total * sizeof(float);
}

extern "C" int stof_edsr_pack_weights(const stof_edsr_desc* desc, const float* const* params, void* out, size_t out_bytes) {
    if (!ed_desc_ok(desc) || !params || !out) return STOF_ERR_BAD_ARG;
    const int B = desc->num_blocks, cq = C / desc->upscale_factor, np = 2 * (2 * B + 3);
    for (int i = 0; i < np; ++i)
        if (!params[i]) return STOF_ERR_BAD_ARG;
    const EdLayout o = ed_layout(desc);
    if (out_bytes < (size_t)o.total * sizeof(float)) return STOF_ERR_WORKSPACE;
    float* const blob = static_cast<float*>(out);
    memset(blob, 0, (size_t)o.total * sizeof(float));
    for (int c = 0; c < C; ++c) {
        for (int j = 0; j < 3; ++j) blob[o.cin + j * C + c] = params[0][c * 3 + j];
        blob[o.cin + 3 * C + c] = params[1][c];
    }
    for (int l = 0; l <= 2 * B; ++l) {                 // params 2 + 2 l, 3 + 2 l: block l / 2 conv1 | conv2, last conv_mid
        float* sec = blob + o.conv0 + (int64_t)l * (FRAG_C + C);
        pack_frag32(params[2 + 2 * l], C, C, 3, C, 2, GC, sec);
        memcpy(sec + FRAG_C, params[3 + 2 * l], sizeof(float) * C);
    }
    const float* wo = params[np - 2];
    for (int c = 0; c < cq; ++c)
        for (int j = 0; j < 3; ++j) blob[o.cout + j * cq + c] = wo[c * 3 + j];
    blob[o.cout + 3 * cq] = params[np - 1][0];
    return STOF_OK;
}

extern "C" size_t stof_edsr_workspace_bytes(const stof_edsr_desc* desc, int64_t N, int64_t L) {
    if (!ed_desc_ok(desc) || N <= 0 || L <= 0) return 0;
    return 3 * (size_t)ed_buffer_floats(N, L) * sizeof(float);
}

extern "C" int stof_edsr_forward(const stof_edsr_desc* desc, const float* x, int64_t N, int64_t L, const void* packed, float* y,
                                 float* trunk, void* workspace, size_t workspace_bytes, void* stream) {
    if (!ed_desc_ok(desc) || !x || !packed || !y || !workspace || N <= 0 || L <= 0) return STOF_ERR_BAD_ARG;
    if (L >= (1ll << 31) || N >= (1ll << 31) || N * L >= (1ll << 31) - 64 || N * (L + GAP) + GAP >= (1ll << 31) - 64)
        return STOF_ERR_UNSUPPORTED;                   // 32-bit m
    const int64_t bf = ed_buffer_floats(N, L);
    if (workspace_bytes < 3 * (size_t)bf * sizeof(float)) return STOF_ERR_WORKSPACE;
    const EdLayout o = ed_layout(desc);
    const float* const blob = static_cast<const float*>(packed);
    float* const first = static_cast<float*>(workspace);
    float* const cur = first + bf;
    float* const tmp = cur + bf;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int B = desc->num_blocks, r = desc->upscale_factor;

    const int64_t gaps = (N + 1) * GAP * C;
    hipLaunchKernelGGL(ed_gaps_kernel, dim3((unsigned)((gaps + 255) / 256)), dim3(256), 0, s, first, cur, tmp, (long long)L,
                       (long long)gaps);
    if (hipGetLastError() != hipSuccess) return STOF_ERR_HIP;
    const int64_t M64 = N * L;
    hipLaunchKernelGGL(ed_in_kernel, dim3((unsigned)((M64 * 16 + 255) / 256)), dim3(256), 0, s, x, (long long)M64, (long long)L,
                       blob + o.cin, first);
    if (hipGetLastError() != hipSuccess) return STOF_ERR_HIP;
    // Small batches: one N tile per wave (2x the waves, each A fragment loaded 2x) so that the GPU fills up.
    const bool narrow = M64 < NARROW_M;
    const unsigned M = (unsigned)M64, Lu = (unsigned)L;
    const dim3 grid((M + 127) / 128, narrow ? 2 : 1);
    const float* src = first;
    for (int b = 0; b < B; ++b) {
        const float* s1 = blob + o.conv0 + (int64_t)(2 * b) * (FRAG_C + C);
        const float* s2 = s1 + FRAG_C + C;
        // tmp = relu(conv1(src)); cur = conv2(tmp) + src (src == cur from block 1 on: in place, the halo comes from tmp)
        if (narrow) launch_conv<1, true, false>(grid, s, src, M, Lu, s1, s1 + FRAG_C, nullptr, tmp, nullptr);
        else launch_conv<2, true, false>(grid, s, src, M, Lu, s1, s1 + FRAG_C, nullptr, tmp, nullptr);
        if (hipGetLastError() != hipSuccess) return STOF_ERR_HIP;
        if (narrow) launch_conv<1, false, true>(grid, s, tmp, M, Lu, s2, s2 + FRAG_C, src, cur, nullptr);
        else launch_conv<2, false, true>(grid, s, tmp, M, Lu, s2, s2 + FRAG_C, src, cur, nullptr);
        if (hipGetLastError() != hipSuccess) return STOF_ERR_HIP;
        src = cur;
    }
    const float* sm = blob + o.conv0 + (int64_t)(2 * B) * (FRAG_C + C);
    if (narrow) launch_conv<1, false, true>(grid, s, src, M, Lu, sm, sm + FRAG_C, first, tmp, trunk);
    else launch_conv<2, false, true>(grid, s, src, M, Lu, sm, sm + FRAG_C, first, tmp, trunk);
    if (hipGetLastError() != hipSuccess) return STOF_ERR_HIP;
    const long long Lr = (long long)L * r, total = (long long)N * Lr;
    const float* co = blob + o.cout;
    switch (C / r) {
        case 64: launch_out<64>(s, tmp, total, L, Lr, co, y); break;
        case 32: launch_out<32>(s, tmp, total, L, Lr, co, y); break;
        case 16: launch_out<16>(s, tmp, total, L, Lr, co, y); break;
        case 8: launch_out<8>(s, tmp, total, L, Lr, co, y); break;
        case 4: launch_out<4>(s, tmp, total, L, Lr, co, y); break;
        case 2: launch_out<2>(s, tmp, total, L, Lr, co, y); break;
        default: launch_out<1>(s, tmp, total, L, Lr, co, y); break;
    }
    return hipGetLastError() == hipSuccess ? STOF_OK : STOF_ERR_HIP;
}

// ------------------------------------------------------------------------------------------------------------ ESPCN
extern "C" size_t stof_espcn_packed_bytes(const stof_espcn_desc* desc) {
    if (!es_desc_ok(desc)) return 0;
    return (size_t)es_layout(desc).total * sizeof(float);
}

extern "C" int stof_espcn_pack_weights(const stof_espcn_desc* desc, const float* const* params, void* out, size_t out_bytes) {
    if (!es_desc_ok(desc) || !params || !out) return STOF_ERR_BAD_ARG;
    for (int i = 0; i < 6; ++i)
        if (!params[i]) return STOF_ERR_BAD_ARG;
    const EsLayout o = es_layout(desc);
    if (out_bytes < (size_t)o.total * sizeof(float)) return STOF_ERR_WORKSPACE;
    float* const blob = static_cast<float*>(out);
    memset(blob, 0, (size_t)o.total * sizeof(float));
    const int r = desc->upscale_factor, nt = es_nt(desc);
    for (int c = 0; c < 64; ++c) {
        for (int j = 0; j < 5; ++j) blob[o.c1 + j * 64 + c] = params[0][c * 5 + j];
        blob[o.c1 + 5 * 64 + c] = params[1][c];
    }
    pack_frag32(params[2], 32, 64, 3, 64, 1, ES_G2, blob + o.frag2);
    memcpy(blob + o.b2, params[3], sizeof(float) * 32);
    pack_frag32(params[4], r, 32, 3, 32, nt, ES_G3, blob + o.frag3);      // output channels >= r are zero
    memcpy(blob + o.b3, params[5], sizeof(float) * r);
    return STOF_OK;
}

extern "C" int stof_espcn_forward(const stof_espcn_desc* desc, const float* x, int64_t N, int64_t L, const void* packed, float* y,
                                  float* logits, void* stream) {
    if (!es_desc_ok(desc) || !x || !packed || !y || N <= 0 || L <= 0) return STOF_ERR_BAD_ARG;
    if (L >= (1ll << 31) || N >= (1ll << 31) || N * L >= (1ll << 31) - 64) return STOF_ERR_UNSUPPORTED;   // grid size
    const EsLayout o = es_layout(desc);
    const float* const blob = static_cast<const float*>(packed);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long tblocks = (L + ES_T - 1) / ES_T;
    const dim3 grid((unsigned)(N * tblocks));
    const float4* f2 = reinterpret_cast<const float4*>(blob + o.frag2);
    const float4* f3 = reinterpret_cast<const float4*>(blob + o.frag3);
    if (es_nt(desc) == 1)
        hipLaunchKernelGGL(es_kernel<1>, grid, dim3(256), 0, s, x, (long long)L, tblocks, (int)desc->upscale_factor, blob + o.c1, f2,
                           blob + o.b2, f3, blob + o.b3, y, logits);
    else
        hipLaunchKernelGGL(es_kernel<2>, grid, dim3(256), 0, s, x, (long long)L, tblocks, (int)desc->upscale_factor, blob + o.c1, f2,
                           blob + o.b2, f3, blob + o.b3, y, logits);
    return hipGetLastError() == hipSuccess ? STOF_OK : STOF_ERR_HIP;
}
