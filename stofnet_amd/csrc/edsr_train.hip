// Training EDSR_1D(1, 64, B, r | 64) (models/edsr_1d.py:22-45): the two ends of the network that the channel-last layer
// kernels of train.hip (stof_train_conv / stof_train_wgrad serve the 2 B + 1 body convolutions 64 -> 64, k 3) do not cover,
// on the vector pipe in exact fp32.  Activations are channel-last [N][L][64], un-gapped; every row end is a predicate.
//
//   ed_in_kernel          relu(conv_input(x)): x [N][L] -> a0 [N][L][64]
//   ed_in_wgrad_kernel    dw (64,1,3), db (64) from g' = (g + g2) * [saved > 0]      (g2 = the long skip's gradient, or NULL)
//   ed_in_dgrad_kernel    dx [N][L] = conv_input^T(g')
//   ed_out_kernel         y [N][L r] = conv_output(SampleShuffle1D(r)(trunk))
//   ed_out_dgrad_kernel   dtrunk [N][L][64] = shuffle^T(conv_output^T(dy))
//   ed_out_wgrad_kernel   dw (1,64/r,3), db (1)
//   ed_wgrad_reduce_kernel  the fixed-order sum over the partials of either weight gradient
//
// The shuffle is free in this layout: with C = 64 / r, the C channels of shuffled sample m of waveform n are the floats
// (n L r + m) C .. + C - 1 of the trunk buffer (S[c][w r + k] = trunk[w][k C + c], utils/sample_shuffle.py:24-27).  So with
// M = n L r + m the flat index of an output sample, conv_output reads trunk[(M + d - 1) C + c] for tap d, and element e of the
// trunk buffer belongs to sample M = e / C, channel c = e % C.
//
// Both [N][L][64] streams are walked 16 bytes per lane: a row is 16 lanes, a wave four rows (1 KiB per wave instruction).
// No float atomics: a weight-gradient work-group walks its 256-row chunks in a fixed assignment (chunk k -> work-group
// k mod grid), keeps its sums in registers, folds them through LDS in a fixed order and writes ONE partial; the reduce kernel
// adds the partials in a fixed order.  The order depends on the shape alone, so two runs are bitwise equal.
// All [N][L][64] operands must be 16-byte aligned.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "stof_common.h"

namespace {

constexpr int EC = 64;                      // num_features
constexpr int ET_ROWS = 64;                 // rows per work-group of the element-wise kernels (4 passes of 16 rows)
constexpr int EW_CHUNK = 256;               // rows per chunk of the weight-gradient kernels (16 passes of 16 rows)
constexpr int EW_MAX_COPIES = 1024;         // partials (work-groups) of a weight-gradient launch
constexpr int ED_TILE = 256;                // outputs per work-group of ed_in_dgrad_kernel
constexpr int64_t E_MAX_ROWS = (1ll << 25) - 1;      // N L 64 stays below 2^31

inline bool r_ok(int32_t r) { return r >= 1 && r <= 64 && (r & (r - 1)) == 0; }
// N L within the range of the 32-bit indices (N, L >= 1)
inline bool rows_ok(int64_t N, int64_t L) { return N <= E_MAX_ROWS / L; }

__device__ inline float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ inline float4 masked_sum(const float* g, const float* g2, const float* saved, size_t at) {
    float4 v = ld4(g + at);
    if (g2) { const float4 u = ld4(g2 + at); v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w; }
    const float4 s = ld4(saved + at);
    return make_float4(s.x > 0.f ? v.x : 0.f, s.y > 0.f ? v.y : 0.f, s.z > 0.f ? v.z : 0.f, s.w > 0.f ? v.w : 0.f);
}

// ---------------------------------------------------------------------------------------------------- conv_input
// Thread = (row slot tid >> 4, channels 4 q .. 4 q + 3): its twelve weights and four biases stay in registers for the four
// rows it writes.  One output: bias, then taps 0..2 as one fmaf chain.
__global__ __launch_bounds__(256) void ed_in_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                    float* __restrict__ y, int total, int L) {
    const int q = threadIdx.x & 15, slot = threadIdx.x >> 4;
    float wr[4][3], br[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        br[i] = b[4 * q + i];
#pragma unroll
        for (int d = 0; d < 3; ++d) wr[i][d] = w[(4 * q + i) * 3 + d];
    }
    const int r0 = blockIdx.x * ET_ROWS + slot;
    if (r0 >= total) return;
    int t = r0 % L;
#pragma unroll
    for (int it = 0; it < ET_ROWS / 16; ++it) {
        const int row = r0 + 16 * it;
        if (row >= total) break;
        const float xm = t > 0 ? x[row - 1] : 0.f, x0 = x[row], xp = t < L - 1 ? x[row + 1] : 0.f;
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = fmaxf(fmaf(wr[i][2], xp, fmaf(wr[i][1], x0, fmaf(wr[i][0], xm, br[i]))), 0.f);
        *reinterpret_cast<float4*>(y + (size_t)row * EC + 4 * q) = make_float4(o[0], o[1], o[2], o[3]);
        t += 16;
        if (t >= L) t %= L;
    }
}

// Fold of a weight-gradient work-group: every thread holds 16 sums, [element i of its float4][tap 0..2 | plain sum]; the 16
// row slots are added pairwise in a fixed order -> fold[pos 0..63][4], pos = 4 q + i the float's position in its 64-float row.
__device__ inline void fold_slots(float (&acc)[16], float* red, float* fold) {
    const int tid = threadIdx.x, q = tid & 15, slot = tid >> 4;
#pragma unroll
    for (int j = 0; j < 16; j += 4)
        *reinterpret_cast<float4*>(red + slot * 256 + q * 16 + j) = make_float4(acc[j], acc[j + 1], acc[j + 2], acc[j + 3]);
    __syncthreads();
    float s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        s[k] = (red[(4 * k) * 256 + tid] + red[(4 * k + 1) * 256 + tid]) + (red[(4 * k + 2) * 256 + tid] + red[(4 * k + 3) * 256 + tid]);
    fold[tid] = (s[0] + s[1]) + (s[2] + s[3]);
    __syncthreads();
}

// dw[f][d] = sum_rows g'[row][f] x[t + d - 1], db[f] = sum_rows g'[row][f].  Partial: [f * 3 + d] (192), then [192 + f].
__global__ __launch_bounds__(256) void ed_in_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                          const float* __restrict__ g2, const float* __restrict__ saved,
                                                          float* __restrict__ copies, int total, int L) {
    __shared__ __attribute__((aligned(16))) float red[16 * 256];
    __shared__ float fold[256];
    const int tid = threadIdx.x, q = tid & 15, slot = tid >> 4;
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    for (long long c0 = (long long)blockIdx.x * EW_CHUNK; c0 < total; c0 += (long long)gridDim.x * EW_CHUNK) {
        const int r0 = (int)c0 + slot;
        int t = r0 % L;
#pragma unroll 4
        for (int it = 0; it < EW_CHUNK / 16; ++it) {
            const int row = r0 + 16 * it;
            if (row >= total) break;
            const float4 v = masked_sum(g, g2, saved, (size_t)row * EC + 4 * q);
            const float xm = t > 0 ? x[row - 1] : 0.f, x0 = x[row], xp = t < L - 1 ? x[row + 1] : 0.f;
            const float gv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc[4 * i] = fmaf(gv[i], xm, acc[4 * i]);
                acc[4 * i + 1] = fmaf(gv[i], x0, acc[4 * i + 1]);
                acc[4 * i + 2] = fmaf(gv[i], xp, acc[4 * i + 2]);
                acc[4 * i + 3] += gv[i];
            }
            t += 16;
            if (t >= L) t %= L;
        }
    }
    fold_slots(acc, red, fold);
    const int f = tid >> 2, d = tid & 3;
    copies[(size_t)blockIdx.x * 256 + (d < 3 ? f * 3 + d : 192 + f)] = fold[tid];
}

// out[e] = out_scale * sum over the `ncopies` partials of E floats, element e < ndw -> dw[e], else db[e - ndw]: 64 elements x
// 16 interleaved slices of the copies per work-group, four chains per slice, combined through LDS in a fixed order
// (conv1_c_wgrad_reduce_kernel of widths.hip).
__global__ __launch_bounds__(1024) void ed_wgrad_reduce_kernel(const float* __restrict__ copies, int ncopies, int stride, int E, int ndw,
                                                               float* __restrict__ dw, float* __restrict__ db, float out_scale) {
    __shared__ float red[16][64];
    const int e = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + e;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    if (i < E) {
        int k = sl;
        for (; k + 48 < ncopies; k += 64) {
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] += copies[(size_t)(k + 16 * j) * stride + i];
        }
        for (; k < ncopies; k += 16) a[0] += copies[(size_t)k * stride + i];
    }
    red[sl][e] = (a[0] + a[1]) + (a[2] + a[3]);
    __syncthreads();
    if (sl != 0 || i >= E) return;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; k += 4) s += (red[k][e] + red[k + 1][e]) + (red[k + 2][e] + red[k + 3][e]);
    if (i < ndw) dw[i] = s * out_scale; else db[i - ndw] = s * out_scale;
}

// dx[row] = out_scale * (p1[row] + p0[row + 1] + p2[row - 1]) with p_d[row] = sum_f w[f][d] g'[row][f] (row ends: the neighbour's
// term drops).  A work-group takes ED_TILE outputs: the 16 lanes of a row each form their four channels' share of the three
// dot products, a fixed xor butterfly over the 16 lanes adds them, the 258 x 3 sums go through LDS.
__global__ __launch_bounds__(256) void ed_in_dgrad_kernel(const float* __restrict__ g, const float* __restrict__ g2,
                                                          const float* __restrict__ saved, const float* __restrict__ w,
                                                          float* __restrict__ dx, int total, int L, float out_scale) {
    __shared__ float ps[3][ED_TILE + 2 + 14];              // [tap][row r0 - 1 + j], j < 258 (272 = 17 passes of 16 rows)
    const int tid = threadIdx.x, q = tid & 15, slot = tid >> 4;
    float wr[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int d = 0; d < 3; ++d) wr[i][d] = w[(4 * q + i) * 3 + d];
    const long long r0 = (long long)blockIdx.x * ED_TILE;
    for (int j = slot; j < ED_TILE + 2 + 14; j += 16) {      // (every lane of a wave stays in the loop: the butterfly needs all 16)
        const long long row = r0 - 1 + j;
        float p[3] = {0.f, 0.f, 0.f};
        if (j < ED_TILE + 2 && row >= 0 && row < total) {
            const float4 v = masked_sum(g, g2, saved, (size_t)row * EC + 4 * q);
            const float gv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int d = 0; d < 3; ++d)
#pragma unroll
                for (int i = 0; i < 4; ++i) p[d] = fmaf(wr[i][d], gv[i], p[d]);
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) p[d] += __shfl_xor(p[d], m, 16);
        }
        if (q == 0) { ps[0][j] = p[0]; ps[1][j] = p[1]; ps[2][j] = p[2]; }
    }
    __syncthreads();
    const long long row = r0 + tid;
    if (row >= total) return;
    const int t = (int)(row % L), j = tid + 1;
    float s = ps[1][j];
    if (t < L - 1) s += ps[0][j + 1];
    if (t > 0) s += ps[2][j - 1];
    dx[row] = s * out_scale;
}

// --------------------------------------------------------------------------------------- shuffle + conv_output
// Thread: output sample M = n (L r) + m.  ed_out_kernel of riders.hip on an un-gapped buffer: bias, then taps d = 0..2 over
// channels c = 0..CQ-1 as one fmaf chain; the taps that leave the waveform (m = 0: d = 0; m = L r - 1: d = 2) are skipped,
// which is what their zero rows contribute there.
template <int CQ>
__global__ __launch_bounds__(256) void ed_out_kernel(const float* __restrict__ trunk, const float* __restrict__ w, const float* __restrict__ b,
                                                     float* __restrict__ y, long long total, int Lr) {
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int m = (int)(o % Lr);
    const float* p = trunk + (o - 1) * CQ;
    float acc = b[0];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        if ((d == 0 && m == 0) || (d == 2 && m == Lr - 1)) continue;
        const float* pd = p + d * CQ;
        if constexpr (CQ >= 4) {
#pragma unroll
            for (int c = 0; c < CQ; c += 4) {
                const float4 v = ld4(pd + c);
                acc = fmaf(w[c * 3 + d], v.x, acc);
                acc = fmaf(w[(c + 1) * 3 + d], v.y, acc);
                acc = fmaf(w[(c + 2) * 3 + d], v.z, acc);
                acc = fmaf(w[(c + 3) * 3 + d], v.w, acc);
            }
        } else {
#pragma unroll
            for (int c = 0; c < CQ; ++c) acc = fmaf(w[c * 3 + d], pd[c], acc);
        }
    }
    y[o] = acc;
}

// Element e of the trunk buffer is channel c = e % CQ of sample M = e / CQ: dtrunk[e] = sum_k w[c][k] dy[M - k + 1], a chain
// over k = 0..2 that skips the taps outside the waveform.  Thread = (row slot, float4 q of the row), four rows per thread.
template <int CQ>
__global__ __launch_bounds__(256) void ed_out_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                           float* __restrict__ dtrunk, int total, int L) {
    constexpr int R = EC / CQ;
    const int q = threadIdx.x & 15, slot = threadIdx.x >> 4;
    float wr[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) wr[i][k] = w[((4 * q + i) % CQ) * 3 + k];
    const int r0 = blockIdx.x * ET_ROWS + slot;
    if (r0 >= total) return;
    int t = r0 % L;
#pragma unroll
    for (int it = 0; it < ET_ROWS / 16; ++it) {
        const int row = r0 + 16 * it;
        if (row >= total) break;
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = (4 * q + i) / CQ;                           // sample t R + j of the waveform
            const long long M = (long long)row * R + j;
            const bool first = t == 0 && j == 0, last = t == L - 1 && j == R - 1;
            float a = last ? 0.f : wr[i][0] * dy[M + 1];
            a = fmaf(wr[i][1], dy[M], a);
            if (!first) a = fmaf(wr[i][2], dy[M - 1], a);
            o[i] = a;
        }
        *reinterpret_cast<float4*>(dtrunk + (size_t)row * EC + 4 * q) = make_float4(o[0], o[1], o[2], o[3]);
        t += 16;
        if (t >= L) t %= L;
    }
}

// dw[c][k] = sum_M dy[M] S[M + k - 1][c], db = sum_M dy[M]: trunk element e (sample M' = e / CQ, channel c) meets
// dy[M' - k + 1] for tap k, so the trunk is read once, 16 bytes per lane; the dy values are cached neighbours.  A thread's four
// floats keep their channels over all rows.  Partial: [c * 3 + k] (3 CQ), then the bias sum.
template <int CQ>
__global__ __launch_bounds__(256) void ed_out_wgrad_kernel(const float* __restrict__ trunk, const float* __restrict__ dy,
                                                           float* __restrict__ copies, int total, int L) {
    constexpr int R = EC / CQ;
    __shared__ __attribute__((aligned(16))) float red[16 * 256];
    __shared__ float fold[256];
    const int tid = threadIdx.x, q = tid & 15, slot = tid >> 4;
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    for (long long c0 = (long long)blockIdx.x * EW_CHUNK; c0 < total; c0 += (long long)gridDim.x * EW_CHUNK) {
        const int r0 = (int)c0 + slot;
        int t = r0 % L;
#pragma unroll 4
        for (int it = 0; it < EW_CHUNK / 16; ++it) {
            const int row = r0 + 16 * it;
            if (row >= total) break;
            const float4 v = ld4(trunk + (size_t)row * EC + 4 * q);
            const float sv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = (4 * q + i) / CQ;
                const long long M = (long long)row * R + j;
                const bool first = t == 0 && j == 0, last = t == L - 1 && j == R - 1;
                const float d0 = dy[M];
                const float dp = last ? 0.f : dy[M + 1], dm = first ? 0.f : dy[M - 1];
                acc[4 * i] = fmaf(sv[i], dp, acc[4 * i]);             // tap 0: output M' + 1
                acc[4 * i + 1] = fmaf(sv[i], d0, acc[4 * i + 1]);
                acc[4 * i + 2] = fmaf(sv[i], dm, acc[4 * i + 2]);     // tap 2: output M' - 1
                if ((4 * q + i) % CQ == 0) acc[4 * i + 3] += d0;      // every dy once: at channel 0 of its sample
            }
            t += 16;
            if (t >= L) t %= L;
        }
    }
    fold_slots(acc, red, fold);
    float* copy = copies + (size_t)blockIdx.x * 256;
    if (tid < 3 * CQ) {                                               // the R positions that hold channel c, in order
        const int c = tid / 3, k = tid - 3 * c;
        float s = 0.f;
        for (int j = 0; j < R; ++j) s += fold[(j * CQ + c) * 4 + k];
        copy[tid] = s;
    } else if (tid == 3 * CQ) {
        float s = 0.f;
        for (int j = 0; j < R; ++j) s += fold[(j * CQ) * 4 + 3];
        copy[tid] = s;
    }
}

inline int wgrad_copies(int64_t rows) {
    const int64_t chunks = (rows + EW_CHUNK - 1) / EW_CHUNK;
    return (int)(chunks < EW_MAX_COPIES ? chunks : EW_MAX_COPIES);
}
constexpr size_t EW_WORKSPACE = (size_t)EW_MAX_COPIES * 256 * sizeof(float);

inline int launched() { return hipGetLastError() == hipSuccess ? STOF_OK : STOF_ERR_HIP; }

#define ED_BY_R(KERNEL, r, ...)                                                          \
    switch (r) {                                                                         \
        case 1: hipLaunchKernelGGL(KERNEL<64>, __VA_ARGS__); break;                      \
        case 2: hipLaunchKernelGGL(KERNEL<32>, __VA_ARGS__); break;                      \
        case 4: hipLaunchKernelGGL(KERNEL<16>, __VA_ARGS__); break;                      \
        case 8: hipLaunchKernelGGL(KERNEL<8>, __VA_ARGS__); break;                       \
        case 16: hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__); break;                      \
        case 32: hipLaunchKernelGGL(KERNEL<2>, __VA_ARGS__); break;                      \
        default: hipLaunchKernelGGL(KERNEL<1>, __VA_ARGS__); break;                      \
    }

}  // namespace

extern "C" int stof_train_edsr_in(const float* x, const float* w, const float* b, float* y, int64_t N, int64_t L, void* stream) {
    if (N < 0 || L < 0) return STOF_ERR_BAD_ARG;
    if (N == 0 || L == 0) return STOF_OK;
    if (!x || !w || !b || !y) return STOF_ERR_BAD_ARG;
    if (!rows_ok(N, L)) return STOF_ERR_UNSUPPORTED;
    const int total = (int)(N * L);
    hipLaunchKernelGGL(ed_in_kernel, dim3((unsigned)((total + ET_ROWS - 1) / ET_ROWS)), dim3(256), 0, static_cast<hipStream_t>(stream), x, w,
                       b, y, total, (int)L);
    return launched();
}

extern "C" size_t stof_train_edsr_in_wgrad_workspace_bytes(void) { return EW_WORKSPACE; }

extern "C" int stof_train_edsr_in_wgrad(const float* x, const float* g, const float* g2, const float* saved, float* dw, float* db,
                                        int64_t N, int64_t L, float out_scale, void* workspace, size_t workspace_bytes, void* stream) {
    if (N < 0 || L < 0 || !dw || !db) return STOF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (N == 0 || L == 0) {
        if (hipMemsetAsync(dw, 0, EC * 3 * sizeof(float), s) != hipSuccess || hipMemsetAsync(db, 0, EC * sizeof(float), s) != hipSuccess)
            return STOF_ERR_HIP;
        return STOF_OK;
    }
    if (!x || !g || !saved || !workspace) return STOF_ERR_BAD_ARG;
    if (workspace_bytes < EW_WORKSPACE) return STOF_ERR_WORKSPACE;
    if (!rows_ok(N, L)) return STOF_ERR_UNSUPPORTED;
    float* copies = static_cast<float*>(workspace);
    const int gx = wgrad_copies(N * L);
    hipLaunchKernelGGL(ed_in_wgrad_kernel, dim3((unsigned)gx), dim3(256), 0, s, x, g, g2, saved, copies, (int)(N * L), (int)L);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    hipLaunchKernelGGL(ed_wgrad_reduce_kernel, dim3(4), dim3(1024), 0, s, copies, gx, 256, 256, 192, dw, db, out_scale);
    return launched();
}

extern "C" int stof_train_edsr_in_dgrad(const float* g, const float* g2, const float* saved, const float* w, float* dx, int64_t N, int64_t L,
                                        float out_scale, void* stream) {
    if (N < 0 || L < 0) return STOF_ERR_BAD_ARG;
    if (N == 0 || L == 0) return STOF_OK;
    if (!g || !saved || !w || !dx) return STOF_ERR_BAD_ARG;
    if (!rows_ok(N, L)) return STOF_ERR_UNSUPPORTED;
    const int total = (int)(N * L);
    hipLaunchKernelGGL(ed_in_dgrad_kernel, dim3((unsigned)((total + ED_TILE - 1) / ED_TILE)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       g, g2, saved, w, dx, total, (int)L, out_scale);
    return launched();
}

extern "C" int stof_train_edsr_out(const float* trunk, const float* w, const float* b, float* y, int64_t N, int64_t L, int32_t r,
                                   void* stream) {
    if (N < 0 || L < 0 || !r_ok(r)) return STOF_ERR_BAD_ARG;
    if (N == 0 || L == 0) return STOF_OK;
    if (!trunk || !w || !b || !y) return STOF_ERR_BAD_ARG;
    if (!rows_ok(N, L)) return STOF_ERR_UNSUPPORTED;
    const long long total = N * L * r;
    ED_BY_R(ed_out_kernel, r, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), trunk, w, b, y, total,
            (int)(L * r));
    return launched();
}

extern "C" int stof_train_edsr_out_dgrad(const float* dy, const float* w, float* dtrunk, int64_t N, int64_t L, int32_t r, void* stream) {
    if (N < 0 || L < 0 || !r_ok(r)) return STOF_ERR_BAD_ARG;
    if (N == 0 || L == 0) return STOF_OK;
    if (!dy || !w || !dtrunk) return STOF_ERR_BAD_ARG;
    if (!rows_ok(N, L)) return STOF_ERR_UNSUPPORTED;
    const int total = (int)(N * L);
    ED_BY_R(ed_out_dgrad_kernel, r, dim3((unsigned)((total + ET_ROWS - 1) / ET_ROWS)), dim3(256), 0, static_cast<hipStream_t>(stream), dy, w,
            dtrunk, total, (int)L);
    return launched();
}

extern "C" size_t stof_train_edsr_out_wgrad_workspace_bytes(int32_t r) { return r_ok(r) ? EW_WORKSPACE : 0; }

extern "C" int stof_train_edsr_out_wgrad(const float* trunk, const float* dy, float* dw, float* db, int64_t N, int64_t L, int32_t r,
                                         float out_scale, void* workspace, size_t workspace_bytes, void* stream) {
    if (N < 0 || L < 0 || !r_ok(r) || !dw || !db) return STOF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int cq = EC / r;
    if (N == 0 || L == 0) {
        if (hipMemsetAsync(dw, 0, (size_t)cq * 3 * sizeof(float), s) != hipSuccess || hipMemsetAsync(db, 0, sizeof(float), s) != hipSuccess)
            return STOF_ERR_HIP;
        return STOF_OK;
    }
    if (!trunk || !dy || !workspace) return STOF_ERR_BAD_ARG;
    if (workspace_bytes < EW_WORKSPACE) return STOF_ERR_WORKSPACE;
    if (!rows_ok(N, L)) return STOF_ERR_UNSUPPORTED;
    float* copies = static_cast<float*>(workspace);
    const int gx = wgrad_copies(N * L);
    ED_BY_R(ed_out_wgrad_kernel, r, dim3((unsigned)gx), dim3(256), 0, s, trunk, dy, copies, (int)(N * L), (int)L);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    hipLaunchKernelGGL(ed_wgrad_reduce_kernel, dim3((unsigned)((3 * cq + 1 + 63) / 64)), dim3(1024), 0, s, copies, gx, 256, 3 * cq + 1, 3 * cq,
                       dw, db, out_scale);
    return launched();
}
