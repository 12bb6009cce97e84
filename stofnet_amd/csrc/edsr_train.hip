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
// conv_input's three kernels are the shared input end of train_ends.h (K = 3, ReLU); the partials of either weight gradient are
// added by partial_reduce_kernel of wgrad_reduce.h.
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
#include "train_ends.h"
#include "wgrad_reduce.h"

namespace {

constexpr int EC = ENDS_C;                  // num_features
constexpr int ET_ROWS = ENDS_TILE;          // rows per work-group of ed_out_dgrad_kernel
constexpr int EW_CHUNK = ENDS_CHUNK;        // rows per chunk of the weight-gradient kernels
constexpr int EW_MAX_COPIES = 1024;         // partials (work-groups) of a weight-gradient launch

inline bool r_ok(int32_t r) { return r >= 1 && r <= 64 && (r & (r - 1)) == 0; }

// conv_input's activation: ReLU; g' = (g + g2) * [saved > 0], g2 the long skip's gradient or NULL
struct Relu {
    static constexpr bool zero_fed_row_ends = true;
    __device__ static float fwd(float v) { return fmaxf(v, 0.f); }
    __device__ static float4 bwd(const float* g, const float* g2, const float* saved, size_t at) {
        float4 v = ld4(g + at);
        if (g2) { const float4 u = ld4(g2 + at); v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w; }
        const float4 s = ld4(saved + at);
        return make_float4(s.x > 0.f ? v.x : 0.f, s.y > 0.f ? v.y : 0.f, s.z > 0.f ? v.z : 0.f, s.w > 0.f ? v.w : 0.f);
    }
};

// ---------------------------------------------------------------------------------------------------- conv_input
__global__ __launch_bounds__(256) void ed_in_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                    float* __restrict__ y, int total, int L) {
    ends_in_fwd<3, Relu>(x, w, b, y, total, L);
}
__global__ __launch_bounds__(256) void ed_in_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                          const float* __restrict__ g2, const float* __restrict__ saved,
                                                          float* __restrict__ copies, int total, int L) {
    ends_in_wgrad<3, Relu>(x, g, g2, saved, copies, total, L);
}
__global__ __launch_bounds__(256) void ed_in_dgrad_kernel(const float* __restrict__ g, const float* __restrict__ g2,
                                                          const float* __restrict__ saved, const float* __restrict__ w,
                                                          float* __restrict__ dx, int total, int L, float out_scale) {
    ends_in_dgrad<3, Relu>(g, g2, saved, w, dx, total, L, out_scale);
}

// Fold of ed_out_wgrad_kernel's work-group: every thread holds 16 sums, [element i of its float4][tap 0..2 | plain sum]; the 16
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

constexpr size_t EW_WORKSPACE = (size_t)EW_MAX_COPIES * 256 * sizeof(float);       // a partial of either weight gradient: <= 256 floats

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
    const int rc = check_rows(N, L, x, w, b, y);
    if (rc != ENDS_GO) return rc;
    const int total = (int)(N * L);
    hipLaunchKernelGGL(ed_in_kernel, dim3((unsigned)((total + ENDS_TILE - 1) / ENDS_TILE)), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                       w, b, y, total, (int)L);
    return launched();
}

extern "C" size_t stof_train_edsr_in_wgrad_workspace_bytes(void) { return EW_WORKSPACE; }

extern "C" int stof_train_edsr_in_wgrad(const float* x, const float* g, const float* g2, const float* saved, float* dw, float* db,
                                        int64_t N, int64_t L, float out_scale, void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = check_wgrad_rows(N, L, dw, EC * 3, db, EC, workspace_bytes, EW_WORKSPACE, s, x, g, saved, workspace);
    if (rc != ENDS_GO) return rc;
    float* copies = static_cast<float*>(workspace);
    const int gx = wgrad_copies(N * L, EW_CHUNK, EW_MAX_COPIES);
    hipLaunchKernelGGL(ed_in_wgrad_kernel, dim3((unsigned)gx), dim3(256), 0, s, x, g, g2, saved, copies, (int)(N * L), (int)L);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    partial_reduce(s, copies, gx, 256, 256, DwThenDb{dw, db, 192}, out_scale);
    return launched();
}

extern "C" int stof_train_edsr_in_dgrad(const float* g, const float* g2, const float* saved, const float* w, float* dx, int64_t N, int64_t L,
                                        float out_scale, void* stream) {
    const int rc = check_rows(N, L, g, saved, w, dx);
    if (rc != ENDS_GO) return rc;
    const int total = (int)(N * L);
    hipLaunchKernelGGL(ed_in_dgrad_kernel, dim3((unsigned)((total + ENDS_DTILE - 1) / ENDS_DTILE)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), g, g2, saved, w, dx, total, (int)L, out_scale);
    return launched();
}

extern "C" int stof_train_edsr_out(const float* trunk, const float* w, const float* b, float* y, int64_t N, int64_t L, int32_t r,
                                   void* stream) {
    if (!r_ok(r)) return STOF_ERR_BAD_ARG;
    const int rc = check_rows(N, L, trunk, w, b, y);
    if (rc != ENDS_GO) return rc;
    const long long total = N * L * r;
    ED_BY_R(ed_out_kernel, r, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), trunk, w, b, y, total,
            (int)(L * r));
    return launched();
}

extern "C" int stof_train_edsr_out_dgrad(const float* dy, const float* w, float* dtrunk, int64_t N, int64_t L, int32_t r, void* stream) {
    if (!r_ok(r)) return STOF_ERR_BAD_ARG;
    const int rc = check_rows(N, L, dy, w, dtrunk);
    if (rc != ENDS_GO) return rc;
    const int total = (int)(N * L);
    ED_BY_R(ed_out_dgrad_kernel, r, dim3((unsigned)((total + ET_ROWS - 1) / ET_ROWS)), dim3(256), 0, static_cast<hipStream_t>(stream), dy, w,
            dtrunk, total, (int)L);
    return launched();
}

extern "C" size_t stof_train_edsr_out_wgrad_workspace_bytes(int32_t r) { return r_ok(r) ? EW_WORKSPACE : 0; }

extern "C" int stof_train_edsr_out_wgrad(const float* trunk, const float* dy, float* dw, float* db, int64_t N, int64_t L, int32_t r,
                                         float out_scale, void* workspace, size_t workspace_bytes, void* stream) {
    if (!r_ok(r)) return STOF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int cq = EC / r;
    const int rc = check_wgrad_rows(N, L, dw, (size_t)cq * 3, db, 1, workspace_bytes, EW_WORKSPACE, s, trunk, dy, workspace);
    if (rc != ENDS_GO) return rc;
    float* copies = static_cast<float*>(workspace);
    const int gx = wgrad_copies(N * L, EW_CHUNK, EW_MAX_COPIES);
    ED_BY_R(ed_out_wgrad_kernel, r, dim3((unsigned)gx), dim3(256), 0, s, trunk, dy, copies, (int)(N * L), (int)L);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    partial_reduce(s, copies, gx, 256, 3 * cq + 1, DwThenDb{dw, db, 3 * cq}, out_scale);
    return launched();
}
