// Training ESPCN_1D(r) (models/espcn_1d.py:31-36), r = 1..64, in exact fp32, one kernel per stage with the activations saved in
// HBM.  Activations are channel-last and un-gapped: h1 [N][L][64], h2 [N][L][32], x / dx [N][L], y / dy [N][L r]; every row
// end is a predicate, so the zero padding of conv2 and conv3 is zeros of h1 and h2 (not tanh(bias)).
//
//   ep_in_kernel          h1 = tanh(conv1(x)), 1 -> 64, k 5                          (vector pipe)
//   pack_frag32_kernel    (mfma32_frag.h) conv2.weight (32,64,3) -> the B-operand fragment image of ep_mid_kernel
//   ep_mid_kernel         h2 = tanh(conv2(h1) + b2), 64 -> 32, k 3                   (v_mfma_f32_32x32x2_f32)
//   ep_out_kernel         y = sigmoid(conv3(h2) + b3), 32 -> r, k 3                  (vector pipe)
//   ep_out_wgrad_kernel   dW3 (r,32,3), db3 (r) from dz = dy y (1 - y) and h2
//   ep_out_dgrad_kernel   g2 [N][L][32] = conv3^T(dz) (1 - h2^2)
//   ep_in_wgrad_kernel    dW1 (64,1,5), db1 (64) from g' = g1 (1 - h1^2) and x
//   ep_in_dgrad_kernel    dx [N][L] = conv1^T(g')
// conv1's three kernels are the shared input end of train_ends.h (K = 5, tanh); the partials of either weight gradient are added
// by partial_reduce_kernel of wgrad_reduce.h.
//
// conv2's two gradient GEMMs are stof_train_wgrad(h1, g2) and stof_train_conv(g2, flipped W2) of train.hip: tanh' of conv2's
// output is already in g2.
//
// The shuffle is free: in channel-last order z [N][L][r] IS the shuffled row [N][L r], one channel survives, so
// y[n][l r + j] = sigmoid(z[n][l][j]).
//
// The rows of all waveforms are one flat sequence of N L rows; a tile of rows may span waveforms, the taps that would cross
// a row end are skipped by t = row % L.  No float atomics: a weight-gradient work-group walks its 256-row chunks in a fixed
// assignment (chunk k -> work-group k mod grid), keeps its sums in registers, folds them through LDS in a fixed order and
// writes ONE partial; the reduce kernel adds the partials in a fixed order.  The order depends on the shape alone, so two
// runs are bitwise equal.  h1, h2, g1, g2 and the fragment image must be 16-byte aligned.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "stof_common.h"
#include "train_ends.h"
#include "wgrad_reduce.h"
#include "mfma32_frag.h"

namespace {

using stof_frag::f32x16;

constexpr int C1 = 64, C2 = 32;             // channels of h1, h2
constexpr int PT_ROWS = ENDS_TILE;          // rows per work-group of ep_out_dgrad_kernel
constexpr int PM_TILE = 128;                // rows per work-group of ep_mid_kernel (4 waves x 32 rows)
constexpr int PM_STRIDE = 68;               // LDS row stride of its h1 tile (floats): 16 lanes of a ds_read_b128 on 16 slots
constexpr int PM_GROUPS = 3 * C1 / 8;       // K groups of conv2: k = tap * 64 + ci, 8 per group
constexpr int PO_OUTS = 2048;               // outputs per work-group of ep_out_kernel (8 passes of 256)
constexpr int PO_WS = 100;                  // LDS stride of one output channel's 96 conv3 weights
constexpr int PW_CHUNK = ENDS_CHUNK;        // rows per chunk of the weight-gradient kernels
constexpr int PW_SUB = 64;                  // rows per LDS stage of ep_out_wgrad_kernel
constexpr int PW_MAX_COPIES = 512;          // partials (work-groups) of a weight-gradient launch
constexpr int PW_IN_E = ends_wgrad_floats<5>();      // floats of a conv1 partial: dw [f * 5 + d], then db [320 + f]

inline bool r_ok(int32_t r) { return r >= 1 && r <= 64; }
__host__ __device__ inline int out_e(int r) { return r * (3 * C2 + 1); }                      // floats of a conv3 partial: dw, then db [r * 96 + j]

// g (1 - s^2): the gradient through tanh, from the saved activation
__device__ inline float4 tanh_bwd(float4 g, float4 s) {
    return make_float4(g.x * fmaf(-s.x, s.x, 1.f), g.y * fmaf(-s.y, s.y, 1.f), g.z * fmaf(-s.z, s.z, 1.f), g.w * fmaf(-s.w, s.w, 1.f));
}

// conv1's activation: tanh; g' = g (1 - saved^2)
struct Tanh {
    static constexpr bool zero_fed_row_ends = false;
    __device__ static float fwd(float v) { return tanhf(v); }
    __device__ static float4 bwd(const float* g, const float*, const float* saved, size_t at) { return tanh_bwd(ld4(g + at), ld4(saved + at)); }
};

// ------------------------------------------------------------------------------------------------------------- conv1
__global__ __launch_bounds__(256) void ep_in_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                    float* __restrict__ h1, int total, int L) {
    ends_in_fwd<5, Tanh>(x, w, b, h1, total, L);
}
__global__ __launch_bounds__(256) void ep_in_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ h1,
                                                          float* __restrict__ copies, int total, int L) {
    ends_in_wgrad<5, Tanh>(x, g, nullptr, h1, copies, total, L);
}
__global__ __launch_bounds__(256) void ep_in_dgrad_kernel(const float* __restrict__ g, const float* __restrict__ h1, const float* __restrict__ w,
                                                          float* __restrict__ dx, int total, int L, float out_scale) {
    ends_in_dgrad<5, Tanh>(g, nullptr, h1, w, dx, total, L, out_scale);
}

// ------------------------------------------------------------------------------------------------------------- conv2
// conv2.weight in torch layout (32,64,3) is packed by pack_frag32_kernel of mfma32_frag.h: one N tile of [24 K groups][64 lanes][4]
// with k = tap * 64 + ci.
// A work-group stages flat rows r0 - 1 .. r0 + PM_TILE of h1 in LDS (row j = flat row r0 - 1 + j, zero outside the buffer) and
// wave w computes rows r0 + 32 w .. + 31: the A operand of lane (i, h) is the float4 at channel 8 (q & 7) + 4 h of row i + tap,
// zeroed where that tap crosses the end of row i's waveform; the 32 output channels are the one N tile.  Eight accumulators,
// K group q into accumulator q & 7 (one per 8-channel group, summed over the taps), added up in order at the end: as in
// es_kernel of riders.hip, a single chain of 192 products loses about 3 bits more in the trained checkpoints.
__global__ __launch_bounds__(256) void ep_mid_kernel(const float* __restrict__ h1, const float4* __restrict__ frag2,
                                                     const float* __restrict__ b2, float* __restrict__ h2, int total, int L) {
    __shared__ __attribute__((aligned(16))) float a1[(PM_TILE + 2) * PM_STRIDE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int r0 = blockIdx.x * PM_TILE;
    for (int k = tid; k < (PM_TILE + 2) * 16; k += 256) {
        const int j = k >> 4, c4 = k & 15;
        const int row = r0 - 1 + j;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row >= 0 && row < total) v = ld4(h1 + (size_t)row * C1 + 4 * c4);
        *reinterpret_cast<float4*>(a1 + j * PM_STRIDE + 4 * c4) = v;
    }
    __syncthreads();
    if (r0 + 32 * wave >= total) return;
    const int m = 32 * wave + i;
    const int t = (r0 + m) % L;
    const bool ok0 = t > 0, ok2 = t < L - 1;
    const float* a = a1 + m * PM_STRIDE + 4 * h;
    const float4* bq = frag2 + lane;
    f32x16 acc8[8] = {};
    float4 bv = bq[0];
#pragma unroll
    for (int q = 0; q < PM_GROUPS; ++q) {
        const int tap = q >> 3;
        float4 av = *reinterpret_cast<const float4*>(a + tap * PM_STRIDE + 8 * (q & 7));
        if ((tap == 0 && !ok0) || (tap == 2 && !ok2)) av = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 cb = bv;
        if (q + 1 < PM_GROUPS) bv = bq[(q + 1) * 64];
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
        const int row = r0 + 32 * wave + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (row < total) h2[(size_t)row * C2 + i] = tanhf(acc[e] + b);
    }
}

// ------------------------------------------------------------------------------------------------------------- conv3
// Thread: output o = row r + j.  The r x 96 weights go through LDS as [j][tap][c]; bias, then taps 0..2 over channels 0..31 as
// one fmaf chain (a tap that leaves the waveform is skipped), then the sigmoid as es_kernel computes it.
__global__ __launch_bounds__(256) void ep_out_kernel(const float* __restrict__ h2, const float* __restrict__ w, const float* __restrict__ b,
                                                     float* __restrict__ y, int total_out, int L, int r) {
    __shared__ __attribute__((aligned(16))) float ws[64 * PO_WS];
    const int tid = threadIdx.x;
    for (int k = tid; k < r * 3 * C2; k += 256) {
        const int j = k / (3 * C2), rem = k - j * (3 * C2), c = rem / 3, tap = rem - 3 * c;
        ws[j * PO_WS + tap * C2 + c] = w[k];
    }
    __syncthreads();
    const long long o0 = (long long)blockIdx.x * PO_OUTS + tid;
    for (int it = 0; it < PO_OUTS / 256; ++it) {
        const long long o = o0 + 256 * it;
        if (o >= total_out) break;
        const int row = (int)(o / r), j = (int)(o - (long long)row * r), t = row % L;
        const float* wj = ws + j * PO_WS;
        float acc = b[j];
#pragma unroll
        for (int tap = 0; tap < 3; ++tap) {
            if ((tap == 0 && t == 0) || (tap == 2 && t == L - 1)) continue;
            const float* p = h2 + ((long long)row + tap - 1) * C2;
#pragma unroll
            for (int c = 0; c < C2; c += 4) {
                const float4 v = ld4(p + c), u = *reinterpret_cast<const float4*>(wj + tap * C2 + c);
                acc = fmaf(u.x, v.x, acc);
                acc = fmaf(u.y, v.y, acc);
                acc = fmaf(u.z, v.z, acc);
                acc = fmaf(u.w, v.w, acc);
            }
        }
        y[o] = 1.f / (1.f + expf(-acc));
    }
}

// g2[row][c] = (1 - h2[row][c]^2) sum_tap sum_j w[j][c][tap] dz[row - tap + 1][j], dz = dy y (1 - y), the terms outside the
// waveform dropped.  A work-group takes PT_ROWS rows: the weights go through LDS as [tap][j][c], the dz tile with its one-row
// halos as [row][r | 1]; thread = (row slot tid >> 3, channels 4 c4 .. + 3), two rows per thread.  Per tap one fmaf chain over
// j = 0 .. r - 1, the three taps' sums added in the order 1, 0, 2.
__global__ __launch_bounds__(256) void ep_out_dgrad_kernel(const float* __restrict__ y, const float* __restrict__ dy,
                                                           const float* __restrict__ h2, const float* __restrict__ w,
                                                           float* __restrict__ g2, int total, int L, int r) {
    __shared__ __attribute__((aligned(16))) float wt[3 * 64 * C2];
    __shared__ float dzs[(PT_ROWS + 2) * 65];
    const int tid = threadIdx.x, c4 = tid & 7, slot = tid >> 3;
    const int r0 = blockIdx.x * PT_ROWS, rs = r | 1;
    for (int k = tid; k < r * 3 * C2; k += 256) {
        const int j = k / (3 * C2), rem = k - j * (3 * C2), c = rem / 3, tap = rem - 3 * c;
        wt[(tap * 64 + j) * C2 + c] = w[k];
    }
    for (int k = tid; k < (PT_ROWS + 2) * r; k += 256) {
        const int lr = k / r, j = k - lr * r;
        const long long row = (long long)r0 - 1 + lr;
        float v = 0.f;
        if (row >= 0 && row < total) {
            const float yv = y[row * r + j];
            v = dy[row * r + j] * yv * (1.f - yv);
        }
        dzs[lr * rs + j] = v;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < PT_ROWS / 32; ++it) {
        const int lr = slot + 32 * it, row = r0 + lr;
        if (row >= total) break;
        const int t = row % L;
        float s[3][4];
#pragma unroll
        for (int tap = 0; tap < 3; ++tap) {
#pragma unroll
            for (int i = 0; i < 4; ++i) s[tap][i] = 0.f;
            if ((tap == 0 && t == L - 1) || (tap == 2 && t == 0)) continue;       // tap 0 meets row + 1, tap 2 row - 1
            const float* dz = dzs + (lr + 2 - tap) * rs;                          // LDS row of flat row `row - tap + 1`
            const float* wp = wt + tap * 64 * C2 + 4 * c4;
            for (int j = 0; j < r; ++j) {
                const float4 u = *reinterpret_cast<const float4*>(wp + j * C2);
                const float d = dz[j];
                s[tap][0] = fmaf(u.x, d, s[tap][0]);
                s[tap][1] = fmaf(u.y, d, s[tap][1]);
                s[tap][2] = fmaf(u.z, d, s[tap][2]);
                s[tap][3] = fmaf(u.w, d, s[tap][3]);
            }
        }
        const size_t at = (size_t)row * C2 + 4 * c4;
        const float4 g = make_float4((s[1][0] + s[0][0]) + s[2][0], (s[1][1] + s[0][1]) + s[2][1], (s[1][2] + s[0][2]) + s[2][2],
                                     (s[1][3] + s[0][3]) + s[2][3]);
        *reinterpret_cast<float4*>(g2 + at) = tanh_bwd(g, ld4(h2 + at));
    }
}

// dw[j][c][tap] = sum_rows dz[row][j] h2[row + tap - 1][c], db[j] = sum_rows dz[row][j].  A chunk goes through LDS in four
// stages of PW_SUB rows (h2 with one-row halos, dz as [row][r | 1]).  Thread = (channels 4 c4 .. + 3, j slot, row part):
// with JS = min(32, r rounded up to a power of two) j slots the 32 thread groups split into P = 32 / JS row parts, part p
// taking rows p, p + P, ... of a stage; a thread serves j = slot and slot + 32.  The P parts are added in order through LDS.
__global__ __launch_bounds__(256) void ep_out_wgrad_kernel(const float* __restrict__ h2, const float* __restrict__ y,
                                                           const float* __restrict__ dy, float* __restrict__ copies, int total, int L,
                                                           int r, int js_log2) {
    __shared__ __attribute__((aligned(16))) float hs[(PW_SUB + 2) * C2];
    __shared__ float dzs[PW_SUB * 65];
    __shared__ float red[256 * 27];
    const int tid = threadIdx.x, c4 = tid & 7, grp = tid >> 3;
    const int JS = 1 << js_log2, P = 32 >> js_log2, jslot = grp & (JS - 1), part = grp >> js_log2;
    const int j0 = jslot, j1 = jslot + 32, rs = r | 1;
    const bool act0 = j0 < r, act1 = j1 < r;
    float acc[2][4][3], sb[2] = {0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int d = 0; d < 3; ++d) acc[a][i][d] = 0.f;
    for (long long c0 = (long long)blockIdx.x * PW_CHUNK; c0 < total; c0 += (long long)gridDim.x * PW_CHUNK) {
        for (int sub = 0; sub < PW_CHUNK / PW_SUB; ++sub) {
            const int s0 = (int)c0 + PW_SUB * sub;
            if (s0 >= total) break;
            __syncthreads();
            for (int k = tid; k < (PW_SUB + 2) * 8; k += 256) {
                const int row = s0 - 1 + (k >> 3);
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row >= 0 && row < total) v = ld4(h2 + (size_t)row * C2 + 4 * (k & 7));
                *reinterpret_cast<float4*>(hs + 4 * k) = v;
            }
            for (int k = tid; k < PW_SUB * r; k += 256) {
                const int lr = k / r, j = k - lr * r;
                float v = 0.f;
                if (s0 + lr < total) {
                    const long long at = (long long)s0 * r + k;
                    const float yv = y[at];
                    v = dy[at] * yv * (1.f - yv);
                }
                dzs[lr * rs + j] = v;
            }
            __syncthreads();
            int t = (s0 + part) % L;
            for (int lr = part; lr < PW_SUB; lr += P) {
                if (s0 + lr >= total) break;
                const float d[2] = {act0 ? dzs[lr * rs + j0] : 0.f, act1 ? dzs[lr * rs + j1] : 0.f};
                const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 hm = t > 0 ? *reinterpret_cast<const float4*>(hs + lr * C2 + 4 * c4) : z4;
                const float4 hc = *reinterpret_cast<const float4*>(hs + (lr + 1) * C2 + 4 * c4);
                const float4 hp = t < L - 1 ? *reinterpret_cast<const float4*>(hs + (lr + 2) * C2 + 4 * c4) : z4;
                const float hv[3][4] = {{hm.x, hm.y, hm.z, hm.w}, {hc.x, hc.y, hc.z, hc.w}, {hp.x, hp.y, hp.z, hp.w}};
#pragma unroll
                for (int a = 0; a < 2; ++a) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int k = 0; k < 3; ++k) acc[a][i][k] = fmaf(d[a], hv[k][i], acc[a][i][k]);
                    sb[a] += d[a];
                }
                t += P;
                if (t >= L) t %= L;
            }
        }
    }
    __syncthreads();
    float* mine = red + tid * 27;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) mine[a * 13 + i * 3 + k] = acc[a][i][k];
        mine[a * 13 + 12] = sb[a];
    }
    __syncthreads();
    if (part != 0) return;
    float* copy = copies + (size_t)blockIdx.x * out_e(r);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int j = a ? j1 : j0;
        if (j >= r) continue;
        for (int e = 0; e < 13; ++e) {
            float s = mine[a * 13 + e];
            for (int p = 1; p < P; ++p) s += red[(tid + p * JS * 8) * 27 + a * 13 + e];
            if (e < 12) copy[(j * C2 + 4 * c4 + e / 3) * 3 + e % 3] = s;
            else if (c4 == 0) copy[r * 3 * C2 + j] = s;
        }
    }
}

constexpr size_t PW_IN_WORKSPACE = (size_t)PW_MAX_COPIES * PW_IN_E * sizeof(float);
inline size_t out_workspace(int r) { return (size_t)PW_MAX_COPIES * out_e(r) * sizeof(float); }

}  // namespace

extern "C" size_t stof_train_espcn_repack_floats(void) { return (size_t)PM_GROUPS * 256; }

extern "C" int stof_train_espcn_repack(const float* w2, float* out, void* stream) {
    if (!w2 || !out) return STOF_ERR_BAD_ARG;
    stof_frag::pack_frag32_device(static_cast<hipStream_t>(stream), w2, 32, C1, 3, C1, PM_GROUPS, out, PM_GROUPS * 256);
    return launched();
}

extern "C" int stof_train_espcn_in(const float* x, const float* w, const float* b, float* h1, int64_t N, int64_t L, void* stream) {
    const int rc = check_rows(N, L, x, w, b, h1);
    if (rc != ENDS_GO) return rc;
    const int total = (int)(N * L);
    hipLaunchKernelGGL(ep_in_kernel, dim3((unsigned)((total + ENDS_TILE - 1) / ENDS_TILE)), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                       w, b, h1, total, (int)L);
    return launched();
}

extern "C" int stof_train_espcn_mid(const float* h1, const float* frag2, const float* b2, float* h2, int64_t N, int64_t L, void* stream) {
    const int rc = check_rows(N, L, h1, frag2, b2, h2);
    if (rc != ENDS_GO) return rc;
    const int total = (int)(N * L);
    hipLaunchKernelGGL(ep_mid_kernel, dim3((unsigned)((total + PM_TILE - 1) / PM_TILE)), dim3(256), 0, static_cast<hipStream_t>(stream), h1,
                       reinterpret_cast<const float4*>(frag2), b2, h2, total, (int)L);
    return launched();
}

extern "C" int stof_train_espcn_out(const float* h2, const float* w, const float* b, float* y, int64_t N, int64_t L, int32_t r,
                                    void* stream) {
    if (!r_ok(r)) return STOF_ERR_BAD_ARG;
    const int rc = check_rows(N, L, h2, w, b, y);
    if (rc != ENDS_GO) return rc;
    const long long total = N * L * r;
    hipLaunchKernelGGL(ep_out_kernel, dim3((unsigned)((total + PO_OUTS - 1) / PO_OUTS)), dim3(256), 0, static_cast<hipStream_t>(stream), h2, w,
                       b, y, (int)total, (int)L, (int)r);
    return launched();
}

extern "C" size_t stof_train_espcn_out_wgrad_workspace_bytes(int32_t r) { return r_ok(r) ? out_workspace(r) : 0; }

extern "C" int stof_train_espcn_out_wgrad(const float* h2, const float* y, const float* dy, float* dw, float* db, int64_t N, int64_t L,
                                          int32_t r, float out_scale, void* workspace, size_t workspace_bytes, void* stream) {
    if (!r_ok(r)) return STOF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = check_wgrad_rows(N, L, dw, (size_t)r * C2 * 3, db, (size_t)r, workspace_bytes, out_workspace(r), s, h2, y, dy, workspace);
    if (rc != ENDS_GO) return rc;
    float* copies = static_cast<float*>(workspace);
    const int gx = wgrad_copies(N * L, PW_CHUNK, PW_MAX_COPIES);
    int js_log2 = 0;
    while ((1 << js_log2) < r && js_log2 < 5) ++js_log2;
    hipLaunchKernelGGL(ep_out_wgrad_kernel, dim3((unsigned)gx), dim3(256), 0, s, h2, y, dy, copies, (int)(N * L), (int)L, (int)r, js_log2);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    const int E = out_e(r);
    partial_reduce(s, copies, gx, E, E, DwThenDb{dw, db, r * 3 * C2}, out_scale);
    return launched();
}

extern "C" int stof_train_espcn_out_dgrad(const float* y, const float* dy, const float* h2, const float* w, float* g2, int64_t N, int64_t L,
                                          int32_t r, void* stream) {
    if (!r_ok(r)) return STOF_ERR_BAD_ARG;
    const int rc = check_rows(N, L, y, dy, h2, w, g2);
    if (rc != ENDS_GO) return rc;
    const int total = (int)(N * L);
    hipLaunchKernelGGL(ep_out_dgrad_kernel, dim3((unsigned)((total + PT_ROWS - 1) / PT_ROWS)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       y, dy, h2, w, g2, total, (int)L, (int)r);
    return launched();
}

extern "C" size_t stof_train_espcn_in_wgrad_workspace_bytes(void) { return PW_IN_WORKSPACE; }

extern "C" int stof_train_espcn_in_wgrad(const float* x, const float* g1, const float* h1, float* dw, float* db, int64_t N, int64_t L,
                                         float out_scale, void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = check_wgrad_rows(N, L, dw, C1 * 5, db, C1, workspace_bytes, PW_IN_WORKSPACE, s, x, g1, h1, workspace);
    if (rc != ENDS_GO) return rc;
    float* copies = static_cast<float*>(workspace);
    const int gx = wgrad_copies(N * L, PW_CHUNK, PW_MAX_COPIES);
    hipLaunchKernelGGL(ep_in_wgrad_kernel, dim3((unsigned)gx), dim3(256), 0, s, x, g1, h1, copies, (int)(N * L), (int)L);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    partial_reduce(s, copies, gx, PW_IN_E, PW_IN_E, DwThenDb{dw, db, C1 * 5}, out_scale);
    return launched();
}

extern "C" int stof_train_espcn_in_dgrad(const float* g1, const float* h1, const float* w, float* dx, int64_t N, int64_t L, float out_scale,
                                         void* stream) {
    const int rc = check_rows(N, L, g1, h1, w, dx);
    if (rc != ENDS_GO) return rc;
    const int total = (int)(N * L);
    hipLaunchKernelGGL(ep_in_dgrad_kernel, dim3((unsigned)((total + ENDS_DTILE - 1) / ENDS_DTILE)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), g1, h1, w, dx, total, (int)L, out_scale);
    return launched();
}
