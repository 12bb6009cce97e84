// StofNet at any width (models/stofnet.py:11,23: num_features F = 1..256, in_channels Cin = 1..16): the pieces of the
// training path that train.hip has for 1 -> 64 channels only, on the vector pipe in exact fp32:
//
//   conv1_c          relu(conv1(x)): x NCL [N][Cin][L] as the module receives it -> channel-last [N][L][F]
//   conv1_c_wgrad    dw[F][Cin][9], db[F] from g' = g * relu'(saved), fixed-order partials, no float atomics
//   conv1_c_dgrad    dx[N][Cin][L] = conv1^T(g'), written in NCL
//   upsample_bwd_c   SemiGlobalBlock: backward of nearest upsample + pad + add for rows of C channels
//
// The shipped geometry (F = 64, Cin = 1) never reaches them: it keeps the kernels of train.hip.  Every sum has one fixed
// order per output element that depends on the shape alone, never on the launch geometry.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "stof_common.h"
#include "stof_hip_util.h"
#include "wgrad_reduce.h"

namespace {

constexpr int WC_MAX_CIN = 16, WC_MAX_F = 256;
constexpr int WC_ROWS = 64;               // time rows per work-group (forward, dgrad)
constexpr int WC_XS = WC_ROWS + 8;        // staged input window per input channel
constexpr int WC_CT = 64;                 // output channels per work-group
constexpr int WC_PAD = WC_CT + 1;         // LDS row stride of [k][channel] arrays: lanes along channels or along k, no conflicts

inline unsigned blocks_for(long long n) { return (unsigned)((n + 255) / 256); }

// conv1 (Cin -> F, k9, pad 4) + ReLU.  A work-group takes 64 rows of one waveform and 64 output channels: the Cin x 72 input
// window and the tile's Cin x 9 x 64 weights go through LDS once; thread = (channel ch = tid & 63, wave = 16 consecutive rows).
// Per input channel a thread holds its 9 weights and the wave's 24-sample window in registers (the window is wave-uniform:
// broadcast reads) for 144 FMAs.  Chain of one output: bias, then input channels in order, taps 0..8 within each.
__global__ __launch_bounds__(256) void conv1_c_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ b, float* __restrict__ y, int L, int Cin, int F,
                                                          int tiles) {
    __shared__ float ws[WC_MAX_CIN * 9 * WC_PAD];                 // [c * 9 + d][channel]
    __shared__ __attribute__((aligned(16))) float xs[WC_MAX_CIN * WC_XS];
    __shared__ float bs[WC_CT];
    const int tid = threadIdx.x, ch = tid & 63, part = tid >> 6;
    const int f0 = blockIdx.y * WC_CT, K9 = Cin * 9;
    const long long n = blockIdx.x / tiles;
    const int t0 = (int)(blockIdx.x - n * tiles) * WC_ROWS;
    for (int i = tid; i < WC_CT * K9; i += 256) {
        const int cl = i / K9, k = i - cl * K9;
        ws[k * WC_PAD + cl] = f0 + cl < F ? w[(size_t)(f0 + cl) * K9 + k] : 0.f;
    }
    if (tid < WC_CT) bs[tid] = f0 + tid < F ? b[f0 + tid] : 0.f;
    for (int i = tid; i < Cin * WC_XS; i += 256) {
        const int c = i / WC_XS, u = t0 + (i - c * WC_XS) - 4;
        xs[i] = (u >= 0 && u < L) ? x[((size_t)n * Cin + c) * L + u] : 0.f;
    }
    __syncthreads();
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = bs[ch];
    for (int c = 0; c < Cin; ++c) {
        float wr[9], xv[24];
#pragma unroll
        for (int d = 0; d < 9; ++d) wr[d] = ws[(c * 9 + d) * WC_PAD + ch];
#pragma unroll
        for (int i = 0; i < 24; ++i) xv[i] = xs[c * WC_XS + part * 16 + i];
#pragma unroll
        for (int j = 0; j < 16; ++j)
#pragma unroll
            for (int d = 0; d < 9; ++d) acc[j] = fmaf(wr[d], xv[j + d], acc[j]);
    }
    if (f0 + ch >= F) return;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int t = t0 + part * 16 + j;
        if (t < L) y[((size_t)n * L + t) * F + f0 + ch] = fmaxf(acc[j], 0.f);
    }
}

// dw[f][c][d] = sum_rows g'[row][f] x[c][t + d - 4], db[f] = sum_rows g'[row][f], g' = g * relu'(saved conv1 output).
// As conv1_wgrad_kernel (train.hip): grid.x work-groups walk the 256-row chunks in a fixed assignment (chunk k -> work-group
// k mod grid.x), keep their sums in registers and write ONE partial each; grid.y = 64-channel tile of F, grid.z = group of CG
// input channels (the sums of CG x 9 taps + the bias fit the register file; g and saved are read once per group).  The row,
// hence its input samples, is wave-uniform.
constexpr int WC_CHUNK = 256;
template <int CG>
__global__ __launch_bounds__(256) void conv1_c_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                            const float* __restrict__ saved, float* __restrict__ copies, int N, int L,
                                                            int Cin, int F) {
    constexpr int NA = CG * 9 + 1;
    __shared__ float red[4][64][NA];
    const int tid = threadIdx.x, ch = tid & 63, part = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int f = blockIdx.y * WC_CT + ch, c0 = blockIdx.z * CG;
    const bool live = f < F;
    const long long total = (long long)N * L;                   // <= 2^31: checked by the caller
    float acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.f;
    for (long long r0 = (long long)blockIdx.x * WC_CHUNK; r0 < total; r0 += (long long)gridDim.x * WC_CHUNK) {
        const long long rend = r0 + WC_CHUNK < total ? r0 + WC_CHUNK : total;
        int t = (int)((r0 + part) % L);
        for (long long r = r0 + part; r < rend; r += 4) {
            const float* xr = x + (size_t)(r - t) * Cin;          // the waveform's [Cin][L] block
            const float gl = live ? g[(size_t)r * F + f] : 0.f, sl = live ? saved[(size_t)r * F + f] : 0.f;
            const float gv = sl > 0.f ? gl : 0.f;
            const bool inside = t >= 4 && t < L - 4;              // (scalar: all nine samples inside the waveform)
#pragma unroll
            for (int cc = 0; cc < CG; ++cc) {
                if (c0 + cc >= Cin) break;
                const float* xc = xr + (size_t)(c0 + cc) * L;
                float xv[9];
                if (inside) {
#pragma unroll
                    for (int d = 0; d < 9; ++d) xv[d] = xc[t + d - 4];
                } else {
#pragma unroll
                    for (int d = 0; d < 9; ++d) { const int u = t + d - 4; xv[d] = (u >= 0 && u < L) ? xc[u] : 0.f; }
                }
#pragma unroll
                for (int d = 0; d < 9; ++d) acc[cc * 9 + d] = fmaf(gv, xv[d], acc[cc * 9 + d]);
            }
            acc[NA - 1] += gv;
            t += 4;
            while (t >= L) t -= L;                                // (L < 4: more than one wrap)
        }
    }
#pragma unroll
    for (int k = 0; k < NA; ++k) red[part][ch][k] = acc[k];
    __syncthreads();
    if (part != 0 || !live) return;
    float* copy = copies + (size_t)blockIdx.x * F * Cin * 10;   // partial: [f][c][9 taps | bias sum (c = 0 only)]
#pragma unroll
    for (int cc = 0; cc < CG; ++cc) {
        if (c0 + cc >= Cin) break;
#pragma unroll
        for (int d = 0; d < 9; ++d) {
            const int k = cc * 9 + d;
            copy[((size_t)f * Cin + c0 + cc) * 10 + d] = (red[0][ch][k] + red[1][ch][k]) + (red[2][ch][k] + red[3][ch][k]);
        }
    }
    if (c0 == 0) copy[(size_t)f * Cin * 10 + 9] = (red[0][ch][NA - 1] + red[1][ch][NA - 1]) + (red[2][ch][NA - 1] + red[3][ch][NA - 1]);
}

// dx[n][c][u] = out_scale * sum_f sum_d w[f][c][d] g'[n][u + 4 - d][f].  A work-group takes 64 samples of one waveform and walks
// F in tiles of 64 channels: the masked 72 x 64 tile of g' and the tile's weights go through LDS; thread = (sample u = tid & 63,
// wave cg: input channels cg, cg + 4, ..): per f it reads its nine g' values once for all its channels, the weights are
// wave-uniform broadcasts.  One output: per tile a chain over f in order, taps 0..8 within each; the tiles' sums added in order.
// Off the hot path (nobody trains the input).
__global__ __launch_bounds__(256) void conv1_c_dgrad_kernel(const float* __restrict__ g, const float* __restrict__ saved,
                                                            const float* __restrict__ w, float* __restrict__ dx, int L, int Cin, int F,
                                                            int tiles, float out_scale) {
    __shared__ float gs[WC_XS * WC_PAD];                          // [row t0 - 4 + k][channel]
    __shared__ float wt[WC_MAX_CIN * 9 * WC_CT];                  // [c * 9 + d][channel]
    const int tid = threadIdx.x, u = tid & 63, cg = tid >> 6, K9 = Cin * 9;
    const long long n = blockIdx.x / tiles;
    const int t0 = (int)(blockIdx.x - n * tiles) * WC_ROWS;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int f0 = 0; f0 < F; f0 += WC_CT) {
        if (f0) __syncthreads();
        for (int i = tid; i < WC_XS * WC_CT; i += 256) {
            const int k = i >> 6, fl = i & 63, t = t0 - 4 + k;
            float v = 0.f;
            if (t >= 0 && t < L && f0 + fl < F) {
                const size_t idx = ((size_t)n * L + t) * F + f0 + fl;
                v = saved[idx] > 0.f ? g[idx] : 0.f;
            }
            gs[k * WC_PAD + fl] = v;
        }
        for (int i = tid; i < K9 * WC_CT; i += 256) {
            const int cd = i >> 6, fl = i & 63;
            wt[i] = f0 + fl < F ? w[(size_t)(f0 + fl) * K9 + cd] : 0.f;
        }
        __syncthreads();
        const int fn = F - f0 < WC_CT ? F - f0 : WC_CT;
        float part[4] = {0.f, 0.f, 0.f, 0.f};                     // this tile's sum: chains of 9 x 64 terms, not 9 x F
        for (int fl = 0; fl < fn; ++fl) {
            float gv[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) gv[k] = gs[(u + k) * WC_PAD + fl];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = cg + 4 * q;
                if (c >= Cin) break;
#pragma unroll
                for (int d = 0; d < 9; ++d) part[q] = fmaf(wt[(c * 9 + d) * WC_CT + fl], gv[8 - d], part[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += part[q];
    }
    const int t = t0 + u;
    if (t >= L) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = cg + 4 * q;
        if (c < Cin) dx[((size_t)n * Cin + c) * L + t] = acc[q] * out_scale;
    }
}

// ge[n][w][ch] = lrelu'(e) * sum_{k < S} g[n][rem_half + w S + k][ch] for rows of C channels (upsample_bwd_kernel of train.hip
// is the 64-channel form; upsample_add_c_kernel is the forward twin).  One thread per element, lanes along the channels; the
// window is walked as four interleaved chains (k mod 4) that are combined in a fixed order.
__global__ __launch_bounds__(256) void upsample_bwd_c_kernel(const float* __restrict__ g, const float* __restrict__ e,
                                                             float* __restrict__ ge, long long total, int L, int P, int rem_half, int S, int C) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;        // (n, w, ch)
    if (i >= total) return;
    const int ch = (int)(i % C);
    const long long nw = i / C;
    const int w = (int)(nw % P);
    const long long n = nw / P;
    const float* src = g + (n * L + rem_half + (long long)w * S) * C + ch;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    int k = 0;
    for (; k + 3 < S; k += 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] += src[(long long)(k + j) * C];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (k + j < S) s[j] += src[(long long)(k + j) * C];
    const float sum = (s[0] + s[1]) + (s[2] + s[3]);
    ge[i] = e[i] > 0.f ? sum : 0.01f * sum;
}

inline bool widths_ok(int32_t Cin, int32_t F) { return Cin >= 1 && Cin <= WC_MAX_CIN && F >= 1 && F <= WC_MAX_F; }
inline int wgrad_cgroup(int32_t Cin) { return Cin == 1 ? 1 : Cin == 2 ? 2 : 4; }
// partials of the weight gradient: ~2048 work-groups over the whole launch, at least 32 per (channel tile, channel group)
inline int wgrad_copies(int32_t Cin, int32_t F) {
    const int cg = wgrad_cgroup(Cin);
    const int c = 2048 / (((F + WC_CT - 1) / WC_CT) * ((Cin + cg - 1) / cg));
    return c < 32 ? 32 : c;
}

}  // namespace

extern "C" int stof_train_conv1_c(const float* x, const float* w, const float* b, float* y, int64_t N, int32_t Cin, int64_t L, int32_t F,
                                  void* stream) {
    if (N < 0 || L < 0 || !widths_ok(Cin, F)) return STOF_ERR_BAD_ARG;
    if (N == 0 || L == 0) return STOF_OK;
    if (!x || !w || !b || !y) return STOF_ERR_BAD_ARG;
    if (N * L > 0x7fffffffLL) return STOF_ERR_UNSUPPORTED;
    const int tiles = (int)((L + WC_ROWS - 1) / WC_ROWS);
    hipLaunchKernelGGL(conv1_c_fwd_kernel, dim3((unsigned)(N * tiles), (unsigned)((F + WC_CT - 1) / WC_CT)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, w, b, y, (int)L, Cin, F, tiles);
    return hipGetLastError() == hipSuccess ? STOF_OK : STOF_ERR_HIP;
}

extern "C" size_t stof_train_conv1_c_wgrad_workspace_bytes(int32_t Cin, int32_t F) {
    if (!widths_ok(Cin, F)) return 0;
    return (size_t)wgrad_copies(Cin, F) * F * Cin * 10 * sizeof(float);
}

extern "C" int stof_train_conv1_c_wgrad(const float* x, const float* g, const float* saved, float* dw, float* db, int64_t N, int32_t Cin,
                                        int64_t L, int32_t F, float out_scale, void* workspace, size_t workspace_bytes, void* stream) {
    if (N < 0 || L < 0 || !widths_ok(Cin, F)) return STOF_ERR_BAD_ARG;
    if (!dw || !db) return STOF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (N == 0 || L == 0) {
        if (hipMemsetAsync(dw, 0, (size_t)F * Cin * 9 * sizeof(float), s) != hipSuccess ||
            hipMemsetAsync(db, 0, (size_t)F * sizeof(float), s) != hipSuccess) return STOF_ERR_HIP;
        return STOF_OK;
    }
    if (!x || !g || !saved || !workspace) return STOF_ERR_BAD_ARG;
    if (workspace_bytes < stof_train_conv1_c_wgrad_workspace_bytes(Cin, F)) return STOF_ERR_WORKSPACE;
    if (N * L > 0x7fffffffLL) return STOF_ERR_UNSUPPORTED;
    float* copies = static_cast<float*>(workspace);
    const int64_t chunks = (N * L + WC_CHUNK - 1) / WC_CHUNK;
    const int ncopies = wgrad_copies(Cin, F);
    const int gx = (int)(chunks < ncopies ? chunks : ncopies);
    const int cg = wgrad_cgroup(Cin);
    const dim3 grid((unsigned)gx, (unsigned)((F + WC_CT - 1) / WC_CT), (unsigned)((Cin + cg - 1) / cg));
    if (cg == 1) hipLaunchKernelGGL(conv1_c_wgrad_kernel<1>, grid, dim3(256), 0, s, x, g, saved, copies, (int)N, (int)L, Cin, F);
    else if (cg == 2) hipLaunchKernelGGL(conv1_c_wgrad_kernel<2>, grid, dim3(256), 0, s, x, g, saved, copies, (int)N, (int)L, Cin, F);
    else hipLaunchKernelGGL(conv1_c_wgrad_kernel<4>, grid, dim3(256), 0, s, x, g, saved, copies, (int)N, (int)L, Cin, F);
    const int E = F * Cin * 10;                                   // the sums (f, c, d) over the partials
    partial_reduce(s, copies, gx, E, E, TapsThenBiasPerInput{dw, db, Cin}, out_scale);
    return hipGetLastError() == hipSuccess ? STOF_OK : STOF_ERR_HIP;
}

extern "C" int stof_train_conv1_c_dgrad(const float* g, const float* saved, const float* w, float* dx, int64_t N, int32_t Cin, int64_t L,
                                        int32_t F, float out_scale, void* stream) {
    if (N < 0 || L < 0 || !widths_ok(Cin, F)) return STOF_ERR_BAD_ARG;
    if (N == 0 || L == 0) return STOF_OK;
    if (!g || !saved || !w || !dx) return STOF_ERR_BAD_ARG;
    if (N * L > 0x7fffffffLL) return STOF_ERR_UNSUPPORTED;
    const int tiles = (int)((L + WC_ROWS - 1) / WC_ROWS);
    hipLaunchKernelGGL(conv1_c_dgrad_kernel, dim3((unsigned)(N * tiles)), dim3(256), 0, static_cast<hipStream_t>(stream), g, saved, w, dx,
                       (int)L, Cin, F, tiles, out_scale);
    return hipGetLastError() == hipSuccess ? STOF_OK : STOF_ERR_HIP;
}

extern "C" int stof_train_upsample_bwd_c(const float* g, const float* e, float* ge, int64_t N, int64_t L, int64_t P, int32_t rem_half,
                                         int32_t scale, int32_t C, void* stream) {
    if (N < 0 || L < 0 || P < 0 || C < 1 || scale < 1 || rem_half < 0 || rem_half + P * scale > L) return STOF_ERR_BAD_ARG;
    if (N * P == 0) return STOF_OK;
    if (!g || !e || !ge) return STOF_ERR_BAD_ARG;
    if (N * L > 0x7fffffffLL) return STOF_ERR_UNSUPPORTED;
    const long long total = (long long)N * P * C;
    if (total > 0x7fffffffLL * 256) return STOF_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(upsample_bwd_c_kernel, dim3(blocks_for(total)), dim3(256), 0, static_cast<hipStream_t>(stream), g, e, ge, total, (int)L,
                       (int)P, rem_half, scale, C);
    return hipGetLastError() == hipSuccess ? STOF_OK : STOF_ERR_HIP;
}
