// What the Wave-U-Net inference kernels (waveunet.hip) and its training kernels (waveunet_train.hip) share: the geometry
// constants, the fp32 interpolation coordinates and the window of their transpose, the virtual input of a convolution
// (decimated | interpolated + concatenated | plain), the encoder-0, implicit-GEMM and head kernels with their epilogues,
// and the fragment order of the B operand.  The layout of activations and of the fragment images is documented in
// waveunet.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

constexpr int CI = 16;                     // channels_interval
constexpr int MAX_LAYERS = 12;
constexpr int TM = 64;                     // positions per work-group of wu_conv_kernel
constexpr int CHUNK = 192;                 // channels per LDS pass
constexpr int ENC_TAPS = 15, DEC_TAPS = 5;

// the A source of a convolution: what window position u, channel c of waveform n holds
constexpr int SRC_DECIMATED = 0;           // prev[n][2 u][c], prev [N, 2 Lout, Cin]
constexpr int SRC_DECODER = 1;             // c < Cu: the x2 interpolation of low [N, Lout / 2, Cu]; else skip[n][u][c - Cu]
constexpr int SRC_PLAIN = 2;               // src[n][u][c], src [N, Lout, Cin]

inline int wu_ntw(int tiles) {
    if (tiles <= 4) return tiles;
    return (tiles % 4 == 0 || tiles % 3 != 0) ? 4 : 3;
}

__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : 0.1f * v; }   // NaN takes the second arm and stays

// ATen's fp32 source coordinates of the x2 linear interpolation with align_corners.  Contraction is off here: r has to be
// the rounded product before i0 is subtracted (an fma would subtract from the exact one and move l1 by up to an ulp of r).
__host__ __device__ __forceinline__ void wu_coords(float scale, int u, int M, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
    const float r = scale * (float)u;
    i0 = (int)r;
    if (i0 > M - 1) i0 = M - 1;
    i1 = i0 + 1 < M ? i0 + 1 : M - 1;
    l1 = r - (float)i0;
    l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
    l0 = 1.f - l1;
}

inline float wu_scale(long long M) { return (float)(M - 1) / (float)(2 * M - 1); }

// The transpose of the interpolation: the high positions u whose i0(u) or i1(u) can be the low position m lie in
// [lo, hi].  In exact arithmetic r(u) = u (M - 1) / (2 M - 1), so i0(u) = m needs u in [2 m, 2 m + 3] and i1(u) = m needs
// i0(u) = m - 1 (or the clamp at M - 1), u in [2 m - 2, 2 m + 1]; the fp32 rounding of scale and of the product moves r
// by less than 1/4 for M <= 2^21, i.e. u by less than one, which the window adds on either side.
constexpr long long WU_INTERP_MAX_M = 1ll << 21;
__host__ __device__ __forceinline__ void wu_interp_window(int m, int M, int& lo, int& hi) {
    lo = 2 * m - 3 < 0 ? 0 : 2 * m - 3;
    hi = 2 * m + 4 > 2 * M - 1 ? 2 * M - 1 : 2 * m + 4;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define MFMA16(a, b, acc) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (acc), 0, 0, 0)

// --------------------------------------------------------------------------------------------------------- encoder 0
// Thread o: flattened position m = o / 4 (m = n L + t), channels 4 (o % 4) .. + 3.  w: rows 0 .. 14 = [tap][c], row 15 =
// the bias.  ACT: LeakyReLU (inference, on the folded weights); without it the raw sum is stored (training: z).
template <bool ACT>
__global__ __launch_bounds__(256) void wu_in_kernel(const float* __restrict__ x, long long M, long long L,
                                                    const float* __restrict__ w, float* __restrict__ out) {
    const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= M * 4) return;
    const long long m = o >> 2, t = m % L;
    const int c = 4 * (int)(o & 3);
    float4 acc = *reinterpret_cast<const float4*>(w + 15 * CI + c);
#pragma unroll
    for (int j = 0; j < ENC_TAPS; ++j) {
        const long long u = t + j - 7;
        const float xv = (u >= 0 && u < L) ? x[m + j - 7] : 0.f;
        const float4 wv = *reinterpret_cast<const float4*>(w + j * CI + c);
        acc.x = fmaf(wv.x, xv, acc.x);
        acc.y = fmaf(wv.y, xv, acc.y);
        acc.z = fmaf(wv.z, xv, acc.z);
        acc.w = fmaf(wv.w, xv, acc.w);
    }
    if constexpr (ACT) acc = make_float4(leaky(acc.x), leaky(acc.y), leaky(acc.z), leaky(acc.w));
    *reinterpret_cast<float4*>(out + m * CI + c) = acc;
}

// ------------------------------------------------------------------------------------------------- implicit-GEMM convs
struct WuConvArgs {
    const float* src;                      // decimated: the previous level [N, 2 Lout, Cin]; decoder: the skip [N, Lout, Cin - Cu];
                                           // plain: [N, Lout, Cin]
    const float* low;                      // decoder: the map to interpolate [N, Lout / 2, Cu]
    const float4* frag;
    const float* bias;                     // may be null without ACT (no bias: the data gradients)
    float* out;                            // [N, Lout, Cout]
    long long Lout;
    int tiles;                             // work-groups per waveform
    int Cin, Cu, Cout, groups;
    float scale;                           // decoder: float(M - 1) / float(2 M - 1), M = Lout / 2
};

// channels c .. c + 3 of position u (inside [0, Lout)) of waveform n of the virtual input
template <int SRC>
__device__ __forceinline__ float4 wu_source(const WuConvArgs& a, long long n, long long u, int c) {
    const long long Lout = a.Lout;
    if constexpr (SRC == SRC_DECIMATED) {
        return *reinterpret_cast<const float4*>(a.src + (n * 2 * Lout + 2 * u) * a.Cin + c);
    } else if constexpr (SRC == SRC_PLAIN) {
        return *reinterpret_cast<const float4*>(a.src + (n * Lout + u) * a.Cin + c);
    } else {
        if (c < a.Cu) {
            const long long M = Lout >> 1;
            int i0, i1;
            float l0, l1;
            wu_coords(a.scale, (int)u, (int)M, i0, i1, l0, l1);
            const float4 p0 = *reinterpret_cast<const float4*>(a.low + (n * M + i0) * a.Cu + c);
            const float4 p1 = *reinterpret_cast<const float4*>(a.low + (n * M + i1) * a.Cu + c);
            return make_float4(l0 * p0.x + l1 * p1.x, l0 * p0.y + l1 * p1.y, l0 * p0.z + l1 * p1.z, l0 * p0.w + l1 * p1.w);
        }
        const int Cs = a.Cin - a.Cu;
        return *reinterpret_cast<const float4*>(a.src + (n * Lout + u) * Cs + (c - a.Cu));
    }
}

// LDS window: row j (of `rows`, S floats apart) holds channels c0 .. c0 + cw - 1 of position u0 + j, zero outside [0, Lout)
template <int SRC>
__device__ __forceinline__ void wu_build_window(float* win, int S, int c0, int cw, long long n, long long u0, int rows,
                                                const WuConvArgs& a, int tid) {
    const int q4 = cw / 4;
    for (int idx = tid; idx < rows * q4; idx += 256) {
        const int j = idx / q4, cl = 4 * (idx - j * q4);
        const long long u = u0 + j;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (u >= 0 && u < a.Lout) v = wu_source<SRC>(a, n, u, c0 + cl);
        *reinterpret_cast<float4*>(win + j * S + cl) = v;
    }
}

// blockIdx.x = (waveform n, tile of TM positions), blockIdx.y = group of NTW N tiles.  LDS window row j holds position
// t0 - PAD + j; lane (i = l & 15, q = l >> 4) of wave w reads rows 16 w + i + tap, channels 16 b + 4 q .. + 3.
// C/D map of the MFMA: channel = lane & 15, position = 4 (lane >> 4) + r.
// ACT: bias + LeakyReLU (inference); without it bias (if any) and the raw sum (training: z, and the data gradients).
template <int TAPS, int SRC, int NTW, bool ACT>
__global__ __launch_bounds__(256) void wu_conv_kernel(const WuConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) float win[];
    constexpr int PAD = TAPS / 2, ROWS = TM + TAPS - 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, q = lane >> 4;
    const long long n = blockIdx.x / a.tiles, t0 = (long long)(blockIdx.x % a.tiles) * TM;
    const long long Lout = a.Lout;
    const int nt0 = blockIdx.y * NTW;
    const bool active = t0 + 16 * wave < Lout;          // a wave past the end of the waveform only takes part in the staging
    const float4* bq = a.frag + (long long)nt0 * a.groups * 64 + lane;
    f32x4 acc[NTW] = {};
    int g = 0;
    for (int c0 = 0; c0 < a.Cin; c0 += CHUNK) {
        const int cw = a.Cin - c0 < CHUNK ? a.Cin - c0 : CHUNK, S = cw + 4;
        if (c0) __syncthreads();
        wu_build_window<SRC>(win, S, c0, cw, n, t0 - PAD, ROWS, a, tid);
        __syncthreads();
        const int blocks = cw / 16;
        if (active) {
            const float* ap = win + (16 * wave + i) * S + 4 * q;
            for (int tap = 0; tap < TAPS; ++tap) {
                for (int b = 0; b < blocks; ++b, ++g) {
                    const float4 av = *reinterpret_cast<const float4*>(ap + tap * S + 16 * b);
                    float4 bv[NTW];
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt) bv[nt] = bq[((long long)nt * a.groups + g) * 64];
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt) acc[nt] = MFMA16(av.x, bv[nt].x, acc[nt]);
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt) acc[nt] = MFMA16(av.y, bv[nt].y, acc[nt]);
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt) acc[nt] = MFMA16(av.z, bv[nt].z, acc[nt]);
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt) acc[nt] = MFMA16(av.w, bv[nt].w, acc[nt]);
                }
            }
        }
    }
    if (!active) return;
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        const int ch = 16 * (nt0 + nt) + i;
        if (ch >= a.Cout) continue;
        float b = 0.f;
        if (ACT || a.bias) b = a.bias[ch];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long p = t0 + 16 * wave + 4 * q + r;
            if (p >= Lout) continue;
            if constexpr (ACT) a.out[(n * Lout + p) * a.Cout + ch] = leaky(acc[nt][r] + b);
            else a.out[(n * Lout + p) * a.Cout + ch] = a.bias ? acc[nt][r] + b : acc[nt][r];
        }
    }
}

// -------------------------------------------------------------------------------------------------------------- head
// Thread m = n L + t: bias, then the 16 decoder channels and x as one fma chain.  w: the 17 weights, b: the bias.
__global__ __launch_bounds__(256) void wu_head_kernel(const float* __restrict__ o, const float* __restrict__ x, long long M,
                                                      const float* __restrict__ w, const float* __restrict__ b,
                                                      float* __restrict__ y, float* __restrict__ logits) {
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    float acc = b[0];
#pragma unroll
    for (int c = 0; c < CI; c += 4) {
        const float4 v = *reinterpret_cast<const float4*>(o + m * CI + c);
        acc = fmaf(w[c], v.x, acc);
        acc = fmaf(w[c + 1], v.y, acc);
        acc = fmaf(w[c + 2], v.z, acc);
        acc = fmaf(w[c + 3], v.w, acc);
    }
    acc = fmaf(w[CI], x[m], acc);
    if (logits) logits[m] = acc;
    y[m] = tanhf(acc);
}

template <int TAPS, int SRC, bool ACT>
inline void wu_launch_conv(int ntw, dim3 grid, size_t lds, hipStream_t s, const WuConvArgs& a) {
    switch (ntw) {
        case 1: hipLaunchKernelGGL((wu_conv_kernel<TAPS, SRC, 1, ACT>), grid, dim3(256), lds, s, a); break;
        case 2: hipLaunchKernelGGL((wu_conv_kernel<TAPS, SRC, 2, ACT>), grid, dim3(256), lds, s, a); break;
        case 3: hipLaunchKernelGGL((wu_conv_kernel<TAPS, SRC, 3, ACT>), grid, dim3(256), lds, s, a); break;
        default: hipLaunchKernelGGL((wu_conv_kernel<TAPS, SRC, 4, ACT>), grid, dim3(256), lds, s, a); break;
    }
}

// grid, LDS bytes and the derived fields of `a` (Lout, Cin, Cu, Cout set by the caller) for N waveforms
inline void wu_conv_geometry(WuConvArgs& a, int taps, int64_t N, int ntw, int ntp, dim3& grid, size_t& lds) {
    a.tiles = (int)((a.Lout + TM - 1) / TM);
    a.groups = taps * a.Cin / 16;
    a.scale = a.Cu ? wu_scale(a.Lout / 2) : 0.f;
    grid = dim3((unsigned)(N * a.tiles), (unsigned)(ntp / ntw));
    const int cw = a.Cin < CHUNK ? a.Cin : CHUNK;
    lds = sizeof(float) * (size_t)(TM + taps - 1) * (cw + 4);
}

}  // namespace
