// Training augmentation of the reference (utils/transforms.py: NormalizeVol -> CropChannelData -> AddNoise, as main.py:49,54,82
// chains them in front of every training sample) for a whole batch in ONE launch.
//
//   aug_kernel       one 256-thread work-group per row, two passes over the row, no LDS staging (rows of any length):
//                      pass 1  max|x| over the row (normalize), and over the crop window sum x^2 and "has a negative
//                              sample"; over all L samples of the padded row sum U and sum U^2.  Each thread keeps double
//                              accumulators over the Philox blocks b = tid, tid + 256, ... (4 samples each) in that order;
//                              the 256 partials are combined by a butterfly inside each wave and then over the 4 waves in
//                              wave order: a fixed tree, so a row's sums are bitwise the same in every run.
//                              sum y^2 = sum x^2 / max^2, sum n^2 = sum U^2 (n = U) or 4 sum U^2 - 4 sum U + L (n = 2U - 1):
//                              the generator runs once per pass.
//                      pass 2  re-reads the row (it sits in L2), regenerates U, y = x[s + j] / max (0 from the crop width
//                              on) + n * scale as one fma, float4 stores when the row of y is 16-byte aligned.
//   uniforms_kernel  writes the U of one generator stream, one thread per Philox block.
//
// Generator: Philox4x32-10 (Salmon et al., SC'11), key (seed lo, seed hi), counter (j >> 2, row, call,
// (rank << 1) | stream); word j & 3 -> U = (word >> 8) * 2^-24.  Stream 0 = noise, stream 1 = crop shift (word 0 of block 0).
// A draw is a pure function of (seed, rank, call, stream, row, j).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "stof_common.h"
#include "philox.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;

__device__ __forceinline__ float to_uniform(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-08f; }   // 2^-24

struct AugArgs {
    const float* x;
    const float* gt;
    const float* noise;         // optional [N, L] uniforms
    const int32_t* shift;       // optional [N]
    float* y;
    float* gt_out;
    int32_t* start;
    long long L, G, width;      // width = L when the crop is off
    double snr_lin;             // 10^(-snr_db / 10)
    uint32_t k0, k1, call, rank2;   // rank2 = rank << 1
    int normalize, crop, add_noise;
};

// max that keeps a NaN once it has seen one (numpy's abs().max() does)
__device__ __forceinline__ float nanmax(float m, float a) { return (a > m || a != a) ? a : m; }

// the four uniforms of Philox block b of `row` (samples 4 b .. 4 b + 3; entries from L on are unspecified)
__device__ __forceinline__ void block_uniforms(const AugArgs& a, long long row, long long b, const float* nrow, float u[4]) {
    if (nrow) {
#pragma unroll
        for (int k = 0; k < 4; ++k) u[k] = 4 * b + k < a.L ? nrow[4 * b + k] : 0.f;
    } else {
        const Philox p = philox4x32_10((uint32_t)b, (uint32_t)row, a.call, a.rank2, a.k0, a.k1);
#pragma unroll
        for (int k = 0; k < 4; ++k) u[k] = to_uniform(p.v[k]);
    }
}

__global__ __launch_bounds__(THREADS) void aug_kernel(const AugArgs a) {
    __shared__ double red[WAVES][4];
    __shared__ float redm[WAVES];
    __shared__ int redneg[WAVES];
    const long long row = blockIdx.x, L = a.L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* xrow = a.x + row * L;
    const float* nrow = a.noise ? a.noise + row * L : nullptr;
    float* yrow = a.y + row * L;

    // ---- the crop window [s, s + width) (CropChannelData.forward), the same scalar work in every thread
    long long s = 0;
    const long long width = a.width;
    if (a.crop) {
        float g = a.gt[row * a.G];
        if (g != g) g = 0.f;
        g = fminf(fmaxf(g, -1073741824.f), 1073741824.f);
        const long long ref = (long long)rintf(g);                       // round half to even, as Python's round
        long long st = ref - width / 2 > 0 ? ref - width / 2 : 0;
        long long en = ref + width / 2 < L ? ref + width / 2 : L;
        if (en == L) st = en - width;
        if (st == 0) en = width;
        const long long md = (ref - st < en - ref ? ref - st : en - ref) >> 1;     // max_dist // 2 (floor)
        const long long low = -(st < md ? st : md), high = L - en < md ? L - en : md;
        long long sh = 0;
        if (a.shift) {
            sh = a.shift[row];
        } else if (high > low) {                                         // the reference's randint raises on an empty range
            const Philox p = philox4x32_10(0u, (uint32_t)row, a.call, a.rank2 | 1u, a.k0, a.k1);
            sh = low + (long long)(((unsigned long long)(p.v[0] >> 8) * (unsigned long long)(high - low)) >> 24);
        }
        s = st + sh;
        s = s < 0 ? 0 : (s > L - width ? L - width : s);                 // a caller's shift cannot move the window out of the row
    }

    // ---- pass 1
    const long long nblocks = (L + 3) >> 2;
    float m = 0.f;
    double sxx = 0.0, su = 0.0, suu = 0.0;
    int neg = 0;
    const bool need_u = a.add_noise != 0;
    for (long long b = tid; b < nblocks; b += THREADS) {
        const long long j0 = 4 * b;
        if (a.normalize) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j0 + k < L) m = nanmax(m, fabsf(xrow[j0 + k]));
        }
        if (need_u) {
            float u[4];
            block_uniforms(a, row, b, nrow, u);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j0 + k < L) {
                    su += (double)u[k];
                    suu += (double)u[k] * (double)u[k];
                }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j0 + k < width) {
                    const float v = xrow[s + j0 + k];
                    sxx += (double)v * (double)v;
                    neg |= v < 0.f;
                }
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        m = nanmax(m, __shfl_xor(m, off));
        sxx += __shfl_xor(sxx, off);
        su += __shfl_xor(su, off);
        suu += __shfl_xor(suu, off);
        neg |= __shfl_xor(neg, off);
    }
    if (lane == 0) {
        red[wave][0] = sxx;
        red[wave][1] = su;
        red[wave][2] = suu;
        redm[wave] = m;
        redneg[wave] = neg;
    }
    __syncthreads();
    m = redm[0];
    sxx = red[0][0];
    su = red[0][1];
    suu = red[0][2];
    neg = redneg[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) {
        m = nanmax(m, redm[w]);
        sxx += red[w][0];
        su += red[w][1];
        suu += red[w][2];
        neg |= redneg[w];
    }

    float scale = 0.f;
    if (need_u) {
        const double syy = a.normalize ? sxx / ((double)m * (double)m) : sxx;
        const double snn = neg ? 4.0 * suu - 4.0 * su + (double)L : suu;
        scale = (float)sqrt(a.snr_lin * syy / snn);
    }

    // ---- pass 2
    const bool vec_y = (((uintptr_t)yrow) & 15) == 0;
    const bool vec_x = (((uintptr_t)(xrow + s)) & 15) == 0;
    for (long long b = tid; b < nblocks; b += THREADS) {
        const long long j0 = 4 * b;
        float v[4];
        if (vec_x && j0 + 4 <= width) {
            const float4 q = *reinterpret_cast<const float4*>(xrow + s + j0);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = j0 + k < width ? xrow[s + j0 + k] : 0.f;
        }
        if (a.normalize) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j0 + k < width) v[k] = v[k] / m;
        }
        if (need_u) {
            float u[4];
            block_uniforms(a, row, b, nrow, u);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = fmaf(neg ? 2.f * (u[k] - 0.5f) : u[k], scale, v[k]);
        }
        if (vec_y && j0 + 4 <= L) {
            *reinterpret_cast<float4*>(yrow + j0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j0 + k < L) yrow[j0 + k] = v[k];
        }
    }

    // ---- ground truth: every column moves with the window; column 0 is the reference's `gt -= start`
    if (tid == 0) a.start[row] = (int32_t)s;
    for (long long c = tid; c < a.G; c += THREADS) {
        const float g = a.gt[row * a.G + c];
        float o = g;
        if (a.crop) {
            o = g - (float)s;
            if (c > 0 && !(g > 0.f && o >= 0.f && o < (float)width)) o = 0.f;     // 0 = "no echo" (main.py:217)
        }
        a.gt_out[row * a.G + c] = o;
    }
}

__global__ __launch_bounds__(THREADS) void uniforms_kernel(float* __restrict__ out, long long N, long long L, uint32_t k0, uint32_t k1,
                                                           uint32_t call, uint32_t c3) {
    const long long nblocks = (L + 3) >> 2;
    const long long o = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (o >= N * nblocks) return;
    const long long row = o / nblocks, b = o - row * nblocks;
    const Philox p = philox4x32_10((uint32_t)b, (uint32_t)row, call, c3, k0, k1);
    float* dst = out + row * L + 4 * b;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (4 * b + k < L) dst[k] = to_uniform(p.v[k]);
}

bool crop_on(const stof_augment_desc* d) { return d->crop_ratio > 0.0 && d->crop_ratio < 1.0; }

}  // namespace

extern "C" int stof_augment(const stof_augment_desc* desc, const float* x, const float* gt, int64_t N, int64_t L, int64_t G,
                            const float* noise, const int32_t* shift, float* y, float* gt_out, int32_t* start, void* stream) {
    if (!desc || !x || !y || !start || N < 0 || L < 0 || G < 0) return STOF_ERR_BAD_ARG;
    if (y == x) return STOF_ERR_BAD_ARG;
    if (G > 0 && (!gt || !gt_out)) return STOF_ERR_BAD_ARG;
    if (desc->add_noise && !isfinite(desc->snr_db)) return STOF_ERR_BAD_ARG;
    if (desc->rank >= (1u << 31)) return STOF_ERR_BAD_ARG;
    const bool crop = crop_on(desc);
    if (crop && G == 0) return STOF_ERR_BAD_ARG;                         // the window is placed around gt[:, 0]
    if (L >= (1ll << 31) || N >= (1ll << 31)) return STOF_ERR_UNSUPPORTED;   // int32 start, 32-bit row / block counters
    long long width = L;
    if (crop) {
        width = (long long)nearbyint((double)L * desc->crop_ratio);      // Python's round(): half to even
        if (width & 1) return STOF_ERR_UNSUPPORTED;                      // the reference asserts on such a window
        if (width > L) width = L;
    }
    if (N == 0 || L == 0) return STOF_OK;
    AugArgs a{};
    a.x = x; a.gt = gt; a.noise = desc->add_noise ? noise : nullptr; a.shift = shift;
    a.y = y; a.gt_out = gt_out; a.start = start;
    a.L = L; a.G = G; a.width = width;
    a.snr_lin = desc->add_noise ? pow(10.0, -desc->snr_db / 10.0) : 0.0;
    a.k0 = (uint32_t)desc->seed; a.k1 = (uint32_t)(desc->seed >> 32);
    a.call = desc->call; a.rank2 = desc->rank << 1;
    a.normalize = desc->normalize != 0; a.crop = crop; a.add_noise = desc->add_noise != 0;
    hipLaunchKernelGGL(aug_kernel, dim3((unsigned)N), dim3(THREADS), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? STOF_OK : STOF_ERR_HIP;
}

extern "C" int stof_augment_uniforms(uint64_t seed, uint32_t rank, uint32_t call, int32_t stream_id, float* out, int64_t N, int64_t L,
                                     void* stream) {
    if (!out || N < 0 || L < 0 || (stream_id != 0 && stream_id != 1) || rank >= (1u << 31)) return STOF_ERR_BAD_ARG;
    if (L >= (1ll << 31) || N >= (1ll << 31)) return STOF_ERR_UNSUPPORTED;
    if (N == 0 || L == 0) return STOF_OK;
    const long long total = N * ((L + 3) >> 2), blocks = (total + THREADS - 1) / THREADS;
    if (blocks >= (1ll << 31)) return STOF_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(uniforms_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, static_cast<hipStream_t>(stream), out, (long long)N,
                       (long long)L, (uint32_t)seed, (uint32_t)(seed >> 32), call, (rank << 1) | (uint32_t)stream_id);
    return hipGetLastError() == hipSuccess ? STOF_OK : STOF_ERR_HIP;
}
