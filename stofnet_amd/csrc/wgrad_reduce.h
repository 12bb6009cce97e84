// The second half of every weight gradient that is summed without float atomics: the work-groups of the first kernel each wrote
// ONE partial of E floats (`copies`, `stride` floats apart), this kernel adds the `ncopies` partials of every element in an
// order that depends on ncopies alone, so two runs are bitwise equal.  The order is part of the results' bits:
//
//   a work-group takes 64 elements x 16 interleaved slices of the partials (slice sl: k = sl, sl + 16, ...); a slice runs four
//   chains while k + 48 < ncopies, the rest goes into chain 0, the chains fold as (a0 + a1) + (a2 + a3); the 16 slices then fold
//   through LDS, four at a time in order: s += (r[k] + r[k + 1]) + (r[k + 2] + r[k + 3]).
//
// Where the sum of element i goes is the caller's `Map`: used(i) (false: a slot that no partial holds) and store(i, value).
// (wgrad_reduce_kernel and sgb_wgrad_reduce_kernel of train.hip are a different scheme.)
//
// Also here, because it decides what a partial holds: how the rows (or tiles) of a reduction are cut into the chunks that one
// work-group each sums.  The rule fixes the order of every fixed-order sum behind it, so it is part of the results' bits: a
// kernel keeps the rule it was written with (tests/test_gpu_baseline_train_bits.py and test_gpu_train_ends_bits.py pin them).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "stof_hip_util.h"

namespace {

using stof::launched;

// n chunks of `per` units each, the last one possibly shorter
struct Chunks {
    long long per;
    int n;
};

// Balanced: as many chunks as `min_per` units each would make, `max_n` at the most, then the units spread evenly over them and
// `per` rounded up to a multiple of `multiple` (Zonzini: 2, an MFMA row pair never straddles two chunks; SincNet: 1).
inline Chunks balanced_chunks(int64_t units, int min_per, int max_n, int multiple) {
    int64_t c = (units + min_per - 1) / min_per;
    if (c > max_n) c = max_n;
    int64_t per = (units + c - 1) / c;
    per = (per + multiple - 1) / multiple * multiple;
    return {per, (int)((units + per - 1) / per)};
}

// Fill to the minimum (Wave-U-Net): every chunk holds `min_per` units until `max_n` chunks are not enough, then they grow.
inline Chunks fill_chunks(int64_t units, int min_per, int max_n) {
    int64_t per = (units + max_n - 1) / max_n;
    if (per < min_per) per = min_per;
    return {per, (int)((units + per - 1) / per)};
}

// elements 0 .. ndw - 1 are dw, the rest db
struct DwThenDb {
    float *dw, *db;
    int ndw;
    __device__ bool used(int) const { return true; }
    __device__ void store(int i, float v) const {
        if (i < ndw) dw[i] = v; else db[i - ndw] = v;
    }
};

// ten per channel: nine taps -> dw (ch, 9), slot 9 -> db (ch)
struct TapsThenBias {
    float *dw, *db;
    __device__ bool used(int) const { return true; }
    __device__ void store(int i, float v) const {
        const int ch = i / 10, d = i - ch * 10;
        if (d < 9) dw[ch * 9 + d] = v; else db[ch] = v;
    }
};

// ten per (f, c): nine taps -> dw (f, c, 9), slot 9 -> db (f) for c = 0; the bias slot of c > 0 is never written
struct TapsThenBiasPerInput {
    float *dw, *db;
    int Cin;
    __device__ bool used(int i) const {
        const int fc = i / 10;
        return i - fc * 10 < 9 || fc % Cin == 0;
    }
    __device__ void store(int i, float v) const {
        const int fc = i / 10, d = i - fc * 10;
        if (d < 9) dw[(size_t)fc * 9 + d] = v; else db[fc / Cin] = v;
    }
};

// a strided convolution's partial in the k order its kernels read: elements co * K + tap * cpad_in + ci -> dw (cout, cin, taps),
// then cout bias slots -> db; the slots of the pad channels ci >= cin are never stored
struct ConvTapsThenBias {
    float *dw, *db;
    int cout, cin, cpad_in, K, taps;
    __device__ bool used(int i) const { return i >= cout * K || (i % K) % cpad_in < cin; }
    __device__ void store(int i, float v) const {
        if (i >= cout * K) { db[i - cout * K] = v; return; }
        const int co = i / K, k = i - co * K, tap = k / cpad_in, ci = k - tap * cpad_in;
        dw[((size_t)co * cin + ci) * taps + tap] = v;
    }
};

// the gradient of a bank of `taps` taps per filter computed `stride` wide: elements filter * stride + tap -> G (filter, taps);
// the slots tap >= taps are never stored
struct BankTaps {
    float* G;
    int taps, stride;
    __device__ bool used(int i) const { return i % stride < taps; }
    __device__ void store(int i, float v) const { G[(size_t)(i / stride) * taps + i % stride] = v; }
};

template <class Map>
__global__ __launch_bounds__(1024) void partial_reduce_kernel(const float* __restrict__ copies, int ncopies, int stride, int E, Map map,
                                                              float out_scale) {
    __shared__ float red[16][64];
    const int e = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + e;
    const bool used = i < E && map.used(i);
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    if (used) {
        int k = sl;
        for (; k + 48 < ncopies; k += 64) {
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] += copies[(size_t)(k + 16 * j) * stride + i];
        }
        for (; k < ncopies; k += 16) a[0] += copies[(size_t)k * stride + i];
    }
    red[sl][e] = (a[0] + a[1]) + (a[2] + a[3]);
    __syncthreads();
    if (sl != 0 || !used) return;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; k += 4) s += (red[k][e] + red[k + 1][e]) + (red[k + 2][e] + red[k + 3][e]);
    map.store(i, s * out_scale);
}

// one work-group per 64 elements
template <class Map>
inline void partial_reduce(hipStream_t s, const float* copies, int ncopies, int stride, int E, Map map, float out_scale) {
    hipLaunchKernelGGL(partial_reduce_kernel<Map>, dim3((unsigned)((E + 63) / 64)), dim3(1024), 0, s, copies, ncopies, stride, E, map,
                       out_scale);
}

}  // namespace
