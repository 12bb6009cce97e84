// GradPeak on float64 envelopes (models/gradpeak.py:8-68) on gfx950.  The reference follows the input's dtype: a float64
// frame stays in double through the gradient, the Gaussian blur (gaussian_filter_1d casts the taps to data.dtype), the
// default threshold, the comparisons and the amplitudes it returns.  These kernels do the same after stof_hilbert_f64.
//
//   gradpeak_f64_rows_kernel<MOMENTS>  one wavefront per row, 64 samples per step: gradient (central differences / (2 g),
//                                      one-sided / g at both ends) -> zero padded correlation with the float64 taps (fma
//                                      chain in tap order) -> the flags (blur > th) and (blur < -th/4) as ballot words ->
//                                      hysteresis pairing (gradpeak_core.h, the same code as the fp32 kernels) -> echo
//                                      rows (onset, peak, env[peak]) in double.  MOMENTS: the pre-pass of the default
//                                      threshold (Q7) -- every work-group writes the sum and the sum of squares of its
//                                      smoothed gradients to its own slot
//   gradpeak_f64_fold_kernel           adds the slots to stats[0..1] in a fixed order (bitwise repeatable: no atomics)
//   gradpeak_f64_threshold_kernel      thres_pos = std**16 * 1.2e13 (:18) in double, on the device
// One host read per call at most (flags = {Q9, Kmax}), as on the fp32 path.
#include <hip/hip_runtime.h>
#include "stof_common.h"
#include "stof_hip_util.h"
#include "gradpeak_core.h"

namespace {

using stof_gp::Config;
using stof_gp::RowState;
constexpr int WAVES = 4;                          // rows in flight per work-group
// grid limit of the row kernel, and the number of slots of the moments pass: a constant (not a multiple of the CU count)
// so that the rows a work-group sums, and with them the rounding of the sums, do not depend on the device
constexpr int MAX_GROUPS = 2048;
constexpr int RING_MAX = 2 * stof_gp::ring_entries(stof_gp::MAXRAD);   // doubles of a wave's gradient ring

// (not inlined, as reduce_row: once per row)
// echo_max reduction of one row in double (models/gradpeak.py:107-114): the echo_max largest amplitudes (ties: the earlier
// echo), then ascending peak time, the reference's zero padding in front of a row with fewer echoes.  `src` holds the
// row's min(nout, cap) echoes written by this wave; they are re-read behind an L1-bypassing load.
__device__ __attribute__((noinline)) void reduce_row_f64(const double* src, long long cnt, long long k, double* __restrict__ dst,
                                                         int lane) {
    auto ld = [&](long long e, int f) {
        const unsigned long long bits = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(src) + 3 * e + f,
                                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return __longlong_as_double((long long)bits);
    };
    const long long npad = k > cnt ? k - cnt : 0;
    for (long long p = lane; p < npad; p += 64) { dst[3 * p] = 0.0; dst[3 * p + 1] = 0.0; dst[3 * p + 2] = 0.0; }
    if (cnt <= k) {
        for (long long e = lane; e < cnt; e += 64)
            for (int f = 0; f < 3; ++f) dst[3 * (npad + e) + f] = ld(e, f);
        return;
    }
    const int nt = (int)((cnt + 63) / 64);                     // cnt <= 4096 (checked by the host)
    unsigned long long taken = 0;                              // bit t: entry lane + 64 t is selected
    for (long long round = 0; round < k; ++round) {
        double best = -1.0;
        int best_e = 0x7fffffff;
        for (int t = 0; t < nt && t < 64; ++t) {
            const long long e = lane + 64ll * t;
            if (e < cnt && !((taken >> t) & 1ull)) {
                const double a = ld(e, 2);
                if (a > best) { best = a; best_e = (int)e; }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o);
            const int oe = __shfl_xor(best_e, o);
            if (ob > best || (ob == best && oe < best_e)) { best = ob; best_e = oe; }
        }
        if ((best_e & 63) == lane && best_e != 0x7fffffff) taken |= 1ull << (best_e >> 6);
    }
    long long pos = 0;
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int t = 0; t < nt && t < 64; ++t) {
        const bool sel = (taken >> t) & 1ull;
        const unsigned long long sm = __ballot(sel);
        if (sel) {
            const long long e = lane + 64ll * t, p = pos + __builtin_popcountll(sm & lt_mask);
            for (int f = 0; f < 3; ++f) dst[3 * p + f] = ld(e, f);
        }
        pos += __builtin_popcountll(sm);
    }
}

// Blurred gradient of the lane's sample from the ring: taps t[0 .. 2 R] against ring[s0 .. s0 + 2 R], fma chain in tap
// order.  The taps come from LDS as 16-byte broadcast reads; the last (odd) tap alone, so no read goes past the window.
template <int R>
__device__ __forceinline__ double blur_fixed(const double* __restrict__ tp, const double* __restrict__ w) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 2 * R; j += 2) {
        const double2 t = *reinterpret_cast<const double2*>(tp + j);
        s = fma(t.x, w[j], s);
        s = fma(t.y, w[j + 1], s);
    }
    return fma(tp[2 * R], w[2 * R], s);
}
__device__ __forceinline__ double blur_any(const double* __restrict__ tp, const double* __restrict__ w, int rad) {
    double s = 0.0;
    for (int j = 0; j < 2 * rad; j += 2) {
        const double2 t = *reinterpret_cast<const double2*>(tp + j);
        s = fma(t.x, w[j], s);
        s = fma(t.y, w[j + 1], s);
    }
    return fma(tp[2 * rad], w[2 * rad], s);
}

// Wave w of a work-group takes rows blockIdx * WAVES + w, + gridDim * WAVES, ...  Iteration c of a row: lane l forms the
// gradient of sample u = 64 c + l (the two envelope samples behind it were requested one iteration earlier), stores it
// twice into the wave's ring (slot and slot + RG: every blur read is `base + j`, no wrap), and blurs sample i = u - rad.
template <bool MOMENTS>
__global__ __launch_bounds__(64 * WAVES) void gradpeak_f64_rows_kernel(const double* __restrict__ env, long long N, Config cf,
                                                                     const double* __restrict__ taps, double th_pos,
                                                                     const double* __restrict__ th_dev,
                                                                     double* __restrict__ echoes, double* __restrict__ reduced,
                                                                     int* __restrict__ counts, int* __restrict__ flags,
                                                                     double* __restrict__ partials) {
    __shared__ __attribute__((aligned(16))) double tp[stof_gp::TAPS_LDS];
    __shared__ __attribute__((aligned(16))) double rings[WAVES][RING_MAX];
    __shared__ double red[2][WAVES];
    __shared__ int wmax[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = cf.L, rad = cf.radius, ntaps = 2 * rad + 1;
    for (int q = tid; q < stof_gp::TAPS_LDS; q += blockDim.x) tp[q] = q < ntaps ? taps[q] : 0.0;
    if (th_dev != nullptr) th_pos = *th_dev;                   // default threshold computed on the device (Q7)
    const double th_neg = -th_pos / 4.0;                       // models/gradpeak.py:19
    __syncthreads();
    double* const ring = rings[wave];
    const int RG = stof_gp::ring_entries(rad), rmask = RG - 1, nw = stof_gp::word_count(L, rad);
    const double sp = (double)cf.spacing, two_sp = 2.0 * sp;
    double mom[2] = {0.0, 0.0};
    int kmax = 0;
    for (long long row = (long long)blockIdx.x * WAVES + wave; row < N; row += (long long)gridDim.x * WAVES) {
        const double* const e = env + row * (long long)L;
        double* const out = MOMENTS ? nullptr : echoes + row * cf.cap * 3;
        RowState st;
        stof_fft::wave_lds_sync();                             // the previous row's reads are behind us
        for (int q = lane; q < 2 * RG; q += 64) ring[q] = 0.0; // = the blur's zero padding left of the row
        double ea, eb;
        auto fetch = [&](int u) {                              // clamped indices; the gradient masks u >= L
            const int uc = u < L ? u : L - 1;
            ea = e[uc + 1 < L ? uc + 1 : L - 1];               // u = 0: 1;  u = L-1: L-1;  else u+1
            eb = e[uc > 0 ? uc - 1 : 0];                       // u = 0: 0;  u = L-1: L-2;  else u-1
        };
        fetch(lane);
        for (int c = 0; c < nw; ++c) {
            const int u = 64 * c + lane;
            const double den = (u == 0 || u == L - 1) ? sp : two_sp;
            const double g = u < L ? (ea - eb) / den : 0.0;
            if (c + 1 < nw) fetch(u + 64);
            stof_fft::wave_lds_sync();
            ring[u & rmask] = g;
            ring[(u & rmask) + RG] = g;
            stof_fft::wave_lds_sync();
            const int i = u - rad;
            const bool in_row = (i >= 0) && (i < L);
            const double* const w = ring + ((u - 2 * rad) & rmask);      // gradients i - rad .. i + rad
            double sm;
            if (rad == 5) sm = blur_fixed<5>(tp, w);                      // rf 10
            else if (rad == 15) sm = blur_fixed<15>(tp, w);               // rf 20
            else if (rad == 2) sm = blur_fixed<2>(tp, w);                 // grad_peak_detect's default grad_step 2
            else sm = blur_any(tp, w, rad);
            if constexpr (MOMENTS) {
                if (in_row) { mom[0] += sm; mom[1] = fma(sm, sm, mom[1]); }
            } else {
                const unsigned long long V = __ballot(in_row && i < L - 1);        // an edge index is 0 .. L-2
                const unsigned long long P = __ballot(in_row && sm > th_pos);     // grad > thres_pos (:23)
                const unsigned long long M = __ballot(in_row && sm < th_neg);     // grad < thres_neg (:24)
                if (c > 0) {
                    const unsigned long long EP = ~st.P & ((st.P >> 1) | (P << 63)) & st.V;
                    const unsigned long long EM = ~st.M & ((st.M >> 1) | (M << 63)) & st.V;
                    stof_gp::pair_word(st, 64 * (c - 1) - rad, EP, EM, lane, cf, out, [&](int idx) { return e[idx]; });
                }
                st.P = P; st.M = M; st.V = V;
            }
        }
        if constexpr (!MOMENTS) {
            // zero padding up to `cap` (:66), counts, Q9 (:54-55), the optional reduction
            for (long long q = 3ll * (st.nout < cf.cap ? st.nout : cf.cap) + lane; q < 3 * cf.cap; q += 64) out[q] = 0.0;
            if (lane == 0) {
                counts[row] = st.nout;
                if (st.any_ap && st.any_am && st.nout == 0) atomicOr(&flags[0], 1);
            }
            if (reduced != nullptr && cf.echo_max > 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_s_waitcnt(0);                                // this wave's echo stores have reached L2
                const long long cnt = st.nout < cf.cap ? st.nout : cf.cap;
                reduce_row_f64(out, cnt, cf.echo_max, reduced + row * cf.echo_max * 3, lane);
            }
            kmax = st.nout > kmax ? st.nout : kmax;
        }
    }
    if constexpr (MOMENTS) {
        // fixed order: butterfly inside the wave, waves in order, one slot per work-group
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mom[0] += __shfl_xor(mom[0], o);
            mom[1] += __shfl_xor(mom[1], o);
        }
        if (lane == 0) { red[0][wave] = mom[0]; red[1][wave] = mom[1]; }
        __syncthreads();
        if (tid == 0) {
            double a = 0.0, b = 0.0;
            for (int w = 0; w < WAVES; ++w) { a += red[0][w]; b += red[1][w]; }
            partials[2 * blockIdx.x] = a;
            partials[2 * blockIdx.x + 1] = b;
        }
    } else {                                                   // Kmax of the batch: one atomic per work-group
        if (lane == 0) wmax[wave] = kmax;
        __syncthreads();
        if (tid == 0) {
            int m = 0;
            for (int w = 0; w < WAVES; ++w) m = wmax[w] > m ? wmax[w] : m;
            if (m > 0) atomicMax(&flags[1], m);
        }
    }
}

// stats[0..1] += the sums of the `groups` slots: lane l takes slots l, l + 64, ... in order, then a butterfly (one wave)
__global__ void gradpeak_f64_fold_kernel(const double* __restrict__ partials, int groups, double* __restrict__ stats) {
    const int lane = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int s = lane; s < groups; s += 64) { a += partials[2 * s]; b += partials[2 * s + 1]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
    if (lane == 0) { stats[0] += a; stats[1] += b; }
}

// thres_pos = (grad_data.std() ** 16) * 1.2e13 (models/gradpeak.py:18) for a float64 grad_data: unbiased std of all the
// smoothed gradients from stats = (sum, sum of squares, count), the power and the product in double
__global__ void gradpeak_f64_threshold_kernel(const double* __restrict__ stats, double* __restrict__ th_out) {
    const double s1 = stats[0], s2 = stats[1], cnt = stats[2];
    double var = (s2 - s1 * s1 / cnt) / (cnt > 1.0 ? cnt - 1.0 : 1.0);
    if (!(var > 0.0)) var = 0.0;
    double p = sqrt(var);
    p *= p; p *= p; p *= p; p *= p;                            // ** 16
    th_out[0] = p * 1.2e13;
}

bool bad_common(int64_t N, int64_t L, int32_t grad_step, int32_t radius, int64_t cap) {
    return N < 0 || L < 0 || radius < 0 || cap < 0 || grad_step <= 0;
}

Config make_config(int64_t L, int32_t grad_step, int32_t radius, int32_t ival_min, int32_t ival_max, int64_t cap, int64_t echo_max) {
    Config cf;
    cf.L = (int)L; cf.spacing = (float)grad_step; cf.radius = radius;
    cf.th_pos = 0.f; cf.th_neg = 0.f;                          // (the float64 thresholds travel as kernel arguments)
    // the gate ival_min < am - ap < ival_max is evaluated in 32-bit arithmetic on positions below 2^30
    cf.ival_min = ival_min < -(1 << 30) ? -(1 << 30) : ival_min;
    cf.ival_max = ival_max > (1 << 30) ? (1 << 30) : ival_max;
    cf.cap = cap; cf.echo_max = echo_max > 0 ? echo_max : 0;
    return cf;
}

int64_t groups_for(int64_t N) {
    const int64_t g = (N + WAVES - 1) / WAVES;
    return g < MAX_GROUPS ? g : MAX_GROUPS;
}

}  // namespace

extern "C" size_t stof_gradpeak_moments_f64_workspace_bytes(int64_t N) {
    return N <= 0 ? 0 : (size_t)groups_for(N) * 2 * sizeof(double);
}

extern "C" int stof_gradpeak_moments_f64(const double* env, int64_t N, int64_t L, int32_t grad_step, const double* taps,
                                         int32_t radius, double* stats, void* workspace, size_t workspace_bytes, void* stream) {
    if (!env || !taps || !stats || bad_common(N, L, grad_step, radius, 0)) return STOF_ERR_BAD_ARG;
    if (N == 0 || L == 0) return STOF_OK;
    if (!workspace || workspace_bytes < stof_gradpeak_moments_f64_workspace_bytes(N)) return STOF_ERR_WORKSPACE;
    if (L < 2 || radius > stof_gp::MAXRAD || L > 0x3fffffffLL || N > 0x7fffffffLL) return STOF_ERR_UNSUPPORTED;
    const Config cf = make_config(L, grad_step, radius, 0, 0, 0, 0);
    const int64_t grid = groups_for(N);
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* const partials = static_cast<double*>(workspace);
    hipLaunchKernelGGL(gradpeak_f64_rows_kernel<true>, dim3((unsigned)grid), dim3(64 * WAVES), 0, s, env, (long long)N, cf, taps,
                       0.0, nullptr, nullptr, nullptr, nullptr, nullptr, partials);
    if (hipGetLastError() != hipSuccess) return STOF_ERR_HIP;
    hipLaunchKernelGGL(gradpeak_f64_fold_kernel, dim3(1), dim3(64), 0, s, partials, (int)grid, stats);
    return hipGetLastError() == hipSuccess ? STOF_OK : STOF_ERR_HIP;
}

extern "C" int stof_gradpeak_threshold_f64(const double* stats, double* threshold_out, void* stream) {
    if (!stats || !threshold_out) return STOF_ERR_BAD_ARG;
    hipLaunchKernelGGL(gradpeak_f64_threshold_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), stats, threshold_out);
    return hipGetLastError() == hipSuccess ? STOF_OK : STOF_ERR_HIP;
}

extern "C" int stof_grad_peak_detect_f64(const double* env, int64_t N, int64_t L, int32_t grad_step, const double* taps,
                                         int32_t radius, double threshold, const double* threshold_dev, int32_t ival_min,
                                         int32_t ival_max, int64_t echo_max, double* echoes, int64_t cap, double* reduced,
                                         int32_t* counts, int32_t* flags, void* stream) {
    if (!env || !taps || !counts || !flags || (!echoes && cap > 0) || bad_common(N, L, grad_step, radius, cap))
        return STOF_ERR_BAD_ARG;
    if (echo_max > 0 && !reduced) return STOF_ERR_BAD_ARG;
    if (echo_max > 0 && cap > 4096) return STOF_ERR_UNSUPPORTED;      // reduce_row_f64 selects among <= 64 x 64 entries per row
    if (N == 0) return STOF_OK;
    if (L < 2 || radius > stof_gp::MAXRAD || L > 0x3fffffffLL || N > 0x7fffffffLL) return STOF_ERR_UNSUPPORTED;
    const Config cf = make_config(L, grad_step, radius, ival_min, ival_max, cap, echo_max);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(flags, 0, 2 * sizeof(int32_t), s) != hipSuccess) return STOF_ERR_HIP;
    hipLaunchKernelGGL(gradpeak_f64_rows_kernel<false>, dim3((unsigned)groups_for(N)), dim3(64 * WAVES), 0, s, env, (long long)N, cf,
                       taps, threshold, threshold_dev, echoes, reduced, counts, flags, nullptr);
    return hipGetLastError() == hipSuccess ? STOF_OK : STOF_ERR_HIP;
}
