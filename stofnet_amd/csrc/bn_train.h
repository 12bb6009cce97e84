// Train-mode BatchNorm of the baselines' training kernels (sincnet_train.hip, waveunet_train.hip), once: the batch statistics,
// a = act(z s + t), and the backward (dgamma, dbeta, dz).  Every sum is a double from the first addition and its order depends
// on the shape alone, so two runs are bitwise equal; tests/test_gpu_baseline_train_bits.py pins the bits of both networks.
//
//   chunk_sums              the rows are cut into chunks (the caller's chunk rule, wgrad_reduce.h), one work-group and one
//                           partial per chunk: thread (channel, row part) runs the two chains s += v, q += v w over its rows,
//                           the parts of a channel are folded through LDS.  The statistics (v = w = z) and the backward
//                           (v = g, w = xhat) are this one skeleton.  part [chunk][2][C] doubles.
//   bn_stats_final_kernel   the partials in ascending order -> stat [4][C] doubles (mean, rstd, s = gamma rstd, t = beta - mean s)
//                           and the new running statistics (momentum, unbiased variance) into temporaries
//   bn_apply_kernel         a = Act::out(fma(z, s, t)): the affine in double, rounded once.  t = beta - mean s carries mean s,
//                           which an fp32 z s + t would not cancel again where the batch variance is small (measured 2.7e-6 of
//                           max |a| at 2 rows of Gaussian z)
//   bn_bnb_final_kernel     the partials in ascending order -> dbeta = sum g, dgamma = sum g xhat, coef [2][C] = both / M
//   bn_dz_kernel            dz = scale (g - mean(g) - xhat mean(g xhat)), rounded once
//
// What a network brings:
//   View   where element (row m, channel c) lives: at(m, c), and split(e) of the flat element index e = m C + c.  `Rows` below
//          is the dense [rows][C] tensor of Wave-U-Net and (C = 1) SincNet's flat one-channel tensor; SincNet's GAP layout is
//          in sincnet_train.hip.
//   Act    the network's arithmetic around the shared one, and nothing else differs between the networks:
//            g(da, a)        the gradient behind the activation (reads_a = false: `a` is not read, and may be NULL)
//            seen(xhat)      xhat as the reductions, and therefore dz, see it
//            scale(...)      dz's factor gamma rstd
//            out(u)          the activation of the affine's double u, rounded to fp32
//          SincNet multiplies the LeakyReLU slope in fp32 and rounds xhat to fp32; Wave-U-Net keeps both in double.
//   Fold   how the row parts of a channel are added: FoldAscending (SincNet: 2 parts at 128 channels, 256 parts at 1 channel)
//          or FoldPairs (Wave-U-Net: 4 parts as (0 + 1) + (2 + 3)).  The fold is part of the bits: changing a network's fold, its
//          chunk rule or its Act changes its results and needs the bits fixture recorded again, on purpose.
//   V      channels per thread of the elementwise kernels: 4 where the view keeps 4 channels adjacent and aligned (C % 4 == 0),
//          1 for the flat tensor.
#pragma once
#include <hip/hip_runtime.h>
#include "stof_hip_util.h"
#include "wgrad_reduce.h"

namespace {

// dense [rows][C]
struct Rows {
    int C;
    __host__ __device__ int channels() const { return C; }
    __device__ long long at(long long m, int c) const { return m * C + c; }
    __device__ void split(long long e, long long& m, int& c) const { m = e / C; c = (int)(e - m * C); }
};

struct FoldAscending {
    template <int PARTS, int CC>
    __device__ static double fold(const double* r) {
        double s = r[0];
        for (int k = 1; k < PARTS; ++k) s += r[k * CC];
        return s;
    }
};
struct FoldPairs {
    template <int PARTS, int CC>
    __device__ static double fold(const double* r) {
        static_assert(PARTS == 4, "FoldPairs folds four parts");
        return (r[0] + r[CC]) + (r[2 * CC] + r[3 * CC]);
    }
};

// grid (chunk, ceil(C / CC)); thread (channel CC blockIdx.y + tid % CC, part = tid / CC) walks rows part, part + PARTS, ... of
// its chunk; row(m, c, v, w) gives the two doubles of one element.
template <int CC, class Fold, class Row>
__device__ __forceinline__ void chunk_sums(Row row, long long M, long long rows_per, int C, double* __restrict__ part) {
    constexpr int PARTS = 256 / CC;
    __shared__ double red[2][256];
    const int cl = threadIdx.x % CC, p = threadIdx.x / CC, c = CC * blockIdx.y + cl;
    const long long m_begin = blockIdx.x * rows_per, m_end = m_begin + rows_per < M ? m_begin + rows_per : M;
    double s = 0.0, q = 0.0;
    if (c < C)
        for (long long m = m_begin + p; m < m_end; m += PARTS) {
            double v, w;
            row(m, c, v, w);
            s += v;
            q += v * w;
        }
    red[0][threadIdx.x] = s;
    red[1][threadIdx.x] = q;
    __syncthreads();
    if (p != 0 || c >= C) return;
    part[((long long)blockIdx.x * 2 + 0) * C + c] = Fold::template fold<PARTS, CC>(&red[0][cl]);
    part[((long long)blockIdx.x * 2 + 1) * C + c] = Fold::template fold<PARTS, CC>(&red[1][cl]);
}

template <int CC, class Fold, class View>
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const float* __restrict__ z, long long M, long long rows_per, View view,
                                                               double* __restrict__ part) {
    chunk_sums<CC, Fold>([&](long long m, int c, double& v, double& w) { v = w = (double)z[view.at(m, c)]; }, M, rows_per, view.channels(),
                         part);
}

template <int CC, class Fold, class Act, class View>
__global__ __launch_bounds__(256) void bn_bnb_partial_kernel(const float* __restrict__ da, const float* __restrict__ a,
                                                             const float* __restrict__ z, const double* __restrict__ stat, long long M,
                                                             long long rows_per, View view, double* __restrict__ part) {
    const int C = view.channels();
    chunk_sums<CC, Fold>([&](long long m, int c, double& v, double& w) {
        const long long at = view.at(m, c);
        v = Act::g(da[at], Act::reads_a ? a[at] : 0.f);
        w = Act::seen(((double)z[at] - stat[c]) * stat[C + c]);
    }, M, rows_per, C, part);
}

__global__ __launch_bounds__(64) void bn_stats_final_kernel(const double* __restrict__ part, int copies, int C, long long M, double eps,
                                                            double momentum, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ run_mean,
                                                            const float* __restrict__ run_var, double* __restrict__ stat,
                                                            float* __restrict__ new_mean, float* __restrict__ new_var) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    double s = 0.0, q = 0.0;
    for (int k = 0; k < copies; ++k) {
        s += part[((long long)k * 2 + 0) * C + c];
        q += part[((long long)k * 2 + 1) * C + c];
    }
    const double m = (double)M, mean = s / m;
    double var = q / m - mean * mean;
    if (var < 0.0) var = 0.0;
    const double rstd = 1.0 / sqrt(var + eps), sc = (double)gamma[c] * rstd;
    stat[c] = mean;
    stat[C + c] = rstd;
    stat[2 * C + c] = sc;
    stat[3 * C + c] = (double)beta[c] - mean * sc;
    new_mean[c] = (float)((1.0 - momentum) * (double)run_mean[c] + momentum * mean);
    new_var[c] = (float)((1.0 - momentum) * (double)run_var[c] + momentum * (var * m / (m - 1.0)));
}

__global__ __launch_bounds__(64) void bn_bnb_final_kernel(const double* __restrict__ part, int copies, int C, long long M,
                                                          float* __restrict__ dgamma, float* __restrict__ dbeta, double* __restrict__ coef) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    double s = 0.0, q = 0.0;
    for (int k = 0; k < copies; ++k) {
        s += part[((long long)k * 2 + 0) * C + c];
        q += part[((long long)k * 2 + 1) * C + c];
    }
    dbeta[c] = (float)s;
    dgamma[c] = (float)q;
    coef[c] = s / (double)M;
    coef[C + c] = q / (double)M;
}

template <int V>
__device__ __forceinline__ void bn_load(const float* p, float (&v)[V]) {
    if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void bn_store(float* p, const float (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}

// thread: V channels of one row
template <int V, class Act, class View>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ z, long long threads, View view,
                                                       const double* __restrict__ stat, float* __restrict__ out) {
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= threads) return;
    const int C = view.channels();
    long long m;
    int c;
    view.split(o * V, m, c);
    const long long at = view.at(m, c);
    float in[V], res[V];
    bn_load<V>(z + at, in);
#pragma unroll
    for (int k = 0; k < V; ++k) res[k] = Act::out(fma((double)in[k], stat[2 * C + c + k], stat[3 * C + c + k]));
    bn_store<V>(out + at, res);
}

template <int V, class Act, class View>
__global__ __launch_bounds__(256) void bn_dz_kernel(const float* __restrict__ da, const float* __restrict__ a, const float* __restrict__ z,
                                                    const double* __restrict__ stat, const double* __restrict__ coef,
                                                    const float* __restrict__ gamma, long long threads, View view, float* __restrict__ dz) {
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= threads) return;
    const int C = view.channels();
    long long m;
    int c;
    view.split(o * V, m, c);
    const long long at = view.at(m, c);
    float d4[V], a4[V] = {}, z4[V], res[V];
    bn_load<V>(da + at, d4);
    if constexpr (Act::reads_a) bn_load<V>(a + at, a4);
    bn_load<V>(z + at, z4);
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const double g = Act::g(d4[k], a4[k]);
        const double xh = Act::seen(((double)z4[k] - stat[c + k]) * stat[C + c + k]);
        res[k] = (float)(Act::scale(gamma, stat, C, c + k) * (g - coef[c + k] - xh * coef[C + c + k]));
    }
    bn_store<V>(dz + at, res);
}

// ------------------------------------------------------------------------------------------------------------ host side
// ch: the network's chunks of the M rows; part holds ch.n partials of 2 C doubles
template <int CC, class Fold, class View>
int bn_stats_launch(hipStream_t s, const float* z, long long M, View view, Chunks ch, double eps, double momentum, const float* gamma,
                    const float* beta, const float* run_mean, const float* run_var, double* stat, float* new_mean, float* new_var,
                    double* part) {
    const int C = view.channels();
    hipLaunchKernelGGL((bn_stats_partial_kernel<CC, Fold, View>), dim3((unsigned)ch.n, (unsigned)((C + CC - 1) / CC)), dim3(256), 0, s, z, M,
                       ch.per, view, part);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    hipLaunchKernelGGL(bn_stats_final_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, s, part, ch.n, C, M, eps, momentum, gamma, beta,
                       run_mean, run_var, stat, new_mean, new_var);
    return launched();
}

// a may be NULL if Act::reads_a is false; gamma if Act::scale does not read it.  coef: 2 C doubles of workspace.
template <int V, int CC, class Fold, class Act, class View>
int bn_bnb_launch(hipStream_t s, const float* da, const float* a, const float* z, const double* stat, const float* gamma, long long M,
                  View view, Chunks ch, float* dgamma, float* dbeta, float* dz, double* part, double* coef) {
    const int C = view.channels();
    hipLaunchKernelGGL((bn_bnb_partial_kernel<CC, Fold, Act, View>), dim3((unsigned)ch.n, (unsigned)((C + CC - 1) / CC)), dim3(256), 0, s, da,
                       a, z, stat, M, ch.per, view, part);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    hipLaunchKernelGGL(bn_bnb_final_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, s, part, ch.n, C, M, dgamma, dbeta, coef);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    const long long threads = M * C / V;
    hipLaunchKernelGGL((bn_dz_kernel<V, Act, View>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, da, a, z, stat, coef, gamma,
                       threads, view, dz);
    return launched();
}

template <int V, class Act, class View>
int bn_apply_launch(hipStream_t s, const float* z, long long M, View view, const double* stat, float* out) {
    const long long threads = M * view.channels() / V;
    hipLaunchKernelGGL((bn_apply_kernel<V, Act, View>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, z, threads, view, stat, out);
    return launched();
}

}  // namespace
