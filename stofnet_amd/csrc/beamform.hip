// Plane-wave delay-and-sum beamformer of the reference (utils/beamform.py: bf_das, bf_das_rx) for a batch of frames.
//
//   das_kernel    DAS_G = 8 neighbouring lanes per pixel, FB frames of the batch per thread.  Lane g of a pixel walks the
//                 elements k = g, g + 8, ... in ascending order, per angle; the delay, both masks, the weights and the
//                 phase of a (pixel, element, angle) are worked out ONCE in double (das_core.h) and reused for the FB
//                 frames, whose gathers are independent loads.  The eight lanes of a pixel read eight neighbouring
//                 columns of (mostly) one sample row: 64 contiguous bytes of complex64.  Elements outside the receive
//                 cone are skipped before any square root.
//                 Order of a frame's sum, fixed: per angle eight partial sums (k = g mod 8, ascending) in accumulators of
//                 the input's scalar type, combined as a butterfly (lanes g ^ 1, g ^ 2, g ^ 4); the angle sums are then
//                 added in ascending order, as the reference does.  No atomics, and nothing depends on F or FB: a frame's
//                 result is bitwise independent of the batch it sits in and of its place there.  The file is compiled
//                 with -ffp-contract=off (build.py): every instantiation performs the same roundings.
//                 Pixels come as a list (x, z, dtx per pixel): any order is correct; raster order (depth fastest) makes
//                 neighbouring pixels read neighbouring sample rows.
//   bmode_log_kernel / bmode_apply_kernel
//                 20 log10 |.| per pixel, the smallest and largest finite value of a frame as a fixed tree (lanes, waves,
//                 block partials in index order), then: non-finite pixels take the smallest finite value and the maximum
//                 is subtracted.  No host read.
//
// The host entries above the kernels run the same das_core.h text in plain loops (elements in ascending order into one
// accumulator); they compile without a HIP compiler (tests/cpu_harness/das_harness.cpp includes this file).
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <limits>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "stof_common.h"
#include "das_core.h"

namespace {

constexpr int DAS_THREADS = 256;
constexpr int DAS_G = 8;                                // lanes per pixel
constexpr int DAS_PIXELS = DAS_THREADS / DAS_G;         // pixels per work-group
constexpr long long BMODE_MAX_PARTIALS = 1024;

bool das_desc_ok(const stof_das_desc* d) { return d && d->dtype >= STOF_DAS_F32 && d->dtype <= STOF_DAS_C128; }
bool das_complex(int dtype) { return dtype == STOF_DAS_C64 || dtype == STOF_DAS_C128; }
das::Geom das_geom(const stof_das_desc* d) { return das::Geom{d->c, d->t0, d->fs, d->f0, d->fnumber}; }
// 64-bit products of the sizes an entry indexes with: every one has to stay below 2^62
bool das_sizes_ok(int64_t F, int64_t A, int64_t S, int64_t Ne, int64_t P) {
    if (F < 0 || A < 0 || S < 0 || Ne < 0 || P < 0) return false;
    const long double lim = 4.0e18L;
    return (long double)F * A * S * Ne * 2 < lim && (long double)F * A * P * 2 < lim && (long double)F * A * Ne < lim;
}
size_t das_out_bytes(const stof_das_desc* d, int64_t F, int64_t A, int64_t P) {
    const size_t scalar = d->dtype == STOF_DAS_F32 || d->dtype == STOF_DAS_C64 ? 4 : 8;
    return (size_t)F * (size_t)(d->compound ? 1 : A) * (size_t)P * (das_complex(d->dtype) ? 2 : 1) * scalar;
}
long long bmode_partials(long long n) {
    const long long nb = (n + 1023) / 1024;
    return nb < 1 ? 1 : (nb > BMODE_MAX_PARTIALS ? BMODE_MAX_PARTIALS : nb);
}

template <typename T, bool CPLX>
void das_host(const das::Geom& g, const T* sig, long long F, long long A, long long S, long long Ne, const double* x,
              const double* z, const double* dtx, long long P, const double* xe, const uint8_t* rot, int compound, T* out) {
    constexpr int C = CPLX ? 2 : 1;
    for (long long f = 0; f < F; ++f)
        for (long long p = 0; p < P; ++p) {
            T fr = 0, fi = 0;
            for (long long a = 0; a < A; ++a) {
                T ar = 0, ai = 0;
                const T* plane = sig + ((f * A + a) * S) * Ne * C;
                for (long long k = 0; k < Ne; ++k) {
                    das::Term<T> t;
                    if (!das::term<T>(g, x[p], z[p], xe[k], dtx[a * P + p], S, CPLX, t)) continue;
                    if (CPLX) {
                        T re, im;
                        das::interp_c<T>(t, plane + k * C, Ne, rot[(f * A + a) * Ne + k] != 0, re, im);
                        ar = ar + re;
                        ai = ai + im;
                    } else {
                        ar = ar + das::interp<T>(t, plane + k, Ne);
                    }
                }
                if (compound) {
                    fr = fr + ar;
                    fi = fi + ai;
                } else {
                    T* o = out + ((f * A + a) * P + p) * C;
                    o[0] = ar;
                    if (CPLX) o[C - 1] = ai;
                }
            }
            if (compound) {
                T* o = out + (f * P + p) * C;
                o[0] = fr;
                if (CPLX) o[C - 1] = fi;
            }
        }
}

}  // namespace

extern "C" int stof_das_tx_distance(const double* xe, int64_t Ne, const double* angles, int64_t A, const double* x, const double* z,
                                    int64_t P, double* dtx) {
    if (Ne < 1 || A < 0 || P < 0 || !xe || (A > 0 && !angles) || (A > 0 && P > 0 && (!x || !z || !dtx))) return STOF_ERR_BAD_ARG;
    const double W = xe[Ne - 1] - xe[0];
    for (int64_t a = 0; a < A; ++a) {
        const das::Source s = das::source(W, angles[a]);
        for (int64_t p = 0; p < P; ++p) dtx[a * P + p] = das::tx_distance(s, x[p], z[p]);
    }
    return STOF_OK;
}

extern "C" int stof_das_beamform_host(const stof_das_desc* desc, const void* sig, int64_t F, int64_t A, int64_t S, int64_t Ne,
                                      const double* x, const double* z, const double* dtx, int64_t P, const double* xe,
                                      const uint8_t* rotate, void* out) {
    if (!das_desc_ok(desc) || !das_sizes_ok(F, A, S, Ne, P)) return STOF_ERR_BAD_ARG;
    if (F == 0 || P == 0 || (desc->compound == 0 && A == 0)) return STOF_OK;
    if (!out) return STOF_ERR_BAD_ARG;
    if (A == 0 || Ne == 0) {               // no term: zeros
        memset(out, 0, das_out_bytes(desc, F, A, P));
        return STOF_OK;
    }
    if (!sig || !x || !z || !dtx || !xe || (das_complex(desc->dtype) && !rotate)) return STOF_ERR_BAD_ARG;
    const das::Geom g = das_geom(desc);
    switch (desc->dtype) {
        case STOF_DAS_F32: das_host<float, false>(g, (const float*)sig, F, A, S, Ne, x, z, dtx, P, xe, rotate, desc->compound, (float*)out); break;
        case STOF_DAS_F64: das_host<double, false>(g, (const double*)sig, F, A, S, Ne, x, z, dtx, P, xe, rotate, desc->compound, (double*)out); break;
        case STOF_DAS_C64: das_host<float, true>(g, (const float*)sig, F, A, S, Ne, x, z, dtx, P, xe, rotate, desc->compound, (float*)out); break;
        default: das_host<double, true>(g, (const double*)sig, F, A, S, Ne, x, z, dtx, P, xe, rotate, desc->compound, (double*)out); break;
    }
    return STOF_OK;
}

extern "C" size_t stof_das_workspace_bytes(int64_t F, int64_t n) {
    if (F <= 0 || n <= 0) return 0;
    return (size_t)F * (size_t)bmode_partials(n) * 2 * sizeof(double);
}

#if defined(__HIPCC__)

namespace {

struct DasArgs {
    const void* sig;
    const double *x, *z, *dtx, *xe;
    const uint8_t* rot;
    void* out;
    long long F, A, S, Ne, P;
    das::Geom g;
    int compound;
};

template <typename T, bool CPLX, int FB>
__global__ __launch_bounds__(DAS_THREADS) void das_kernel(const DasArgs a) {
    constexpr int C = CPLX ? 2 : 1;
    const long long p = (long long)blockIdx.x * DAS_PIXELS + threadIdx.x / DAS_G;
    const int g = threadIdx.x % DAS_G;
    if (p >= a.P) return;                   // (the eight lanes of a pixel leave together)
    const long long f0 = (long long)blockIdx.y * FB;
    const int nf = a.F - f0 < FB ? (int)(a.F - f0) : FB;
    const T* sig = static_cast<const T*>(a.sig);
    T* out = static_cast<T*>(a.out);
    const double x = a.x[p], z = a.z[p];
    const long long plane = a.S * a.Ne * C;
    T fr[FB], fi[FB];
#pragma unroll
    for (int j = 0; j < FB; ++j) fr[j] = fi[j] = 0;
    for (long long ang = 0; ang < a.A; ++ang) {
        T ar[FB], ai[FB];
#pragma unroll
        for (int j = 0; j < FB; ++j) ar[j] = ai[j] = 0;
        const double dtx = a.dtx[ang * a.P + p];
        for (long long k = g; k < a.Ne; k += DAS_G) {
            das::Term<T> t;
            if (!das::term<T>(a.g, x, z, a.xe[k], dtx, a.S, CPLX, t)) continue;
#pragma unroll
            for (int j = 0; j < FB; ++j) {
                if (j >= nf) break;
                const long long fa = (f0 + j) * a.A + ang;
                const T* col = sig + fa * plane + k * C;
                if (CPLX) {
                    T re, im;
                    das::interp_c<T>(t, col, a.Ne, a.rot[fa * a.Ne + k] != 0, re, im);
                    ar[j] = ar[j] + re;
                    ai[j] = ai[j] + im;
                } else {
                    ar[j] = ar[j] + das::interp<T>(t, col, a.Ne);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < FB; ++j) {
#pragma unroll
            for (int off = 1; off < DAS_G; off <<= 1) {     // a + b == b + a bit for bit: all eight lanes hold the same sum
                ar[j] = ar[j] + __shfl_xor(ar[j], off);
                if (CPLX) ai[j] = ai[j] + __shfl_xor(ai[j], off);
            }
        }
#pragma unroll
        for (int j = 0; j < FB; ++j) {
            if (j >= nf) break;
            if (a.compound) {
                fr[j] = fr[j] + ar[j];
                fi[j] = fi[j] + ai[j];
            } else if (g == 0) {
                T* o = out + (((f0 + j) * a.A + ang) * a.P + p) * C;
                o[0] = ar[j];
                if (CPLX) o[C - 1] = ai[j];
            }
        }
    }
    if (a.compound && g == 0) {
#pragma unroll
        for (int j = 0; j < FB; ++j) {
            if (j >= nf) break;
            T* o = out + ((f0 + j) * a.P + p) * C;
            o[0] = fr[j];
            if (CPLX) o[C - 1] = fi[j];
        }
    }
}

template <typename T>
__device__ __forceinline__ bool finite_t(T v) { return fabs(v) <= std::numeric_limits<T>::max(); }   // false for NaN
__device__ __forceinline__ float log_mag(float re, float im, bool cplx) { return 20.f * log10f(cplx ? hypotf(re, im) : fabsf(re)); }
__device__ __forceinline__ double log_mag(double re, double im, bool cplx) { return 20.0 * log10(cplx ? hypot(re, im) : fabs(re)); }

// (mn, mx) of the block in every thread: lanes by butterfly, the 4 waves in wave order
template <typename T>
__device__ __forceinline__ void block_minmax(T& mn, T& mx, T (*red)[2]) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        mn = fmin(mn, __shfl_xor(mn, off));
        mx = fmax(mx, __shfl_xor(mx, off));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[wave][0] = mn;
        red[wave][1] = mx;
    }
    __syncthreads();
    mn = red[0][0];
    mx = red[0][1];
#pragma unroll
    for (int w = 1; w < DAS_THREADS / 64; ++w) {
        mn = fmin(mn, red[w][0]);
        mx = fmax(mx, red[w][1]);
    }
}

// grid (nb, F): out = 20 log10 |img|, partial[f][b] = (min, max) over the finite values block b saw
template <typename T, bool CPLX>
__global__ __launch_bounds__(DAS_THREADS) void bmode_log_kernel(const T* __restrict__ img, T* __restrict__ out, T* __restrict__ partial,
                                                                long long n) {
    __shared__ T red[DAS_THREADS / 64][2];
    const long long f = blockIdx.y, nb = gridDim.x;
    const T* src = img + f * n * (CPLX ? 2 : 1);
    T* dst = out + f * n;
    T mn = std::numeric_limits<T>::infinity(), mx = -std::numeric_limits<T>::infinity();
    for (long long i = (long long)blockIdx.x * DAS_THREADS + threadIdx.x; i < n; i += nb * DAS_THREADS) {
        const T lg = CPLX ? log_mag(src[2 * i], src[2 * i + 1], true) : log_mag(src[i], (T)0, false);
        dst[i] = lg;
        if (finite_t(lg)) {
            mn = fmin(mn, lg);
            mx = fmax(mx, lg);
        }
    }
    block_minmax<T>(mn, mx, red);
    if (threadIdx.x == 0) {
        partial[(f * nb + blockIdx.x) * 2] = mn;
        partial[(f * nb + blockIdx.x) * 2 + 1] = mx;
    }
}

// grid (nb, F): every block folds the frame's nb partials in the same order, then rewrites its share of the frame
template <typename T>
__global__ __launch_bounds__(DAS_THREADS) void bmode_apply_kernel(T* __restrict__ out, const T* __restrict__ partial, long long n) {
    __shared__ T red[DAS_THREADS / 64][2];
    const long long f = blockIdx.y, nb = gridDim.x;
    T mn = std::numeric_limits<T>::infinity(), mx = -std::numeric_limits<T>::infinity();
    for (long long j = threadIdx.x; j < nb; j += DAS_THREADS) {
        mn = fmin(mn, partial[(f * nb + j) * 2]);
        mx = fmax(mx, partial[(f * nb + j) * 2 + 1]);
    }
    block_minmax<T>(mn, mx, red);
    const bool none = !finite_t(mn);        // no finite non-zero pixel in the frame: zeros
    T* dst = out + f * n;
    for (long long i = (long long)blockIdx.x * DAS_THREADS + threadIdx.x; i < n; i += nb * DAS_THREADS) {
        T v = dst[i];
        if (!finite_t(v)) v = mn;
        dst[i] = none ? (T)0 : v - mx;
    }
}

template <typename T, bool CPLX>
int das_launch(const DasArgs& a, hipStream_t stream) {
    constexpr int FBMAX = sizeof(T) == 4 ? 8 : 4;       // frames per thread: the geometry is worked out once for them
    const long long bx = (a.P + DAS_PIXELS - 1) / DAS_PIXELS;
    const int fb = a.F == 1 ? 1 : FBMAX;
    const long long by = (a.F + fb - 1) / fb;
    if (bx >= (1ll << 31) || by > 65535) return STOF_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)bx, (unsigned)by), block(DAS_THREADS);
    if (fb == 1)
        hipLaunchKernelGGL((das_kernel<T, CPLX, 1>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((das_kernel<T, CPLX, FBMAX>), grid, block, 0, stream, a);
    return hipGetLastError() == hipSuccess ? STOF_OK : STOF_ERR_HIP;
}

template <typename T, bool CPLX>
int bmode_launch(const void* img, int64_t F, int64_t n, void* out, void* ws, hipStream_t stream) {
    const dim3 grid((unsigned)bmode_partials(n), (unsigned)F), block(DAS_THREADS);
    hipLaunchKernelGGL((bmode_log_kernel<T, CPLX>), grid, block, 0, stream, (const T*)img, (T*)out, (T*)ws, (long long)n);
    hipLaunchKernelGGL((bmode_apply_kernel<T>), grid, block, 0, stream, (T*)out, (const T*)ws, (long long)n);
    return hipGetLastError() == hipSuccess ? STOF_OK : STOF_ERR_HIP;
}

}  // namespace

extern "C" int stof_das_beamform(const stof_das_desc* desc, const void* sig, int64_t F, int64_t A, int64_t S, int64_t Ne,
                                 const double* x, const double* z, const double* dtx, int64_t P, const double* xe,
                                 const uint8_t* rotate, void* out, void* stream) {
    if (!das_desc_ok(desc) || !das_sizes_ok(F, A, S, Ne, P)) return STOF_ERR_BAD_ARG;
    if (F == 0 || P == 0 || (desc->compound == 0 && A == 0)) return STOF_OK;
    if (!out) return STOF_ERR_BAD_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (A == 0 || Ne == 0)                 // no term: zeros
        return hipMemsetAsync(out, 0, das_out_bytes(desc, F, A, P), st) == hipSuccess ? STOF_OK : STOF_ERR_HIP;
    if (!sig || !x || !z || !dtx || !xe || (das_complex(desc->dtype) && !rotate)) return STOF_ERR_BAD_ARG;
    DasArgs a{};
    a.sig = sig; a.x = x; a.z = z; a.dtx = dtx; a.xe = xe; a.rot = rotate; a.out = out;
    a.F = F; a.A = A; a.S = S; a.Ne = Ne; a.P = P;
    a.g = das_geom(desc);
    a.compound = desc->compound != 0;
    switch (desc->dtype) {
        case STOF_DAS_F32: return das_launch<float, false>(a, st);
        case STOF_DAS_F64: return das_launch<double, false>(a, st);
        case STOF_DAS_C64: return das_launch<float, true>(a, st);
        default: return das_launch<double, true>(a, st);
    }
}

extern "C" int stof_das_bmode(int32_t dtype, const void* img, int64_t F, int64_t n, void* bmode, void* workspace,
                              size_t workspace_bytes, void* stream) {
    if (dtype < STOF_DAS_F32 || dtype > STOF_DAS_C128 || F < 0 || n < 0) return STOF_ERR_BAD_ARG;
    if (F == 0 || n == 0) return STOF_OK;
    if (!img || !bmode || !workspace) return STOF_ERR_BAD_ARG;
    if (F > 65535 || (long double)F * n * 2 >= 4.0e18L) return STOF_ERR_UNSUPPORTED;
    if (workspace_bytes < stof_das_workspace_bytes(F, n)) return STOF_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case STOF_DAS_F32: return bmode_launch<float, false>(img, F, n, bmode, workspace, st);
        case STOF_DAS_F64: return bmode_launch<double, false>(img, F, n, bmode, workspace, st);
        case STOF_DAS_C64: return bmode_launch<float, true>(img, F, n, bmode, workspace, st);
        default: return bmode_launch<double, true>(img, F, n, bmode, workspace, st);
    }
}
#endif  // __HIPCC__
