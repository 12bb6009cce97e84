// What the SincNet inference file (sincnet.hip) and its training file (sincnet_train.hip) share: the geometry, the packed
// blob's layout, the forward kernels and the chain rule of the sinc filter synthesis.
//
// Activations between layers are channel-last fp32 with GAP zero rows around every waveform (the "GAP layout"):
//   buffer row r = GAP + n (L + GAP) + t holds act[n][t][0 .. 128), rows GAP + n (L + GAP) - GAP .. - 1 are zero.
// The zero rows are the convolutions' padding, so the K span (tap, input channel) of output (n, t) is the contiguous
// run of rows t - P .. t + P of that layout, read straight into the A operand (as zz_conv_kernel in zonzini_net.h does).
//
//   sn_gaps_kernel    zeroes the GAP rows of both ping-pong buffers (the workspace is not assumed to be clean)
//   sn_sinc_kernel    layer 0: implicit GEMM on v_mfma_f32_32x32x2_f32, M = time, N = 128 filters, K = 1024 taps (tap
//                     1023 is zero).  A work-group owns 128 samples of one row and stages x[t0 - 511 .. t0 + 639] in LDS
//                     with zeros outside [0, L); the A operand is the sliding window over that image.
//   sn_conv_kernel    layers 1 and 2: conv + bias + BN + LeakyReLU as one implicit GEMM, M = (row, t) flattened over the
//                     batch, N = 128, K = tap x 128 + input channel.  Each wave owns 32 outputs x all 128 channels (four
//                     32 x 32 accumulators share every A fragment); below NARROW_M outputs a wave owns one 32-channel
//                     tile, so that small batches still fill the GPU (the same k order: results are bitwise the same).
//   sn_out_kernel     layer 3 (128 -> 1, k 7, 0.2 % of the work) on the vector pipe: one wave per 16 samples of a row,
//                     lane l owns channels 2l, 2l + 1, a fixed xor-butterfly sums the lanes.
//
// The epilogue is a template flag.  EPI_BN (inference): leaky(acc * s + t), the eval-mode BatchNorm affine of the blob;
// EPI_BIAS (training forward): the raw pre-BatchNorm acc + bias, `st` pointing at the bias (NULL: none); EPI_NONE (the data
// gradient, a "same" convolution of dz with the flipped image): acc.  The flag is a compile-time branch, so the inference
// instantiations keep their instructions and their bits.
//
// Every output element is one fixed-order chain (MFMA k order, fixed loops and butterfly, no atomics), so a row's
// result does not depend on its batch, its chunk or its position there.  NaN propagates as in torch (conv sums, BN,
// LeakyReLU are all NaN-preserving).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include "mfma32_frag.h"
#include "stof_common.h"

namespace {

using namespace stof_frag;

constexpr int C = 128;                 // filters of layers 0..2
constexpr int K0 = 1023;               // sinc taps
constexpr int K0P = 1024;              // packed taps (tap 1023 is zero)
constexpr int HALF0 = 511;             // (K0 - 1) / 2: padding of layer 0 on each side
constexpr int K1 = 11, K2 = 9, K3 = 7;
constexpr int GAP = 8;                 // zero rows between waveforms (>= the largest padding of layers 1..3, 5)
constexpr int TILE0 = 128;             // samples per work-group of sn_sinc_kernel (4 waves x 32)
constexpr int XS0 = TILE0 + K0P;       // LDS image of sn_sinc_kernel: x[t0 - 511 .. t0 + 640]
constexpr int OUT_T = 16;              // samples per wave of sn_out_kernel
constexpr int64_t NARROW_M = 128 * 1024;   // below N L = this, waves of the MFMA kernels own one N tile instead of four
constexpr int NUM_PARAMS = 24;         // see stof_sincnet_pack_weights in include/stofnet_amd.h
constexpr int EPI_BN = 0, EPI_BIAS = 1, EPI_NONE = 2;

// Packed blob (floats, every section starts on a 256-byte boundary):
//   frag0 [4 N tiles][K0P / 8][64 lanes][4]        the synthesised filter bank, k = tap
//   st0   [2][128]                                  s, t of BN 0
//   frag1 [4][K1 * 128 / 8][64][4], st1 [2][128]    k = tap * 128 + ci
//   frag2 [4][K2 * 128 / 8][64][4], st2 [2][128]
//   w3    [7][128] (w3[tap][ci]), st3 [2]           s, t of BN 3 (conv bias folded into t)
// A fragment lane l, element e of K group q holds W[32 tile + (l & 31)][k = 8 q + 4 (l >> 5) + e]; the A operand of lane
// l reads the activation at the same k with one float4.
struct Layout {
    int64_t frag0, st0, frag1, st1, frag2, st2, w3, st3, total;
};

inline Layout layout() {
    Layout o{};
    int64_t at = 0;
    o.frag0 = at; at = align_up(at + (int64_t)C * K0P);
    o.st0 = at; at = align_up(at + 2 * C);
    o.frag1 = at; at = align_up(at + (int64_t)C * K1 * C);
    o.st1 = at; at = align_up(at + 2 * C);
    o.frag2 = at; at = align_up(at + (int64_t)C * K2 * C);
    o.st2 = at; at = align_up(at + 2 * C);
    o.w3 = at; at = align_up(at + K3 * C);
    o.st3 = at; at = align_up(at + 2);
    o.total = at;
    return o;
}

inline int64_t buffer_floats(int64_t N, int64_t L) { return align_up((N * (L + GAP) + GAP) * C); }

inline bool desc_ok(const stof_sincnet_desc* d) {
    return d && std::isfinite(d->fs) && d->fs > 0.0 && std::isfinite(d->bn_eps) && d->bn_eps >= 0.0;
}

__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : 0.2f * v; }   // NaN: 0.2 * NaN = NaN

// ------------------------------------------------------------------------------------------------------------- gaps
__global__ __launch_bounds__(256) void sn_gaps_kernel(float* __restrict__ b0, float* __restrict__ b1, long long L,
                                                      long long total) {
    const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // (gap g, gap row, channel)
    if (o >= total) return;
    const long long g = o / (GAP * C), w = o % (GAP * C);
    const long long at = g * (L + GAP) * C + w;
    b0[at] = 0.f;
    b1[at] = 0.f;
}

// ---------------------------------------------------------------------------------------------------------- layer 0
// Work-group (row n, t-block; N tiles blockIdx.y NTW ..): wave w owns samples t0 + 32 w .. + 31 and NTW N tiles.  Lane (i = l & 31, h = l >> 5)
// element e of K group q is x[t - 511 + 8 q + 4 h + e] = xs[32 w + i + 8 q + 4 h + e].  The last group's k = 1023 entry
// (h = 1, e = 3) is set to 0 rather than multiplied by the zero tap, so that a NaN one sample past the receptive field
// stays out, as in the reference.
template <int NTW, int EPI>
__global__ __launch_bounds__(256) void sn_sinc_kernel(const float* __restrict__ x, long long L, long long tblocks,
                                                      const float4* __restrict__ frag, const float* __restrict__ st,
                                                      float* __restrict__ out) {
    __shared__ float xs[XS0];
    const long long n = blockIdx.x / tblocks, t0 = (long long)(blockIdx.x % tblocks) * TILE0;
    const float* xr = x + n * L;
    for (int j = threadIdx.x; j < XS0; j += 256) {
        const long long t = t0 - HALF0 + j;
        xs[j] = (t >= 0 && t < L) ? xr[t] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, h = lane >> 5;
    if (t0 + 32 * wave >= L) return;
    const float* a = xs + 32 * wave + i + 4 * h;
    constexpr int G = K0P / 8;
    const int nt0 = blockIdx.y * NTW;
    const float4* bq = frag + (long long)nt0 * G * 64 + lane;
    f32x16 acc[NTW] = {};
    for (int q = 0; q < G; ++q) {
        float4 av = make_float4(a[8 * q], a[8 * q + 1], a[8 * q + 2], a[8 * q + 3]);
        if (q == G - 1 && h) av.w = 0.f;
        float4 bv[NTW];
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) bv[nt] = bq[((long long)nt * G + q) * 64];
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) acc[nt] = MFMA32(av.x, bv[nt].x, acc[nt]);
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) acc[nt] = MFMA32(av.y, bv[nt].y, acc[nt]);
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) acc[nt] = MFMA32(av.z, bv[nt].z, acc[nt]);
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) acc[nt] = MFMA32(av.w, bv[nt].w, acc[nt]);
    }
    // C/D map: column (channel) = lane & 31, row (sample) = (r & 3) + 8 (r >> 2) + 4 h
    float* const orow = out + (GAP + n * (L + GAP)) * C;
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        const int c = 32 * (nt0 + nt) + i;
        float s = 0.f, b = 0.f;
        if constexpr (EPI == EPI_BN) {
            s = st[c];
            b = st[C + c];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long t = t0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * h;
            if constexpr (EPI == EPI_BN) {
                if (t < L) orow[t * C + c] = leaky(fmaf(acc[nt][r], s, b));
            } else {
                if (t < L) orow[t * C + c] = acc[nt][r];                    // the sinc layer has no bias
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------ layers 1, 2
// Wave (blockIdx.x, w) owns flattened outputs m0 .. m0 + 31 (m = n L + t) and N tiles blockIdx.y NTW .. + NTW - 1.  Lane (i, h) reads rows
// t - P .. t + P of its own waveform (the GAP rows supply the padding) at k = 8 q + 4 h .. + 3; the next group's
// operands are loaded before this group's 16 MFMAs.
template <int KT, int NTW, int EPI>
__global__ __launch_bounds__(256) void sn_conv_kernel(const float* __restrict__ in, unsigned M, unsigned L,
                                                      const float4* __restrict__ frag, const float* __restrict__ st,
                                                      float* __restrict__ out) {
    constexpr int P = (KT - 1) / 2, G = KT * C / 8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned m0 = ((unsigned)blockIdx.x * 4 + wave) * 32;
    if (m0 >= M) return;
    const int i = lane & 31, h = lane >> 5;
    unsigned m = m0 + i;
    if (m >= M) m = M - 1;                            // tail lanes compute a duplicate and store nothing
    const unsigned n = m / L, t = m - n * L;
    const float* a = in + ((long long)GAP + (long long)n * (L + GAP) + t - P) * C + 4 * h;
    const int nt0 = blockIdx.y * NTW;
    const float4* bq = frag + (long long)nt0 * G * 64 + lane;
    f32x16 acc[NTW] = {};
    mfma32_k_loop<NTW, G>(a, bq, acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned row = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row >= M) continue;
        const unsigned rn = row / L;
        float* const o = out + ((long long)GAP + (long long)rn * GAP + row) * C + 32 * nt0 + i;
        if constexpr (EPI == EPI_NONE) {                           // st is NULL here: no pointer is formed from it
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) o[32 * nt] = acc[nt][r];
        } else {
            const float* const sc = st + 32 * nt0 + i;
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
                if constexpr (EPI == EPI_BN) o[32 * nt] = leaky(fmaf(acc[nt][r], sc[32 * nt], sc[C + 32 * nt]));
                if constexpr (EPI == EPI_BIAS) o[32 * nt] = acc[nt][r] + sc[32 * nt];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- layer 3
// Wave w: row n, samples t0 .. t0 + 15.  Lane l keeps channels 2l, 2l + 1 of rows t0 - 3 .. t0 + 18 (rows past L + 2
// feed no stored output and are not read: they can lie past the buffer), then per sample the fma chain over (tap,
// channel pair) and the xor-butterfly over the lanes (every lane ends with the same sum).
template <int EPI>
__global__ __launch_bounds__(256) void sn_out_kernel(const float* __restrict__ in, long long N, long long L, long long tblocks,
                                                     const float* __restrict__ w3, const float* __restrict__ st3,
                                                     float* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= N * tblocks) return;
    const long long n = wid / tblocks, t0 = (wid % tblocks) * OUT_T;
    constexpr int R = OUT_T + K3 - 1;
    const float* base = in + (GAP + n * (L + GAP)) * C + 2 * lane;
    float2 v[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const long long t = t0 - 3 + j;                // >= -3: inside the leading GAP rows
        v[j] = t <= L + 2 ? *reinterpret_cast<const float2*>(base + t * C) : make_float2(0.f, 0.f);
    }
    float2 w[K3];
#pragma unroll
    for (int j = 0; j < K3; ++j) w[j] = *reinterpret_cast<const float2*>(w3 + j * C + 2 * lane);
    const float s = st3[0], b = EPI == EPI_BN ? st3[1] : 0.f;               // EPI_BIAS: st3[0] is the conv bias
#pragma unroll
    for (int u = 0; u < OUT_T; ++u) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < K3; ++j) {
            acc = fmaf(w[j].x, v[u + j].x, acc);
            acc = fmaf(w[j].y, v[u + j].y, acc);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if constexpr (EPI == EPI_BN) {
            if (lane == u && t0 + u < L) y[n * L + t0 + u] = fmaf(acc, s, b);
        } else {
            if (lane == u && t0 + u < L) y[n * L + t0 + u] = acc + s;
        }
    }
}

// ------------------------------------------------------------------------------------- the synthesis and its chain rule
// SincConv_fast.forward (models/sincnet.py:147-188, min_low_hz = min_band_hz = 50), in double:
//   low = 50 + |low_hz_|, high = clamp(low + 50 + |band_hz_|, 50, fs / 2), band = high - low
//   n_j = 2 pi (j - 511) / fs, j = 0 .. 510; window_j = 0.54 - 0.46 cos(2 pi u_j / 1023), u = linspace(0, 510.5, 511)
//   left_j = (sin(high n_j) - sin(low n_j)) / (n_j / 2) window_j, centre 2 band, right = mirror of left; all / (2 band)
struct SincBand {
    double low, high, band;
    bool inside;                      // the clamp passes its gradient (closed interval)
};

__host__ __device__ inline SincBand sinc_band(double fs, float low_hz, float band_hz) {
    SincBand b;
    b.low = 50.0 + fabs((double)low_hz);
    const double raw = b.low + 50.0 + fabs((double)band_hz);
    b.high = fmin(fmax(raw, 50.0), fs / 2.0);
    b.band = b.high - b.low;
    b.inside = raw >= 50.0 && raw <= fs / 2.0;
    return b;
}

// Taps j0, j0 + stride, ... < 511 of one filter: with f_j = (sin(high n_j) - sin(low n_j)) c_j / (2 band), c_j = window_j /
// (n_j / 2), and g_j = G[j] + G[1022 - j] (the mirrored right half shares the left half's value; the centre tap is the
// constant 1 and has no gradient), adds sum g_j df_j/dhigh to *dhigh and sum g_j df_j/dlow to *dlow.
__host__ __device__ inline void sinc_band_grad_taps(double fs, const SincBand& b, const float* G, int j0, int stride, double* dhigh,
                                                    double* dlow) {
    const double pi = 3.14159265358979323846;
    double dh = 0.0, dl = 0.0;
    for (int j = j0; j < HALF0; j += stride) {
        const double u = (double)j * (K0 / 2.0 - 1.0) / (HALF0 - 1);
        const double win = 0.54 - 0.46 * cos(2.0 * pi * u / K0);
        const double nn = 2.0 * pi * (double)(j - HALF0) / fs;
        const double cj = win / (nn / 2.0);
        const double g = (double)G[j] + (double)G[K0 - 1 - j];
        const double num = sin(b.high * nn) - sin(b.low * nn);
        const double q = num / (2.0 * b.band * b.band);
        dh += g * cj * (cos(b.high * nn) * nn / (2.0 * b.band) - q);
        dl += g * cj * (q - cos(b.low * nn) * nn / (2.0 * b.band));
    }
    *dhigh += dh;
    *dlow += dl;
}

// From the two sums to the parameters: high follows low where the clamp passes; abs gives the sign (0 at 0).
__host__ __device__ inline void sinc_band_grad_finish(const SincBand& b, float low_hz, float band_hz, double dhigh, double dlow,
                                                      double* dlow_hz, double* dband_hz) {
    const double draw = b.inside ? dhigh : 0.0;
    const double sl = low_hz > 0.f ? 1.0 : (low_hz < 0.f ? -1.0 : 0.0);
    const double sb = band_hz > 0.f ? 1.0 : (band_hz < 0.f ? -1.0 : 0.0);
    *dlow_hz = (dlow + draw) * sl;
    *dband_hz = draw * sb;
}

}  // namespace
