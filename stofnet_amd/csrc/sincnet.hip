// The SincNet baseline (models/sincnet.py of the reference: SincNet with the option dict of main.py:145-157) on gfx950,
// inference only, exact fp32.
//
//   x [N, 1, L] -> sinc band-pass conv 1 -> 128 (1023 taps, "same" zero padding 511/511) -> BN -> LeakyReLU(0.2)
//               -> Conv1d 128 -> 128 (k 11, pad 5/5) -> BN -> LeakyReLU(0.2)
//               -> Conv1d 128 -> 128 (k 9, pad 4/4)  -> BN -> LeakyReLU(0.2)
//               -> Conv1d 128 -> 1 (k 7, pad 3/3)    -> BN -> identity (LeakyReLU(1))        -> y [N, 1, L]
// BatchNorm runs in eval mode; each one (with the conv bias before it) is the per-channel affine acc * s + t that the
// packer precomputes in double.
//
// Activations between layers are channel-last fp32 with GAP zero rows around every waveform:
//   buffer row r = GAP + n (L + GAP) + t holds act[n][t][0 .. 128), rows GAP + n (L + GAP) - GAP .. - 1 are zero.
// The zero rows are the convolutions' padding, so the K span (tap, input channel) of output (n, t) is the contiguous
// run of rows t - P .. t + P of that layout, read straight into the A operand (as zz_conv_kernel in zonzini.hip does).
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
// Every output element is one fixed-order chain (MFMA k order, fixed loops and butterfly, no atomics), so a row's
// result does not depend on its batch, its chunk or its position there.  NaN propagates as in torch (conv sums, BN,
// LeakyReLU are all NaN-preserving).
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

Layout layout() {
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

int64_t buffer_floats(int64_t N, int64_t L) { return align_up((N * (L + GAP) + GAP) * C); }

bool desc_ok(const stof_sincnet_desc* d) {
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
template <int NTW>
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
        const float s = st[c], b = st[C + c];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long t = t0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (t < L) orow[t * C + c] = leaky(fmaf(acc[nt][r], s, b));
        }
    }
}

// ------------------------------------------------------------------------------------------------------ layers 1, 2
// Wave (blockIdx.x, w) owns flattened outputs m0 .. m0 + 31 (m = n L + t) and N tiles blockIdx.y NTW .. + NTW - 1.  Lane (i, h) reads rows
// t - P .. t + P of its own waveform (the GAP rows supply the padding) at k = 8 q + 4 h .. + 3; the next group's
// operands are loaded before this group's 16 MFMAs.
template <int KT, int NTW>
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
        const float* const sc = st + 32 * nt0 + i;
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) o[32 * nt] = leaky(fmaf(acc[nt][r], sc[32 * nt], sc[C + 32 * nt]));
    }
}

// ---------------------------------------------------------------------------------------------------------- layer 3
// Wave w: row n, samples t0 .. t0 + 15.  Lane l keeps channels 2l, 2l + 1 of rows t0 - 3 .. t0 + 18 (rows past L + 2
// feed no stored output and are not read: they can lie past the buffer), then per sample the fma chain over (tap,
// channel pair) and the xor-butterfly over the lanes (every lane ends with the same sum).
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
    const float s = st3[0], b = st3[1];
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
        if (lane == u && t0 + u < L) y[n * L + t0 + u] = fmaf(acc, s, b);
    }
}

// --------------------------------------------------------------------------------------------------------- packing
// The filter bank of SincConv_fast.forward (models/sincnet.py:147-188, min_low_hz = min_band_hz = 50), in double:
//   low = 50 + |low_hz_|, high = clamp(low + 50 + |band_hz_|, 50, fs / 2), band = high - low
//   n_j = 2 pi (j - 511) / fs, j = 0 .. 510; window_j = 0.54 - 0.46 cos(2 pi u_j / 1023), u = linspace(0, 510.5, 511)
//   left_j = (sin(high n_j) - sin(low n_j)) / (n_j / 2) window_j, centre 2 band, right = mirror of left; all / (2 band)
void sinc_bank(double fs, const float* low_hz, const float* band_hz, double* bank /* [C][K0] */) {
    const double pi = 3.14159265358979323846;
    double win[HALF0], nn[HALF0];
    for (int j = 0; j < HALF0; ++j) {
        const double u = (double)j * (K0 / 2.0 - 1.0) / (HALF0 - 1);
        win[j] = 0.54 - 0.46 * cos(2.0 * pi * u / K0);
        nn[j] = 2.0 * pi * (double)(j - HALF0) / fs;
    }
    for (int c = 0; c < C; ++c) {
        const double low = 50.0 + fabs((double)low_hz[c]);
        const double high = fmin(fmax(low + 50.0 + fabs((double)band_hz[c]), 50.0), fs / 2.0);
        const double band = high - low;
        double* f = bank + (int64_t)c * K0;
        for (int j = 0; j < HALF0; ++j) {
            const double v = (sin(high * nn[j]) - sin(low * nn[j])) / (nn[j] / 2.0) * win[j] / (2.0 * band);
            f[j] = v;
            f[K0 - 1 - j] = v;
        }
        f[HALF0] = 2.0 * band / (2.0 * band);
    }
}

// BN (eval) after a conv with bias `bias` (NULL: none): y = (acc + bias - mean) / sqrt(var + eps) * gamma + beta
void bn_affine(const float* const* bn, const float* bias, int c, double eps, float* s, float* t) {
    const double sc = (double)bn[0][c] / sqrt((double)bn[3][c] + eps);
    *s = (float)sc;
    *t = (float)(((bias ? (double)bias[c] : 0.0) - (double)bn[2][c]) * sc + (double)bn[1][c]);
}

}  // namespace

extern "C" size_t stof_sincnet_packed_bytes(const stof_sincnet_desc* desc) {
    if (!desc_ok(desc)) return 0;
    return (size_t)layout().total * sizeof(float);
}

extern "C" int stof_sincnet_filter_bank(const stof_sincnet_desc* desc, const float* low_hz, const float* band_hz, float* bank) {
    if (!desc_ok(desc) || !low_hz || !band_hz || !bank) return STOF_ERR_BAD_ARG;
    double* d = static_cast<double*>(malloc(sizeof(double) * C * K0));
    if (!d) return STOF_ERR_WORKSPACE;
    sinc_bank(desc->fs, low_hz, band_hz, d);
    for (int64_t i = 0; i < (int64_t)C * K0; ++i) bank[i] = (float)d[i];
    free(d);
    return STOF_OK;
}

extern "C" int stof_sincnet_pack_weights(const stof_sincnet_desc* desc, const float* const* params, void* out, size_t out_bytes) {
    if (!desc_ok(desc) || !params || !out) return STOF_ERR_BAD_ARG;
    for (int i = 0; i < NUM_PARAMS; ++i)
        if (!params[i]) return STOF_ERR_BAD_ARG;
    const Layout o = layout();
    if (out_bytes < (size_t)o.total * sizeof(float)) return STOF_ERR_WORKSPACE;
    float* const blob = static_cast<float*>(out);
    memset(blob, 0, (size_t)o.total * sizeof(float));
    // layer 0: bank [C][1][1023] -> k = tap, the last tap of the 1024 zero
    {
        float* bank = static_cast<float*>(malloc(sizeof(float) * C * K0));
        if (!bank) return STOF_ERR_WORKSPACE;
        stof_sincnet_filter_bank(desc, params[0], params[1], bank);
        pack_frag32(bank, C, 1, K0, 1, C / 32, K0P / 8, blob + o.frag0);
        free(bank);
    }
    // layers 1, 2: weight [C][C][K] -> k = tap * C + ci
    pack_frag32(params[2], C, C, K1, C, C / 32, K1 * C / 8, blob + o.frag1);
    pack_frag32(params[4], C, C, K2, C, C / 32, K2 * C / 8, blob + o.frag2);
    // layer 3: weight [1][C][7] -> w3[tap][ci]
    for (int ci = 0; ci < C; ++ci)
        for (int j = 0; j < K3; ++j) blob[o.w3 + j * C + ci] = params[6][ci * K3 + j];
    // BN affines: params 8 + 4 i .. 11 + 4 i = bn.i weight, bias, running_mean, running_var
    const int64_t st_at[3] = {o.st0, o.st1, o.st2};
    for (int l = 0; l < 3; ++l)
        for (int c = 0; c < C; ++c)
            bn_affine(params + 8 + 4 * l, l == 0 ? nullptr : params[3 + 2 * (l - 1)], c, desc->bn_eps, blob + st_at[l] + c,
                      blob + st_at[l] + C + c);
    bn_affine(params + 20, params[7], 0, desc->bn_eps, blob + o.st3, blob + o.st3 + 1);
    return STOF_OK;
}

extern "C" size_t stof_sincnet_workspace_bytes(const stof_sincnet_desc* desc, int64_t N, int64_t L) {
    if (!desc_ok(desc) || N <= 0 || L <= 0) return 0;
    return 2 * (size_t)buffer_floats(N, L) * sizeof(float);
}

extern "C" int stof_sincnet_forward(const stof_sincnet_desc* desc, const float* x, int64_t N, int64_t L, const void* packed,
                                    float* y, void* workspace, size_t workspace_bytes, void* stream) {
    if (!desc_ok(desc) || !x || !packed || !workspace || N <= 0 || L <= 0) return STOF_ERR_BAD_ARG;
    if (desc->stop_after < 0 || desc->stop_after > 3 || (!y && desc->stop_after == 0)) return STOF_ERR_BAD_ARG;
    if (N * L >= (1ll << 31) - 64 || N * (L + GAP) + GAP >= (1ll << 31) - 64) return STOF_ERR_UNSUPPORTED;   // 32-bit m
    const int64_t bf = buffer_floats(N, L);
    if (workspace_bytes < 2 * (size_t)bf * sizeof(float)) return STOF_ERR_WORKSPACE;
    const Layout o = layout();
    const float* const blob = static_cast<const float*>(packed);
    float* const buf[2] = {static_cast<float*>(workspace), static_cast<float*>(workspace) + bf};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int layers = desc->stop_after == 0 ? 4 : desc->stop_after;

    const int64_t gaps = (N + 1) * GAP * C;
    hipLaunchKernelGGL(sn_gaps_kernel, dim3((unsigned)((gaps + 255) / 256)), dim3(256), 0, s, buf[0], buf[1], (long long)L,
                       (long long)gaps);
    if (hipGetLastError() != hipSuccess) return STOF_ERR_HIP;
    // Small batches: one N tile per wave (4x the waves, each A fragment loaded 4x) so that the GPU fills up.
    const bool narrow = N * L < NARROW_M;
    const int64_t tb0 = (L + TILE0 - 1) / TILE0;
    const dim3 sgrid((unsigned)(N * tb0), narrow ? 4 : 1);
    if (narrow)
        hipLaunchKernelGGL(sn_sinc_kernel<1>, sgrid, dim3(256), 0, s, x, (long long)L, (long long)tb0,
                           reinterpret_cast<const float4*>(blob + o.frag0), blob + o.st0, buf[0]);
    else
        hipLaunchKernelGGL(sn_sinc_kernel<4>, sgrid, dim3(256), 0, s, x, (long long)L, (long long)tb0,
                           reinterpret_cast<const float4*>(blob + o.frag0), blob + o.st0, buf[0]);
    if (hipGetLastError() != hipSuccess) return STOF_ERR_HIP;
    if (layers == 1) return STOF_OK;
    const unsigned M = (unsigned)(N * L);
    const dim3 cgrid((unsigned)((M + 127) / 128), narrow ? 4 : 1);
    for (int l = 1; l <= 2; ++l) {
        const float* in = buf[(l - 1) & 1];
        const float4* fr = reinterpret_cast<const float4*>(blob + (l == 1 ? o.frag1 : o.frag2));
        const float* st = blob + (l == 1 ? o.st1 : o.st2);
        float* out = buf[l & 1];
        if (l == 1 && narrow) hipLaunchKernelGGL((sn_conv_kernel<K1, 1>), cgrid, dim3(256), 0, s, in, M, (unsigned)L, fr, st, out);
        if (l == 1 && !narrow) hipLaunchKernelGGL((sn_conv_kernel<K1, 4>), cgrid, dim3(256), 0, s, in, M, (unsigned)L, fr, st, out);
        if (l == 2 && narrow) hipLaunchKernelGGL((sn_conv_kernel<K2, 1>), cgrid, dim3(256), 0, s, in, M, (unsigned)L, fr, st, out);
        if (l == 2 && !narrow) hipLaunchKernelGGL((sn_conv_kernel<K2, 4>), cgrid, dim3(256), 0, s, in, M, (unsigned)L, fr, st, out);
        if (hipGetLastError() != hipSuccess) return STOF_ERR_HIP;
        if (layers == l + 1) return STOF_OK;
    }
    const int64_t tblocks = (L + OUT_T - 1) / OUT_T, waves = N * tblocks;
    hipLaunchKernelGGL(sn_out_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, buf[0], (long long)N, (long long)L,
                       (long long)tblocks, blob + o.w3, blob + o.st3, y);
    return hipGetLastError() == hipSuccess ? STOF_OK : STOF_ERR_HIP;
}
